"""A recording stand-in for CsiEngine with the surface sweep.py uses, and the characterisation of run_sweep built on it
(tests/test_sweep_plan_host.py, tools/record_sweep_plan.py).  The engine computes nothing.  It writes down, in order, every device
call, upload, download and synchronize of a run and hands back deterministic numbers for every download, so that the host side of
the sweep - means, errors / n_info, confidence intervals, both field orders, the table - runs on real values.

Device arrays are named by their first appearance in the event sequence plus their shape ('a7(4, 2, 8, 234)'), not by allocation
order: allocations (empty) and frees are no events and may move, launches, copies and syncs may not.  A host array is recorded as
dtype, shape and the SHA-256 of the float32 bytes the real engine would upload (to_device, *_set_basis convert to float32 planes);
hashing the fp64 bytes of an SVD basis instead would pin the LAPACK build, not the sweep."""
import contextlib
import hashlib
import io
import itertools
import json
import os

import numpy as np

N_DATA, SYM_LEN = 234, 320
LEVELS, N_TRAIN, N_TEST, SEED = (-5, 10), 8, 4, 3
NT, NR, RAYS = 8, 2, 20


def _values(key, n):
    """n float32 in [1, 5) from `key` (splitmix64 of a counter, 23 bits each): as int32 they are positive, a pair as float64 is finite."""
    seed = int.from_bytes(hashlib.sha256(key.encode()).digest()[:8], 'little')
    with np.errstate(over='ignore'):
        z = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (1.0 + (z >> np.uint64(41)).astype(np.float64) * (4.0 / 2 ** 23)).astype(np.float32)


def _host(a):
    a = np.asarray(a)
    planes = [a.real, a.imag] if np.iscomplexobj(a) else [a]
    h = hashlib.sha256()
    for p in planes:
        h.update(np.ascontiguousarray(p, np.float32).tobytes())
    return ['host', str(a.dtype), list(a.shape), h.hexdigest()[:16]]


class FakeArray:
    def __init__(self, engine, shape):
        self.engine, self.shape = engine, tuple(int(s) for s in shape)
        self.name, self.freed, self.last = None, False, None
        engine.arrays.append(self)

    def download(self):
        e = self.engine
        name = e._use(self)
        e.events.append(['download', name])
        return _values('%s@%s' % (name, self.last), int(np.prod(self.shape))).reshape(self.shape)

    def free(self):
        if self.freed:
            self.engine.double_free.append(self.name or 'unnamed%s' % (self.shape,))
        self.freed = True


class FakeEngine:
    FB_LAYOUT_W, FB_LAYOUT_CSI = 0, 1
    JSDM_PGP = 1

    def __init__(self, nt=NT, nr=NR, rays=RAYS):
        self.nt, self.nr = nt, nr
        self.pilot = np.ones((nt, nt))
        self.dictionary = np.ones((nt, rays), np.complex128)
        self.events, self.arrays, self.names = [], [], 0
        self.double_free, self.use_after_free, self.levels = [], [], []

    # ---- bookkeeping
    def _use(self, a, index=None):
        if a.name is None:
            a.name = 'a%d%s' % (self.names, a.shape)
            self.names += 1
        if a.freed:
            self.use_after_free.append(a.name)
        if index is not None:
            a.last = index
        return a.name

    def _arg(self, v, index):
        if isinstance(v, FakeArray):
            return self._use(v, index)
        if isinstance(v, (list, tuple)):
            return [self._arg(x, index) for x in v]
        if isinstance(v, np.ndarray):
            return _host(v)
        if v is None or isinstance(v, (bool, str)):
            return v
        if isinstance(v, (int, np.integer)):
            return int(v)
        if isinstance(v, (float, np.floating)):
            return float(v)
        raise TypeError('argument %r of a device call' % (v,))

    def _call(self, name, args, kwargs):
        index = len(self.events)
        self.events.append([name, [self._arg(v, index) for v in args], {k: self._arg(kwargs[k], index) for k in sorted(kwargs)}])

    def end_of_level(self):
        """What evaluate_level(keep=False) must leave behind: nothing.  Appends and returns the findings of the level."""
        found = dict(leaked=[a.name or 'unnamed%s' % (a.shape,) for a in self.arrays if not a.freed],
                     double_free=self.double_free, use_after_free=self.use_after_free)
        self.levels.append(found)
        self.arrays, self.double_free, self.use_after_free = [], [], []
        return found

    # ---- the surface of CsiEngine
    def empty(self, shape):
        return FakeArray(self, shape)

    def to_device(self, host):
        host = np.asarray(host)
        a = FakeArray(self, host.shape)
        self.events.append(['to_device', self._use(a, len(self.events)), _host(host)])
        return a

    def synchronize(self):
        self.events.append(['synchronize'])

    def link_frame_bits(self, ns, n_sym=10, bps=2):
        n_coded = int(ns) * int(n_sym) * N_DATA * int(bps)
        return n_coded // 3 - 6, n_coded

    def _synth(self, name, npkt, n_scat, want_channel, want_noise_std, want_tau, scalars):
        ltf, plane = (npkt, self.nr, SYM_LEN * self.nt), (npkt, self.nr, self.nt, N_DATA)
        out = [self.empty(ltf), self.empty(ltf)] + [self.empty(plane) if want_channel else None for _ in range(2)]
        out.append(self.empty((npkt,)) if want_noise_std else None)
        if n_scat is not None:
            out.append(self.empty((npkt, n_scat)) if want_tau else None)
        self._call(name, [], dict(scalars, out=out))
        return tuple(out)

    def synth_structured(self, seed, first_pkt, npkt, snr_db=None, n_taps=8, amp_scale=True, want_channel=True, want_noise_std=True):
        return self._synth('synth_structured', int(npkt), None, want_channel, want_noise_std, False,
                           dict(seed=seed, first_pkt=first_pkt, npkt=npkt, snr_db=snr_db, n_taps=n_taps, amp_scale=bool(amp_scale)))

    def synth_scattering(self, seed, first_pkt, npkt, snr_db=None, n_scat=100, range_m=100.0, az_deg=30.0, el_deg=0.0, box_frac=0.1,
                         random_users=False, amp_scale=True, want_channel=True, want_noise_std=True, want_tau=False, sample_rate_hz=100e6):
        return self._synth('synth_scattering', int(npkt), int(n_scat), want_channel, want_noise_std, want_tau,
                           dict(seed=seed, first_pkt=first_pkt, npkt=npkt, snr_db=snr_db, n_scat=n_scat, range_m=float(range_m), az_deg=float(az_deg),
                                el_deg=float(el_deg), box_frac=float(box_frac), random_users=bool(random_users), amp_scale=bool(amp_scale),
                                sample_rate_hz=float(sample_rate_hz)))

    def __getattr__(self, name):
        if name.endswith('_device') or name.endswith('_set_basis'):
            return lambda *args, **kwargs: self._call(name, args, kwargs)
        raise AttributeError(name)


def combinations():
    """{id: keyword arguments of run_sweep}: the full valid option matrix at ns = 1 and two all-on runs beside it."""
    ber1 = dict(ns=1, ntrf=1, n_sym=2, bps=2)
    fb1, jsdm1 = dict(b_phi=4, b_psi=2), dict(b=2, r_star=2)
    out = {}
    for chan, blind, dly, beams, ber in itertools.product((0, 1), repeat=5):
        base = dict(channel={} if chan else None, blind=bool(blind), delay_taps=6 if dly else None, delay_pre=1 if dly else 0, beams=bool(beams))
        tag = 'ch%d-bl%d-dl%d-bm%d' % (chan, blind, dly, beams)
        if not ber:
            out[tag + '-ber0'] = base
            continue
        for rx, fb, users in itertools.product((0, 1), (0, 1), (None, 2)):
            for muh, muj in itertools.product((0, 1), repeat=2) if users else [(0, 0)]:
                out[tag + '-ber1-rx%d-fb%d-u%d-muh%d-muj%d' % (rx, fb, users or 1, muh, muj)] = dict(
                    base, ber=dict(ber1), rx_estimate=bool(rx), feedback=dict(fb1) if fb else None, users=users,
                    mu_hybrid=3 if muh else None, mu_jsdm=dict(jsdm1) if muj else None)
    all_on = dict(channel={}, blind=True, delay_taps=6, delay_pre=1, beams=True, rx_estimate=True)
    out['all-on-rzf'] = dict(all_on, ber=dict(ber1), feedback=dict(fb1), users=2, mu_hybrid=3, mu_jsdm=dict(jsdm1), mu_reg='rzf')
    out['all-on-ns2'] = dict(all_on, ber=dict(ns=2, ntrf=2, n_sym=2, bps=4), feedback=dict(b_phi=0, b_psi=0, ng=2), users=3, mu_hybrid=7,
                             mu_jsdm=dict(b=2, r_star=1, mode='jgp'))
    return out


ALL_OFF, ALL_ON = 'ch0-bl0-dl0-bm0-ber0', 'ch1-bl1-dl1-bm1-ber1-rx1-fb1-u2-muh1-muj1'
FULL_RECORDS = (ALL_OFF, ALL_ON, 'all-on-ns2')      # the fixture keeps these whole, a digest of every other one


def record(sweep, kwargs, workdir):
    """One run_sweep of the module `sweep` on a fresh recording engine, with the models 'loaded' from nowhere.  Returns what the
    fixture pins: the events, sweep.json as text without its wall times, per level the fields of metrics.mat in file order with their
    values, the printed table, the key order of every per-packet dict, and per level what evaluate_level left unfreed or freed twice."""
    from scipy.io import loadmat
    engine = FakeEngine()
    evaluate, load = sweep.evaluate_level, sweep.load_models

    def evaluate_and_check(*a, **k):
        out = evaluate(*a, **k)
        engine.end_of_level()
        return out

    sweep.evaluate_level, sweep.load_models = evaluate_and_check, lambda engine, modeldir: None
    printed = io.StringIO()
    try:
        with contextlib.redirect_stdout(printed):
            res = sweep.run_sweep(engine, workdir, levels=LEVELS, n_train=N_TRAIN, n_test=N_TEST, seed=SEED, modeldir='unused', verbose=False, **kwargs)
    finally:
        sweep.evaluate_level, sweep.load_models = evaluate, load
    with open(os.path.join(workdir, 'sweep.json')) as f:
        saved = json.load(f)
    for d in [saved] + saved['levels']:
        for k in ('seconds', 'dataset_seconds'):
            d.pop(k, None)
    metrics = []
    for snr in LEVELS:
        mat = loadmat(os.path.join(workdir, 'BS%d_SNR%g' % (engine.nt, snr), 'metrics.mat'))
        metrics.append([[k, v.tolist()] for k, v in mat.items() if not k.startswith('__')])
    return dict(events=engine.events, sweep_json=json.dumps(saved, indent=1), metrics=metrics, table=printed.getvalue(),
                per_packet_keys=[list(res['per_packet'][float(snr)]) for snr in LEVELS], clean=engine.levels)


def digest(rec):
    return hashlib.sha256(json.dumps(rec, sort_keys=True).encode()).hexdigest()
