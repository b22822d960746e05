"""GPU tests of channel aging (csi_scatter_channel_at_device, csrc/scatter_aged.hip.h) against its fp64 statement
tests/scatter_aging_ref.py: the planes at several times, bit identity with csi_synth_scattering at t = 0 and at speed 0, slice /
range / repeat identity, the one-scatterer known answer, the memory contract, the refusals, a captured call and a miniature sweep.

Error bound of a slice: B = 2^-23 (1 + pi (Nt / 2 + Nr / 2 + tau_max + 1)) relative per row - the bound of tests/test_gpu_scatter.py
with one more phase term: the turn count nu_s t is reduced in fp64 and rounded once to fp32 in [-1/2, 1/2], half an ulp of half a turn =
pi / 2 2^-23 of phase; the + 1 is twice that.  Largest measured ratios to B are kept in profiles/scatter_aging.txt."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import rel_rows

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scatter_aging_ref as ar      # noqa: E402
from guarded import Guarded      # noqa: E402

TOL_NMSE = 1e-6          # tests/test_gpu_eval_kernels.py, the metric
T1 = [0.0]
T3 = [-2e-3, 0.0, 5e-3]
T16 = [0.1, -5e-3, -2e-3, -1e-3, -2.5e-4, 0.0, 1e-4, 2.5e-4, 5e-4, 1e-3, 2e-3, 4e-3, 8e-3, 2e-2, 5e-2, -0.1]      # any sign, any order


def _planes(c):
    return np.concatenate([np.asarray(c).real, np.asarray(c).imag], -1)


def _dl(re, im):
    return re.download().astype(np.float64) + 1j * im.download().astype(np.float64)


def _bound(nt, nr, tau_max):
    return 2.0 ** -23 * (1.0 + np.pi * (nt / 2.0 + nr / 2.0 + tau_max + 1.0))


def _engine(pkg, nt, nr, **kw):
    return pkg.CsiEngine(nt, nr, hidden=(8,), **kw)      # no pilot matrix: no LTF is made


# (Nt, Nr, S, npkt, first_pkt, amp_scale, random_users, random_heading, times, speed): every shape of the issue; both amplitude
# settings, fixed and random users, fixed and random heading spread over them; at 30 m/s the times of +-0.1 s reach 280 turns
CASES = [(4, 1, 1, 2, 0, True, False, False, T1, 1.0), (4, 2, 3, 3, 7, False, True, True, T3, 1.5), (4, 2, 3, 3, 7, True, False, False, T16, 30.0),
         (8, 4, 37, 2, 0, True, True, False, T16, 30.0), (32, 4, 100, 2, 7, False, False, True, T16, 30.0),
         (32, 4, 256, 1, 0, True, True, True, T3, 10.0), (128, 16, 100, 1, 7, False, False, False, T3, 3.0)]


@pytest.mark.parametrize('nt,nr,S,npkt,first,amp,rnd,rndh,times,speed', CASES)
def test_a_planes_against_the_replay(pkg, oracle, nt, nr, S, npkt, first, amp, rnd, rndh, times, speed):
    seed = 700 + nt + S
    e = _engine(pkg, nt, nr)
    kw = dict(speed_mps=speed, heading_az_deg=-65.0, heading_el_deg=12.0, random_heading=rndh, n_scat=S, range_m=100.0 if nt < 32 else 1000.0,
              random_users=rnd, amp_scale=amp)
    ref = ar.replay(seed, first, npkt, nr, oracle.hadamard(nt), times, **kw)
    h_re, h_im = e.scatter_channel_at(seed, first, npkt, times, **kw)
    e.synchronize()
    got = _dl(h_re, h_im)
    assert got.shape == (len(times), npkt, nr, nt, 234)
    tau_max = float(ref['tau_excess'].max())
    B = _bound(nt, nr, tau_max)
    turns = float(np.abs(ref['nu']).max() * np.abs(times).max())
    if times is T16:
        assert turns > 100.0, turns
    errs = [rel_rows(_planes(got[k]), _planes(ref['h'][k])) for k in range(len(times))]
    print(f'nt {nt} nr {nr} S {S} amp {amp} random users {rnd} heading {rndh} first {first}, {len(times)} times at {speed:g} m/s: tau_max {tau_max:.2f}, '
          f'largest |nu t| {turns:.1f} turns, worst slice {max(errs):.3e} = {max(errs) / B:.3f} B (B {B:.3e})')
    assert max(errs) < B, (errs, B)


SHAPES_B = [(4, 2, 3), (8, 2, 37), (32, 4, 100), (128, 16, 100)]


@pytest.mark.parametrize('nt,nr,S', SHAPES_B)
def test_b_identity_with_the_parent_and_with_itself(pkg, oracle, nt, nr, S):
    e = _engine(pkg, nt, nr)
    e.set_pilot(oracle.hadamard(nt))                     # for the parent's call only
    npkt, seed, first = (1 if nt == 128 else 2), 77, 5
    motion = dict(speed_mps=2.5, heading_az_deg=100.0, heading_el_deg=-20.0)
    for amp in (True, False):
        for rnd in (False, True):
            ch = dict(n_scat=S, random_users=rnd, amp_scale=amp)
            parent = [a.download() for a in e.synth_scattering(seed, first, npkt, **ch)[2:4]]
            three = [a.download() for a in e.scatter_channel_at(seed, first, npkt, T3, random_heading=rnd, **motion, **ch)]
            static = [a.download() for a in e.scatter_channel_at(seed, first, npkt, T3, speed_mps=0.0, heading_az_deg=100.0, random_heading=not rnd, **ch)]
            for p, a, s in zip(parent, three, static):
                assert np.array_equal(a[1], p), (amp, rnd, 'the t = 0 slice is not the parent\'s h')
                assert all(np.array_equal(s[k], p) for k in range(3)), (amp, rnd, 'a static user\'s slice is not the parent\'s h')
                assert not np.array_equal(a[0], p) and not np.array_equal(a[2], p)      # a nonzero time at a nonzero speed
    ch = dict(n_scat=S, **motion)
    many = [a.download() for a in e.scatter_channel_at(seed, first, 4, T3, **ch)]
    again = [a.download() for a in e.scatter_channel_at(seed, first, 4, T3, **ch)]
    one = [a.download() for a in e.scatter_channel_at(seed, first, 4, T3[2], **ch)]
    lo = [a.download() for a in e.scatter_channel_at(seed, first, 2, T3, **ch)]
    hi = [a.download() for a in e.scatter_channel_at(seed, first + 2, 2, T3, **ch)]
    other = [a.download() for a in e.scatter_channel_at(seed + 1, first, 4, T3, **ch)]
    for m, a, o, l, h, x in zip(many, again, one, lo, hi, other):
        assert np.array_equal(m, a)                                                   # a repeated call repeats
        assert o.shape[0] == 1 and np.array_equal(m[2], o[0])                       # the slice of a multi-time call = the one-time call
        assert np.array_equal(m[:, :2], l) and np.array_equal(m[:, 2:], h)           # packets [5, 9) = [5, 7) + [7, 9)
        assert not np.array_equal(m, x)                                               # another seed differs


def test_c_one_scatterer_on_the_device(pkg, oracle):
    nt, nr, npkt, seed, first, t = 8, 2, 2, 17, 2, 3e-3
    e = _engine(pkg, nt, nr)
    kw = dict(speed_mps=4.0, heading_az_deg=25.0, heading_el_deg=5.0, n_scat=1)
    ref = ar.replay(seed, first, npkt, nr, oracle.hadamard(nt), [0.0, t], **kw)
    got = _dl(*e.scatter_channel_at(seed, first, npkt, [0.0, t], **kw))
    B = _bound(nt, nr, 0.0)
    for p in range(npkt):
        ratio = got[1, p] / got[0, p]
        want = np.exp(2j * np.pi * ref['nu'][p, 0] * t)
        spread, mod = np.abs(ratio - ratio.mean()).max(), np.abs(np.abs(ratio) - 1.0).max()
        print(f'packet {p}: nu {ref["nu"][p, 0]:.3f} Hz, ratio spread {spread:.3e}, modulus error {mod:.3e}, against the replay {np.abs(ratio - want).max():.3e} (B {B:.3e})')
        assert spread < B and mod < B and np.abs(ratio - want).max() < B
        assert abs(ref['nu'][p, 0] * t) > 0.05                                        # a phase that can be told from none


@pytest.mark.parametrize('n_times', [1, 16])
def test_d_memory_contract(pkg, n_times):
    nt, nr, npkt, S = 8, 2, 3, 37
    e = _engine(pkg, nt, nr)
    times = T16[:n_times]
    out = [Guarded(e, (n_times, npkt, nr, nt, 234), 'out', name=n) for n in ('h_re', 'h_im')]
    kw = dict(speed_mps=2.0, heading_az_deg=10.0, n_scat=S)
    e.scatter_channel_at_device(3, 4, 0, times, out[0], out[1], **kw)                  # npkt = 0: nothing is written
    e.synchronize()
    for g in out:
        g.check()
        assert g.count_unwritten() == g.n
    e.scatter_channel_at_device(3, 4, npkt, times, out[0], out[1], **kw)
    e.synchronize()
    want = [a.download() for a in e.scatter_channel_at(3, 4, npkt, times, **kw)]
    for g, w in zip(out, want):
        g.check()                                                                      # written nowhere else
        assert g.count_unwritten() == 0                                                # and completely
        assert np.array_equal(g.download(), w)
        g.free()


def test_e_refusals_carry_text_and_leave_the_outputs_alone(pkg, oracle):
    from dl_channel_estimation_mamimo_amd._lib import CsiMotionConfig, CsiScatterConfig
    nt, nr = 4, 2
    e = _engine(pkg, nt, nr)
    lib, ctx = e._lib, e._ctx
    out = [Guarded(e, (2, 2, nr, nt, 234), 'out', name=n) for n in ('h_re', 'h_im')]
    nan, inf = float('nan'), float('inf')

    def call(cfg=None, motion=None, times=(0.0, 1e-3), n_times=None, seed=1, first=0, npkt=2, re=out[0].ptr, im=out[1].ptr):
        t = (ctypes.c_double * max(1, len(times)))(*times) if times is not None else None
        return lib.csi_scatter_channel_at_device(ctx, seed, first, npkt, ctypes.byref(CsiScatterConfig(**cfg)) if cfg is not None else None,
                                                 ctypes.byref(CsiMotionConfig(**motion)) if motion is not None else None, t,
                                                 len(times) if n_times is None else n_times, re, im)

    def refused(text, **kw):
        assert call(**kw) == -1, (text, kw)
        assert text in lib.csi_last_error(ctx).decode(), (text, lib.csi_last_error(ctx))

    refused('n_times 0 outside 1 .. 16', n_times=0)
    refused('n_times 17 outside 1 .. 16', times=[0.0] * 17)
    refused('null t_s', times=None, n_times=2)
    refused('t_s[1]', times=(0.0, nan))
    refused('t_s[0]', times=(-inf, 0.0))
    refused('speed_mps', motion=dict(speed_mps=-1.0))
    refused('speed_mps', motion=dict(speed_mps=inf))
    refused('heading_az_deg', motion=dict(heading_az_deg=nan))
    refused('heading_el_deg', motion=dict(heading_el_deg=90.5))
    refused('heading_el_deg', motion=dict(heading_el_deg=nan))
    refused('carrier_hz', motion=dict(carrier_hz=-1.0))
    refused('carrier_hz', motion=dict(carrier_hz=inf))
    refused('unknown motion flag bits', motion=dict(flags=2))
    refused('d_h_re', re=None)
    refused('d_h_im', im=None)
    refused('16-byte', re=out[0].ptr + 4)
    refused('exceed one launch', npkt=2 ** 31 // nr + 1)
    # what the parent refuses about the range and the configuration, under this entry point's name
    refused('csi_scatter_channel_at_device: npkt -1', npkt=-1)
    refused('must not be negative', first=-2)
    refused('n_scat 257 outside 1 .. 256', cfg=dict(n_scat=257))
    refused('range_m', cfg=dict(range_m=-1.0))
    refused('box_frac', cfg=dict(box_frac=nan))
    refused('sample_rate_hz', cfg=dict(sample_rate_hz=inf))
    refused('az_deg', cfg=dict(az_deg=inf))
    refused('el_deg', cfg=dict(el_deg=-91.0))
    refused('unknown flag bits', cfg=dict(flags=4))
    t = (ctypes.c_double * 1)(0.0)
    assert lib.csi_scatter_channel_at_device(None, 1, 0, 1, None, None, t, 1, out[0].ptr, out[1].ptr) == -1      # a null context
    e.synchronize()
    for g in out:
        g.check()
        assert g.count_unwritten() == g.n
    # the context stays usable; NULL records are the defaults and a static user; npkt = 0 needs no planes
    assert call() == 0 and call(npkt=0, re=None, im=None) == 0
    e.synchronize()
    e.set_pilot(oracle.hadamard(nt))                     # the parent needs one
    parent = [a.download() for a in e.synth_scattering(1, 0, 2, amp_scale=False)[2:4]]
    for g, p in zip(out, parent):
        assert np.array_equal(g.download()[0], p) and np.array_equal(g.download()[1], p)
        g.free()
    assert 'scatter_aged' in e.profile()


def test_f_a_captured_call_and_the_counters(pkg):
    nt, nr, npkt, S = 8, 2, 3, 37
    e = _engine(pkg, nt, nr)
    kw = dict(speed_mps=2.0, heading_az_deg=-30.0, n_scat=S)
    n_aged, n_parent = e.get_option('scatter_aged_launches'), e.get_option('scatter_launches')
    eager = [a.download() for a in e.scatter_channel_at(9, 1, npkt, T3, **kw)]
    cap = [e.empty((3, npkt, nr, nt, 234)) for _ in range(2)]
    for a in cap:
        a.upload(np.zeros(a.shape, np.float32))
    e.synchronize()
    e.capture_begin()
    try:
        e.scatter_channel_at_device(9, 1, npkt, T3, cap[0], cap[1], **kw)
    finally:
        g = e.capture_end()
    e.synchronize()
    assert not cap[0].download().any(), 'a recorded call must not run'
    g.launch()
    e.synchronize()
    g.free()
    for a, b in zip(eager, cap):
        assert np.array_equal(a, b.download())
    assert e.get_option('scatter_aged_launches') == n_aged + 2 and e.get_option('scatter_launches') == n_parent
    e.scatter_channel_at(9, 1, npkt, T16, speed_mps=0.0, n_scat=S)                     # one kernel whatever the times and the user
    assert e.get_option('scatter_aged_launches') == n_aged + 3 and e.get_option('scatter_launches') == n_parent


def test_g_miniature_sweep_with_aging(pkg, oracle, tmp_path):
    """Nt = 8, Nr = 2, one level, two users: with a static user every aged field equals its un-aged twin exactly; with a real speed and
    delay MSEA_perfect is the NMSE of the two downloaded truths and the perfect source no longer reports the un-aged dtSNR."""
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    nt, nr, n_train, n_test, snr = 8, 2, 24, 6, 10.0
    common = ['--nTX', str(nt), '--nRX', str(nr), '--nn', '16', '--trainPkts', str(n_train), '--testPkts', str(n_test), '--snr', '10', '--quiet',
              '--channel', 'scattering', '--scatterers', '37', '--ber', '--numSTS', '1', '--users', '2', '--rays', '64', '--dataSymbols', '2']
    still, moving = (str(tmp_path / d) for d in ('still', 'moving'))
    assert sweep.main(['-d', still, '--epochs', '2', '--bs', '32', '--aging', '2', '--speed', '0'] + common) == 0
    m = loadmat(os.path.join(still, 'BS8_SNR10', 'metrics.mat'))
    for x in ('LS', 'MMSE', 'DNN'):
        assert np.array_equal(m['MSEA_' + x], m['MSE_' + x]), x
    assert not m['MSEA_perfect'].any()
    for x in sweep.SOURCES:
        for aged, twin in (('bersA_', 'bers_'), ('EVM_rmsA_', 'EVM_rms_'), ('dtSNRA_', 'dtSNR_'), ('bersMUA_', 'bersMU_'),
                           ('EVM_rmsMUA_', 'EVM_rmsMU_'), ('sinrMUA_', 'sinrMU_')):
            assert np.array_equal(m[aged + x], m[twin + x]), (aged, x)
    assert sweep.main(['-d', moving, '--modeldir', still, '--aging', '2', '--speed', '1.5', '--heading', '70'] + common) == 0
    m = loadmat(os.path.join(moving, 'BS8_SNR10', 'metrics.mat'))
    new = [k for k in m if any(k.startswith(f) for f in sweep.MSEA_FIELDS + sweep.LINKA_FIELDS + sweep.MUA_FIELDS)]
    assert len(new) == 4 + 3 * 4 + 3 * 4
    for k in new:
        assert m[k].shape == (1, n_test) and np.isfinite(m[k]).all(), k
    assert (m['MSEA_perfect'] > 0).all()
    e = pkg.CsiEngine(nt, nr, hidden=(16,))
    e.set_pilot(oracle.hadamard(nt))
    h0 = _dl(*e.synth_scattering(1, n_train, n_test, snr_db=snr, n_scat=37)[2:4])
    hT = _dl(*e.scatter_channel_at(1, n_train, n_test, 2e-3, speed_mps=1.5, heading_az_deg=70.0, n_scat=37))[0]
    want = np.array([oracle.nmse_subk(hT[p], h0[p]) for p in range(n_test)])
    err = np.abs(m['MSEA_perfect'][0] / want - 1.0).max()
    print(f'MSEA_perfect {m["MSEA_perfect"][0].mean():.4e} against the NMSE of the two downloaded truths: relative difference {err:.3e}; '
          f'dtSNR_perfect {m["dtSNR_perfect"][0].mean():.3f} dB, dtSNRA_perfect {m["dtSNRA_perfect"][0].mean():.3f} dB; '
          f'sinrMU_perfect {m["sinrMU_perfect"][0].mean():.2f} dB, sinrMUA_perfect {m["sinrMUA_perfect"][0].mean():.2f} dB')
    assert err < TOL_NMSE
    assert not np.array_equal(m['dtSNRA_perfect'], m['dtSNR_perfect'])
