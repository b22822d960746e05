"""GPU tests of the link simulation (csi_link_sim_device / csi_viterbi_decode_device, csrc/link_sim.hip.h) against
the host restatement tests/link_ref.py.

The decoder is compared bit for bit where fp32 sums are exact (LLRs on a 2^-6 grid: only the tie rule decides) and through the fp64
path metric of its codeword where they are not.  The transmit / receive pass is compared with fp64 for x and csi (bound: the
normal-equations form loses cond(G)^2 of the fp32 budget), and every later stage is REPLAYED in fp64 from the device's own x and csi,
so that a soft bit near zero or a nearest-point decision is judged on the value the device actually had.

Figures recorded on an MI355X (also in profiles/link_sim.txt): (d) float32 host decoder shortfall 0 and device shortfall 0 at 0 dB -
the device repeats the host decoder's choices; (e) largest error / bound 0.151 over the five shapes (cond(G) up to 4.5e3)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import link_ref as L      # noqa: E402

# (Nt, Nr, ns, ntrf, bps, n_sym, npkt)
SHAPES = [(8, 4, 1, 1, 2, 2, 3), (8, 4, 2, 2, 2, 2, 3), (8, 2, 2, 3, 4, 1, 3), (16, 4, 3, 5, 2, 1, 2), (32, 4, 4, 4, 4, 1, 2)]
SEED, FIRST = 21, 4
_cache = {}


def _c(re, im):
    return re.download().astype(np.float64) + 1j * im.download().astype(np.float64)


def _c64(a):
    """what the library receives: fp32 planes, as complex128"""
    a = np.asarray(a)
    return a.real.astype(np.float32).astype(np.float64) + 1j * a.imag.astype(np.float32).astype(np.float64)


def _engine(pkg, oracle, nt, nr, **kw):
    e = pkg.CsiEngine(nt, nr, hidden=(8,), device=0, **kw)
    e.set_pilot(oracle.hadamard(nt))
    return e


def _inputs(e, shape, seed=SEED, first=FIRST, snr_db=12.0):
    """true channel of csi_synth_structured, random fbb, unit-modulus frf_mean, noise `snr_db` below the mean |G d|^2 per rx antenna"""
    nt, nr, ns, ntrf, bps, n_sym, npkt = shape
    rng = np.random.default_rng(nt * 100 + ns * 10 + ntrf)
    arr = e.synth_structured(seed, first, npkt, snr_db=None)
    e.synchronize()
    h = _c(arr[2], arr[3])
    for a in arr:
        if a is not None:
            a.free()
    fbb = _c64(rng.standard_normal((npkt, L.N, ns, ntrf)) + 1j * rng.standard_normal((npkt, L.N, ns, ntrf)))
    frf = _c64(np.exp(2j * np.pi * rng.random((npkt, ntrf, nt))))
    nv = np.empty(npkt, np.float32)
    for p in range(npkt):
        G = L.effective_channel(h[p], L.precoder(frf[p], fbb[p]))
        nv[p] = (np.abs(G) ** 2).sum((1, 2)).mean() / nr * 10.0 ** (-snr_db / 10.0)
    return h, fbb, frf, nv


def _run(pkg, oracle, shape):
    """one device call and the fp64 model per shape, shared by the tests that read them"""
    if shape not in _cache:
        nt, nr, ns, ntrf, bps, n_sym, npkt = shape
        e = _engine(pkg, oracle, nt, nr)
        h, fbb, frf, nv = _inputs(e, shape)
        dev = e.link_sim(h, fbb, frf, nv, seed=SEED, first_pkt=FIRST, n_sym=n_sym, bps=bps, details=True)
        ref = [L.simulate(SEED, FIRST + p, h[p], frf[p], fbb[p], float(nv[p]), n_sym, bps) for p in range(npkt)]
        _cache[shape] = (e, h, fbb, frf, nv, dev, ref)
    return _cache[shape]


# ------------------------------------------------------------------------------------------------ the decoder alone
@pytest.fixture(scope='module')
def dec_engine(pkg, oracle):
    return _engine(pkg, oracle, 4, 2)


def _quantised(rng, ncw, n_steps):
    """LLRs on the 2^-6 grid in [-8, 8]: odd codewords pure noise (many ties), even ones a noisy frame"""
    q = rng.integers(-512, 513, (ncw, 3 * n_steps)).astype(np.float64)
    bits = rng.integers(0, 2, (ncw, n_steps - 6)).astype(np.uint8)
    frame = np.clip(np.rint(64.0 * (2.0 * (1.0 - 2.0 * L.encode(bits)) + 2.0 * rng.standard_normal((ncw, 3 * n_steps)))), -512, 512)
    q[::2] = frame[::2]
    return (q / 64.0).astype(np.float32)


@pytest.mark.parametrize('ncw', [1, 3, 130])
@pytest.mark.parametrize('n_steps', [7, 64, 65, 1560, 6240, 8190])
def test_a_decoder_bit_exact_on_quantised_llrs(dec_engine, n_steps, ncw):
    """every fp32 sum is exact (|metric| <= 8190 x 24 x 64 grid units < 2^24), so host float32 and device differ only if the tie rule does"""
    llr = _quantised(np.random.default_rng(n_steps * 1000 + ncw), ncw, n_steps)
    got = dec_engine.viterbi_decode(llr)
    want = L.viterbi(llr, np.float32)
    assert got.shape == want.shape == (ncw, n_steps - 6)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


@pytest.mark.parametrize('n_info', [1, 59, 300, 8184])
def test_b_c_noiseless_and_flipped_codewords(dec_engine, n_info):
    rng = np.random.default_rng(n_info)
    bits = rng.integers(0, 2, (5, n_info)).astype(np.uint8)
    llr = 1.0 - 2.0 * L.encode(bits).astype(np.float32)
    assert np.array_equal(dec_engine.viterbi_decode(llr), bits)
    for i in range(5):                                                           # 7 flips: below half the free distance of 15
        llr[i, rng.choice(llr.shape[1], 7, replace=False)] *= -1.0
    assert np.array_equal(dec_engine.viterbi_decode(llr), bits)


@pytest.mark.parametrize('n_steps', [1560, 8190])
def test_d_ml_shortfall_on_real_llrs(dec_engine, n_steps):
    """Encoded frames + Gaussian noise at 0 dB.  In fp64 the path metric of the device's codeword may fall short of the fp64 decoder's
    optimum by at most 4 x the largest shortfall of the float32 HOST decoder on the same inputs, relative to sum |llr| (fp32
    accumulation over thousands of steps is not derivable tighter).  Recorded: yardstick 0, device 0 at both lengths."""
    rng = np.random.default_rng(n_steps)
    ncw = 12
    bits = rng.integers(0, 2, (ncw, n_steps - 6)).astype(np.uint8)
    y = (1.0 - 2.0 * L.encode(bits)) + rng.standard_normal((ncw, 3 * n_steps))
    llr = (2.0 * y).astype(np.float32)
    norm = np.abs(llr.astype(np.float64)).sum(1)
    best = L.path_metric(llr, L.viterbi(llr, np.float64))
    host = (best - L.path_metric(llr, L.viterbi(llr, np.float32))) / norm
    dev_bits = dec_engine.viterbi_decode(llr)
    dev = (best - L.path_metric(llr, dev_bits)) / norm
    print('n_steps %d: float32 host decoder shortfall max %.3e (yardstick), device %.3e, bound %.3e; device bit errors %d of %d'
          % (n_steps, host.max(), dev.max(), 4 * host.max(), int((dev_bits != bits).sum()), bits.size))
    assert host.min() >= -1e-12 and dev.min() >= -1e-12            # nothing beats the fp64 optimum
    assert dev.max() <= 4.0 * host.max()


# ------------------------------------------------------------------------------------------------ transmit / receive pass
@pytest.mark.parametrize('shape', SHAPES)
def test_e_equalised_symbols_and_csi_against_fp64(pkg, oracle, shape):
    """every item: |x - x_ref| <= max(1e-5, 1e-6 cond(G)^2) max(1, |x_ref|); csi the same bound relative to csi_ref itself (1 / [A^-1]_ss
    inherits the relative error of A^-1, cond(A) = cond(G)^2 units of fp32).  Recorded: largest error / bound 0.151."""
    e, h, fbb, frf, nv, dev, ref = _run(pkg, oracle, shape)
    worst = 0.0
    for p, r in enumerate(ref):
        assert np.isfinite(r['cond']).all()
        bound = np.maximum(1e-5, 1e-6 * r['cond'] ** 2)                           # [234]
        ex = np.abs(dev.xeq[p].astype(np.complex128) - r['x']) / np.maximum(1.0, np.abs(r['x'])) / bound
        ec = np.abs(dev.csi[p].astype(np.float64) - r['csi']) / r['csi'] / bound
        worst = max(worst, ex.max(), ec.max())
    print('%s: cond(G) up to %.3g, largest error / bound %.3f' % (shape, max(r['cond'].max() for r in ref), worst))
    assert worst <= 1.0


@pytest.mark.parametrize('shape', SHAPES)
def test_f_replay_of_the_later_stages(pkg, oracle, shape):
    e, h, fbb, frf, nv, dev, ref = _run(pkg, oracle, shape)
    nt, nr, ns, ntrf, bps, n_sym, npkt = shape
    for p, r in enumerate(ref):
        x, csi = dev.xeq[p].astype(np.complex128), dev.csi[p].astype(np.float64)
        llr = L.soft_bits(x, csi, float(nv[p]), bps)
        err = np.abs(dev.llr[p] - llr).max() / np.abs(llr).max()
        assert err <= 1e-5, (p, err)
        evm = L.evm_rms(x, bps)
        assert abs(dev.evm_rms[p] - evm) <= 1e-5 * evm, (p, dev.evm_rms[p], evm)
        assert abs(dev.dt_snr_db[p] - r['dt_snr_db']) <= 1e-4, (p, dev.dt_snr_db[p], r['dt_snr_db'])
        assert dev.bit_errors[p] == int((dev.bits[p] ^ r['bits']).sum())
    assert np.array_equal(dev.bits, e.viterbi_decode(dev.llr))
    assert dev.n_info == L.frame_bits(ns, n_sym, bps)[0] == dev.bits.shape[1]
    print('%s: bit errors %s, EVM %s %%, dtSNR %s dB' % (shape, dev.bit_errors.tolist(), np.round(dev.evm_rms.astype(np.float64), 2).tolist(), np.round(dev.dt_snr_db.astype(np.float64), 2).tolist()))


def test_g_noise_and_bit_streams(pkg, oracle):
    """H = identity on every subcarrier, frf_mean = fbb = identity: F = I, |F|_F = 2, W = sqrt(4) I / 2 = I, G = I, so x = d + w.  The
    data cannot be switched off; the fp64 symbols of the host bit replay are subtracted instead.  noise_var 0.02: |x| < 1.3, half an
    ulp of x is 6e-8, and the fp32 logf / cosf of tr_normal stay below 1e-6 of a deviate scaled by 0.1."""
    nt = nr = ns = ntrf = 4
    n_sym, bps, npkt, seed, first = 2, 2, 2, 77, 9
    e = _engine(pkg, oracle, nt, nr)
    eye = np.eye(4)
    h = np.broadcast_to(eye[None, :, :, None], (npkt, nr, nt, L.N)).astype(np.complex128)
    fbb = np.broadcast_to(eye, (npkt, L.N, ns, ntrf)).astype(np.complex128)
    frf = np.broadcast_to(eye, (npkt, ntrf, nt)).astype(np.complex128)
    nv = np.float32(0.02)
    dev = e.link_sim(h, fbb, frf, nv, seed=seed, first_pkt=first, n_sym=n_sym, bps=bps, details=True)
    n_info = L.frame_bits(ns, n_sym, bps)[0]
    for p in range(npkt):
        bits = L.info_bits(seed, first + p, n_info)
        d = L.map_bits(L.encode(bits), ns, n_sym, bps)                            # [s, n, k]
        w = np.sqrt(float(nv) / 2.0) * L.noise_normals(seed, first + p, n_sym, nr)  # [n, k, r]; G = I: stream s is rx antenna s
        got = dev.xeq[p].astype(np.complex128) - d
        err = np.abs(got - w.transpose(2, 0, 1)).max()
        print('packet %d: |w_dev - w_replay| max %.3e' % (first + p, err))
        assert err <= 1e-6
        assert np.array_equal(dev.bits[p], bits) and dev.bit_errors[p] == 0
        assert np.abs(dev.csi[p] - 1.0).max() <= 1e-6
    assert np.abs(dev.dt_snr_db).max() <= 1e-5                                    # |H W|^2 = |H|^2


# ------------------------------------------------------------------------------------------------ determinism
def _device_call(e, dev_in, seed, first, npkt, ns, ntrf, n_sym, bps, n_info, n_coded, outs=None):
    if outs is None:
        outs = [e.empty((npkt,)) for _ in range(3)] + [e.empty((npkt, ns, n_sym, L.N)), e.empty((npkt, ns, n_sym, L.N)),
                                                       e.empty((npkt, ns, L.N)), e.empty((npkt, n_coded)), e.empty(((npkt * n_info + 3) // 4,))]
    e.link_sim_device(*dev_in, seed, first, npkt, ns, ntrf, *outs[:3], n_sym=n_sym, bps=bps, d_xeq_re=outs[3], d_xeq_im=outs[4], d_csi=outs[5],
                      d_llr=outs[6], d_bits=outs[7])
    return outs


def _fetch(e, outs, npkt, n_info):
    e.synchronize()
    return [o.download().view(np.uint32) for o in outs[:7]] + [outs[7].download().view(np.uint8)[:npkt * n_info]]


def test_h_determinism_ranges_chunks_and_graph(pkg, oracle):
    shape = (8, 4, 2, 2, 2, 2, 6)
    nt, nr, ns, ntrf, bps, n_sym, npkt = shape
    n_info, n_coded = L.frame_bits(ns, n_sym, bps)
    e = _engine(pkg, oracle, nt, nr)
    h, fbb, frf, nv = _inputs(e, shape, snr_db=3.0)
    host_in = [h.real, h.imag, fbb.real, fbb.imag, frf.real, frf.imag, nv]
    dev_in = [e.to_device(np.ascontiguousarray(a, np.float32)) for a in host_in]
    full = _fetch(e, _device_call(e, dev_in, SEED, FIRST, npkt, ns, ntrf, n_sym, bps, n_info, n_coded), npkt, n_info)
    assert full[0].view(np.int32).sum() > 0                                       # 3 dB: there are bit errors to repeat
    again = _fetch(e, _device_call(e, dev_in, SEED, FIRST, npkt, ns, ntrf, n_sym, bps, n_info, n_coded), npkt, n_info)
    assert all(np.array_equal(a, b) for a, b in zip(full, again))
    # two calls of 3 packets
    for half in (0, 3):
        part_in = [e.to_device(np.ascontiguousarray(a[half:half + 3], np.float32)) for a in host_in]
        part = _fetch(e, _device_call(e, part_in, SEED, FIRST + half, 3, ns, ntrf, n_sym, bps, n_info, n_coded), 3, n_info)
        for f, q in zip(full[:7], part[:7]):
            assert np.array_equal(f[half:half + 3], q)
        assert np.array_equal(full[7][half * n_info:(half + 3) * n_info], part[7])
    # a workspace of one packet's bytes: six chunks, with and without the caller's llr array
    small = _engine(pkg, oracle, nt, nr, workspace_bytes=1024)
    s_in = [small.to_device(np.ascontiguousarray(a, np.float32)) for a in host_in]
    n0 = small.get_option('link_launches')
    chunked = _fetch(small, _device_call(small, s_in, SEED, FIRST, npkt, ns, ntrf, n_sym, bps, n_info, n_coded), npkt, n_info)
    assert small.get_option('link_launches') == n0 + 3 * npkt
    assert all(np.array_equal(a, b) for a, b in zip(full, chunked))
    outs = [small.empty((npkt,)) for _ in range(3)]
    small.link_sim_device(*s_in, SEED, FIRST, npkt, ns, ntrf, *outs, n_sym=n_sym, bps=bps)
    small.synchronize()
    assert all(np.array_equal(o.download().view(np.uint32), f) for o, f in zip(outs, full[:3]))
    # a bf16 context is served with the same bits
    b = _engine(pkg, oracle, nt, nr, dtype='bf16')
    b_in = [b.to_device(np.ascontiguousarray(a, np.float32)) for a in host_in]
    assert all(np.array_equal(x, y) for x, y in zip(full, _fetch(b, _device_call(b, b_in, SEED, FIRST, npkt, ns, ntrf, n_sym, bps, n_info, n_coded), npkt, n_info)))
    # a captured graph replays to the eager bits
    outs = _device_call(e, dev_in, SEED, FIRST, npkt, ns, ntrf, n_sym, bps, n_info, n_coded)
    e.synchronize()
    e.capture_begin()
    try:
        _device_call(e, dev_in, SEED, FIRST, npkt, ns, ntrf, n_sym, bps, n_info, n_coded, outs=outs)
    finally:
        g = e.capture_end()
    for o in outs:
        o.upload(np.zeros(o.shape, np.float32))
    g.launch()
    replay = _fetch(e, outs, npkt, n_info)
    assert all(np.array_equal(a, b) for a, b in zip(full, replay))
    g.free()


# ------------------------------------------------------------------------------------------------ degenerate inputs, refusals
def test_i_degenerate_inputs(pkg, oracle):
    shape = (8, 4, 2, 2, 2, 2, 8)
    nt, nr, ns, ntrf, bps, n_sym, npkt = shape
    e = _engine(pkg, oracle, nt, nr)
    h, fbb, frf, nv = _inputs(e, shape)
    fbb[1, 7] = 0.0
    dev = e.link_sim(h, fbb, frf, nv, seed=3, first_pkt=0, n_sym=n_sym, bps=bps, details=True)
    assert (dev.xeq[1, :, :, 7] == 0).all() and (dev.csi[1, :, 7] == 0).all()
    assert (dev.llr.reshape(npkt, ns, n_sym, L.N, bps)[1, :, :, 7] == 0).all()
    for a in (dev.evm_rms, dev.dt_snr_db, dev.xeq.real, dev.xeq.imag, dev.csi, dev.llr):
        assert np.isfinite(a).all()
    assert (dev.csi[0] > 0).all()
    # noise far above the signal: the decoder sees noise only
    dev = e.link_sim(h, fbb, frf, np.float32(1e30), seed=3, first_pkt=0, n_sym=n_sym, bps=bps)
    ber = dev.bit_errors.sum() / (npkt * dev.n_info)
    print('noise_var 1e30: BER %.4f over %d bits' % (ber, npkt * dev.n_info))
    assert np.isfinite(dev.evm_rms).all() and np.isfinite(dev.dt_snr_db).all()
    assert abs(ber - 0.5) <= 0.05


def test_j_refusals_carry_text(pkg, oracle):
    nt, nr = 8, 2
    e = _engine(pkg, oracle, nt, nr)
    lib, ctx = e._lib, e._ctx
    buf = e.empty((3 * 8200,))
    p = buf.ptr

    def link(text, seed=1, first=0, npkt=1, ns=1, ntrf=1, n_sym=1, bps=2, req=(p,) * 10, opt=(None,) * 5):
        args = list(req[:7]) + [seed, first, npkt, ns, ntrf, n_sym, bps] + list(req[7:]) + list(opt)
        assert lib.csi_link_sim_device(ctx, *args) == -1
        assert text in lib.csi_last_error(ctx).decode(), lib.csi_last_error(ctx)

    link('bps 3 is not 2', bps=3)
    link('bps 6 is not 2', bps=6)
    link('ns 0 outside 1 .. min(4, Nr 2, ntrf 1)', ns=0)
    link('ns 2 outside 1 .. min(4, Nr 2, ntrf 1)', ns=2)
    link('ns 3 outside 1 .. min(4, Nr 2, ntrf 4)', ns=3, ntrf=4)
    link('ntrf 0 must be at least 1', ntrf=0)
    link('n_sym 0 must be at least 1', n_sym=0)
    link('n_steps 8268 = ns 1 x n_sym 53 x 234 x bps 2 / 3 exceeds 8190', n_sym=53)
    link('must not be negative', npkt=-1)
    link('must not be negative', first=-1)
    for i in range(10):
        link('null required pointer', req=tuple(None if j == i else p for j in range(10)))
    link('come as a pair', opt=(p, None, None, None, None))
    assert lib.csi_link_sim_device(ctx, *[None] * 7, 1, 0, 0, 1, 1, 1, 2, *[None] * 8) == 0          # nothing to do
    # 52 symbols: n_steps = 8112 is served
    assert lib.csi_link_frame_bits(1, 52, 2, None, None) == 0

    def vit(text, *args):
        assert lib.csi_viterbi_decode_device(ctx, *args) == -1
        assert text in lib.csi_last_error(ctx).decode(), lib.csi_last_error(ctx)

    vit('n_steps 8191 outside 7 .. 8190', p, 1, 8191, p)
    vit('n_steps 6 outside 7 .. 8190', p, 1, 6, p)
    vit('ncw -1 is negative', p, -1, 7, p)
    vit('null required pointer', None, 1, 7, p)
    vit('null required pointer', p, 1, 7, None)
    assert lib.csi_viterbi_decode_device(ctx, None, 0, 7, None) == 0
    with pytest.raises(pkg.CsiError, match='llr must be'):
        e.viterbi_decode(np.zeros((2, 20), np.float32))
    with pytest.raises(pkg.CsiError, match='csi_link_frame_bits'):
        e.link_frame_bits(1, 10, 3)
    one = pkg.CsiEngine(0, 1, hidden=(16,), len_ltf=64)
    assert one._lib.csi_link_sim_device(one._ctx, *[p] * 7, 1, 0, 1, 1, 1, 1, 2, *[p] * 3, *[None] * 5) == -1
    assert 'single-input context' in one._lib.csi_last_error(one._ctx).decode()


# ------------------------------------------------------------------------------------------------ noise level, sweep
def test_k_noise_level_of_the_sounding_phase(pkg, oracle):
    """The LS estimate of a link averages Nt bins of noise variance link_noise_var (P P^T = Nt I): its mean squared error against the true
    planes is link_noise_var / Nt.  8 x 4 x 8 x 234 = 59904 complex samples: the sampling deviation of the mean is 1 / sqrt(59904) = 0.4 %."""
    nt, nr, npkt = 8, 4, 8
    e = _engine(pkg, oracle, nt, nr)
    d_re, d_im, h_re, h_im, d_std = e.synth_structured(31, 0, npkt, snr_db=0.0)
    l_re, l_im = e.empty((npkt, nr, nt, L.N)), e.empty((npkt, nr, nt, L.N))
    e.ls_estimate_device(d_re, d_im, npkt, l_re, l_im)
    e.synchronize()
    mse = (np.abs(_c(l_re, l_im) - _c(h_re, h_im)) ** 2).mean((1, 2, 3))
    want = pkg.synth.link_noise_var(d_std.download()) / nt
    ratio = float((mse / want).mean())
    print('LS error / (link_noise_var / Nt): %.4f (per packet %s)' % (ratio, np.round(mse / want, 3).tolist()))
    assert abs(ratio - 1.0) <= 0.05


def test_l_sweep_with_the_data_phase(pkg, oracle, tmp_path):
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    out = str(tmp_path / 'ber')
    common = ['--nTX', '8', '--nRX', '2', '--nn', '16', '--trainPkts', '24', '--testPkts', '6', '--snr', '-10', '10', '--epochs', '1',
              '--bs', '32', '--quiet']
    assert sweep.main(['-d', out] + common + ['--ber', '--numSTS', '1', '--rays', '64', '--dataSymbols', '2']) == 0
    names = [f + x for f in ('MSE_', 'bers_', 'EVM_rms_', 'dtSNR_') for x in ('LS', 'MMSE', 'DNN', 'perfect')]
    n_info = L.frame_bits(1, 2, 2)[0]
    for snr in (-10, 10):
        m = loadmat(os.path.join(out, 'BS8_SNR%g' % snr, 'metrics.mat'))
        assert sorted(k for k in m if not k.startswith('__')) == sorted(names)
        for k in names:
            assert m[k].shape == (1, 6) and np.isfinite(m[k]).all(), k
        for x in ('LS', 'MMSE', 'DNN', 'perfect'):
            errs = m['bers_' + x][0] * n_info
            assert np.abs(errs - np.rint(errs)).max() < 1e-9 and (m['bers_' + x] >= 0).all() and (m['bers_' + x] <= 1).all()
            assert (m['EVM_rms_' + x] > 0).all()
        assert (m['MSE_perfect'] == 0).all()
        print('snr %g dB: BER %s' % (snr, {x: float(m['bers_' + x].mean()) for x in ('LS', 'MMSE', 'DNN', 'perfect')}))
        if snr == 10:
            assert (m['bers_perfect'] == 0).all()
    import json
    res = json.load(open(os.path.join(out, 'sweep.json')))
    assert res['ber'] == dict(ns=1, ntrf=1, n_sym=2, bps=2)
    assert all('BER_' + x in lv for lv in res['levels'] for x in ('LS', 'MMSE', 'DNN', 'perfect'))
    # without --ber: today's fields, today's keys
    out2 = str(tmp_path / 'plain')
    assert sweep.main(['-d', out2, '--modeldir', out] + common) == 0
    for snr in (-10, 10):
        m = loadmat(os.path.join(out2, 'BS8_SNR%g' % snr, 'metrics.mat'))
        assert sorted(k for k in m if not k.startswith('__')) == ['MSE_DNN', 'MSE_LS', 'MSE_MMSE']
        assert np.array_equal(m['MSE_LS'], loadmat(os.path.join(out, 'BS8_SNR%g' % snr, 'metrics.mat'))['MSE_LS'])
    res2 = json.load(open(os.path.join(out2, 'sweep.json')))
    assert 'ber' not in res2 and set(res2['levels'][0]) == {'snr_db', 'seconds', 'LS', 'MMSE', 'DNN'}
