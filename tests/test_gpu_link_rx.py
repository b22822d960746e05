"""GPU tests of the link simulation whose receiver estimates the effective channel from a precoded preamble (csi_link_sim_rx_device,
csrc/link_sim.hip.h + link_txrx_body.inc) against the fp64 restatement tests/link_rx_ref.py and against
csi_link_sim_device, the receiver that knows the channel.

The shapes and the input recipe are those of tests/test_gpu_link.py (12 dB); one device call per shape serves the tests (a) - (e).
The estimate is compared with fp64 directly (a); the equaliser is judged in fp64 on the device's OWN estimate (b), and the later
stages on the device's own x and csi (c), so that every stage is held to the error it can add itself.

Figures recorded on an MI355X (also in profiles/link_rx.txt): (a) max |gest - Ghat| / max |G|, the largest packet of each of the five
shapes: 2.017e-07, 2.195e-07, 1.807e-07, 2.331e-07, 4.358e-07 (GEST_RECORDED is the largest); (b) largest error / bound 0.127, cond(Ghat)
up to 522; (e) g_nmse within 1.26e-7 relative of fp64, mean |gest - G|^2 / (noise_var / n_ltf) = 0.9888 over 14976 samples."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import link_ref as L            # noqa: E402
import link_rx_ref as R         # noqa: E402
import test_gpu_link as T       # noqa: E402  (SHAPES, the input recipe)
from test_gpu_memory_contract import both_ways, _cplx, _f32      # noqa: E402

SHAPES, SEED, FIRST = T.SHAPES, T.SEED, T.FIRST
# (a): the largest max |gest - Ghat| / max |G| of a packet over SHAPES as recorded; asserted: 4 x that (other seeds - the fp32 order of
# accumulation is fixed), and never more than 1e-4
GEST_RECORDED = 4.358e-07
GEST_BOUND = min(4.0 * GEST_RECORDED, 1e-4)
_cache = {}


def _run(pkg, oracle, shape):
    """one device call (every output) and the fp64 model per shape"""
    if shape not in _cache:
        nt, nr, ns, ntrf, bps, n_sym, npkt = shape
        e = T._engine(pkg, oracle, nt, nr)
        h, fbb, frf, nv = T._inputs(e, shape)
        dev = e.link_sim_rx(h, fbb, frf, nv, seed=SEED, first_pkt=FIRST, n_sym=n_sym, bps=bps, details=True)
        ref = [R.simulate_rx(SEED, FIRST + p, h[p], frf[p], fbb[p], float(nv[p]), n_sym, bps) for p in range(npkt)]
        _cache[shape] = (e, h, fbb, frf, nv, dev, ref)
    return _cache[shape]


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


# ------------------------------------------------------------------------------------------------ the estimate
@pytest.mark.parametrize('shape', SHAPES)
def test_a_estimate_against_fp64(pkg, oracle, shape):
    """gest against the fp64 Ghat of the fp32 inputs: max |gest - Ghat| <= GEST_BOUND max |G| per packet.  Recorded per shape: 2.017e-07,
    2.195e-07, 1.807e-07, 2.331e-07, 4.358e-07; GEST_BOUND = 4 x the largest = 1.743e-06."""
    e, h, fbb, frf, nv, dev, ref = _run(pkg, oracle, shape)
    nt, nr, ns, ntrf, bps, n_sym, npkt = shape
    assert dev.gest.shape == (npkt, L.N, nr, ns) and dev.gest.dtype == np.complex64 and dev.g_nmse.shape == (npkt,)
    worst = max(np.abs(dev.gest[p].astype(np.complex128) - r['Ghat']).max() / np.abs(r['G']).max() for p, r in enumerate(ref))
    print('%s: max |gest - Ghat| / max |G| = %.3e (bound %.3e)' % (shape, worst, GEST_BOUND))
    assert worst <= GEST_BOUND


@pytest.mark.parametrize('shape', SHAPES)
def test_b_equaliser_against_fp64_on_the_device_estimate(pkg, oracle, shape):
    """x and csi against fp64 zero forcing of the device's own gest on the fp64 received symbols: the yardstick of
    test_gpu_link.test_e, max(1e-5, 1e-6 cond(Ghat)^2), x relative to max(1, |x_ref|) and csi relative to csi_ref."""
    e, h, fbb, frf, nv, dev, ref = _run(pkg, oracle, shape)
    worst = cmax = 0.0
    for p, r in enumerate(ref):
        x_ref, csi_ref, cond = L.zero_forcing(dev.gest[p].astype(np.complex128), r['y'])
        assert np.isfinite(cond).all()
        bound = np.maximum(1e-5, 1e-6 * cond ** 2)
        ex = np.abs(dev.xeq[p].astype(np.complex128) - x_ref) / np.maximum(1.0, np.abs(x_ref)) / bound
        ec = np.abs(dev.csi[p].astype(np.float64) - csi_ref) / csi_ref / bound
        worst, cmax = max(worst, ex.max(), ec.max()), max(cmax, cond.max())
    print('%s: cond(Ghat) up to %.3g, largest error / bound %.3f' % (shape, cmax, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('shape', SHAPES)
def test_c_replay_of_the_later_stages(pkg, oracle, shape):
    """llr, evm_rms and bit_errors replayed in fp64 from the device's own x and csi (as test_gpu_link.test_f); the decoded bits are
    those of the float32 host decoder on the device's llr"""
    e, h, fbb, frf, nv, dev, ref = _run(pkg, oracle, shape)
    nt, nr, ns, ntrf, bps, n_sym, npkt = shape
    for p, r in enumerate(ref):
        x, csi = dev.xeq[p].astype(np.complex128), dev.csi[p].astype(np.float64)
        llr = L.soft_bits(x, csi, float(nv[p]), bps)
        err = np.abs(dev.llr[p] - llr).max() / np.abs(llr).max()
        assert err <= 1e-5, (p, err)
        evm = L.evm_rms(x, bps)
        assert abs(dev.evm_rms[p] - evm) <= 1e-5 * evm, (p, dev.evm_rms[p], evm)
        assert dev.bit_errors[p] == int((dev.bits[p] ^ r['bits']).sum())
    assert np.array_equal(dev.bits, L.viterbi(dev.llr, np.float32))
    assert dev.n_info == L.frame_bits(ns, n_sym, bps)[0] == dev.bits.shape[1]
    print('%s: bit errors %s, EVM %s %%, g_nmse %s' % (shape, dev.bit_errors.tolist(), np.round(dev.evm_rms.astype(np.float64), 2).tolist(),
                                                      ['%.3e' % v for v in dev.g_nmse]))


def test_d_one_stream_without_noise_is_the_genie_receiver(pkg, oracle):
    """ns = 1: n_ltf = 1 and P = 1, so without noise Ghat is G to the bit and every output repeats csi_link_sim_device's"""
    shape = SHAPES[0]
    nt, nr, ns, ntrf, bps, n_sym, npkt = shape
    assert (ns, ntrf) == (1, 1)
    e, h, fbb, frf, nv = _run(pkg, oracle, shape)[:5]
    rx = e.link_sim_rx(h, fbb, frf, np.float32(0.0), seed=SEED, first_pkt=FIRST, n_sym=n_sym, bps=bps, details=True)
    ge = e.link_sim(h, fbb, frf, np.float32(0.0), seed=SEED, first_pkt=FIRST, n_sym=n_sym, bps=bps, details=True)
    for f in ('bit_errors', 'evm_rms', 'dt_snr_db', 'xeq', 'csi', 'llr', 'bits'):
        a, b = getattr(rx, f), getattr(ge, f)
        a, b = (a.view(np.float32), b.view(np.float32)) if a.dtype == np.complex64 else (a, b)
        assert np.array_equal(_bits(a), _bits(b)), f
    assert (rx.g_nmse == 0).all() and (rx.bit_errors == 0).all()


@pytest.mark.parametrize('shape', SHAPES)
def test_e_gain_and_estimation_error(pkg, oracle, shape):
    """dt_snr_db is that of the true G: the genie entry's bits.  g_nmse within 1e-5 relative of the fp64 value."""
    e, h, fbb, frf, nv, dev, ref = _run(pkg, oracle, shape)
    nt, nr, ns, ntrf, bps, n_sym, npkt = shape
    ge = e.link_sim(h, fbb, frf, nv, seed=SEED, first_pkt=FIRST, n_sym=n_sym, bps=bps)
    assert np.array_equal(_bits(dev.dt_snr_db), _bits(ge.dt_snr_db))
    want = np.array([r['g_nmse'] for r in ref])
    err = np.abs(dev.g_nmse.astype(np.float64) - want) / want
    print('%s: g_nmse %s, relative error to fp64 max %.3e' % (shape, ['%.4e' % v for v in want], err.max()))
    assert err.max() <= 1e-5


def test_e_estimation_error_level(pkg, oracle):
    """Ghat - G ~ CN(0, noise_var / n_ltf) on the device's gest: 8 x 234 x 4 x 2 = 14976 complex samples, bound 5 / sqrt(N)"""
    shape = (8, 4, 2, 2, 2, 2, 8)
    nt, nr, ns, ntrf, bps, n_sym, npkt = shape
    e = T._engine(pkg, oracle, nt, nr)
    h, fbb, frf, nv = T._inputs(e, shape)
    dev = e.link_sim_rx(h, fbb, frf, nv, seed=SEED, first_pkt=FIRST, n_sym=n_sym, bps=bps, details=True)
    unit = []
    for p in range(npkt):
        G = L.effective_channel(h[p], L.precoder(frf[p], fbb[p]))
        unit.append(np.abs(dev.gest[p].astype(np.complex128) - G).reshape(-1) ** 2 / (float(nv[p]) / R.N_LTF[ns]))
    unit = np.concatenate(unit)
    assert unit.size == 14976
    print('mean |gest - G|^2 / (noise_var / n_ltf) = %.4f over %d samples, bound %.4f' % (unit.mean(), unit.size, 5 / np.sqrt(unit.size)))
    assert abs(unit.mean() - 1.0) <= 5.0 / np.sqrt(unit.size)


# ------------------------------------------------------------------------------------------------ determinism
def _device_call(e, dev_in, seed, first, npkt, ns, ntrf, n_sym, bps, n_info, n_coded, outs=None):
    nr = e.nr
    if outs is None:
        outs = [e.empty((npkt,)) for _ in range(4)] + [e.empty((npkt, ns, n_sym, L.N)), e.empty((npkt, ns, n_sym, L.N)), e.empty((npkt, ns, L.N)),
                                                       e.empty((npkt, n_coded)), e.empty((npkt, L.N, nr, ns)), e.empty((npkt, L.N, nr, ns)),
                                                       e.empty(((npkt * n_info + 3) // 4,))]
    e.link_sim_rx_device(*dev_in, seed, first, npkt, ns, ntrf, *outs[:4], n_sym=n_sym, bps=bps, d_xeq_re=outs[4], d_xeq_im=outs[5], d_csi=outs[6],
                         d_llr=outs[7], d_gest_re=outs[8], d_gest_im=outs[9], d_bits=outs[10])
    return outs


def _fetch(e, outs, npkt, n_info):
    """ten arrays with the packet on the leading axis, then the bits"""
    e.synchronize()
    return [o.download().view(np.uint32).reshape(npkt, -1) for o in outs[:10]] + [outs[10].download().view(np.uint8)[:npkt * n_info].reshape(npkt, n_info)]


def test_f_determinism_ranges_chunks_and_graph(pkg, oracle):
    shape = (8, 4, 2, 2, 2, 2, 6)
    nt, nr, ns, ntrf, bps, n_sym, npkt = shape
    n_info, n_coded = L.frame_bits(ns, n_sym, bps)
    e = T._engine(pkg, oracle, nt, nr)
    h, fbb, frf, nv = T._inputs(e, shape, snr_db=3.0)
    host_in = [h.real, h.imag, fbb.real, fbb.imag, frf.real, frf.imag, nv]
    dev_in = [e.to_device(np.ascontiguousarray(a, np.float32)) for a in host_in]
    args = (ns, ntrf, n_sym, bps, n_info, n_coded)
    full = _fetch(e, _device_call(e, dev_in, SEED, FIRST, npkt, *args), npkt, n_info)
    assert full[0].view(np.int32).sum() > 0                                       # 3 dB: there are bit errors to repeat
    again = _fetch(e, _device_call(e, dev_in, SEED, FIRST, npkt, *args), npkt, n_info)
    assert all(np.array_equal(a, b) for a, b in zip(full, again))
    # two calls of 3 packets
    for half in (0, 3):
        part_in = [e.to_device(np.ascontiguousarray(a[half:half + 3], np.float32)) for a in host_in]
        part = _fetch(e, _device_call(e, part_in, SEED, FIRST + half, 3, *args), 3, n_info)
        for f, q in zip(full, part):
            assert np.array_equal(f[half:half + 3], q)
    # a workspace of two packets' coded bits: three chunks
    small = T._engine(pkg, oracle, nt, nr, workspace_bytes=2 * n_coded + 200)
    s_in = [small.to_device(np.ascontiguousarray(a, np.float32)) for a in host_in]
    n0 = small.get_option('link_launches')
    chunked = _fetch(small, _device_call(small, s_in, SEED, FIRST, npkt, *args), npkt, n_info)
    assert small.get_option('link_launches') == n0 + 3 * 3
    assert all(np.array_equal(a, b) for a, b in zip(full, chunked))
    # a captured graph replays to the eager bits
    outs = _device_call(e, dev_in, SEED, FIRST, npkt, *args)
    e.synchronize()
    e.capture_begin()
    try:
        _device_call(e, dev_in, SEED, FIRST, npkt, *args, outs=outs)
    finally:
        g = e.capture_end()
    for o in outs:
        o.upload(np.zeros(o.shape, np.float32))
    g.launch()
    replay = _fetch(e, outs, npkt, n_info)
    assert all(np.array_equal(a, b) for a, b in zip(full, replay))
    g.free()


# ------------------------------------------------------------------------------------------------ degenerate inputs, refusals
def test_g_degenerate_inputs(pkg, oracle):
    shape = (8, 4, 2, 2, 2, 2, 4)
    nt, nr, ns, ntrf, bps, n_sym, npkt = shape
    e = T._engine(pkg, oracle, nt, nr)
    h, fbb, frf, nv = T._inputs(e, shape)
    zero = np.zeros_like(fbb)
    dev = e.link_sim_rx(h, zero, frf, np.float32(0.0), seed=3, first_pkt=0, n_sym=n_sym, bps=bps, details=True)
    assert (dev.xeq == 0).all() and (dev.csi == 0).all() and (dev.g_nmse == 0).all() and (dev.gest == 0).all() and (dev.llr == 0).all()
    dev = e.link_sim_rx(h, zero, frf, nv, seed=3, first_pkt=0, n_sym=n_sym, bps=bps, details=True)
    for a in (dev.evm_rms, dev.xeq.real, dev.xeq.imag, dev.csi, dev.llr, dev.gest.real, dev.gest.imag):
        assert np.isfinite(a).all()
    assert (dev.dt_snr_db == -np.inf).all() and (dev.g_nmse == np.inf).all()
    assert (dev.csi > 0).all()                                                    # the estimate of a zero channel is noise: regular
    dev = e.link_sim_rx(h, fbb, frf, np.float32(1e30), seed=3, first_pkt=0, n_sym=n_sym, bps=bps, details=True)
    assert not np.isnan(dev.evm_rms).any() and not np.isnan(dev.llr).any() and (dev.bit_errors >= 0).all() and (dev.bit_errors <= dev.n_info).all()
    ber = dev.bit_errors.sum() / (npkt * dev.n_info)
    print('noise_var 1e30: BER %.4f over %d bits' % (ber, npkt * dev.n_info))


def test_h_refusals_carry_text(pkg, oracle):
    nt, nr = 8, 2
    e = T._engine(pkg, oracle, nt, nr)
    lib, ctx = e._lib, e._ctx
    buf = e.empty((3 * 8200,))
    p = buf.ptr

    def link(text, seed=1, first=0, npkt=1, ns=1, ntrf=1, n_sym=1, bps=2, req=(p,) * 11, opt=(None,) * 7):
        """req: the seven inputs, bit_errors, evm_rms, dt_snr_db, g_nmse; opt: xeq_re, xeq_im, csi, llr, bits, gest_re, gest_im"""
        args = list(req[:7]) + [seed, first, npkt, ns, ntrf, n_sym, bps] + list(req[7:10]) + list(opt[:5]) + [req[10]] + list(opt[5:])
        assert lib.csi_link_sim_rx_device(ctx, *args) == -1
        msg = lib.csi_last_error(ctx).decode()
        assert text in msg and 'csi_link_sim_rx_device' in msg, msg

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
    for i in range(11):                                                           # g_nmse (the last) is required too
        link('null required pointer', req=tuple(None if j == i else p for j in range(11)))
    link('the xeq planes come as a pair', opt=(p, None, None, None, None, None, None))
    link('the gest planes come as a pair', opt=(None, None, None, None, None, p, None))
    link('the gest planes come as a pair', opt=(None, None, None, None, None, None, p))
    assert lib.csi_link_sim_rx_device(ctx, *[None] * 7, 1, 0, 0, 1, 1, 1, 2, *[None] * 11) == 0         # nothing to do
    # the LDS image holds G twice: Nr 64, ns 4 needs 2 x 128 KiB for the two arrays alone; the genie entry serves the shape's G (128 KiB + fbb)
    big = pkg.CsiEngine(8, 64, hidden=(8,))
    args = [p] * 7 + [1, 0, 1, 4, 4, 1, 2] + [p] * 3 + [None] * 5 + [p, None, None]
    assert big._lib.csi_link_sim_rx_device(big._ctx, *args) == -1
    msg = big._lib.csi_last_error(big._ctx).decode()
    assert 'bytes of LDS (160 KiB per workgroup)' in msg and 'csi_link_sim_rx_device' in msg, msg
    one = pkg.CsiEngine(0, 1, hidden=(16,), len_ltf=64)
    assert one._lib.csi_link_sim_rx_device(one._ctx, *[p] * 7, 1, 0, 1, 1, 1, 1, 2, *[p] * 3, *[None] * 5, p, None, None) == -1
    assert 'single-input context' in one._lib.csi_last_error(one._ctx).decode()
    with pytest.raises(pkg.CsiError, match='csi_link_preamble_symbols'):
        e.link_preamble_symbols(5)
    assert [e.link_preamble_symbols(ns) for ns in (1, 2, 3, 4)] == [1, 2, 4, 4]


# ------------------------------------------------------------------------------------------------ memory contract
@pytest.mark.parametrize('ns,ntrf,bps', [(1, 1, 2), (3, 3, 4)])
def test_i_guard_bands(pkg, oracle, ns, ntrf, bps):
    """every output of the new entry between guard bands (tests/guarded.py), as test_gpu_memory_contract.test_a_link_sim_device"""
    nt, nr, n_sym, npkt = 8, 4, 2, 3
    rng = np.random.default_rng(70 + ns)
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(oracle.hadamard(nt))
    n_info, n_coded = e.link_frame_bits(ns, n_sym, bps)
    h, fbb = _cplx(rng, (npkt, nr, nt, L.N)), _cplx(rng, (npkt, L.N, ns, ntrf))
    frf = np.exp(2j * np.pi * rng.random((npkt, ntrf, nt))).astype(np.complex64)
    ins = {'h_re': _f32(h.real), 'h_im': _f32(h.imag), 'fbb_re': _f32(fbb.real), 'fbb_im': _f32(fbb.imag), 'frf_re': _f32(frf.real),
           'frf_im': _f32(frf.imag), 'noise_var': _f32(np.full(npkt, 0.05))}
    xeq, gest = (npkt, ns, n_sym, L.N), (npkt, L.N, nr, ns)
    outs = {'bit_errors': (npkt,), 'evm_rms': (npkt,), 'dt_snr_db': (npkt,), 'g_nmse': (npkt,), 'xeq_re': xeq, 'xeq_im': xeq,
            'csi': (npkt, ns, L.N), 'llr': (npkt, n_coded), 'bits': ((npkt * n_info + 3) // 4,), 'gest_re': gest, 'gest_im': gest}

    def call(i, o):
        e.link_sim_rx_device(i['h_re'], i['h_im'], i['fbb_re'], i['fbb_im'], i['frf_re'], i['frf_im'], i['noise_var'], 21, 4, npkt, ns, ntrf,
                             o['bit_errors'], o['evm_rms'], o['dt_snr_db'], o['g_nmse'], n_sym=n_sym, bps=bps, d_xeq_re=o['xeq_re'],
                             d_xeq_im=o['xeq_im'], d_csi=o['csi'], d_llr=o['llr'], d_bits=o['bits'], d_gest_re=o['gest_re'], d_gest_im=o['gest_im'])

    got = both_ways(e, call, ins, outs, {'link_launches': 3}, byte_len={'bits': npkt * n_info})
    assert np.isfinite(got['llr']).all() and np.isfinite(got['gest_re']).all() and (got['g_nmse'] > 0).all()
    assert (got['bits'].view(np.uint8)[:npkt * n_info] <= 1).all()
    e.close()


# ------------------------------------------------------------------------------------------------ sweep
def test_j_sweep_with_the_estimating_receiver(pkg, oracle, tmp_path):
    import json
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    out, out2 = str(tmp_path / 'rx'), str(tmp_path / 'genie')
    common = ['--nTX', '8', '--nRX', '4', '--nn', '16', '--trainPkts', '24', '--testPkts', '6', '--snr', '0', '15', '--epochs', '1',
              '--bs', '32', '--quiet', '--ber', '--numSTS', '2', '--rays', '64', '--dataSymbols', '2']
    assert sweep.main(['-d', out] + common + ['--rxEstimate']) == 0
    assert sweep.main(['-d', out2, '--modeldir', out] + common) == 0
    new = [f + x for x in sweep.SOURCES for f in sweep.RX_FIELDS]
    for snr in (0, 15):
        m = loadmat(os.path.join(out, 'BS8_SNR%g' % snr, 'metrics.mat'))
        m2 = loadmat(os.path.join(out2, 'BS8_SNR%g' % snr, 'metrics.mat'))
        old = sorted(k for k in m2 if not k.startswith('__'))
        assert sorted(k for k in m if not k.startswith('__')) == sorted(old + new)
        for k in old:
            assert np.array_equal(m[k], m2[k]), k
        for k in new:
            assert m[k].shape == (1, 6) and np.isfinite(m[k]).all(), k
        for x in sweep.SOURCES:
            assert (m['gNMSE_' + x] > 0).all() and (m['EVM_rmsRx_' + x] > 0).all()
            assert (m['bersRx_' + x] >= 0).all() and (m['bersRx_' + x] <= 1).all()
        print('snr %g dB: EVM %s, with the estimate %s, gNMSE %s' % (snr, {x: round(float(m['EVM_rms_' + x].mean()), 2) for x in sweep.SOURCES},
              {x: round(float(m['EVM_rmsRx_' + x].mean()), 2) for x in sweep.SOURCES}, {x: '%.2e' % m['gNMSE_' + x].mean() for x in sweep.SOURCES}))
    res, res2 = json.load(open(os.path.join(out, 'sweep.json'))), json.load(open(os.path.join(out2, 'sweep.json')))
    assert res['rx_estimate'] is True and 'rx_estimate' not in res2
    for lv, lv2 in zip(res['levels'], res2['levels']):
        keys = [k for k in lv2 if k != 'seconds']
        assert list(lv)[:len(lv2)] == list(lv2) and list(lv)[len(lv2):] == new
        assert all(lv[k] == lv2[k] for k in keys)
