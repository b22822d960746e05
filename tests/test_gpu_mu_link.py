"""GPU tests of the multi-user downlink (csi_mu_precoder_device / csi_mu_link_sim_device, csrc/mu_link.hip.h) against
the host restatement tests/mu_link_ref.py.

The precoder is compared with fp64 per item (bound: the Gram form loses cond(B)^2 of the fp32 budget; tests/test_mu_link_host.py holds
the fp32 emulation the bound rests on).  Every later stage is judged on what the device actually had in front of it: the effective
channel against H W of the device's own W, the equaliser against the fp64 replay from the device's own g, soft bits and decoding from
the device's own x and csi.  Inputs are i.i.d. complex Gaussian planes of a seeded generator, rounded to fp32."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import link_ref as L        # noqa: E402
import mu_link_ref as MU    # noqa: E402
from guarded import Guarded  # noqa: E402

# (Nt, Nr, U, ns, bps, n_sym, npkt)
SHAPES = [(4, 2, 2, 1, 2, 1, 3), (4, 2, 2, 2, 2, 2, 3), (8, 4, 2, 4, 4, 1, 2), (8, 2, 4, 1, 2, 3, 5), (32, 4, 4, 4, 2, 1, 2), (32, 4, 8, 2, 4, 2, 2),
          (32, 4, 1, 4, 2, 1, 2)]
SEED, FIRST = 33, 5
_cache = {}
_engines = {}


def _f32(a):
    """what the library receives: fp32 planes, as complex128"""
    a = np.asarray(a)
    return a.real.astype(np.float32).astype(np.float64) + 1j * a.imag.astype(np.float32).astype(np.float64)


def _engine(pkg, oracle, nt, nr, **kw):
    key = (nt, nr) + tuple(sorted(kw.items()))
    if key not in _engines:
        e = pkg.CsiEngine(nt, nr, hidden=(8,), device=0, **kw)
        e.set_pilot(oracle.hadamard(nt))
        _engines[key] = e
    return _engines[key]


def _channels(shape, seed=0):
    nt, nr, nu, ns, bps, n_sym, npkt = shape
    rng = np.random.default_rng(1000 * nt + 100 * nu + 10 * ns + seed)
    return [_f32((rng.standard_normal((npkt, nr, nt, L.N)) + 1j * rng.standard_normal((npkt, nr, nt, L.N))) / np.sqrt(2.0)) for _ in range(nu)]


def _noise_var(h, W, ns, snr_db):
    """[U, npkt]: snr_db below the mean own-signal power per addressed antenna"""
    nv = np.empty((len(h), W.shape[0]), np.float32)
    for u in range(len(h)):
        for p in range(W.shape[0]):
            G = MU.effective_channel(h[u][p], W[p], ns)[:, :, u * ns:(u + 1) * ns]
            nv[u, p] = (np.abs(G) ** 2).sum((1, 2)).mean() / ns * 10.0 ** (-snr_db / 10.0)
    return nv


def _run(pkg, oracle, shape, est_err=0.0, snr_db=14.0):
    """one precoder call, one data-phase call and the fp64 precoder per (shape, estimate error), shared by the tests that read them"""
    key = (shape, est_err, snr_db)
    if key not in _cache:
        nt, nr, nu, ns, bps, n_sym, npkt = shape
        e = _engine(pkg, oracle, nt, nr)
        h = _channels(shape)
        hest = h
        if est_err > 0.0:
            rng = np.random.default_rng(77)
            hest = [_f32(x + np.sqrt(est_err / 2.0) * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))) for x in h]
        W = e.mu_precoder(hest, ns).astype(np.complex128)
        ref = [MU.precoder([x[p] for x in hest], ns, 0.0) for p in range(npkt)]
        nv = _noise_var(h, W, ns, snr_db)
        dev = e.mu_link_sim(h, W, nv, seed=SEED, first_pkt=FIRST, ns=ns, n_sym=n_sym, bps=bps, details=True)
        _cache[key] = (e, h, hest, W, ref, nv, dev)
    return _cache[key]


def _precoder_ratio(W, ref):
    """largest per-item |W - Wref|_F / |Wref|_F over max(1e-5, 1e-6 cond(B)^2); every item counts"""
    worst = 0.0
    for p, (Wr, cond) in enumerate(ref):
        assert np.isfinite(cond).all() and (np.abs(Wr).sum((0, 1)) > 0).all()
        err = np.sqrt((np.abs(W[p] - Wr) ** 2).sum((0, 1)) / (np.abs(Wr) ** 2).sum((0, 1)))
        worst = max(worst, float((err / np.maximum(1e-5, 1e-6 * cond ** 2)).max()))
    return worst


# ------------------------------------------------------------------------------------------------ a, b: precoder, effective channel
@pytest.mark.parametrize('shape', SHAPES)
def test_a_precoder_against_fp64(pkg, oracle, shape):
    e, h, hest, W, ref, nv, dev = _run(pkg, oracle, shape)
    nt, nr, nu, ns = shape[:4]
    worst = _precoder_ratio(W, ref)
    print('%s: cond(B) up to %.3g, largest precoder error / bound %.4f' % (shape, max(c.max() for _, c in ref), worst))
    assert worst <= 1.0
    assert np.abs((np.abs(W) ** 2).sum((1, 2)) - nt).max() <= 1e-5 * nt                # |W|_F^2 = Nt per item


@pytest.mark.parametrize('shape', SHAPES)
def test_b_effective_channel_of_the_device_precoder(pkg, oracle, shape):
    """every element of g within 4 (Nt + 2) 2^-24 sum_j |h_ij| |W_jm| of H_u W_device in fp64"""
    e, h, hest, W, ref, nv, dev = _run(pkg, oracle, shape)
    nt, nr, nu, ns, bps, n_sym, npkt = shape
    worst = 0.0
    for u in range(nu):
        for p in range(npkt):
            G = MU.effective_channel(h[u][p], W[p], ns)                                  # [234, ns, M]
            bound = 4.0 * (nt + 2) * 2.0 ** -24 * np.einsum('ijk,mjk->kim', np.abs(h[u][p][:ns]), np.abs(W[p]))
            got = dev.g[u, p].astype(np.complex128).transpose(2, 0, 1)                   # [ns, M, 234] -> [234, ns, M]
            worst = max(worst, float((np.abs(got - G) / bound).max()))
    print('%s: largest |g - H W| / bound %.4f' % (shape, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ c, d: equaliser, later stages, SINR
def _replay(shape, dev, nv, u, p, seed=SEED, first=FIRST):
    """fp64 replay of user u, packet p from the device's own g: y = G d + w, zero forcing on G_uu"""
    nt, nr, nu, ns, bps, n_sym, npkt = shape
    G = dev.g[u, p].astype(np.complex128).transpose(2, 0, 1)
    d_all = np.concatenate([MU.user_symbols(seed, first + p, v, ns, n_sym, bps)[2] for v in range(nu)], 0)
    clean = np.einsum('kim,mnk->nki', G, d_all)
    w = np.sqrt(float(nv[u, p]) / 2.0) * L.noise_normals(MU.user_seed(seed, u), first + p, n_sym, ns)
    x, csi, cond = L.zero_forcing(np.ascontiguousarray(G[:, :, u * ns:(u + 1) * ns]), clean + w)
    return G, clean, w, x, csi, cond


@pytest.mark.parametrize('shape', SHAPES)
def test_c_equaliser_and_later_stages(pkg, oracle, shape):
    e, h, hest, W, ref, nv, dev = _run(pkg, oracle, shape)
    nt, nr, nu, ns, bps, n_sym, npkt = shape
    n_info = L.frame_bits(ns, n_sym, bps)[0]
    assert dev.n_info == n_info == dev.bits.shape[2]
    worst = 0.0
    host_bits = L.viterbi(dev.llr.reshape(nu * npkt, -1), np.float32).reshape(nu, npkt, n_info)
    for u in range(nu):
        for p in range(npkt):
            G, clean, w, x, csi, cond = _replay(shape, dev, nv, u, p)
            assert np.isfinite(cond).all()
            bound = np.maximum(1e-5, 1e-6 * cond ** 2)
            ex = np.abs(dev.xeq[u, p].astype(np.complex128) - x) / np.maximum(1.0, np.abs(x)) / bound
            ec = np.abs(dev.csi[u, p].astype(np.float64) - csi) / csi / bound
            worst = max(worst, float(ex.max()), float(ec.max()))
            # the later stages from the device's own x and csi
            xd, cd = dev.xeq[u, p].astype(np.complex128), dev.csi[u, p].astype(np.float64)
            llr = L.soft_bits(xd, cd, float(nv[u, p]), bps)
            assert np.abs(dev.llr[u, p] - llr).max() <= 1e-5 * np.abs(llr).max(), (u, p)
            evm = L.evm_rms(xd, bps)
            assert abs(dev.evm_rms[u, p] - evm) <= 1e-5 * evm, (u, p)
            assert np.array_equal(dev.bits[u, p], host_bits[u, p]), (u, p)
            want = L.info_bits(MU.user_seed(SEED, u), FIRST + p, n_info)
            assert dev.bit_errors[u, p] == int((dev.bits[u, p] ^ want).sum()), (u, p)
    print('%s: largest equaliser error / bound %.4f; bit errors %s' % (shape, worst, dev.bit_errors.tolist()))
    assert worst <= 1.0


@pytest.mark.parametrize('shape', SHAPES)
def test_d_sinr_against_fp64_of_the_device_g(pkg, oracle, shape):
    """two sums of at most 234 ns M non-negative fp32 terms: relative error 234 ns M 2^-24 <= 9e-4 each, 0.008 dB together; bound 0.01 dB"""
    e, h, hest, W, ref, nv, dev = _run(pkg, oracle, shape, est_err=0.05)
    nt, nr, nu, ns, bps, n_sym, npkt = shape
    worst = 0.0
    for u in range(nu):
        for p in range(npkt):
            G = dev.g[u, p].astype(np.complex128).transpose(2, 0, 1)
            worst = max(worst, abs(float(dev.sinr_db[u, p]) - MU.sinr_db(G, u, ns, nv[u, p])))
    print('%s: largest |sinr_db - fp64| %.2e dB' % (shape, worst))
    assert np.isfinite(dev.sinr_db).all() and worst <= 0.01


# ------------------------------------------------------------------------------------------------ e: perfect CSI, no noise
@pytest.mark.parametrize('shape', SHAPES)
def test_e_perfect_csi_without_noise_has_no_bit_errors(pkg, oracle, shape):
    nt, nr, nu, ns = shape[:4]
    e = _engine(pkg, oracle, nt, nr)
    h = _channels(shape)
    W = e.mu_precoder(h, ns)
    dev = e.mu_link_sim(h, W, 0.0, seed=SEED, first_pkt=FIRST, ns=ns, n_sym=1, bps=2)
    assert dev.bit_errors.shape == (nu, shape[6]) and (dev.bit_errors == 0).all()
    print('%s: sinr_db without noise at least %.1f dB (interference at the rounding level of W)' % (shape, float(dev.sinr_db.min())))


# ------------------------------------------------------------------------------------------------ f: the single-user kernel
def test_f_cross_check_against_the_single_user_kernel(pkg, oracle):
    """Nt = 4, U = 1, ns = Nr = 2: csi_link_sim_device with frf_mean = I_4 and fbb_k = W_k^T has F = W, |F|_F^2 = Nt, its own normalisation 1
    to rounding.  xeq within twice the yardstick of (c); with noise_var = 0 the decoded bits are identical."""
    shape = (4, 2, 1, 2, 2, 2, 3)
    nt, nr, nu, ns, bps, n_sym, npkt = shape
    e = _engine(pkg, oracle, nt, nr)
    h = _channels(shape)
    W = e.mu_precoder(h, ns)                                                             # [npkt, 2, 4, 234]
    nv = _noise_var(h, W.astype(np.complex128), ns, 10.0)
    fbb = np.ascontiguousarray(W.transpose(0, 3, 1, 2))                                  # [npkt, 234, ns, ntrf = 4]
    frf = np.broadcast_to(np.eye(nt), (npkt, nt, nt)).astype(np.complex64)
    for noise in (nv, np.zeros_like(nv)):
        mu = e.mu_link_sim(h, W, noise, seed=SEED, first_pkt=FIRST, ns=ns, n_sym=n_sym, bps=bps, details=True)
        su = e.link_sim(h[0], fbb, frf, noise[0], seed=SEED, first_pkt=FIRST, n_sym=n_sym, bps=bps, details=True)
        for p in range(npkt):
            cond = _replay(shape, mu, noise, 0, p)[5]
            bound = 2.0 * np.maximum(1e-5, 1e-6 * cond ** 2)
            err = np.abs(mu.xeq[0, p].astype(np.complex128) - su.xeq[p]) / np.maximum(1.0, np.abs(su.xeq[p])) / bound
            assert err.max() <= 1.0, (p, err.max())
        if not noise.any():
            assert np.array_equal(mu.bits[0], su.bits) and (mu.bit_errors == 0).all() and (su.bit_errors == 0).all()
    print('xeq of the two kernels agree; identical bits without noise')


# ------------------------------------------------------------------------------------------------ g: streams
def test_g_noise_and_bit_streams_of_the_users(pkg, oracle):
    """ns = 1: y = x G_uu, so the realised noise is x G_uu - clean.  Bound per sample: the fp32 chain y (M + 1 terms), z, x and the product
    back, 8 (M + 4) 2^-24 (sum_m |G_m| |d_m| + |w|), plus 1e-5 of the noise deviation for the fp32 logf / cosf of the draw
    (tests/test_gpu_link.py test_g: below 1e-6 of a deviate).  Users 0 and U - 1; at 30 dB their decoded bits are the host's bits."""
    shape = (8, 2, 4, 1, 2, 3, 5)
    nt, nr, nu, ns, bps, n_sym, npkt = shape
    e, h, hest, W, ref, nv, dev = _run(pkg, oracle, shape, snr_db=30.0)
    n_info = L.frame_bits(ns, n_sym, bps)[0]
    worst = 0.0
    for u in (0, nu - 1):
        for p in range(npkt):
            G, clean, w, x, csi, cond = _replay(shape, dev, nv, u, p)
            guu = G[:, 0, u]                                                             # [234]
            got = dev.xeq[u, p, 0].astype(np.complex128) * guu[None, :] - clean[:, :, 0]
            d_abs = np.abs(np.concatenate([MU.user_symbols(SEED, FIRST + p, v, ns, n_sym, bps)[2] for v in range(nu)], 0))  # [M, n, k]
            mag = np.einsum('km,mnk->nk', np.abs(G[:, 0, :]), d_abs) + np.abs(w[:, :, 0])
            tol = 8.0 * (nu * ns + 4) * 2.0 ** -24 * mag + 1e-5 * np.sqrt(float(nv[u, p]) / 2.0)
            worst = max(worst, float((np.abs(got - w[:, :, 0]) / tol).max()))
            assert np.array_equal(dev.bits[u, p], L.info_bits(MU.user_seed(SEED, u), FIRST + p, n_info)) and dev.bit_errors[u, p] == 0
    print('realised noise of users 0 and %d: largest deviation from the host replay / bound %.4f' % (nu - 1, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ h: bit for bit
def _device_inputs(e, h, W, nv):
    return ([e.to_device(np.ascontiguousarray(x.real, np.float32)) for x in h], [e.to_device(np.ascontiguousarray(x.imag, np.float32)) for x in h],
            e.to_device(np.ascontiguousarray(W.real, np.float32)), e.to_device(np.ascontiguousarray(W.imag, np.float32)),
            e.to_device(np.ascontiguousarray(nv, np.float32)))


def _device_call(e, ins, shape, first, npkt, with_llr=True):
    nt, nr, nu, ns, bps, n_sym, _ = shape
    n_info, n_coded = L.frame_bits(ns, n_sym, bps)
    m = nu * ns
    outs = [e.empty((nu, npkt)) for _ in range(3)] + [e.empty((nu, npkt, ns, m, L.N)) for _ in range(2)] + \
           [e.empty((nu, npkt, ns, n_sym, L.N)) for _ in range(2)] + [e.empty((nu, npkt, ns, L.N)), e.empty((nu, npkt, n_coded)),
                                                                      e.empty(((nu * npkt * n_info + 3) // 4,))]
    e.mu_link_sim_device(ins[0], ins[1], ins[2], ins[3], ins[4], SEED, first, npkt, ns, *outs[:3], n_sym=n_sym, bps=bps, d_g_re=outs[3],
                         d_g_im=outs[4], d_xeq_re=outs[5], d_xeq_im=outs[6], d_csi=outs[7], d_llr=outs[8] if with_llr else None, d_bits=outs[9])
    e.synchronize()
    res = [o.download().view(np.uint32) for o in outs[:9]] + [outs[9].download().view(np.uint8)[:nu * npkt * n_info].reshape(nu, npkt, n_info)]
    for o in outs:
        o.free()
    return res


def test_h_repeats_chunks_and_packet_ranges_bit_for_bit(pkg, oracle):
    shape = (8, 2, 4, 1, 2, 3, 5)
    nt, nr, nu, ns, bps, n_sym, npkt = shape
    e = _engine(pkg, oracle, nt, nr)
    h = _channels(shape)
    rng = np.random.default_rng(9)
    hest = [_f32(x + 0.2 * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))) for x in h]
    W = e.mu_precoder(hest, ns)
    assert np.array_equal(W.view(np.uint32), e.mu_precoder(hest, ns).view(np.uint32))     # the precoder repeats
    for p0, p1 in ((0, 2), (2, 5)):                                                       # ... and a packet does not depend on its call
        assert np.array_equal(W[p0:p1].view(np.uint32), e.mu_precoder([x[p0:p1] for x in hest], ns).view(np.uint32))
    nv = _noise_var(h, W.astype(np.complex128), ns, 2.0)
    ins = _device_inputs(e, h, W, nv)
    full = _device_call(e, ins, shape, FIRST, npkt)
    assert full[0].view(np.int32).sum() > 0                                               # 2 dB with interference: there are bit errors to repeat
    again = _device_call(e, ins, shape, FIRST, npkt)
    assert all(np.array_equal(a, b) for a, b in zip(full, again))
    # two calls over packet ranges
    for p0, p1 in ((0, 2), (2, 5)):
        part_in = _device_inputs(e, [x[p0:p1] for x in h], W[p0:p1], nv[:, p0:p1])
        part = _device_call(e, part_in, shape, FIRST + p0, p1 - p0)
        for f, q in zip(full, part):
            assert np.array_equal(f[:, p0:p1], q)
    # a workspace of one packet's bytes: five chunks, with and without the caller's llr array
    small = _engine(pkg, oracle, nt, nr, workspace_bytes=1024)
    s_in = _device_inputs(small, h, W, nv)
    n0 = small.get_option('mu_launches')
    chunked = _device_call(small, s_in, shape, FIRST, npkt)
    assert small.get_option('mu_launches') == n0 + npkt * (2 * nu + 1)
    assert all(np.array_equal(a, b) for a, b in zip(full, chunked))
    no_llr = _device_call(small, s_in, shape, FIRST, npkt, with_llr=False)
    assert all(np.array_equal(a, b) for i, (a, b) in enumerate(zip(full, no_llr)) if i != 8)
    # a bf16 context is served with the same bits
    b = _engine(pkg, oracle, nt, nr, dtype='bf16')
    assert np.array_equal(W.view(np.uint32), b.mu_precoder(hest, ns).view(np.uint32))
    assert all(np.array_equal(x, y) for x, y in zip(full, _device_call(b, _device_inputs(b, h, W, nv), shape, FIRST, npkt)))


# ------------------------------------------------------------------------------------------------ i: mismatch shows
def test_i_estimation_error_becomes_interference(pkg, oracle):
    """estimates = truth + CN(0, mean |h|^2 / Nt): the LS error level of a sounding phase at 0 dB (an LS link averages Nt bins)"""
    shape = (8, 2, 4, 1, 2, 3, 5)
    nt, nr, nu, ns, bps, n_sym, npkt = shape
    perfect = _run(pkg, oracle, shape)
    h = perfect[1]
    err = float(np.mean([np.abs(x) ** 2 for x in h])) / nt
    e, h, hest, W, ref, nv, dev = _run(pkg, oracle, shape, est_err=err)
    assert _precoder_ratio(W, ref) <= 1.0
    good = e.mu_link_sim(h, perfect[3], nv, seed=SEED, first_pkt=FIRST, ns=ns, n_sym=n_sym, bps=bps)
    for u in range(nu):
        for p in range(npkt):
            G = dev.g[u, p].astype(np.complex128).transpose(2, 0, 1)
            assert abs(float(dev.sinr_db[u, p]) - MU.sinr_db(G, u, ns, nv[u, p])) <= 0.01
            full = MU.sinr_db(MU.effective_channel(h[u][p], ref[p][0], ns), u, ns, nv[u, p])          # the whole chain in fp64
            assert abs(float(dev.sinr_db[u, p]) - full) <= 0.01
    print('sinr_db with estimates %s, with perfect CSI %s' % (np.round(dev.sinr_db.mean(1).astype(np.float64), 2).tolist(), np.round(good.sinr_db.mean(1).astype(np.float64), 2).tolist()))
    assert (dev.sinr_db < good.sinr_db).all()


# ------------------------------------------------------------------------------------------------ j: degenerate inputs
def test_j_degenerate_inputs(pkg, oracle):
    """Two users with identical estimated rows: entries in {+-1, +-j} at Nt = 4, so that A = [[4, 4], [4, 4]], L = [[2, 0], [2, 0]] and the
    second pivot 4 - 4 are exact in fp32 - the rule is a pivot <= 0, and only an exact zero is certain to meet it."""
    nt, nr, nu, ns, n_sym, bps, npkt = 4, 2, 2, 1, 1, 2, 2
    e = _engine(pkg, oracle, nt, nr)
    shape = (nt, nr, nu, ns, bps, n_sym, npkt)
    h = _channels(shape)
    rng = np.random.default_rng(1)
    hest = [x.copy() for x in h]
    same = np.array([1, 1j, -1, -1j])[rng.integers(0, 4, (nt, 60))]
    for x in hest:
        x[1, 0, :, 40:100] = same                                                         # packet 1, subcarriers 40 .. 99
    W = e.mu_precoder(hest, ns).astype(np.complex128)
    assert (W[1, :, :, 40:100] == 0).all()
    keep = np.r_[0:40, 100:L.N]
    ref = MU.precoder([x[1] for x in hest], ns, 0.0)
    assert (ref[0][:, :, 40:100] == 0).all()
    assert _precoder_ratio(W[:1], [MU.precoder([x[0] for x in hest], ns, 0.0)]) <= 1.0
    err = np.sqrt((np.abs(W[1] - ref[0]) ** 2).sum((0, 1))[keep] / (np.abs(ref[0]) ** 2).sum((0, 1))[keep])
    assert (err / np.maximum(1e-5, 1e-6 * ref[1][keep] ** 2)).max() <= 1.0
    dev = e.mu_link_sim(h, W, 0.01, seed=1, first_pkt=0, ns=ns, n_sym=n_sym, bps=bps, details=True)
    assert (dev.xeq[:, 1, :, :, 40:100] == 0).all() and (dev.csi[:, 1, :, 40:100] == 0).all() and (dev.g[:, 1, :, :, 40:100] == 0).all()
    assert (dev.llr.reshape(nu, npkt, ns, n_sym, L.N, bps)[:, 1, :, :, 40:100] == 0).all()
    for a in (dev.evm_rms, dev.sinr_db, dev.xeq.real, dev.xeq.imag, dev.csi, dev.llr):
        assert np.isfinite(a).all()
    assert (dev.csi[:, 0] > 0).all()
    # the same with reg > 0: finite W within (a)
    Wr = e.mu_precoder(hest, ns, reg=0.25).astype(np.complex128)
    refr = [MU.precoder([x[p] for x in hest], ns, 0.25) for p in range(npkt)]
    worst = 0.0
    for p in range(npkt):
        cond_a = np.array([np.linalg.cond(b @ np.conj(b).T + 0.25 * np.eye(2)) for b in MU.stack_rows([x[p] for x in hest], ns)])
        errp = np.sqrt((np.abs(Wr[p] - refr[p][0]) ** 2).sum((0, 1)) / (np.abs(refr[p][0]) ** 2).sum((0, 1)))
        worst = max(worst, float((errp / np.maximum(1e-5, 1e-6 * cond_a)).max()))     # cond(A) stands for cond(B)^2: B itself is singular
    assert np.isfinite(Wr).all() and (np.abs(Wr).sum((1, 2)) > 0).all() and worst <= 1.0
    # an all-zero channel: W = 0, and with W = 0 nothing is received
    zero = [np.zeros_like(x) for x in h]
    assert (e.mu_precoder(zero, ns) == 0).all()
    dz = e.mu_link_sim(h, np.zeros_like(W), 0.01, seed=1, first_pkt=0, ns=ns, n_sym=n_sym, bps=bps, details=True)
    assert (dz.xeq == 0).all() and (dz.csi == 0).all() and (dz.llr == 0).all() and (dz.evm_rms > 0).all()
    assert np.isneginf(dz.sinr_db).all()                                                  # 0 / (0 + 234 ns noise_var)


# ------------------------------------------------------------------------------------------------ k: refusals
def test_k_refusals_carry_text_and_launch_nothing(pkg, oracle):
    """every refusal of the header; the LDS refusal cannot be reached through the interface (M <= 16 and ns <= 4 keep both images inside
    160 KiB: 80 KiB and 131 KiB at the caps) and stays as a guard for a later change of the caps"""
    import ctypes
    nt, nr = 8, 2
    e = _engine(pkg, oracle, nt, nr)
    lib, ctx = e._lib, e._ctx
    buf = e.empty((1 << 16,))
    p = buf.ptr
    n0 = e.get_option('mu_launches')

    def arr(n, null=None, off=None):
        return (ctypes.c_void_p * max(n, 8))(*[None if i == null else (p + 4 if i == off else p) for i in range(n)] + [None] * (8 - n))

    def pre(text, nu=2, re=None, im=None, npkt=1, ns=1, reg=None, w=(p, p)):
        assert lib.csi_mu_precoder_device(ctx, nu, arr(nu) if re is None else re, arr(nu) if im is None else im, npkt, ns, reg, *w) == -1
        assert text in lib.csi_last_error(ctx).decode(), lib.csi_last_error(ctx)

    def link(text, nu=2, re=None, im=None, w=(p, p), nv=p, first=0, npkt=1, ns=1, n_sym=1, bps=2, req=(p, p, p), opt=(None,) * 7):
        assert lib.csi_mu_link_sim_device(ctx, nu, arr(nu) if re is None else re, arr(nu) if im is None else im, *w, nv, 1, first, npkt, ns, n_sym, bps,
                                          *req, *opt) == -1
        assert text in lib.csi_last_error(ctx).decode(), lib.csi_last_error(ctx)

    for f in (pre, link):
        f('n_users 0 outside 1 .. 8', nu=0)
        f('n_users 9 outside 1 .. 8', nu=9)
        f('ns 0 outside 1 .. min(4, Nr 2)', ns=0)
        f('ns 3 outside 1 .. min(4, Nr 2)', ns=3)
        f('= 10 streams exceed min(16, Nt 8)', nu=5, ns=2)
        f('must not be negative', npkt=-1)
        f('null required pointer (d_h', re=arr(2, null=1))
        f('null required pointer (d_h', im=arr(2, null=0))
        f('must start on a 16-byte boundary', re=arr(2, off=1))
        f('must start on a 16-byte boundary', w=(p + 4, p))
        f('must start on a 16-byte boundary', w=(p, p + 8))
    pre('null required pointer', w=(None, p))
    pre('null required pointer', w=(p, None))
    pre('null required pointer (d_hest_re)', re=ctypes.cast(None, ctypes.POINTER(ctypes.c_void_p)))
    link('must not be negative', first=-1)
    link('bps 3 is not 2', bps=3)
    link('bps 6 is not 2', bps=6)
    link('n_sym 0 must be at least 1', n_sym=0)
    link('n_steps 8268 = ns 1 x n_sym 53 x 234 x bps 2 / 3 exceeds 8190', n_sym=53)
    link('null required pointer', w=(None, p))
    link('null required pointer', nv=None)
    for i in range(3):
        link('null required pointer', req=tuple(None if j == i else p for j in range(3)))
    link('the g planes come as a pair', opt=(p, None) + (None,) * 5)
    link('the xeq planes come as a pair', opt=(None, None, None, p) + (None,) * 3)
    link('must start on a 16-byte boundary', opt=(p + 4, p) + (None,) * 5)
    link('must start on a 16-byte boundary', opt=(None, None, p, p + 4) + (None,) * 3)
    big = _engine(pkg, oracle, 32, 4)
    assert big._lib.csi_mu_precoder_device(big._ctx, 5, arr(5), arr(5), 1, 4, None, p, p) == -1          # M = 20 > 16
    assert '= 20 streams exceed min(16, Nt 32)' in big._lib.csi_last_error(big._ctx).decode()
    one = pkg.CsiEngine(0, 1, hidden=(16,), len_ltf=64)
    assert one._lib.csi_mu_precoder_device(one._ctx, 1, arr(1), arr(1), 1, 1, None, p, p) == -1
    assert 'single-input context' in one._lib.csi_last_error(one._ctx).decode()
    assert one._lib.csi_mu_link_sim_device(one._ctx, 1, arr(1), arr(1), p, p, p, 1, 0, 1, 1, 1, 2, p, p, p, *[None] * 7) == -1
    assert 'single-input context' in one._lib.csi_last_error(one._ctx).decode()
    # nothing to do
    assert lib.csi_mu_precoder_device(ctx, 2, None, None, 0, 1, None, None, None) == 0
    assert lib.csi_mu_link_sim_device(ctx, 2, None, None, None, None, None, 1, 0, 0, 1, 1, 2, *[None] * 10) == 0
    e.synchronize()
    assert e.get_option('mu_launches') == n0
    buf.free()


# ------------------------------------------------------------------------------------------------ l: memory contract
def test_l_guard_bands_of_both_entry_points(pkg, oracle):
    """every input and output a slice between guard bands: nothing outside the arrays is written or reaches a result, inputs are not
    modified, every output element is written, and the results are those of plain arrays"""
    shape = (8, 2, 4, 1, 2, 3, 5)
    nt, nr, nu, ns, bps, n_sym, npkt = shape
    m = nu * ns
    n_info, n_coded = L.frame_bits(ns, n_sym, bps)
    e = _engine(pkg, oracle, nt, nr)
    h = _channels(shape)
    plain_w = e.mu_precoder(h, ns, reg=0.1)
    gin = [Guarded(e, x.shape, 'in', np.ascontiguousarray(part, np.float32), 'h%d' % i) for i, x in enumerate(h) for part in (x.real, x.imag)]
    g_reg = Guarded(e, (npkt,), 'in', np.full(npkt, 0.1, np.float32), 'reg')
    g_w = [Guarded(e, (npkt, m, nt, L.N), 'out', name='w_' + z) for z in ('re', 'im')]
    e.mu_precoder_device(gin[0::2], gin[1::2], npkt, ns, g_w[0], g_w[1], g_reg)
    e.synchronize()
    for a in gin + [g_reg] + g_w:
        a.check()
    assert all(a.unchanged() for a in gin + [g_reg]) and all(a.count_unwritten() == 0 for a in g_w)
    assert np.array_equal(g_w[0].download().view(np.uint32), np.ascontiguousarray(plain_w.real).view(np.uint32))
    assert np.array_equal(g_w[1].download().view(np.uint32), np.ascontiguousarray(plain_w.imag).view(np.uint32))
    # the data phase reads the guarded W it just wrote
    nv = _noise_var(h, plain_w.astype(np.complex128), ns, 8.0)
    plain = e.mu_link_sim(h, plain_w, nv, seed=SEED, first_pkt=FIRST, ns=ns, n_sym=n_sym, bps=bps, details=True)
    for a in g_w:
        a.fill, a.sent = 'out', a.download()
    g_nv = Guarded(e, (nu, npkt), 'in', nv, 'noise_var')
    shapes = [(nu, npkt)] * 3 + [(nu, npkt, ns, m, L.N)] * 2 + [(nu, npkt, ns, n_sym, L.N)] * 2 + [(nu, npkt, ns, L.N), (nu, npkt, n_coded),
                                                                                                   ((nu * npkt * n_info + 3) // 4,)]
    names = ['bit_errors', 'evm_rms', 'sinr_db', 'g_re', 'g_im', 'xeq_re', 'xeq_im', 'csi', 'llr', 'bits']
    outs = [Guarded(e, s, 'out', name=n) for s, n in zip(shapes, names)]
    e.mu_link_sim_device(gin[0::2], gin[1::2], g_w[0], g_w[1], g_nv, SEED, FIRST, npkt, ns, *outs[:3], n_sym=n_sym, bps=bps, d_g_re=outs[3],
                         d_g_im=outs[4], d_xeq_re=outs[5], d_xeq_im=outs[6], d_csi=outs[7], d_llr=outs[8], d_bits=outs[9])
    e.synchronize()
    for a in gin + g_w + [g_nv] + outs:
        a.check()
    assert all(a.unchanged() for a in gin + g_w + [g_nv])
    assert all(a.count_unwritten() == 0 for a in outs[:9])
    got = [a.download() for a in outs]
    assert np.array_equal(got[0].view(np.int32), plain.bit_errors)
    assert np.array_equal(got[1], plain.evm_rms) and np.array_equal(got[2], plain.sinr_db)
    assert np.array_equal(got[3], plain.g.real) and np.array_equal(got[5], plain.xeq.real) and np.array_equal(got[7], plain.csi)
    assert np.array_equal(got[8], plain.llr)
    assert np.array_equal(got[9].view(np.uint8)[:nu * npkt * n_info].reshape(nu, npkt, n_info), plain.bits)
    for a in gin + g_w + [g_reg, g_nv] + outs:
        a.free()


# ------------------------------------------------------------------------------------------------ m: sweep
def test_m_sweep_with_two_users(pkg, oracle, tmp_path):
    from scipy.io import loadmat
    import json
    from dl_channel_estimation_mamimo_amd import sweep
    out = str(tmp_path / 'mu')
    common = ['--nTX', '4', '--nRX', '2', '--nn', '16', '--trainPkts', '24', '--testPkts', '6', '--snr', '0', '20', '--epochs', '1',
              '--bs', '16', '--quiet', '--ber', '--numSTS', '1', '--rays', '32', '--dataSymbols', '2']
    assert sweep.main(['-d', out] + common + ['--users', '2']) == 0
    old = [f + x for f in ('MSE_', 'bers_', 'EVM_rms_', 'dtSNR_') for x in ('LS', 'MMSE', 'DNN', 'perfect')]
    new = [f + x for f in sweep.MU_FIELDS for x in sweep.SOURCES]
    n_info = L.frame_bits(1, 2, 2)[0]
    out2 = str(tmp_path / 'plain')
    assert sweep.main(['-d', out2, '--modeldir', out] + common) == 0
    res, res2 = json.load(open(os.path.join(out, 'sweep.json'))), json.load(open(os.path.join(out2, 'sweep.json')))
    assert res['mu'] == dict(users=2, reg='zf', spacing=15.0) and 'mu' not in res2
    for i, snr in enumerate((0, 20)):
        m = loadmat(os.path.join(out, 'BS4_SNR%g' % snr, 'metrics.mat'))
        m2 = loadmat(os.path.join(out2, 'BS4_SNR%g' % snr, 'metrics.mat'))
        assert sorted(k for k in m if not k.startswith('__')) == sorted(old + new)
        assert sorted(k for k in m2 if not k.startswith('__')) == sorted(old)               # without --users: the parent's field list
        written = sweep.metric_fields({k: m[k] for k in m if not k.startswith('__')})
        assert written[:len(old)] == sweep.metric_fields({k: m2[k] for k in old}) and written[len(old):] == [f + x for x in sweep.SOURCES for f in sweep.MU_FIELDS]
        for k in old:
            assert np.array_equal(m[k], m2[k]), k                                         # user 0 keeps its bits
        for k in new:
            assert m[k].shape == (1, 6) and np.isfinite(m[k]).all(), k
        lv = res['levels'][i]
        for x in sweep.SOURCES:
            per = lv['mu_users'][x]
            assert np.asarray(per['bers']).shape == (2, 6)
            assert np.allclose(np.mean(per['bers'], 0), m['bersMU_' + x][0]) and np.allclose(np.mean(per['sinr'], 0), m['sinrMU_' + x][0])
            errs = np.asarray(per['bers']) * n_info
            assert np.abs(errs - np.rint(errs)).max() < 1e-9
        assert set(res2['levels'][i]) == set(lv) - {f + x for f in sweep.MU_FIELDS for x in sweep.SOURCES} - {'mu_users'}
        print('snr %g dB: two-user BER %s, SINR %s dB' % (snr, {x: float(m['bersMU_' + x].mean()) for x in sweep.SOURCES},
                                                          {x: round(float(m['sinrMU_' + x].mean()), 2) for x in sweep.SOURCES}))
        if snr == 20:
            assert (m['bersMU_perfect'] == 0).all() and m['sinrMU_perfect'].mean() > m['sinrMU_LS'].mean()
