"""GPU tests of the multi-user hybrid precoder (csi_mu_hybrid_precoder_device, csrc/mu_hybrid.hip.h) against the host
restatement tests/mu_hybrid_ref.py.

Inputs: per user a seeded single-bounce scattering channel (synth.scattering_channel: the users sit at different azimuths, so the beam
scores have structure) on the 234 data carriers, rounded to fp32; the dictionary is the sweep's (steering_ula of random rays; random
phases for the largest one), as the engine holds it after its rounding to fp32.  Scores are judged against fp64 with the error of the same statement in numpy complex64 as
the yardstick, indices against the fp64 selection with a margin rule, W and Fbb against the fp64 baseband stage run with the DEVICE's
indices - so every packet is compared whatever a near tie did to the selection."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import link_ref as L          # noqa: E402
import mu_link_ref as MU      # noqa: E402
import mu_hybrid_ref as MH    # noqa: E402
from guarded import Guarded   # noqa: E402

N = L.N
# (Nt, Nr, U, ns, n_rf, R, npkt)
CASES = [(8, 2, 2, 1, 2, 16, 3),        # smallest
         (12, 2, 3, 1, 5, 33, 2),       # no power of two, ray tail of 1
         (32, 4, 4, 2, 12, 500, 5),     # the reference's ray count
         (32, 2, 8, 2, 16, 64, 2),      # M = n_rf = 16, the LDS limit (the 32-lane baseband kernel)
         (8, 2, 1, 1, 1, 4096, 1)]      # the largest dictionary
FIVE = CASES[2]
MARGIN = 1e-4
_cache = {}
_engines = {}
_inputs = {}


def _f32(a):
    """what the library receives: fp32 planes, as complex128"""
    a = np.asarray(a)
    return a.real.astype(np.float32).astype(np.float64) + 1j * a.imag.astype(np.float32).astype(np.float64)


def dictionary(nt, rays):
    """the sweep's dictionary: array responses of random rays.  4096 of them at Nt = 8 lie so densely that the best two differ by 1e-5 of
    their score for any channel: the largest dictionary holds columns of independent random phases instead (columns are used as given)"""
    from dl_channel_estimation_mamimo_amd import synth
    rng = np.random.default_rng(100 * nt + rays)
    if rays > 1024:
        return np.exp(2j * np.pi * rng.random((nt, rays)))
    az, el = synth.random_rays(rng, rays)
    return synth.steering_ula(nt, az, el)


def channels(case):
    """U arrays [npkt, nr, nt, 234]: user u at azimuth -50 + 100 (u + 1/2) / U degrees, 12 scatterers per packet, unit mean power"""
    if case not in _inputs:
        from dl_channel_estimation_mamimo_amd import synth
        from oracle import csi_oracle
        nt, nr, nu, ns, n_rf, rays, npkt = case
        rng = np.random.default_rng(7 + 1000 * nt + 10 * nu + rays)
        bins = np.asarray(csi_oracle.data_carrier_indices()) - 1
        out = []
        for u in range(nu):
            h = np.empty((npkt, nr, nt, N), np.complex128)
            for p in range(npkt):
                g = (rng.standard_normal(12) + 1j * rng.standard_normal(12)) / np.sqrt(2.0)
                H, _ = synth.scattering_channel(rng.random((12, 3)), g, 100.0, -50.0 + 100.0 * (u + 0.5) / nu, 0.0, nr, nt)
                h[p] = np.fft.fftshift(H, axes=-1)[..., bins]
            out.append(_f32(h))
        _inputs[case] = out
    return _inputs[case]


def _engine(pkg, oracle, nt, nr, rays, **kw):
    key = (nt, nr, rays) + tuple(sorted(kw.items()))
    if key not in _engines:
        e = pkg.CsiEngine(nt, nr, hidden=(8,), device=0, **kw)
        e.set_dictionary(dictionary(nt, rays))
        _engines[key] = e
    return _engines[key]


def _reg(case):
    return (0.05 + 0.1 * np.arange(case[6])).astype(np.float32)


def _run(pkg, oracle, case, with_reg):
    """one device call with every output kept and the fp64 scores per (case, reg), shared by the tests that read them"""
    key = (case, with_reg)
    if key not in _cache:
        nt, nr, nu, ns, n_rf, rays, npkt = case
        e = _engine(pkg, oracle, nt, nr, rays)
        h = channels(case)
        reg = _reg(case) if with_reg else None
        w_re, w_im, idx, fbb, score = e.mu_hybrid_precoder(h, ns, n_rf, reg=reg, keep_fbb=True, keep_score=True)
        At = e.dictionary.astype(np.complex128)
        S64 = np.stack([MH.scores([x[p] for x in h], ns, At) for p in range(npkt)])
        _cache[key] = dict(e=e, h=h, reg=reg, W=w_re.astype(np.float64) + 1j * w_im, w_re=w_re, w_im=w_im, idx=idx, fbb=fbb, score=score, At=At, S64=S64)
    return _cache[key]


# ------------------------------------------------------------------------------------------------ a: scores
@pytest.mark.parametrize('case', CASES)
def test_a_scores_against_fp64(pkg, oracle, case):
    """per row (packet, stream): max_r |S - S64| / max_r S64.  Yardstick: the same statement in numpy complex64 / float32 on the same input;
    the device gets 4 x that (another summation order, another grouping inside the fp32 MFMA)"""
    r = _run(pkg, oracle, case, False)
    nt, nr, nu, ns, n_rf, rays, npkt = case
    S32 = np.stack([MH.scores([x[p] for x in r['h']], ns, r['At'], np.complex64) for p in range(npkt)])
    assert S32.dtype == np.float32 and r['score'].shape == r['S64'].shape == (npkt, nu * ns, rays)
    top = r['S64'].max(-1)
    yard = float((np.abs(S32 - r['S64']).max(-1) / top).max())
    dev = float((np.abs(r['score'] - r['S64']).max(-1) / top).max())
    print('%s: score error relative to the row maximum: device %.3e, numpy complex64 %.3e' % (case, dev, yard))
    assert np.isfinite(r['score']).all() and dev <= 4.0 * yard
    assert np.array_equal(r['score'], _run(pkg, oracle, case, True)['score'])            # reg does not enter the scores


# ------------------------------------------------------------------------------------------------ b: indices
@pytest.mark.parametrize('case', CASES)
def test_b_indices_against_the_fp64_selection(pkg, oracle, case):
    """slot by slot among the rays the device has left free: the fp64 choice wherever it leads its runner-up by more than 1e-4 relative,
    one of the two otherwise.  The inputs leave the fp64 selection alone at most 10 % of its (packet, slot) pairs under that margin."""
    r = _run(pkg, oracle, case, False)
    nt, nr, nu, ns, n_rf, rays, npkt = case
    M = nu * ns
    close = sum(m <= MARGIN for p in range(npkt) for m, _ in MH.margins(r['S64'][p], MH.select(r['S64'][p], n_rf)))
    assert close <= 0.10 * npkt * n_rf, close
    tight = 0
    for p in range(npkt):
        S = r['S64'][p]
        dev = r['idx'][p]
        assert len(set(dev.tolist())) == n_rf and dev.min() >= 0 and dev.max() < rays
        for q in range(n_rf):
            row = S[q % M].copy()
            row[dev[:q]] = -np.inf
            best = int(np.argmax(row))
            top = row[best]
            row[best] = -np.inf
            second = int(np.argmax(row)) if rays > q + 1 else best
            if rays > q + 1 and (top - row[second]) <= MARGIN * top:
                tight += 1
                assert dev[q] in (best, second), (p, q, dev[q], best, second)
            else:
                assert dev[q] == best, (p, q, dev[q], best)
    print('%s: %d of %d (packet, slot) pairs of the fp64 selection under the margin, %d met on the device\'s path' % (case, close, npkt * n_rf, tight))
    assert np.array_equal(r['idx'], _run(pkg, oracle, case, True)['idx'])


# ------------------------------------------------------------------------------------------------ c: W and Fbb
def _baseband_ratio(r, case):
    """largest per-item max |W - Wref| / max |Wref| (and the same for Fbb) over max(1e-5, 1e-6 cond(G)^2), the reference run with the device's idx"""
    nt, nr, nu, ns, n_rf, rays, npkt = case
    worst, conds = 0.0, []
    for p in range(npkt):
        Wr, Fr, cond = MH.baseband([x[p] for x in r['h']], ns, r['At'], r['idx'][p], 0.0 if r['reg'] is None else float(r['reg'][p]))
        assert np.isfinite(cond).all() and (np.abs(Wr).max((0, 1)) > 0).all()
        bound = np.maximum(1e-5, 1e-6 * cond ** 2)
        ew = np.abs(r['W'][p] - Wr).max((0, 1)) / np.abs(Wr).max((0, 1))
        ef = np.abs(r['fbb'][p].astype(np.complex128) - Fr).max((1, 2)) / np.abs(Fr).max((1, 2))
        worst = max(worst, float((ew / bound).max()), float((ef / bound).max()))
        conds.append(cond)
    return worst, np.stack(conds)


@pytest.mark.parametrize('with_reg', [False, True])
@pytest.mark.parametrize('case', CASES)
def test_c_baseband_against_fp64_with_the_device_indices(pkg, oracle, case, with_reg):
    r = _run(pkg, oracle, case, with_reg)
    nt, nr, nu, ns, n_rf, rays, npkt = case
    worst, cond = _baseband_ratio(r, case)
    print('%s reg %s: cond(G) up to %.3g, largest W / Fbb error over the bound %.4f (digital precoder: 0.036)' % (case, with_reg, cond.max(), worst))
    assert worst <= 1.0
    W = r['W']
    # |W|_F^2 = Nt per item; where cond(G)^2 passes the fp32 range (1e-6 cond^2 >= 1: the bound above allows any W) a pivot may come out <= 0: W = 0
    pw = (np.abs(W) ** 2).sum((1, 2))
    assert ((np.abs(pw - nt) <= 1e-5 * nt) | ((pw == 0) & (cond >= 1e3))).all()
    print('    items the singular rule zeroed: %d of %d' % (int((pw == 0).sum()), pw.size))
    Frf = r['At'][:, r['idx']]                                                           # [nt, npkt, n_rf]
    prod = np.einsum('jpq,pkqm->pmjk', Frf, r['fbb'].astype(np.complex128))
    mag = np.einsum('jpq,pkqm->pmjk', np.abs(Frf), np.abs(r['fbb']).astype(np.float64))
    ok = mag > 0
    assert (np.abs(prod - W)[ok] <= 4.0 * (n_rf + 2) * 2.0 ** -24 * mag[ok]).all() and (W[~ok] == 0).all()      # W = Frf Fbb, n_rf fp32 terms each


# ------------------------------------------------------------------------------------------------ d: the digital precoder
def test_d_unitary_dictionary_with_all_chains_is_the_digital_precoder(pkg, oracle):
    """the DFT beams, n_rf = Nt = 8, U = 2, ns = 2: G G^H = B B^H, V = B^H A^-1.  Both kernels within their yardsticks of fp64, so within
    the sum of the two of each other; cond(G) = cond(B)"""
    from dl_channel_estimation_mamimo_amd import beamspace
    nt, nr, nu, ns, npkt = 8, 2, 2, 2, 3
    e = pkg.CsiEngine(nt, nr, hidden=(8,), device=0)
    e.set_dictionary(beamspace.dft_basis(nt))
    rng = np.random.default_rng(21)
    h = [_f32((rng.standard_normal((npkt, nr, nt, N)) + 1j * rng.standard_normal((npkt, nr, nt, N))) / np.sqrt(2.0)) for _ in range(nu)]
    for reg in (None, 0.2):
        w_re, w_im, idx = e.mu_hybrid_precoder(h, ns, nt, reg=reg)
        Wd = e.mu_precoder(h, ns, reg=reg).astype(np.complex128)
        assert all(sorted(i.tolist()) == list(range(nt)) for i in idx)
        worst = 0.0
        for p in range(npkt):
            cond = MU.precoder([x[p] for x in h], ns, 0.0)[1]
            err = np.abs(w_re[p] + 1j * w_im[p] - Wd[p]).max((0, 1)) / np.abs(Wd[p]).max((0, 1))
            worst = max(worst, float((err / (2.0 * np.maximum(1e-5, 1e-6 * cond ** 2))).max()))
        print('reg %s: hybrid with a unitary dictionary against the digital precoder: largest deviation over the two yardsticks %.4f' % (reg, worst))
        assert worst <= 1.0
    e.close()


# ------------------------------------------------------------------------------------------------ e: through the existing link
@pytest.mark.parametrize('case', CASES)
def test_e_through_the_existing_link(pkg, oracle, case):
    """true = estimated planes, reg = 0, noise 60 dB under a stream's mean power: far below any decision distance, far above the
    interference the fp32 rounding of either precoder leaves (cond^2 2^-48), so that sinr_db is sig / noise for both.  B W = diag(c_m) for
    both precoders and the digital c_m is the largest possible (the minimum-norm V): the hybrid sinr_db is not above the digital one."""
    r = _run(pkg, oracle, case, False)
    nt, nr, nu, ns, n_rf, rays, npkt = case
    e, h = r['e'], r['h']
    Wd = e.mu_precoder(h, ns)
    nv = np.float32(1e-6 * nt / (nu * ns) * np.mean([np.abs(x[:, :ns]) ** 2 for x in h]))
    hyb = e.mu_link_sim(h, r['W'].astype(np.complex64), nv, seed=3, first_pkt=1, ns=ns, n_sym=1, bps=2)
    dig = e.mu_link_sim(h, Wd, nv, seed=3, first_pkt=1, ns=ns, n_sym=1, bps=2)
    print('%s: sinr_db hybrid %s, digital %s' % (case, np.round(hyb.sinr_db.astype(np.float64), 2).tolist(), np.round(dig.sinr_db.astype(np.float64), 2).tolist()))
    assert hyb.bit_errors.shape == (nu, npkt) and (hyb.bit_errors == 0).all()
    assert np.isfinite(hyb.sinr_db).all() and (hyb.sinr_db <= dig.sinr_db + 0.01).all()


# ------------------------------------------------------------------------------------------------ f: bit for bit
def _device_call(e, case, h, reg=None, fbb=True, score=True):
    """one csi_mu_hybrid_precoder_device call over fresh DeviceArrays -> the outputs as uint32 words (None where not kept)"""
    nt, nr, nu, ns, n_rf, rays, _ = case
    npkt, m = h[0].shape[0], nu * ns
    ins = [e.to_device(np.ascontiguousarray(x.real, np.float32)) for x in h] + [e.to_device(np.ascontiguousarray(x.imag, np.float32)) for x in h]
    d_reg = e.to_device(np.ascontiguousarray(reg, np.float32)) if reg is not None else None
    outs = [e.empty((npkt, m, nt, N)), e.empty((npkt, m, nt, N)), e.empty((npkt, n_rf))]
    outs += [e.empty((npkt, N, n_rf, m)), e.empty((npkt, N, n_rf, m))] if fbb else [None, None]
    outs += [e.empty((npkt, m, rays))] if score else [None]
    e.mu_hybrid_precoder_device(ins[:nu], ins[nu:], npkt, ns, n_rf, outs[0], outs[1], outs[2], d_reg, outs[3], outs[4], outs[5])
    e.synchronize()
    res = [None if o is None else o.download().view(np.uint32) for o in outs]
    for a in ins + outs + [d_reg]:
        if a is not None:
            a.free()
    return res


def test_f_repeats_packet_ranges_chunks_and_optional_outputs_bit_for_bit(pkg, oracle):
    case = FIVE
    nt, nr, nu, ns, n_rf, rays, npkt = case
    e = _engine(pkg, oracle, nt, nr, rays)
    h, reg = channels(case), _reg(case)
    full = _device_call(e, case, h, reg)
    assert all(np.array_equal(a, b) for a, b in zip(full, _device_call(e, case, h, reg)))               # a repeat call
    part = _device_call(e, case, [x[2:5] for x in h], reg[2:5])                                         # packets 2 .. 4 alone
    assert all(np.array_equal(a[2:5], b) for a, b in zip(full, part))
    for fbb, score in ((False, True), (True, False), (False, False)):                                   # optional outputs kept or not
        got = _device_call(e, case, h, reg, fbb=fbb, score=score)
        assert all(np.array_equal(a, b) for a, b in zip(full, got) if b is not None), (fbb, score)
    # a workspace of less than one packet's score planes: one packet per chunk, three launches each
    small = _engine(pkg, oracle, nt, nr, rays, workspace_bytes=1024)
    n0 = small.get_option('mu_launches')
    got = _device_call(small, case, h, reg, score=False)
    assert small.get_option('mu_launches') == n0 + 3 * npkt
    assert all(np.array_equal(a, b) for a, b in zip(full, got) if b is not None)
    got = _device_call(small, case, h, reg)                                                             # the caller's score array: one chunk
    assert small.get_option('mu_launches') == n0 + 3 * npkt + 3
    assert all(np.array_equal(a, b) for a, b in zip(full, got))
    # a bf16 context is served with the same bits
    b = _engine(pkg, oracle, nt, nr, rays, dtype='bf16')
    assert all(np.array_equal(x, y) for x, y in zip(full, _device_call(b, case, h, reg)))


# ------------------------------------------------------------------------------------------------ g: graph
def test_g_capture_and_replay(pkg, oracle):
    case = CASES[1]
    nt, nr, nu, ns, n_rf, rays, npkt = case
    m = nu * ns
    e = pkg.CsiEngine(nt, nr, hidden=(8,), device=0)
    e.set_dictionary(dictionary(nt, rays))
    h = channels(case)
    ins = [e.to_device(np.ascontiguousarray(x.real, np.float32)) for x in h] + [e.to_device(np.ascontiguousarray(x.imag, np.float32)) for x in h]
    one = [e.to_device(np.ascontiguousarray(x[:1].real, np.float32)) for x in h] + [e.to_device(np.ascontiguousarray(x[:1].imag, np.float32)) for x in h]
    shapes = [(npkt, m, nt, N), (npkt, m, nt, N), (npkt, n_rf), (npkt, N, n_rf, m), (npkt, N, n_rf, m)]
    eager = [e.empty(s) for s in shapes]
    o1 = [e.empty((1,) + s[1:]) for s in shapes]
    # an eager call of ONE packet sizes the workspace for one packet
    e.mu_hybrid_precoder_device(one[:nu], one[nu:], 1, ns, n_rf, *o1[:3], None, *o1[3:])
    e.synchronize()
    n0 = e.get_option('mu_launches')
    e.capture_begin()
    try:
        e.mu_hybrid_precoder_device(one[:nu], one[nu:], 1, ns, n_rf, *o1[:3], None, *o1[3:])
        with pytest.raises(pkg.CsiError, match='sized by an eager call of the same shape'):
            e.mu_hybrid_precoder_device(ins[:nu], ins[nu:], npkt, ns, n_rf, *eager[:3], None, *eager[3:])       # two packets: the workspace would grow
    finally:
        g1 = e.capture_end()
    assert e.get_option('mu_launches') == n0 + 3
    g1.launch()
    e.synchronize()
    g1.free()
    # the context is usable: eager call of the whole shape, capture, replay
    e.mu_hybrid_precoder_device(ins[:nu], ins[nu:], npkt, ns, n_rf, *eager[:3], None, *eager[3:])
    e.synchronize()
    want = [a.download().view(np.uint32) for a in eager]
    replay = [e.to_device(np.zeros(s, np.float32)) for s in shapes]
    e.capture_begin()
    try:
        e.mu_hybrid_precoder_device(ins[:nu], ins[nu:], npkt, ns, n_rf, *replay[:3], None, *replay[3:])
    finally:
        g = e.capture_end()
    assert not any(a.download().any() for a in replay), 'a captured call must not run'
    g.launch()
    e.synchronize()
    assert all(np.array_equal(a.download().view(np.uint32), w) for a, w in zip(replay, want))
    assert all(np.array_equal(a, b) for a, b in zip(want, _device_call(e, case, h, fbb=True, score=False)[:5]))
    g.free()
    for a in ins + one + eager + o1 + replay:
        a.free()
    e.close()


# ------------------------------------------------------------------------------------------------ h: singular items
def test_h_singular_items(pkg, oracle):
    """Two users with identical estimated rows on subcarriers 40 .. 99 of packet 1, entries in {+-1, +-j}, Nt = 4, the four columns of the
    unnormalised DFT matrix as dictionary and n_rf = 4: G holds Gaussian integers with |g|^2 summing to 4 |b|^2 = 16 (Parseval), so
    A = [[16, 16], [16, 16]], L = [[4, 0], [4, .]] and the second pivot 16 - 16 are exact in fp32 - the rule is a pivot <= 0, and only an
    exact zero is certain to meet it."""
    nt, nr, nu, ns, n_rf, npkt = 4, 2, 2, 1, 4, 2
    e = pkg.CsiEngine(nt, nr, hidden=(8,), device=0)
    At = np.array([[1j ** (j * r) for r in range(4)] for j in range(4)])
    e.set_dictionary(At)
    rng = np.random.default_rng(1)
    h = [_f32(rng.standard_normal((npkt, nr, nt, N)) + 1j * rng.standard_normal((npkt, nr, nt, N))) for _ in range(nu)]
    same = np.array([1, 1j, -1, -1j])[rng.integers(0, 4, (nt, 60))]
    for x in h:
        x[1, 0, :, 40:100] = same
    w_re, w_im, idx, fbb, score = e.mu_hybrid_precoder(h, ns, n_rf, keep_fbb=True, keep_score=True)
    W = w_re.astype(np.float64) + 1j * w_im
    assert (W[1, :, :, 40:100] == 0).all() and (fbb[1, 40:100] == 0).all()
    for a in (w_re, w_im, fbb.real, fbb.imag, score):
        assert np.isfinite(a).all()
    keep = np.r_[0:40, 100:N]
    r = dict(h=h, reg=None, W=W, idx=idx, fbb=fbb, At=e.dictionary.astype(np.complex128))
    for p in range(npkt):
        Wr, Fr, cond = MH.baseband([x[p] for x in h], ns, r['At'], idx[p], 0.0)
        k = keep if p == 1 else np.arange(N)
        if p == 1:
            assert (Wr[:, :, 40:100] == 0).all() and (Fr[40:100] == 0).all()
        bound = np.maximum(1e-5, 1e-6 * cond[k] ** 2)
        assert ((np.abs(W[p] - Wr).max((0, 1))[k] / np.abs(Wr).max((0, 1))[k]) / bound).max() <= 1.0
        assert ((np.abs(fbb[p] - Fr).max((1, 2))[k] / np.abs(Fr).max((1, 2))[k]) / bound).max() <= 1.0
    assert (np.abs(W[0]).max((0, 1)) > 0).all()                                           # the other packet is untouched by the rule
    # the same with reg > 0: finite and non-zero everywhere
    w_re, w_im, _ = e.mu_hybrid_precoder(h, ns, n_rf, reg=0.25)
    assert np.isfinite(w_re).all() and np.isfinite(w_im).all() and ((np.abs(w_re) + np.abs(w_im)).sum((1, 2)) > 0).all()
    # an all-zero channel: every score is 0, the lowest rays are taken, W = 0
    z = e.mu_hybrid_precoder([np.zeros_like(x) for x in h], ns, n_rf, keep_fbb=True)
    assert (z[0] == 0).all() and (z[1] == 0).all() and (z[3] == 0).all() and (z[2] == np.arange(n_rf)).all()
    e.close()


# ------------------------------------------------------------------------------------------------ i: memory contract
def test_i_guard_bands(pkg, oracle):
    """every input and output a slice between guard bands: nothing outside the arrays is written or reaches a result, inputs are not
    modified, every output element is written, and the results are those of plain arrays"""
    case = CASES[1]
    nt, nr, nu, ns, n_rf, rays, npkt = case
    m = nu * ns
    r = _run(pkg, oracle, case, True)
    e, h = r['e'], r['h']
    gin = [Guarded(e, x.shape, 'in', np.ascontiguousarray(part, np.float32), 'h%d' % i) for i, x in enumerate(h) for part in (x.real, x.imag)]
    g_reg = Guarded(e, (npkt,), 'in', r['reg'], 'reg')
    shapes = [(npkt, m, nt, N), (npkt, m, nt, N), (npkt, n_rf), (npkt, N, n_rf, m), (npkt, N, n_rf, m), (npkt, m, rays)]
    outs = [Guarded(e, s, 'out', name=n) for s, n in zip(shapes, ('w_re', 'w_im', 'idx', 'fbb_re', 'fbb_im', 'score'))]
    e.mu_hybrid_precoder_device(gin[0::2], gin[1::2], npkt, ns, n_rf, outs[0], outs[1], outs[2], g_reg, outs[3], outs[4], outs[5])
    e.synchronize()
    for a in gin + [g_reg] + outs:
        a.check()
    assert all(a.unchanged() for a in gin + [g_reg]) and all(a.count_unwritten() == 0 for a in outs)
    got = [a.download() for a in outs]
    assert np.array_equal(got[0].view(np.uint32), r['w_re'].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), r['w_im'].view(np.uint32))
    assert np.array_equal(got[2].view(np.int32), r['idx']) and np.array_equal(got[5].view(np.uint32), r['score'].view(np.uint32))
    assert np.array_equal(got[3], r['fbb'].real) and np.array_equal(got[4], r['fbb'].imag)
    # the score planes in the workspace: the same guards around what remains
    keep = [Guarded(e, s, 'out', name=n) for s, n in zip(shapes[:3], ('w_re', 'w_im', 'idx'))]
    e.mu_hybrid_precoder_device(gin[0::2], gin[1::2], npkt, ns, n_rf, keep[0], keep[1], keep[2], g_reg)
    e.synchronize()
    for a in gin + [g_reg] + keep:
        a.check()
    assert all(a.count_unwritten() == 0 for a in keep) and all(np.array_equal(a.download().view(np.uint32), b.view(np.uint32)) for a, b in zip(keep, got))
    for a in gin + [g_reg] + outs + keep:
        a.free()


# ------------------------------------------------------------------------------------------------ j: refusals
def test_j_refusals_carry_text_and_launch_nothing(pkg, oracle):
    """every refusal of the header.  The LDS refusal is met by the score kernel's four dictionary tiles (1 KiB per antenna) from Nt = 161 on;
    the baseband kernel's image stays inside 160 KiB for every M, n_rf <= 16 there and keeps its refusal as a guard"""
    nt, nr, rays = 8, 2, 16
    e = pkg.CsiEngine(nt, nr, hidden=(8,), device=0)
    lib, ctx = e._lib, e._ctx
    buf = e.empty((1 << 16,))
    p = buf.ptr

    def arr(n, null=None, off=None):
        return (ctypes.c_void_p * max(n, 8))(*[None if i == null else (p + 4 if i == off else p) for i in range(n)] + [None] * (8 - n))

    def call(text, nu=2, re=None, im=None, npkt=1, ns=1, n_rf=2, reg=None, w=(p, p), idx=p, fbb=(None, None), score=None, code=-1):
        assert lib.csi_mu_hybrid_precoder_device(ctx, nu, arr(nu) if re is None else re, arr(nu) if im is None else im, npkt, ns, n_rf, reg, *w, idx,
                                                 *fbb, score) == code
        assert text in lib.csi_last_error(ctx).decode(), lib.csi_last_error(ctx)

    call('no dictionary set', code=-2)                                                    # CSI_ERR_NOT_READY
    e.set_dictionary(dictionary(nt, rays))
    n0 = e.get_option('mu_launches')
    call('n_users 0 outside 1 .. 8', nu=0)
    call('n_users 9 outside 1 .. 8', nu=9)
    call('ns 0 outside 1 .. min(4, Nr 2)', ns=0)
    call('ns 3 outside 1 .. min(4, Nr 2)', ns=3)
    call('= 10 streams exceed min(16, Nt 8)', nu=5, ns=2, n_rf=8)
    call('n_rf 1 outside M 2 .. min(16, Nt 8, rays 16)', n_rf=1)
    call('n_rf 9 outside M 2 .. min(16, Nt 8, rays 16)', n_rf=9)
    call('must not be negative', npkt=-1)
    call('null required pointer (d_hest_re[1])', re=arr(2, null=1))
    call('null required pointer (d_hest_im[0])', im=arr(2, null=0))
    call('null required pointer (d_hest_re)', re=ctypes.cast(None, ctypes.POINTER(ctypes.c_void_p)))
    call('must start on a 16-byte boundary', re=arr(2, off=1))
    call('null required pointer', w=(None, p))
    call('null required pointer', w=(p, None))
    call('null required pointer', idx=None)
    call('must start on a 16-byte boundary', w=(p + 4, p))
    call('must start on a 16-byte boundary', w=(p, p + 8))
    call('the fbb planes come as a pair', fbb=(p, None))
    call('the fbb planes come as a pair', fbb=(None, p))
    call('d_fbb_re must start on a 16-byte boundary', fbb=(p + 4, p))
    call('d_fbb_im must start on a 16-byte boundary', fbb=(p, p + 4))
    call('d_score must start on a 16-byte boundary', score=p + 8)
    few = pkg.CsiEngine(nt, nr, hidden=(8,), device=0)
    few.set_dictionary(dictionary(nt, 16)[:, :3])
    assert few._lib.csi_mu_hybrid_precoder_device(few._ctx, 2, arr(2), arr(2), 1, 1, 4, None, p, p, p, None, None, None) == -1
    assert 'n_rf 4 outside M 2 .. min(16, Nt 8, rays 3)' in few._lib.csi_last_error(few._ctx).decode()
    wide = pkg.CsiEngine(192, 2, hidden=(8,), device=0)
    wide.set_dictionary(dictionary(192, 16))
    assert wide._lib.csi_mu_hybrid_precoder_device(wide._ctx, 2, arr(2), arr(2), 1, 1, 2, None, p, p, p, None, None, None) == -1
    assert 'Nt 192 needs 196608 bytes of LDS' in wide._lib.csi_last_error(wide._ctx).decode()
    one = pkg.CsiEngine(0, 1, hidden=(16,), len_ltf=64)
    assert one._lib.csi_mu_hybrid_precoder_device(one._ctx, 1, arr(1), arr(1), 1, 1, 1, None, p, p, p, None, None, None) == -1
    assert 'single-input context' in one._lib.csi_last_error(one._ctx).decode()
    # an open capture that would have to grow the workspace (no eager call yet); a call that keeps its scores needs none and is recorded
    e.capture_begin()
    try:
        assert lib.csi_mu_hybrid_precoder_device(ctx, 2, arr(2), arr(2), 1, 1, 2, None, p, p, p, None, None, p) == 0
        call('sized by an eager call of the same shape')
    finally:
        e.capture_end().free()
    n0 += 3
    # nothing to do
    assert lib.csi_mu_hybrid_precoder_device(ctx, 2, None, None, 0, 1, 2, None, None, None, None, None, None, None) == 0
    e.synchronize()
    assert e.get_option('mu_launches') == n0
    assert few.get_option('mu_launches') == 0 and one.get_option('mu_launches') == 0 and wide.get_option('mu_launches') == 0
    with pytest.raises(pkg.CsiError, match='every h must be'):
        e.mu_hybrid_precoder([np.zeros((1, nr, nt, 7), np.complex64)], 1, 2)
    buf.free()
    for x in (e, few, one, wide):
        x.close()


# ------------------------------------------------------------------------------------------------ k: sweep
def test_k_sweep_miniature(pkg, oracle, tmp_path):
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    out, out2 = str(tmp_path / 'muh'), str(tmp_path / 'mu')
    common = ['--nTX', '8', '--nRX', '2', '--nn', '16', '--trainPkts', '24', '--testPkts', '6', '--snr', '20', '--epochs', '1',
              '--bs', '16', '--quiet', '--ber', '--numSTS', '1', '--rays', '32', '--dataSymbols', '2', '--users', '2']
    assert sweep.main(['-d', out] + common + ['--muHybrid', '4']) == 0
    assert sweep.main(['-d', out2, '--modeldir', out] + common) == 0
    res, res2 = json.load(open(os.path.join(out, 'sweep.json'))), json.load(open(os.path.join(out2, 'sweep.json')))
    assert res['mu_hybrid'] == dict(n_rf=4) and 'mu_hybrid' not in res2 and res['mu'] == res2['mu']
    m = loadmat(os.path.join(out, 'BS8_SNR20', 'metrics.mat'))
    m2 = loadmat(os.path.join(out2, 'BS8_SNR20', 'metrics.mat'))
    new = [f + x for x in sweep.SOURCES for f in sweep.MUH_FIELDS]
    old = sorted(k for k in m2 if not k.startswith('__'))
    assert sorted(k for k in m if not k.startswith('__')) == sorted(old + new)
    written = sweep.metric_fields({k: m[k] for k in m if not k.startswith('__')})
    assert written[:len(old)] == sweep.metric_fields({k: m2[k] for k in old}) and written[len(old):] == new
    for k in old:
        assert np.array_equal(m[k], m2[k]), k                                            # the MU fields (and every other) are unchanged
    for k in new:
        assert m[k].shape == (1, 6) and np.isfinite(m[k]).all(), k
    lv, lv2 = res['levels'][0], res2['levels'][0]
    assert set(lv2) == set(lv) - set(new) - {'muh_users'} and lv['mu_users'] == lv2['mu_users']
    for x in sweep.SOURCES:
        per = lv['muh_users'][x]
        assert np.asarray(per['bers']).shape == (2, 6) and np.asarray(per['beams']).shape == (6, 4)
        assert all(len(set(b)) == 4 and 0 <= min(b) and max(b) < 32 for b in per['beams'])
        assert np.allclose(np.mean(per['bers'], 0), m['bersMUH_' + x][0]) and np.allclose(np.mean(per['sinr'], 0), m['sinrMUH_' + x][0])
    hyb, dig = np.asarray(lv['muh_users']['perfect']['sinr']), np.asarray(lv['mu_users']['perfect']['sinr'])
    print('20 dB, two users: sinr_db perfect CSI digital %s, hybrid (4 chains) %s' % (np.round(dig.mean(1), 2).tolist(), np.round(hyb.mean(1), 2).tolist()))
    assert (hyb <= dig + 0.01).all()
