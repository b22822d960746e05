"""GPU tests (-m gpu) of receive combining (csi_rx_combiner_device, csi_rx_apply_combiner_device, csrc/rx_combine.hip.h)
against the fp64 statement tests/rx_combine_ref.py.

Shapes (Nt, Nr, ns) with 3 packets = 702 items, no multiple of 64: (8, 2, 1) and (8, 4, 2) keep C in registers in the apply kernel,
(16, 16, 4) is the 8-lane LDS image of the combiner and the LDS path of the apply kernel.  One combiner call per shape is shared.

Bounds.  Combiner on planes U S V^H with S = 4, 2, 1, ... : per element 2 x the complex64 restatement's worst error on the same planes +
2^-23; sigma 2^-22 relative.  On i.i.d. planes only invariants: |C C^H - I| <= 8 x 2^-24 Nr, |C H|_F^2 against the fp64 sum of the top ns
sigma^2 to 1e-6.  Against the shipped feedback path: |conj(E[s][j]) - sigma_s d_v[s][j]| <= 2 (Nr + 5) 2^-24 sigma_1 (Nr products, the
rounding of C and of d_v, a factor 2 for the phase).  Apply: per element (Nr + 1) 2^-24 sum_i |C[s][i]| |H[i][j]|."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feedback_ref as R      # noqa: E402
import mu_link_ref as MU      # noqa: E402
import rx_combine_ref as C    # noqa: E402

N = R.N
U24 = 2.0 ** -24
NPKT = 3
SHAPES = [(8, 2, 1), (8, 4, 2), (16, 16, 4)]
IDS = ['nt%d_nr%d_ns%d' % s for s in SHAPES]
_engines, _cache = {}, {}


def _engine(pkg, nt, nr):
    if (nt, nr) not in _engines:
        _engines[(nt, nr)] = pkg.CsiEngine(nt, nr, hidden=(64, 64), device=0)
    return _engines[(nt, nr)]


def _rows(c):
    """device layout [npkt, a, b, 234] -> items [npkt 234, a, b]"""
    return np.ascontiguousarray(c.transpose(0, 3, 1, 2)).reshape(-1, c.shape[1], c.shape[2])


def _run(pkg, shape, kind):
    key = shape + (kind,)
    if key not in _cache:
        nt, nr, ns = shape
        e = _engine(pkg, nt, nr)
        h = C.planes_usv(11 + nt + nr, NPKT, nr, nt) if kind == 'usv' else R.planes(21 + nt + nr, NPKT, nr, nt)
        n0 = e.get_option('combine_launches')
        c, sigma = e.rx_combiner(h, ns, keep_sigma=True)
        assert e.get_option('combine_launches') == n0 + 1
        assert c.shape == (NPKT, ns, nr, N) and sigma.shape == (NPKT, ns, N)
        _cache[key] = dict(e=e, h=h, c=c, sigma=sigma, H=C.items(h).astype(np.complex128))
    return _cache[key]


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_a_combiner_against_fp64(pkg, shape):
    nt, nr, ns = shape
    r = _run(pkg, shape, 'usv')
    Cr, sr = C.combiner(r['H'], ns)
    C32, _ = C.combiner(r['H'], ns, np.float32)
    yard = np.abs(C32.astype(np.complex128) - Cr).max()
    err = np.abs(_rows(r['c']).astype(np.complex128) - Cr).max()
    sd = np.ascontiguousarray(r['sigma'].transpose(0, 2, 1)).reshape(-1, ns).astype(np.float64)
    rel = (np.abs(sd - sr) / sr).max()
    print('%s: |C - C_ref| %.3g, complex64 restatement %.3g, bound %.3g; sigma relative %.3g' % (shape, err, yard, 2 * yard + 2 * U24, rel))
    assert err <= 2.0 * yard + 2.0 ** -23
    assert rel <= 2.0 ** -22


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_b_invariants_on_gaussian_planes(pkg, shape):
    nt, nr, ns = shape
    r = _run(pkg, shape, 'iid')
    Cd = _rows(r['c']).astype(np.complex128)
    orth = np.abs(Cd @ np.conj(Cd.transpose(0, 2, 1)) - np.eye(ns)).max()
    energy = (np.abs(Cd @ r['H']) ** 2).sum((1, 2))
    top = (np.linalg.svd(r['H'], compute_uv=False)[:, :ns] ** 2).sum(1)
    rel = (np.abs(energy - top) / top).max()
    print('%s: |C C^H - I| %.3g (bound %.3g), energy relative %.3g' % (shape, orth, 8 * U24 * nr, rel))
    assert orth <= 8 * U24 * nr
    assert rel <= 1e-6


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_c_singular_items(pkg, shape):
    """packet 0: a zero plane (rank 0); packet 1: rows 0 .. Nr-2 equal, the last one different (rank min(2, Nr)); small integers, so the
    Gram matrices are exact"""
    nt, nr, ns = shape
    e = _engine(pkg, nt, nr)
    rng = np.random.default_rng(5 + nr)
    h = np.zeros((2, nr, nt, N), np.complex64)
    row = rng.integers(-3, 4, (nt, N)) + 1j * rng.integers(-3, 4, (nt, N))
    row[0] += 4                                                 # no zero row by chance
    h[1, :nr - 1] = row
    h[1, nr - 1] = rng.integers(-3, 4, (nt, N)) + 1j * rng.integers(-3, 4, (nt, N)) + 4j
    c, sigma = e.rx_combiner(h, ns, keep_sigma=True)
    assert np.isfinite(c.view(np.float32)).all() and np.isfinite(sigma).all()
    assert not c[0].any() and not sigma[0].any()
    rank = min(2, nr)
    assert (sigma[1, :min(rank, ns)] > 0).all()
    assert not c[1, rank:].any() and not sigma[1, rank:].any()
    ed = e.rx_apply_combiner(c, h)
    assert np.isfinite(ed.view(np.float32)).all() and not ed[0].any()


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_d_cross_check_with_the_feedback_path(pkg, shape):
    nt, nr, ns = shape
    r = _run(pkg, shape, 'iid')
    e = r['e']
    rep = e.feedback_compress(r['h'], ns, 0, 0, 1, keep_v=True)
    E = e.rx_apply_combiner(r['c'], r['h'])[:, :ns].astype(np.complex128)
    want = rep.sigma.astype(np.float64)[:, :, None, :] * rep.v.astype(np.complex128)
    bound = 2 * (nr + 5) * U24 * rep.sigma.astype(np.float64)[:, :1, None, :]
    ratio = (np.abs(np.conj(E) - want) / bound).max()
    print('%s: |conj(E) - sigma d_v| / bound %.3f' % (shape, ratio))
    assert ratio <= 1.0
    assert np.abs(r['sigma'].astype(np.float64) - rep.sigma).max() <= 2.0 ** -22 * rep.sigma.max()


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_e_apply_against_the_fp64_product(pkg, shape):
    nt, nr, ns = shape
    r = _run(pkg, shape, 'iid')
    e, h = r['e'], r['h']
    E = e.rx_apply_combiner(r['c'], h)
    assert E.shape == h.shape and not E[:, ns:].any()
    Cd = _rows(r['c']).astype(np.complex128)
    ref = Cd @ r['H']
    bound = (nr + 1) * U24 * (np.abs(Cd) @ np.abs(r['H']))
    ratio = (np.abs(_rows(E[:, :ns]).astype(np.complex128) - ref) / bound).max()
    print('%s: apply error / bound %.3f' % (shape, ratio))
    assert ratio <= 1.0
    eye = np.zeros((NPKT, ns, nr, N), np.complex64)
    for s in range(ns):
        eye[:, s, s] = 1
    picked = e.rx_apply_combiner(eye, h)
    assert np.array_equal(picked[:, :ns].view(np.uint64), h[:, :ns].view(np.uint64)) and not picked[:, ns:].any()


def test_f_data_phase_through_the_combiners(pkg):
    """Two users at (8, 4, 2), perfect CSI, continuous angles, 2 symbols, QPSK: compress, expand (CSI layout), precoder, data phase on E_u"""
    nt, nr, ns = 8, 4, 2
    e = _engine(pkg, nt, nr)
    hs = [R.planes(80 + u, NPKT, nr, nt) for u in range(2)]
    rebuilt = [e.feedback_expand(e.feedback_compress(h, ns, 0, 0, 1), 'csi') for h in hs]
    W = e.mu_precoder(rebuilt, ns)
    Es = [e.rx_apply_combiner(e.rx_combiner(h, ns), h) for h in hs]
    res = e.mu_link_sim(Es, W, 1e-3, seed=9, ns=ns, n_sym=2, bps=2, details=True)
    plain = e.mu_link_sim(hs, W, 1e-3, seed=9, ns=ns, n_sym=2, bps=2)
    g = res.g.astype(np.complex128)                                     # [U, npkt, ns, M, 234]
    G = [[g[u, p].transpose(2, 0, 1) for u in range(2)] for p in range(NPKT)]
    leak = max(C.leakage(G[p], ns) for p in range(NPKT))
    # the complex64 restatement of the same chain: the report's vectors decomposed and expanded in float32, S V^H in complex64, the
    # precoder of mu_link_ref on those planes rounded to complex64, the combiner and E_u in complex64, G = E_u W as a complex64 product
    yard = 0.0
    for p in range(NPKT):
        est, heard = [], []
        for h in hs:
            Hm = h[p].transpose(2, 0, 1)
            V, s = R.svd_vectors(Hm, ns)
            V32 = R.column_phases(V.astype(np.complex64), np.float32)
            phi, psi, _ = R.decompose(V32, np.float32)
            svh = s.astype(np.float32)[:, :, None] * np.conj(R.expand_angles(phi, psi, nt, ns, np.float32)).transpose(0, 2, 1)
            full = np.zeros((N, nr, nt), np.complex64)
            full[:, :ns] = svh
            est.append(full.transpose(1, 2, 0))
            C32, _ = C.combiner(Hm, ns, np.float32)
            heard.append(C.apply(C32, Hm, np.float32).transpose(1, 2, 0))
        Wr = MU.precoder(est, ns, 0.0)[0].astype(np.complex64)
        yard = max(yard, C.leakage([np.einsum('ijk,mjk->kim', x[:ns], Wr) for x in heard], ns))
    print('leakage %.3g, complex64 restatement %.3g' % (leak, yard))
    assert leak <= 4.0 * yard
    assert not res.bit_errors.any()
    for u in range(2):
        for p in range(NPKT):
            assert abs(float(res.sinr_db[u, p]) - MU.sinr_db(G[p][u], u, ns, 1e-3)) <= 1e-3
    print('sinr_db combined %s, uncombined %s' % (res.sinr_db.mean(1), plain.sinr_db.mean(1)))
    assert (res.sinr_db > plain.sinr_db).all()


def test_g_position_chunks_and_a_bf16_context(pkg):
    shape = SHAPES[1]
    nt, nr, ns = shape
    r = _run(pkg, shape, 'iid')
    e, h = r['e'], r['h']
    E = e.rx_apply_combiner(r['c'], h)
    part = e.rx_combiner(h[1:], ns, keep_sigma=True)
    assert np.array_equal(part[0].view(np.uint64), r['c'][1:].view(np.uint64)) and np.array_equal(part[1].view(np.uint32), r['sigma'][1:].view(np.uint32))
    assert np.array_equal(e.rx_apply_combiner(r['c'][1:], h[1:]).view(np.uint64), E[1:].view(np.uint64))
    for kw in (dict(workspace_bytes=1), dict(dtype='bf16')):
        other = pkg.CsiEngine(nt, nr, hidden=(64, 64), device=0, **kw)
        c2, s2 = other.rx_combiner(h, ns, keep_sigma=True)
        assert np.array_equal(c2.view(np.uint64), r['c'].view(np.uint64)) and np.array_equal(s2.view(np.uint32), r['sigma'].view(np.uint32))
        assert np.array_equal(other.rx_apply_combiner(c2, h).view(np.uint64), E.view(np.uint64))
        other.close()


def test_h_sweep_miniature(pkg, tmp_path):
    """sweep --ber --users 2 --feedback 9 7 --rxCombine against the same run without --rxCombine"""
    import json
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    out, out2 = str(tmp_path / 'comb'), str(tmp_path / 'plain')
    common = ['--nTX', '8', '--nRX', '2', '--nn', '16', '--trainPkts', '24', '--testPkts', '6', '--snr', '20', '--epochs', '1',
              '--bs', '16', '--quiet', '--ber', '--numSTS', '1', '--rays', '32', '--dataSymbols', '2', '--users', '2', '--feedback', '9', '7']
    assert sweep.main(['-d', out] + common + ['--rxCombine']) == 0
    assert sweep.main(['-d', out2, '--modeldir', out] + common) == 0
    res, res2 = json.load(open(os.path.join(out, 'sweep.json'))), json.load(open(os.path.join(out2, 'sweep.json')))
    assert res['rx_combine'] is True and 'rx_combine' not in res2
    m, m2 = loadmat(os.path.join(out, 'BS8_SNR20', 'metrics.mat')), loadmat(os.path.join(out2, 'BS8_SNR20', 'metrics.mat'))
    old = [k for k in m2 if not k.startswith('__')]
    new = ([f + x for x in sweep.SOURCES for f in sweep.FBC_FIELDS] + [f + x for x in sweep.SOURCES for f in sweep.MUC_FIELDS]
           + [f + x for x in sweep.SOURCES for f in sweep.MUFBC_FIELDS])
    assert [k for k in m if not k.startswith('__')] == old + new
    for k in old:
        assert np.array_equal(m[k], m2[k]), k                                            # every existing field is unchanged
    for k in new:
        assert m[k].shape == (1, 6) and np.isfinite(m[k]).all(), k
    mean = lambda k: float(m[k].mean())                                                  # noqa: E731
    print('20 dB perfect: sinrMU %.2f, sinrMUFB %.2f, sinrMUC %.2f, sinrMUFBC %.2f, sinrFB %.2f, sinrFBC %.2f dB'
          % tuple(mean(k + '_perfect') for k in ('sinrMU', 'sinrMUFB', 'sinrMUC', 'sinrMUFBC', 'sinrFB', 'sinrFBC')))
    assert mean('sinrMUFBC_perfect') > mean('sinrMUFB_perfect') + 10.0
    assert mean('sinrMUFBC_perfect') > mean('sinrMU_perfect')
    lv = res['levels'][0]
    assert np.asarray(lv['mufbc_users']['perfect']['sinr']).shape == (2, 6) and np.asarray(lv['muc_users']['LS']['bers']).shape == (2, 6)
