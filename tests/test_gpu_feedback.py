"""GPU tests (-m gpu) of the quantised CSI feedback (csi_feedback_compress_device, csi_feedback_expand_device, csrc/feedback.hip.h,
DESIGN.md 4.24) against the fp64 statement tests/feedback_ref.py.

Shapes (Nt, Nr, nc, npkt, ng): 3 packets give 702 reports, no multiple of 64; ng = 2 and 4 have a partial last group (117 and 59
reports); (4, 4, 4) takes the min(nc, Nt-1) branch; Nt = 32 is the array the sweep runs.  Every case runs with its own bit pair, the
ends of both ranges among them.  One compress call and the expansions of a case are shared by the tests that read them.

Bounds.  sigma: 1e-5 relative, the project's row contract.  d_v: 1 - |v^H v_ref| <= 1e-5 on the reports whose eigenvalue gaps
(l_s - l_{s+1}) / l_1, s < nc and s + 1 < Nr, exceed 0.05; at least 80 % of the reports must qualify.  Codes, against the fp64
decomposition of the device's OWN d_v: every difference is one code (cyclic for phi), in at most 1e-3 of the case's angles, and per
report the fp64 expansion of the device's codes is no further from d_v than that of the reference's codes plus 1e-5.  Expansion: the
largest elementwise error against the fp64 expansion is at most 4 x that of the complex64 restatement on the same codes plus 2^-23 (the
margin covers operation order); |Vhat^H Vhat - I| within the same yardstick."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feedback_ref as R      # noqa: E402
import mu_link_ref as MU      # noqa: E402

N = R.N
EPS = 2.0 ** -23
# (Nt, Nr, nc, npkt, ng), (b_phi, b_psi)
CASES = [((4, 2, 1, 3, 1), (4, 2)), ((4, 2, 2, 3, 2), (6, 4)), ((4, 4, 4, 2, 1), (9, 7)), ((8, 4, 2, 3, 4), (7, 5)), ((32, 4, 1, 2, 1), (10, 8)),
         ((32, 4, 2, 2, 1), (2, 1))]
IDS = ['nt%d_nr%d_nc%d_p%d_ng%d' % c[0] for c in CASES]
_engines, _cache = {}, {}


def _engine(pkg, nt, nr):
    if (nt, nr) not in _engines:
        _engines[(nt, nr)] = pkg.CsiEngine(nt, nr, hidden=(8,), device=0)
    return _engines[(nt, nr)]


def _items(a):
    """[npkt, x, n_rep] -> [npkt n_rep, x]"""
    return np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(-1, a.shape[1])


def _vmat(v):
    """[npkt, nc, nt, n_rep] -> [npkt n_rep, nt, nc]"""
    return np.ascontiguousarray(v.transpose(0, 3, 2, 1)).reshape(-1, v.shape[2], v.shape[1])


def _w_items(W, ng):
    """W layout [npkt, nc, nt, 234] -> the reported carriers' matrices [npkt n_rep, nt, nc]"""
    return np.ascontiguousarray(W[..., ::ng].transpose(0, 3, 2, 1)).reshape(-1, W.shape[2], W.shape[1])


def _run(pkg, case):
    if case not in _cache:
        (nt, nr, nc, npkt, ng), (b_phi, b_psi) = case
        e = _engine(pkg, nt, nr)
        h = R.planes(100 + nt + nc, npkt, nr, nt)
        n0 = e.get_option('feedback_launches')
        rep = e.feedback_compress(h, nc, b_phi, b_psi, ng, keep_angles=True, keep_v=True)
        assert e.get_option('feedback_launches') == n0 + 1
        Vd = _vmat(rep.v).astype(np.complex128)
        phi, psi, left = R.decompose(Vd)
        kphi, kpsi = R.quantise(phi, psi, b_phi, b_psi)
        rng = np.random.default_rng(7 + nt)
        rnd = rep._replace(phi_code=rng.integers(0, 2 ** b_phi, rep.phi_code.shape).astype(np.uint16),
                           psi_code=rng.integers(0, 2 ** b_psi, rep.psi_code.shape).astype(np.uint16))
        out = dict(e=e, h=h, rep=rep, Vd=Vd, phi=phi, psi=psi, left=left, kphi=kphi, kpsi=kpsi, rnd=rnd)
        for name, r in (('own', rep), ('rnd', rnd)):
            out['w_' + name] = e.feedback_expand(r, 'w')
            out['csi_' + name] = e.feedback_expand(r, 'csi')
            out['csi1_' + name] = e.feedback_expand(r, 'csi', use_sigma=False)
        out['w_cont'] = e.feedback_expand(rep, 'w', continuous=True)
        _cache[case] = out
    return _cache[case]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_a_singular_values_and_vectors(pkg, case):
    (nt, nr, nc, npkt, ng), _ = case
    c = _run(pkg, case)
    H = R.reported(c['h'], ng)
    Vr, sr = R.svd_vectors(H, nc)
    sd = _items(c['rep'].sigma).astype(np.float64)
    rel = np.abs(sd - sr).max() / sr.max()
    row = (np.linalg.norm(sd - sr, axis=1) / np.linalg.norm(sr, axis=1)).max()
    lam = np.linalg.svd(H.astype(np.complex128), compute_uv=False) ** 2
    m = min(nc, nr - 1)
    ok = ((lam[:, :m] - lam[:, 1:m + 1]) / lam[:, :1]).min(1) > 0.05 if m else np.ones(len(lam), bool)
    align = 1.0 - np.abs(np.einsum('njs,njs->ns', np.conj(c['Vd']), Vr))
    last = c['Vd'][:, -1, :]
    print('%s: sigma row error %.3g, %.3f of the reports qualify, 1 - |v^H v_ref| %.3g on them (%.3g on all)'
          % (case[0], row, ok.mean(), align[ok].max(), align.max()))
    assert row <= 1e-5 and rel <= 1e-5
    assert ok.mean() >= 0.8
    assert align[ok].max() <= 1e-5
    assert (last.imag == 0).all() and (last.real >= 0).all()                               # step 2: the last row real and >= 0, to the bit
    assert np.abs(np.linalg.norm(c['Vd'], axis=1) - 1).max() <= 1e-5


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_b_codes_against_the_fp64_decomposition_of_the_own_vectors(pkg, case):
    (nt, nr, nc, npkt, ng), (b_phi, b_psi) = case
    c = _run(pkg, case)
    rep = c['rep']
    n_ang = R.n_angles(nt, nc)
    assert rep.phi_code.shape == rep.psi_code.shape == rep.phi.shape == (npkt, n_ang, R.n_reports(ng))
    # (d_v is fp32: its columns are orthonormal to rounding, and so is what the fp64 decomposition leaves of them)
    assert np.abs(c['left'] - np.eye(nt, nc)).max() <= 8 * nt * EPS
    dphi, dpsi = _items(rep.phi_code), _items(rep.psi_code)
    assert dphi.max() < 2 ** b_phi and dpsi.max() < 2 ** b_psi
    d1, d2 = R.cyclic_diff(dphi, c['kphi'], b_phi), np.abs(dpsi.astype(np.int64) - c['kpsi'])
    share = ((d1 != 0).sum() + (d2 != 0).sum()) / (2.0 * d1.size)
    far = lambda kp, ks: np.linalg.norm(R.expand(kp, ks, nt, nc, b_phi, b_psi) - c['Vd'], axis=(1, 2))      # noqa: E731
    excess = (far(dphi.astype(np.int64), dpsi.astype(np.int64)) - far(c['kphi'], c['kpsi'])).max()
    # the continuous angles, where the element they are taken from has modulus above 1e-2 (below, the angle is the rounding's)
    aphi, apsi = _items(rep.phi).astype(np.float64), _items(rep.psi).astype(np.float64)
    mod_phi, mod_psi = _moduli(c['Vd'])
    ephi = np.abs(np.angle(np.exp(1j * (aphi - c['phi']))))
    epsi = np.abs(apsi - c['psi'])
    print('%s bits %s: %d + %d codes differ (share %.3g), all by one: %s; distance excess %.3g; angle error phi %.3g psi %.3g'
          % (case[0], (b_phi, b_psi), (d1 != 0).sum(), (d2 != 0).sum(), share, d1.max() <= 1 and d2.max() <= 1, excess,
             ephi[mod_phi > 1e-2].max(), epsi[mod_psi > 1e-2].max()))
    assert d1.max() <= 1 and d2.max() <= 1
    assert share <= 1e-3
    assert excess <= 1e-5
    # an fp32 angle below 2 pi is a few ulp of 4 EPS off (format and atan2f); an element of modulus m that carries the rounding of up to
    # Nt rotations and phases in front of it turns by 4 Nt EPS / m at the most
    for err_a, mod in ((ephi, mod_phi), (epsi, mod_psi)):
        big = mod > 1e-2
        assert (err_a[big] <= 8 * EPS + 4 * nt * EPS / mod[big]).all()
    assert aphi.min() >= 0 and aphi.max() < 2 * np.pi and apsi.min() >= 0 and apsi.max() <= np.float32(np.pi / 2)


def _moduli(V):
    """the moduli the angles of the fp64 decomposition are taken from: |V[l][i]| for phi, hypot(a, b) for psi, in angle order"""
    V = V.copy()
    n, nt, nc = V.shape
    mphi, mpsi = [], []
    for i in range(min(nc, nt - 1)):
        x = V[:, i:nt - 1, i]
        m = np.abs(x)
        mphi.append(m)
        V[:, i:nt - 1, :] *= np.conj(np.where(m > 0, x / np.where(m > 0, m, 1), 1))[:, :, None]
        for l in range(i + 1, nt):
            a, b = V[:, i, i].real.copy(), V[:, l, i].real.copy()
            hh = np.hypot(a, b)
            mpsi.append(hh)
            cc, ss = np.where(hh > 0, a / np.where(hh > 0, hh, 1), 1)[:, None], np.where(hh > 0, b / np.where(hh > 0, hh, 1), 0)[:, None]
            ri, rl = V[:, i, :].copy(), V[:, l, :].copy()
            V[:, i, :], V[:, l, :] = cc * ri + ss * rl, cc * rl - ss * ri
    return np.concatenate(mphi, 1), np.stack(mpsi, 1)


@pytest.mark.parametrize('which', ['own', 'rnd'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_c_expansion_against_fp64(pkg, case, which):
    """the device's own codes, and random codes over the whole code range, in both layouts"""
    (nt, nr, nc, npkt, ng), (b_phi, b_psi) = case
    c = _run(pkg, case)
    rep = c['rep'] if which == 'own' else c['rnd']
    kphi, kpsi = _items(rep.phi_code).astype(np.int64), _items(rep.psi_code).astype(np.int64)
    ref = R.expand(kphi, kpsi, nt, nc, b_phi, b_psi)
    yard = 4.0 * np.abs(R.expand(kphi, kpsi, nt, nc, b_phi, b_psi, np.float32) - ref).max() + EPS
    W, C, C1 = c['w_' + which], c['csi_' + which], c['csi1_' + which]
    assert W.shape == (npkt, nc, nt, N) and C.shape == C1.shape == (npkt, nr, nt, N)
    scale = np.float32(np.sqrt(nt / nc))
    Vh = _w_items(W, ng).astype(np.complex128) / np.float64(scale)
    err = np.abs(Vh - ref).max()
    orth = np.abs(np.conj(Vh.transpose(0, 2, 1)) @ Vh - np.eye(nc)).max()
    v32 = R.expand(kphi, kpsi, nt, nc, b_phi, b_psi, np.float32).astype(np.complex128)
    yard_orth = 4.0 * np.abs(np.conj(v32.transpose(0, 2, 1)) @ v32 - np.eye(nc)).max() + EPS      # (the float32 tables: cos^2 + sin^2 = 1 to 2^-24 only)
    print('%s %s codes, bits %s: error %.3g = %.3f of the yardstick %.3g; orthonormality %.3g = %.3f of its yardstick'
          % (case[0], which, (b_phi, b_psi), err, err / yard, yard, orth, orth / yard_orth))
    assert err <= yard                                                                     # (the scale is one more rounding: inside the 2^-23)
    assert orth <= yard_orth
    assert np.abs((np.abs(W.astype(np.complex128)) ** 2).sum((1, 2)) - nt).max() <= 1e-5 * nt
    # a carrier inside a group holds its report's matrix to the bit
    k = np.arange(N)
    for A in (W, C, C1):
        assert np.array_equal(A.view(np.uint64), A[..., (k // ng) * ng].view(np.uint64))
    # the CSI layout: row s < nc = sigma_s conj(Vhat[:, s]), the other rows zero to the bit
    assert not C[:, nc:].view(np.uint64).any() and not C1[:, nc:].view(np.uint64).any()
    assert np.abs(_w_items(np.conj(C1[:, :nc]), ng) - ref).max() <= yard
    sig = _items(rep.sigma).astype(np.float64)
    got = _w_items(np.conj(C[:, :nc]), ng).astype(np.complex128)
    assert (np.abs(got - ref * sig[:, None, :]) / sig[:, None, :]).max() <= yard + EPS


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_d_continuous_round_trip(pkg, case):
    """b = 0: the expansion of the continuous angles is sqrt(Nt / nc) d_v, held along the group.  Yardstick: the complex64 restatement of
    decomposition and expansion on the same vectors"""
    (nt, nr, nc, npkt, ng), _ = case
    c = _run(pkg, case)
    e = c['e']
    cont = e.feedback_compress(c['h'], nc, 0, 0, ng, keep_v=True)
    assert cont.phi_code is None and cont.psi_code is None
    assert np.array_equal(cont.phi.view(np.uint32), c['rep'].phi.view(np.uint32)) and np.array_equal(cont.psi.view(np.uint32), c['rep'].psi.view(np.uint32))
    assert np.array_equal(cont.v.view(np.uint64), c['rep'].v.view(np.uint64)) and np.array_equal(cont.sigma.view(np.uint32), c['rep'].sigma.view(np.uint32))
    W = e.feedback_expand(cont, 'w')
    assert np.array_equal(W.view(np.uint64), c['w_cont'].view(np.uint64))
    p32, s32, _ = R.decompose(c['Vd'].astype(np.complex64), np.float32)
    yard = 4.0 * np.abs(R.expand_angles(p32, s32, nt, nc, np.float32) - c['Vd']).max() + EPS
    Vh = _w_items(W, ng).astype(np.complex128) / np.float64(np.float32(np.sqrt(nt / nc)))
    err = np.abs(Vh - c['Vd']).max()
    print('%s: continuous round trip error %.3g = %.3f of the yardstick %.3g' % (case[0], err, err / yard, yard))
    assert err <= yard
    k = np.arange(N)
    assert np.array_equal(W.view(np.uint64), W[..., (k // ng) * ng].view(np.uint64))


def test_e_through_the_existing_data_phase(pkg):
    """ns = 1, Nt = 8, Nr = 2, 16 packets, noise_var fixed.  csi_mu_link_sim_device sends a user's ns streams to its FIRST ns receive
    antennas (G_uu = H[:ns] W), so the report is taken of the rows the data phase addresses - the planes handed to the compression hold
    the true row 0 and a zero row 1.  Their dominant right singular vector maximises sum_k |H[:ns] v|^2, which is the numerator of
    sinr_db: the SINR with the quantised W never exceeds that with the continuous-angle W (1e-3 dB per packet), and the continuous one
    is within 1e-3 dB of a W from the fp64 singular vectors.  (With the second row left in, the vector serves an antenna the data phase
    does not listen on, and the order of the two SINRs is chance: measured -0.0015 .. 0.0014 dB at bits (9, 7).)"""
    nt, nr, ns, npkt = 8, 2, 1, 16
    e = _engine(pkg, nt, nr)
    h = R.planes(55, npkt, nr, nt)
    addressed = h.copy()
    addressed[:, ns:] = 0
    Vr, _ = R.svd_vectors(R.reported(addressed, 1), ns)
    W_ref = (np.sqrt(nt / ns) * R.column_phases(Vr)).reshape(npkt, N, nt, ns).transpose(0, 3, 2, 1)
    cont = e.feedback_compress(addressed, ns, 0, 0, 1)
    sinr = lambda W: e.mu_link_sim([h], W, 0.1, seed=3, ns=ns, n_sym=1, bps=2).sinr_db[0].astype(np.float64)      # noqa: E731
    s_ref, s_cont = sinr(W_ref), sinr(e.feedback_expand(cont, 'w'))
    print('continuous against fp64 vectors: %.3g dB' % np.abs(s_cont - s_ref).max())
    assert np.abs(s_cont - s_ref).max() <= 1e-3
    for bits in ((2, 1), (4, 2), (9, 7)):
        s_q = sinr(e.feedback_expand(e.feedback_compress(addressed, ns, bits[0], bits[1], 1), 'w'))
        print('bits %s: SINR loss %.4f .. %.4f dB' % (bits, (s_cont - s_q).min(), (s_cont - s_q).max()))
        assert (s_q - s_cont).max() <= 1e-3


def test_f_two_users_through_the_existing_precoder(pkg):
    """csi_mu_precoder_device on the continuous CSI-layout planes of two users against its fp64 statement on S V^H of the true planes"""
    nt, nr, nc, npkt = 8, 2, 2, 3
    e = _engine(pkg, nt, nr)
    hs = [R.planes(60 + u, npkt, nr, nt) for u in range(2)]
    rebuilt, exact = [], []
    for h in hs:
        rebuilt.append(e.feedback_expand(e.feedback_compress(h, nc, 0, 0, 1), 'csi'))
        V, s = R.svd_vectors(R.reported(h, 1), nc)
        svh = s[:, :, None] * np.conj(R.column_phases(V)).transpose(0, 2, 1)               # [n, nc, nt]
        exact.append(svh.reshape(npkt, N, nc, nt).transpose(0, 2, 3, 1))
    W = e.mu_precoder(rebuilt, nc).astype(np.complex128)
    worst = 0.0
    for p in range(npkt):
        Wr, cond = MU.precoder([x[p] for x in exact], nc, 0.0)
        err = np.sqrt((np.abs(W[p] - Wr) ** 2).sum((0, 1)) / (np.abs(Wr) ** 2).sum((0, 1)))
        worst = max(worst, float((err / np.maximum(1e-5, 1e-6 * cond ** 2)).max()))
    print('two users: largest precoder error / bound %.4f' % worst)
    assert worst <= 1.0


def test_g_two_runs_chunks_and_a_bf16_context_are_bit_identical(pkg):
    case = CASES[3]
    (nt, nr, nc, npkt, ng), (b_phi, b_psi) = case
    c = _run(pkg, case)
    e = c['e']
    rep = e.feedback_compress(c['h'], nc, b_phi, b_psi, ng, keep_angles=True, keep_v=True)
    for a, b in zip(rep[:6], c['rep'][:6]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert np.array_equal(e.feedback_expand(rep, 'w').view(np.uint64), c['w_own'].view(np.uint64))
    assert np.array_equal(e.feedback_expand(rep, 'csi').view(np.uint64), c['csi_own'].view(np.uint64))
    # a small workspace: one packet per chunk, the same bits
    small = pkg.CsiEngine(nt, nr, hidden=(8,), device=0, workspace_bytes=1)
    n0 = small.get_option('feedback_launches')
    rep2 = small.feedback_compress(c['h'], nc, b_phi, b_psi, ng, keep_angles=True, keep_v=True)
    assert small.get_option('feedback_launches') == n0 + npkt
    for a, b in zip(rep2[:6], c['rep'][:6]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    small.close()
    # a bf16 context is served alike: all planes of these entries are fp32
    half = pkg.CsiEngine(nt, nr, hidden=(8,), device=0, dtype='bf16')
    rep3 = half.feedback_compress(c['h'], nc, b_phi, b_psi, ng, keep_angles=True, keep_v=True)
    for a, b in zip(rep3[:6], c['rep'][:6]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert np.array_equal(half.feedback_expand(rep3, 'csi').view(np.uint64), c['csi_own'].view(np.uint64))
    half.close()


class _At:
    def __init__(self, ptr):
        self.ptr = ptr


def test_h_refusals(pkg):
    """every refusal raises with text that names the argument, and nothing is counted"""
    nt, nr, npkt = 8, 4, 2
    e = _engine(pkg, nt, nr)
    big = [e.to_device(np.zeros((npkt, nr, nt, N + 8), np.float32)) for _ in range(9)]
    n0 = e.get_option('feedback_launches')

    def comp(text, nc=2, b=(4, 2), ng=1, n=npkt, eng=e, **kw):
        a = dict(d_phi_code=big[2], d_psi_code=big[3], d_phi=big[4], d_psi=big[5], d_sigma=big[6], d_v_re=big[7], d_v_im=big[8])
        a.update(kw)
        with pytest.raises(pkg.CsiError) as err:
            eng.feedback_compress_device(a.pop('h_re', big[0]), a.pop('h_im', big[1]), n, nc, b[0], b[1], ng, **a)
        assert err.value.code == -1 and text in str(err.value), (text, str(err.value))

    def exp(text, nc=2, b=(4, 2), ng=1, n=npkt, layout=0, eng=e, **kw):
        a = dict(d_phi_code=big[2], d_psi_code=big[3], d_sigma=big[6])
        a.update(kw)
        with pytest.raises(pkg.CsiError) as err:
            eng.feedback_expand_device(n, nc, b[0], b[1], ng, layout, a.pop('out_re', big[0]), a.pop('out_im', big[1]), **a)
        assert err.value.code == -1 and text in str(err.value), (text, str(err.value))

    for f in (comp, exp):
        f('nc 0 outside', nc=0)
        f('nc 5 outside', nc=5)
        f('ng 3 is not', ng=3)
        f('b_phi 1 outside', b=(1, 2))
        f('b_phi 11 outside', b=(11, 2))
        f('b_psi 9 outside', b=(4, 9))
        f('only one of them is 0', b=(0, 3))
        f('only one of them is 0', b=(4, 0))
        f('npkt -1', n=-1)
    comp('null required pointer (h_re, h_im)', h_re=_At(None))
    comp('null required pointer (d_phi_code, d_psi_code)', d_phi_code=None, d_psi_code=None)
    comp('null required pointer (d_phi, d_psi', b=(0, 0), d_phi=None, d_psi=None)
    comp('d_phi_code / d_psi_code come as a pair', d_psi_code=None)
    comp('d_phi / d_psi come as a pair', d_psi=None)
    comp('the v planes come as a pair', d_v_im=None)
    for name, key in (('d_h_re', 'h_re'), ('d_h_im', 'h_im'), ('d_v_re', 'd_v_re'), ('d_v_im', 'd_v_im')):
        comp('%s must start on a 16-byte boundary' % name, **{key: _At(big[0].ptr + 4)})
    comp('d_phi_code must be aligned', d_phi_code=_At(big[2].ptr + 1))
    exp('layout 7 is not', layout=7)
    exp('exactly one of the pairs', d_phi=big[4], d_psi=big[5])
    exp('exactly one of the pairs', d_phi_code=None, d_psi_code=None)
    exp('d_phi_code / d_psi_code come as a pair', d_psi_code=None)
    exp('null required pointer (out_re, out_im)', out_im=_At(None))
    exp('d_out_re must start on a 16-byte boundary', out_re=_At(big[0].ptr + 4))
    exp('d_out_im must start on a 16-byte boundary', out_im=_At(big[1].ptr + 4))
    exp('codes need their bit widths', b=(0, 0))
    e.synchronize()
    assert e.get_option('feedback_launches') == n0
    assert all(not a.download().any() for a in big), 'a refused call wrote'
    # npkt == 0 returns 0 and launches nothing
    e.feedback_compress_device(big[0], big[1], 0, 2, 4, 2, 1, big[2], big[3])
    e.feedback_expand_device(0, 2, 4, 2, 1, 0, big[0], big[1], d_phi_code=big[2], d_psi_code=big[3])
    assert e.get_option('feedback_launches') == n0
    # shapes of the context: nc above Nr, Nr above 16, an LDS image beyond 160 KiB, a single-input context
    two = _engine(pkg, 4, 2)
    comp('nc 3 outside 1 .. min(4, Nr 2, Nt 4)', nc=3, eng=two)
    many = pkg.CsiEngine(32, 32, hidden=(8,), device=0)
    comp('Nr 32 > 16', eng=many)
    exp('Nr 32 > 16', eng=many)
    wide = pkg.CsiEngine(1024, 4, hidden=(8,), device=0)
    comp('bytes of LDS (160 KiB per workgroup)', nc=4, eng=wide)
    exp('bytes of LDS (160 KiB per workgroup)', nc=4, eng=wide)
    one = pkg.CsiEngine(0, 1, hidden=(16,), len_ltf=64)
    comp('single-input context', nc=1, eng=one)
    exp('single-input context', nc=1, eng=one)
    for x in (many, wide, one):
        assert x.get_option('feedback_launches') == 0
        x.close()
    # the context stays usable
    rep = e.feedback_compress(R.planes(1, 1, nr, nt), 2, 4, 2, 1)
    assert e.get_option('feedback_launches') == n0 + 1 and rep.phi_code.shape == (1, R.n_angles(nt, 2), N)


def test_i_sweep_miniature(pkg, tmp_path):
    """sweep --ber --users 2 --feedback 9 7 against the same run without it: every existing field unchanged, the FB and MUFB families
    behind them, the report size and the per-user arrays in sweep.json"""
    import json
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    out, out2 = str(tmp_path / 'fb'), str(tmp_path / 'plain')
    common = ['--nTX', '8', '--nRX', '2', '--nn', '16', '--trainPkts', '24', '--testPkts', '6', '--snr', '20', '--epochs', '1',
              '--bs', '16', '--quiet', '--ber', '--numSTS', '1', '--rays', '32', '--dataSymbols', '2', '--users', '2']
    assert sweep.main(['-d', out] + common + ['--feedback', '9', '7', '--feedbackNg', '2']) == 0
    assert sweep.main(['-d', out2, '--modeldir', out] + common) == 0
    res, res2 = json.load(open(os.path.join(out, 'sweep.json'))), json.load(open(os.path.join(out2, 'sweep.json')))
    assert res['feedback'] == dict(b_phi=9, b_psi=7, ng=2, report_bits=7 * 16 * 117) and 'feedback' not in res2
    m, m2 = loadmat(os.path.join(out, 'BS8_SNR20', 'metrics.mat')), loadmat(os.path.join(out2, 'BS8_SNR20', 'metrics.mat'))
    new = [f + x for x in sweep.SOURCES for f in sweep.FB_FIELDS] + [f + x for x in sweep.SOURCES for f in sweep.MUFB_FIELDS]
    old = sorted(k for k in m2 if not k.startswith('__'))
    assert sorted(k for k in m if not k.startswith('__')) == sorted(old + new)
    written = sweep.metric_fields({k: m[k] for k in m if not k.startswith('__')})
    assert written[:len(old)] == sweep.metric_fields({k: m2[k] for k in old}) and written[len(old):] == new
    for k in old:
        assert np.array_equal(m[k], m2[k]), k                                            # every existing field is unchanged
    for k in new:
        assert m[k].shape == (1, 6) and np.isfinite(m[k]).all(), k
    lv, lv2 = res['levels'][0], res2['levels'][0]
    assert set(lv2) == set(lv) - set(new) - {'mufb_users'} and lv['mu_users'] == lv2['mu_users']
    for x in sweep.SOURCES:
        per = lv['mufb_users'][x]
        assert np.asarray(per['bers']).shape == (2, 6)
        assert np.allclose(np.mean(per['sinr'], 0), m['sinrMUFB_' + x][0])
    print('20 dB: sinrFB perfect %.2f dB, sinrMU / sinrMUFB perfect %.2f / %.2f dB'
          % (m['sinrFB_perfect'].mean(), m['sinrMU_perfect'].mean(), m['sinrMUFB_perfect'].mean()))
