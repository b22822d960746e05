"""GPU tests of the multi-user JSDM precoder (csi_mu_covariance_device, csi_mu_jsdm_precoder_device, csrc/mu_jsdm.hip.h)
against the host restatement tests/jsdm_ref.py.

Inputs: planes with a prescribed covariance (jsdm_ref.planes: DFT eigenvectors rolled by 5 u per user, eigenvalues 0.6^j), rounded to
fp32, so that the eigen-gaps are known.  The covariance is judged against fp64 with numpy complex64 as the yardstick; the eigenpairs
are judged gap-free against the DEVICE's own covariance (and the second stage against the nulled covariance rebuilt in fp64 from the
device's own U*), by residual, orthonormality and Weyl's bound, with eps = 2^-23 and l_0 the largest eigenvalue of the item; only the
end-to-end projector comparison divides by the gaps (Davis-Kahan).  Margin rule: a (packet, group) whose relative gap is below 1e-3 or
whose tested ratio lies within 1e-3 of rank_tol is left out of the comparisons that depend on it, at most 10 % of the items."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import link_ref as L          # noqa: E402
import mu_link_ref as MU      # noqa: E402
import jsdm_ref as JS         # noqa: E402
from guarded import Guarded   # noqa: E402

N = L.N
EPS = 2.0 ** -23
OWN = None
# (Nt, Nr, U, ns, group, r_star, b)
# csi_create serves Nt in multiples of 4 only (16-byte rows): the smallest Nt and one that is no power of two (six rotations per step)
# lead the list; the eigen solver's other sizes (6, and 7 with its sit-out path) run in tests/test_mu_jsdm_host.py on the float32
# restatement of the kernel's arithmetic
CASES = [(4, 2, 2, 1, OWN, 1, 1),
         (12, 2, 2, 1, OWN, 2, 2),                         # no power of two
         (8, 2, 3, 1, (0, 1, 0), 2, 2),                    # a two-user group
         (16, 4, 4, 2, OWN, 2, 2),
         (32, 4, 4, 1, OWN, 4, 4),                         # n_rf = 16
         (32, 4, 8, 2, (0, 0, 1, 1, 2, 2, 3, 3), 4, 4),    # M = n_rf = 16
         (64, 2, 4, 1, OWN, 4, 4)]                         # Nt = 64
TOLS = [0.0, 0.3]
MODES = ['pgp', 'jgp']
MARGIN = 1e-3
SMALL = CASES[2]
_cache, _engines, _inputs, _ref = {}, {}, {}, {}


def _npkt(case):
    return 3 if case[0] == 64 else 5


def _f32(a):
    """what the library receives: fp32 planes, as complex128"""
    a = np.asarray(a)
    return a.real.astype(np.float32).astype(np.float64) + 1j * a.imag.astype(np.float32).astype(np.float64)


def _groups(case):
    nu, group = case[2], case[4]
    return (np.arange(nu) if group is None else np.asarray(group)), (nu if group is None else max(group) + 1)


def channels(case):
    key = case[:3]
    if key not in _inputs:
        nt, nr, nu = key
        _inputs[key] = [_f32(x) for x in JS.planes(nt, nr, nu, _npkt(case))]
    return _inputs[key]


def _engine(pkg, nt, nr, **kw):
    key = (nt, nr) + tuple(sorted(kw.items()))
    if key not in _engines:
        _engines[key] = pkg.CsiEngine(nt, nr, hidden=(8,), device=0, **kw)
    return _engines[key]


def reference(case, tol):
    """the fp64 statement per packet, shared and left unchanged"""
    key = (case, tol)
    if key not in _ref:
        nt, nr, nu, ns, group, r_star, b = case
        h = channels(case)
        _ref[key] = [JS.analog([x[p] for x in h], group, r_star, b, tol) for p in range(_npkt(case))]
    return _ref[key]


def _run(pkg, case, tol, mode):
    key = (case, tol, mode)
    if key not in _cache:
        nt, nr, nu, ns, group, r_star, b = case
        e = _engine(pkg, nt, nr)
        h = channels(case)
        w_re, w_im, frf, fbb, eig, ustar, rank = e.mu_jsdm_precoder(h, ns, r_star, b, groups=group, rank_tol=tol, mode=mode, keep_frf=True,
                                                                    keep_fbb=True, keep_eig=True)
        if ('cov', case[:3]) not in _cache:
            _cache[('cov', case[:3])] = e.mu_covariance(h)
        _cache[key] = dict(e=e, h=h, W=w_re.astype(np.float64) + 1j * w_im, w_re=w_re, w_im=w_im, frf=frf, fbb=fbb, eig=eig, ustar=ustar,
                           rank=rank, cov=_cache[('cov', case[:3])])
    return _cache[key]


def _group_cov(r, case, p, g):
    """R_g of the device's own covariance, in fp64"""
    grp, G = _groups(case)
    mem = [u for u in range(case[2]) if grp[u] == g]
    return sum(r['cov'][p, u].astype(np.complex128) for u in mem) / len(mem)


def _nulled_dev(r, case, p, g):
    """Rt_g rebuilt in fp64 from the device's own covariance, U*, ranks and l_0; and Q_g"""
    grp, G = _groups(case)
    us = [r['ustar'][p, y][:, :r['rank'][p, y, 0]].astype(np.complex128) for y in range(G)]
    Xi = np.concatenate([us[y] for y in range(G) if y != g] + [np.zeros((case[0], 0), np.complex128)], 1)
    Q = JS.gram_schmidt(Xi)
    return JS.nulled(_group_cov(r, case, p, g), Q, float(r['eig'][p, g, 0])), Q


def _left_out(case, tol):
    """(packet, group) pairs the margin rule leaves out"""
    out = set()
    for p, an in enumerate(reference(case, tol)):
        for g in range(an['rank'].shape[0]):
            if an['gaps'][g].min() < MARGIN or an['margin'][g] < MARGIN:
                out.add((p, g))
    assert len(out) <= 0.10 * len(reference(case, tol)) * reference(case, tol)[0]['rank'].shape[0], out
    return out


# ------------------------------------------------------------------------------------------------ 1: covariance
@pytest.mark.parametrize('case', CASES)
def test_1_covariance_against_fp64(pkg, oracle, case):
    """per (packet, user): max |R - R64| / max |R64|.  Yardstick: the same statement in numpy complex64; the device gets 4 x that
    (another summation order, another grouping inside the fp32 MFMA), the factor of the sibling tests.  Hermitian to the bit."""
    r = _run(pkg, case, 0.0, 'pgp')
    nt, nr, nu = case[:3]
    cov = r['cov']
    assert cov.shape == (_npkt(case), nu, nt, nt) and np.isfinite(cov.real).all() and np.isfinite(cov.imag).all()
    dev = yard = 0.0
    for p in range(_npkt(case)):
        for u in range(nu):
            R64 = JS.covariance(r['h'][u][p])
            R32 = JS.covariance(r['h'][u][p], np.complex64)
            assert R32.dtype == np.complex64
            top = np.abs(R64).max()
            dev = max(dev, float(np.abs(cov[p, u] - R64).max() / top))
            yard = max(yard, float(np.abs(R32 - R64).max() / top))
    print('%s: covariance error relative to the largest entry: device %.3e, numpy complex64 %.3e' % (case, dev, yard))
    assert dev <= 4.0 * yard
    re, im = np.ascontiguousarray(cov.real), np.ascontiguousarray(cov.imag)
    assert np.array_equal(re.view(np.uint32), np.ascontiguousarray(re.swapaxes(2, 3)).view(np.uint32))
    assert np.array_equal(im, -im.swapaxes(2, 3)) and (np.einsum('pujj->puj', im) == 0).all()


# ------------------------------------------------------------------------------------------------ 2: eigenpairs
@pytest.mark.parametrize('tol', TOLS)
@pytest.mark.parametrize('case', CASES)
def test_2_eigenpairs_against_the_device_covariance(pkg, oracle, case, tol):
    r = _run(pkg, case, tol, 'pgp')
    nt, nr, nu, ns, group, r_star, b = case
    grp, G = _groups(case)
    left = _left_out(case, tol)
    ref = reference(case, tol)
    worst = dict(res=0.0, orth=0.0, eig=0.0, res2=0.0, ray=0.0, orth2=0.0)
    yard = dict(res=0.0, orth=0.0, eig=0.0)
    for p in range(_npkt(case)):
        for g in range(G):
            R = _group_cov(r, case, p, g)
            w = np.linalg.eigvalsh(R)[::-1]
            l0 = w[0]
            lam = r['eig'][p, g].astype(np.float64)
            assert (np.diff(lam) <= 0).all()
            worst['eig'] = max(worst['eig'], float(np.abs(lam - w).max() / (nt * EPS * l0)))
            rg, qg = r['rank'][p, g]
            if (p, g) not in left:
                assert (rg, qg) == tuple(ref[p]['rank'][g]), (p, g, rg, qg, ref[p]['rank'][g])
            U = r['ustar'][p, g].astype(np.complex128)
            assert (U[:, rg:] == 0).all() and 0 <= rg <= r_star
            U = U[:, :rg]
            if rg:
                worst['res'] = max(worst['res'], float(np.sqrt((np.abs(R @ U - U * lam[:rg]) ** 2).sum(0)).max() / (4 * nt * EPS * l0)))
                worst['orth'] = max(worst['orth'], float(np.abs(np.conj(U).T @ U - np.eye(rg)).max() / (4 * nt * EPS)))
                _check_phase(U)
            # numpy complex64 on the same matrix, for the record
            l32, V32 = JS.eig_desc(R.astype(np.complex64))
            V32 = V32.astype(np.complex128)
            yard['eig'] = max(yard['eig'], float(np.abs(l32 - w).max() / (nt * EPS * l0)))
            yard['res'] = max(yard['res'], float(np.sqrt((np.abs(R @ V32 - V32 * l32) ** 2).sum(0)).max() / (4 * nt * EPS * l0)))
            yard['orth'] = max(yard['orth'], float(np.abs(np.conj(V32).T @ V32 - np.eye(nt)).max() / (4 * nt * EPS)))
            # second stage: the beams against the nulled covariance rebuilt from the device's own U*
            Rt, Q = _nulled_dev(r, case, p, g)
            assert qg == Q.shape[1]
            F = r['frf'][p][:, g * b:(g + 1) * b].astype(np.complex128)
            wt = np.linalg.eigvalsh(Rt)[::-1]
            rho = np.einsum('jq,jq->q', np.conj(F), Rt @ F).real / (np.abs(F) ** 2).sum(0)      # f^H Rt f / f^H f
            worst['ray'] = max(worst['ray'], float(np.abs(rho - wt[:b]).max() / (nt * EPS * l0)))
            worst['res2'] = max(worst['res2'], float(np.sqrt((np.abs(Rt @ F - F * rho) ** 2).sum(0)).max() / (4 * nt * EPS * l0)))
            worst['orth2'] = max(worst['orth2'], float(np.abs(np.conj(F).T @ F - np.eye(b)).max() / (4 * nt * EPS)))
            _check_phase(F)
    print('%s tol %s: over the bounds - residual %.3f (complex64 %.3f), orthonormality %.3f (%.3f), eigenvalues %.3f (%.3f); beams: residual %.3f, '
          'Rayleigh quotients %.3f, orthonormality %.3f; left out %d' % (case, tol, worst['res'], yard['res'], worst['orth'], yard['orth'], worst['eig'],
                                                                         yard['eig'], worst['res2'], worst['ray'], worst['orth2'], len(left)))
    assert max(worst.values()) <= 1.0, worst


def _check_phase(V):
    """in each column the entry of largest modulus is real and positive (exactly), the lowest j on a tie"""
    for c in range(V.shape[1]):
        a = np.abs(V[:, c])
        j = int(np.flatnonzero((V[:, c].imag == 0) & (V[:, c].real > 0) & (a >= a.max() * (1 - 4 * EPS)))[0])
        assert a[j] >= a.max() * (1 - 4 * EPS) and (a[:j] < a[j]).all(), (c, j)


# ------------------------------------------------------------------------------------------------ 3: nulling
@pytest.mark.parametrize('tol', TOLS)
@pytest.mark.parametrize('case', CASES)
def test_3_beams_null_the_other_groups(pkg, oracle, case, tol):
    r = _run(pkg, case, tol, 'jgp')
    nt, b = case[0], case[6]
    grp, G = _groups(case)
    worst = 0.0
    for p in range(_npkt(case)):
        for g in range(G):
            F = r['frf'][p][:, g * b:(g + 1) * b].astype(np.complex128)
            for y in range(G):
                if y == g:
                    continue
                U = r['ustar'][p, y][:, :r['rank'][p, y, 0]].astype(np.complex128)
                worst = max(worst, float(np.sqrt((np.abs(np.conj(U).T @ F) ** 2).sum()) / (8 * nt * EPS)))
            assert np.abs(np.conj(F).T @ F - np.eye(b)).max() <= 4 * nt * EPS
    print('%s tol %s: leakage |U*^H F|_F over 8 Nt eps: %.3f' % (case, tol, worst))
    assert worst <= 1.0
    assert np.array_equal(r['frf'], _run(pkg, case, tol, 'pgp')['frf'])                   # the mode does not enter the analog part


# ------------------------------------------------------------------------------------------------ 4: end to end
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('tol', TOLS)
@pytest.mark.parametrize('case', CASES)
def test_4_end_to_end(pkg, oracle, case, tol, mode):
    """the projector F_g F_g^H against fp64 within 8 Nt eps / (g1 g2) (Davis-Kahan through both stages, g1, g2 the relative gaps at r_g
    and at b, 1 where absent); W and Fbb against the fp64 baseband stage run with the device's own Frf within max(1e-5, 1e-6 cond(Gm)^2)"""
    r = _run(pkg, case, tol, mode)
    nt, nr, nu, ns, group, r_star, b = case
    grp, G = _groups(case)
    M, Q = nu * ns, G * b
    left, ref = _left_out(case, tol), reference(case, tol)
    wp = wb = 0.0
    flags = JS.PGP if mode == 'pgp' else 0
    for p in range(_npkt(case)):
        for g in range(G):
            if (p, g) in left or any((p, y) in left for y in range(G)):
                continue
            F = r['frf'][p][:, g * b:(g + 1) * b].astype(np.complex128)
            F64 = ref[p]['Frf'][:, g * b:(g + 1) * b]
            g1 = min(ref[p]['gaps'][y][0] for y in range(G))
            g2 = ref[p]['gaps'][g][1]
            wp = max(wp, float(np.linalg.norm(F @ np.conj(F).T - F64 @ np.conj(F64).T, 2) / (8 * nt * EPS / (g1 * g2))))
        Wr, Fr, cond = JS.baseband([x[p] for x in r['h']], ns, r['frf'][p].astype(np.complex128), group, b, flags)
        assert np.isfinite(cond).all() and (np.abs(Wr).max((0, 1)) > 0).all()
        bound = np.maximum(1e-5, 1e-6 * cond ** 2)
        ew = np.abs(r['W'][p] - Wr).max((0, 1)) / np.abs(Wr).max((0, 1))
        ef = np.abs(r['fbb'][p].astype(np.complex128) - Fr).max((1, 2)) / np.abs(Fr).max((1, 2))
        wb = max(wb, float((ew / bound).max()), float((ef / bound).max()))
    print('%s tol %s %s: projector error over 8 Nt eps / (g1 g2) %.4f, W / Fbb error over the bound %.4f' % (case, tol, mode, wp, wb))
    assert wp <= 1.0 and wb <= 1.0
    W, fbb, frf = r['W'], r['fbb'].astype(np.complex128), r['frf'].astype(np.complex128)
    assert (np.abs((np.abs(W) ** 2).sum((1, 2)) - nt) <= 1e-5 * nt).all()
    prod = np.einsum('pjq,pkqm->pmjk', frf, fbb)
    mag = np.einsum('pjq,pkqm->pmjk', np.abs(frf), np.abs(fbb))
    assert (np.abs(prod - W) <= 4.0 * (Q + 2) * 2.0 ** -24 * mag + 1e-30).all()             # W = Frf Fbb, n_rf fp32 terms each
    if mode == 'pgp':
        off = np.repeat(grp, ns)[None, :] != (np.arange(Q) // b)[:, None]                 # [n_rf, M]
        assert (r['fbb'][:, :, off] == 0).all() and (r['fbb'][:, :, ~off] != 0).any()


# ------------------------------------------------------------------------------------------------ 5: unit modulus
@pytest.mark.parametrize('case', CASES)
def test_5_unit_modulus(pkg, oracle, case):
    """every entry of modulus 1 / sqrt(Nt) to 4 eps; the entries are exp(i arg) of the plain beams.  Against fp64: the beams of the nulled
    covariance rebuilt from the device's own U*, column phases aligned; a residual of 4 Nt eps l_0 turns an eigenvector by at most that
    over its absolute gap, which moves the phase of an entry of modulus |f| by at most the turn over |f|.  Entries below 1e-2 of the
    column maximum are left out."""
    nt, nr, nu, ns, group, r_star, b = case
    e, h = _engine(pkg, nt, nr), channels(case)
    plain = _run(pkg, case, 0.0, 'pgp')
    frf = e.mu_jsdm_precoder(h, ns, r_star, b, groups=group, rank_tol=0.0, mode='pgp', unit_modulus=True, keep_frf=True)[2]
    a = np.abs(frf.astype(np.complex128))
    assert np.abs(a * np.sqrt(nt) - 1).max() <= 4 * EPS
    want = plain['frf'].astype(np.complex128)
    ok = np.abs(want) > 0
    assert np.abs(frf * np.sqrt(nt) - want / np.where(ok, np.abs(want), 1))[ok].max() <= 8 * EPS and (frf[~ok] == np.float32(1 / np.sqrt(nt))).all()
    grp, G = _groups(case)
    worst, skipped = 0.0, 0
    for p in range(_npkt(case)):
        for g in range(G):
            Rt, _ = _nulled_dev(plain, case, p, g)
            lt, Vt = JS.eig_desc(Rt)
            l0 = float(plain['eig'][p, g, 0])
            for q in range(b):
                gap = min(lt[q] - lt[q + 1] if q + 1 < nt else np.inf, lt[q - 1] - lt[q] if q else np.inf)
                f64, f = Vt[:, q], frf[p][:, g * b + q].astype(np.complex128) * np.sqrt(nt)
                keep = np.abs(f64) >= 1e-2 * np.abs(f64).max()
                skipped += int((~keep).sum())
                u64 = f64 / np.abs(f64).clip(1e-300)
                rot = np.vdot(u64[keep], f[keep])
                rot /= abs(rot)
                turn = 4 * nt * EPS * l0 / gap
                worst = max(worst, float((np.abs(f - u64 * rot)[keep] / (2 * turn / np.abs(f64[keep]) + 8 * EPS)).max()))
    print('%s: unit-modulus entries against fp64, over the bound: %.3f; entries left out %d' % (case, worst, skipped))
    assert worst <= 1.0 and skipped == 0


# ------------------------------------------------------------------------------------------------ 6, 7: identities, through the link
def confined(npkt=3, seed=11):
    """identity (a): Nt = 16, two users on unitary DFT columns 0-3 and 6-9, Gaussian coefficients of variance 0.5^i"""
    nt, nr = 16, 2
    rng = np.random.default_rng(seed)
    F = JS.dft(nt)
    out = []
    for cols in (np.arange(0, 4), np.arange(6, 10)):
        z = (rng.standard_normal((npkt, nr, 4, N)) + 1j * rng.standard_normal((npkt, nr, 4, N))) / np.sqrt(2.0)
        out.append(_f32(np.einsum('jc,pick->pijk', F[:, cols], z * np.sqrt(0.5 ** np.arange(4))[None, None, :, None])))
    return out


def _against_digital(e, h, ns, W):
    Wd = e.mu_precoder(h, ns).astype(np.complex128)
    worst = 0.0
    for p in range(h[0].shape[0]):
        cond = MU.precoder([x[p] for x in h], ns, 0.0)[1]
        err = np.abs(W[p] - Wd[p]).max((0, 1)) / np.abs(Wd[p]).max((0, 1))
        worst = max(worst, float((err / (2.0 * np.maximum(1e-5, 1e-6 * cond ** 2))).max()))
    return worst, Wd


def test_6_identities_against_the_digital_precoder(pkg, oracle):
    """(a) users confined to disjoint sets of DFT beams, (r_star, b) = (4, 4), n_rf = 8 < Nt: W is the digital precoder's in both modes.
    (b) one group with b = Nt = 8, r_star = 0: Frf is unitary and W is the digital precoder's.  Both kernels within their yardsticks of
    fp64, so within the sum of the two of each other."""
    h = confined()
    e = _engine(pkg, 16, 2)
    for mode in MODES:
        w_re, w_im, frf = e.mu_jsdm_precoder(h, 2, 4, 4, rank_tol=0.0, mode=mode, keep_frf=True)
        worst, _ = _against_digital(e, h, 2, w_re.astype(np.float64) + 1j * w_im)
        print('(a) %s: JSDM on confined users against the digital precoder: largest deviation over the two yardsticks %.4f' % (mode, worst))
        assert worst <= 1.0
    rng = np.random.default_rng(21)
    nt, nr, npkt = 8, 2, 3
    h8 = [_f32((rng.standard_normal((npkt, nr, nt, N)) + 1j * rng.standard_normal((npkt, nr, nt, N))) / np.sqrt(2.0)) for _ in range(2)]
    e8 = _engine(pkg, nt, nr)
    for mode in MODES:
        w_re, w_im, frf = e8.mu_jsdm_precoder(h8, 2, 0, 8, groups=[0, 0], mode=mode, keep_frf=True)
        F = frf.astype(np.complex128)
        assert np.abs(np.einsum('pjq,pjr->pqr', np.conj(F), F) - np.eye(nt)).max() <= 4 * nt * EPS
        worst, _ = _against_digital(e8, h8, 2, w_re.astype(np.float64) + 1j * w_im)
        print('(b) %s: one group, b = Nt: largest deviation over the two yardsticks %.4f' % (mode, worst))
        assert worst <= 1.0


def test_7_through_the_existing_link(pkg, oracle):
    """true = estimated planes, reg = 0, noise 60 dB under a stream's mean power: no bit error for either set of users in either mode -
    also where per-group processing leaves the other groups' interference to the analog stage (the prescribed planes, 2 of 8 directions
    nulled: 5 ... 12 dB, which rate-1/3 coded QPSK still decodes).  B W = diag(c) for the joint form and the digital V is the minimum-norm
    solution: JGP sinr_db is never above the digital one by more than 1e-3 dB; PGP on the confined users (where it is the digital
    precoder) within 0.01 dB of it."""
    for name, (nt, nr), h, ns, kw in (('confined', (16, 2), confined(), 2, dict(r_star=4, n_beams=4, rank_tol=0.0)),
                                      ('prescribed', SMALL[:2], channels(SMALL), 1, dict(r_star=2, n_beams=2, groups=SMALL[4], rank_tol=0.0))):
        e = _engine(pkg, nt, nr)
        nu = len(h)
        Wd = e.mu_precoder(h, ns)
        nv = np.float32(1e-6 * nt / (nu * ns) * np.mean([np.abs(x[:, :ns]) ** 2 for x in h]))
        dig = e.mu_link_sim(h, Wd, nv, seed=3, first_pkt=1, ns=ns, n_sym=1, bps=2)
        for mode in MODES:
            w_re, w_im = e.mu_jsdm_precoder(h, ns, mode=mode, **kw)[:2]
            got = e.mu_link_sim(h, (w_re + 1j * w_im).astype(np.complex64), nv, seed=3, first_pkt=1, ns=ns, n_sym=1, bps=2)
            print('%s %s: sinr_db JSDM %s, digital %s' % (name, mode, np.round(got.sinr_db.astype(np.float64), 3).tolist(),
                                                          np.round(dig.sinr_db.astype(np.float64), 3).tolist()))
            print('    bit errors %s' % got.bit_errors.tolist())
            assert np.isfinite(got.sinr_db).all() and got.bit_errors.shape == (nu, h[0].shape[0]) and (got.bit_errors == 0).all()
            if mode == 'jgp':
                assert (got.sinr_db <= dig.sinr_db + 1e-3).all()
            if name == 'confined':
                assert (np.abs(got.sinr_db - dig.sinr_db) <= 0.01).all()


# ------------------------------------------------------------------------------------------------ 8: robustness
SHAPES = ('w_re', 'w_im', 'frf_re', 'frf_im', 'fbb_re', 'fbb_im', 'eig', 'ustar_re', 'ustar_im', 'rank')


def _shapes(case, npkt):
    nt, nr, nu, ns, group, r_star, b = case
    G = _groups(case)[1]
    m, q = nu * ns, G * b
    return [(npkt, m, nt, N), (npkt, m, nt, N), (npkt, nt, q), (npkt, nt, q), (npkt, N, q, m), (npkt, N, q, m), (npkt, G, nt), (npkt, G, nt, r_star),
            (npkt, G, nt, r_star), (npkt, G, 2)]


def _device_call(e, case, h, tol=0.3, flags=1, reg=None, keep=(True,) * 5, cov=None):
    """one csi_mu_jsdm_precoder_device call over fresh DeviceArrays -> the ten outputs as uint32 words (None where not kept); keep: frf,
    fbb, eig, ustar, rank"""
    nt, nr, nu, ns, group, r_star, b = case
    npkt = h[0].shape[0]
    ins = [e.to_device(np.ascontiguousarray(x.real, np.float32)) for x in h] + [e.to_device(np.ascontiguousarray(x.imag, np.float32)) for x in h]
    d_reg = e.to_device(np.ascontiguousarray(reg, np.float32)) if reg is not None else None
    d_cov = [None, None] if cov is None else [e.to_device(np.ascontiguousarray(cov.real, np.float32)), e.to_device(np.ascontiguousarray(cov.imag, np.float32))]
    want = [True, True, keep[0], keep[0], keep[1], keep[1], keep[2], keep[3], keep[3], keep[4]]
    outs = [e.empty(s) if k else None for s, k in zip(_shapes(case, npkt), want)]
    e.mu_jsdm_precoder_device(ins[:nu], ins[nu:], npkt, ns, r_star, b, outs[0], outs[1], group, tol, flags, d_reg, d_cov[0], d_cov[1], *outs[2:])
    e.synchronize()
    res = [None if o is None else o.download().view(np.uint32) for o in outs]
    for a in ins + outs + d_cov + [d_reg]:
        if a is not None:
            a.free()
    return res


def _same(full, got, sl=slice(None)):
    return all(np.array_equal(a[sl], b) for a, b in zip(full, got) if b is not None)


def test_8a_repeats_ranges_chunks_contexts_and_optional_outputs_bit_for_bit(pkg, oracle):
    case = CASES[3]
    nt, nr, nu, ns, group, r_star, b = case
    npkt = _npkt(case)
    e = _engine(pkg, nt, nr)
    h = channels(case)
    reg = (0.05 + 0.1 * np.arange(npkt)).astype(np.float32)
    full = _device_call(e, case, h, reg=reg)
    assert _same(full, _device_call(e, case, h, reg=reg))                                   # a repeat call
    assert _same(full, _device_call(e, case, [x[2:5] for x in h], reg=reg[2:5]), slice(2, 5))       # packets 2 .. 4 alone
    for keep in ((False,) * 5, (True, False, False, False, False), (False, True, False, True, False), (False, False, True, False, True)):
        assert _same(full, _device_call(e, case, h, reg=reg, keep=keep)), keep               # optional outputs kept or not
    # the covariance handed back in: the same bits as the internal step, one launch fewer
    cov = e.mu_covariance(h)
    n0 = e.get_option('mu_launches')
    assert _same(full, _device_call(e, case, h, reg=reg, cov=cov))
    assert e.get_option('mu_launches') == n0 + 3
    # a workspace of less than one packet: one packet per chunk, four launches each
    small = _engine(pkg, nt, nr, workspace_bytes=1024)
    n0 = small.get_option('mu_launches')
    assert _same(full, _device_call(small, case, h, reg=reg))
    assert small.get_option('mu_launches') == n0 + 4 * npkt
    assert _same(full, _device_call(small, case, h, reg=reg, keep=(False,) * 5))
    # a bf16 context is served with the same bits
    assert _same(full, _device_call(_engine(pkg, nt, nr, dtype='bf16'), case, h, reg=reg))
    # the flags reach the kernels: joint processing and unit modulus change the result
    assert not np.array_equal(full[0], _device_call(e, case, h, reg=reg, flags=0)[0])
    assert not np.array_equal(full[2], _device_call(e, case, h, reg=reg, flags=3)[2])


def test_8b_capture_and_replay(pkg, oracle):
    case = SMALL
    nt, nr, nu, ns, group, r_star, b = case
    npkt = _npkt(case)
    e = pkg.CsiEngine(nt, nr, hidden=(8,), device=0)
    h = channels(case)
    ins = [e.to_device(np.ascontiguousarray(x.real, np.float32)) for x in h] + [e.to_device(np.ascontiguousarray(x.imag, np.float32)) for x in h]
    one = [e.to_device(np.ascontiguousarray(x[:1].real, np.float32)) for x in h] + [e.to_device(np.ascontiguousarray(x[:1].imag, np.float32)) for x in h]
    eager = [e.empty(s) for s in _shapes(case, npkt)]
    o1 = [e.empty(s) for s in _shapes(case, 1)]
    call = lambda src, n, o: e.mu_jsdm_precoder_device(src[:nu], src[nu:], n, ns, r_star, b, o[0], o[1], group, 0.3, 1, None, None, None, *o[2:])
    call(one, 1, o1)                                                                       # sizes the workspace for one packet
    e.synchronize()
    n0 = e.get_option('mu_launches')
    e.capture_begin()
    try:
        call(one, 1, o1)
        with pytest.raises(pkg.CsiError, match='sized by an eager call of the same shape'):
            call(ins, npkt, eager)                                                         # five packets: the workspace would grow
    finally:
        g1 = e.capture_end()
    assert e.get_option('mu_launches') == n0 + 4
    g1.launch()
    e.synchronize()
    g1.free()
    call(ins, npkt, eager)
    e.synchronize()
    want = [a.download().view(np.uint32) for a in eager]
    replay = [e.to_device(np.zeros(s, np.float32)) for s in _shapes(case, npkt)]
    e.capture_begin()
    try:
        call(ins, npkt, replay)
    finally:
        g = e.capture_end()
    assert not any(a.download().any() for a in replay), 'a captured call must not run'
    g.launch()
    e.synchronize()
    assert all(np.array_equal(a.download().view(np.uint32), w) for a, w in zip(replay, want))
    assert _same(want, _device_call(e, case, h))
    g.free()
    for a in ins + one + eager + o1 + replay:
        a.free()
    e.close()


def test_8c_singular_items(pkg, oracle):
    """The exact singular case of DESIGN 4.22 through this entry: Nt = 4, two users of one group with identical estimated rows on
    subcarriers 40 .. 99 of packet 1, entries in {+-1, +-j}; the covariance handed in is the identity, whose eigenvectors are the unit
    vectors (no rotation is applied), so Frf = I (b = 4, r_star = 0), Gm = B and A = [[4, 4], [4, 4]]: the second pivot 4 - 4 is exact."""
    nt, nr, npkt = 4, 2, 2
    e = _engine(pkg, nt, nr)
    rng = np.random.default_rng(1)
    h = [_f32(rng.standard_normal((npkt, nr, nt, N)) + 1j * rng.standard_normal((npkt, nr, nt, N))) for _ in range(2)]
    same = np.array([1, 1j, -1, -1j])[rng.integers(0, 4, (nt, 60))]
    for x in h:
        x[1, 0, :, 40:100] = same
    cov = np.broadcast_to(np.eye(nt, dtype=np.complex64), (npkt, 2, nt, nt))
    w_re, w_im, frf, fbb = e.mu_jsdm_precoder(h, 1, 0, 4, groups=[0, 0], cov=cov, keep_frf=True, keep_fbb=True)
    assert np.array_equal(frf, np.broadcast_to(np.eye(nt, dtype=np.complex64), (npkt, nt, nt)))
    W = w_re.astype(np.float64) + 1j * w_im
    assert (W[1, :, :, 40:100] == 0).all() and (fbb[1, 40:100] == 0).all()
    assert np.isfinite(w_re).all() and np.isfinite(w_im).all() and np.isfinite(fbb.real).all() and np.isfinite(fbb.imag).all()
    keep = np.r_[0:40, 100:N]
    assert (np.abs(W[1][:, :, keep]).max((0, 1)) > 0).all() and (np.abs(W[0]).max((0, 1)) > 0).all()
    Wd = e.mu_precoder(h, 1).astype(np.complex128)
    assert (Wd[1, :, :, 40:100] == 0).all() and _against_digital(e, [x[:1] for x in h], 1, W[:1])[0] <= 1.0      # Gm = B: the digital precoder
    w_re, w_im = e.mu_jsdm_precoder(h, 1, 0, 4, groups=[0, 0], cov=cov, reg=0.25)           # reg > 0: finite and non-zero everywhere
    assert np.isfinite(w_re).all() and np.isfinite(w_im).all() and ((np.abs(w_re) + np.abs(w_im)).sum((1, 2)) > 0).all()
    z = e.mu_jsdm_precoder([np.zeros_like(x) for x in h], 1, 0, 4, groups=[0, 0], keep_fbb=True, keep_eig=True)
    assert (z[0] == 0).all() and (z[1] == 0).all() and (z[2] == 0).all() and (z[3] == 0).all() and (z[5] == 0).all()


def test_8d_guard_bands(pkg, oracle):
    """every input and output a slice between guard bands: nothing outside the arrays is written or reaches a result, inputs are not
    modified, every output element is written, and the results are those of plain arrays"""
    case = SMALL
    nt, nr, nu, ns, group, r_star, b = case
    npkt = _npkt(case)
    e, h = _engine(pkg, nt, nr), channels(case)
    plain = _device_call(e, case, h)
    gin = [Guarded(e, x.shape, 'in', np.ascontiguousarray(part, np.float32), 'h%d' % i) for i, x in enumerate(h) for part in (x.real, x.imag)]
    outs = [Guarded(e, s, 'out', name=n) for s, n in zip(_shapes(case, npkt), SHAPES)]
    e.mu_jsdm_precoder_device(gin[0::2], gin[1::2], npkt, ns, r_star, b, outs[0], outs[1], group, 0.3, 1, None, None, None, *outs[2:])
    e.synchronize()
    for a in gin + outs:
        a.check()
    assert all(a.unchanged() for a in gin) and all(a.count_unwritten() == 0 for a in outs)
    assert all(np.array_equal(a.download().view(np.uint32), w) for a, w in zip(outs, plain))
    # the planes in the workspace: the same guards around what remains; and the covariance entry point
    keep = [Guarded(e, s, 'out', name=n) for s, n in zip(_shapes(case, npkt)[:2], SHAPES)]
    gcov = [Guarded(e, (npkt, nu, nt, nt), 'out', name=n) for n in ('cov_re', 'cov_im')]
    e.mu_jsdm_precoder_device(gin[0::2], gin[1::2], npkt, ns, r_star, b, keep[0], keep[1], group, 0.3, 1)
    e.mu_covariance_device(gin[0::2], gin[1::2], npkt, gcov[0], gcov[1])
    e.synchronize()
    for a in gin + keep + gcov:
        a.check()
    assert all(a.count_unwritten() == 0 for a in keep + gcov)
    assert all(np.array_equal(a.download().view(np.uint32), w) for a, w in zip(keep, plain))
    cov = e.mu_covariance(h)
    assert np.array_equal(gcov[0].download(), cov.real) and np.array_equal(gcov[1].download(), cov.imag)
    # the covariance as a guarded input
    gc = [Guarded(e, cov.shape, 'in', np.ascontiguousarray(part, np.float32), n) for part, n in ((cov.real, 'cov_re'), (cov.imag, 'cov_im'))]
    again = [Guarded(e, s, 'out', name=n) for s, n in zip(_shapes(case, npkt)[:2], SHAPES)]
    e.mu_jsdm_precoder_device(gin[0::2], gin[1::2], npkt, ns, r_star, b, again[0], again[1], group, 0.3, 1, None, gc[0], gc[1])
    e.synchronize()
    for a in gc + again:
        a.check()
    assert all(a.unchanged() for a in gc) and all(np.array_equal(a.download().view(np.uint32), w) for a, w in zip(again, plain))
    for a in gin + outs + keep + gcov + gc + again:
        a.free()


def test_8e_refusals_carry_text_and_launch_nothing(pkg, oracle):
    nt, nr = 8, 2
    e = pkg.CsiEngine(nt, nr, hidden=(8,), device=0)
    lib, ctx = e._lib, e._ctx
    buf = e.empty((1 << 16,))
    p = buf.ptr
    n0 = e.get_option('mu_launches')

    def arr(n, null=None, off=None):
        return (ctypes.c_void_p * max(n, 8))(*[None if i == null else (p + 4 if i == off else p) for i in range(n)] + [None] * (8 - n))

    def grp(*g):
        return (ctypes.c_int32 * len(g))(*g) if g else None

    def call(text, nu=2, re=None, im=None, npkt=1, ns=1, group=None, r_star=1, b=1, tol=0.05, flags=1, reg=None, cov=(None, None), w=(p, p),
             frf=(None, None), fbb=(None, None), eig=None, ustar=(None, None), rank=None, code=-1, lib=lib, ctx=ctx):
        assert lib.csi_mu_jsdm_precoder_device(ctx, nu, arr(nu) if re is None else re, arr(nu) if im is None else im, npkt, ns, group, r_star, b, tol,
                                               flags, reg, *cov, *w, *frf, *fbb, eig, *ustar, rank) == code
        assert text in lib.csi_last_error(ctx).decode(), lib.csi_last_error(ctx)

    call('n_users 0 outside 1 .. 8', nu=0)
    call('n_users 9 outside 1 .. 8', nu=9)
    call('ns 0 outside 1 .. min(4, Nr 2)', ns=0)
    call('ns 3 outside 1 .. min(4, Nr 2)', ns=3)
    call('= 10 streams exceed min(16, Nt 8)', nu=5, ns=2, b=2)
    call('group[1] = 2 outside 0 .. G-1', group=grp(0, 2))
    call('group[0] = -1 outside 0 .. G-1', group=grp(-1, 0))
    call('group 0 of 0 .. 1 has no user', group=grp(1, 1))
    call('n_beams 0 must be at least 1', b=0)
    call('= 18 RF chains exceed 16', nu=3, b=6)
    call('streams for n_beams 1 chains', group=grp(0, 0))
    call('streams for n_beams 1 chains', ns=2)
    call('r_star -1 outside 0 .. Nt 8', r_star=-1)
    call('r_star 9 outside 0 .. Nt 8', r_star=9)
    call('directions to null leave fewer than n_beams 2 of Nt 8', r_star=7, b=2)
    call('rank_tol -0.1 must be finite and not negative', tol=-0.1)
    call('must be finite and not negative', tol=float('nan'))
    call('must be finite and not negative', tol=float('inf'))
    call('unknown flag bits 0x4', flags=4)
    call('must not be negative', npkt=-1)
    call('null required pointer (d_hest_re[1])', re=arr(2, null=1))
    call('null required pointer (d_hest_im[0])', im=arr(2, null=0))
    call('null required pointer (d_hest_re)', re=ctypes.cast(None, ctypes.POINTER(ctypes.c_void_p)))
    call('must start on a 16-byte boundary', re=arr(2, off=1))
    call('null required pointer (w_re, w_im)', w=(None, p))
    call('null required pointer (w_re, w_im)', w=(p, None))
    call('d_w_re must start on a 16-byte boundary', w=(p + 4, p))
    for name in ('cov', 'frf', 'fbb', 'ustar'):
        call('the %s planes come as a pair' % name, **{name: (p, None)})
        call('the %s planes come as a pair' % name, **{name: (None, p)})
        call('d_%s_re must start on a 16-byte boundary' % name, **{name: (p + 4, p)})
        call('d_%s_im must start on a 16-byte boundary' % name, **{name: (p, p + 8)})
    call('d_eig must start on a 16-byte boundary', eig=p + 4)
    call('d_reg / d_rank must be aligned', rank=p + 2)
    wide = pkg.CsiEngine(68, 2, hidden=(8,), device=0)
    call('Nt 68 exceeds 64', lib=wide._lib, ctx=wide._ctx)
    assert wide._lib.csi_mu_covariance_device(wide._ctx, 2, arr(2), arr(2), 1, p, p) == -1 and 'Nt 68 exceeds 64' in wide._lib.csi_last_error(wide._ctx).decode()
    one = pkg.CsiEngine(0, 1, hidden=(16,), len_ltf=64)
    call('single-input context', nu=1, lib=one._lib, ctx=one._ctx)
    for kw, text in ((dict(nu=0), 'n_users 0 outside 1 .. 8'), (dict(npkt=-1), 'must not be negative'), (dict(cov=(None, p)), 'null required pointer (cov_re, cov_im)'),
                     (dict(cov=(p + 4, p)), 'd_cov_re must start on a 16-byte boundary'), (dict(re=arr(2, null=0)), 'null required pointer (d_hest_re[0])')):
        a = dict(nu=2, re=arr(2), im=arr(2), npkt=1, cov=(p, p))
        a.update(kw)
        assert lib.csi_mu_covariance_device(ctx, a['nu'], a['re'], a['im'], a['npkt'], *a['cov']) == -1
        assert text in lib.csi_last_error(ctx).decode(), lib.csi_last_error(ctx)
    assert lib.csi_mu_covariance_device(None, 2, arr(2), arr(2), 1, p, p) == -1 and lib.csi_mu_covariance_device(ctx, 2, None, None, 0, None, None) == 0
    # an open capture that would have to grow the workspace (no eager call yet)
    e.capture_begin()
    try:
        call('sized by an eager call of the same shape')
    finally:
        e.capture_end().free()
    assert lib.csi_mu_jsdm_precoder_device(ctx, 2, None, None, 0, 1, None, 1, 1, 0.05, 1, *[None] * 13) == 0           # nothing to do
    assert lib.csi_mu_jsdm_precoder_device(None, 2, None, None, 1, 1, None, 1, 1, 0.05, 1, *[None] * 13) == -1          # a null context
    e.synchronize()
    assert e.get_option('mu_launches') == n0 and wide.get_option('mu_launches') == 0 and one.get_option('mu_launches') == 0
    with pytest.raises(pkg.CsiError, match='every h must be'):
        e.mu_jsdm_precoder([np.zeros((1, nr, nt, 7), np.complex64)], 1, 1, 1)
    with pytest.raises(pkg.CsiError, match="not 'pgp' or 'jgp'"):
        e.mu_jsdm_precoder([np.zeros((1, nr, nt, N), np.complex64)], 1, 1, 1, mode='x')
    buf.free()
    for x in (e, wide, one):
        x.close()


def test_8f_threshold_above_every_ratio_and_dependent_groups(pkg, oracle):
    """rank_tol so large that r_g = 0: no nulling, q_g = 0, the beams are the covariance's own leading eigenvectors.  Two groups with
    identical planes beside a third: the dependent columns are dropped, q_g = r_g of one."""
    case = SMALL
    nt, nr, nu, ns, group, r_star, b = case
    e, h = _engine(pkg, nt, nr), channels(case)
    out = e.mu_jsdm_precoder(h, ns, r_star, b, groups=group, rank_tol=1.5, keep_frf=True, keep_eig=True)
    frf, eig, ustar, rank = out[2], out[3], out[4], out[5]
    assert (rank == 0).all() and (ustar == 0).all()
    zero = e.mu_jsdm_precoder(h, ns, 0, b, groups=group, keep_frf=True)[2]
    assert np.array_equal(frf, zero)                                                      # the same as nulling no direction at all
    hh = [h[0], h[0], h[1]]
    out = e.mu_jsdm_precoder(hh, 1, 2, 2, rank_tol=0.0, mode='jgp', keep_frf=True, keep_eig=True)
    frf, ustar, rank = out[2], out[4], out[5]
    assert (rank[:, :, 0] == 2).all() and (rank[:, 2, 1] == 2).all() and (rank[:, :2, 1] == 4).all(), rank.tolist()
    assert np.array_equal(ustar[:, 0], ustar[:, 1])
    for p in range(frf.shape[0]):
        F = frf[p][:, 4:6].astype(np.complex128)
        assert np.sqrt((np.abs(np.conj(ustar[p, 0].astype(np.complex128)).T @ F) ** 2).sum()) <= 8 * nt * EPS


def test_8g_sweep_miniature(pkg, oracle, tmp_path):
    """two users at Nt = 8 with --muJSDM 2 beside --muHybrid 4: the new fields behind every other, everything else unchanged"""
    import json
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    out, out2 = str(tmp_path / 'muj'), str(tmp_path / 'muh')
    common = ['--nTX', '8', '--nRX', '2', '--nn', '16', '--trainPkts', '24', '--testPkts', '6', '--snr', '20', '--epochs', '1',
              '--bs', '16', '--quiet', '--ber', '--numSTS', '1', '--rays', '32', '--dataSymbols', '2', '--users', '2', '--muHybrid', '4']
    assert sweep.main(['-d', out] + common + ['--muJSDM', '2', '--jsdmRank', '2']) == 0
    assert sweep.main(['-d', out2, '--modeldir', out] + common) == 0
    res, res2 = json.load(open(os.path.join(out, 'sweep.json'))), json.load(open(os.path.join(out2, 'sweep.json')))
    assert res['mu_jsdm'] == dict(b=2, r_star=2, tol=0.05, mode='pgp') and 'mu_jsdm' not in res2 and res['mu'] == res2['mu']
    m = loadmat(os.path.join(out, 'BS8_SNR20', 'metrics.mat'))
    m2 = loadmat(os.path.join(out2, 'BS8_SNR20', 'metrics.mat'))
    new = [f + x for x in sweep.SOURCES for f in sweep.MUJ_FIELDS]
    old = sorted(k for k in m2 if not k.startswith('__'))
    assert sorted(k for k in m if not k.startswith('__')) == sorted(old + new)
    written = sweep.metric_fields({k: m[k] for k in m if not k.startswith('__')})
    assert written[:len(old)] == sweep.metric_fields({k: m2[k] for k in old}) and written[len(old):] == new
    for k in old:
        assert np.array_equal(m[k], m2[k]), k                                            # every other field is unchanged
    for k in new:
        assert m[k].shape == (1, 6) and np.isfinite(m[k]).all(), k
    lv, lv2 = res['levels'][0], res2['levels'][0]
    assert set(lv2) == set(lv) - set(new) - {'muj_users'} and lv['mu_users'] == lv2['mu_users'] and lv['muh_users'] == lv2['muh_users']
    for x in sweep.SOURCES:
        per = lv['muj_users'][x]
        assert np.asarray(per['bers']).shape == (2, 6) and 0 <= per['r_g'] <= 2 and 0 <= per['q_g'] <= 2
        assert np.allclose(np.mean(per['bers'], 0), m['bersMUJ_' + x][0]) and np.allclose(np.mean(per['sinr'], 0), m['sinrMUJ_' + x][0])
    dig, hyb, jsd = (np.asarray(lv[k]['perfect']['sinr']) for k in ('mu_users', 'muh_users', 'muj_users'))
    print('20 dB, two users: sinr_db perfect CSI digital %s, hybrid (4 chains) %s, JSDM (2 x 2 chains, pgp) %s'
          % (np.round(dig.mean(1), 2).tolist(), np.round(hyb.mean(1), 2).tolist(), np.round(jsd.mean(1), 2).tolist()))
