"""CPU tests of the multi-user JSDM precoder (csi_mu_covariance_device, csi_mu_jsdm_precoder_device, csrc/mu_jsdm.hip.h):
the C-ABI surface, the sweep's --muJSDM arguments, and the fp64 restatement tests/jsdm_ref.py against known answers - the digital
precoder of tests/mu_link_ref.py where the identities hold, the deflation property on a scattering channel (tests/scatter_ref.py), the
threshold counts and the Gram-Schmidt drop rule."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mu_link_ref as MU      # noqa: E402
import jsdm_ref as JS         # noqa: E402

N = MU.N


def test_entry_points_in_header_table_and_library(pkg):
    pkg.build_library()
    lib = pkg.load_library()
    header = open(os.path.join(REPO, 'include', 'csi_mamimo.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(csi_[a-z0-9_]+)\s*\(', header))
    from dl_channel_estimation_mamimo_amd import _lib
    for name, nargs in (('csi_mu_covariance_device', 7), ('csi_mu_jsdm_precoder_device', 24)):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
        assert len(_lib.SYMBOLS[name][1]) == nargs                                         # the prototype of the header, argument by argument
        proto = re.search(r'\b%s\s*\(([^;]*)\);' % name, header).group(1)
        assert len(proto.split(',')) == nargs
    assert lib.csi_abi_version() == 1            # the change is additive
    blob = open(pkg.library_path(), 'rb').read()
    for k in (b'mu_cov_kernel', b'mu_jsdm_eig_kernel', b'mu_jsdm_baseband_kernel'):
        assert k in blob, k
    for m in ('mu_covariance', 'mu_covariance_device', 'mu_jsdm_precoder', 'mu_jsdm_precoder_device'):
        assert hasattr(pkg.CsiEngine, m), m
    names = [lib.csi_profile_kernel_name(i).decode() for i in range(lib.csi_profile_num_kernels())]
    assert all(n in names for n in ('mu_cov', 'mu_jsdm_eig', 'mu_jsdm_baseband'))
    assert lib.csi_mu_covariance_device(None, 2, None, None, 1, None, None) == -1          # a null context
    assert lib.csi_mu_jsdm_precoder_device(None, 2, None, None, 1, 1, None, 1, 1, 0.05, 1, *[None] * 13) == -1


def test_sweep_arguments_and_field_order():
    from dl_channel_estimation_mamimo_amd import sweep
    args = sweep.parse_args(['-d', 'x', '--ber', '--users', '2', '--muJSDM', '2'])
    assert args.muJSDM == 2 and args.jsdmRank == 4 and args.jsdmTol == 0.05 and args.jsdmMode == 'pgp'
    assert sweep.parse_args(['-d', 'x', '--ber', '--users', '2']).muJSDM == 0
    args = sweep.parse_args(['-d', 'x', '--ber', '--users', '4', '--numSTS', '2', '--muJSDM', '4', '--jsdmRank', '8', '--jsdmTol', '0.2', '--jsdmMode', 'jgp'])
    assert (args.muJSDM, args.jsdmRank, args.jsdmTol, args.jsdmMode) == (4, 8, 0.2, 'jgp')
    for bad in (['--muJSDM', '2'], ['--ber', '--muJSDM', '2'], ['--users', '2', '--muJSDM', '2'],
                ['--ber', '--users', '2', '--numSTS', '2', '--muJSDM', '1'],                  # numSTS > B
                ['--ber', '--users', '5', '--muJSDM', '4'],                                    # U B > 16
                ['--ber', '--users', '4', '--nTX', '16', '--muJSDM', '2', '--jsdmRank', '5'],  # (U-1) R > nTX - B
                ['--ber', '--users', '2', '--nTX', '128', '--muJSDM', '2'],                    # nTX > 64
                ['--ber', '--users', '2', '--muJSDM', '2', '--jsdmMode', 'x'], ['--ber', '--users', '2', '--muJSDM', '2', '--jsdmTol', '-1'],
                ['--ber', '--users', '2', '--muJSDM', '2', '--jsdmRank', '-1']):
        with pytest.raises(SystemExit):
            sweep.parse_args(['-d', 'x'] + bad)
    one = np.zeros(3)
    mse = {'MSE_' + e: one for e in sweep.ESTIMATORS}
    mse.update({f + x: one for x in sweep.SOURCES for f in sweep.LINK_FIELDS}, MSE_perfect=one)
    mse.update({f + x: one for x in sweep.SOURCES for f in sweep.MU_FIELDS})
    mse.update({f + x: one for x in sweep.SOURCES for f in sweep.MUH_FIELDS})
    before = sweep.metric_fields(mse)
    assert sweep.MUJ_FIELDS == ('bersMUJ_', 'EVM_rmsMUJ_', 'sinrMUJ_')
    mse.update({f + x: one for x in sweep.SOURCES for f in sweep.MUJ_FIELDS})
    after = sweep.metric_fields(mse)
    assert after[:len(before)] == before and after[len(before):] == [f + x for x in sweep.SOURCES for f in sweep.MUJ_FIELDS]
    with pytest.raises(ValueError, match='mu_jsdm needs the multi-user data phase'):
        sweep.run_sweep(None, '/nonexistent', mu_jsdm=dict(b=2))


def _confined(rng):
    """Nt = 16, two users on unitary DFT columns 0-3 and 6-9, Gaussian coefficients of variance 0.5^i"""
    F = JS.dft(16)
    out = []
    for cols in (np.arange(0, 4), np.arange(6, 10)):
        z = (rng.standard_normal((2, 4, N)) + 1j * rng.standard_normal((2, 4, N))) / np.sqrt(2.0)
        out.append(np.einsum('jc,ick->ijk', F[:, cols], z * np.sqrt(0.5 ** np.arange(4))[None, :, None]))
    return out


@pytest.mark.parametrize('flags', [0, JS.PGP])
def test_identity_confined_users_give_the_digital_precoder(flags):
    """(a): users confined to disjoint sets of DFT beams, ns = 2, (r_star, b) = (4, 4), n_rf = 8 < Nt"""
    h = _confined(np.random.default_rng(11))
    W, Fbb, cond, an = JS.precoder(h, 2, None, 4, 4, 0.0, flags)
    Wd, _ = MU.precoder(h, 2, 0.0)
    assert an['Frf'].shape == (16, 8) and an['rank'].tolist() == [[4, 4], [4, 4]]
    assert np.abs(W - Wd).max() <= 1e-12 * np.abs(Wd).max()
    if flags & JS.PGP:
        assert (Fbb[:, :4, 2:] == 0).all() and (Fbb[:, 4:, :2] == 0).all()


@pytest.mark.parametrize('flags', [0, JS.PGP])
def test_identity_one_group_with_every_chain_is_the_digital_precoder(flags):
    """(b): one group with b = Nt = 8, r_star = 0: Frf is unitary"""
    rng = np.random.default_rng(3)
    h = [rng.standard_normal((2, 8, N)) + 1j * rng.standard_normal((2, 8, N)) for _ in range(2)]
    W, Fbb, cond, an = JS.precoder(h, 2, [0, 0], 0, 8, 0.05, flags)
    F = an['Frf']
    assert np.abs(np.conj(F).T @ F - np.eye(8)).max() <= 1e-12 and an['rank'].tolist() == [[0, 0]]
    Wd, _ = MU.precoder(h, 2, 0.0)
    assert np.abs(W - Wd).max() <= 1e-12 * np.abs(Wd).max()
    assert np.abs(np.einsum('jq,kqm->mjk', F, Fbb) - W).max() <= 1e-12 * np.abs(W).max()
    assert np.abs((np.abs(W) ** 2).sum((0, 1)) - 8).max() <= 1e-12 * 8


def _scattering_users(nt=32, nr=4, nu=4, spacing=15.0, seed=2):
    """four users 15 degrees apart on the scattering channel of tests/scatter_ref.py, 100 scatterers each, the 234 data carriers"""
    import scatter_ref as SR
    from oracle import csi_oracle
    bins = np.asarray(csi_oracle.data_carrier_indices()) - 1
    out = []
    for u in range(nu):
        _, box, g = SR.draws(seed + u, 0, 100)
        geo = SR.geometry(box, 100.0, spacing * (u - (nu - 1) / 2.0), 0.0, 0.1, 100e6)
        out.append(np.fft.fftshift(SR.response(g, geo, nr, nt), axes=-1)[..., bins])
    return out


def test_deflation_keeps_the_beams_in_the_null_space():
    """(r_star, b) = (8, 4) on the scattering channel: 24 directions nulled of 32, and a user's covariance has about five eigenvalues of
    weight - P R P has rank below b there, and its trailing 'leading' eigenvectors are arbitrary in its null space, which holds span(Q).
    With the deflation term the leakage |Q_g^H F_g| is rounding; without it, it is not."""
    h = _scattering_users()
    with_term = JS.analog(h, None, 8, 4, 0.0)
    plain = JS.analog(h, None, 8, 4, 0.0, deflate=False)
    # no threshold: every user hands over eight directions, most of them junk of weight 1e-17 l_0 - where two users' junk happens to be
    # dependent to 1e-3 the Gram-Schmidt drops a column, so q_g is 24 at the most
    assert (with_term['rank'][:, 0] == 8).all() and (with_term['rank'][:, 1] <= 24).all() and (with_term['rank'][:, 1] >= 16).all()
    leak = lambda an: max(np.abs(np.conj(an['Q'][g]).T @ an['Frf'][:, 4 * g:4 * g + 4]).max() for g in range(4))
    assert leak(with_term) < 1e-12
    assert leak(plain) > 1e-9, leak(plain)                                                # how far is chance: orders above rounding on this draw
    # a direction the Gram-Schmidt dropped lies within 1e-3 of span(Q_g): that is what is left of it in the beams
    ustar = lambda an: max(np.abs(np.conj(an['ustar'][y]).T @ an['Frf'][:, 4 * g:4 * g + 4]).max() for g in range(4) for y in range(4) if y != g)
    assert ustar(with_term) <= 1e-3
    for g in range(4):
        F = with_term['Frf'][:, 4 * g:4 * g + 4]
        assert np.abs(np.conj(F).T @ F - np.eye(4)).max() < 1e-12


def test_threshold_counts_and_margins():
    lam = np.array([1.0, 0.5, 0.2, 0.04, 0.01])
    assert JS.kept_rank(lam, 4, 0.0) == 4 and JS.kept_rank(lam, 5, 0.05) == 3 and JS.kept_rank(lam, 2, 0.05) == 2
    assert JS.kept_rank(lam, 4, 0.2) == 2                                                # l_i > tol l_0, not >=
    assert JS.kept_rank(lam, 4, 1.0) == 0 and JS.kept_rank(lam, 0, 0.0) == 0
    assert JS.kept_rank(np.array([0.0, 0.0]), 2, 0.0) == 0 and JS.kept_rank(np.array([-1.0, -2.0]), 2, 0.0) == 0
    assert JS.kept_rank(np.array([np.nan, 1.0]), 2, 0.0) == 0 and JS.kept_rank(np.array([np.inf, 1.0]), 2, 0.0) == 0
    # the prescribed planes of the GPU tests: 0.6^j, so 0.3 keeps three of four directions (0.6^2 = 0.36 > 0.3 > 0.216)
    h = [x[0] for x in JS.planes(32, 4, 4, 1)]
    an = JS.analog(h, None, 4, 4, 0.3)
    assert an['rank'][:, 0].tolist() == [3, 3, 3, 3] and an['rank'][:, 1].tolist() == [9, 9, 9, 9]
    assert an['gaps'].min() > 1e-3 and an['margin'].min() > 1e-3
    an32 = JS.analog(h, None, 4, 4, 0.3, dtype=np.complex64)
    assert an32['Frf'].dtype == np.complex64 and np.array_equal(an32['rank'], an['rank'])
    # the covariance: Hermitian, a beam's mean gain, the group mean
    R = an['cov']
    assert np.abs(R - np.conj(R.transpose(0, 2, 1))).max() <= 1e-15
    w = np.random.default_rng(0).standard_normal(32) + 0j
    gain = np.mean(np.abs(np.einsum('ijk,j->ik', h[1], w)) ** 2)
    assert abs(np.real(np.conj(w) @ R[1] @ w) - gain) <= 1e-12 * gain
    two = JS.analog(h, [0, 0, 1, 1], 2, 2, 0.0)
    assert np.abs(two['Rg'][0] - (R[0] + R[1]) / 2).max() <= 1e-15 and len(two['Rg']) == 2
    # the phase convention and unit modulus
    for g in range(4):
        for V in (an['ustar'][g], an['Frf'][:, 4 * g:4 * g + 4]):
            j = np.argmax(np.abs(V), 0)
            top = V[j, np.arange(V.shape[1])]
            assert (top.imag == 0).all() and (top.real > 0).all()
    um = JS.analog(h, None, 4, 4, 0.3, JS.UNIT)['Frf']
    assert np.abs(np.abs(um) - 1 / np.sqrt(32)).max() <= 1e-15
    assert JS.unit_modulus(np.array([[0.0 + 0j], [2j]]))[:, 0].tolist() == [1 / np.sqrt(2), 1j / np.sqrt(2)]


def test_gram_schmidt_drop_rule():
    rng = np.random.default_rng(4)
    X = rng.standard_normal((8, 3)) + 1j * rng.standard_normal((8, 3))
    Q = JS.gram_schmidt(X)
    assert Q.shape == (8, 3) and np.abs(np.conj(Q).T @ Q - np.eye(3)).max() <= 1e-14
    assert np.abs(Q @ (np.conj(Q).T @ X) - X).max() <= 1e-13                               # the same span
    # a copy, a combination and a zero column are dropped; a column 2e-3 away from the span is kept, one 5e-4 away is not
    unit = Q[:, 0]
    far = rng.standard_normal(8) + 0j
    far -= Q @ (np.conj(Q).T @ far)
    far /= np.linalg.norm(far)
    for eps, kept in ((2e-3, 1), (5e-4, 0)):
        v = unit + eps * far
        Y = np.concatenate([X, X[:, :1], (X[:, 1] - 2j * X[:, 2])[:, None], np.zeros((8, 1)), v[:, None]], 1)
        assert JS.gram_schmidt(Y).shape[1] == 3 + kept, eps
    assert JS.gram_schmidt(np.zeros((8, 0), complex)).shape == (8, 0)
    # the nulled covariance: span(Q) at -l_0, the rest is R restricted to the complement
    R = JS.covariance(rng.standard_normal((2, 8, N)) + 1j * rng.standard_normal((2, 8, N)))
    l0 = np.linalg.eigvalsh(R)[-1]
    Rt = JS.nulled(R, Q, l0)
    assert np.abs(Rt @ Q + l0 * Q).max() <= 1e-13 and np.abs(Rt - np.conj(Rt).T).max() == 0
    lt = np.linalg.eigvalsh(Rt)
    assert np.abs(lt[:3] + l0).max() <= 1e-13 and lt[3] >= -1e-13


@pytest.mark.parametrize('nt', [4, 6, 7, 12, 64])
def test_round_robin_ordering_meets_every_pair_once_per_sweep(nt):
    """the eigen kernel's ordering (jsdm_ref.round_robin restates it): per step disjoint pairs over n' = nt rounded up to even; over the
    n' - 1 steps of a sweep every pair of indices exactly once; with an odd nt exactly one index sits out per step, each index once"""
    n2 = (nt + 1) & ~1
    seen, sat_out = [], []
    for t in range(n2 - 1):
        pairs = JS.round_robin(nt, t)
        assert len(pairs) == n2 // 2 and all(0 <= p < q < n2 for p, q in pairs)
        assert sorted(i for pq in pairs for i in pq) == list(range(n2))                   # disjoint, and every index of n' in one pair
        real = [pq for pq in pairs if pq[1] < nt]
        assert len(real) == nt // 2                                                       # at most Nt / 2 rotations per step
        seen += real
        sat_out += [p for p, q in pairs if q >= nt]
    assert sorted(seen) == [(p, q) for p in range(nt) for q in range(p + 1, nt)]
    assert sorted(sat_out) == (list(range(nt)) if nt % 2 else [])


@pytest.mark.parametrize('nt,nr', [(6, 2), (7, 2), (12, 2)])
def test_float32_jacobi_of_the_kernel_against_eigh(nt, nr):
    """The solver of mu_jsdm_eig_kernel restated in float32 (jsdm_ref.jacobi_f32), at the sizes no context reaches (csi_create serves Nt
    in multiples of 4: 6 is even and no multiple, 7 is odd and takes the sit-out path) beside one the GPU tests run.  On the covariances
    and the nulled covariances of the prescribed planes, with eps = 2^-23 and l_0 the largest eigenvalue, the bounds of the GPU tests:
    residual |R v - l v|_2 <= 4 Nt eps l_0, orthonormality within 4 Nt eps, eigenvalues within Nt eps l_0 of eigvalsh, the phase
    convention; and the stop rule ends the iteration well inside the cap of 24 sweeps."""
    eps = 2.0 ** -23
    h = JS.planes(nt, nr, 2, 3)
    for p in range(3):
        an = JS.analog([x[p] for x in h], None, 2, 2, 0.0, dtype=np.complex64)
        for R32 in an['Rg'] + an['Rt']:
            R32 = R32.astype(np.complex64)
            lam, V, sweeps = JS.jacobi_f32(R32)
            assert lam.dtype == np.float32 and V.dtype == np.complex64 and 2 <= sweeps <= 12, sweeps
            R, V, lam = R32.astype(np.complex128), V.astype(np.complex128), lam.astype(np.float64)
            w = np.linalg.eigvalsh(R)[::-1]
            l0 = np.abs(w).max()
            assert (np.diff(lam) <= 0).all() and np.abs(lam - w).max() <= nt * eps * l0
            assert np.sqrt((np.abs(R @ V - V * lam) ** 2).sum(0)).max() <= 4 * nt * eps * l0
            assert np.abs(np.conj(V).T @ V - np.eye(nt)).max() <= 4 * nt * eps
            j = np.argmax(np.abs(V), 0)
            top = V[j, np.arange(nt)]
            assert (top.imag == 0).all() and (top.real > 0).all()
