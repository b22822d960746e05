"""CPU tests of the delay-subspace smoother (csi_subspace_set_basis, csi_subspace_smooth[_device]): the basis and the weights of
dl_channel_estimation_mamimo_amd.subspace in fp64, the carrier and sign convention on a host-made noise-free packet, the C-ABI surface
and the sweep's --delayTaps switch as far as it runs without a device."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subspace_ref as sr      # noqa: E402

WINDOWS = ((8, 0), (16, 0), (64, 0), (64, 8), (100, 0), (128, 16))
ENTRY_POINTS = ('csi_subspace_set_basis', 'csi_subspace_smooth', 'csi_subspace_smooth_device')


def test_carriers(pkg):
    f = pkg.subspace.data_carrier_offsets()
    assert f.shape == (234,) and f.min() == -121 and f.max() == 121 and np.all(np.diff(f) > 0)
    ind = f + 129
    for b in (1, 7, 129, 251, 256, 26, 54, 90, 118, 140, 168, 204, 232):
        assert b not in ind
    assert 8 in ind and 250 in ind and 128 in ind and 130 in ind


@pytest.mark.parametrize('window', WINDOWS, ids=['L%d_pre%d' % w for w in WINDOWS])
def test_basis_is_orthonormal_and_full_rank(pkg, window):
    Q, lam = pkg.subspace.delay_basis(*window)
    L = window[0]
    assert Q.dtype == np.complex128 and Q.shape == (234, L) and lam.shape == (L,), 'r = L for this window'
    assert np.abs(Q.conj().T @ Q - np.eye(L)).max() <= 1e-12
    assert abs(lam.sum() - 234.0) <= 1e-9 and np.all(lam > 0) and np.all(np.diff(lam) <= 0)
    # Q diag(lam) Q^H is the correlation of a uniform profile over the window
    f = pkg.subspace.data_carrier_offsets().astype(np.float64)
    F = np.exp(-2j * np.pi * np.outer(f, np.arange(L) - window[1]) / 256)
    assert np.abs((Q * lam) @ Q.conj().T - F @ F.conj().T / L).max() <= 1e-10


def test_basis_arguments(pkg):
    for bad in ((0, 0), (129, 0), (8, 9), (8, -1)):
        with pytest.raises(ValueError):
            pkg.subspace.delay_basis(*bad)
    # a tolerance that cuts: the rank follows the singular values
    Q, lam = pkg.subspace.delay_basis(128, 16, tol=1e-2)
    assert Q.shape[1] == lam.size < 128


@pytest.mark.parametrize('nu', [1e-3, 1.0, 1e3])
@pytest.mark.parametrize('window', [(8, 0), (64, 8)], ids=['L8', 'L64_pre8'])
def test_robust_weights_are_the_lmmse_smoother(pkg, window, nu):
    Q, lam = pkg.subspace.delay_basis(*window)
    w = pkg.subspace.robust_weights(lam, nu)
    assert np.array_equal(w, lam / (lam + nu))
    R = (Q * lam) @ Q.conj().T
    direct = np.linalg.solve((R + nu * np.eye(234)).T, R.T).T          # R (R + nu I)^-1
    assert np.abs((Q * w) @ Q.conj().T - direct).max() <= 1e-10
    assert pkg.subspace.robust_weights(lam, np.full((3, 2, 1), nu)).shape == (3, 2, lam.size)


def test_carrier_and_sign_convention(pkg, oracle):
    """A host-made noise-free 8-tap packet (oracle.make_structured_packets, preamble rounded to complex64 as the device holds it) and
    the oracle's LS estimate of it: the projection with the window (8, 0) moves the LS estimate by no more than twice the LS
    estimate's own distance to the true channel; with the frequency sign flipped (the conjugate basis) it fails that bound."""
    nt, nr, npkt = 4, 2, 3
    P = oracle.hadamard(nt)
    ltf, h = oracle.make_structured_packets(np.random.default_rng(12), npkt, nr, P, snr_db=None)
    ls = oracle.ls_estimate(ltf.astype(np.complex64), P)
    Q, _ = pkg.subspace.delay_basis(8, 0)
    own = np.linalg.norm((ls - h).reshape(-1, 234), axis=1)
    moved = np.linalg.norm((sr.smooth(ls, Q) - ls).reshape(-1, 234), axis=1)
    flipped = np.linalg.norm((sr.smooth(ls, Q.conj()) - ls).reshape(-1, 234), axis=1)
    size = np.linalg.norm(h.reshape(-1, 234), axis=1)
    print('LS off the channel by %.3e, projection moves LS by %.3e, flipped basis by %.3e (relative to |h|, worst row)' % (
        (own / size).max(), (moved / size).max(), (flipped / size).min()))
    assert np.all(own > 0)
    assert np.all(moved <= 2.0 * own)
    assert np.all(flipped > 2.0 * own)
    # and the true channel itself lies in the window
    assert (np.linalg.norm((sr.smooth(h, Q) - h).reshape(-1, 234), axis=1) / size).max() <= 1e-13


def test_reference_in_both_precisions(pkg):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((2, 2, 4, 234)) + 1j * rng.standard_normal((2, 2, 4, 234))).astype(np.complex64)
    Q, _ = pkg.subspace.delay_basis(16)
    w = rng.random((2, 2, 16)).astype(np.float32)
    y64, y32 = sr.smooth(x, Q, w), sr.smooth(x, Q, w, np.complex64)
    assert y64.dtype == np.complex128 and y32.dtype == np.complex64
    e = sr.row_err(y32, y64, x).max()
    assert 0 < e < 1e-6
    # per (packet, rx) weights: a swapped index shows
    assert sr.row_err(sr.smooth(x, Q, w[:, ::-1]), y64, x).max() > 1e-2
    assert np.abs(sr.smooth(x, Q, np.ones_like(w)) - sr.smooth(x, Q)).max() == 0


def test_surface(pkg):
    pkg.build_library()
    lib = pkg.load_library()
    header = open(os.path.join(REPO, 'include', 'csi_mamimo.h')).read()
    assert re.search(r'no reference counterpart[^*]*\*[^*]*csi_subspace_set_basis, csi_subspace_smooth\[_device\]', header), 'row of the call-site table'
    para = header[header.index('Device pointers ('):header.index('An array of exactly the documented')]
    assert 'csi_subspace_smooth_device' in para
    assert '"subspace_launches"' in header and '"subspace_smooth"' in header
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(csi_[a-z0-9_]+)\s*\(', code))
    from dl_channel_estimation_mamimo_amd import _lib
    integration = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    for sym in ENTRY_POINTS:
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(lib, sym), sym
        assert '`%s`' % sym in integration, sym
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    assert lib.csi_abi_version() == 1            # the change is additive
    names = [lib.csi_profile_kernel_name(i).decode() for i in range(lib.csi_profile_num_kernels())]
    assert names.count('subspace_smooth') == 1
    assert b'subspace_smooth_kernel' in open(pkg.library_path(), 'rb').read()
    assert lib.csi_subspace_set_basis(None, None, None, 1) == -1
    assert lib.csi_subspace_smooth(None, None, None, 1, None, None, None) == -1
    assert lib.csi_subspace_smooth_device(None, None, None, 1, None, None, None) == -1
    for m in ('subspace_set_basis', 'subspace_smooth', 'subspace_smooth_device'):
        assert hasattr(pkg.CsiEngine, m), m
    for f in ('data_carrier_offsets', 'delay_basis', 'robust_weights'):
        assert hasattr(pkg.subspace, f), f


def test_sweep_parser_and_metric_fields(pkg, tmp_path):
    """The parser, and the field lists of write_metrics / format_table with and without the estimator DLY (without it they hold
    exactly what they held before)."""
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    a = sweep.parse_args(['-d', 'x'])
    assert a.delayTaps == 0 and a.delayPre == 0
    a = sweep.parse_args(['-d', 'x', '--delayTaps', '8', '--delayPre', '2'])
    assert (a.delayTaps, a.delayPre) == (8, 2)
    for bad in (['--delayTaps', '129'], ['--delayTaps', '8', '--delayPre', '9'], ['--delayPre', '1']):
        with pytest.raises(SystemExit):
            sweep.parse_args(['-d', 'x'] + bad)
    assert sweep.ESTIMATORS == ('LS', 'MMSE', 'DNN') and sweep.DELAY == 'DLY'
    rng = np.random.default_rng(1)
    mse = {'MSE_' + e: rng.random(8) for e in sweep.ESTIMATORS}
    keys = lambda path: {k for k in loadmat(path) if not k.startswith('__')}
    assert keys(sweep.write_metrics(str(tmp_path / 'a' / 'metrics.mat'), mse)) == {'MSE_LS', 'MSE_MMSE', 'MSE_DNN'}
    assert sweep.metric_fields(mse) == ['MSE_LS', 'MSE_MMSE', 'MSE_DNN']
    mse['MSE_DLY'] = rng.random(8)
    path = sweep.write_metrics(str(tmp_path / 'b' / 'metrics.mat'), mse)
    assert keys(path) == {'MSE_LS', 'MSE_MMSE', 'MSE_DNN', 'MSE_DLY'} and sweep.metric_fields(mse)[-1] == 'MSE_DLY'
    assert np.array_equal(loadmat(path)['MSE_DLY'][0], mse['MSE_DLY'])
    lv = {e: dict(mean=1.0, ci_low=0.5, ci_high=1.5) for e in ('LS', 'MMSE', 'DNN', 'DLY')}
    plain = sweep.format_table(dict(levels=[dict(lv, snr_db=0.0)]))
    assert 'DLY' not in plain and 'DLY' in sweep.format_table(dict(levels=[dict(lv, snr_db=0.0)], delay=dict(taps=8, pre=0, rank=8)))
