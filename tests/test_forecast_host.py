"""CPU tests of the channel forecast (csi_forecast_*, csrc/forecast.hip.h).  They check the fp64 statement
tests/forecast_ref.py, so that the GPU tests stand on something: the known answers of one and of M exponentials, the fallback, the
pooling, the conditions of use on the replayed ageing channel of tests/scatter_aging_ref.py, and the C-ABI surface."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forecast_ref as fr      # noqa: E402
import scatter_aging_ref as ar      # noqa: E402

ENTRY_POINTS = ('csi_forecast_gram_device', 'csi_forecast_gram_blocks_device', 'csi_forecast_fit_device', 'csi_forecast_apply_device',
                'csi_forecast_device', 'csi_forecast', 'csi_sounding_noise_device')


def _cplx(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def test_one_exponential_order_one():
    """x_i = a z^i per element, M = 1: G = S sum |z|^(2 (p - d)), rhs = z^d G, so c = z^d / (1 + ridge)"""
    rng = np.random.default_rng(1)
    npkt, nr, nt = 2, 2, 4
    a = _cplx(rng, (npkt, nr, nt, 234))
    for z, P, d, ridge in ((np.exp(0.37j), 6, 2, 1e-5), (0.93 * np.exp(-1.1j), 9, 4, 1e-2), (np.exp(2.5j), 2, 1, 0.0)):
        x = np.stack([a * z ** i for i in range(P)])
        y, f = fr.forecast(x, 1, d, ridge)
        assert np.abs(f['c'][..., 0] - z ** d / (1.0 + ridge)).max() < 1e-12
        assert not f['info'].any()
        assert np.abs(y - a * z ** (P - 1 + d) / (1.0 + ridge)).max() < 1e-11 * np.abs(a).max()
        want_err = 1.0 - 1.0 / (1.0 + ridge)                      # 1 - Re(conj(c) rhs) / energy with |z^d|^2 G = energy
        assert np.abs(f['fit_err'] - want_err).max() < 1e-12


@pytest.mark.parametrize('M,d', [(1, 1), (2, 1), (3, 2), (4, 3)])
def test_m_exponentials_are_forecast_exactly(M, d):
    """M distinct exponentials, ridge 0, P = 2 M + d - 1 (M equations): the forecast is the truth"""
    rng = np.random.default_rng(10 + M)
    npkt, nr, nt = 2, 1, 4
    P = 2 * M + d - 1
    zs = np.exp(1j * np.array([0.4, -1.3, 2.2, -2.9][:M]))
    amps = _cplx(rng, (M, npkt, nr, nt, 234))
    seq = lambda i: sum(amps[m] * zs[m] ** i for m in range(M))      # noqa: E731
    x = np.stack([seq(i) for i in range(P)])
    y, f = fr.forecast(x, M, d, 0.0)
    truth = seq(P - 1 + d)
    assert not f['info'].any()
    assert np.abs(y - truth).max() < 1e-9 * np.abs(truth).max(), np.abs(y - truth).max()
    assert f['fit_err'].max() < 1e-9


def test_fallback_on_zeros_and_on_non_finite():
    x = np.zeros((5, 2, 2, 4, 234), np.complex128)
    rng = np.random.default_rng(3)
    x[:, 1] = _cplx(rng, (5, 2, 4, 234))
    y, f = fr.forecast(x, 2, 1, 1e-5)
    assert f['info'][0].all() and not f['info'][1].any()
    assert np.array_equal(f['c'][0], np.array([[1, 0], [1, 0]], np.complex128))
    assert np.array_equal(y[0], x[-1, 0]) and np.all(f['fit_err'][0] == 0.0)
    T = fr.gram(x)
    T[1, 0, 0, 0] = np.nan
    g = fr.fit(T, 2, 1)
    assert g['info'][1, 0] == 1 and g['info'][1, 1] == 0 and np.array_equal(g['c'][1, 0], [1, 0])
    # pooled: one rx of zeros does not take the packet down
    x[:, 1, 0] = 0.0
    assert not fr.forecast(x, 2, 1, 1e-5, pool_rx=True)[1]['info'][1].any()


def test_pooling_is_the_fit_of_the_summed_systems():
    rng = np.random.default_rng(4)
    P, M, d, ridge = 7, 3, 2, 1e-3
    x = _cplx(rng, (P, 2, 3, 4, 234))
    T = fr.gram(x)
    f = fr.fit(T, M, d, ridge, pool_rx=True)
    for p in range(2):
        G, rhs, en = (sum(fr.system(T[p, r], M, d)[k] for r in range(3)) for k in range(3))
        c = np.linalg.solve(G + ridge * np.trace(G).real / M * np.eye(M), rhs)
        for r in range(3):
            assert np.abs(f['c'][p, r] - c).max() < 1e-12 * np.abs(c).max()
            assert abs(f['fit_err'][p, r] - (1.0 - np.vdot(c, rhs).real / en)) < 1e-12
    # ... which is the fit of the rx antennas laid side by side as one block
    wide = x.reshape(P, 2, 1, 12, 234)
    one = fr.fit(fr.gram(wide), M, d, ridge)
    assert np.abs(one['c'][:, 0] - f['c'][:, 0]).max() < 1e-12
    assert np.abs(fr.fit(T, M, d, ridge)['c'] - f['c']).max() > 1e-3      # the per-rx fits differ


def test_gram_is_hermitian_and_solve_matches_numpy():
    rng = np.random.default_rng(5)
    x = _cplx(rng, (6, 1, 2, 4, 234))
    T = fr.gram(x)
    assert np.array_equal(T, np.conj(np.swapaxes(T, -1, -2)))
    G, rhs, en = fr.system(T[0, 1], 3, 2)
    c, info, fe, A = fr.solve(G, rhs, en, 1e-4)
    assert info == 0 and np.abs(A @ c - rhs).max() < 1e-10 * np.abs(rhs).max()
    # the residual identity behind fit_err at ridge 0
    c0 = fr.solve(G, rhs, en, 0.0)[0]
    res = sum(np.sum(np.abs(x[p, 0, 1] - sum(c0[a] * x[p - 2 - a, 0, 1] for a in range(3))) ** 2) for p in range(4, 6))
    assert abs(res / en - fr.solve(G, rhs, en, 0.0)[2]) < 1e-10


@pytest.fixture(scope='module')
def aged(oracle):
    """the replayed channel of the issue: Nt = 8, Nr = 2, S = 100, 2 packets, 1 m/s at 28 GHz, 12 soundings 0.5 ms apart and the
    channel 2 ms behind the newest"""
    P, d, dt = 12, 4, 0.5e-3
    times = [-(P - 1 - i) * dt for i in range(P)] + [d * dt]
    h = ar.replay(31, 0, 2, 2, oracle.hadamard(8), times, speed_mps=1.0, heading_az_deg=20.0, n_scat=100)['h']
    return h[:P], h[P]


def test_conditions_of_use_on_the_replayed_channel(aged):
    x, truth = aged
    y, f = fr.forecast(x, 4, 4, 1e-5)
    hold, fc = fr.nmse(x[-1], truth), fr.nmse(y, truth)
    print(f'noise-free: hold {hold:.4f}, forecast {fc:.5f}, cond {f["cond"].max():.3g}')
    assert not f['info'].any()
    assert fc <= 0.02 and hold >= 0.4, (fc, hold)
    # 20 dB: white error of variance 10^-2 x the mean element power on every sounding but the truth
    v = np.full((2, 2), 1e-2 * np.mean(np.abs(x) ** 2), np.float32)
    xn = np.stack([fr.sounding_noise(x[i], v, 31 ^ ((i + 1) << 32), 0) for i in range(12)])
    yn = fr.forecast(xn, 4, 4, 1e-5)[0]
    hold_n, fc_n = fr.nmse(xn[-1], truth), fr.nmse(yn, truth)
    print(f'20 dB: hold {hold_n:.4f}, forecast {fc_n:.4f}')
    assert fc_n < 0.5 * hold_n, (fc_n, hold_n)
    # float32 Gram entries move the coefficients but not the result
    T32 = fr.gram(x).astype(np.complex64).astype(np.complex128)
    y32 = fr.apply(x, fr.fit(T32, 4, 4, 1e-5)['c'])
    assert abs(fr.nmse(y32, truth) - fc) < 1e-2 * fc


def test_noise_replay_statistics():
    z = fr.noise_normals(7, 3, 2, 2, 4)
    assert abs(np.mean(np.abs(z) ** 2) - 2.0) < 0.1 and abs(np.mean(z)) < 0.05
    assert np.array_equal(z[1], fr.noise_normals(7, 4, 1, 2, 4)[0])      # a packet's draws do not depend on the call
    x = np.ones((2, 2, 4, 234), np.complex128)
    assert np.array_equal(fr.sounding_noise(x, np.zeros((2, 2)), 7, 3), x)


def test_surface_header_table_library_and_profile(pkg):
    pkg.build_library()
    lib = pkg.load_library()
    from dl_channel_estimation_mamimo_amd import _lib
    header = open(os.path.join(REPO, 'include', 'csi_mamimo.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(csi_[a-z0-9_]+)\s*\(', code))
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
        assert len(re.search(r'\b' + name + r'\s*\(([^)]*)\)', code).group(1).split(',')) == len(_lib.SYMBOLS[name][1]), name
    assert lib.csi_abi_version() == 1            # the change is additive
    names = [lib.csi_profile_kernel_name(i).decode() for i in range(lib.csi_profile_num_kernels())]
    for k in ('forecast_gram', 'forecast_fit', 'forecast_apply', 'sounding_noise'):
        assert k in names and '"%s"' % k in header, k
    assert names[-4:] == ['synth_scattering', 'lmmse_null_noise', 'lmmse_freq_corr', 'lmmse_blind']
    assert '"forecast_launches"' in header
    blob = open(pkg.library_path(), 'rb').read()
    for k in (b'forecast_gram_kernel', b'forecast_fit_kernel', b'forecast_apply_kernel', b'sounding_noise_kernel'):
        assert k in blob
    assert lib.csi_forecast_gram_device(None, None, None, 2, 1, None, None) == -1          # a null context
    assert lib.csi_forecast_gram_blocks_device(None, None, None, 2, 1, 2, None, None) == -1
    assert lib.csi_forecast_fit_device(None, None, None, 2, 1, 1, 1, 0.0, 0, None, None, None, None) == -1
    assert lib.csi_forecast_apply_device(None, None, None, 2, 1, 1, None, None, None, None) == -1
    assert lib.csi_forecast_device(None, None, None, 2, 1, 1, 1, 0.0, 0, None, None, None, None, None, None) == -1
    assert lib.csi_forecast(None, None, None, 2, 1, 1, 1, 0.0, 0, None, None, None, None, None, None) == -1
    assert lib.csi_sounding_noise_device(None, 1, 0, 1, None, None, None, None, None) == -1
    for m in ('forecast', 'forecast_device', 'forecast_gram_device', 'forecast_fit_device', 'forecast_apply_device', 'sounding_noise_device'):
        assert hasattr(pkg.CsiEngine, m)
