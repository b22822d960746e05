"""CPU tests of the link simulation with an estimated effective channel (csi_link_sim_rx_device, csrc/link_sim.hip.h):
the C-ABI surface, csi_link_preamble_symbols, the fp64 restatement tests/link_rx_ref.py against known answers, and the sweep's
--rxEstimate argument."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import link_ref as L        # noqa: E402
import link_rx_ref as R     # noqa: E402

NEW = ['csi_link_preamble_symbols', 'csi_link_sim_rx_device']


def _taps_channel(rng, npkt, nr, nt, n_taps=8):
    """true channel planes shaped like the generator's: n_taps complex Gaussian taps with the profile exp(-0.5 t) / sqrt(2) per link,
    their 256-point transform on 234 bins"""
    cir = rng.standard_normal((npkt, nr, nt, n_taps)) + 1j * rng.standard_normal((npkt, nr, nt, n_taps))
    cir *= np.exp(-0.5 * np.arange(n_taps)) / np.sqrt(2.0)
    full = np.fft.fftshift(np.fft.fft(cir, n=256, axis=-1), axes=-1)
    return full[..., 11:11 + L.N]


def _weights(rng, npkt, nt, ns, ntrf):
    fbb = rng.standard_normal((npkt, L.N, ns, ntrf)) + 1j * rng.standard_normal((npkt, L.N, ns, ntrf))
    frf = np.exp(2j * np.pi * rng.random((npkt, ntrf, nt)))
    return fbb, frf


def test_new_entry_points_in_header_table_and_library(pkg):
    pkg.build_library()
    lib = pkg.load_library()
    header = open(os.path.join(REPO, 'include', 'csi_mamimo.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(csi_[a-z0-9_]+)\s*\(', header))
    from dl_channel_estimation_mamimo_amd import _lib
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.csi_abi_version() == 1            # the change is additive
    assert b'link_txrx_rx_kernel' in open(pkg.library_path(), 'rb').read()
    assert hasattr(pkg.CsiEngine, 'link_sim_rx') and hasattr(pkg.CsiEngine, 'link_sim_rx_device')


def test_null_context_and_preamble_symbols(pkg):
    lib = pkg.load_library()
    assert lib.csi_link_sim_rx_device(None, *[None] * 7, 0, 0, 1, 1, 1, 1, 2, *[None] * 11) == -1
    assert [lib.csi_link_preamble_symbols(ns) for ns in (1, 2, 3, 4)] == [1, 2, 4, 4] == [R.N_LTF[ns] for ns in (1, 2, 3, 4)]
    assert lib.csi_link_preamble_symbols(0) == -1 and lib.csi_link_preamble_symbols(5) == -1


def test_pilot_matrix_rows_are_orthogonal():
    for ns in (1, 2, 3, 4):
        P = R.preamble_matrix(ns)
        assert P.shape == (ns, R.N_LTF[ns]) and set(np.unique(P)) <= {-1.0, 1.0}
        assert np.array_equal(P @ P.T, R.N_LTF[ns] * np.eye(ns))


def test_noiseless_estimate_is_the_channel():
    rng = np.random.default_rng(3)
    for ns in (1, 2, 3, 4):
        G = rng.standard_normal((L.N, 4, ns)) + 1j * rng.standard_normal((L.N, 4, ns))
        assert np.abs(R.estimate(G, 0.0, 5, 2, 3, 4) - G).max() <= 1e-12
        assert R.g_nmse(R.estimate(G, 0.0, 5, 2, 3, 4), G) <= 1e-24
    assert R.g_nmse(np.zeros((L.N, 2, 1)), np.zeros((L.N, 2, 1))) == 0.0
    assert R.g_nmse(np.ones((L.N, 2, 1)), np.zeros((L.N, 2, 1))) == np.inf


def test_data_symbols_keep_the_noise_of_the_genie_simulation():
    """the preamble continues the stream: rows 0 .. n_sym - 1 of the longer draw are the genie simulation's, and the received data
    symbols of simulate_rx are those of link_ref.simulate"""
    seed, pkt, n_sym, nr = 9, 6, 3, 4
    for ns in (1, 2, 3):
        longer = L.noise_normals(seed, pkt, n_sym + R.N_LTF[ns], nr)
        assert np.array_equal(longer[:n_sym], L.noise_normals(seed, pkt, n_sym, nr))
    rng = np.random.default_rng(4)
    h = _taps_channel(rng, 1, nr, 8)[0]
    fbb, frf = _weights(rng, 1, 8, 2, 2)
    a = R.simulate_rx(seed, pkt, h, frf[0], fbb[0], 0.3, n_sym, 2)
    b = L.simulate(seed, pkt, h, frf[0], fbb[0], 0.3, n_sym, 2)
    assert np.array_equal(a['w'], b['w']) and np.array_equal(a['y'], b['y']) and np.array_equal(a['x_genie'], b['x'])
    assert a['dt_snr_db'] == b['dt_snr_db'] and np.array_equal(a['bits'], b['bits'])
    want = np.sqrt(0.3 / 2.0) * L.noise_normals(seed, pkt, n_sym + 2, nr)[n_sym:]
    P = R.preamble_matrix(2)
    assert np.abs(a['Ghat'] - a['G'] - np.einsum('mkr,sm->krs', want, P) / 2).max() <= 1e-12


@pytest.mark.parametrize('ns', [1, 2, 3, 4])
def test_estimation_error_level(ns):
    """Ghat - G ~ CN(0, noise_var / n_ltf): the mean of N squared magnitudes of unit-variance complex normals has the standard
    deviation 1 / sqrt(N); bound 5 / sqrt(N)"""
    nr, noise_var, n_pkt = 4, 0.37, 12
    rng = np.random.default_rng(ns)
    G = rng.standard_normal((L.N, nr, ns)) + 1j * rng.standard_normal((L.N, nr, ns))
    err = np.concatenate([(R.estimate(G, noise_var, 11, p, 2, nr) - G).reshape(-1) for p in range(n_pkt)])
    n = err.size
    assert n >= 10000
    ratio = (np.abs(err) ** 2).mean() / (noise_var / R.N_LTF[ns])
    print('ns %d: %d samples, mean |Ghat - G|^2 / (noise_var / n_ltf) = %.4f, bound %.4f' % (ns, n, ratio, 5 / np.sqrt(n)))
    assert abs(ratio - 1.0) <= 5.0 / np.sqrt(n)


def test_one_stream_pays_three_decibels():
    """ns = 1, Nt = 8, Nr = 4, 16 packets x 4 symbols at 20 dB: x - d = g^H w / |g|^2 for the genie receiver, and the estimate's own
    error (the same variance: n_ltf = 1) adds as much again to first order in the noise - the post-equaliser error power doubles"""
    nt, nr, ns, npkt, n_sym, bps = 8, 4, 1, 16, 4, 2
    rng = np.random.default_rng(20)
    h = _taps_channel(rng, npkt, nr, nt)
    fbb, frf = _weights(rng, npkt, nt, ns, 1)
    rx = genie = 0.0
    for p in range(npkt):
        G = L.effective_channel(h[p], L.precoder(frf[p], fbb[p]))
        nv = (np.abs(G) ** 2).sum((1, 2)).mean() / nr * 10.0 ** (-20.0 / 10.0)
        r = R.simulate_rx(7, p, h[p], frf[p], fbb[p], nv, n_sym, bps)
        assert np.isfinite(r['cond']).all()
        rx += (np.abs(r['x'] - r['d']) ** 2).sum()
        genie += (np.abs(r['x_genie'] - r['d']) ** 2).sum()
    print('error power with the estimate / with the exact channel: %.4f' % (rx / genie))
    assert abs(rx / genie - 2.0) <= 0.1


def test_sweep_argument_and_field_lists():
    from dl_channel_estimation_mamimo_amd import sweep
    args = sweep.parse_args(['-d', 'x', '--ber', '--rxEstimate'])
    assert args.rxEstimate and args.ber
    assert not sweep.parse_args(['-d', 'x', '--ber']).rxEstimate
    with pytest.raises(SystemExit):
        sweep.parse_args(['-d', 'x', '--rxEstimate'])
    one = np.zeros(3)
    mse = {'MSE_' + e: one for e in sweep.ESTIMATORS}
    assert sweep.metric_fields(mse) == ['MSE_LS', 'MSE_MMSE', 'MSE_DNN']
    mse.update({f + x: one for x in sweep.SOURCES for f in sweep.LINK_FIELDS}, MSE_perfect=one)
    plain = sweep.metric_fields(mse)
    assert plain == ['MSE_LS', 'MSE_MMSE', 'MSE_DNN'] + [f + x for x in ('LS', 'MMSE', 'DNN', 'perfect')
                                                         for f in ('bers_', 'EVM_rms_', 'dtSNR_')] + ['MSE_perfect']
    mse.update({f + x: one for x in sweep.SOURCES for f in sweep.RX_FIELDS})
    assert sweep.RX_FIELDS == ('bersRx_', 'EVM_rmsRx_', 'gNMSE_')
    with_rx = sweep.metric_fields(mse)
    assert with_rx[:len(plain)] == plain                                   # the new fields are written behind every existing one
    assert with_rx[len(plain):] == [f + x for x in sweep.SOURCES for f in sweep.RX_FIELDS]
