"""CPU tests of the beam-space smoother (csi_beam_*, csi_null_noise_device): the DFT beams and the weight rule of
dl_channel_estimation_mamimo_amd.beamspace, their sign convention against the scattering channel, what the reference of
tests/beam_ref.py gains on host-made scattering channels, the C-ABI surface and the sweep's --beams switch as far as it runs without a
device."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as br      # noqa: E402

ENTRY_POINTS = ('csi_beam_set_basis', 'csi_beam_power_device', 'csi_beam_smooth', 'csi_beam_smooth_device', 'csi_beam_wiener',
                'csi_beam_wiener_device', 'csi_null_noise_device')


@pytest.mark.parametrize('nt', [4, 12, 32, 128])
def test_dft_basis_is_unitary(pkg, nt):
    A = pkg.beamspace.dft_basis(nt)
    assert A.dtype == np.complex128 and A.shape == (nt, nt)
    assert np.abs(A.conj().T @ A - np.eye(nt)).max() <= 1e-12
    assert np.abs(A @ A.conj().T - np.eye(nt)).max() <= 1e-12
    assert np.abs(np.abs(A) - 1 / np.sqrt(nt)).max() <= 1e-15


def test_dft_basis_arguments(pkg):
    assert pkg.beamspace.MAX_NT == 128
    for bad in (0, 129):
        with pytest.raises(ValueError):
            pkg.beamspace.dft_basis(bad)


@pytest.mark.parametrize('nt', [4, 12, 32])
def test_beam_b_points_at_u_b(pkg, nt):
    """Column b correlates most with the transmit factor of a path at the direction cosine u_b = 2 (b - nt / 2) / nt - the conjugate of
    synth.steering_ula, as synth.scattering_channel states - among 8 nt directions in [-1, 1) (u = 1 is the alias of u = -1 on a
    half-wavelength array)."""
    A = pkg.beamspace.dft_basis(nt)
    u = -1.0 + 2.0 * np.arange(8 * nt) / (8 * nt)
    tx = pkg.synth.steering_ula(nt, np.rad2deg(np.arcsin(u))).conj()           # [nt, directions] = exp(-2 pi i y_j u)
    corr = np.abs(A.conj().T @ tx)                                             # [beam, direction]
    for b in range(nt):
        assert abs(u[corr[b].argmax()] - 2.0 * (b - nt / 2.0) / nt) <= 1e-12, b
        assert abs(corr[b].max() - np.sqrt(nt)) <= 1e-9
    # the mirrored convention points elsewhere for every beam but u = -1 and u = 0
    mirrored = np.abs(A.T @ tx)
    assert sum(mirrored[b].argmax() != corr[b].argmax() for b in range(nt)) == nt - 2


def _carriers(pkg, H):
    """the 234 data carriers, ascending, of a channel in FFT bin order [..., 256]"""
    return H[..., pkg.subspace.data_carrier_offsets() % 256]


def test_one_scatterer_falls_into_one_beam(pkg):
    rng = np.random.default_rng(5)
    nt, nr = 32, 2
    for _ in range(8):
        H, _ = pkg.synth.scattering_channel(rng.random((1, 3)), np.ones(1), 100.0, rng.uniform(-80.0, 80.0), 0.0, nr, nt)
        E = br.power(_carriers(pkg, H)[None], pkg.beamspace.dft_basis(nt))
        share = E.max(axis=-1) / E.sum(axis=-1)
        assert share.min() > 0.4, share


def test_wiener_weights(pkg):
    E = np.array([[[0.0, 0.5, 1.0, 2.0, 4.0], [0.0, 3.0, 3.0000002, 6.0, 1e30]]])
    v = np.array([[1.0, 3.0]])
    w = pkg.beamspace.wiener_weights(E, v)
    assert w.dtype == np.float32 and w.shape == E.shape
    assert np.array_equal(w[0, 0], np.array([0, 0, 0, 0.5, 0.75], np.float32))
    e32, v32 = E[0, 1].astype(np.float32), np.float32(3.0)
    assert np.array_equal(w[0, 1], np.array([0, 0, np.float32(1) - v32 / e32[2], 0.5, 1.0], np.float32)) and 0 < w[0, 1, 2] < 1e-6
    assert not pkg.beamspace.wiener_weights(np.zeros((2, 1, 3)), np.zeros((2, 1))).any(), 'E = 0 gives 0 even at v = 0'
    assert np.array_equal(pkg.beamspace.wiener_weights(np.ones((2, 1, 3)), np.zeros((2, 1))), np.ones((2, 1, 3), np.float32))
    assert np.array_equal(w, br.weights(E.astype(np.float32), v))


def _draw(pkg, rng, nt, nr, npkt, iid=False):
    """true channels complex128 [npkt, nr, nt, 234]: synth.scattering_channel with the generator's defaults (S = 100, range 100 m,
    az 30 degrees, box_frac 0.1), or 8 i.i.d. taps of the tap generator's profile per link"""
    h = np.empty((npkt, nr, nt, br.N), np.complex128)
    for p in range(npkt):
        if iid:
            taps = (rng.standard_normal((nr, nt, 8)) + 1j * rng.standard_normal((nr, nt, 8))) * np.exp(-0.5 * np.arange(8)) / 2.0
            H = np.fft.fft(taps, 256, axis=-1)
        else:
            g = (rng.standard_normal(100) + 1j * rng.standard_normal(100)) / np.sqrt(2.0)
            H, _ = pkg.synth.scattering_channel(rng.random((100, 3)), g, 100.0, 30.0, 0.0, nr, nt)
        h[p] = _carriers(pkg, H)
    return h


def _ratio(pkg, h, rng, snr_db):
    """white error of exactly known variance v = mean power of the (packet, rx) / SNR on every element; NMSE after the Wiener step over
    NMSE before it"""
    v = np.mean(np.abs(h) ** 2, axis=(2, 3)) * 10.0 ** (-snr_db / 10.0)
    x = h + np.sqrt(v / 2.0)[..., None, None] * (rng.standard_normal(h.shape) + 1j * rng.standard_normal(h.shape))
    y, _ = br.wiener(x, pkg.beamspace.dft_basis(h.shape[2]), v)
    return br.nmse(y, h) / br.nmse(x, h)


@pytest.mark.parametrize('shape,want', [((32, 4, 8), {-10.0: 0.057, 10.0: 0.39}), ((8, 2, 24), {-10.0: 0.064, 10.0: 0.51})],
                         ids=['nt32_nr4_8pkt', 'nt8_nr2_24pkt'])
def test_reference_gain_on_scattering_channels(pkg, shape, want):
    """The fp64 reference on scattering-channel draws meets the ratios of the design table (0.057 / 0.39 at Nt = 32, 0.064 / 0.51 at
    Nt = 8, at -10 / 10 dB) within 15 %."""
    nt, nr, npkt = shape
    rng = np.random.default_rng(1)
    h = _draw(pkg, rng, nt, nr, npkt)
    for snr, w in want.items():
        r = _ratio(pkg, h, rng, snr)
        print('Nt %d Nr %d %d packets, %g dB: NMSE ratio to LS %.4f (table %.3f)' % (nt, nr, npkt, snr, r, w))
        assert abs(r - w) <= 0.15 * w


def test_reference_never_loses_without_spatial_structure(pkg):
    rng = np.random.default_rng(2)
    h = _draw(pkg, rng, 32, 4, 6, iid=True)
    for snr in (-10.0, 10.0):
        r = _ratio(pkg, h, rng, snr)
        print('i.i.d. taps, %g dB: NMSE ratio to LS %.4f' % (snr, r))
        assert r < 1.0


def test_reference_in_both_precisions(pkg):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((2, 2, 12, 234)) + 1j * rng.standard_normal((2, 2, 12, 234))).astype(np.complex64)
    A = br.random_basis(rng, 12, 7)
    w = rng.random((2, 2, 7)).astype(np.float32)
    y64, y32 = br.smooth(x, A, w), br.smooth(x, A, w, np.complex64)
    assert y64.dtype == np.complex128 and y32.dtype == np.complex64
    assert 0 < br.row_err(y32, y64, x).max() < 1e-6
    assert br.power(x, A).dtype == np.float64 and br.power(x, A, np.complex64).dtype == np.float32
    assert br.row_err(br.smooth(x, A, w[:, ::-1]), y64, x).max() > 1e-2, 'per (packet, rx) weights: a swapped index shows'
    assert np.abs(br.smooth(x, A, np.ones_like(w)) - br.smooth(x, A)).max() == 0
    # Parseval for a unitary basis
    U = pkg.beamspace.dft_basis(12)
    assert np.abs(br.power(x, U).sum(-1) - (np.abs(x.astype(np.complex128)) ** 2).sum(2).mean(-1)).max() <= 1e-12
    y, wv = br.wiener(x, U, np.zeros((2, 2)))
    assert np.array_equal(wv, np.ones_like(wv)) and br.row_err(y, x, x).max() <= 1e-14


def test_surface(pkg):
    pkg.build_library()
    lib = pkg.load_library()
    header = open(os.path.join(REPO, 'include', 'csi_mamimo.h')).read()
    assert re.search(r'no reference counterpart[^*]*\*[^*]*\*[^*]*csi_beam_set_basis, csi_beam_power_device, csi_beam_smooth\[_device\], '
                     r'csi_beam_wiener\[_device\], csi_null_noise_device', header), 'row of the call-site table'
    para = header[header.index('Device pointers ('):header.index('An array of exactly the documented')]
    for sym in ENTRY_POINTS:
        if sym.endswith('_device'):
            assert sym in para, sym
    for name in ('"beam_launches"', '"beam_power"', '"beam_smooth"'):
        assert name in header, name
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
    assert names.count('beam_power') == 1 and names.count('beam_smooth') == 1
    blob = open(pkg.library_path(), 'rb').read()
    for kernel in (b'beam_smooth_kernel', b'beam_power_kernel', b'beam_wiener_weights_kernel'):
        assert kernel in blob, kernel
    assert lib.csi_beam_set_basis(None, None, None, 1) == -1
    assert lib.csi_beam_power_device(None, None, None, 1, None) == -1
    assert lib.csi_beam_smooth(None, None, None, 1, None, None, None) == -1
    assert lib.csi_beam_smooth_device(None, None, None, 1, None, None, None) == -1
    assert lib.csi_beam_wiener(None, None, None, 1, None, None, None, None) == -1
    assert lib.csi_beam_wiener_device(None, None, None, 1, None, None, None, None) == -1
    assert lib.csi_null_noise_device(None, None, None, 1, None) == -1
    for m in ('beam_set_basis', 'beam_power', 'beam_smooth', 'beam_wiener', 'null_noise', 'beam_power_device', 'beam_smooth_device',
              'beam_wiener_device', 'null_noise_device'):
        assert hasattr(pkg.CsiEngine, m), m
    for f in ('dft_basis', 'wiener_weights', 'MAX_NT'):
        assert hasattr(pkg.beamspace, f), f


def test_sweep_parser_and_metric_fields(pkg, tmp_path):
    """The parser, and the field lists of write_metrics / format_table with and without the estimators ANG and DLYANG (without them
    they hold exactly what they held before)."""
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    assert sweep.parse_args(['-d', 'x']).beams is False
    assert sweep.parse_args(['-d', 'x', '--beams']).beams is True
    with pytest.raises(SystemExit):
        sweep.parse_args(['-d', 'x', '--beams', '--nTX', '256'])
    assert sweep.ESTIMATORS == ('LS', 'MMSE', 'DNN') and sweep.BEAMS == 'ANG' and sweep.DELAY_BEAMS == 'DLYANG'
    rng = np.random.default_rng(1)
    keys = lambda path: [k for k in loadmat(path) if not k.startswith('__')]
    mse = {'MSE_' + e: rng.random(8) for e in sweep.ESTIMATORS}
    assert sweep.metric_fields(mse) == ['MSE_LS', 'MSE_MMSE', 'MSE_DNN']
    assert set(keys(sweep.write_metrics(str(tmp_path / 'a' / 'metrics.mat'), mse))) == {'MSE_LS', 'MSE_MMSE', 'MSE_DNN'}
    mse['MSE_DLY'] = rng.random(8)
    assert sweep.metric_fields(mse) == ['MSE_LS', 'MSE_MMSE', 'MSE_DNN', 'MSE_DLY']
    mse['MSE_ANG'] = rng.random(8)
    mse['MSE_DLYANG'] = rng.random(8)
    assert sweep.metric_fields(mse) == ['MSE_LS', 'MSE_MMSE', 'MSE_DNN', 'MSE_DLY', 'MSE_ANG', 'MSE_DLYANG']
    path = sweep.write_metrics(str(tmp_path / 'b' / 'metrics.mat'), mse)
    assert set(keys(path)) == {'MSE_LS', 'MSE_MMSE', 'MSE_DNN', 'MSE_DLY', 'MSE_ANG', 'MSE_DLYANG'}
    assert np.array_equal(loadmat(path)['MSE_ANG'][0], mse['MSE_ANG'])
    # the multi-user data phase: ANG is one more source, behind every field that exists without it
    link = {f + x: rng.random(8) for x in sweep.SOURCES for f in sweep.LINK_FIELDS}
    mu = {f + x: rng.random(8) for x in sweep.SOURCES + ('DLY',) for f in sweep.MU_FIELDS}
    base = dict({k: v for k, v in mse.items() if 'ANG' not in k}, MSE_perfect=np.zeros(8), **link, **mu)
    before = sweep.metric_fields(base)
    with_ang = dict(base, MSE_ANG=mse['MSE_ANG'], MSE_DLYANG=mse['MSE_DLYANG'], **{f + 'ANG': rng.random(8) for f in sweep.MU_FIELDS})
    assert sweep.metric_fields(with_ang) == before + ['MSE_ANG', 'MSE_DLYANG', 'bersMU_ANG', 'EVM_rmsMU_ANG', 'sinrMU_ANG']
    lv = {e: dict(mean=1.0, ci_low=0.5, ci_high=1.5) for e in ('LS', 'MMSE', 'DNN', 'DLY', 'ANG', 'DLYANG')}
    plain = sweep.format_table(dict(levels=[dict(lv, snr_db=0.0)]))
    assert 'ANG' not in plain
    assert sweep.format_table(dict(levels=[dict(lv, snr_db=0.0)], delay=dict(taps=8, pre=0, rank=8))) == \
        sweep.format_table(dict(levels=[dict(lv, snr_db=0.0)], delay=dict(taps=8, pre=0, rank=8), beams=False))
    table = sweep.format_table(dict(levels=[dict(lv, snr_db=0.0)], delay=dict(taps=8, pre=0, rank=8), beams=True))
    assert 'ANG' in table and 'DLYANG' in table
    assert 'DLYANG' not in sweep.format_table(dict(levels=[dict(lv, snr_db=0.0)], beams=True))
