"""CPU tests of the blind LMMSE smoother (csi_lmmse_blind[_device]): the C-ABI surface, the fp64 reference tests/blind_lmmse_ref.py
(np.linalg.solve against the kernel's recursion restated in numpy, the guards), the statistics against the realised LS error, and the
sweep's --blind switch as far as it runs without a device."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blind_lmmse_ref as br      # noqa: E402


def _packets(oracle, seed, npkt, nr, nt, snr_db):
    """(ltf complex64, h_true, h_ls complex64: the preamble and its LS estimate as the device holds them) of oracle.make_structured_packets"""
    rng = np.random.default_rng(seed)
    P = oracle.hadamard(nt)
    ltf, h = oracle.make_structured_packets(rng, npkt, nr, P, snr_db=snr_db)
    ltf = ltf.astype(np.complex64)
    return ltf, h, oracle.ls_estimate(ltf, P).astype(np.complex64)


def test_surface(pkg):
    pkg.build_library()
    lib = pkg.load_library()
    header = open(os.path.join(REPO, 'include', 'csi_mamimo.h')).read()
    assert re.search(r'helperMIMOChannelEstimate\.m:37-39[^*]*\*[^*]*csi_lmmse_blind\[_device\]', header), 'row of the call-site table'
    assert 'The DC bin IS counted' in header and '"lmmse_blind_fallbacks"' in header
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(csi_[a-z0-9_]+)\s*\(', code))
    from dl_channel_estimation_mamimo_amd import _lib
    for sym in ('csi_lmmse_blind', 'csi_lmmse_blind_device'):
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(lib, sym), sym
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    assert lib.csi_abi_version() == 1            # the change is additive
    names = [lib.csi_profile_kernel_name(i).decode() for i in range(lib.csi_profile_num_kernels())]
    assert names[-3:] == ['lmmse_null_noise', 'lmmse_freq_corr', 'lmmse_blind'], names     # appended behind the existing ids
    assert names.index('lmmse_levinson') == 11 and names[-4] == 'synth_scattering'
    blob = open(pkg.library_path(), 'rb').read()
    for k in (b'lmmse_null_noise_kernel', b'lmmse_freq_corr_kernel', b'lmmse_blind_kernel', b'lmmse_levinson_kernel'):
        assert k in blob, k
    assert lib.csi_lmmse_blind(None, None, None, None, None, 1, None, None, None, None) == -1
    assert lib.csi_lmmse_blind_device(None, None, None, None, None, 1, None, None, None, None) == -1
    assert hasattr(pkg.CsiEngine, 'lmmse_blind') and hasattr(pkg.CsiEngine, 'lmmse_blind_device')


def test_sweep_parser_and_metric_fields(pkg, tmp_path):
    """The sweep has no device-free path through run_sweep, so: the parser, and the field lists of write_metrics with and without
    the blind estimator (without it the file holds exactly what it held before)."""
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    assert sweep.build_parser().parse_args(['-d', 'x']).blind is False
    assert sweep.build_parser().parse_args(['-d', 'x', '--blind']).blind is True
    assert sweep.ESTIMATORS == ('LS', 'MMSE', 'DNN') and sweep.SOURCES == ('LS', 'MMSE', 'DNN', 'perfect') and sweep.BLIND == 'MMSEb'
    rng = np.random.default_rng(1)
    mse = {'MSE_' + e: rng.random(8) for e in sweep.ESTIMATORS}
    keys = lambda path: {k for k in loadmat(path) if not k.startswith('__')}
    assert keys(sweep.write_metrics(str(tmp_path / 'a' / 'metrics.mat'), mse)) == {'MSE_LS', 'MSE_MMSE', 'MSE_DNN'}
    mse['MSE_MMSEb'] = rng.random(8)
    path = sweep.write_metrics(str(tmp_path / 'b' / 'metrics.mat'), mse)
    assert keys(path) == {'MSE_LS', 'MSE_MMSE', 'MSE_DNN', 'MSE_MMSEb'}
    assert np.array_equal(loadmat(path)['MSE_MMSEb'][0], mse['MSE_MMSEb'])
    link = {f + x: rng.random(8) for x in sweep.SOURCES + ('MMSEb',) for f in sweep.LINK_FIELDS}
    full = dict(mse, MSE_perfect=np.zeros(8), **link)
    assert keys(sweep.write_metrics(str(tmp_path / 'c' / 'metrics.mat'), full)) == set(full)
    del full['MSE_MMSEb']
    for f in sweep.LINK_FIELDS:
        del full[f + 'MMSEb']
    assert keys(sweep.write_metrics(str(tmp_path / 'd' / 'metrics.mat'), full)) == set(full)
    lv = {e: dict(mean=1.0, ci_low=0.5, ci_high=1.5) for e in ('LS', 'MMSE', 'DNN', 'MMSEb')}
    plain = sweep.format_table(dict(levels=[dict(lv, snr_db=0.0)]))
    assert 'MMSEb' not in plain and 'MMSEb' in sweep.format_table(dict(levels=[dict(lv, snr_db=0.0)], blind=True))


@pytest.mark.parametrize('nt', [4, 32])
def test_solve_and_recursion_agree(oracle, nt):
    """np.linalg.solve on the explicit matrix against the kernel's recursion restated, at -10, 10, 40 dB and noise-free: within 1e-12
    per row (measured 1.5e-14 when the estimator was designed); T is positive definite at every level."""
    worst = 0.0
    for snr in (-10.0, 10.0, 40.0, None):
        ltf, _, h_ls = _packets(oracle, 100 + nt, 1, 2, nt, snr)
        out, nv, c = br.blind_ref(ltf, h_ls)
        for r in range(2):
            T = br.toeplitz(c[0, r])
            assert np.array_equal(T, T.conj().T)
            ev = np.linalg.eigvalsh(T)
            assert ev[0] > 0.0, (snr, ev[0])
            got, fell = br.levinson_blind(h_ls[0, r].T.astype(np.complex128), c[0, r], nv[0, r], nt)
            assert not fell
            err = br.rel_rows_c(got.T, out[0, r]).max()
            print('Nt %d snr %s rx %d: recursion vs solve %.3e, condition number %.3g, nv %.4g' % (nt, snr, r, err, ev[-1] / ev[0], nv[0, r]))
            worst = max(worst, err)
            assert err < 1e-12, (snr, err)
            assert ev[-1] / ev[0] <= 1e5
    print('Nt %d: worst %.3e' % (nt, worst))


def test_exact_null_carrier_sums_of_the_reference(oracle):
    """noise_var's exact form (twiddles to 60 digits, exact products, math.fsum) against the plain complex128 form: the same number
    where noise fills the null carriers, and the plain form's own error where only rounding residue is left - which is why the
    reference of the GPU tests is the exact one."""
    wr, wi = br.twiddles_exact()
    u = np.arange(256)
    assert max(abs(float(a) - b) for a, b in zip(wr, np.cos(2 * np.pi * u / 256))) < 1e-15
    assert max(abs(float(a) + b) for a, b in zip(wi, np.sin(2 * np.pi * u / 256))) < 1e-15
    assert all(abs(a * a + b * b - 1) < 1e-60 for a, b in zip(wr, wi))
    parts = br._split3(wr)
    assert np.array_equal(parts[:2], parts[:2].astype(np.float32)) and np.abs(parts[2]).max() < 2.0 ** -45
    nt = 8
    ltf, _, _ = _packets(oracle, 31, 2, 2, nt, 10.0)
    a, b = br.noise_var(ltf, nt), br.noise_var(ltf, nt, exact=False)
    assert np.max(np.abs(a - b) / a) < 1e-12
    ltf, _, _ = _packets(oracle, 31, 2, 2, nt, None)
    a, b = br.noise_var(ltf, nt), br.noise_var(ltf, nt, exact=False)
    print('noise-free: nv %.3e, plain complex128 form off by %.3e' % (a.max(), np.max(np.abs(a - b) / a)))
    assert (a > 0).all() and a.max() < 1e-12


def test_guards_of_the_reference(oracle):
    ltf, _, h_ls = _packets(oracle, 5, 2, 2, 4, 10.0)
    # all-zero LS rows: zeros out, from the solve and from the recursion, and no fallback
    z = np.zeros_like(h_ls)
    out, nv, c = br.blind_ref(ltf, z)
    assert not out.any() and not c.any() and (nv > 0).all()
    got, fell = br.levinson_blind(z[0, 0].T.astype(np.complex128), c[0, 0], nv[0, 0], 4)
    assert not got.any() and not fell
    assert not br.noise_var(np.zeros_like(ltf), 4).any()
    # the input built to break a recursion step: that (packet, rx) falls back to its LS rows, bit for bit; its neighbour does not
    bad = br.break_input(h_ls, 1, 0)
    c = br.freq_corr(bad)
    nv = br.noise_var(ltf, 4)
    got, fell = br.levinson_blind(bad[1, 0].T.astype(np.complex128), c[1, 0], nv[1, 0], 4)
    assert fell and np.array_equal(got.astype(np.complex64).view(np.uint32), bad[1, 0].T.copy().view(np.uint32))
    got, fell = br.levinson_blind(bad[1, 1].T.astype(np.complex128), c[1, 1], nv[1, 1], 4)
    assert not fell and np.isfinite(got).all()


def test_noise_estimate_against_the_realised_ls_error(oracle):
    """Nt = 8, Nr = 2, 64 packets at 0 dB: nv / Nt over the realised LS error variance of the same (packet, rx), mean over the 128
    pairs, within 5 standard errors of 1.  One standard error: nv averages 14 * 8 squared magnitudes per pair, 1 / sqrt(14 * 8 * 128)
    = 0.84 % (the realised variance averages 8 * 234 and adds little)."""
    nt, nr, npkt = 8, 2, 64
    ltf, h, h_ls = _packets(oracle, 2024, npkt, nr, nt, 0.0)
    nv = br.noise_var(ltf, nt, exact=False)          # 0 dB: far above the rounding floor where the exact form matters
    realised = np.mean(np.abs(h_ls.astype(np.complex128) - h) ** 2, axis=(2, 3))
    ratio = float(np.mean(nv / nt / realised))
    se = 1.0 / np.sqrt(14 * nt * npkt * nr)
    print('mean of (nv / Nt) / realised LS error variance = %.4f (%.2f standard errors of %.4f)' % (ratio, (ratio - 1.0) / se, se))
    assert abs(ratio - 1.0) < 5.0 * se
    # and the smoother does what it is for on these packets
    out, _, _ = br.blind_ref(ltf[:4], h_ls[:4])
    ls, sm = br.nmse(h_ls[:4], h[:4]), br.nmse(out, h[:4])
    print('NMSE at 0 dB: LS %.4f -> smoothed %.4f' % (ls, sm))
    assert sm < 0.5 * ls
