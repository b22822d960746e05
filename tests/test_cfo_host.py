"""CPU tests of the carrier-frequency-offset stage (csi_cfo_*, csrc/cfo.hip.h).  They check the fp64 statement
tests/cfo_ref.py on the oracle's own packets, so that the GPU tests stand on something - the offset a noise-free packet returns, the
quality against snr / (1 + snr), the round trip, what the offset does to the LS estimate and what the correction leaves of it - and
the C-ABI surface and synth.cfo_offsets."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfo_ref as cr      # noqa: E402

ENTRY_POINTS = ('csi_cfo_estimate_device', 'csi_cfo_rotate_device', 'csi_cfo_correct_device', 'csi_cfo_correct')


@pytest.mark.parametrize('nt,nr', [(4, 1), (8, 2), (32, 4)])
def test_noise_free_packets_return_their_offset(oracle, nt, nr):
    rng = np.random.default_rng(nt)
    npkt = 6
    ltf, _ = oracle.make_structured_packets(rng, npkt, nr, oracle.hadamard(nt), snr_db=None)
    eps = np.concatenate([[0.45, -0.45], rng.uniform(-0.45, 0.45, npkt - 2)])
    y = cr.rotate(ltf, eps)
    for cp_skip in (0, 16, 63):
        got, quality = cr.estimate(y, cp_skip)
        print(f'Nt {nt} Nr {nr} cp_skip {cp_skip}: |eps_hat - eps| <= {np.abs(got - eps).max():.2e}, 1 - quality <= {np.abs(1 - quality).max():.2e}')
        assert np.abs(got - eps).max() <= 1e-15
        assert np.abs(quality - 1.0).max() < 1e-12


def test_quality_is_snr_over_one_plus_snr(oracle):
    """The mean over 8 packets, the figure a level of the sweep reports.  One packet's own quality scatters around it: the oracle sets
    the noise against the mean power of the batch, so a packet's own snr follows its channel draw, and 8192 correlated samples leave a
    standard deviation near 0.01 on top."""
    rng = np.random.default_rng(5)
    P = oracle.hadamard(32)
    for snr_db in (0.0, 10.0, 20.0):
        ltf, _ = oracle.make_structured_packets(rng, 8, 4, P, snr_db=snr_db)
        y = cr.rotate(ltf, rng.uniform(-0.3, 0.3, 8))
        snr = 10.0 ** (snr_db / 10.0)
        quality = cr.estimate(y)[1]
        print(f'{snr_db:g} dB: quality {quality.mean():.4f}, snr / (1 + snr) {snr / (1 + snr):.4f}')
        assert abs(quality.mean() - snr / (1.0 + snr)) < 0.02


def test_round_trip_and_zero_packet(oracle):
    rng = np.random.default_rng(6)
    ltf, _ = oracle.make_structured_packets(rng, 3, 2, oracle.hadamard(8), snr_db=10.0)
    eps = np.array([0.49999, -0.2, 0.0])
    back = cr.rotate(cr.rotate(ltf, eps), eps, -1.0)
    assert np.abs(back - ltf).max() <= 1e-13 * np.abs(ltf).max()
    assert np.array_equal(cr.rotate(ltf, eps)[2], ltf[2])
    e, q = cr.estimate(np.zeros((2, 2, 320 * 8), np.complex128))
    assert not e.any() and not q.any()


def test_ls_nmse_under_an_offset_and_after_the_correction(oracle):
    """Nt = 32, Nr = 4, eps uniform in +-0.01: corrected within 1.15 of clean at 10 / 20 / 40 dB, uncorrected above 3 x clean at 20 dB"""
    P = oracle.hadamard(32)
    for snr_db in (10.0, 20.0, 40.0):
        rng = np.random.default_rng(7)
        ltf, h = oracle.make_structured_packets(rng, 8, 4, P, snr_db=snr_db)
        y = cr.rotate(ltf, rng.uniform(-0.01, 0.01, 8))
        clean = oracle.nmse_subk(h, oracle.ls_estimate(ltf, P))
        offset = oracle.nmse_subk(h, oracle.ls_estimate(y, P))
        fixed = oracle.nmse_subk(h, oracle.ls_estimate(cr.correct(y)[0], P))
        print(f'{snr_db:g} dB: LS NMSE clean {clean:.3e}, offset {offset:.3e} ({offset / clean:.1f} x), corrected {fixed:.3e} ({fixed / clean:.3f} x)')
        assert fixed <= 1.15 * clean, (snr_db, fixed, clean)
        if snr_db == 20.0:
            assert offset > 3.0 * clean, (offset, clean)


def test_offsets_of_a_sub_range(pkg):
    from dl_channel_estimation_mamimo_amd import synth
    a = synth.cfo_offsets(11, 100, 64, 0.25)
    assert a.dtype == np.float64 and a.shape == (64,) and np.abs(a).max() <= 0.25 and np.abs(a).max() > 0.2
    assert np.array_equal(synth.cfo_offsets(11, 120, 8, 0.25), a[20:28])
    assert np.array_equal(synth.cfo_offsets(11, 100, 64, 0.5), 2.0 * a)
    assert not np.array_equal(synth.cfo_offsets(12, 100, 64, 0.25), a)
    assert abs(np.mean(synth.cfo_offsets(3, 0, 20000, 1.0))) < 0.02


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
    for k in ('cfo_corr', 'cfo_rotate'):
        assert k in names and '"%s"' % k in header, k
    assert names.index('cfo_rotate') + 1 == names.index('synth_scattering') and names.index('sounding_noise') + 1 == names.index('cfo_corr')
    assert names[-4:] == ['synth_scattering', 'lmmse_null_noise', 'lmmse_freq_corr', 'lmmse_blind']
    assert names.index('lmmse_levinson') == 11
    assert '"cfo_launches"' in header
    blob = open(pkg.library_path(), 'rb').read()
    for k in (b'cfo_corr_kernel', b'cfo_rotate_kernel'):
        assert k in blob
    assert lib.csi_cfo_estimate_device(None, None, None, 1, 0, None, None) == -1          # a null context
    assert lib.csi_cfo_rotate_device(None, None, None, 1, None, 1.0, None, None) == -1
    assert lib.csi_cfo_correct_device(None, None, None, 1, 0, None, None, None, None) == -1
    assert lib.csi_cfo_correct(None, None, None, 1, 0, None, None, None, None) == -1
    for m in ('cfo_estimate_device', 'cfo_rotate_device', 'cfo_correct_device', 'cfo_correct'):
        assert hasattr(pkg.CsiEngine, m)
