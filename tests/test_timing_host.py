"""CPU tests of the symbol-timing stage (csi_sync_*, csrc/sync.hip.h).  They check the fp64 statement
tests/timing_ref.py on the oracle's own packets, so that the GPU tests stand on something - the start a packet embedded in a capture
returns, the offset and quality at that start, what a wrong start does to the LS estimate and what the estimated start leaves of it -
and the C-ABI surface and synth.timing_offsets."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfo_ref as cr         # noqa: E402
import timing_ref as tr      # noqa: E402

ENTRY_POINTS = ('csi_sync_embed_device', 'csi_sync_estimate_device', 'csi_sync_extract_device', 'csi_sync_correct_device', 'csi_sync_correct')


def _std_of(ltf, snr_db):
    """the deviation per real component of the noise inside an oracle packet batch at snr_db (the oracle scales it to the batch's mean
    power): the margins get the level of the packet's own noise"""
    if snr_db is None:
        return None
    snr = 10.0 ** (snr_db / 10.0)
    power = np.mean(np.abs(ltf) ** 2) * snr / (1.0 + snr)
    return np.full(ltf.shape[0], np.sqrt(0.5 * power / snr))


def _capture(oracle, pkg, nt, nr, npkt, span, snr_db, n_taps=8, with_eps=True):
    from dl_channel_estimation_mamimo_amd import synth
    rng = np.random.default_rng(100 * nt + span)
    ltf, h = oracle.make_structured_packets(rng, npkt, nr, oracle.hadamard(nt), snr_db=snr_db, n_taps=n_taps)
    eps = np.concatenate([[0.45, -0.45], rng.uniform(-0.45, 0.45, npkt)])[:npkt] if with_eps else np.zeros(npkt)
    theta = synth.timing_offsets(nt, 0, npkt, span)
    theta[0], theta[1] = 0, span
    x = cr.rotate(ltf, eps)
    cap, _ = tr.embed(x, theta, span, seed=nt, first_pkt=0, std=_std_of(ltf, snr_db))
    return ltf, h, x, cap, theta, eps


@pytest.mark.parametrize('snr_db', [None, 20.0], ids=['noise-free', '20dB'])
@pytest.mark.parametrize('nt,nr,span,n_taps,npkt', [(4, 1, 4, 8, 6), (4, 1, 256, 8, 6), (4, 2, 64, 64, 6), (32, 4, 256, 8, 4), (128, 1, 64, 8, 3)])
def test_every_start_is_found(oracle, pkg, nt, nr, span, n_taps, npkt, snr_db):
    _, _, x, cap, theta, eps = _capture(oracle, pkg, nt, nr, npkt, span, snr_db, n_taps)
    for rho in (1.0, 0.5):
        th, eps_hat, quality, lam, _ = tr.estimate(cap, span, rho)
        err = np.abs(cr.wrap(eps_hat - eps)).max()
        print(f'Nt {nt} Nr {nr} span {span} rho {rho} {"noise-free" if snr_db is None else "%g dB" % snr_db}: theta_hat == theta for '
              f'{int(np.sum(th == theta))} of {npkt}, |eps_hat - eps| <= {err:.2e}, quality {quality.min():.4f} .. {quality.max():.4f}, '
              f'smallest runner-up gap {tr.runner_up_gap(lam).min():.3e}')
        assert np.array_equal(th, theta), (rho, th, theta)
        if snr_db is None:
            assert err <= 1e-8                      # the window lies inside a noise-free packet: exact but for rounding
            assert np.abs(quality - 1.0).max() < 1e-9
        # the cut-out at the estimate returns the packet, and with eps_hat the unrotated one
        assert np.array_equal(tr.extract(cap, th, span), x)


def test_quality_is_snr_over_one_plus_snr(oracle, pkg):
    """the mean over the packets, as in the CFO stage's test: one packet's own snr follows its channel draw"""
    for snr_db in (0.0, 10.0, 20.0):
        _, _, _, cap, theta, _ = _capture(oracle, pkg, 32, 4, 8, 64, snr_db)
        th, _, quality, _, _ = tr.estimate(cap, 64)
        snr = 10.0 ** (snr_db / 10.0)
        print(f'{snr_db:g} dB: quality {quality.mean():.4f}, snr / (1 + snr) {snr / (1 + snr):.4f}, exact starts {int(np.sum(th == theta))} of 8')
        assert abs(quality.mean() - snr / (1.0 + snr)) < 0.02


def test_ls_nmse_at_the_fixed_cut_and_at_the_estimated_cut(oracle, pkg):
    """Nt = 8, Nr = 2, start uniform in 0 .. 64: the packet cut out at the fixed start 32 gives an LS NMSE near 2 at every SNR; cut
    out at the estimated start it gives the clean value, because every start is found and the cut-out is then the packet itself"""
    nt, nr, span, npkt = 8, 2, 64, 24
    P = oracle.hadamard(nt)
    for snr_db in (10.0, 20.0, 40.0):
        ltf, h, _, cap, theta, _ = _capture(oracle, pkg, nt, nr, npkt, span, snr_db, with_eps=False)
        clean = oracle.nmse_subk(h, oracle.ls_estimate(ltf, P))
        fixed = oracle.nmse_subk(h, oracle.ls_estimate(tr.extract(cap, np.full(npkt, span // 2), span), P))
        th = tr.estimate(cap, span)[0]
        found = oracle.nmse_subk(h, oracle.ls_estimate(tr.extract(cap, th, span), P))
        print(f'{snr_db:g} dB: LS NMSE clean {clean:.3e}, cut at the fixed start {fixed:.3f}, cut at the estimated start {found:.3e} '
              f'({int(np.sum(th == theta))} of {npkt} starts exact)')
        assert np.array_equal(th, theta)
        assert found == clean
        assert fixed > 1.0 and fixed > 5.0 * clean


def test_zero_capture_and_clamp(oracle):
    th, eps, quality, lam, _ = tr.estimate(np.zeros((2, 2, 320 * 4 + 64), np.complex128), 64)
    assert not th.any() and not eps.any() and not quality.any() and not lam.any()
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 1, 320 * 4)) + 1j * rng.standard_normal((4, 1, 320 * 4))
    wild = np.array([-5, 0, 8, 17])
    cap, inside = tr.embed(x, wild, 8)
    kept, _ = tr.embed(x, np.array([0, 0, 8, 8]), 8)
    assert np.array_equal(cap, kept) and inside.sum() == 4 * 320 * 4
    assert np.array_equal(tr.extract(cap, wild, 8), x)
    assert np.array_equal(tr.clamp([-2 ** 31, 2 ** 31 - 1, 3], 8), [0, 8, 3])


def test_margins_are_their_own_stream(oracle):
    """the margin draws differ from the packet's noise draws (kind 1) and from the next packet's taps (what a kind 2 would be)"""
    import synth_streams as st
    km = tr.margin_key(7, 3)
    assert km != st.key(7, 3, 1) and km != st.key(7, 4, 0) and km != tr.margin_key(7, 4) and km != tr.margin_key(8, 3)
    x = np.zeros((2, 2, 320 * 4), np.complex128)
    cap, inside = tr.embed(x, [3, 60], 64, seed=7, first_pkt=3, std=np.array([0.5, 0.0]))
    z = tr.margin_normals(7, 3, 2, 320 * 4 + 64)[0]
    assert np.array_equal(cap[0][:, ~inside[0]], 0.5 * z[:, ~inside[0]]) and not cap[0][:, inside[0]].any() and not cap[1].any()
    assert abs(np.std(cap[0][:, ~inside[0]].real) - 0.5) < 0.1
    sub, _ = tr.embed(x[1:], [60], 64, seed=7, first_pkt=4, std=np.array([0.5]))
    both, _ = tr.embed(x, [3, 60], 64, seed=7, first_pkt=3, std=np.array([0.5, 0.5]))
    assert np.array_equal(sub[0], both[1])


def test_offsets_of_a_sub_range(pkg):
    from dl_channel_estimation_mamimo_amd import synth
    a = synth.timing_offsets(11, 100, 64, 64)
    assert a.dtype == np.int32 and a.shape == (64,) and a.min() >= 0 and a.max() <= 64 and a.max() > 56 and a.min() < 8
    assert np.array_equal(synth.timing_offsets(11, 120, 8, 64), a[20:28])
    assert not np.array_equal(synth.timing_offsets(12, 100, 64, 64), a)
    big = synth.timing_offsets(3, 0, 51400, 256)
    counts = np.bincount(big, minlength=257)
    assert counts.size == 257 and counts.min() > 120 and counts.max() < 290          # 200 expected per start, both ends included
    small = synth.timing_offsets(3, 0, 1000, 4)
    assert set(small.tolist()) == {0, 1, 2, 3, 4}
    # independent of the frequency offsets of the same packets
    assert abs(np.corrcoef(synth.timing_offsets(3, 0, 20000, 256), synth.cfo_offsets(3, 0, 20000, 1.0))[0, 1]) < 0.03


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
    for k in ('sync_metric', 'sync_extract', 'sync_embed'):
        assert k in names and '"%s"' % k in header, k
    i = names.index('sync_metric')
    assert names[i - 1:i + 4] == ['forecast_apply', 'sync_metric', 'sync_extract', 'sync_embed', 'sounding_noise']
    assert names[-4:] == ['synth_scattering', 'lmmse_null_noise', 'lmmse_freq_corr', 'lmmse_blind']
    assert names.index('lmmse_levinson') == 11
    assert '"sync_launches"' in header
    para = header[header.index('Device pointers ('):header.index('An array of exactly the documented')]
    assert 'csi_sync_*_device' in para
    blob = open(pkg.library_path(), 'rb').read()
    for k in (b'sync_metric_kernel', b'sync_extract_kernel', b'sync_embed_kernel'):
        assert k in blob
    assert lib.csi_sync_embed_device(None, 1, 0, 1, 4, None, None, None, None, None, None) == -1          # a null context
    assert lib.csi_sync_estimate_device(None, None, None, 1, 4, 1.0, None, None, None, None) == -1
    assert lib.csi_sync_extract_device(None, None, None, 1, 4, None, None, None, None) == -1
    assert lib.csi_sync_correct_device(None, None, None, 1, 4, 1.0, 0, None, None, None, None, None) == -1
    assert lib.csi_sync_correct(None, None, None, 1, 4, 1.0, 0, None, None, None, None, None) == -1
    for m in ('sync_embed_device', 'sync_estimate_device', 'sync_extract_device', 'sync_correct_device', 'sync_correct'):
        assert hasattr(pkg.CsiEngine, m)
