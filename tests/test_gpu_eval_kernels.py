"""GPU tests (-m gpu) of the two kernels behind every number of the NMSE-vs-SNR sweep: the LMMSE smoother (csrc/lmmse.hip.h,
csi_lmmse_estimate[_device]) against the fp64 reference tests/lmmse_ref.py over delay-spread / SNR regimes, column layouts, the
zero-hvec row and the host entry point's packet chunks; the NMSE metric (csrc/metrics.hip.h, csi_nmse[_device]) against fp64 numpy
over bin counts, the grid-stride loop, the long sum, link scales and the host entry point's link chunks.  Engines carry no model and
no pilot: the LS planes are random complex64 and no LS kernel runs.

csi_create admits only antenna counts that are multiples of 4 (16-byte rows; test_odd_antenna_counts_are_refused), so the column
counts here are the admissible ones next to the 32-column workgroup boundary: the shortest tail a workgroup can have is 4 columns."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lmmse_ref as lr      # noqa: E402

TOL_LMMSE = 1e-6      # fp64 recursion, one fp32 rounding on the way out (6e-8); its host restatement measures 5e-8 (test_lmmse_ref_host.py)
TOL_60DB = 1e-5       # the BASELINE.json contract: R + s I has a condition number of 1e8 and more at 60 dB


def _cplx(rng, shape):
    return (rng.standard_normal(shape, dtype=np.float32) + 1j * rng.standard_normal(shape, dtype=np.float32)).astype(np.complex64)


def _engine(pkg, nt, nr):
    return pkg.CsiEngine(nt, nr, hidden=(8,))


def _tap_profile8():
    from dl_channel_estimation_mamimo_amd import sweep
    return sweep.tap_profile(8)


def _lmmse_device(e, h_ls, hvec, snr_db):
    """csi_lmmse_estimate_device on uploaded planes -> complex64"""
    h_ls = np.asarray(h_ls)
    hvec, snr_db = np.ascontiguousarray(hvec, np.float32), np.ascontiguousarray(snr_db, np.float32)
    d_re, d_im = e.to_device(h_ls.real), e.to_device(h_ls.imag)
    d_hv, d_snr = e.to_device(hvec), e.to_device(snr_db)
    o_re, o_im = e.empty(h_ls.shape), e.empty(h_ls.shape)
    e.lmmse_estimate_device(d_re, d_im, h_ls.shape[0], d_hv, hvec.shape[1], d_snr, o_re, o_im)
    e.synchronize()
    out = (o_re.download() + 1j * o_im.download()).astype(np.complex64)
    for a in (d_re, d_im, d_hv, d_snr, o_re, o_im):
        a.free()
    return out


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.real.view(np.uint32), b.real.view(np.uint32)) \
        and np.array_equal(a.imag.view(np.uint32), b.imag.view(np.uint32))


# ------------------------------------------------------------------------------------ LMMSE smoother
def test_lmmse_regimes_against_the_reference(pkg):
    """Six delay profiles (tau_rms 0 ... 99.5 bins) x five SNR levels (-25 ... 60 dB), R + s I from well conditioned to 1e8 and
    more: every packet of a call has its own profile and every (packet, rx) its own level, three calls cover the grid.  Both
    entry points, the same bits.  The table it prints is kept in profiles/lmmse_regimes.txt."""
    rng = np.random.default_rng(51)
    npkt, nr, nt = 6, 2, 4
    prof = lr.profiles(_tap_profile8())
    names = list(prof)
    assert len(names) == npkt
    hvec = lr.pad([prof[n] for n in names])                  # L = 200; the one-tap row of length 1 runs in the known-answer test
    e = _engine(pkg, nt, nr)
    worst = {}
    for call in range(3):
        h_ls = _cplx(rng, (npkt, nr, nt, 234))
        level = np.array([[(p + 2 * call + r) % 5 for r in range(nr)] for p in range(npkt)])
        snr = np.asarray(lr.SNR_GRID, np.float32)[level]
        got = e.lmmse_estimate(h_ls, hvec, snr)
        assert got.shape == h_ls.shape and got.dtype == np.complex64
        assert _same_bits(got, _lmmse_device(e, h_ls, hvec, snr)), 'csi_lmmse_estimate and csi_lmmse_estimate_device differ'
        err = lr.rel_rows_c(got, lr.lmmse_ref(h_ls, hvec, snr)).max(axis=2)
        for p in range(npkt):
            for r in range(nr):
                key = (names[p], float(snr[p, r]))
                worst[key] = max(worst.get(key, 0.0), float(err[p, r]))
    assert len(worst) == len(names) * len(lr.SNR_GRID)
    print('\nLMMSE on the device vs lmmse_ref, max norm-relative row error (bounds: %g up to 40 dB, %g at 60 dB)' % (TOL_LMMSE, TOL_60DB))
    print('%-16s %9s' % ('profile', 'tau_rms') + ''.join('%11g dB' % s for s in lr.SNR_GRID))
    for n in names:
        print('%-16s %9.4f' % (n, lr.tau_rms(prof[n])) + ''.join('%14.3e' % worst[(n, s)] for s in lr.SNR_GRID))
    lo = max(v for (n, s), v in worst.items() if s <= 40.0)
    hi = max(v for (n, s), v in worst.items() if s > 40.0)
    print('maxima: %.3e up to 40 dB, %.3e at 60 dB' % (lo, hi))
    assert lo < TOL_LMMSE, sorted((v, k) for k, v in worst.items() if k[1] <= 40.0)[-3:]
    assert hi < TOL_60DB, sorted((v, k) for k, v in worst.items() if k[1] > 40.0)[-3:]


def test_lmmse_known_answer_on_the_device(pkg):
    """A one-tap hvec (L = 1) makes R the all-ones matrix, and a channel constant over the bins is its eigenvector:
    H_mmse = H 234 / (234 + s).  At 60 dB with the flat profile (smallest eigenvalue of R ~ 2e-3 >> s) the smoother is nearly
    the identity."""
    rng = np.random.default_rng(52)
    npkt, nr, nt = 2, 2, 4
    e = _engine(pkg, nt, nr)
    a = _cplx(rng, (npkt, nr, nt))
    h_ls = np.ascontiguousarray(np.repeat(a[..., None], 234, axis=-1))
    snr = np.array([[-10.0, 20.0], [20.0, -10.0]], np.float32)
    got = e.lmmse_estimate(h_ls, np.array([[0.75], [3.0]], np.float32), snr)
    s = 10.0 ** (-snr.astype(np.float64) / 10.0)
    want = h_ls.astype(np.complex128) * (234.0 / (234.0 + s))[:, :, None, None]
    err = lr.rel_rows_c(got, want).max()
    print(f'one tap, constant channel: device vs H 234 / (234 + s) {err:.3e}')
    assert err < 1e-6
    h2 = _cplx(rng, (npkt, nr, nt, 234))
    out = e.lmmse_estimate(h2, np.ones((npkt, 100), np.float32), np.full((npkt, nr), 60.0, np.float32))
    moved = lr.rel_rows_c(out, h2).max()
    print(f'flat profile at 60 dB: |out - in| / |in| {moved:.3e}')
    assert moved < 1e-3


@pytest.mark.parametrize('nt', [3, 5, 31, 33, 65])
def test_odd_antenna_counts_are_refused(pkg, nt):
    """why no test here runs them: the context itself does not exist"""
    with pytest.raises(pkg.CsiError, match='multiple of 4'):
        _engine(pkg, nt, 2)


@pytest.mark.parametrize('nt', [4, 28, 32, 36, 68, 128])
def test_lmmse_column_layout(pkg, nt):
    """Every nt fills or crosses the 32-column workgroup differently: a short one, one short of full, full, just over, two full
    and a tail, four full.  At nt = 68: a permutation of the tx columns permutes the output bit for bit - every right-hand side
    runs the same arithmetic whatever its lane group and workgroup -, and a zero column comes back exactly zero without touching
    the others."""
    rng = np.random.default_rng(530 + nt)
    npkt, nr = 2, 2
    e = _engine(pkg, nt, nr)
    h_ls = _cplx(rng, (npkt, nr, nt, 234))
    hvec = np.tile(_tap_profile8(), (npkt, 1))
    snr = np.full((npkt, nr), 10.0, np.float32)
    got = e.lmmse_estimate(h_ls, hvec, snr)
    err = lr.rel_rows_c(got, lr.lmmse_ref(h_ls, hvec, snr)).max()
    print(f'nt {nt}: device vs lmmse_ref {err:.3e}')
    assert err < TOL_LMMSE
    if nt != 68:
        return
    perm = np.random.default_rng(53).permutation(nt)
    assert (perm // 32 != np.arange(nt) // 32).sum() > 16          # columns change workgroup, not only lane group
    assert _same_bits(e.lmmse_estimate(np.ascontiguousarray(h_ls[:, :, perm]), hvec, snr), got[:, :, perm])
    holed = h_ls.copy()
    holed[:, :, 40] = 0
    out = e.lmmse_estimate(holed, hvec, snr)
    assert (out[:, :, 40] == 0).all()
    keep = np.arange(nt) != 40
    assert _same_bits(out[:, :, keep], got[:, :, keep])


def test_lmmse_zero_hvec_row_is_zero_delay_spread(pkg):
    """An all-zero hvec row means tau_rms = 0 (include/csi_mamimo.h; the reference formula divides 0 by 0 there): the packet's
    output is that of a one-tap row, bit for bit, and its neighbours are what they are without it."""
    rng = np.random.default_rng(54)
    npkt, nr, nt = 3, 2, 4
    e = _engine(pkg, nt, nr)
    h_ls = _cplx(rng, (npkt, nr, nt, 234))
    snr = np.array([[0.0, 15.0], [5.0, 30.0], [-5.0, 10.0]], np.float32)
    hvec = np.tile(_tap_profile8(), (npkt, 1))
    hvec[1] = 0.0
    one_tap = hvec.copy()
    one_tap[1, 0] = 1.0
    for run in (e.lmmse_estimate, lambda *a: _lmmse_device(e, *a)):
        got = run(h_ls, hvec, snr)
        assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
        assert _same_bits(got, run(h_ls, one_tap, snr))
        assert _same_bits(got[[0, 2]], run(h_ls[[0, 2]], hvec[[0, 2]], snr[[0, 2]]))
        err = lr.rel_rows_c(got, lr.lmmse_ref(h_ls, hvec, snr)).max()
        assert err < TOL_LMMSE, err
    # and the zero-spread smoother did something: the packet moved, by another amount than under the sweep profile
    assert np.linalg.norm(got[1] - h_ls[1]) > 1e-2 * np.linalg.norm(h_ls[1])
    assert not _same_bits(got[1], e.lmmse_estimate(h_ls, np.tile(_tap_profile8(), (npkt, 1)), snr)[1])


def test_lmmse_host_chunk_boundary(pkg, oracle):
    """csi_lmmse_estimate stages 2^28 / (16 nr nt 234) packets at a time: 35 at nt = 128, nr = 16, so 37 packets leave a second
    chunk of 2, whose hvec rows start at 35 L and whose SNR values at 35 nr.  Every packet has its own profile and every
    (packet, rx) its own SNR: the packets on both sides of the boundary equal the device entry point's result on each alone."""
    rng = np.random.default_rng(55)
    nt, nr, npkt = 128, 16, 37
    assert (1 << 28) // (16 * nr * nt * 234) == 35
    e = _engine(pkg, nt, nr)
    base = _cplx(rng, (nr, nt, 234))
    gain = (1.0 + 0.03125 * np.arange(npkt)).astype(np.float32)
    h_ls = base[None] * gain[:, None, None, None]
    assert h_ls.dtype == np.complex64
    hvec = (_tap_profile8().astype(np.float64)[None, :] ** (1.0 + 0.1 * np.arange(npkt))[:, None]).astype(np.float32)
    snr = (-10.0 + 0.05 * np.arange(npkt * nr)).reshape(npkt, nr).astype(np.float32)
    assert np.unique(snr).size == npkt * nr and np.unique(hvec, axis=0).shape[0] == npkt
    got = e.lmmse_estimate(h_ls, hvec, snr)
    for p in (0, 34, 35, 36):
        alone = _lmmse_device(e, h_ls[p:p + 1], hvec[p:p + 1], snr[p:p + 1])
        assert _same_bits(got[p:p + 1], alone), f'packet {p} differs from the same packet smoothed alone'
    for r, j in ((0, 0), (7, 65), (15, 127)):
        want = oracle.lmmse_estimate(h_ls[36:, r:r + 1, j:j + 1], hvec[36:].astype(np.float64), snr[36:, r:r + 1].astype(np.float64))
        err = lr.rel_rows_c(got[36:, r:r + 1, j:j + 1], want).max()
        print(f'packet 36 link (rx {r}, tx {j}) vs oracle.lmmse_estimate {err:.3e}')
        assert err < 1e-6


# ------------------------------------------------------------------------------------ NMSE metric
def _ratios64(ref, est):
    ref = ref.astype(np.complex128)
    return (np.abs(ref - est) ** 2).sum(-1) / (np.abs(ref) ** 2).sum(-1)


def _nmse_device(e, ref, est):
    """csi_nmse_device on uploaded planes -> (mean, float32 per-link ratios)"""
    d = [e.to_device(p) for p in (ref.real, ref.imag, est.real, est.imag)]
    per = e.empty((ref.shape[0],))
    mean = e.nmse_device(d[0], d[1], d[2], d[3], ref.shape[0], ref.shape[1], per)
    ratios = per.download()
    for a in d + [per]:
        a.free()
    return mean, ratios


@pytest.fixture(scope='module')
def engine8(pkg):
    return _engine(pkg, 8, 2)


@pytest.mark.parametrize('n_bins', [1, 63, 64, 65, 234, 1000])
def test_nmse_bin_counts(engine8, n_bins):
    """Bin counts below, at and around one wave, and above it; 37 links.  est = ref / 2 and est = ref have exact answers: every
    product and sum of the first is a quarter of the matching one of the denominator."""
    e = engine8
    rng = np.random.default_rng(600 + n_bins)
    ref = _cplx(rng, (37, n_bins))
    est = (ref + np.float32(0.05) * _cplx(rng, ref.shape)).astype(np.complex64)
    want = _ratios64(ref, est)
    mean, ratios = _nmse_device(e, ref, est)
    host = e.nmse(ref, est)
    print(f'n_bins {n_bins}: mean {abs(mean / want.mean() - 1):.3e}, ratios {np.abs(ratios / want - 1).max():.3e} (relative)')
    np.testing.assert_allclose(ratios, want, rtol=2e-6)
    assert abs(mean - want.mean()) <= 1e-6 * want.mean()
    assert abs(host - want.mean()) <= 1e-6 * want.mean()          # (mean * 37) / 37 of csi_nmse need not be mean to the last bit
    half = (np.float32(0.5) * ref).astype(np.complex64)
    mean_h, ratios_h = _nmse_device(e, ref, half)
    assert mean_h == 0.25 and (ratios_h == np.float32(0.25)).all() and e.nmse(ref, half) == 0.25
    mean_0, ratios_0 = _nmse_device(e, ref, ref)
    assert mean_0 == 0.0 and (ratios_0 == 0).all() and e.nmse(ref, ref) == 0.0


def test_nmse_grid_stride_and_long_sum(engine8):
    """40001 links: more than the 8192 workgroups x 4 waves of one pass, and 39 or 40 terms per thread of the 1024-way sum.
    Every link has its own error level, so a link left out or taken twice moves the mean."""
    e = engine8
    rng = np.random.default_rng(61)
    nlinks, n_bins = 40001, 16
    ref = _cplx(rng, (nlinks, n_bins))
    level = (0.01 * (1 + np.arange(nlinks) % 7)).astype(np.float32)
    est = (ref + level[:, None] * _cplx(rng, ref.shape)).astype(np.complex64)
    want = _ratios64(ref, est)
    mean, ratios = _nmse_device(e, ref, est)
    print(f'40001 links: mean {abs(mean / want.mean() - 1):.3e}, ratios {np.abs(ratios / want - 1).max():.3e} (relative)')
    np.testing.assert_allclose(ratios, want, rtol=2e-6)
    assert abs(mean - want.mean()) <= 1e-6 * want.mean()
    again, ratios2 = _nmse_device(e, ref, est)
    assert again == mean and np.array_equal(ratios, ratios2)
    assert abs(e.nmse(ref, est) - want.mean()) <= 1e-6 * want.mean()


def test_nmse_scale_invariance(engine8):
    """Link l scaled by 2^(-40 + 2 l): exact in fp32, and the squares (2^-80 ... 2^64) are exact in the fp64 sums, so ratios and
    mean keep their bits.  fp32 sums would leave their range."""
    e = engine8
    rng = np.random.default_rng(62)
    ref = _cplx(rng, (37, 234))
    est = (ref + np.float32(0.05) * _cplx(rng, ref.shape)).astype(np.complex64)
    scale = np.ldexp(np.float32(1.0), -40 + 2 * np.arange(37)).astype(np.float32)[:, None]
    mean, ratios = _nmse_device(e, ref, est)
    mean_s, ratios_s = _nmse_device(e, ref * scale, est * scale)
    assert (ref * scale).dtype == np.complex64
    assert np.array_equal(ratios.view(np.uint32), ratios_s.view(np.uint32))
    assert mean_s == mean
    assert e.nmse(ref * scale, est * scale) == e.nmse(ref, est)


def test_nmse_host_chunk_boundary(engine8):
    """csi_nmse stages 2^28 / (16 n_bins) links at a time, 71697 at 234 bins, and weighs every chunk's mean with its link count:
    80000 links leave a ragged second chunk of 8303.  Error level 0.05 in the first chunk and 0.5 behind it: the unweighted mean
    of the two chunk means is about 4 times the true mean, and a chunk read from a wrong offset has the wrong level."""
    e = engine8
    rng = np.random.default_rng(63)
    nlinks, n_bins, tile = 80000, 234, 2000
    chunk = (1 << 28) // (16 * n_bins)
    assert chunk == 71697 and nlinks - chunk == 8303
    gain = np.ldexp(np.float32(1.0), np.arange(nlinks) % 5).astype(np.float32)[:, None]          # links of one tile row differ
    level = np.where(np.arange(nlinks) < chunk, np.float32(0.05), np.float32(0.5)).astype(np.float32)[:, None]
    base_r, base_n = _cplx(rng, (tile, n_bins)), _cplx(rng, (tile, n_bins))
    planes = []
    for part in (base_r.real, base_r.imag):
        planes.append(np.tile(part, (nlinks // tile, 1)) * gain)
    for k, part in enumerate((base_n.real, base_n.imag)):
        planes.append(planes[k] + np.tile(part, (nlinks // tile, 1)) * gain * level)
    assert all(p.dtype == np.float32 and p.shape == (nlinks, n_bins) and p.flags.c_contiguous for p in planes)
    want, step = 0.0, 10000
    for l0 in range(0, nlinks, step):
        rr, ri, er, ei = (p[l0:l0 + step].astype(np.float64) for p in planes)
        want += (((rr - er) ** 2 + (ri - ei) ** 2).sum(-1) / (rr ** 2 + ri ** 2).sum(-1)).sum()
    want /= nlinks
    out = ctypes.c_double(0.0)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    e._check(e._lib.csi_nmse(e._ctx, fp(planes[0]), fp(planes[1]), fp(planes[2]), fp(planes[3]), nlinks, n_bins, ctypes.byref(out)))
    print(f'80000 links in two chunks: host entry point {out.value:.9e}, fp64 numpy {want:.9e}, relative {abs(out.value / want - 1):.3e}')
    assert abs(out.value - want) <= 1e-6 * want
