"""GPU tests of the hybrid beamforming weights (csrc/hybrid_weights.hip.h) in the regimes the replay of tests/test_gpu_hybrid.py does
not reach: the singular vectors themselves (a pursuit over a whole unitary dictionary hands Fopt back), items of one wave that stop
at different steps and a stop_tol other than the default, equal dictionary columns (lowest index on a tie) and the stop on a column
inside the span of the earlier ones, inputs scaled by 2^+-40 and all-zero items.  The inputs come from tests/hybrid_ref.py, whose
designs tests/test_hybrid_host.py checks with the fp64 definition; every bound is the replay's (TOL, GAP_MIN, 1 % left out) or exact."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hybrid_ref as R      # noqa: E402
from test_gpu_hybrid import GAP_MIN, TOL, check_items, dictionary, engine      # noqa: E402

N = R.N


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def device_call(pkg, e, h, ns, ntrf, stop_tol=0.0):
    """csi_hybrid_weights_device on fresh arrays (h_eval NULL) -> HybridWeights like the host entry point's"""
    npkt, _, nt, _ = h.shape
    d_h = [e.to_device(np.ascontiguousarray(h.real)), e.to_device(np.ascontiguousarray(h.imag))]
    d_f = [e.empty((npkt, N, ns, ntrf)) for _ in range(2)]
    d_idx, d_na, d_gain = e.empty((npkt, N, ntrf)), e.empty((npkt, N)), e.empty((npkt, N))
    d_m = [e.empty((npkt, ntrf, nt)) for _ in range(2)]
    e.hybrid_weights_device(d_h[0], d_h[1], npkt, ns, ntrf, d_f[0], d_f[1], d_idx, d_na, d_gain, d_m[0], d_m[1], stop_tol=stop_tol)
    e.synchronize()
    out = pkg.HybridWeights((d_f[0].download() + 1j * d_f[1].download()).astype(np.complex64), d_idx.download().view(np.int32),
                                   d_na.download().view(np.int32), d_gain.download(), (d_m[0].download() + 1j * d_m[1].download()).astype(np.complex64))
    for d in d_h + d_f + d_m + [d_idx, d_na, d_gain]:
        d.free()
    return out


def slots_are_consistent(tag, w, rays):
    """idx: valid and distinct in front of the stop, -1 with zero coefficients behind it; n_atoms counts the valid ones"""
    ntrf = w.idx.shape[-1]
    idx, na, fbb = w.idx.reshape(-1, ntrf), w.n_atoms.reshape(-1), w.fbb.reshape(-1, w.fbb.shape[-2], ntrf)
    used = np.arange(ntrf)[None, :] < na[:, None]
    assert (na >= 1).all() and (na <= ntrf).all(), (tag, np.unique(na))
    assert ((idx >= 0) & (idx < rays))[used].all() and (idx[~used] == -1).all(), tag
    assert (fbb.transpose(0, 2, 1)[~used] == 0).all(), tag + ': a coefficient behind the stop'
    srt = np.sort(np.where(used, idx, -1 - np.arange(ntrf)[None, :]), axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), tag + ': an item chose the same column twice'


# ------------------------------------------------------------------------------------------------ 2. the singular vectors, directly
@pytest.mark.parametrize('nt,nr,ns', R.FULL_SPAN_CASES)
def test_full_span_pursuit_returns_fopt(pkg, oracle, nt, nr, ns):
    """At = the unitary DFT matrix, NtRF = rays = Nt: after the last step A C = Fopt, so frf^T fbb^T is Fopt itself and the gain against
    the input is the sum of the ns largest squared singular values - on every item, without a gap mask: the energy a subspace
    captures is stationary in the subspace.  The projector is checked by check_items under its gap rule."""
    h = R.ls_csi(oracle, nt, nr, R.FULL_SPAN_SNR, R.FULL_SPAN_PACKETS)
    At = R.dft_dictionary(nt)
    e = engine(pkg, nt, nr, At)
    w = e.hybrid_weights(h, ns=ns, ntrf=nt)
    n = h.shape[0] * N
    tag = 'full span Nt %d Nr %d Ns %d (%d lanes per workgroup)' % (nt, nr, ns, R.svd_lanes(nr))
    assert (w.n_atoms == nt).all(), (tag, np.unique(w.n_atoms))
    H = R.csi_to_items(h)
    _, sv = R.fopt_of(H, ns)
    err = np.abs(w.gain.reshape(n) / (sv[:, :ns] ** 2).sum(axis=1) - 1.0)
    print('%s: |gain / sum of the %d largest sigma^2 - 1| max %.3g at item %d (bound %.0e)' % (tag, ns, err.max(), int(err.argmax()), TOL))
    assert err.max() <= TOL, (tag, err.max(), int(err.argmax()))
    check_items(tag, H, H, At, ns, nt, w.fbb.reshape(n, ns, nt), w.idx.reshape(n, nt), w.n_atoms.reshape(n), w.gain.reshape(n))


# ------------------------------------------------------------------------------------------------ 3. mixed stopping inside one wave
_MIXED = {}


def _mixed():
    if not _MIXED:
        h, At, kind, cols = R.mixed_stop_inputs()
        _MIXED.update(h=h, At=At, kind=kind, cols=cols, H=R.csi_to_items(h))
    return _MIXED


@pytest.mark.parametrize('stop_tol', list(R.MIXED_STOP_TABLE), ids=lambda t: 'default' if t is None else 'stop_tol_%g' % t)
def test_items_of_one_wave_stop_at_different_steps(pkg, stop_tol):
    """Subcarrier k is built from 1 + k % 4 dictionary columns (kind 4: white), so the four stop steps alternate along the lanes of
    every wave and the later correlation / solve launches run over finished neighbours.  Both entry points, the default stop_tol and the
    two of hybrid_ref.MIXED_STOP_TABLE: the designed atom counts, the fp64 definition's indices (its own choices: every one of them
    is at least 1e-3 from a tie, tests/test_hybrid_host.py), empty slots, the mean of the analog part, weights and gain."""
    m = _mixed()
    h, At, kind, cols, H = m['h'], m['At'], m['kind'], m['cols'], m['H']
    nt, nr, ntrf, ns = R.MIXED_NT, R.MIXED_NR, R.MIXED_NTRF, 1
    tol = 0.0 if stop_tol is None else stop_tol
    e = engine(pkg, nt, nr, At)
    w = e.hybrid_weights(h, ns=ns, ntrf=ntrf, stop_tol=tol)
    wd = device_call(pkg, e, h, ns, ntrf, tol)
    for name, x, y in zip(w._fields, w, wd):
        assert same_bits(x, y), 'host-pointer and device-pointer entry points differ in ' + name
    n = h.shape[0] * N
    tag = 'mixed stop, stop_tol %s' % ('default' if stop_tol is None else stop_tol)
    idx, na, fbb, gain = w.idx.reshape(n, ntrf), w.n_atoms.reshape(n), w.fbb.reshape(n, ns, ntrf), w.gain.reshape(n)
    want_na = R.mixed_stop_counts(kind, stop_tol)
    wrong = np.flatnonzero(na != want_na)
    assert wrong.size == 0, (tag, 'n_atoms', wrong[:8], na[wrong[:8]], want_na[wrong[:8]])
    slots_are_consistent(tag, w, At.shape[1])
    # the designed columns in descending-magnitude order, as far as the item got
    for t in (1, 2, 3):
        sel = kind == t
        k = int(want_na[sel][0])
        assert np.array_equal(idx[sel, :k], cols[sel, :k]), (tag, 'kind %d' % t)
    fbb_ref, idx_ref, na_ref = R.omp(H, At, ns, ntrf, R.DEFAULT_STOP_TOL if stop_tol is None else stop_tol)
    assert np.array_equal(na_ref, want_na) and np.array_equal(idx, idx_ref), tag
    # frf_mean: the mean of At[:, idx] with the empty slots as zeros
    frf = pkg.frf_from_idx(At.astype(np.complex128), w.idx)
    err = np.abs(w.frf_mean - frf.mean(axis=1)).max()
    print('%s: frf_mean absolute error max %.3g' % (tag, err))
    assert err <= 1e-6
    # weights against the definition (the gap rule of check_items: the white items have a second singular value) and the gain
    T, T_ref = R.weights_matrix(At, idx, fbb), R.weights_matrix(At, idx_ref, fbb_ref)
    _, sv = R.fopt_of(H, ns)
    g = R.gap_at_cut(sv, ns)
    keep = g >= GAP_MIN
    ratio = R.projector_error(T, T_ref) / (TOL * np.maximum(1.0, 0.1 / g))
    print('%s: projector error / bound max %.3g, left out %.4f' % (tag, ratio[keep].max(), 1.0 - keep.mean()))
    assert 1.0 - keep.mean() <= 0.01 and ratio[keep].max() <= 1.0, (tag, ratio[keep].max())
    # fbb itself where Fopt is unique up to a phase (rank-one items): aligned by that phase
    r1 = kind < 4
    ph = (fbb[r1] * np.conj(fbb_ref[r1])).sum((1, 2))
    err = np.abs(fbb[r1] * (np.conj(ph) / np.abs(ph))[:, None, None] - fbb_ref[r1]).max()
    print('%s: fbb of the rank-one items (phase aligned) absolute error max %.3g' % (tag, err))
    assert err <= TOL
    g_own, g_ref = R.gain(H, T), R.gain(H, T_ref)
    err = np.abs(gain / g_own - 1.0).max()
    err_ref = np.abs(gain[r1] / g_ref[r1] - 1.0).max()
    print('%s: gain relative error max %.3g from its own weights, %.3g from the definition\'s on the rank-one items' % (tag, err, err_ref))
    assert err <= TOL and err_ref <= TOL


# ------------------------------------------------------------------------------------------------ 4. ties and the span stop
def test_equal_columns_go_to_the_lower_index(pkg):
    """Four dictionary columns are copies of lower ones: in another register of the same lane, in the other half wave, in another
    tile of 32 rays and in the partial last tile.  Equal columns pass through the same fp32 operations, so their metrics have equal
    bits and the lower index must win everywhere."""
    h, At, want = R.tie_inputs()
    e = engine(pkg, R.TIE_NT, R.TIE_NR, At)
    w = e.hybrid_weights(h, ns=1, ntrf=1)
    idx = w.idx.reshape(-1)
    for copy, orig in R.TIE_COPIES:
        sel = want == min(copy, orig)
        print('pair (%d, %d): %d items, chosen %s' % (orig, copy, sel.sum(), np.unique(idx[sel]).tolist()))
    wrong = np.flatnonzero(idx != want)
    assert wrong.size == 0, ('items', wrong[:8], 'chose', idx[wrong[:8]], 'for', want[wrong[:8]])
    assert (w.n_atoms == 1).all()
    nrm = np.linalg.norm(At.astype(np.complex128)[:, idx], axis=0)
    err = np.abs(np.abs(w.fbb.reshape(-1)) * nrm - 1.0).max()
    print('ties: | |fbb| |a| - 1 | max %.3g' % err)
    assert err <= TOL


def test_a_column_in_the_span_of_the_earlier_ones_stops_the_item(pkg):
    """Two identical columns, white items, ntrf = 2: step 1 can only choose a column that step 0 spans (pivot <= 1e-6 of the
    column's norm), so the item stops with one atom and gives the bits of a call with ntrf = 1."""
    h, At = R.span_stop_inputs()
    nt, nr = At.shape[0], h.shape[1]
    e = engine(pkg, nt, nr, At)
    w2 = e.hybrid_weights(h, ns=1, ntrf=2)
    w1 = e.hybrid_weights(h, ns=1, ntrf=1)
    assert (w2.n_atoms == 1).all(), np.unique(w2.n_atoms)
    assert (w2.idx[..., 0] == 0).all() and (w2.idx[..., 1] == -1).all()
    assert (w2.fbb[..., 1] == 0).all()
    assert same_bits(w2.fbb[..., 0], w1.fbb[..., 0]) and same_bits(w2.gain, w1.gain)
    assert (w1.idx == 0).all() and (w1.n_atoms == 1).all()
    assert same_bits(w2.frf_mean[:, 0], w1.frf_mean[:, 0]) and (w2.frf_mean[:, 1] == 0).all()
    assert np.isfinite(w2.gain).all() and (w2.gain > 0).all()


# ------------------------------------------------------------------------------------------------ 5. range
_RANGE = {}


def _range_case(pkg, oracle, npkt):
    """the (32, 4, 2, 4, 500 rays, 0 dB) inputs of the replay, their dictionary and an engine"""
    if npkt not in _RANGE:
        At = dictionary(pkg, 32, 500)
        _RANGE[npkt] = (R.ls_csi(oracle, 32, 4, 0, npkt), At, engine(pkg, 32, 4, At))
    return _RANGE[npkt]


@pytest.mark.parametrize('power', [40, -40])
def test_a_power_of_two_scales_nothing_but_the_gain(pkg, oracle, power):
    """h times 2^+-40 (exact in fp32): every quantity of the fp64 Jacobi scales by an exact power of two, its skip threshold is
    relative and Fopt is scale-free, so idx, n_atoms, fbb and frf_mean keep their bits and the gain is the unscaled one times
    2^+-80, exactly."""
    h, At, e = _range_case(pkg, oracle, 2)
    ns, ntrf = 2, 4
    scaled = (h * np.float32(2.0 ** power)).astype(np.complex64)
    assert np.array_equal(scaled.real * np.float32(2.0 ** -power), h.real) and np.isfinite(scaled).all()
    a = e.hybrid_weights(h, ns=ns, ntrf=ntrf)
    b = e.hybrid_weights(scaled, ns=ns, ntrf=ntrf)
    for name in ('idx', 'n_atoms', 'fbb', 'frf_mean'):
        diff = np.flatnonzero(_bits(getattr(a, name)) != _bits(getattr(b, name)))
        assert diff.size == 0, ('2^%d' % power, name, 'differs at flat positions', diff[:8])
    want = a.gain * np.float32(2.0 ** (2 * power))
    assert np.isfinite(want).all() and (want > 0).all()
    diff = np.flatnonzero(_bits(b.gain).reshape(-1) != _bits(want).reshape(-1))
    assert diff.size == 0, ('2^%d' % power, 'gain differs at items', diff[:8], b.gain.reshape(-1)[diff[:8]], want.reshape(-1)[diff[:8]])


def test_all_zero_items(pkg, oracle):
    """One all-zero item in the middle of a packet and one whole packet of zeros.  The rule (include/csi_mamimo.h): Fopt = 0, every
    metric is 0, the first step takes column 0 with zero coefficients and stops: n_atoms 1, idx (0, -1, ..), fbb 0, gain 0.  All the
    other items keep the bits of the same call with ones in place of the zeros."""
    h, At, e = _range_case(pkg, oracle, 3)
    ns, ntrf = 2, 4
    hz, zero = R.with_zero_items(h)
    ho, _ = R.with_zero_items(h, fill=1.0)
    assert zero.sum() == N + 1 and not R.csi_to_items(hz)[zero].any() and R.csi_to_items(hz)[~zero].all(axis=(1, 2)).all()
    w = e.hybrid_weights(hz, ns=ns, ntrf=ntrf)
    wo = e.hybrid_weights(ho, ns=ns, ntrf=ntrf)
    for name, x in zip(w._fields, w):
        assert np.isfinite(x).all(), name
    slots_are_consistent('zero items', w, At.shape[1])
    n = 3 * N
    fbb, idx, na, gain = w.fbb.reshape(n, ns, ntrf), w.idx.reshape(n, ntrf), w.n_atoms.reshape(n), w.gain.reshape(n)
    assert (fbb[zero] == 0).all() and (gain[zero] == 0).all()
    assert (na[zero] == 1).all() and (idx[zero, 0] == 0).all() and (idx[zero, 1:] == -1).all(), 'the rule of the header'
    for name in ('fbb', 'idx', 'n_atoms', 'gain'):
        x, y = getattr(w, name).reshape(n, -1), getattr(wo, name).reshape(n, -1)
        assert same_bits(x[~zero], y[~zero]), name + ': a zero item changed its neighbours'
    # frf_mean is per packet: packet 2 holds no zero item
    assert same_bits(w.frf_mean[2], wo.frf_mean[2])
    frf = pkg.frf_from_idx(At.astype(np.complex128), w.idx)
    assert np.abs(w.frf_mean - frf.mean(axis=1)).max() <= 1e-6
