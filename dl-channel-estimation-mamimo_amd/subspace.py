"""Delay-subspace bases for the smoother csi_subspace_smooth[_device] (include/csi_mamimo.h): the LS row of a link is
fitted with a channel of at most L delay taps and the fit evaluated on the 234 data carriers, y = Q diag(w) Q^H x.  The module
builds Q and the eigenvalues in numpy fp64; the products run on the device (CsiEngine.subspace_set_basis / subspace_smooth)."""
import numpy as np

N_FFT = 256
NULL_BINS = tuple(range(1, 8)) + (129,) + tuple(range(251, 257))      # 1-based shifted bins, generate_maMIMO_LTF.m:72-78
PILOT_BINS = (26, 54, 90, 118, 140, 168, 204, 232)
MAX_RANK = 128


def data_carrier_offsets():
    """f_k = ind_k - 129 of the 234 data carriers (ind: the 1-based shifted bins 1 .. 256 without nulls and pilots), int64 [234] in
    -128 .. 127, ascending: the order of the last axis of every CSI plane."""
    drop = set(NULL_BINS) | set(PILOT_BINS)
    ind = np.array([b for b in range(1, N_FFT + 1) if b not in drop], np.int64)
    assert ind.size == 234
    return ind - 129


def delay_basis(n_taps, pre=0, tol=1e-10):
    """Orthonormal basis of the channels with taps at delays -pre .. n_taps - pre - 1, seen on the data carriers.
    F[k][l] = exp(-2 pi i f_k (l - pre) / 256), l < n_taps; thin SVD F = U S V^H; r = number of s_j > tol s_0.
    Returns (Q complex128 [234, r] = U[:, :r], lam float64 [r] = s_j^2 / n_taps): Q diag(lam) Q^H = F F^H / n_taps, the frequency
    correlation of a uniform delay profile over the window.  The sign is that of synth.structured_packets,
    H[b] = sum_l c_l exp(-2 pi i b l / 256)."""
    n_taps, pre = int(n_taps), int(pre)
    if not 1 <= n_taps <= MAX_RANK:
        raise ValueError('n_taps %d outside 1 .. %d' % (n_taps, MAX_RANK))
    if not 0 <= pre <= n_taps:
        raise ValueError('pre %d outside 0 .. n_taps = %d' % (pre, n_taps))
    f = data_carrier_offsets().astype(np.float64)
    delays = np.arange(n_taps, dtype=np.float64) - pre
    F = np.exp(-2j * np.pi * np.outer(f, delays) / N_FFT)
    u, s, _ = np.linalg.svd(F, full_matrices=False)
    r = int(np.count_nonzero(s > tol * s[0]))
    return np.ascontiguousarray(u[:, :r]), s[:r] ** 2 / n_taps


def robust_weights(lam, nu):
    """lam / (lam + nu): with these weights Q diag(w) Q^H is R (R + nu I)^-1 for R = Q diag(lam) Q^H, the LMMSE smoother for a uniform
    delay profile at the noise-to-signal ratio nu.  nu may be a scalar or broadcast against lam (for instance [npkt, nr, 1])."""
    lam = np.asarray(lam, np.float64)
    return lam / (lam + np.asarray(nu, np.float64))
