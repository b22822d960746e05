"""Reference of the delay-subspace smoother (csi_subspace_smooth[_device]; test helper, no test collects from here): the two-stage map
y = Q diag(w) Q^H x of include/csi_mamimo.h in numpy - in complex128 as the truth, and in complex64 as the yardstick an fp32
implementation that sums in another order is measured against."""
import numpy as np

N = 234


def smooth(x, Q, w=None, dtype=np.complex128):
    """x complex [npkt, nr, nt, 234], Q complex [234, r], w real [npkt, nr, r] or None.  Every array is cast to `dtype` (w to its real
    type) first and both products run in it:  t_j = sum_k conj(Q[k][j]) x_k,  y_k = sum_j Q[k][j] w_j t_j."""
    dtype = np.dtype(dtype)
    x = np.asarray(x).astype(dtype)
    Q = np.asarray(Q).astype(dtype)
    t = x @ Q.conj()
    if w is not None:
        t = t * np.asarray(w).astype(dtype.type(0).real.dtype)[:, :, None, :]
    y = t @ Q.T
    assert y.dtype == dtype
    return y


def row_err(y, ref, x):
    """|y - ref|_2 / |x_row|_2 per row, float64 [rows]"""
    d = np.asarray(y, np.complex128).reshape(-1, N) - np.asarray(ref, np.complex128).reshape(-1, N)
    return np.linalg.norm(d, axis=1) / np.linalg.norm(np.asarray(x, np.complex128).reshape(-1, N), axis=1)


def random_basis(rng, rank):
    """complex128 [234, rank] with orthonormal columns and no delay structure"""
    a = rng.standard_normal((N, rank)) + 1j * rng.standard_normal((N, rank))
    q, _ = np.linalg.qr(a)
    return q


def nmse(est, ref):
    """mean over links of |ref - est|^2 / |ref|^2 (NMSE_subk)"""
    est, ref = np.asarray(est, np.complex128).reshape(-1, N), np.asarray(ref, np.complex128).reshape(-1, N)
    return float(np.mean(np.sum(np.abs(ref - est) ** 2, axis=1) / np.sum(np.abs(ref) ** 2, axis=1)))
