"""Reference of the beam-space smoother (csi_beam_*; test helper, no test collects from here): the statement of include/csi_mamimo.h
along the antenna axis in numpy - in complex128 as the truth, and in complex64 as the yardstick an fp32 implementation that sums in
another order is measured against."""
import numpy as np

N = 234


def _cast(x, A, dtype):
    dtype = np.dtype(dtype)
    return np.asarray(x).astype(dtype), np.asarray(A).astype(dtype), dtype.type(0).real.dtype


def beams(x, A, dtype=np.complex128):
    """t[p, r, b, k] = sum_j conj(A[j][b]) x[p, r, j, k]; x complex [npkt, nr, nt, 234], A complex [nt, nb], both cast to `dtype`"""
    x, A, _ = _cast(x, A, dtype)
    t = np.einsum('jb,prjk->prbk', A.conj(), x)
    assert t.dtype == x.dtype
    return t


def power(x, A, dtype=np.complex128):
    """E[p, r, b] = (1 / 234) sum_k |t_b[k]|^2 in the real type of `dtype`"""
    t = beams(x, A, dtype)
    return (t.real ** 2 + t.imag ** 2).sum(axis=-1) / t.real.dtype.type(N)


def smooth(x, A, w=None, dtype=np.complex128):
    """y[p, r, j, k] = sum_b A[j][b] w[p, r, b] t_b[k]; w real [npkt, nr, nb] or None (all ones)"""
    x, A, real = _cast(x, A, dtype)
    t = beams(x, A, dtype)
    if w is not None:
        t = t * np.asarray(w).astype(real)[..., None]
    y = np.einsum('jb,prbk->prjk', A, t)
    assert y.dtype == x.dtype
    return y


def weights(E, v):
    """w = 1 - v / E where E > v, 0 everywhere else (E = 0 included), in the type of E; v [npkt, nr]"""
    E = np.asarray(E)
    v = np.asarray(v).astype(E.dtype)[..., None]
    with np.errstate(divide='ignore', invalid='ignore'):
        w = 1 - v / E
    return np.where(E > v, w, 0).astype(E.dtype)


def wiener(x, A, v, dtype=np.complex128):
    """smooth(x, A, weights(power(x, A), v)), everything in `dtype`; returns (y, w)"""
    w = weights(power(x, A, dtype), v)
    return smooth(x, A, w, dtype), w


def row_err(y, ref, x):
    """|y - ref|_2 / |x_row|_2 per row of 234 carriers, float64 [rows]"""
    d = np.asarray(y, np.complex128).reshape(-1, N) - np.asarray(ref, np.complex128).reshape(-1, N)
    return np.linalg.norm(d, axis=1) / np.linalg.norm(np.asarray(x, np.complex128).reshape(-1, N), axis=1)


def random_basis(rng, nt, nb):
    """complex128 [nt, nb] with orthonormal columns and no array structure"""
    a = rng.standard_normal((nt, nb)) + 1j * rng.standard_normal((nt, nb))
    q, _ = np.linalg.qr(a)
    return q


def nmse(est, ref):
    """mean over links of |ref - est|^2 / |ref|^2 (NMSE_subk)"""
    est, ref = np.asarray(est, np.complex128).reshape(-1, N), np.asarray(ref, np.complex128).reshape(-1, N)
    return float(np.mean(np.sum(np.abs(ref - est) ** 2, axis=1) / np.sum(np.abs(ref) ** 2, axis=1)))
