"""fp64 restatement of the LMMSE smoother (LMMSE_ce.m:23-39 with Nfft = Np = 234, Nps = 1, called per link from
helperMIMOChannelEstimate.m:37-39) for the tests of csi_lmmse_estimate: plain numpy, one solve per (packet, rx) for all tx columns.

    tau_rms = sqrt(r2 - r^2),  r = sum |h_k|^2 k / sum |h_k|^2,  r2 = sum |h_k|^2 k^2 / sum |h_k|^2        (:27-30)
    R[a][b] = 1 / (1 + j 2 pi tau_rms (a - b) / 234)                                                       (:31-36)
    H_mmse  = R (R + s I)^-1 H_ls = H_ls - s (R + s I)^-1 H_ls,   s = 10^(-snr_db / 10)                    (:23, :38-39)

`oracle.lmmse_estimate` forms inv(R + s I) once per link as :39 does (about 9 ms per link); this solves instead
(`np.linalg.solve`, complex128), which is what the product with the inverse stands for, and costs about 4 ms per (packet, rx).

Two places where this is not the literal formula, both where the formula leaves the reals:
  * an all-zero h (hh == 0) divides 0 by 0 in :28-29 and the reference returns NaN; here, and in the kernel, it means no delay
    spread: tau_rms = 0;
  * r2 - r^2 is clamped at 0 before the root, as in the kernel: it is negative only by rounding (a one-tap h), where the
    reference would carry an imaginary tau_rms of rounding size.

`levinson` is the kernel's own recursion (csrc/lmmse.hip.h) in numpy, with its normalisation, for the CPU test of the algorithm."""
import numpy as np

N = 234


def tau_rms(hvec):
    """hvec real [L] -> the rms "delay" of LMMSE_ce.m:27-30 (float)"""
    h = np.asarray(hvec, np.float64).reshape(-1)
    k = np.arange(h.size, dtype=np.float64)
    hh = float(h @ h)
    if hh == 0.0:
        return 0.0
    tmp = h * h * k
    r = tmp.sum() / hh
    r2 = (tmp @ k) / hh
    return float(np.sqrt(max(r2 - r * r, 0.0)))


def correlation(tau, n=N):
    """R [n][n] complex128"""
    d = np.arange(n)[:, None] - np.arange(n)[None, :]
    return 1.0 / (1.0 + 2j * np.pi * tau * d / n)


def lmmse_ref(h_ls, hvec, snr_db):
    """h_ls complex [npkt][nr][nt][234], hvec [npkt][L], snr_db [npkt][nr] -> complex128 like h_ls"""
    h_ls = np.asarray(h_ls).astype(np.complex128)
    hvec, snr_db = np.asarray(hvec, np.float64), np.asarray(snr_db, np.float64)
    npkt, nr, nt, n = h_ls.shape
    assert n == N and hvec.shape[0] == npkt and snr_db.shape == (npkt, nr)
    out = np.empty_like(h_ls)
    for p in range(npkt):
        R = correlation(tau_rms(hvec[p]))
        for i in range(nr):
            s = 10.0 ** (-0.1 * snr_db[p, i])
            H = h_ls[p, i].T                                         # [234][nt]
            out[p, i] = (H - s * np.linalg.solve(R + s * np.eye(N), H)).T
    return out


def levinson(H, tau, snr_db):
    """The kernel's recursion for one (packet, rx): H complex128 [234][nt] -> H_mmse [234][nt].
    Normalised system M z = H with M = (R + s I) / (1 + s): first column t[0] = 1, t[d] = 1 / ((1 + j c d)(1 + s)), c = 2 pi tau / 234;
    forward vector f and solution z grown one row at a time; H_mmse = H - s / (1 + s) z."""
    H = np.asarray(H, np.complex128)
    n = H.shape[0]
    s = 10.0 ** (-0.1 * float(snr_db))
    c = 2.0 * np.pi * tau / n
    d = np.arange(n, dtype=np.float64)
    t = 1.0 / ((1.0 + 1j * c * d) * (1.0 + s))
    t[0] = 1.0
    f = np.array([1.0 + 0j])
    x = np.zeros_like(H)
    x[0] = H[0]
    for k in range(1, n):
        tk = t[k:0:-1]                                               # t[k - i], i = 0 .. k-1
        ef = tk @ f
        ex = tk @ x[:k]
        fn = (np.append(f, 0.0) - ef * np.append(0.0, np.conj(f[::-1]))) / (1.0 - abs(ef) ** 2)
        x[:k + 1] += np.conj(fn[::-1])[:, None] * (H[k] - ex)[None, :]
        f = fn
    return H - (s / (1.0 + s)) * x


def rel_rows_c(y, ref):
    """norm-relative error per row (last axis) of complex arrays -> array of the leading shape"""
    y, ref = np.asarray(y).astype(np.complex128), np.asarray(ref).astype(np.complex128)
    return np.linalg.norm(y - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


def profiles(tap_profile8):
    """The hvec rows of the regime grid, by name (float32, of differing lengths)"""
    one5 = np.zeros(16, np.float32)
    one5[5] = 1.0
    far = np.zeros(200, np.float32)
    far[0] = far[199] = 1.0
    return {'sweep': np.asarray(tap_profile8, np.float32),
            'one_tap_L1': np.array([0.75], np.float32),
            'one_tap_in_L16': one5,
            'two_far_L200': far,
            'flat_L100': np.ones(100, np.float32),
            'two_near': np.array([1.0, 1e-3], np.float32)}


def pad(rows, L=None):
    """rows of differing lengths -> [len(rows)][L] float32, zero-padded at the end (zeros add nothing to the three sums)"""
    L = L or max(r.size for r in rows)
    out = np.zeros((len(rows), L), np.float32)
    for i, r in enumerate(rows):
        out[i, :r.size] = r
    return out


SNR_GRID = (-25.0, 10.0, 25.0, 40.0, 60.0)
