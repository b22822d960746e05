"""fp64 restatement of the blind LMMSE smoother (csi_lmmse_blind, csrc/lmmse.hip.h, include/csi_mamimo.h) for its tests: plain
numpy in complex128, no test collects from here.  Per (packet, rx), contiguous-index convention (Nfft = Np = 234, Nps = 1):

    nv     = sum_{s, b} |Y[s][b]|^2 / (14 Nt),  Y[s][b] = sum_{n < 256} x[320 s + 64 + n] exp(-2 pi i b n / 256),  b in NULL_BINS
             (evaluated exactly on the fp32 samples, see noise_var: on noise-free packets the sums cancel to rounding residue)
    c[d]   = 1 / (234 Nt) sum_j sum_{k < 234 - d} h[j][k + d] conj(h[j][k])            (biased: Toeplitz(c) is positive definite)
    out[j] = h[j] - (nv / Nt) T^-1 h[j],  T = Toeplitz(c)                                (T estimates R_h + (nv / Nt) I as it stands)

`blind_ref` solves with np.linalg.solve on the explicit 234 x 234 matrix.  `levinson_blind` is the kernel's recursion restated
(normalised by c[0], gain (nv / Nt) / c[0]) with its two guards: c[0] == 0 hands the rows back, and so does a step whose
1 - |ef|^2 is not positive or not finite - which then counts as a fallback."""
import numpy as np

N = 234
NULL_BINS = np.array([0] + list(range(122, 135)))          # FFT bins of the 1-based shifted null carriers [1:7 129 251:256]


def twiddles_exact():
    """exp(-2 pi i u / 256), u = 0 .. 255, to 60 decimal digits: (cos, -sin) as lists of Decimal.  Half-angle steps from cos(pi / 2) = 0
    down to pi / 128, then 255 rotations - no library's cos is trusted."""
    from decimal import Decimal, getcontext
    getcontext().prec = 70
    c, s = Decimal(0), Decimal(1)                                        # angle pi / 2
    for _ in range(6):
        c, s = ((1 + c) / 2).sqrt(), ((1 - c) / 2).sqrt()                # angle halved: pi / 128 after six steps
    wr, wi = [Decimal(1)], [Decimal(0)]
    for _ in range(255):
        wr, wi = wr + [wr[-1] * c - wi[-1] * s], wi + [wr[-1] * s + wi[-1] * c]
    wr[64], wr[192], wi[128], wi[0] = Decimal(0), Decimal(0), Decimal(0), Decimal(0)
    return wr, [-v for v in wi]


def _split3(vals):
    """Decimal values -> three float64 arrays whose exact sum is the value to 2^-100: two parts of 24 significant bits (a product
    with an fp32 sample is exact in fp64) and the rest"""
    from decimal import Decimal
    a = [float(np.float32(float(v))) for v in vals]
    r = [v - Decimal(x) for v, x in zip(vals, a)]
    b = [float(np.float32(float(v))) for v in r]
    c = [float(v - Decimal(x)) for v, x in zip(r, b)]
    return np.array([a, b, c])


_TW3 = None


def noise_var(ltf, nt, exact=True):
    """ltf complex64 [npkt][nr][>= 320 nt] -> nv float64 [npkt][nr].

    exact=True evaluates every Y[s][b] without rounding until the end: twiddles to 2^-100 in three parts, products of an fp32 sample
    with a 24-bit part are exact in fp64, and math.fsum adds the 1536 terms of a component exactly.  That matters on noise-free
    packets, where the null carriers hold only rounding residue and the 256 terms cancel to 1e-8 of their size: the plain complex128
    form (exact=False) then carries 1e-8 ... 3e-7 of error of its own.  exact=False is for inputs too large for a Python loop and
    well above that floor (its own error: 256 roundings of 1e-16 |x| against |Y|)."""
    import math
    global _TW3
    ltf = np.asarray(ltf)
    npkt, nr = ltf.shape[:2]
    x = ltf[..., :320 * nt].reshape(npkt, nr, nt, 320)[..., 64:]
    if not exact:
        x = x.astype(np.complex128)
        w = np.exp(-2j * np.pi * np.outer(NULL_BINS, np.arange(256)) / 256.0)      # [14][256]
        y = x @ w.T
        return (np.abs(y) ** 2).sum(axis=(2, 3)) / (NULL_BINS.size * nt)
    assert ltf.dtype == np.complex64, 'the exact form needs fp32 samples'
    if _TW3 is None:
        wr, wi = twiddles_exact()
        idx = np.outer(NULL_BINS, np.arange(256)) % 256
        _TW3 = (_split3(wr)[:, idx], _split3(wi)[:, idx])                # [3][14][256] each
    wr, wi = _TW3
    xr, xi = x.real.astype(np.float64), x.imag.astype(np.float64)       # [npkt][nr][nt][256]
    nv = np.zeros((npkt, nr))
    for p in range(npkt):
        for r in range(nr):
            a, b = xr[p, r][:, None, None, :], xi[p, r][:, None, None, :]           # [nt][1][1][256] against [3][14][256]
            t_re = np.concatenate([a * wr[None], -(b * wi[None])], axis=1)          # [nt][6][14][256]
            t_im = np.concatenate([a * wi[None], b * wr[None]], axis=1)
            tot = 0.0
            for t in (t_re, t_im):
                rows = np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(nt * NULL_BINS.size, -1)
                y = np.array([math.fsum(row) for row in rows.tolist()])
                tot += math.fsum((y * y).tolist())
            nv[p, r] = tot / (NULL_BINS.size * nt)
    return nv


def freq_corr(h_ls):
    """h_ls complex [..., nt, 234] -> c complex128 [..., 234]"""
    h = np.asarray(h_ls).astype(np.complex128)
    nt = h.shape[-2]
    c = np.empty(h.shape[:-2] + (N,), np.complex128)
    with np.errstate(invalid='ignore'):                                  # a non-finite input is carried, not screened
        for d in range(N):
            c[..., d] = (h[..., d:] * np.conj(h[..., :N - d])).sum(axis=(-2, -1))
        return c / (N * nt)


def toeplitz(c):
    """T[a][b] = c[a - b] for a >= b, conj(c[b - a]) above the diagonal"""
    c = np.asarray(c, np.complex128)
    d = np.arange(N)[:, None] - np.arange(N)[None, :]
    return np.where(d >= 0, c[np.abs(d)], np.conj(c[np.abs(d)]))


def smooth_solve(H, c, nv, nt):
    """one (packet, rx): H complex128 [234][nt] -> out [234][nt] by np.linalg.solve; all-zero rows come back as they are"""
    if c[0].real == 0.0:
        return H.copy()
    return H - (nv / nt) * np.linalg.solve(toeplitz(c), H)


def blind_ref(ltf, h_ls, exact=True):
    """ltf complex64 [npkt][nr][len_ltf], h_ls complex [npkt][nr][nt][234] -> (out complex128 like h_ls, nv [npkt][nr], c [npkt][nr][234]);
    `exact` as in noise_var"""
    h = np.asarray(h_ls).astype(np.complex128)
    npkt, nr, nt, n = h.shape
    assert n == N
    nv, c = noise_var(ltf, nt, exact), freq_corr(h)
    out = np.empty_like(h)
    for p in range(npkt):
        for i in range(nr):
            out[p, i] = smooth_solve(h[p, i].T, c[p, i], nv[p, i], nt).T
    return out, nv, c


def levinson_blind(H, c, nv, nt):
    """The kernel's recursion for one (packet, rx): H complex128 [234][nt] -> (out [234][nt], fell_back).  Normalised system M z = H with
    M = T / c[0]: first column t[d] = c[d] / c[0], t[0] = 1; out = H - (nv / Nt) / c[0] z."""
    H = np.asarray(H, np.complex128)
    c = np.asarray(c, np.complex128)
    c0 = c[0].real
    if c0 == 0.0:
        return H.copy(), False
    with np.errstate(all='ignore'):
        t = c / c0
        t[0] = 1.0
        f = np.array([1.0 + 0j])
        x = np.zeros_like(H)
        x[0] = H[0]
        for k in range(1, N):
            tk = t[k:0:-1]                                               # t[k - i], i = 0 .. k-1
            ef = tk @ f
            ex = tk @ x[:k]
            den = 1.0 - (ef.real * ef.real + ef.imag * ef.imag)
            if not (den > 0.0 and den <= 1.0):
                return H.copy(), True
            fn = (np.append(f, 0.0) - ef * np.append(0.0, np.conj(f[::-1]))) / den
            x[:k + 1] += np.conj(fn[::-1])[:, None] * (H[k] - ex)[None, :]
            f = fn
        return H - (nv / nt / c0) * x, False


def rel_rows_c(y, ref):
    """norm-relative error per row (last axis) of complex arrays -> array of the leading shape"""
    y, ref = np.asarray(y).astype(np.complex128), np.asarray(ref).astype(np.complex128)
    return np.linalg.norm(y - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


def nmse(est, ref):
    """NMSE_subk: per-link ||ref - est||^2 / ||ref||^2, mean over the links"""
    est, ref = np.asarray(est).astype(np.complex128), np.asarray(ref).astype(np.complex128)
    return float(np.mean(np.sum(np.abs(ref - est) ** 2, -1) / np.sum(np.abs(ref) ** 2, -1)))


def break_input(h_ls, p=0, r=0):
    """a copy of the LS tensor whose (packet p, rx r) breaks the recursion: one +Inf sample makes c[0] infinite and t[] NaN, so the
    first step's 1 - |ef|^2 is not finite (Toeplitz(c) is positive definite for every finite non-zero input; only a non-finite one
    gets there)"""
    h = np.array(h_ls, np.complex64)
    h[p, r, 0, 5] = np.complex64(complex(np.inf, 0.0))
    return h
