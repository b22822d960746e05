"""fp64 restatement of the hybrid beamforming weights (SVD + orthogonal matching pursuit) for the tests of
csi_hybrid_weights: plain numpy, batched over items (one item = one packet and subcarrier).

    Fopt = right singular vectors of H (Nr x Nt) for the Ns largest singular values
    for m = 1 .. NtRF:  k_m = argmax_k sum_s |At[:,k]^H Res[:,s]|^2 (lowest k on a tie),
                        C = (A^H A)^-1 A^H Fopt,  T = Fopt - A C,  e = |T|_F,  Res = T / e,  stop when e <= stop_tol
    Fbb = sqrt(Ns) C / |A C|_F,   fbb = Fbb^T [Ns][NtRF],   frf = At[:, idx]^T [NtRF][Nt]

The dictionary of the reference is full of near-duplicate columns, so two correct runs in different precisions may
choose different indices; `replay` therefore follows a given index sequence (the GPU's) and reports, per step, how far
the given choice falls short of the best metric, and the fp64 coefficients for the given index set."""
import numpy as np


def csi_to_items(h):
    """[npkt][nr][nt][234] -> [npkt * 234][nr][nt] (complex128)"""
    h = np.asarray(h)
    npkt, nr, nt, nk = h.shape
    return np.ascontiguousarray(h.transpose(0, 3, 1, 2)).reshape(npkt * nk, nr, nt).astype(np.complex128)


def fopt_of(H, ns):
    """H [items][nr][nt] -> Fopt [items][nt][ns], singular values [items][min(nr, nt)]"""
    _, sv, vh = np.linalg.svd(H, full_matrices=False)
    return np.conj(vh[:, :ns, :]).transpose(0, 2, 1), sv


def gap_at_cut(sv, ns):
    """relative singular-value gap at the cut, (sigma_ns - sigma_ns+1) / sigma_1; 1 where ns takes them all"""
    if ns >= sv.shape[1]:
        return np.ones(sv.shape[0])
    return (sv[:, ns - 1] - sv[:, ns]) / sv[:, 0]


def metric(At, res):
    """sum_s |At[:,k]^H Res[:,s]|^2 -> [items][rays]"""
    n, nt, ns = res.shape
    psi = np.conj(At).T @ res.transpose(1, 0, 2).reshape(nt, n * ns)          # one product [rays][nt] x [nt][items * ns]
    return (np.abs(psi.reshape(At.shape[1], n, ns)) ** 2).sum(-1).T


def _coeffs(At, idx_m, fopt):
    """C = (A^H A)^-1 A^H Fopt for A = At[:, idx_m]; idx_m [items][m] -> A [items][nt][m], C [items][m][ns]"""
    A = At.T[idx_m].transpose(0, 2, 1)
    Ah = np.conj(A).transpose(0, 2, 1)
    return A, np.linalg.solve(Ah @ A, Ah @ fopt)


def omp(H, At, ns, ntrf, stop_tol=1e-5):
    """The whole definition in fp64 with its own choices.  Returns fbb [items][ns][ntrf], idx [items][ntrf] (-1 behind
    an early stop), n_atoms [items]."""
    At = np.asarray(At, np.complex128)
    fopt, _ = fopt_of(np.asarray(H, np.complex128), ns)
    n = fopt.shape[0]
    idx = np.full((n, ntrf), -1, np.int64)
    coef = np.zeros((n, ntrf, ns), np.complex128)
    n_atoms = np.zeros(n, np.int64)
    live = np.arange(n)
    res = fopt.copy()
    for m in range(ntrf):
        if live.size == 0:
            break
        idx[live, m] = np.argmax(metric(At, res[live]), axis=1)
        A, C = _coeffs(At, idx[live, :m + 1], fopt[live])
        T = fopt[live] - A @ C
        e = np.sqrt((np.abs(T) ** 2).sum((1, 2)))
        coef[live, :m + 1] = C
        n_atoms[live] = m + 1
        go = e > stop_tol
        res[live[go]] = T[go] / e[go, None, None]
        live = live[go]
    return _normalise(At, idx, coef, ns), idx, n_atoms


def _normalise(At, idx, coef, ns):
    A = np.where(idx[:, None, :] >= 0, At.T[np.maximum(idx, 0)].transpose(0, 2, 1), 0.0)
    nrm = np.sqrt((np.abs(A @ coef) ** 2).sum((1, 2)))
    fbb = np.sqrt(ns) * coef / nrm[:, None, None]
    return fbb.transpose(0, 2, 1)


def replay(H, At, ns, idx):
    """Follow the index sequence idx [items][ntrf] (all >= 0) in fp64.  Returns
    shortfall [items][ntrf] = 1 - metric[idx] / max(metric) at every step, computed with the given earlier choices, and
    fbb [items][ns][ntrf] = the normalised fp64 coefficients for the given index set."""
    At = np.asarray(At, np.complex128)
    idx = np.asarray(idx, np.int64)
    fopt, _ = fopt_of(np.asarray(H, np.complex128), ns)
    n, ntrf = idx.shape
    short = np.zeros((n, ntrf))
    coef = np.zeros((n, ntrf, ns), np.complex128)
    res = fopt.copy()
    rows = np.arange(n)
    for m in range(ntrf):
        met = metric(At, res)
        short[:, m] = 1.0 - met[rows, idx[:, m]] / met.max(axis=1)
        A, C = _coeffs(At, idx[:, :m + 1], fopt)
        T = fopt - A @ C
        e = np.sqrt((np.abs(T) ** 2).sum((1, 2)))
        res = T / e[:, None, None]
        coef[:, :m + 1] = C
    return short, _normalise(At, idx, coef, ns)


def frf_from_idx(At, idx):
    """frf [items][ntrf][nt] = At[:, idx]^T, zero rows where idx is -1"""
    At = np.asarray(At)
    idx = np.asarray(idx, np.int64)
    return np.where(idx[..., None] >= 0, At.T[np.maximum(idx, 0)], 0.0)


def weights_matrix(At, idx, fbb):
    """T = frf^T fbb^T [items][nt][ns]"""
    frf = frf_from_idx(np.asarray(At, np.complex128), idx)
    return frf.transpose(0, 2, 1) @ np.asarray(fbb, np.complex128).transpose(0, 2, 1)


def gain(H_eval, T):
    """|H_eval T|_F^2 per item"""
    return (np.abs(np.asarray(H_eval, np.complex128) @ T) ** 2).sum((1, 2))


def projector_error(T, T_ref):
    """|T T^H - T_ref T_ref^H|_F / |T_ref T_ref^H|_F per item"""
    P = T @ np.conj(T).transpose(0, 2, 1)
    Pr = T_ref @ np.conj(T_ref).transpose(0, 2, 1)
    return np.sqrt((np.abs(P - Pr) ** 2).sum((1, 2)) / (np.abs(Pr) ** 2).sum((1, 2)))


# ---------------------------------------------------------------------------------------------- inputs of the regime tests
# Everything below builds inputs (and states what the kernels' layout makes of them); tests/test_hybrid_host.py checks the designs
# with the fp64 definition above, so the GPU tests can assert exact indices and counts.
N = 234
DEFAULT_STOP_TOL = 1e-5
RAY_TILE = 32               # hyb_corr_kernel: rays per pass of the dictionary through LDS

# rows of the replay grid beyond powers of two, (Nt, Nr, Ns, NtRF, rays, SNR dB, packets): Nr = 1 (no Jacobi pair); odd Nr with fewer
# rays than a tile and one ray past a tile; singular-vector workgroups of 56, 41 and 14 lanes (Nr = 6, 7, 12); Nt no power of two and
# above 128; Nt and rays at their caps (64 KiB of LDS for the dictionary tile); NtRF at its cap with Ns = Nr
NEW_SHAPES = [(8, 1, 1, 1, 64, 10, 2), (8, 3, 2, 2, 31, 0, 2), (12, 5, 2, 3, 33, 0, 2), (16, 6, 3, 4, 100, 0, 2), (16, 7, 4, 4, 100, -10, 2),
              (36, 12, 4, 6, 200, 0, 1), (100, 4, 2, 4, 500, 0, 1), (132, 2, 1, 2, 64, 10, 1), (256, 4, 2, 4, 4096, 0, 1),
              (16, 4, 4, 16, 333, 0, 1)]
# the pursuit over a whole unitary dictionary: (Nt, Nr, Ns) with NtRF = rays = Nt
FULL_SPAN_CASES = [(nt, nr, ns) for nt in (8, 12, 16) for nr, ns in ((1, 1), (3, 2), (5, 3), (7, 4), (12, 4)) if nr <= nt]
FULL_SPAN_SNR, FULL_SPAN_PACKETS = 0, 2


def svd_lanes(nr):
    """workgroup width of hyb_svd_kernel: 32 nr^2 bytes of LDS per lane against 64 KiB, 64 lanes at the most"""
    return max(1, min(64, 65536 // (32 * nr * nr)))


def pm1_pilot(nt, seed=29):
    """A seeded non-singular +-1 pilot matrix for the Nt at which there is no Sylvester-Hadamard matrix"""
    rng = np.random.default_rng(seed)
    while True:
        P = rng.integers(0, 2, (nt, nt)) * 2.0 - 1.0
        if np.linalg.matrix_rank(P) == nt:
            return P


def ls_csi(oracle, nt, nr, snr, npkt, seed=11, block=250):
    """fp64 LS estimates of make_structured_packets(default_rng(seed), ...), rounded to the complex64 the library receives.  The pilot
    is the Hadamard matrix where Nt is a power of two and pm1_pilot(Nt) elsewhere (the oracle's LS takes any P)."""
    rng = np.random.default_rng(seed)
    P = oracle.hadamard(nt) if nt & (nt - 1) == 0 else pm1_pilot(nt)
    out = []
    for p0 in range(0, npkt, block):
        ltf, _ = oracle.make_structured_packets(rng, min(block, npkt - p0), nr, P, snr_db=snr)
        out.append(oracle.ls_estimate(ltf, P).astype(np.complex64))
    return np.concatenate(out)


def dft_dictionary(nt):
    """the unitary DFT matrix of order nt as the complex64 the library receives"""
    j = np.arange(nt)
    return (np.exp(2j * np.pi * np.outer(j, j) / nt) / np.sqrt(nt)).astype(np.complex64)


def left_out_share(H, ns, gap_min):
    """share of the items whose singular-value gap at the cut is under gap_min, and the smallest gap"""
    _, sv = fopt_of(np.asarray(H, np.complex128), ns)
    g = gap_at_cut(sv, ns)
    return float((g < gap_min).mean()), float(g.min())


def omp_margins(H, At, ns, ntrf, stop_tol=DEFAULT_STOP_TOL):
    """omp, with two more results per item: the smallest 1 - second / best metric over its steps (how far every choice is from a
    tie) and the residual e after each step [items][ntrf] (nan behind the stop)"""
    At = np.asarray(At, np.complex128)
    fopt, _ = fopt_of(np.asarray(H, np.complex128), ns)
    n = fopt.shape[0]
    idx = np.full((n, ntrf), -1, np.int64)
    margin = np.ones(n)
    resid = np.full((n, ntrf), np.nan)
    live = np.arange(n)
    res = fopt.copy()
    for m in range(ntrf):
        if live.size == 0:
            break
        met = metric(At, res[live])
        idx[live, m] = np.argmax(met, axis=1)
        if met.shape[1] > 1:
            top = np.sort(met, axis=1)
            margin[live] = np.minimum(margin[live], 1.0 - top[:, -2] / top[:, -1])
        A, C = _coeffs(At, idx[live, :m + 1], fopt[live])
        T = fopt[live] - A @ C
        e = np.sqrt((np.abs(T) ** 2).sum((1, 2)))
        resid[live, m] = e
        go = e > stop_tol
        res[live[go]] = T[go] / e[go, None, None]
        live = live[go]
    return idx, margin, resid


# ---- mixed stopping: neighbouring items of one wave finish at different steps
MIXED_NT, MIXED_NR, MIXED_NTRF, MIXED_PACKETS = 32, 4, 4, 2
MIXED_MAGS = (1.0, 0.6, 0.35)
# stop_tol -> atoms of the items built from 1, 2, 3 dictionary columns and of the white items (None: the default)
MIXED_STOP_TABLE = {None: (1, 2, 3, 4), 0.4: (1, 2, 2, 4), 0.55: (1, 1, 2, 4)}


def mixed_stop_inputs(seed=41):
    """Nt 32, Nr 4, 2 packets over the unitary DFT dictionary.  Subcarrier k is of kind 1 + k % 4.  Kinds 1 - 3 are rank one,
    H = u f^H with f = sum of that many distinct dictionary columns of magnitude 1, 0.6, 0.35 and random phases (Fopt = f / |f|: the
    pursuit takes the columns in that order and fits exactly); kind 4 is white.  The default seed is one at which every choice of the
    fp64 definition is at least 1e-3 from a tie (tests/test_hybrid_host.py), a hundred times the fp32 contract.
    Returns h complex64 [2][4][32][234], At complex64 [32][32], kind [468], cols [468][3] (-1 where unused)."""
    rng = np.random.default_rng(seed)
    nt, nr, npkt = MIXED_NT, MIXED_NR, MIXED_PACKETS
    At = dft_dictionary(nt)
    A = At.astype(np.complex128)
    h = np.zeros((npkt, nr, nt, N), np.complex128)
    kind = np.tile(1 + np.arange(N) % 4, npkt)
    cols = np.full((npkt * N, 3), -1, np.int64)
    for p in range(npkt):
        for k in range(N):
            t = kind[p * N + k]
            if t == 4:
                h[p, :, :, k] = rng.standard_normal((nr, nt)) + 1j * rng.standard_normal((nr, nt))
                continue
            c = rng.choice(nt, t, replace=False)
            f = A[:, c] @ (np.array(MIXED_MAGS[:t]) * np.exp(2j * np.pi * rng.random(t)))
            u = rng.standard_normal(nr) + 1j * rng.standard_normal(nr)
            h[p, :, :, k] = np.outer(u, np.conj(f))
            cols[p * N + k, :t] = c
    return h.astype(np.complex64), At, kind, cols


def mixed_stop_counts(kind, stop_tol):
    """designed n_atoms per item at a stop_tol of MIXED_STOP_TABLE"""
    return np.asarray(MIXED_STOP_TABLE[stop_tol])[np.asarray(kind) - 1]


# ---- ties: equal dictionary columns at the places where the correlation kernel's order decides
TIE_NT, TIE_RAYS, TIE_NR, TIE_PACKETS = 16, 70, 2, 2
TIE_COPIES = ((9, 1), (6, 2), (35, 3), (67, 10))          # (copy, original): column `copy` is overwritten by column `original`


def corr_lane_of(ray):
    """where hyb_corr_kernel holds the metric of a ray: (tile of 32 rays, half wave, accumulator register); a lane scans its
    registers in ascending order, tiles run in ascending order, and the two half waves are merged last"""
    r = ray % RAY_TILE
    return ray // RAY_TILE, (r >> 2) & 1, 4 * (r >> 3) + (r & 3)


def ula_dictionary(nt, rays):
    """half-wavelength uniform linear array at `rays` distinct directions, uniform in sin(azimuth) over +-0.95: complex64 [nt][rays]"""
    s = np.linspace(-0.95, 0.95, rays)
    return np.exp(1j * np.pi * np.outer(np.arange(nt) - (nt - 1) / 2.0, s)).astype(np.complex64)


def tie_inputs(seed=37):
    """Nt 16, 70 rays, the four copies of TIE_COPIES.  Item (p, k) is rank one on the duplicated column of pair k % 4,
    H = u a^H, so the copy and the original have the best metric, bit for bit the same.
    Returns h complex64 [2][2][16][234], At complex64 [16][70], want [468] = the lower index of the item's pair."""
    rng = np.random.default_rng(seed)
    At = ula_dictionary(TIE_NT, TIE_RAYS)
    for copy, orig in TIE_COPIES:
        At[:, copy] = At[:, orig]
    want = np.tile(np.array([min(c) for c in TIE_COPIES])[np.arange(N) % 4], TIE_PACKETS)
    u = rng.standard_normal((TIE_PACKETS, TIE_NR, 1, N)) + 1j * rng.standard_normal((TIE_PACKETS, TIE_NR, 1, N))
    a = np.conj(At.astype(np.complex128)[:, want].reshape(TIE_NT, TIE_PACKETS, N)).transpose(1, 0, 2)          # [p][j][k]
    return (u * a[:, None, :, :]).astype(np.complex64), At, want


def span_stop_inputs(seed=43, nt=16, nr=4, npkt=2):
    """A dictionary of two identical unit-modulus columns under white items: the second step can only choose a column in the span
    of the first.  Returns h complex64 [npkt][nr][nt][234], At complex64 [nt][2]."""
    rng = np.random.default_rng(seed)
    col = np.exp(2j * np.pi * rng.random(nt)).astype(np.complex64)
    h = rng.standard_normal((npkt, nr, nt, N)) + 1j * rng.standard_normal((npkt, nr, nt, N))
    return h.astype(np.complex64), np.stack([col, col], axis=1)


# ---- range
ZERO_ITEM = (0, 117)        # one all-zero (packet, subcarrier) in the middle of packet 0
ZERO_PACKET = 1             # and a whole packet of zeros


def with_zero_items(h, fill=0.0):
    """h [>= 3 packets][nr][nt][234] with the item ZERO_ITEM and the packet ZERO_PACKET set to `fill`; returns the copy and the
    mask [npkt * 234] of those items"""
    out = np.array(h, np.complex64)
    out[ZERO_ITEM[0], :, :, ZERO_ITEM[1]] = fill
    out[ZERO_PACKET] = fill
    mask = np.zeros((out.shape[0], N), bool)
    mask[ZERO_ITEM] = True
    mask[ZERO_PACKET] = True
    return out, mask.reshape(-1)
