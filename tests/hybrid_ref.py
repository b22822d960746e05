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
    psi = np.einsum('jk,ijs->iks', np.conj(At), res)
    return (np.abs(psi) ** 2).sum(-1)


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
