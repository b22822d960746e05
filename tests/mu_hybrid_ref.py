"""Host restatement of the multi-user hybrid precoder (csrc/mu_hybrid.hip.h), numpy fp64, on top of tests/mu_link_ref.py.
Written from the definition of include/csi_mamimo.h, not from a device run (no test collects from here).

  score     S[m][r] = sum_k | sum_j B_k[m][j] At[j][r] |^2,  B_k[m][j] = hest_u[s][j][k], m = u ns + s
  select    q = 0 .. n_rf-1: stream m = q mod M; idx[q] = argmax over the rays not yet taken of S[m][r], lowest r on a tie, a non-finite
            score compares as -inf;  Frf[:, q] = At[:, idx[q]]
  baseband  per subcarrier: G = B_k Frf, A = G G^H + reg I, Cholesky (a pivot <= 0 or not finite: W = 0, Fbb = 0), Vbb = G^H A^-1,
            V = Frf Vbb, c_m = sqrt(Nt / M) / |V[:, m]|_2 (zero / non-finite norm: 0), W[:, m] = c_m V[:, m], Fbb[:, m] = c_m Vbb[:, m]"""
import numpy as np

import mu_link_ref as MU

N = MU.N


def scores(hest_list, ns, At, dtype=np.complex128):
    """One packet.  hest_list: U arrays [nr, nt, 234], At [nt, R] -> S [M, R] (float64 for complex128, float32 for complex64: the same
    statement in the narrower type, the yardstick of the device's error)"""
    B = MU.stack_rows(hest_list, ns).astype(dtype)                                       # [234, M, nt]
    psi = B @ np.asarray(At).astype(dtype)                                               # [234, M, R]
    return (psi.real ** 2 + psi.imag ** 2).sum(0)


def select(S, n_rf):
    """S [M, R] -> idx int32 [n_rf]"""
    S = np.where(np.isfinite(S), np.asarray(S, np.float64), -np.inf)
    M, R = S.shape
    free = np.ones(R, bool)
    idx = np.empty(n_rf, np.int32)
    for q in range(n_rf):
        row = np.where(free, S[q % M], -np.inf)
        cand = np.flatnonzero(free & (row == row.max()))                                 # every free ray is a candidate when all are -inf
        idx[q] = cand[0]
        free[idx[q]] = False
    return idx


def margins(S, idx):
    """per slot q: (relative margin of the chosen score over the runner-up among the rays free at that slot, the runner-up's index or -1)"""
    S = np.where(np.isfinite(S), np.asarray(S, np.float64), -np.inf)
    M, R = S.shape
    free = np.ones(R, bool)
    out = []
    for q, r in enumerate(idx):
        row = np.where(free, S[q % M], -np.inf)
        row[r] = -np.inf
        second = int(np.argmax(row)) if np.isfinite(row.max()) else -1
        best = S[q % M, r]
        out.append(((best - row[second]) / best if second >= 0 and best > 0 else np.inf, second))
        free[r] = False
    return out


def baseband(hest_list, ns, At, idx, reg=0.0):
    """One packet with the beams idx.  Returns (W complex128 [M, nt, 234], Fbb [234, n_rf, M], cond(G) [234]).  Singular items: zeros."""
    B = MU.stack_rows(hest_list, ns)
    K, M, nt = B.shape
    Frf = np.asarray(At, np.complex128)[:, np.asarray(idx)]                              # [nt, n_rf]
    Q = Frf.shape[1]
    W = np.zeros((M, nt, K), np.complex128)
    Fbb = np.zeros((K, Q, M), np.complex128)
    cond = np.full(K, np.inf)
    for k in range(K):
        G = B[k] @ Frf
        if not np.isfinite(G).all():
            continue
        sv = np.linalg.svd(G, compute_uv=False)
        if sv[-1] > 0:
            cond[k] = sv[0] / sv[-1]
        A = G @ np.conj(G).T + float(reg) * np.eye(M)
        Lm = MU._cholesky(A) if np.isfinite(A).all() else None
        if Lm is None:
            continue
        Vbb = np.conj(np.linalg.solve(np.conj(Lm).T, np.linalg.solve(Lm, G))).T          # G^H A^-1 = (A^-1 G)^H, [n_rf, M]
        V = Frf @ Vbb
        nrm = np.sqrt((np.abs(V) ** 2).sum(0))
        good = np.isfinite(nrm) & (nrm > 0)
        c = np.where(good, np.sqrt(nt / M) / np.where(good, nrm, 1.0), 0.0)
        W[:, :, k] = (V * c).T
        Fbb[k] = Vbb * c
    return W, Fbb, cond


def precoder(hest_list, ns, At, n_rf, reg=0.0, idx=None):
    """One packet: (W [M, nt, 234], idx int32 [n_rf], Fbb [234, n_rf, M], S [M, R], cond(G) [234]).  A given idx skips the selection."""
    S = scores(hest_list, ns, At)
    if idx is None:
        idx = select(S, n_rf)
    idx = np.asarray(idx, np.int32)
    W, Fbb, cond = baseband(hest_list, ns, At, idx, reg)
    return W, idx, Fbb, S, cond
