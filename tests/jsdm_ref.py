"""Host restatement of the multi-user JSDM precoder (csrc/mu_jsdm.hip.h), numpy, on top of tests/mu_link_ref.py.  Written
from the definition of include/csi_mamimo.h, not from a device run (no test collects from here).  Every function takes dtype=complex128
(the fp64 statement) or complex64 (the same statement in the narrower type, the yardstick of the device's error).

  cov       R_u[j][j'] = (1 / (Nr 234)) sum_i sum_k conj(h_u[i][j][k]) h_u[i][j'][k];  R_g = the mean over the group's users, ascending
  eig       R_g = U L U^H, descending; in each eigenvector the entry of largest modulus real and positive (lowest j on a tie);
            r_g = #{i < r_star: l_i > rank_tol l_0} (l_0 <= 0 or not finite: 0);  U*_g = the first r_g columns
  null      Xi_g = [U*_g' : g' != g, ascending];  Q_g = modified Gram-Schmidt in column order, two passes, a column whose residual is
            <= 1e-3 of its norm is dropped;  Rt_g = P R_g P - l_0(R_g) Q_g Q_g^H, P = I - Q_g Q_g^H, symmetrised
  beams     F_g = the first b eigenvectors of Rt_g, same convention; unit modulus: exp(i arg) / sqrt(Nt), arg 0 = 0;  Frf = [F_0 ... F_{G-1}]
  baseband  per subcarrier: Gm = B_k Frf (per-group processing: entries whose chain's group differs from the stream's group are 0),
            A = Gm Gm^H + reg I, Cholesky (singular: W = 0, Fbb = 0), Vbb = Gm^H A^-1, V = Frf Vbb, c_m = sqrt(Nt / M) / |V[:, m]|,
            W[:, m] = c_m V[:, m], Fbb[:, m] = c_m Vbb[:, m]"""
import numpy as np

import mu_link_ref as MU

N = MU.N
PGP, UNIT = 1, 2


def dft(nt):
    j = np.arange(nt)
    return np.exp(-2j * np.pi * np.outer(j, j) / nt) / np.sqrt(nt)


def planes(nt, nr, nu, npkt, seed=5, decay=0.6):
    """The planes of the tests, with a prescribed covariance: user u uses F[:, roll(arange(Nt), -(5u mod Nt))], l_j = decay^j,
    z ~ CN(0,1) [Nr][234][Nt], rows (z sqrt(l)) F_u^H; default_rng(seed), users drawn in order within a packet.
    Returns U arrays [npkt, nr, nt, 234] complex128."""
    rng = np.random.default_rng(seed)
    F = dft(nt)
    lam = decay ** np.arange(nt)
    out = [np.empty((npkt, nr, nt, N), np.complex128) for _ in range(nu)]
    for p in range(npkt):
        for u in range(nu):
            Fu = F[:, np.roll(np.arange(nt), -((5 * u) % nt))]
            z = (rng.standard_normal((nr, N, nt)) + 1j * rng.standard_normal((nr, N, nt))) / np.sqrt(2.0)
            rows = (z * np.sqrt(lam)) @ np.conj(Fu).T                                    # [nr, 234, nt]
            out[u][p] = rows.transpose(0, 2, 1)
    return out


def groups_of(nu, group=None):
    g = np.arange(nu) if group is None else np.asarray(group, int)
    G = int(g.max()) + 1
    assert g.shape == (nu,) and g.min() >= 0 and all((g == x).any() for x in range(G))
    return g, G


def covariance(h, dtype=np.complex128):
    """h [nr, nt, 234] -> R [nt, nt]"""
    h = np.asarray(h).astype(dtype)
    nr, nt, n = h.shape
    X = h.transpose(0, 2, 1).reshape(nr * n, nt)                                         # rows h[i][:, k]
    R = np.conj(X).T @ X / dtype(nr * n).real
    return R.astype(dtype)


def phase(V):
    """columns of V with their entry of largest modulus real and positive (lowest j on a tie)"""
    V = np.array(V)
    for c in range(V.shape[1]):
        j = int(np.argmax(np.abs(V[:, c])))
        a = np.abs(V[j, c])
        if a > 0 and np.isfinite(a):
            V[:, c] = V[:, c] * (np.conj(V[j, c]) / a)
            V[j, c] = a
    return V


def eig_desc(R):
    """Hermitian R -> (eigenvalues descending, eigenvectors with the phase convention)"""
    R = np.asarray(R)
    lam, V = np.linalg.eigh((R + np.conj(R).T) / 2)
    order = np.argsort(-lam, kind='stable')
    return lam[order], phase(V[:, order])


def kept_rank(lam, r_star, rank_tol):
    l0 = lam[0]
    if not (l0 > 0) or not np.isfinite(l0):
        return 0
    return int(sum(1 for i in range(r_star) if lam[i] > rank_tol * l0))


def gram_schmidt(X):
    """modified Gram-Schmidt in column order, two passes over the columns kept so far; a column whose residual is <= 1e-3 of its norm is
    dropped.  X [nt, c] -> Q [nt, q]"""
    X = np.asarray(X)
    Q = np.zeros((X.shape[0], 0), X.dtype)
    for c in range(X.shape[1]):
        v = X[:, c].copy()
        n0 = np.sqrt((np.abs(v) ** 2).sum())
        for _ in range(2):
            for q in range(Q.shape[1]):
                v = v - Q[:, q] * (np.conj(Q[:, q]) @ v)
        res = np.sqrt((np.abs(v) ** 2).sum())
        if res > 1e-3 * n0 and np.isfinite(res):
            Q = np.concatenate([Q, (v / res)[:, None]], 1)
    return Q


def nulled(R, Q, lam0, deflate=True):
    """Rt = P R P - lam0 Q Q^H, symmetrised (deflate=False: plain P R P, what the deflation term is compared against)"""
    nt = R.shape[0]
    P = np.eye(nt, dtype=R.dtype) - Q @ np.conj(Q).T
    Rt = P @ R @ P
    if deflate:
        Rt = Rt - R.dtype.type(lam0) * (Q @ np.conj(Q).T)
    return (Rt + np.conj(Rt).T) / 2


def unit_modulus(F):
    nt = F.shape[0]
    a = np.abs(F)
    ph = np.where(a > 0, F / np.where(a > 0, a, 1), 1.0)
    return (ph / np.sqrt(nt)).astype(F.dtype)


def analog(hest_list=None, group=None, r_star=0, b=1, rank_tol=0.0, flags=0, cov=None, ustar=None, dtype=np.complex128, deflate=True):
    """One packet.  hest_list: U arrays [nr, nt, 234] (or cov: U matrices [nt, nt]).  A given ustar (list of G arrays [nt, r_g]) replaces
    the first stage's eigenvectors in the nulling.  Returns a dict: Frf [nt, G b], cov [U, nt, nt], Rg [G], eig [G, nt], ustar (list of
    [nt, r_g]), rank [G, 2] = (r_g, q_g), Rt [G], eig_t [G, nt], gaps [G, 2] (relative gap at r_g of R_g - 1 where r_g is 0 or r_star
    reaches no further eigenvalue -, relative gap at b of Rt_g), margin [G] (distance of the nearest tested ratio l_i / l_0 to rank_tol)"""
    if cov is None:
        cov = [covariance(h, dtype) for h in hest_list]
    cov = [np.asarray(c).astype(dtype) for c in cov]
    nu, nt = len(cov), cov[0].shape[0]
    g, G = groups_of(nu, group)
    Rg, lams, vecs, ranks, margin = [], [], [], [], []
    for x in range(G):
        mem = [u for u in range(nu) if g[u] == x]
        R = cov[mem[0]].copy()
        for u in mem[1:]:
            R = R + cov[u]
        R = R / dtype(len(mem)).real
        lam, V = eig_desc(R)
        Rg.append(R); lams.append(lam); vecs.append(V)
        ranks.append(kept_rank(lam, r_star, rank_tol))
        margin.append(min([abs(lam[i] / lam[0] - rank_tol) for i in range(r_star)], default=np.inf) if lam[0] > 0 else np.inf)
    us = [vecs[x][:, :ranks[x]] for x in range(G)] if ustar is None else [np.asarray(x).astype(dtype) for x in ustar]
    Frf = np.zeros((nt, G * b), dtype)
    Rts, lamts, qs, gaps, Qs = [], [], [], [], []
    for x in range(G):
        Xi = np.concatenate([us[y] for y in range(G) if y != x] + [np.zeros((nt, 0), dtype)], 1)
        Q = gram_schmidt(Xi)
        Rt = nulled(Rg[x], Q, lams[x][0], deflate)
        lt, Vt = eig_desc(Rt)
        F = Vt[:, :b]
        if flags & UNIT:
            F = unit_modulus(F)
        Frf[:, x * b:(x + 1) * b] = F
        Rts.append(Rt); lamts.append(lt); qs.append(Q.shape[1]); Qs.append(Q)
        r = ranks[x]
        g1 = (lams[x][r - 1] - lams[x][r]) / lams[x][0] if 0 < r < nt else 1.0
        g2 = (lt[b - 1] - lt[b]) / max(lams[x][0], lt[0]) if b < nt else 1.0
        gaps.append((float(g1), float(g2)))
    return dict(Frf=Frf, cov=np.stack(cov), Rg=Rg, eig=np.stack(lams), ustar=us, rank=np.array([(ranks[x], qs[x]) for x in range(G)]),
                Rt=Rts, eig_t=np.stack(lamts), gaps=np.array(gaps), margin=np.array(margin), vecs=vecs, Q=Qs)


def baseband(hest_list, ns, Frf, group=None, b=None, flags=0, reg=0.0):
    """One packet with the analog matrix Frf [nt, n_rf].  Returns (W complex128 [M, nt, 234], Fbb [234, n_rf, M], cond(Gm) [234])."""
    B = MU.stack_rows(hest_list, ns)
    K, M, nt = B.shape
    Frf = np.asarray(Frf, np.complex128)
    Q = Frf.shape[1]
    g, G = groups_of(len(hest_list), group)
    b = Q // G if b is None else b
    mask = np.ones((M, Q))
    if flags & PGP:
        mask = (np.repeat(g, ns)[:, None] == (np.arange(Q) // b)[None, :]).astype(float)
    W = np.zeros((M, nt, K), np.complex128)
    Fbb = np.zeros((K, Q, M), np.complex128)
    cond = np.full(K, np.inf)
    for k in range(K):
        Gm = (B[k] @ Frf) * mask
        if not np.isfinite(Gm).all():
            continue
        sv = np.linalg.svd(Gm, compute_uv=False)
        if sv[-1] > 0:
            cond[k] = sv[0] / sv[-1]
        A = Gm @ np.conj(Gm).T + float(reg) * np.eye(M)
        Lm = MU._cholesky(A) if np.isfinite(A).all() else None
        if Lm is None:
            continue
        Vbb = np.conj(np.linalg.solve(np.conj(Lm).T, np.linalg.solve(Lm, Gm))).T          # Gm^H A^-1, [n_rf, M]
        V = Frf @ Vbb
        nrm = np.sqrt((np.abs(V) ** 2).sum(0))
        good = np.isfinite(nrm) & (nrm > 0)
        c = np.where(good, np.sqrt(nt / M) / np.where(good, nrm, 1.0), 0.0)
        W[:, :, k] = (V * c).T
        Fbb[k] = Vbb * c
    return W, Fbb, cond


def precoder(hest_list, ns, group=None, r_star=0, b=1, rank_tol=0.0, flags=0, reg=0.0, cov=None):
    """One packet in fp64: (W [M, nt, 234], Fbb [234, n_rf, M], cond [234], the dict of analog())"""
    an = analog(hest_list, group, r_star, b, rank_tol, flags, cov=cov)
    W, Fbb, cond = baseband(hest_list, ns, an['Frf'], group, b, flags, reg)
    return W, Fbb, cond, an


# ------------------------------------------------------------------------------------------------ the eigen kernel's arithmetic
def round_robin(nt, t):
    """The pairs of step t (0 .. n' - 2) of the kernel's parallel ordering, n' = nt rounded up to even (circle method: n' - 1 stays, the
    others turn): n' / 2 pairs (p, q) with p < q.  With an odd nt the pair that holds n' - 1 = nt is no rotation: its p sits out."""
    n2 = (nt + 1) & ~1
    steps = n2 - 1
    out = []
    for i in range(n2 // 2):
        x = n2 - 1 if i == 0 else (t + i) % steps
        y = t if i == 0 else (t - i + steps) % steps
        out.append((min(x, y), max(x, y)))
    return out


def jacobi_f32(A, max_sweeps=24):
    """mu_jsdm_eig_kernel's solver step by step in float32 / complex64 (one numpy operation per device operation, no fused
    multiply-add): the ordering of round_robin, per pair t = sgn(tau) / (|tau| + sqrt(1 + tau^2)) with the phase of a_pq folded into the
    rotation J = [[c, s], [-s e^{-i phi}, c e^{-i phi}]], every 2 x 2 block (pair i, pair j), i <= j, as J_i^H B J_j and mirrored, a
    rotation applied where |a_pq| > 2^-23 max_j |A[j][j]| of the input, the first sweep without one ends the iteration.  Returns
    (eigenvalues descending float32, vectors complex64 with the phase convention, sweeps run including the last, empty one)."""
    f, c64 = np.float32, np.complex64
    A = np.array(A, c64)
    nt = A.shape[0]
    V = np.eye(nt, dtype=c64)
    thr = f(np.abs(A.diagonal().real).max()) * f(2.0 ** -23)
    n2 = (nt + 1) & ~1
    sweeps = 0
    for sweeps in range(1, max_sweeps + 1):
        rotated = False
        for t in range(n2 - 1):
            rots = []
            for pp, qq in round_robin(nt, t):
                c, s, e, tb, on = f(1), f(0), c64(1), f(0), False
                if qq < nt:
                    bq = A[pp, qq]
                    bm = f(np.abs(bq))
                    if bm > thr and np.isfinite(bm):
                        tau = f((A[qq, qq].real - A[pp, pp].real) / (f(2) * bm))
                        tt = f((f(1) if tau >= 0 else f(-1)) / (f(abs(tau)) + f(np.sqrt(f(tau * tau + f(1))))))
                        c = f(f(1) / f(np.sqrt(f(tt * tt + f(1)))))
                        s, e, tb, on = f(tt * c), c64(bq / bm), f(tt * bm), True
                        rotated = True
                rots.append((pp, qq, c, s, e, tb, on))
            B = A.copy()
            for i in range(len(rots)):
                for j in range(i, len(rots)):
                    pi, qi, ci, si, ei, tbi, oi = rots[i]
                    pj, qj, cj, sj, ej, tbj, oj = rots[j]
                    if i == j:
                        if oi:
                            B[pi, pi] = f(A[pi, pi].real - tbi)
                            B[qi, qi] = f(A[qi, qi].real + tbi)
                            B[pi, qi] = B[qi, pi] = 0
                        continue
                    if not oi and not oj:
                        continue
                    hi, hj = qi < nt, qj < nt
                    b00, b01 = A[pi, pj], (A[pi, qj] if hj else c64(0))
                    b10, b11 = (A[qi, pj] if hi else c64(0)), (A[qi, qj] if hi and hj else c64(0))
                    z0, z1 = c64(ei * b10), c64(ei * b11)                                # rows by J_i^H
                    b00, b01, b10, b11 = c64(ci * b00 - si * z0), c64(ci * b01 - si * z1), c64(si * b00 + ci * z0), c64(si * b01 + ci * z1)
                    z0, z1 = c64(np.conj(ej) * b01), c64(np.conj(ej) * b11)              # columns by J_j
                    b00, b10, b01, b11 = c64(cj * b00 - sj * z0), c64(cj * b10 - sj * z1), c64(sj * b00 + cj * z0), c64(sj * b10 + cj * z1)
                    B[pi, pj], B[pj, pi] = b00, np.conj(b00)
                    if hj:
                        B[pi, qj], B[qj, pi] = b01, np.conj(b01)
                    if hi:
                        B[qi, pj], B[pj, qi] = b10, np.conj(b10)
                    if hi and hj:
                        B[qi, qj], B[qj, qi] = b11, np.conj(b11)
            A = B
            for pj, qj, c, s, e, tb, on in rots:
                if on:
                    v0, z = V[:, pj].copy(), c64(np.conj(e)) * V[:, qj]
                    V[:, pj], V[:, qj] = c * v0 - s * z, s * v0 + c * z
        if not rotated:
            break
    lam = A.diagonal().real.astype(f)
    order = np.argsort(-lam, kind='stable')
    return lam[order], phase(V[:, order]), sweeps
