"""Host restatement of the multi-user downlink (csrc/mu_link.hip.h), numpy fp64, on top of tests/link_ref.py and
tests/synth_streams.py.  Written from the definitions of that header, not from a device run (no test collects from here).

  precoder   per (packet, subcarrier): B[m][j] = hest_u[s][j][k], m = u ns + s;  A = B B^H + reg I;  Cholesky A = L L^H (a pivot <= 0
             or not finite: W = 0);  V = B^H A^-1;  W[:, m] = sqrt(Nt / M) V[:, m] / |V[:, m]|_2 (zero / non-finite norm: 0)
  user seed  seed_0 = seed, seed_u = splitmix64(seed ^ splitmix64(u))
  data       bits, encoder and mapper of link_ref for (ns, n_sym, bps) on the stream seed_u;  y_u = G_u d + w, G_u = H_u[0:ns] W
             (ns x M), w from link_ref.noise_normals(seed_u, pkt, n_sym, nr = ns);  the single-user equaliser on G_uu;  soft bits with
             csi_s / noise_var (no interference term);  sinr_db = 10 log10(sum |G_uu|^2 / (sum |G_u,others|^2 + 234 ns noise_var))"""
import numpy as np

import link_ref as L
import train_streams as ts

N = L.N


def user_seed(seed, u):
    if u == 0:
        return int(seed) & ts.MASK64
    inner = int(ts.splitmix64(np.uint64(u)))
    return int(ts.splitmix64(np.uint64((int(seed) & ts.MASK64) ^ inner)))


def stack_rows(hest_list, ns):
    """U arrays [nr, nt, 234] -> B [234, M, nt], row m = u ns + s"""
    B = np.concatenate([np.asarray(h, np.complex128)[:ns] for h in hest_list], 0)       # [M, nt, 234]
    return np.ascontiguousarray(B.transpose(2, 0, 1))


def _cholesky(A):
    """the stated rule, in fp64: the factor L, or None when a pivot of the factorisation is not finite or not > 0.  (Only an exact
    dependence is certain to give such a pivot: a rank-deficient B whose pivot is rounding noise of either sign passes or fails by chance,
    on the host as on the device - the tests use inputs whose arithmetic is exact.)"""
    n = A.shape[0]
    Lm = np.zeros_like(A)
    for c in range(n):
        d = A[c, c].real - (np.abs(Lm[c, :c]) ** 2).sum()
        if not (d > 0.0) or not np.isfinite(d):
            return None
        Lm[c, c] = np.sqrt(d)
        for i in range(c + 1, n):
            Lm[i, c] = (A[i, c] - (Lm[i, :c] * np.conj(Lm[c, :c])).sum()) / Lm[c, c]
    return Lm


def precoder(hest_list, ns, reg=0.0):
    """One packet.  hest_list: U arrays [nr, nt, 234] -> (W complex128 [M, nt, 234], cond(B) [234]).  Singular items: W = 0."""
    B = stack_rows(hest_list, ns)
    K, M, nt = B.shape
    W = np.zeros((M, nt, K), np.complex128)
    cond = np.full(K, np.inf)
    for k in range(K):
        sv = np.linalg.svd(B[k], compute_uv=False)
        if sv[-1] > 0:
            cond[k] = sv[0] / sv[-1]
        A = B[k] @ np.conj(B[k]).T + float(reg) * np.eye(M)
        Lm = _cholesky(A) if np.isfinite(A).all() else None
        if Lm is None:
            continue
        V = np.conj(np.linalg.solve(np.conj(Lm).T, np.linalg.solve(Lm, B[k]))).T         # B^H A^-1 = (A^-1 B)^H, [nt, M]
        nrm = np.sqrt((np.abs(V) ** 2).sum(0))
        good = np.isfinite(nrm) & (nrm > 0)
        scale = np.where(good, np.sqrt(nt / M) / np.where(good, nrm, 1.0), 0.0)
        W[:, :, k] = (V * scale).T
    return W, cond


def effective_channel(h, W, ns):
    """h [nr, nt, 234] (true planes of one user), W [M, nt, 234] -> G_u [234, ns, M]"""
    return np.einsum('ijk,mjk->kim', np.asarray(h, np.complex128)[:ns], np.asarray(W, np.complex128))


def sinr_db(G, u, ns, noise_var):
    """G [234, ns, M] of user u"""
    p = np.abs(G) ** 2
    own = p[:, :, u * ns:(u + 1) * ns].sum()
    others = p[:, :, :u * ns].sum() + p[:, :, (u + 1) * ns:].sum()
    with np.errstate(divide='ignore', invalid='ignore'):
        return 10.0 * np.log10(own / (others + N * ns * float(noise_var)))


def user_symbols(seed, pkt, u, ns, n_sym, bps):
    """(bits, coded, d [ns, n_sym, 234]) of user u's codeword in packet pkt"""
    n_info, _ = L.frame_bits(ns, n_sym, bps)
    bits = L.info_bits(user_seed(seed, u), pkt, n_info)
    coded = L.encode(bits)
    return bits, coded, L.map_bits(coded, ns, n_sym, bps)


def simulate(seed, pkt, h_list, W, noise_var, ns, n_sym, bps):
    """One packet in fp64.  h_list: U TRUE arrays [nr, nt, 234]; W [M, nt, 234]; noise_var [U].  Returns one dict per user: bits, coded, d,
    G, clean, w, y, x, csi, cond (of G_uu), llr, evm_rms, sinr_db."""
    U = len(h_list)
    sym = [user_symbols(seed, pkt, u, ns, n_sym, bps) for u in range(U)]
    d_all = np.concatenate([s[2] for s in sym], 0)                                       # [M, n_sym, 234]
    out = []
    for u in range(U):
        nv = float(np.asarray(noise_var).reshape(-1)[u])
        G = effective_channel(h_list[u], W, ns)
        clean = np.einsum('kim,mnk->nki', G, d_all)
        w = np.sqrt(nv / 2.0) * L.noise_normals(user_seed(seed, u), pkt, n_sym, ns)
        y = clean + w
        x, csi, cond = L.zero_forcing(np.ascontiguousarray(G[:, :, u * ns:(u + 1) * ns]), y)
        out.append(dict(bits=sym[u][0], coded=sym[u][1], d=sym[u][2], G=G, clean=clean, w=w, y=y, x=x, csi=csi, cond=cond,
                        llr=L.soft_bits(x, csi, nv, bps), evm_rms=L.evm_rms(x, bps), sinr_db=sinr_db(G, u, ns, nv)))
    return out
