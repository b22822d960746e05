"""Host statement of the channel forecast (csrc/forecast.hip.h), numpy only, fp64 throughout, written from the
definition in include/csi_mamimo.h and not from a device run.

The soundings x_0 .. x_{P-1} run oldest to newest, equally spaced; x is complex [P, npkt, nr, nt, 234].  Per (packet, rx), order M,
horizon d sounding intervals:

    T[i][q]  = sum_j sum_k conj(x_i[j][k]) x_q[j][k]                                 gram
    G[a][b]  = sum_{p = M+d-1}^{P-1} T[p-d-a][p-d-b],  rhs[a] = sum_p T[p-d-a][p]    system
    (G + ridge trace(G) / M I) c = rhs                                               solve (Cholesky; a pivot <= 0 or not finite: c = e_0, info 1)
    y = sum_{m < M} c_m x_{P-1-m}                                                    apply
    fit_err = max(0, 1 - Re(c^H rhs) / sum_p T[p][p])   (0 where that energy is not positive)

Pooling: G, rhs and the energy of a packet's rx antennas are added in ascending rx order before the solve.  The estimation error of a
simulated history (csi_sounding_noise_device) is replayed from tests/train_streams.py (the device's tr_normal) and synth_streams.key."""
import numpy as np

import synth_streams as ss
import train_streams as ts

N_DATA = 234


def gram(x):
    """T complex128 [npkt, nr, P, P] of x [P, npkt, nr, nt, 234]"""
    x = np.asarray(x, np.complex128)
    P, npkt, nr = x.shape[:3]
    f = x.reshape(P, npkt, nr, -1)
    return np.einsum('ipre,qpre->priq', f.conj(), f)


def system(T, M, d):
    """(G [M, M], rhs [M], energy) of one Gram matrix T [P, P]"""
    T = np.asarray(T, np.complex128)
    P = T.shape[0]
    assert 1 <= M and 1 <= d and M + d <= P, (P, M, d)
    G, rhs, energy = np.zeros((M, M), np.complex128), np.zeros(M, np.complex128), 0.0
    for p in range(M + d - 1, P):
        idx = p - d - np.arange(M)
        G += T[np.ix_(idx, idx)]
        rhs += T[idx, p]
        energy += T[p, p].real
    return G, rhs, energy


def solve(G, rhs, energy, ridge):
    """(c [M], info, fit_err, A): the ridge, an explicit Cholesky with the pivot rule, the two triangular solves"""
    M = G.shape[0]
    A = G + ridge * np.trace(G).real / M * np.eye(M)
    L = np.zeros((M, M), np.complex128)
    bad = False
    with np.errstate(all='ignore'):
        for j in range(M):
            dj = A[j, j].real - np.sum(np.abs(L[j, :j]) ** 2)
            if not (dj > 0.0) or not np.isfinite(dj):
                bad = True
                break
            L[j, j] = np.sqrt(dj)
            for i in range(j + 1, M):
                L[i, j] = (A[i, j] - np.sum(L[i, :j] * L[j, :j].conj())) / L[j, j]
    if bad:
        c = np.zeros(M, np.complex128)
        c[0] = 1.0
    else:
        z = np.zeros(M, np.complex128)
        for j in range(M):
            z[j] = (rhs[j] - np.sum(L[j, :j] * z[:j])) / L[j, j]
        c = np.zeros(M, np.complex128)
        for j in range(M - 1, -1, -1):
            c[j] = (z[j] - np.sum(L[j + 1:, j].conj() * c[j + 1:])) / L[j, j]
    fit_err = 0.0
    if energy > 0.0:
        with np.errstate(all='ignore'):
            fe = 1.0 - np.vdot(c, rhs).real / energy
        fit_err = fe if fe > 0.0 else 0.0
    return c, int(bad), fit_err, A


def fit(T, M, d, ridge=1e-5, pool_rx=False):
    """T [npkt, nr, P, P] -> dict of c complex128 [npkt, nr, M], info int [npkt, nr], fit_err [npkt, nr], cond [npkt, nr] (the 2-norm
    condition number of the matrix the solve sees; inf for a fallback) and amp [npkt, nr] = sum_a |c_a| |rhs_a| / energy, the size of the terms
    behind fit_err (0 without energy)"""
    T = np.asarray(T, np.complex128)
    npkt, nr = T.shape[:2]
    out = dict(c=np.zeros((npkt, nr, M), np.complex128), info=np.zeros((npkt, nr), np.int64), fit_err=np.zeros((npkt, nr)), cond=np.zeros((npkt, nr)),
               amp=np.zeros((npkt, nr)))
    for p in range(npkt):
        sys_r = [system(T[p, r], M, d) for r in range(nr)]
        if pool_rx:
            G, rhs, en = sys_r[0]
            for r in range(1, nr):
                G, rhs, en = G + sys_r[r][0], rhs + sys_r[r][1], en + sys_r[r][2]
            sys_r = [(G, rhs, en)] * nr
        for r in range(nr):
            c, info, fe, A = solve(*sys_r[r], ridge)
            with np.errstate(all='ignore'):
                cond = np.linalg.cond(A) if not info and np.all(np.isfinite(A)) else np.inf
            out['c'][p, r], out['info'][p, r], out['fit_err'][p, r], out['cond'][p, r] = c, info, fe, cond
            out['amp'][p, r] = np.sum(np.abs(c) * np.abs(sys_r[r][1])) / sys_r[r][2] if sys_r[r][2] > 0.0 else 0.0
    return out


def apply(x, c):
    """y [npkt, nr, nt, 234] = sum_m c_m x_{P-1-m}; c [npkt, nr, M]"""
    x = np.asarray(x, np.complex128)
    c = np.asarray(c, np.complex128)
    P = x.shape[0]
    y = np.zeros(x.shape[1:], np.complex128)
    for m in range(c.shape[-1]):
        y += c[:, :, m, None, None] * x[P - 1 - m]
    return y


def forecast(x, M, d, ridge=1e-5, pool_rx=False):
    """(y, fit dict) of the soundings x"""
    f = fit(gram(x), M, d, ridge, pool_rx)
    return apply(x, f['c']), f


def nmse(est, true):
    """sum |est - true|^2 / sum |true|^2 over everything"""
    est, true = np.asarray(est, np.complex128), np.asarray(true, np.complex128)
    return float(np.sum(np.abs(est - true) ** 2) / np.sum(np.abs(true) ** 2))


def noise_normals(seed, first_pkt, npkt, nr, nt):
    """complex128 [npkt, nr, nt, 234]: n_re + i n_im of csi_sounding_noise_device, element e = (r nt + j) 234 + k of packet
    first_pkt + p drawing normal(kn, 2 e) and normal(kn, 2 e + 1) of kn = key(seed, first_pkt + p, 1)"""
    out = np.empty((npkt, nr, nt, N_DATA), np.complex128)
    e = np.arange(nr * nt * N_DATA, dtype=np.uint64) * np.uint64(2)
    for p in range(npkt):
        kn = ss.key(seed, first_pkt + p, 1)
        out[p] = (ts.normal(kn, e)[0] + 1j * ts.normal(kn, e + np.uint64(1))[0]).reshape(nr, nt, N_DATA)
    return out


def sounding_noise(x, err_var, seed, first_pkt):
    """x + s (n_re + i n_im) with s = sqrtf(0.5f v) as the device forms it: x [npkt, nr, nt, 234], err_var [npkt, nr]"""
    x = np.asarray(x, np.complex128)
    npkt, nr, nt = x.shape[:3]
    s = np.sqrt(np.float32(0.5) * np.asarray(err_var, np.float32), dtype=np.float32).astype(np.float64)
    return x + s[:, :, None, None] * noise_normals(seed, first_pkt, npkt, nr, nt)
