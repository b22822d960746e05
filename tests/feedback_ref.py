"""The quantised CSI feedback of DESIGN.md 4.24 (IEEE 802.11-2016 19.3.12.3.6 with Nt rows) stated in numpy: the decomposition of the
singular vectors into Givens angles, the quantiser and the expansion (test helper, no test collects from here).

Everything is vectorised over the leading axis (one entry = one (packet, reported carrier) report).  `dtype` selects the arithmetic:
np.float64 is the reference; np.float32 is the complex64 RESTATEMENT - the same operations in the device's number format, the yardstick
for what fp32 rounding alone does to a result.  Both expansions rotate with the same cos / sin numbers: the tables of the bin centres
computed in double and rounded to float32, as the library's host side computes them."""
import numpy as np

N = 234


def n_angles(nt, nc):
    return sum(nt - 1 - i for i in range(min(nc, nt - 1)))


def n_reports(ng):
    return -(-N // ng)


def _ct(dtype):
    return np.complex64 if dtype == np.float32 else np.complex128


def svd_vectors(H, nc):
    """H [n, nr, nt] complex -> (V [n, nt, nc], sigma [n, nc]) in fp64: the nc dominant right singular vectors, a zero column where
    sigma_s = 0 (the column phases are whatever LAPACK left: column_phases fixes them)"""
    H = np.asarray(H, np.complex128)
    _, s, vh = np.linalg.svd(H, full_matrices=False)
    V = np.conj(vh[:, :nc, :]).transpose(0, 2, 1).copy()
    s = s[:, :nc]
    V[np.broadcast_to((s == 0)[:, None, :], V.shape)] = 0
    return V, s


def column_phases(V, dtype=np.float64):
    """step 2: every column times exp(-j arg V[Nt-1][s]): the last row real and >= 0; arg 0 = 0"""
    V = np.asarray(V).astype(_ct(dtype))
    last = V[:, -1:, :]
    m = np.abs(last).astype(dtype)
    u = np.where(m > 0, last / np.where(m > 0, m, 1), 1).astype(_ct(dtype))
    out = (V * np.conj(u)).astype(_ct(dtype))
    out[:, -1, :] = m[:, 0, :]
    return out


def decompose(V, dtype=np.float64):
    """V [n, nt, nc] after column_phases -> (phi [n, n_ang] in [0, 2 pi), psi [n, n_ang] in [0, pi/2], what is left of V: the first nc
    columns of the identity up to rounding).  Phases and rotations use c, s from the moduli (hypot); angles from arctan2."""
    ct = _ct(dtype)
    V = np.asarray(V).astype(ct).copy()
    n, nt, nc = V.shape
    two_pi = dtype(2 * np.pi)
    phis, psis = [], []
    for i in range(min(nc, nt - 1)):
        x = V[:, i:nt - 1, i]
        m = np.abs(x).astype(dtype)
        u = np.where(m > 0, x / np.where(m > 0, m, 1), 1).astype(ct)
        phi = np.where(m > 0, np.arctan2(x.imag, x.real), 0).astype(dtype)
        phi = np.where(phi < 0, phi + two_pi, phi).astype(dtype)
        phi = np.where(phi < two_pi, phi, 0).astype(dtype)
        phis.append(phi)
        V[:, i:nt - 1, :] = (V[:, i:nt - 1, :] * np.conj(u)[:, :, None]).astype(ct)
        V[:, i:nt - 1, i] = m
        for l in range(i + 1, nt):
            a, b = V[:, i, i].real.astype(dtype), V[:, l, i].real.astype(dtype)
            h = np.hypot(a, b).astype(dtype)
            c = np.where(h > 0, a / np.where(h > 0, h, 1), 1).astype(dtype)[:, None]
            s = np.where(h > 0, b / np.where(h > 0, h, 1), 0).astype(dtype)[:, None]
            psis.append(np.clip(np.arctan2(b, a), 0, dtype(np.pi / 2)).astype(dtype))
            ri, rl = V[:, i, :].copy(), V[:, l, :].copy()
            V[:, i, :] = (c * ri + s * rl).astype(ct)
            V[:, l, :] = (c * rl - s * ri).astype(ct)
    return np.concatenate(phis, 1), np.stack(psis, 1), V


def quantise(phi, psi, b_phi, b_psi):
    """k_phi = floor(phi 2^(b_phi-1) / pi) mod 2^b_phi, k_psi = min(floor(psi 2^(b_psi+1) / pi), 2^b_psi - 1), in the angles' own dtype"""
    dt = phi.dtype.type
    kp = np.floor(phi * dt(2.0 ** (b_phi - 1) / np.pi)).astype(np.int64) % (2 ** b_phi)
    ks = np.minimum(np.floor(psi * dt(2.0 ** (b_psi + 1) / np.pi)).astype(np.int64), 2 ** b_psi - 1)
    return kp, np.maximum(ks, 0)


def centres(b_phi, b_psi):
    phi = np.pi * (2.0 ** -b_phi + np.arange(2 ** b_phi) * 2.0 ** (1 - b_phi))
    psi = np.pi * (2.0 ** -(b_psi + 2) + np.arange(2 ** b_psi) * 2.0 ** -(b_psi + 1))
    return phi, psi


def centre_tables(b_phi, b_psi):
    """cos phi, sin phi, cos psi, sin psi of the bin centres: double, rounded to float32"""
    phi, psi = centres(b_phi, b_psi)
    return tuple(t.astype(np.float32) for t in (np.cos(phi), np.sin(phi), np.cos(psi), np.sin(psi)))


def _expand(cphi, sphi, cpsi, spsi, nt, nc, dtype):
    """the steps backwards on the identity; cphi .. spsi [n, n_ang] in dtype"""
    ct = _ct(dtype)
    n = cphi.shape[0]
    V = np.zeros((n, nt, nc), ct)
    for s in range(nc):
        V[:, s, s] = 1
    off = n_angles(nt, nc)
    for i in reversed(range(min(nc, nt - 1))):
        cnt = nt - 1 - i
        off -= cnt
        for l in reversed(range(i + 1, nt)):
            c, s = cpsi[:, off + l - i - 1][:, None], spsi[:, off + l - i - 1][:, None]
            ri, rl = V[:, i, :].copy(), V[:, l, :].copy()
            V[:, i, :] = (c * ri - s * rl).astype(ct)
            V[:, l, :] = (s * ri + c * rl).astype(ct)
        u = (cphi[:, off:off + cnt] + 1j * sphi[:, off:off + cnt]).astype(ct)
        V[:, i:nt - 1, :] = (V[:, i:nt - 1, :] * u[:, :, None]).astype(ct)
    return V


def expand(kphi, kpsi, nt, nc, b_phi, b_psi, dtype=np.float64, exact=False):
    """codes [n, n_ang] -> Vhat [n, nt, nc], rotating with the float32 tables of the bin centres (what the device rotates with: cos^2 +
    sin^2 = 1 only to 2^-24); exact=True: with the cos / sin of the centres in double, the definition itself"""
    if exact:
        phi, psi = centres(b_phi, b_psi)
        return expand_angles(phi[kphi], psi[kpsi], nt, nc, np.float64)
    t = [x.astype(dtype) for x in centre_tables(b_phi, b_psi)]
    return _expand(t[0][kphi], t[1][kphi], t[2][kpsi], t[3][kpsi], nt, nc, dtype)


def expand_angles(phi, psi, nt, nc, dtype=np.float64):
    """continuous angles [n, n_ang] -> Vhat [n, nt, nc]"""
    phi, psi = np.asarray(phi).astype(dtype), np.asarray(psi).astype(dtype)
    return _expand(np.cos(phi), np.sin(phi), np.cos(psi), np.sin(psi), nt, nc, dtype)


def planes(seed, npkt, nr, nt):
    """i.i.d. complex Gaussian CSI planes [npkt, nr, nt, 234] of unit variance, complex64"""
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((npkt, nr, nt, N)) + 1j * rng.standard_normal((npkt, nr, nt, N))) / np.sqrt(2.0)).astype(np.complex64)


def reported(h, ng):
    """[npkt, nr, nt, 234] -> the matrices of the reported carriers [npkt n_rep, nr, nt] (packet-major)"""
    npkt, nr, nt, _ = h.shape
    return np.asarray(h)[..., ::ng].transpose(0, 3, 1, 2).reshape(-1, nr, nt)


def cyclic_diff(a, b, b_phi):
    """|a - b| modulo 2^b_phi, as a distance on the circle"""
    d = (np.asarray(a, np.int64) - np.asarray(b, np.int64)) % (2 ** b_phi)
    return np.minimum(d, 2 ** b_phi - d)
