"""Receive combining of DESIGN.md 4.25 (csrc/rx_combine.hip.h) stated in numpy on top of tests/feedback_ref.py and tests/mu_link_ref.py:
the U^H combiner of a CSI matrix with the phase rule of the feedback report, the rank rule, and the apply step (test helper, no test
collects from here).

Everything is vectorised over the leading axis (one entry = one (packet, carrier) item).  `dtype` selects the arithmetic: np.float64 is
the reference (numpy.linalg.svd in double); np.float32 is the complex64 RESTATEMENT - the same statement with the decomposition, the phase
and the products in single precision, the yardstick for what fp32 rounding alone does to a result."""
import numpy as np

import feedback_ref as R
import mu_link_ref as MU

N = R.N
RANK_FLOOR = 2.0 ** -20          # sigma_s / sigma_1 at or below which a row is rank noise (2^-40 on the eigenvalues of H H^H)


def _ct(dtype):
    return np.complex64 if dtype == np.float32 else np.complex128


def items(h):
    """[npkt, nr, nt, 234] -> the matrices of the items [npkt 234, nr, nt] (packet-major)"""
    return R.reported(h, 1)


def rows_of_items(c, npkt):
    """[npkt 234, a, b] -> the device layout [npkt, a, b, 234]"""
    return np.ascontiguousarray(c.reshape(npkt, N, c.shape[1], c.shape[2]).transpose(0, 2, 3, 1))


def combiner(H, ns, dtype=np.float64):
    """H [n, nr, nt] -> (C [n, ns, nr], sigma [n, ns]): row s = exp(i t_s) u_s^H of the s-th largest singular value, t_s making
    (C H)[s][nt-1] real and >= 0 (that element 0: no rotation); a row whose sigma is not finite, not > 0 or not > 2^-20 sigma_1 is zero
    and so is its sigma."""
    ct = _ct(dtype)
    H = np.asarray(H).astype(ct)
    u, s, _ = np.linalg.svd(H, full_matrices=False)
    s = s[:, :ns].astype(dtype)
    uh = np.conj(u[:, :, :ns]).transpose(0, 2, 1).astype(ct)                   # [n, ns, nr]
    z = (uh @ H[:, :, -1:])[:, :, 0]                                            # (u_s^H H)[nt-1]
    m = np.abs(z).astype(dtype)
    turn = (m > 0) & np.isfinite(m)
    f = np.where(turn, np.conj(z) / np.where(turn, m, 1), 1).astype(ct)
    live = np.isfinite(s) & (s > 0) & (s > dtype(RANK_FLOOR) * s[:, :1])
    C = np.where(live[:, :, None], f[:, :, None] * uh, 0).astype(ct)
    return C, np.where(live, s, 0).astype(dtype)


def apply(C, H, dtype=np.float64):
    """C [n, ns, nr], H [n, nr, nt] -> E [n, nr, nt]: rows s < ns = C H, the other rows zero"""
    ct = _ct(dtype)
    C, H = np.asarray(C).astype(ct), np.asarray(H).astype(ct)
    E = np.zeros(H.shape, ct)
    E[:, :C.shape[1], :] = C @ H
    return E


def planes_usv(seed, npkt, nr, nt):
    """CSI planes [npkt, nr, nt, 234] complex64 built per item as U S V^H with S = 4, 2, 1, 0.5, ...: the ratio 2 between neighbouring
    singular values keeps every singular vector well defined"""
    rng = np.random.default_rng(seed)
    n, r = npkt * N, min(nr, nt)
    qa, _ = np.linalg.qr(rng.standard_normal((n, nr, nr)) + 1j * rng.standard_normal((n, nr, nr)))
    qb, _ = np.linalg.qr(rng.standard_normal((n, nt, nt)) + 1j * rng.standard_normal((n, nt, nt)))
    s = 4.0 * 0.5 ** np.arange(r)
    H = (qa[:, :, :r] * s) @ np.conj(qb[:, :, :r]).transpose(0, 2, 1)
    return rows_of_items(H, npkt).astype(np.complex64)


def leakage(G_list, ns):
    """sum |G_u,others|^2 / sum |G_uu|^2 over the users; G_list[u] [234, ns, M] (mu_link_ref.effective_channel)"""
    own = others = 0.0
    for u, G in enumerate(G_list):
        p = np.abs(np.asarray(G)) ** 2
        mine = p[:, :, u * ns:(u + 1) * ns].sum()
        own, others = own + mine, others + p.sum() - mine
    return others / own


def arrangements(h_list, ns, noise_var):
    """One packet, perfect CSI, zero forcing; h_list = U true arrays [nr, nt, 234].  Returns {name: (mean sinr_db over the users, leakage)}
    of the three arrangements of the issue's table: 'MU' - precoder on the first rows, receiver on the first antennas; 'MUFB' - precoder on
    S V^H = C H, receiver on the first antennas; 'MUC' - precoder on C H, receiver applies C."""
    nr, nt, _ = h_list[0].shape
    comb = []
    for h in h_list:
        Hm = np.asarray(h, np.complex128).transpose(2, 0, 1)
        C, _ = combiner(Hm, ns)
        comb.append(apply(C, Hm).transpose(1, 2, 0))                            # [nr, nt, 234]
    out = {}
    for name, est, heard in (('MU', h_list, h_list), ('MUFB', comb, h_list), ('MUC', comb, comb)):
        W, _ = MU.precoder(est, ns, 0.0)
        G = [MU.effective_channel(h, W, ns) for h in heard]
        out[name] = (float(np.mean([MU.sinr_db(g, u, ns, noise_var) for u, g in enumerate(G)])), leakage(G, ns))
    return out
