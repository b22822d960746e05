"""Host restatement of the link simulation (csrc/link_sim.hip.h), numpy only.  Written from the definitions in
that header, not from a device run.  Two parts:

  * fp64: information bits (the device's splitmix64 stream, exact), encoder, Gray QAM mapper, precoder, channel, noise draws (the
    host replay of tr_normal, tests/train_streams.py), zero forcing, max-log soft bits (brute force over the whole constellation),
    EVM and beamforming gain;
  * a Viterbi decoder written twice - float64 and float32 - with the stated operation order and tie rule:
        branch = ((1-2c0) l0 + (1-2c1) l1) + (1-2c2) l2;  new = old + branch;  the larger sum survives, on equal sums the
        predecessor with the lower state number; start and end state 0, no renormalisation.

    key(p, kind) = splitmix64(seed ^ splitmix64(2 p + kind)),  kind 2 = link noise, 3 = information bits
    bit i = splitmix64(key(p, 3) ^ splitmix64(i)) >> 63
    w[n][k][r] = sqrt(noise_var / 2) (normal(key(p, 2), i) + j normal(key(p, 2), i + 1)),  i = ((n 234 + k) Nr + r) 2"""
import numpy as np

import train_streams as ts
from synth_streams import key

N = 234
TAIL = 6
GENERATORS = (0o133, 0o171, 0o165)
KIND_NOISE, KIND_BITS = 2, 3


# ---------------------------------------------------------------------------------------------------- bits and code
def frame_bits(ns, n_sym, bps):
    n_coded = ns * n_sym * N * bps
    return n_coded // 3 - TAIL, n_coded


def info_bits(seed, pkt, n_info):
    k = np.uint64(key(seed, pkt, KIND_BITS))
    h = ts.splitmix64(k ^ ts.splitmix64(np.arange(n_info, dtype=np.uint64)))
    return (h >> np.uint64(63)).astype(np.uint8)


def _parity(x):
    x = np.asarray(x, np.int64)
    p = np.zeros_like(x)
    for i in range(7):
        p ^= (x >> i) & 1
    return p


def encode(bits, terminate=True):
    """rate 1/3, K = 7, (133, 171, 165): state = the last 6 inputs, newest in bit 5; reg = (b << 6) | state.
    uint8 [..., n] -> uint8 [..., 3 (n + 6)] (terminate) or [..., 3 n]"""
    b = np.asarray(bits, np.int64)
    if terminate:
        b = np.concatenate([b, np.zeros(b.shape[:-1] + (TAIL,), np.int64)], -1)
    n = b.shape[-1]
    pad = np.concatenate([np.zeros(b.shape[:-1] + (TAIL,), np.int64), b], -1)
    reg = np.zeros_like(b)
    for d in range(TAIL + 1):                      # bit 6 - d = the input d steps ago
        reg |= pad[..., TAIL - d:TAIL - d + n] << (6 - d)
    out = np.stack([_parity(reg & g) for g in GENERATORS], -1)
    return out.reshape(b.shape[:-1] + (3 * n,)).astype(np.uint8)


def encode_literal(bits):
    """the shift-register loop, one step at a time (no termination)"""
    state, out = 0, []
    for b in bits:
        reg = (int(b) << 6) | state
        out.append([bin(reg & g).count('1') & 1 for g in GENERATORS])
        state = reg >> 1
    return np.array(out, np.uint8)


# ---------------------------------------------------------------------------------------------------- mapper
def pam_level(b):
    """Gray PAM in units of a: 1 bit: 0 -> +1, 1 -> -1;  2 bits: 00 -> +3, 01 -> +1, 11 -> -1, 10 -> -3"""
    b = np.asarray(b)
    if b.shape[-1] == 1:
        return 1.0 - 2.0 * b[..., 0]
    return (1.0 - 2.0 * b[..., 0]) * (3.0 - 2.0 * b[..., 1])


def unit(bps):
    return {2: 1.0 / np.sqrt(2.0), 4: 1.0 / np.sqrt(10.0)}[bps]


def constellation(bps):
    """(points complex128 [2^bps], labels uint8 [2^bps, bps]): the first bps / 2 bits select the in-phase level"""
    lab = ((np.arange(1 << bps)[:, None] >> np.arange(bps - 1, -1, -1)) & 1).astype(np.uint8)
    m = bps // 2
    return unit(bps) * (pam_level(lab[:, :m]) + 1j * pam_level(lab[:, m:])), lab


def map_bits(coded, ns, n_sym, bps):
    """coded bit c = ((s n_sym + n) 234 + k) bps + b  ->  symbols complex128 [ns, n_sym, 234]"""
    c = np.asarray(coded).reshape(ns, n_sym, N, bps)
    m = bps // 2
    return unit(bps) * (pam_level(c[..., :m]) + 1j * pam_level(c[..., m:]))


# ---------------------------------------------------------------------------------------------------- precoder, channel
def precoder(frf_mean, fbb):
    """frf_mean [ntrf, nt], fbb [234, ns, ntrf] -> W complex128 [234, nt, ns] = sqrt(nt) F / |F|_F (0 where F = 0)"""
    F = np.einsum('mj,ksm->kjs', np.asarray(frf_mean, np.complex128), np.asarray(fbb, np.complex128))
    nrm = np.sqrt((np.abs(F) ** 2).sum((1, 2)))
    nt = F.shape[1]
    scale = np.where(nrm > 0, np.sqrt(nt) / np.where(nrm > 0, nrm, 1.0), 0.0)
    return F * scale[:, None, None]


def effective_channel(h, W):
    """h [nr, nt, 234], W [234, nt, ns] -> G [234, nr, ns]"""
    return np.einsum('rjk,kjs->krs', np.asarray(h, np.complex128), W)


def noise_normals(seed, pkt, n_sym, nr):
    """complex128 [n_sym, 234, nr] standard normals per real component"""
    pos = (np.arange(n_sym * N * nr, dtype=np.uint64) * np.uint64(2)).reshape(n_sym, N, nr)
    k = key(seed, pkt, KIND_NOISE)
    re, _ = ts.normal(k, pos)
    im, _ = ts.normal(k, pos + np.uint64(1))
    return re + 1j * im


def dt_snr_db(h, G):
    return 10.0 * np.log10((np.abs(G) ** 2).sum() / (np.abs(np.asarray(h, np.complex128)) ** 2).sum())


# ---------------------------------------------------------------------------------------------------- receiver
def zero_forcing(G, y):
    """G [234, nr, ns], y [n_sym, 234, nr] -> x [ns, n_sym, 234], csi [ns, 234], cond [234]; singular items give x = 0, csi = 0"""
    K, nr, ns = G.shape
    x = np.zeros((ns, y.shape[0], K), np.complex128)
    csi = np.zeros((ns, K))
    cond = np.full(K, np.inf)
    for k in range(K):
        A = np.conj(G[k]).T @ G[k]
        sv = np.linalg.svd(G[k], compute_uv=False)
        if sv[-1] <= 1e-12 * max(sv[0], 1e-300):
            continue
        cond[k] = sv[0] / sv[-1]
        Ai = np.linalg.inv(A)
        x[:, :, k] = Ai @ np.conj(G[k]).T @ y[:, k, :].T
        csi[:, k] = 1.0 / np.real(np.diag(Ai))
    return x, csi, cond


def soft_bits(x, csi, noise_var, bps):
    """max-log: llr = csi / noise_var (min_{b=1} |x - q|^2 - min_{b=0} |x - q|^2), brute force over the constellation.
    x [ns, n_sym, 234], csi [ns, 234] -> llr float64 [ns n_sym 234 bps] in coded-bit order.  noise_var = 0: the factor is csi."""
    q, lab = constellation(bps)
    d2 = np.abs(np.asarray(x, np.complex128)[..., None] - q) ** 2                   # [ns, n_sym, 234, 2^bps]
    out = np.empty(x.shape + (bps,))
    for b in range(bps):
        out[..., b] = d2[..., lab[:, b] == 1].min(-1) - d2[..., lab[:, b] == 0].min(-1)
    scale = csi / noise_var if noise_var > 0 else csi
    return (out * scale[:, None, :, None]).reshape(-1)


def evm_rms(x, bps):
    q, _ = constellation(bps)
    d2 = (np.abs(np.asarray(x, np.complex128)[..., None] - q) ** 2).min(-1)
    return 100.0 * np.sqrt(d2.mean())


def simulate(seed, pkt, h, frf_mean, fbb, noise_var, n_sym, bps):
    """One packet in fp64.  h [nr, nt, 234], frf_mean [ntrf, nt], fbb [234, ns, ntrf].  Returns a dict: bits, coded, d, W, G, clean, w,
    y, x, csi, cond, llr, evm_rms, dt_snr_db."""
    nr = h.shape[0]
    ns = fbb.shape[1]
    n_info, _ = frame_bits(ns, n_sym, bps)
    bits = info_bits(seed, pkt, n_info)
    coded = encode(bits)
    d = map_bits(coded, ns, n_sym, bps)
    W = precoder(frf_mean, fbb)
    G = effective_channel(h, W)
    clean = np.einsum('krs,snk->nkr', G, d)
    w = np.sqrt(noise_var / 2.0) * noise_normals(seed, pkt, n_sym, nr)
    y = clean + w
    x, csi, cond = zero_forcing(G, y)
    return dict(bits=bits, coded=coded, d=d, W=W, G=G, clean=clean, w=w, y=y, x=x, csi=csi, cond=cond,
                llr=soft_bits(x, csi, noise_var, bps), evm_rms=evm_rms(x, bps), dt_snr_db=dt_snr_db(h, G))


# ---------------------------------------------------------------------------------------------------- decoder
def _branch_signs():
    j = np.arange(64)
    reg = ((j >> 5) << 6) | ((j & 31) << 1)                                    # into state j from predecessor 2 (j & 31)
    return [1.0 - 2.0 * _parity(reg & g) for g in GENERATORS], (j & 31) << 1


def viterbi(llr, dtype=np.float64):
    """llr [ncw, 3 n_steps] (or [3 n_steps]) -> uint8 [ncw, n_steps - 6].  All arithmetic in `dtype`."""
    llr = np.asarray(llr)
    one = llr.ndim == 1
    l = np.atleast_2d(llr).astype(dtype)
    ncw, n_steps = l.shape[0], l.shape[1] // 3
    sg, src = _branch_signs()
    s0, s1, s2 = (s.astype(dtype) for s in sg)
    pm = np.full((ncw, 64), -np.inf, dtype)
    pm[:, 0] = 0
    dec = np.empty((n_steps, ncw, 64), bool)
    for t in range(n_steps):
        bm = (s0 * l[:, 3 * t, None] + s1 * l[:, 3 * t + 1, None]) + s2 * l[:, 3 * t + 2, None]
        m0 = pm[:, src] + bm
        m1 = pm[:, src + 1] - bm                                                # all generators end in 1: the other branch is the negative
        dec[t] = m1 > m0
        pm = np.where(dec[t], m1, m0)
        assert pm.dtype == dtype
    st = np.zeros(ncw, np.int64)
    rows = np.arange(ncw)
    out = np.empty((ncw, n_steps), np.uint8)
    for t in range(n_steps - 1, -1, -1):
        out[:, t] = st >> 5
        st = ((st & 31) << 1) | dec[t, rows, st]
    out = out[:, :n_steps - TAIL]
    return out[0] if one else out


def path_metric(llr, bits):
    """fp64 metric sum_c (1 - 2 c) llr_c of the terminated codeword of `bits` ([ncw, n_info] or [n_info])"""
    c = encode(bits).astype(np.float64)
    return ((1.0 - 2.0 * c) * np.asarray(llr, np.float64)).sum(-1)
