"""Integer-lattice fixtures of the DNN path: models, pilots and preambles on which no kernel has any rounding to do.

Every operand is a small integer (or a power of two times one), so it is exact in bf16, in hi + lo f16 halves and in fp32, and every
sum of |terms| stays below 2^24, so any order of fp32 accumulation gives the same number.  The device output of every arithmetic mode
and every route must then EQUAL the fp64 oracle; a mismatch is an indexing fact with coordinates, not a rounding budget.

  * BatchNormalization: eps = 2^-10 and moving_variance = 1 - 2^-10, whose sum is exactly 1.0 in fp32 and fp64 (with the keras default
    1e-3 the fp64 oracle itself leaves the lattice); gamma in {+-1, +-2}, beta in [-2, 2], moving_mean in [0, 3]: the folded scale is a
    power of two and the shift an integer, also after the bf16 load-time fold diag(sc) W / b + sh W.
  * layer 0: kernel dense in {-1, 0, 1}; every preamble part has L0_NNZ = 16 non-zeros in {+-1, +-2}.  The count is what bf16 allows:
    h1 feeds four +-2 h1 terms into every h2, h2 must fit bf16's 8 significand bits, so |h1| has to stay near 30 - 16 terms plus the
    Nt pilot terms.  The positions walk the k axis with a stride coprime to it, so the 16 M1 non-zeros of a batch are all at different
    k (complete cover of the 320 Nt preamble columns needs 20 Nt preambles; the builder reports the cover it reaches), and the first
    and the last preamble of a batch hold the first / last column and the first column of the last 64-wide k tile.
  * later layers and regressor, "sparse": max(4, ceil(K / N)) non-zeros of +-1 per output column at rows (n q + j) s mod K, s coprime
    to K - every input row is used (4 per column where 4 N >= K; a [1024, 64] kernel needs 16 to reach every row).
  * "dense" (fp32 contexts only - h2 would need more than 8 bits): +-1 everywhere.
  * biases: integers in [-3, 3].

  * CONV1D models (conv_lattice_case): the same FC stack behind the front end's 64 len_ltf features, which integer samples, taps of +-1 and
    a conv BatchNormalization of the kind above keep on multiples of 1/2 - see the section "CONV1D models" below.

Everything is generated from seeds derived from the shape; there are no golden files.  TEST INFRASTRUCTURE ONLY."""
import functools
import math
import types

import numpy as np

from oracle import csi_oracle as o

BN_EPS = 2.0 ** -10
L0_NNZ = 16
SUM_LIMIT = 2.0 ** 24

# ---------------------------------------------------------------------------------------------------------------- the cases of the GPU module
# (nt, nr, npkt, hidden, n_out, pm1_pilot): shared with test_lattice_host.py, which proves every one of them on the lattice
BF16_TILE_CASES = [(8, 2, 37, (64, 64), 234, False), (4, 2, 70, (96, 40, 24), 234, False), (16, 2, 21, (64,), 234, False),
                   (64, 2, 5, (128, 72), 234, False)]
BF16_BAND_CASES = [(32, 1, 3, (256, 256), 52, False), (32, 4, 5, (256, 512), 234, False), (48, 2, 7, (512, 256), 234, True),
                   (40, 3, 11, (384, 768), 234, True), (8, 2, 37, (256, 256), 234, False)]
BF16_SPLIT_CASES = [(32, 3, 13, (256, 512), 234, False), (64, 4, 1, (1024, 1024), 234, False)]
BF16_L0_STREAM_CASES = [(32, 3, 11, (208, 512), 234, False), (8, 4, 90, (64, 64), 234, False)]
BF16_L0_FUSED_CASES = [(16, 4, 400, (1024, 64), 234, False)]
BF16_CASES = BF16_TILE_CASES + BF16_BAND_CASES + BF16_SPLIT_CASES + BF16_L0_STREAM_CASES + BF16_L0_FUSED_CASES

F32_TILE_CASES = [(4, 2, 70, (64, 48), 234, False), (32, 2, 9, (96, 64), 234, False), (128, 1, 3, (64, 64), 234, False)]
F32_FUSE_REG_CASES = [(8, 2, 70, (64, 256), 234, False)]
F32_BAND_CASES = [(8, 2, 70, (128, 256), 234, False), (16, 2, 41, (128, 256), 234, False)]        # per-lane form / LDS-staged form
F32_BAND_TAIL_CASES = [(16, 2, 2208, (128, 512), 234, False)]
F32_BAND_SPLIT_CASES = [(16, 2, 9, (128, 512), 234, False)]
F32_L0_STREAM_CASES = [(16, 2, 21, (208, 512), 234, False)]
F32_L0_MFMA_CASES = [(8, 2, 70, (64, 48), 234, False), (4, 3, 100, (80, 48), 234, False), (16, 1, 30, (48,), 234, False)]
F32_SMALL_CASES = [(8, 2, 1, (64, 64), 234, False), (12, 2, 3, (40, 24), 234, True)]
F32_GRAPH_CASES = [(16, 4, 200, (128, 64), 234, False)]
POOL_CASES = [(8, 2, 60, (64, 32), 234, False)]                    # decimated-input models ("input_pool" max / avg), bf16 and fp32 contexts
F32_CASES = (F32_TILE_CASES + F32_FUSE_REG_CASES + F32_BAND_CASES + F32_BAND_TAIL_CASES + F32_BAND_SPLIT_CASES + F32_L0_STREAM_CASES
             + F32_L0_MFMA_CASES + F32_SMALL_CASES + F32_GRAPH_CASES)


def case_id(c):
    return 'nt%d-nr%d-p%d-h%s-o%d%s' % (c[0], c[1], c[2], 'x'.join(map(str, c[3])), c[4], '-pm1' if c[5] else '')


# ---------------------------------------------------------------------------------------------------------------- builders
def coprime_stride(k):
    """A stride near 0.618 k that is coprime to k: i -> i s mod k walks all k indices before it repeats."""
    s = max(1, int(k * 0.6180339887))
    while math.gcd(s, k) != 1:
        s += 1
    return s


def sparse_kernel(rng, k, n):
    """[k, n] with max(4, ceil(k / n)) entries of +-1 per column, placed so that every one of the k rows is used."""
    q = min(k, max(4, -(-k // n)))
    rows = (np.arange(n * q, dtype=np.int64) * coprime_stride(k)) % k
    cols = np.repeat(np.arange(n), q)
    w = np.zeros((k, n), dtype=np.float32)
    w[rows, cols] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), n * q)
    return w


def make_model(rng, nt, hidden, n_out, dense, len_in=None):
    w = {'bn_eps': BN_EPS}
    fan = (len_in or 320 * nt) + nt
    for i, h in enumerate(hidden):
        if i == 0:
            w['fc_dense0.kernel'] = rng.integers(-1, 2, (fan, h)).astype(np.float32)
        elif dense:
            w[f'fc_dense{i}.kernel'] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), (fan, h))
        else:
            w[f'fc_dense{i}.kernel'] = sparse_kernel(rng, fan, h)
        w[f'fc_dense{i}.bias'] = rng.integers(-3, 4, h).astype(np.float32)
        w[f'bn{i}.gamma'] = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], dtype=np.float32), h)
        w[f'bn{i}.beta'] = rng.integers(-2, 3, h).astype(np.float32)
        w[f'bn{i}.moving_mean'] = rng.integers(0, 4, h).astype(np.float32)
        w[f'bn{i}.moving_variance'] = np.full(h, 1.0 - BN_EPS, dtype=np.float32)
        fan = h
    w['fc_regressor.kernel'] = (rng.choice(np.array([-1.0, 1.0], dtype=np.float32), (fan, n_out)) if dense
                                else sparse_kernel(rng, fan, n_out))
    w['fc_regressor.bias'] = rng.integers(-3, 4, n_out).astype(np.float32)
    return w


def l0_positions(nt, m1, part):
    """[m1, L0_NNZ] k indices of the non-zeros of preamble part `part` (0 real, 1 imag) of every (packet, rx) preamble."""
    k = 320 * nt
    i = np.arange(m1 * L0_NNZ, dtype=np.int64).reshape(m1, L0_NNZ)
    pos = (i * coprime_stride(k) + part * (k // 2 + 7)) % k
    pos[0, 1] = k - 1 if part == 0 else 0                    # first / last column of the k axis ...
    pos[0, 0] = 0 if part == 0 else k - 1
    pos[-1, 2] = k - 64                                      # ... and the first column of the last 64-wide k tile
    return pos


def make_packets(rng, nt, nr, npkt):
    """complex64 [npkt, nr, 320 nt]: real and imaginary part each with L0_NNZ integers of {+-1, +-2} per preamble."""
    m1, k = npkt * nr, 320 * nt
    planes = []
    for part in (0, 1):
        x = np.zeros((m1, k), dtype=np.float32)
        pos = l0_positions(nt, m1, part)
        x[np.arange(m1)[:, None], pos] = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], dtype=np.float32), pos.shape)
        planes.append(x.reshape(npkt, nr, k))
    return (planes[0] + 1j * planes[1]).astype(np.complex64)


def revive_dead_units(w, x, P):
    """A hidden unit whose relu output is zero in every row of the batch would leave its k index of the next layer untested.  Such a
    unit gets its kernel column negated and its bias made positive (z <= 0 everywhere becomes -(z - b) + max(|b|, 1) > 0): still a column
    of the recipe's alphabet.  x [M1, 320 nt] is the preamble part this model reads; layers are repaired front to back, in place."""
    len_ltf = x.shape[1]
    i = 0
    h = None
    while f'fc_dense{i}.kernel' in w:
        k, b = w[f'fc_dense{i}.kernel'].astype(np.float64), w[f'fc_dense{i}.bias'].astype(np.float64)
        if i == 0:
            z = ((x @ k[:len_ltf])[:, None, :] + (P @ k[len_ltf:] + b)[None, :, :]).reshape(-1, k.shape[1])
        else:
            z = h @ k + b
        dead = ~(z > 0).any(0)
        if dead.any():
            w[f'fc_dense{i}.kernel'][:, dead] *= -1
            w[f'fc_dense{i}.bias'][dead] = np.maximum(np.abs(w[f'fc_dense{i}.bias'][dead]), 1)
            z[:, dead] = -(z[:, dead] - b[dead]) + np.maximum(np.abs(b[dead]), 1)
        sc, sh = bn_fold(w, i)
        h = np.maximum(z, 0.0) * sc + sh
        i += 1


def pool_ltf(ltf, mode):
    """MaxPooling1D / AveragePooling1D (pool 2, stride 2) of each component plane, as tests/test_gpu_input_pool.py states it: on these
    preambles (isolated non-zeros of {+-1, +-2}) the pooled samples are max(v, 0) or v / 2 - multiples of 0.5, exact in every format."""
    def pool(x):
        a, b = x[..., 0::2], x[..., 1::2]
        return np.maximum(a, b) if mode == 'max' else np.float32(0.5) * (a + b)
    return (pool(ltf.real) + 1j * pool(ltf.imag)).astype(np.complex64)


@functools.lru_cache(maxsize=2)
def lattice_case(nt, nr, npkt, hidden, n_out=234, pm1_pilot=False, dense=False, pool=None):
    """The fixture of one shape: namespace with w_re, w_im, P [nt, nt] float64, ltf complex64 [npkt, nr, 320 nt], bn_eps, pool (None / 'max' / 'avg':
    a decimated-input model - layer 0 has 160 nt + nt rows and reads ltf_in, the pooled preambles; without pooling ltf_in is ltf), and
    `cover` = (share of k indices of all layers behind the preamble columns that meet a non-zero activation and a non-zero weight in
    some row - the minimum over layers and models, share of non-zero output elements), both from the fp64 forward `trace`."""
    hidden = tuple(hidden)
    seed = [nt, n_out, int(dense), len(hidden)] + list(hidden) + ([1 + ('max', 'avg').index(pool)] if pool else [])
    rng = np.random.default_rng(seed)
    len_in = 160 * nt if pool else 320 * nt
    w_re = make_model(rng, nt, hidden, n_out, dense, len_in)
    w_im = make_model(rng, nt, hidden, n_out, dense, len_in)
    if pm1_pilot or nt & (nt - 1):
        P = np.random.default_rng([nt, 77]).choice([-1.0, 1.0], (nt, nt))
    else:
        P = o.hadamard(nt)
    ltf = make_packets(np.random.default_rng([nt, nr, npkt]), nt, nr, npkt)
    P = np.asarray(P, dtype=np.float64)
    ltf_in = pool_ltf(ltf, pool) if pool else ltf            # what layer 0 reads: the oracle's input (the engine pools `ltf` itself)
    revive_dead_units(w_re, ltf_in.real.astype(np.float64).reshape(npkt * nr, -1), P)
    revive_dead_units(w_im, ltf_in.imag.astype(np.float64).reshape(npkt * nr, -1), P)
    c = types.SimpleNamespace(nt=nt, nr=nr, npkt=npkt, hidden=hidden, n_out=n_out, dense=dense, bn_eps=BN_EPS, pool=pool, conv=None,
                              w_re=w_re, w_im=w_im, P=np.asarray(P, dtype=np.float64), ltf=ltf, ltf_in=ltf_in)
    c.trace = functools.lru_cache(maxsize=None)(lambda d: trace(c, d))
    c.cover = lambda: (min(c.trace(d).k_cover for d in ('real', 'imag')), min(c.trace(d).nonzero_out for d in ('real', 'imag')))
    return c


# ---------------------------------------------------------------------------------------------------------------- CONV1D models
# The front end (csrc/conv_frontend.hip.h) turns a preamble part x[L] into 64 L features; layer 0 then has K0 = 64 L + nt rows.
#   * cnn1d_1: two taps of +-1 per channel (channel c holds tap c mod 7 and one other, so every tap index is used by ~36 channels), the
#     rest 0; conv_bn: variance 1 - 2^-10 (scale = gamma exactly), gamma in {+-1, +-2}, integer mean.  With integer samples every
#     relu(conv) * scale + shift is an integer and every pooled feature a multiple of 1/2.
#   * 'zero_rest' (both context types): bias in {0, -1}, beta = mean gamma - the folded shift is exactly 0 (the fold is still computed from
#     non-zero statistics), so a feature is non-zero only around a non-zero sample and layer 0's sum stays inside bf16's 8 bits.
#   * 'full' (fp32 contexts): bias in [-2, 2], free beta in [-2, 2] - every one of the 64 L features of every preamble is non-zero.
#   * 'tie' (bf16 contexts, compared with the bf16 emulation): 'zero_rest' with the walked samples raised to +-257 / +-259, whose pooled
#     features 128.5 / 129.5 lie half way between two bf16 numbers - nearest-even, truncation and half-up store three different arrays.
#   * samples: `nnz` integers of {+-1, +-2} per part at walked positions, and pinned ones (CONV_TILE = 128 samples per front-end tile):
#     t in {0, 1, 2, L-3, L-2, L-1} in preambles 0 AND 1 (a halo that reads the neighbouring row meets data where zeros belong), and
#     e-3 ... e+2 around the first and the last interior tile edge e, value +-2, dealt over the preambles with free slots (they reach the
#     neighbouring tile only through its halo; both parities of t, hence both members of a pooled pair, for every tap).
# (nt, nr, npkt, hidden, variant, nnz): shared with test_lattice_host.py, which proves every one of them
CONV_TILE = 128
CONV_F32_SMALL_CASES = [(4, 2, 1, (64,), v, 16) for v in ('zero_rest', 'full')] + [(4, 2, 2, (64,), v, 16) for v in ('zero_rest', 'full')]
CONV_F32_MID_CASES = [(4, 2, 37, (64,), 'zero_rest', 16), (4, 2, 37, (64,), 'full', 16)]          # 74 preambles: 9 ... 256
CONV_F32_STRIDE_CASES = [(4, 2, 110, (64,), 'full', 16)]           # 2200 front-end tiles: more than the 2048 workgroups of a launch
CONV_RANGES_CASES = [(16, 3, 3, (64,), 'zero_rest', 8)]            # K0 = 327680: 256 k ranges of layer 0 (fp32 and bf16 contexts)
CONV_BF16_CASES = [(4, 4, 1, (64,), 'zero_rest', 8), (4, 2, 37, (64,), 'zero_rest', 9), (4, 2, 140, (64,), 'zero_rest', 8)]
CONV_TIE_CASES = [(4, 2, 3, (64,), 'tie', 8)]
CONV_F32_CASES = CONV_F32_SMALL_CASES + CONV_F32_MID_CASES + CONV_F32_STRIDE_CASES + CONV_RANGES_CASES
CONV_CASES = CONV_F32_CASES + [c for c in CONV_BF16_CASES if c not in CONV_F32_CASES]


def conv_id(c):
    return 'conv-nt%d-nr%d-p%d-h%s-%s-nnz%d' % (c[0], c[1], c[2], 'x'.join(map(str, c[3])), c[4], c[5])


def make_conv_front(rng, variant):
    """cnn1d_1.kernel [7, 1, 128] / .bias and conv_bn.* of one component model"""
    ch = np.arange(128)
    j1 = ch % 7
    j2 = (j1 + 1 + (ch // 7) % 6) % 7
    taps = np.zeros((7, 1, 128), dtype=np.float32)
    taps[j1, 0, ch] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), 128)
    taps[j2, 0, ch] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), 128)
    gamma = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], dtype=np.float32), 128)
    mean = rng.integers(0, 4, 128).astype(np.float32)
    if variant == 'full':
        bias, beta = rng.integers(-2, 3, 128).astype(np.float32), rng.integers(-2, 3, 128).astype(np.float32)
    else:
        bias, beta = -(ch % 8 == 7).astype(np.float32), mean * gamma
    return {'cnn1d_1.kernel': taps, 'cnn1d_1.bias': bias, 'conv_bn.gamma': gamma, 'conv_bn.beta': beta, 'conv_bn.moving_mean': mean,
            'conv_bn.moving_variance': np.full(128, 1.0 - BN_EPS, dtype=np.float32)}


def conv_edges(nt):
    """the interior tile edges the pins surround: the first and the last"""
    return (CONV_TILE, 320 * nt - CONV_TILE)


def conv_positions(nt, m1, part, nnz):
    """(pos [m1, nnz] sample indices of the non-zeros of preamble part `part`, pins): pins is a list of (preamble, slot, t, edge) with
    edge = None for the row-end pins; every slot that is not pinned walks the sample axis on a stride coprime to it."""
    L = 320 * nt
    assert m1 >= 2 and nnz >= 6 and m1 * nnz >= 24, 'no room for the pinned samples'
    i = np.arange(m1 * nnz, dtype=np.int64).reshape(m1, nnz)
    pos = (i * coprime_stride(L) + part * (L // 2 + 7)) % L
    pins = []
    for m in (0, 1):
        for s, t in enumerate((0, 1, 2, L - 3, L - 2, L - 1)):
            pos[m, s] = t
            pins.append((m, s, t, None))
    free = [6, 6] + [0] * (m1 - 2)
    order = list(range(2, m1)) + [0, 1]
    at = 0
    for off in range(-3, 3):
        for e in conv_edges(nt):
            while free[order[at % len(order)]] >= nnz:
                at += 1
            m = order[at % len(order)]
            pos[m, free[m]] = e + off
            pins.append((m, free[m], e + off, e))
            free[m] += 1
            at += 1
    return pos, pins


def make_conv_packets(rng, nt, nr, npkt, nnz, tie):
    m1, L = npkt * nr, 320 * nt
    planes = []
    for part in (0, 1):
        pos, pins = conv_positions(nt, m1, part, nnz)
        v = rng.choice(np.array([-2.0, -1.0, -1.0, -1.0, 1.0, 1.0, 1.0, 2.0], dtype=np.float32), pos.shape)      # three +-1 for every +-2
        pinned = np.zeros(pos.shape, dtype=bool)
        for m, s, _, e in pins:
            pinned[m, s] = True
            if e is not None:
                v[m, s] = np.sign(v[m, s]) * 2              # also a channel of bias -1 answers a +-2
        if tie:
            v = np.where(pinned, v, np.sign(v) * np.where(np.abs(v) == 1, 257.0, 259.0)).astype(np.float32)
        x = np.zeros((m1, L), dtype=np.float32)
        x[np.arange(m1)[:, None], pos] = v
        for m, s, t, _ in pins:                                 # (a walked slot of the same preamble may fall on a pinned sample)
            x[m, t] = v[m, s]
        planes.append(x.reshape(npkt, nr, L))
    return (planes[0] + 1j * planes[1]).astype(np.complex64)


def conv_fold(w):
    """(scale, shift) of conv_bn in fp64, as csi_load_weights folds it"""
    sc = w['conv_bn.gamma'].astype(np.float64) / np.sqrt(w['conv_bn.moving_variance'].astype(np.float64) + float(w['bn_eps']))
    return sc, w['conv_bn.beta'].astype(np.float64) - w['conv_bn.moving_mean'].astype(np.float64) * sc


def conv_features(x, w, rows_per_pass=32):
    """fp64 statement of the front end: x [rows, L] -> [rows, 64 L].  conv[t, c] = b[c] + sum_j K[j, c] x[t + j - 3] (zeros outside the row),
    q = relu(conv) scale + shift, f[u 128 + c] = (q[2u, c] + q[2u + 1, c]) / 2."""
    x = np.asarray(x, dtype=np.float64)
    rows, L = x.shape
    k = w['cnn1d_1.kernel'].astype(np.float64).reshape(7, 128)
    b = w['cnn1d_1.bias'].astype(np.float64)
    sc, sh = conv_fold(w)
    out = np.empty((rows, 64 * L))
    for r0 in range(0, rows, rows_per_pass):
        xp = np.pad(x[r0:r0 + rows_per_pass], ((0, 0), (3, 3)))
        win = np.lib.stride_tricks.sliding_window_view(xp, 7, axis=1)              # [rows, L, 7]: x[t - 3 .. t + 3]
        q = np.maximum(win @ k + b, 0.0) * sc + sh
        out[r0:r0 + rows_per_pass] = (0.5 * (q[:, 0::2] + q[:, 1::2])).reshape(len(xp), 64 * L)
    return out


def conv_rest(w):
    """[128] the feature of channel c where no sample is in reach: relu(b) scale + shift"""
    sc, sh = conv_fold(w)
    return np.maximum(w['cnn1d_1.bias'].astype(np.float64), 0.0) * sc + sh


def conv_feat_want(c, d):
    """The feature columns the samples of the batch move, derived from the sample list alone (no dense forward): every (sample, channel,
    tap) term is summed into its conv output by key, the change of relu(conv) scale against the rest value is summed into its pooled
    position, and a column counts where that sum is non-zero in some preamble and layer 0 holds a non-zero weight for it."""
    w = c.w_re if d == 'real' else c.w_im
    L, m1 = 320 * c.nt, c.npkt * c.nr
    x = (c.ltf.real if d == 'real' else c.ltf.imag).reshape(m1, L)
    m, t = np.nonzero(x)
    v = x[m, t].astype(np.float64)
    k = w['cnn1d_1.kernel'].astype(np.float64).reshape(7, 128)
    j, ch = np.nonzero(k)
    to = t[:, None] + 3 - j[None, :]                                              # the output sample tap j of a sample at t lands in
    ok = (to >= 0) & (to < L)
    key = ((m[:, None] * L + to) * 128 + ch[None, :])[ok]
    term = (v[:, None] * k[j, ch][None, :])[ok]
    key, inv = np.unique(key, return_inverse=True)
    s = np.zeros(len(key))
    np.add.at(s, inv.ravel(), term)
    chk = key % 128
    b, (sc, _) = w['cnn1d_1.bias'].astype(np.float64), conv_fold(w)
    dq = (np.maximum(b[chk] + s, 0.0) - np.maximum(b[chk], 0.0)) * sc[chk]
    mt = key // 128                                                                # m L + t
    key2 = ((mt // L) * (L // 2) + (mt % L) // 2) * 128 + chk
    key2, inv2 = np.unique(key2, return_inverse=True)
    s2 = np.zeros(len(key2))
    np.add.at(s2, inv2.ravel(), dq)
    col = np.unique(key2[s2 != 0] % (64 * L))
    used = np.abs(w['fc_dense0.kernel'][:64 * L]).sum(1) > 0
    return float(np.count_nonzero(used[col])) / (64 * L)


def conv_feat_cover(c, d):
    """measured on the features layer 0 reads: share of columns that differ from their channel's rest value in some preamble and meet a weight"""
    w = c.w_re if d == 'real' else c.w_im
    f = (c.ltf_in.real if d == 'real' else c.ltf_in.imag).reshape(c.npkt * c.nr, -1)
    moved = (f != np.tile(conv_rest(w), f.shape[1] // 128).astype(np.float32)).any(0)
    return float(np.mean(moved & (np.abs(w['fc_dense0.kernel'][:f.shape[1]]).sum(1) > 0)))


@functools.lru_cache(maxsize=2)
def conv_lattice_case(nt, nr, npkt, hidden, variant='zero_rest', nnz=16, n_out=234):
    """The fixture of one CONV1D shape: the namespace of lattice_case, with w_re / w_im carrying cnn1d_1.* and conv_bn.* as well, ltf the raw
    preambles the engine gets, ltf_in complex64 [npkt, nr, 64 * 320 nt] the features layer 0 reads (conv_features of each part through its
    own model: the oracle's input), conv = the variant, pins[part] = the pinned samples, feat_cover() = the minimum over both models."""
    hidden = tuple(hidden)
    vi = ('zero_rest', 'full', 'tie').index(variant)
    rng = np.random.default_rng([nt, n_out, len(hidden)] + list(hidden) + [7, vi])
    L = 320 * nt
    ws = []
    for _ in range(2):
        w = make_model(rng, nt, hidden, n_out, False, 64 * L)
        w.update(make_conv_front(rng, variant))
        ws.append(w)
    w_re, w_im = ws
    P = np.asarray(o.hadamard(nt), dtype=np.float64)
    ltf = make_conv_packets(np.random.default_rng([nt, nr, npkt, nnz, 11]), nt, nr, npkt, nnz, variant == 'tie')
    f_re = conv_features(ltf.real.reshape(npkt * nr, L), w_re)
    f_im = conv_features(ltf.imag.reshape(npkt * nr, L), w_im)
    revive_dead_units(w_re, f_re, P)
    revive_dead_units(w_im, f_im, P)
    ltf_in = np.empty((npkt, nr, 64 * L), dtype=np.complex64)
    ltf_in.real, ltf_in.imag = f_re.reshape(ltf_in.shape), f_im.reshape(ltf_in.shape)
    assert np.array_equal(ltf_in.real.reshape(f_re.shape), f_re) and np.array_equal(ltf_in.imag.reshape(f_im.shape), f_im)     # exact as float32
    c = types.SimpleNamespace(nt=nt, nr=nr, npkt=npkt, hidden=hidden, n_out=n_out, dense=False, bn_eps=BN_EPS, pool=None, conv=variant, nnz=nnz,
                              w_re=w_re, w_im=w_im, P=P, ltf=ltf, ltf_in=ltf_in,
                              pins=[conv_positions(nt, npkt * nr, part, nnz)[1] for part in (0, 1)])
    c.trace = functools.lru_cache(maxsize=None)(lambda d: trace(c, d))
    c.cover = lambda: (min(c.trace(d).k_cover for d in ('real', 'imag')), min(c.trace(d).nonzero_out for d in ('real', 'imag')))
    c.feat_cover = lambda: min(conv_feat_cover(c, d) for d in ('real', 'imag'))
    return c


def bn_fold(w, i):
    """(scale, shift) of BatchNormalization i in fp64."""
    inv = w[f'bn{i}.gamma'].astype(np.float64) / np.sqrt(w[f'bn{i}.moving_variance'].astype(np.float64) + float(w['bn_eps']))
    return inv, w[f'bn{i}.beta'].astype(np.float64) - w[f'bn{i}.moving_mean'].astype(np.float64) * inv


def trace(c, d):
    """fp64 forward of one component model over the whole batch (layer 0 shared across the Nt pairs of a preamble, as
    oracle.predict_packets_shared) that keeps what the host tests assert: out [npkt, nr, nt, n_out]; k_cover (see lattice_case);
    l0_cover = share of the 320 Nt preamble columns that hold a non-zero sample in some preamble and a non-zero weight; l0_want = the
    share 16 M1 distinct positions can reach; max_abs_sum = max over layers and outputs of sum |a| |w|; act_bf16_exact = every relu
    output equals its bf16 rounding; max_in / max_act = largest |preamble sample| / |layer input behind layer 0| (split-f16 range)."""
    w = c.w_re if d == 'real' else c.w_im
    k0 = w['fc_dense0.kernel'].astype(np.float64)
    len_ltf = c.ltf_in.shape[-1]
    x = (c.ltf_in.real if d == 'real' else c.ltf_in.imag).astype(np.float64).reshape(c.npkt * c.nr, len_ltf)
    t = types.SimpleNamespace()
    row_used = np.abs(k0).sum(1) > 0
    t.l0_cover = float(np.mean((np.abs(x).sum(0) > 0) & row_used[:len_ltf]))
    plain = not c.pool and not getattr(c, 'conv', None)          # (pooled and CONV1D models: layer 0 reads features, not the walked samples)
    t.l0_want = min(1.0, np.unique(l0_positions(c.nt, c.npkt * c.nr, 0 if d == 'real' else 1)).size / len_ltf) if plain else None
    covers = [float(np.mean((np.abs(c.P).sum(0) > 0) & row_used[len_ltf:]))]
    abs_sum = [float((np.abs(x) @ np.abs(k0[:len_ltf])).max() + (np.abs(c.P) @ np.abs(k0[len_ltf:])).max())]
    z = (x @ k0[:len_ltf])[:, None, :] + (c.P @ k0[len_ltf:] + w['fc_dense0.bias'].astype(np.float64))[None, :, :]
    h = np.maximum(z, 0.0).reshape(c.npkt * c.nr * c.nt, -1)
    t.act_bf16_exact = bool(np.array_equal(h, o.bf16_round(h).astype(np.float64)))
    t.max_in, t.max_act = float(np.abs(x).max()), 0.0
    i = 0
    while True:
        sc, sh = bn_fold(w, i)
        a = h * sc + sh
        i += 1
        name = f'fc_dense{i}' if f'fc_dense{i}.kernel' in w else 'fc_regressor'
        k = w[name + '.kernel'].astype(np.float64)
        covers.append(float(np.mean((np.abs(h).sum(0) > 0) & (np.abs(k).sum(1) > 0))))      # the bare relu output: what bf16 contexts multiply
        abs_sum.append(float((np.abs(a) @ np.abs(k)).max()))
        t.max_act = max(t.max_act, float(np.abs(a).max()), float(np.abs(h).max()))
        z = a @ k + w[name + '.bias'].astype(np.float64)
        if name == 'fc_regressor':
            break
        h = np.maximum(z, 0.0)
        t.act_bf16_exact = t.act_bf16_exact and bool(np.array_equal(h, o.bf16_round(h).astype(np.float64)))
    t.out = z.reshape(c.npkt, c.nr, c.nt, -1)
    t.k_cover = min(covers)
    t.max_abs_sum = max(abs_sum)
    t.nonzero_out = float(np.mean(t.out != 0))
    return t


# ---------------------------------------------------------------------------------------------------------------- mutable emulation
def bf16_truncate(x):
    a = np.ascontiguousarray(x, dtype=np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).reshape(a.shape)


def forward_bf16_hooked(x, w, h1_hook=None, round_h1=o.bf16_round):
    """oracle.fc_forward_bf16 with two places to break it: `h1_hook` maps the rounded h1 [rows, h1] to what the next layer reads (a
    row swap), `round_h1` replaces the rounding of h1 (truncation).  With neither it equals the oracle (asserted by the host tests)."""
    h = o.bf16_round(x).astype(np.float64)
    sc = sh = None
    i = 0
    while True:
        name = f'fc_dense{i}' if f'fc_dense{i}.kernel' in w else 'fc_regressor'
        k = w[name + '.kernel'].astype(np.float64)
        b = w[name + '.bias'].astype(np.float64)
        if sc is not None:
            b = b + sh @ k
            k = k * sc[:, None]
        z = h @ o.bf16_round(k.astype(np.float32)).astype(np.float64) + b.astype(np.float32).astype(np.float64)
        if name == 'fc_regressor':
            return z.astype(np.float32)
        z = np.maximum(z.astype(np.float32), np.float32(0))
        inv = (np.float32(1) / np.sqrt(w[f'bn{i}.moving_variance'].astype(np.float32) + np.float32(w['bn_eps']))) * w[f'bn{i}.gamma'].astype(np.float32)
        sc = inv.astype(np.float64)
        sh = (w[f'bn{i}.beta'].astype(np.float32) - w[f'bn{i}.moving_mean'].astype(np.float32) * inv).astype(np.float64)
        h = (round_h1 if i == 0 else o.bf16_round)(z).astype(np.float64)
        if i == 0 and h1_hook is not None:
            h = h1_hook(h)
        i += 1


def bf16_half_up(x):
    """round half away from zero on the magnitude bits: what `u + 0x8000` in place of the nearest-even increment stores"""
    a = np.ascontiguousarray(x, dtype=np.float32)
    return ((a.view(np.uint32).astype(np.uint64) + 0x8000) & 0xFFFF0000).astype(np.uint32).view(np.float32).reshape(a.shape)


CONV_MUTANTS = ('halo_from_neighbouring_row', 'halo_zero_at_tile_edges', 'taps_reversed', 'pool_pairs_shifted', 'channels_first',
                'bn_before_relu', 'other_model', 'lane_groups_of_4_swapped', 'lane_groups_of_8_swapped', 'position_dropped_at_tile_end')


def frontend_f32(x, w, mutant=None, other=None):
    """The front end in float32 in the operation order of conv_frontend_kernel: x [rows, L] -> [rows, 64 L] float32.  e / o start at the bias
    and take the taps j = 0 .. 6 in turn (fma: exact products here), q = fma(relu, scale, shift) with the constants folded in double and
    stored as float32, f = 0.5 (qe + qo).  `mutant` (one of CONV_MUTANTS) breaks it the way a kernel port would; `other` = the weights of
    the other component model, which 'other_model' takes its constants from.  Tiles of CONV_TILE samples as the kernel cuts them."""
    f32 = np.float32
    x = np.ascontiguousarray(x, dtype=f32)
    rows, L = x.shape
    src = other if mutant == 'other_model' else w
    k = src['cnn1d_1.kernel'].astype(f32).reshape(7, 128)
    if mutant == 'taps_reversed':
        k = k[::-1]
    b = src['cnn1d_1.bias'].astype(f32)
    sc, sh = (v.astype(f32) for v in conv_fold(src))
    if mutant == 'halo_from_neighbouring_row':                     # x[r L + t] for t outside [0, L): the neighbouring rows, zeros only around the plane
        flat = np.concatenate([np.zeros(3, f32), x.ravel(), np.zeros(3, f32)])
        xp = np.lib.stride_tricks.sliding_window_view(flat, L + 6)[::L]
    elif mutant == 'halo_zero_at_tile_edges':                      # every tile sees zeros beyond its own samples
        xp = np.pad(x.reshape(rows * (L // CONV_TILE), CONV_TILE), ((0, 0), (3, 3)))
    else:
        xp = np.pad(x, ((0, 0), (3, 3)))
    n, T = xp.shape[0], xp.shape[1] - 6
    acc = np.broadcast_to(b, (n, T, 128)).astype(f32)
    for j in range(7):
        acc = xp[:, j:j + T, None] * k[j] + acc
    acc = acc.reshape(rows, L, 128)
    if mutant == 'bn_before_relu':
        q = np.maximum(acc * sc + sh, f32(0))
    else:
        q = np.maximum(acc, f32(0)) * sc + sh
    if mutant == 'pool_pairs_shifted':                             # (q[2u - 1], q[2u])
        q = np.roll(q, 1, axis=1)
    f = f32(0.5) * (q[:, 0::2] + q[:, 1::2])                       # [rows, L / 2, 128]
    if mutant == 'lane_groups_of_4_swapped':
        f = f.copy()
        f[..., 0:4], f[..., 4:8] = f[..., 4:8].copy(), f[..., 0:4].copy()
    if mutant == 'lane_groups_of_8_swapped':
        f = f.copy()
        f[..., 0:8], f[..., 8:16] = f[..., 8:16].copy(), f[..., 0:8].copy()
    if mutant == 'position_dropped_at_tile_end':                   # the last pooled position of the first tile is never written
        f = f.copy()
        f[:, CONV_TILE // 2 - 1] = 0
    if mutant == 'channels_first':
        f = f.transpose(0, 2, 1)
    return np.ascontiguousarray(f).reshape(rows, 64 * L)


def forward_shared(x, P, w):
    """fp64 forward of one component model from its layer-0 inputs x [M1, K0] (layer 0 shared across the Nt pairs): [M1 nt, n_out]"""
    k0 = w['fc_dense0.kernel'].astype(np.float64)
    K0 = x.shape[1]
    z = (np.asarray(x, np.float64) @ k0[:K0])[:, None, :] + (P @ k0[K0:] + w['fc_dense0.bias'].astype(np.float64))[None, :, :]
    h = np.maximum(z, 0.0).reshape(-1, k0.shape[1])
    i = 0
    while True:
        sc, sh = bn_fold(w, i)
        a = h * sc + sh
        i += 1
        name = f'fc_dense{i}' if f'fc_dense{i}.kernel' in w else 'fc_regressor'
        z = a @ w[name + '.kernel'].astype(np.float64) + w[name + '.bias'].astype(np.float64)
        if name == 'fc_regressor':
            return z
        h = np.maximum(z, 0.0)
