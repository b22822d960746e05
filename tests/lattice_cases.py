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
    c =types.SimpleNamespace(nt=nt, nr=nr, npkt=npkt, hidden=hidden, n_out=n_out, dense=dense, bn_eps=BN_EPS, pool=pool,
                              w_re=w_re, w_im=w_im, P=np.asarray(P, dtype=np.float64), ltf=ltf, ltf_in=ltf_in)
    c.trace = functools.lru_cache(maxsize=None)(lambda d: trace(c, d))
    c.cover = lambda: (min(c.trace(d).k_cover for d in ('real', 'imag')), min(c.trace(d).nonzero_out for d in ('real', 'imag')))
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
    t.l0_want = min(1.0, np.unique(l0_positions(c.nt, c.npkt * c.nr, 0 if d == 'real' else 1)).size / len_ltf) if not c.pool else None
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
