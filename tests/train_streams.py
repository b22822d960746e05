"""Host replay of the training step's counter-based random streams (csrc/train.hip.h tr_uniform / tr_normal / glorot_kernel,
csrc/csi_train.hpp tr_stream), numpy only.  Written from the formulas there, not from a device run: the integer part repeats
the device bit for bit (uint64 arithmetic wraps the same way), the fp32 part repeats every operation whose result IEEE-754
fixes (conversion, add, multiply); logf / sqrtf / cosf of the normal draw are evaluated in fp64 instead, so the normal is the
value the device approximates, not the device's own rounding of it.

    stream  = mix(seed + G * (step * 64 + tag + 1) + R * rank)        tr_stream; rank only for the noise / dropout tags
    h       = splitmix64(stream ^ splitmix64(index))
    uniform = (float(h >> 40) + 0.5f) * 2^-24                         dropout (keep when uniform >= p), Glorot
    normal  = sqrt(-2 ln u1) * cos(6.2831855f * u2),  u1 / u2 from the high / low 32 bits of h         input noise

Tags: hidden layer li for its dropout mask, 40 + li for the Glorot kernel of layer li (the regressor is layer n_hidden), 60 for
the input noise.  step is 1 for the first train_step / train_backward after train_begin; Glorot runs at step 0."""
import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
RANK_GOLDEN = 0xD6E8FEB86659FD93
TAG_GLOROT = 40
TAG_NOISE = 60

_U = np.uint64


def _mix(x):
    """finaliser of splitmix64 on uint64 arrays (wrapping multiplies)"""
    with np.errstate(over='ignore'):
        x = (x ^ (x >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U(27))) * _U(0x94D049BB133111EB)
        return x ^ (x >> _U(31))


def splitmix64(x):
    """output of a splitmix64 generator whose state is x (uint64 array or scalar)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over='ignore'):
        return _mix(x + _U(GOLDEN))


def tr_stream(seed, step, tag, rank=0):
    """Stream key of (seed, step, tag).  The rank of a data-parallel fit enters the noise and dropout streams only: the
    initialisation stream (tags 40 ...) is the same on every rank, and rank 0 has the streams of a single process."""
    if TAG_GLOROT <= tag < TAG_NOISE:
        rank = 0
    n = (int(step) * 64 + int(tag) + 1) & MASK64
    x = (int(seed) + GOLDEN * n + RANK_GOLDEN * int(rank)) & MASK64
    return int(_mix(np.asarray(x, dtype=np.uint64)))


def _hash(stream, idx):
    idx = np.asarray(idx, dtype=np.uint64)
    return splitmix64(_U(stream) ^ splitmix64(idx))


def uniform(stream, idx):
    """tr_uniform: fp32 in (0, 1) from the top 24 bits"""
    h = _hash(stream, idx)
    return ((h >> _U(40)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def normal_parts(stream, idx):
    """(u1, angle) of tr_normal as the device holds them in fp32"""
    h = _hash(stream, idx)
    scale = np.float32(2.0 ** -32)
    u1 = ((h >> _U(32)).astype(np.float32) + np.float32(0.5)) * scale
    u2 = ((h & _U(0xFFFFFFFF)).astype(np.float32) + np.float32(0.5)) * scale
    return u1, np.float32(6.283185307179586) * u2


def normal(stream, idx):
    """tr_normal: (value, radius) in fp64 from the device's fp32 u1 and angle; radius = sqrt(-2 ln u1)"""
    u1, ang = normal_parts(stream, idx)
    assert u1.dtype == np.float32 and ang.dtype == np.float32
    radius = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    return radius * np.cos(ang.astype(np.float64)), radius


def dropout_masks(seed, step, B, widths, p, rank=0):
    """Keep masks as oracle.train_forward_backward(masks=) takes them: one bool [B, F] per hidden layer (element (b, j)
    from index b * F + j of the layer's stream), None for the last hidden layer, which has no Dropout behind it."""
    masks = []
    for li, F in enumerate(widths):
        if li == len(widths) - 1:
            masks.append(None)
            continue
        u = uniform(tr_stream(seed, step, li, rank), np.arange(B * F, dtype=np.uint64)).reshape(B, F)
        masks.append(u >= np.float32(p))
    return masks


def input_noise(seed, step, B, kraw, n_noisy, rank=0, with_radius=False):
    """Standard normals [B, kraw] (fp64) the AWGN layer draws for raw element (b, k) (index b * kraw + k); zero on the
    pilot columns k >= n_noisy."""
    z, r = normal(tr_stream(seed, step, TAG_NOISE, rank), np.arange(B * kraw, dtype=np.uint64))
    z, r = z.reshape(B, kraw), r.reshape(B, kraw)
    z[:, n_noisy:] = 0.0
    return (z, r) if with_radius else z


def glorot_limit(fan_in, fan_out):
    return np.sqrt(np.float32(6.0) / np.float32(fan_in + fan_out), dtype=np.float32)


def glorot(seed, li, fan_in, fan_out):
    """Glorot-uniform kernel of layer li in the keras layout [fan_in, fan_out] (fp32): element (k, o) from index
    o * fan_in + k of stream (seed, step 0, tag 40 + li)."""
    u = uniform(tr_stream(seed, 0, TAG_GLOROT + li), np.arange(fan_in * fan_out, dtype=np.uint64))
    w = (np.float32(2.0) * u - np.float32(1.0)) * glorot_limit(fan_in, fan_out)
    return np.ascontiguousarray(w.reshape(fan_out, fan_in).T)
