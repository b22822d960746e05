"""The random side of the training step (GaussianNoise, Dropout, Glorot initialisation; csrc/train.hip.h, csrc/csi_train.hpp).

The generator is counter-based, so nothing here is statistical on the device: tests/train_streams.py replays the streams on the
host, the CPU tests establish on the replay that the design draws what it should (N(0,1) noise, keep rate 1 - p, U(-l, l)
kernels, streams that do not repeat over rows / steps / layers / ranks), and the GPU tests hold the device to the replay: the
staged noise element by element, the whole stochastic step against the fp64 oracle fed with the replayed noise and masks.

No tolerance below comes from a device run: each is bit-equality, an ulp bound derived from the operations involved, a
|z| < 4 rule whose inputs are fixed (seeds) and were checked on the CPU, or a tolerance tests/test_train.py already uses for
the deterministic step (the noise and the masks are inputs of the step, they add no arithmetic of their own)."""
import math
import os
import struct
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_streams as ts      # noqa: E402

STREAM_PAIRS = [(77, 1), (1, 1), (1, 2), (0, 3)]          # (seed, step) whose replayed statistics were checked to satisfy |z| < 4
Z_MAX = 4.0                                                # two-sided normal tail 6e-5 per statistic
B_STAT, K_STAT = 256, 1284                                 # the reference's batch, nt = 4


# ------------------------------------------------------------------------------------ second, scalar statement (python int)
M64 = 2 ** 64 - 1


def _sm_int(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _stream_int(seed, step, tag, rank=0):
    x = (seed + 0x9E3779B97F4A7C15 * (step * 64 + tag + 1) + (0 if 40 <= tag < 60 else 0xD6E8FEB86659FD93 * rank)) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _f32(v):
    """round a python float (double) to fp32"""
    return struct.unpack('f', struct.pack('f', v))[0]


def _uniform_int(stream, i):
    h = _sm_int(stream ^ _sm_int(i))
    return _f32((h >> 40) + 0.5) * 2.0 ** -24          # the sum is exact in double, then rounded once to fp32; the scaling is exact


def _normal_int(stream, i):
    h = _sm_int(stream ^ _sm_int(i))
    u1 = _f32(_f32(float(h >> 32)) + 0.5) * 2.0 ** -32
    u2 = _f32(_f32(float(h & 0xFFFFFFFF)) + 0.5) * 2.0 ** -32
    ang = _f32(_f32(6.283185307179586) * u2)            # the product of two fp32 is exact in double, then rounded once
    r = math.sqrt(-2.0 * math.log(u1))
    return r * math.cos(ang), r


def _z_corr(a, b):
    """z-score of the sample correlation of two (nominally independent, zero-mean-after-centering) arrays"""
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    a = (a - a.mean()) / a.std()
    b = (b - b.mean()) / b.std()
    return float(np.mean(a * b) * np.sqrt(a.size))


# ------------------------------------------------------------------------------------ CPU: the replay itself
def test_replay_known_answers():
    """splitmix64 against its published first output; stream keys, hashes, uniforms and normals of one (seed, step, tag) as
    literals, and the vectorised numpy statement against the scalar python-int statement."""
    assert int(ts.splitmix64(0)) == 0xE220A8397B1DCDAF == _sm_int(0)
    assert int(ts.splitmix64(M64)) == _sm_int(M64)                       # wraps
    keys = {(77, 1, 60): 0x5E94F04465EE1B2E, (77, 1, 0): 0x8683FF169C0B59F5, (1, 2, 1): 0x528F9E0312CACFF8,
            (77, 0, 41): 0x0CEF5D9ED47684CA, (M64, 3, 60): 0x3408ED1386E775FD}
    for args, key in keys.items():
        assert ts.tr_stream(*args) == key == _stream_int(*args), args
    # rank: noise / dropout keys move, the initialisation key does not, rank 0 is the single-process key
    assert ts.tr_stream(77, 1, 60, rank=0) == keys[(77, 1, 60)]
    assert ts.tr_stream(77, 1, 60, rank=1) == 0xCEF0D0DFD57507B0 == _stream_int(77, 1, 60, 1)
    assert ts.tr_stream(77, 1, 0, rank=3) == _stream_int(77, 1, 0, 3) != keys[(77, 1, 0)]
    assert ts.tr_stream(77, 0, 41, rank=1) == keys[(77, 0, 41)]
    s = keys[(77, 1, 60)]
    assert [_sm_int(s ^ _sm_int(i)) for i in range(4)] == [0xCE9D29C6B9E2B2DF, 0xBB17F09684424DF2, 0x7E340200C66FD08D, 0xA9E79ED2409565BF]
    u = ts.uniform(s, np.arange(4))
    assert u.dtype == np.float32
    assert [float(v) for v in u] == [0.8070856332778931, 0.7308340072631836, 0.49298110604286194, 0.663690447807312]
    z, r = ts.normal(s, np.arange(4))
    np.testing.assert_allclose(z, [-0.09788535226247752, -0.7875975665081328, 0.18711672585044148, -0.012968877168578752], rtol=1e-13)
    np.testing.assert_allclose(r, [0.6547144465094865, 0.7919202481417053, 1.1893565408100248, 0.9054715251854757], rtol=1e-13)
    # vectorised against scalar over a longer run and large indices (the last rows of a 300 x 2568 batch and beyond 2^32)
    idx = np.concatenate([np.arange(300), 770000 + np.arange(100), (1 << 33) + np.arange(50)]).astype(np.uint64)
    for key in keys.values():
        u = ts.uniform(key, idx)
        z, r = ts.normal(key, idx)
        for n, i in enumerate(idx.tolist()):
            assert float(u[n]) == _uniform_int(key, i)
            zi, ri = _normal_int(key, i)
            assert abs(z[n] - zi) <= 1e-14 * max(1.0, abs(zi)) and abs(r[n] - ri) <= 1e-14 * ri
    # layouts
    assert np.array_equal(ts.dropout_masks(77, 1, 5, (7, 3), 0.5)[0][3], ts.uniform(keys[(77, 1, 0)], 21 + np.arange(7)) >= np.float32(0.5))
    m3 = ts.dropout_masks(77, 1, 5, (7, 6, 3), 0.5)
    assert m3[2] is None and m3[1].shape == (5, 6) and m3[0].shape == (5, 7)
    zn = ts.input_noise(77, 1, 3, 8, 6)
    assert np.all(zn[:, 6:] == 0.0) and zn[2, 5] == ts.normal(s, np.array([21]))[0][0]
    g = ts.glorot(77, 1, 5, 3)
    lim = float(ts.glorot_limit(5, 3))
    assert g.shape == (5, 3) and g.dtype == np.float32 and lim == _f32(math.sqrt(_f32(6.0 / 8.0)))
    for k, o in ((0, 0), (4, 0), (1, 2), (4, 2)):
        assert float(g[k, o]) == _f32((2.0 * _uniform_int(keys[(77, 0, 41)], o * 5 + k) - 1.0) * lim), (k, o)


@pytest.mark.parametrize('seed,step', STREAM_PAIRS)
def test_replayed_streams_are_what_the_layers_should_draw(seed, step):
    """The design, on the host: the input noise is N(0,1) (mean, variance, fourth moment), uncorrelated along rows and columns;
    dropout keeps 1 - p of the units and drops none in every row; the streams of two steps, two layers, two ranks, and the
    noise and the mask of one step are uncorrelated.  |z| < 4 for every statistic."""
    stats = {}
    z, radius = ts.input_noise(seed, step, B_STAT, K_STAT, K_STAT, with_radius=True)
    n = z.size
    stats['mean'] = z.mean() * np.sqrt(n)
    stats['variance'] = (np.mean(z ** 2) - 1.0) / np.sqrt(2.0 / n)                  # var(z^2) = 2
    stats['fourth moment'] = (np.mean(z ** 4) - 3.0) / np.sqrt(96.0 / n)            # var(z^4) = 105 - 9
    stats['lag 1 along rows'] = np.mean(z[:, 1:] * z[:, :-1]) * np.sqrt(z[:, 1:].size)
    stats['lag 1 along columns'] = np.mean(z[1:] * z[:-1]) * np.sqrt(z[1:].size)
    stats['lag 32 along rows'] = np.mean(z[:, 32:] * z[:, :-32]) * np.sqrt(z[:, 32:].size)
    # a normal, not something else with two right moments: 330k samples reach beyond 4 sigma and stay below 6
    assert 4.0 < np.abs(z).max() < 6.0
    u1, _ = ts.normal_parts(ts.tr_stream(seed, step, ts.TAG_NOISE), np.arange(n, dtype=np.uint64))
    assert 0.0 < u1.min() < 1e-4 and 0.9999 < u1.max() <= 1.0 and np.isfinite(radius).all()
    stats['noise of two steps'] = _z_corr(z, ts.input_noise(seed, step + 1, B_STAT, K_STAT, K_STAT))
    stats['noise of two ranks'] = _z_corr(z, ts.input_noise(seed, step, B_STAT, K_STAT, K_STAT, rank=1))
    for F, p in ((96, 0.5), (100, 0.15), (1024, 0.15)):
        m0, m1, _ = ts.dropout_masks(seed, step, B_STAT, (F, F, 8), p)
        stats[f'keep rate F={F} p={p}'] = (m0.mean() - (1.0 - p)) / np.sqrt(p * (1.0 - p) / m0.size)
        assert not (~m0).all(axis=0).any() and not m0.all(axis=0).any()            # no unit dropped (or kept) in all 256 rows
        assert not (m0 == m0[0]).all() and not np.array_equal(m0[:, :32], m0[:, 32:64])     # not one mask for every row, no period 32
        stats[f'mask lag 1 along rows F={F}'] = _z_corr(m0[:, 1:], m0[:, :-1])
        stats[f'mask lag 1 along columns F={F}'] = _z_corr(m0[1:], m0[:-1])
        stats[f'masks of two layers F={F}'] = _z_corr(m0, m1)
        stats[f'masks of two steps F={F}'] = _z_corr(m0, ts.dropout_masks(seed, step + 1, B_STAT, (F, 8), p)[0])
        stats[f'masks of two ranks F={F}'] = _z_corr(m0, ts.dropout_masks(seed, step, B_STAT, (F, 8), p, rank=1)[0])
        stats[f'noise and mask F={F}'] = _z_corr(z[:, :F], m0)
    print({k: round(float(v), 2) for k, v in stats.items()})
    bad = {k: float(v) for k, v in stats.items() if not abs(v) < Z_MAX}
    assert not bad, bad


@pytest.mark.parametrize('seed', [77, 1, 0])
def test_replayed_glorot_is_uniform_in_the_keras_limit(seed):
    """U(-l, l), l = sqrt(6 / (fan_in + fan_out)): mean, variance l^2 / 3, the limit itself, no correlation between the kernels
    of two layers of one seed nor between a kernel and its transpose-indexed self (fan-in / fan-out swapped)."""
    fan_in, fan_out = 1284, 96
    w0, w1 = ts.glorot(seed, 0, fan_in, fan_out).astype(np.float64), ts.glorot(seed, 1, fan_in, fan_out).astype(np.float64)
    lim = float(ts.glorot_limit(fan_in, fan_out))
    assert abs(lim - math.sqrt(6.0 / (fan_in + fan_out))) < 1e-7 * lim
    n = w0.size
    stats = {'mean': w0.mean() / (lim / np.sqrt(3.0)) * np.sqrt(n),
             'variance': (np.mean(w0 ** 2) - lim ** 2 / 3.0) / (lim ** 2 * np.sqrt(4.0 / 45.0 / n)),      # var(w^2) = l^4 (1/5 - 1/9)
             'two layers': _z_corr(w0, w1),
             'lag 1 along fan-in': _z_corr(w0[1:], w0[:-1]), 'lag 1 along fan-out': _z_corr(w0[:, 1:], w0[:, :-1])}
    assert np.abs(w0).max() <= lim and np.abs(w0).max() > 0.999 * lim
    assert not np.array_equal(ts.glorot(seed, 0, fan_in, fan_out), ts.glorot(seed + 1, 0, fan_in, fan_out))
    print({k: round(float(v), 2) for k, v in stats.items()})
    bad = {k: float(v) for k, v in stats.items() if not abs(v) < Z_MAX}
    assert not bad, bad


def test_fit_hands_the_rank_to_the_engine(pkg, monkeypatch):
    """trainer.fit(data_parallel=True) sets 'train_rank' from the process group before the trainer exists; a single-process
    fit does not touch the option (rank 0 is the default of a context)."""
    calls = []

    class Engine:
        def set_option(self, name, value):
            calls.append(('set_option', name, value))

        def train_begin(self, model, **kw):
            calls.append(('train_begin',))

        def train_backward(self, model, rows, y, noise_std=0.0):
            return 1.0

        train_step = train_backward

        def synchronize(self):
            pass

        def train_grads(self, model):
            return 0, 0

        def train_apply(self, model):
            pass

        def train_eval(self, model, rows, y):
            return 1.0

        def train_weights(self, model):
            return {}

        def train_end(self, model, commit=True):
            pass

    d = pkg.trainer.dist
    assert d.rank() == 0                                     # no process group: a single process is rank 0
    monkeypatch.setattr(d, 'rank', lambda: 3)
    monkeypatch.setattr(d, 'world_size', lambda: 4)
    monkeypatch.setattr(d, 'all_reduce_device', lambda ptr, count, average=True: None)
    monkeypatch.setattr(d, 'all_reduce_sum', lambda v, device=None: 4 * v)
    monkeypatch.setattr(d, 'all_reduce_mean_arrays', lambda a: a)
    gen = [([np.zeros((4, 8), np.float32), np.zeros((4, 2), np.float32)], np.zeros((4, 3), np.float32), None)]
    pkg.trainer.fit(Engine(), 'real', gen, gen, epochs=1, method='default', verbose=False, commit=False, data_parallel=True)
    assert calls[:2] == [('set_option', 'train_rank', 3), ('train_begin',)]
    del calls[:]
    pkg.trainer.fit(Engine(), 'real', gen, gen, epochs=1, method='default', verbose=False, commit=False)
    assert calls == [('train_begin',)]


# ------------------------------------------------------------------------------------ shared pieces of the step comparisons
NOISE_STD = 0.3
# nt, hidden, B, use_bn, dropout
STEP_CASES = [(4, (96, 40), 64, True, 0.15), (4, (100, 72, 24), 33, True, 0.5), (4, (100, 72, 24), 256, False, 0.15),
              (8, (128, 128), 256, True, 0.5), (4, (96, 40), 300, False, 0.5)]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _problem(oracle, rng, nt, hidden, B, use_bn=True):
    d_in = 321 * nt
    w = oracle.make_weights(rng, d_in, hidden, 234, use_bn=use_bn)
    x = rng.standard_normal((B, d_in)).astype(np.float32)
    y = rng.standard_normal((B, 234)).astype(np.float32)
    return w, x, y


def _replayed_inputs(seed, step, B, nt, hidden, p, noise_std, rank=0):
    """noise= and masks= of the oracle for the step the device numbers `step`"""
    std = float(np.float32(noise_std))                       # the C-ABI takes the stddev as a float
    noise = std * ts.input_noise(seed, step, B, 321 * nt, 320 * nt, rank=rank) if noise_std else None
    masks = ts.dropout_masks(seed, step, B, hidden, p, rank=rank) if p > 0.0 else None
    return noise, masks


def _assert_step(e, model, loss, rloss, g, ref_new, lr, n_steps, what):
    """tolerances of test_train.py::test_train_step_matches_oracle"""
    assert abs(loss - rloss) < 2e-5 * max(1.0, rloss), (what, loss, rloss)
    for name, gk in g.items():
        assert _rel(e.train_get(model, 'grad:' + name), gk) < 2e-4, (what, name)
    for name in e.train_tensor_names():
        got = e.train_get(model, name)
        assert np.max(np.abs(got - ref_new[name])) < 0.05 * lr * n_steps + 1e-6, (what, name)
        assert _rel(got, ref_new[name]) < 1e-4, (what, name)


@pytest.mark.parametrize('nt,hidden,B,use_bn,p', STEP_CASES)
def test_wrong_masks_miss_the_gradient_tolerance(oracle, nt, hidden, B, use_bn, p):
    """The stochastic-step comparison has teeth at its shapes (host only): the oracle run with the masks of the next step, of
    another layer's stream, or with noise of the next step misses the 2e-4 gradient tolerance by more than 10x in every kernel
    gradient (masks) / in the layer-0 kernel (noise)."""
    seed = 11
    rng = np.random.default_rng(nt * 100 + B)
    w, x, y = _problem(oracle, rng, nt, hidden, B, use_bn=use_bn)
    noise, masks = _replayed_inputs(seed, 1, B, nt, hidden, p, NOISE_STD)
    _, g, _ = oracle.train_forward_backward(w, x, y, use_bn=use_bn, noise=noise, masks=masks, dropout=p)
    noise2, masks2 = _replayed_inputs(seed, 2, B, nt, hidden, p, NOISE_STD)
    _, gm, _ = oracle.train_forward_backward(w, x, y, use_bn=use_bn, noise=noise, masks=masks2, dropout=p)
    for name in g:
        # (behind a BatchNormalization the batch sum of the regressor's input is B * beta whatever the mask, so the regressor's bias
        # gradient and the last beta's cannot see it: the kernels all do)
        if name.endswith('.kernel'):
            assert _rel(gm[name], g[name]) > 10 * 2e-4, name
    _, gn, _ = oracle.train_forward_backward(w, x, y, use_bn=use_bn, noise=noise2, masks=masks, dropout=p)
    assert _rel(gn['fc_dense0.kernel'], g['fc_dense0.kernel']) > 10 * 2e-4
    # a mask drawn with the padded width as the row pitch (b * ld + j) differs wherever the width is not a multiple of 32
    if hidden[0] % 32:
        ld = (hidden[0] + 31) // 32 * 32
        wrong = ts.dropout_masks(seed, 1, B, (ld,) + tuple(hidden[1:]), p)
        wrong[0] = wrong[0][:, :hidden[0]]
        _, gw, _ = oracle.train_forward_backward(w, x, y, use_bn=use_bn, noise=noise, masks=wrong, dropout=p)
        assert _rel(gw['fc_dense0.kernel'], g['fc_dense0.kernel']) > 10 * 2e-4


# ------------------------------------------------------------------------------------ GPU 1 / 2: the staged noise
def _noise_bound(radius):
    """Bound on |z_dev - z_ref| per element, derived, not measured.  The replay repeats every fp32 operation of tr_normal
    exactly except logf, sqrtf, cosf and two multiplies (-2 * log is exact; radius * cos and the rounding of the square root's
    argument are not).  With the OpenCL full-profile bounds the device library keeps when built without fast-math (log 3 ulp,
    sqrt 3 ulp, cos 4 ulp) the error is at most radius * 2^-24 * (3/2 [log, halved by the square root] + 3 [sqrt] + 1 + 1
    [multiplies] + 4 [cos]) = 10.5 ulp-units of the radius, rounded up to 16.  The floor 2^-10 is for u1 -> 1, where the
    radius goes to zero while the error of the logarithm stays an ulp of its result."""
    return 16.0 * 2.0 ** -24 * np.maximum(radius, 2.0 ** -10)


def _zero_ltf_rows(rng, B, nt):
    x = np.zeros((B, 321 * nt), np.float32)
    x[:, 320 * nt:] = rng.integers(1, 5, (B, nt)).astype(np.float32) * rng.choice([-1.0, 1.0], (B, nt)).astype(np.float32)
    return x


def _device_normals(pkg, nt, B, seed, n_steps=1, rank=0, hidden=(40,)):
    """the device's own N(0,1) draws of steps 1..n_steps: zero LTF columns, noise_std 1 (adding to zero and multiplying by one are exact)"""
    e = pkg.CsiEngine(nt, 2, hidden=hidden)
    if rank:
        e.set_option('train_rank', rank)
    rng = np.random.default_rng(B)
    x, y = _zero_ltf_rows(rng, B, nt), rng.standard_normal((B, 234)).astype(np.float32)
    e.train_begin('real', lr=1e-4, dropout=0.0, seed=seed)
    out = []
    for _ in range(n_steps):
        e.train_step('real', x, y, noise_std=1.0)
        out.append(e.train_staged_input('real', B))
    e.train_end('real', commit=False)
    return x, out


@pytest.mark.gpu
@pytest.mark.parametrize('nt,B,seed', [(4, 33, 77), (4, 300, 1), (8, 64, 0), (4, 256, 2 ** 64 - 1)])
def test_staged_noise_is_the_replayed_normal(pkg, nt, B, seed):
    """x = 0 on the LTF columns, noise_std = 1: the staged input IS the device's normal draw.  Pilot columns bit-equal to x,
    LTF columns within the derived bound of the replay - at step 1, step 2 (another stream), and step 3 after a train_eval
    that must neither add noise nor advance the step."""
    e = pkg.CsiEngine(nt, 2, hidden=(40,))
    rng = np.random.default_rng(B)
    x, y = _zero_ltf_rows(rng, B, nt), rng.standard_normal((B, 234)).astype(np.float32)
    K, L = 321 * nt, 320 * nt
    e.train_begin('real', lr=1e-4, dropout=0.0, seed=seed)
    drawn = []
    for step in (1, 2, 3):
        if step == 3:
            e.train_eval('real', x, y)
            np.testing.assert_array_equal(e.train_staged_input('real', B), x)          # evaluation stages the clean rows
        e.train_step('real', x, y, noise_std=1.0)
        z_dev = e.train_staged_input('real', B)
        np.testing.assert_array_equal(z_dev[:, L:], x[:, L:])
        z_ref, radius = ts.input_noise(seed, step, B, K, L, with_radius=True)
        err = np.abs(z_dev[:, :L].astype(np.float64) - z_ref[:, :L])
        ratio = err / _noise_bound(radius[:, :L])
        print(f'step {step}: max |z_dev - z_ref| / bound = {ratio.max():.3f} (bound = 16 ulp-units of the radius)')
        assert ratio.max() <= 1.0, (step, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
        drawn.append(z_dev)
    assert not np.array_equal(drawn[0], drawn[1]) and not np.array_equal(drawn[1], drawn[2]) and not np.array_equal(drawn[0], drawn[2])
    assert abs(_z_corr(drawn[0][:, :L], drawn[1][:, :L])) < Z_MAX
    e.train_end('real', commit=False)


def _is_rounding_of(got, exact):
    """got (fp32) is a correct rounding of the exact rational"""
    g = Fraction(float(got))
    half = Fraction(float(np.spacing(np.abs(np.float32(got))))) / 2
    return abs(g - exact) <= half


@pytest.mark.gpu
@pytest.mark.parametrize('noise_std', [0.3, 3.0])
def test_noise_is_scaled_and_added_to_the_ltf_columns(pkg, noise_std):
    """staged = fl32(x + noise_std * z_dev) with z_dev from a zero-input run of the same seed and step: every element is
    bit-equal to one of the two legal evaluations (product rounded, then the sum; or one fused multiply-add - hipcc may
    contract), which puts it within one fp32 ulp of the result; pilot columns are copied."""
    nt, B, seed = 4, 64, 77
    L = 320 * nt
    _, (z_dev,) = _device_normals(pkg, nt, B, seed)
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal((B, 321 * nt)).astype(np.float32), rng.standard_normal((B, 234)).astype(np.float32)
    e = pkg.CsiEngine(nt, 2, hidden=(40,))
    e.train_begin('real', lr=1e-4, dropout=0.0, seed=seed)
    e.train_step('real', x, y, noise_std=noise_std)
    got = e.train_staged_input('real', B)
    e.train_end('real', commit=False)
    np.testing.assert_array_equal(got[:, L:], x[:, L:])
    std = np.float32(noise_std)
    g, xs, zs = got[:, :L], x[:, :L], z_dev[:, :L]
    two_roundings = xs + std * zs                                                      # fp32 throughout
    exact64 = xs.astype(np.float64) + np.float64(std) * zs.astype(np.float64)          # the product is exact in fp64, the sum nearly always
    open_ = ~((g == two_roundings) | (g == exact64.astype(np.float32)))
    print(f'noise_std {noise_std}: {int((g == two_roundings).sum())} of {g.size} equal the two-rounding form, {int(open_.sum())} checked exactly')
    for b, k in zip(*np.nonzero(open_)):                                              # (double rounding of the fp64 sum): exact arithmetic
        exact = Fraction(float(xs[b, k])) + Fraction(float(std)) * Fraction(float(zs[b, k]))
        assert _is_rounding_of(g[b, k], exact), (b, k, float(g[b, k]), float(exact))
    assert open_.sum() < 1e-3 * g.size


@pytest.mark.gpu
def test_noise_std_zero_stages_the_rows_unchanged(pkg):
    nt, B = 4, 33
    rng = np.random.default_rng(4)
    x, y = rng.standard_normal((B, 321 * nt)).astype(np.float32), rng.standard_normal((B, 234)).astype(np.float32)
    e = pkg.CsiEngine(nt, 2, hidden=(40,))
    e.train_begin('real', lr=1e-4, dropout=0.5, seed=77)
    e.train_step('real', x, y, noise_std=0.0)
    np.testing.assert_array_equal(e.train_staged_input('real', B), x)
    e.train_end('real', commit=False)


# ------------------------------------------------------------------------------------ GPU 3: the stochastic step against fp64
@pytest.mark.gpu
@pytest.mark.parametrize('nt,hidden,B,use_bn,p', STEP_CASES)
def test_stochastic_step_matches_oracle(pkg, oracle, nt, hidden, B, use_bn, p):
    """noise_std 0.3 and dropout on: loss, every gradient, every parameter after Adam and the moving statistics of three
    consecutive steps against the fp64 oracle given the replayed noise and masks of the device's step number."""
    seed, lr = 11, 1e-3
    rng = np.random.default_rng(nt * 100 + B)
    w, x, y = _problem(oracle, rng, nt, hidden, B, use_bn=use_bn)
    e = pkg.CsiEngine(nt, 2, hidden=hidden, use_bn=use_bn)
    e.train_begin('real', weights=w, lr=lr, dropout=p, seed=seed)
    ref = {k: np.asarray(v, np.float64) for k, v in w.items() if k != 'bn_eps'}
    state = oracle.adam_init(ref)
    for step in (1, 2, 3):
        xs = (x + 0.1 * (step - 1)).astype(np.float32)
        loss = e.train_step('real', xs, y, noise_std=NOISE_STD)
        noise, masks = _replayed_inputs(seed, step, B, nt, hidden, p, NOISE_STD)
        rloss, ref_new, g = oracle.train_step_reference(ref, state, xs, y, lr=lr, use_bn=use_bn, noise=noise, masks=masks, dropout=p)
        _assert_step(e, 'real', loss, rloss, g, ref_new, lr, step, step)
        ref = ref_new
    e.train_end('real', commit=False)


@pytest.mark.gpu
def test_one_hidden_layer_has_no_dropout(pkg, oracle):
    """The reference puts no Dropout behind the last hidden layer: with one hidden layer a dropout rate changes nothing, bit
    for bit, and the step is the oracle's step without masks."""
    nt, hidden, B, seed, lr = 4, (40,), 33, 5, 1e-3
    rng = np.random.default_rng(6)
    w, x, y = _problem(oracle, rng, nt, hidden, B)
    runs = []
    for p in (0.5, 0.0):
        e = pkg.CsiEngine(nt, 2, hidden=hidden)
        e.train_begin('real', weights=w, lr=lr, dropout=p, seed=seed)
        losses = [e.train_step('real', x, y, noise_std=NOISE_STD) for _ in range(3)]
        runs.append((losses, e.train_weights('real'), {n: e.train_get('real', 'grad:' + n) for n in e.train_tensor_names() if 'moving' not in n}))
        if p:
            ref = {k: np.asarray(v, np.float64) for k, v in w.items() if k != 'bn_eps'}
            state = oracle.adam_init(ref)
            for step in (1, 2, 3):
                noise, _ = _replayed_inputs(seed, step, B, nt, hidden, 0.0, NOISE_STD)
                rloss, ref, g = oracle.train_step_reference(ref, state, x, y, lr=lr, noise=noise)
                assert abs(losses[step - 1] - rloss) < 2e-5 * max(1.0, rloss)
            _assert_step(e, 'real', losses[2], rloss, g, ref, lr, 3, 'one hidden layer')
        e.train_end('real', commit=False)
    assert runs[0][0] == runs[1][0]
    for part in (1, 2):
        for k in runs[0][part]:
            np.testing.assert_array_equal(runs[0][part][k], runs[1][part][k])


# ------------------------------------------------------------------------------------ GPU 4: the entry points share the streams
@pytest.mark.gpu
@pytest.mark.parametrize('hidden,use_bn,p', [((100, 72, 24), True, 0.15), ((96, 40), False, 0.5)])
def test_entry_points_share_the_streams(pkg, oracle, hidden, use_bn, p):
    """train_step, train_backward + train_apply, and train_step_indexed on a resident dataset holding the same rows: the same
    three stochastic steps bit for bit, and (through train_step) the oracle's steps under the replayed noise and masks."""
    nt, nr, B, seed, lr = 4, 2, 64, 21, 1e-3
    rng = np.random.default_rng(50)
    n = 96                                                       # samples of the resident set; a batch takes 64 of them
    table = rng.standard_normal((n, 320 * nt)).astype(np.float32)
    P = rng.integers(-2, 3, (nt, nt)).astype(np.float64)
    itx = (np.arange(n) % nt).astype(np.int32)
    yall = rng.standard_normal((n, 234)).astype(np.float32)
    rows = np.concatenate([table, P[itx].astype(np.float32)], axis=1)
    w = oracle.make_weights(rng, 321 * nt, hidden, 234, use_bn=use_bn)
    batches = [rng.permutation(n)[:B] for _ in range(3)]
    results = []
    for path in ('step', 'backward_apply', 'indexed'):
        e = pkg.CsiEngine(nt, nr, hidden=hidden, use_bn=use_bn)
        e.set_pilot(P)
        e.train_begin('imag', weights=w, lr=lr, dropout=p, seed=seed)
        if path == 'indexed':
            e.train_set_dataset('imag', table, np.arange(n, dtype=np.int32), itx, yall)
        ref = {k: np.asarray(v, np.float64) for k, v in w.items() if k != 'bn_eps'}
        state = oracle.adam_init(ref)
        trace = []
        for step, ids in enumerate(batches, start=1):
            xs, ys = rows[ids], yall[ids]
            if path == 'step':
                loss = e.train_step('imag', xs, ys, noise_std=NOISE_STD)
                noise, masks = _replayed_inputs(seed, step, B, nt, hidden, p, NOISE_STD)
                rloss, ref, g = oracle.train_step_reference(ref, state, xs, ys, lr=lr, use_bn=use_bn, noise=noise, masks=masks, dropout=p)
                _assert_step(e, 'imag', loss, rloss, g, ref, lr, step, step)
            elif path == 'backward_apply':
                loss = e.train_backward('imag', xs, ys, noise_std=NOISE_STD)
                e.train_apply('imag')
            else:
                loss = e.train_step_indexed('imag', ids, noise_std=NOISE_STD)
            trace.append((loss, e.train_staged_input('imag', B), e.train_weights('imag'),
                          {k: e.train_get('imag', 'grad:' + k) for k in e.train_tensor_names() if 'moving' not in k}))
        results.append(trace)
        e.train_end('imag', commit=False)
    for other in results[1:]:
        for (l0, s0, w0, g0), (l1, s1, w1, g1) in zip(results[0], other):
            assert l0 == l1
            np.testing.assert_array_equal(s0, s1)
            for k in w0:
                np.testing.assert_array_equal(w0[k], w1[k])
            for k in g0:
                np.testing.assert_array_equal(g0[k], g1[k])


# ------------------------------------------------------------------------------------ GPU 5: the batch size changes on one trainer
BATCH_SEQUENCE = (256, 33, 300, 64)


@pytest.mark.gpu
@pytest.mark.parametrize('hidden,use_bn', [((100, 72, 24), True), ((96, 40), False)])
@pytest.mark.parametrize('stochastic', [True, False])
def test_changing_batch_size_on_one_trainer(pkg, oracle, hidden, use_bn, stochastic):
    """B = 256, 33, 300, 64 on one trainer against the oracle carried through the same four steps: the buffers are re-created
    above 256 rows and the K padding of the transposed wgrad operands holds the columns of the previous, larger batch unless
    it is cleared - a leak is an O(1) error of grad:*.kernel.  Without noise and dropout the B = 33 gradients are
    additionally bit-equal to those of a fresh trainer started from the same parameters."""
    nt, seed = 4, 31
    p, std = (0.15, NOISE_STD) if stochastic else (0.0, 0.0)
    lr = 1e-3 if stochastic else 1e-9                            # tiny: the fresh trainer's Adam state does not matter for its gradients
    rng = np.random.default_rng(70)
    w = oracle.make_weights(rng, 321 * nt, hidden, 234, use_bn=use_bn)
    e = pkg.CsiEngine(nt, 2, hidden=hidden, use_bn=use_bn)
    e.train_begin('real', weights=w, lr=lr, dropout=p, seed=seed)
    ref = {k: np.asarray(v, np.float64) for k, v in w.items() if k != 'bn_eps'}
    state = oracle.adam_init(ref)
    for step, B in enumerate(BATCH_SEQUENCE, start=1):
        x = rng.standard_normal((B, 321 * nt)).astype(np.float32)
        y = rng.standard_normal((B, 234)).astype(np.float32)
        before = e.train_weights('real') if (B == 33 and not stochastic) else None
        loss = e.train_step('real', x, y, noise_std=std)
        noise, masks = _replayed_inputs(seed, step, B, nt, hidden, p, std)
        rloss, ref_new, g = oracle.train_step_reference(ref, state, x, y, lr=lr, use_bn=use_bn, noise=noise, masks=masks, dropout=p)
        _assert_step(e, 'real', loss, rloss, g, ref_new, lr, step, (step, B))
        ref = ref_new
        if before is not None:
            f = pkg.CsiEngine(nt, 2, hidden=hidden, use_bn=use_bn)
            f.train_begin('real', weights=before, lr=lr, dropout=p, seed=seed)
            assert f.train_step('real', x, y, noise_std=std) == loss
            for k in g:
                np.testing.assert_array_equal(f.train_get('real', 'grad:' + k), e.train_get('real', 'grad:' + k))
            f.train_end('real', commit=False)
    e.train_end('real', commit=False)


# ------------------------------------------------------------------------------------ GPU 6: Glorot initialisation
@pytest.mark.gpu
@pytest.mark.parametrize('nt,hidden,use_bn,pool,seed', [(4, (96, 40), True, None, 5), (4, (100, 72, 24), False, None, 0),
                                                        (8, (128, 128), True, None, 77), (4, (96, 40), True, 'max', 5)])
def test_glorot_initialisation_is_the_replayed_kernel(pkg, oracle, nt, hidden, use_bn, pool, seed):
    """train_begin(weights=None): every kernel equals the replayed Glorot kernel within 2 fp32 ulp (the limit goes through a
    division and sqrtf), biases 0, gamma 1, beta 0, moving mean 0, moving variance 1; a decimated-input model uses the pooled
    fan-in.  After train_end(commit) the inference model predicts with exactly these tensors (zero padding of the K-major
    copies beyond the fan-in included)."""
    e = pkg.CsiEngine(nt, 2, hidden=hidden, use_bn=use_bn, input_pool=pool)
    e.train_begin('real', lr=1e-4, seed=seed)
    got = e.train_weights('real')
    widths = (e.l0_in,) + tuple(hidden) + (234,)
    assert e.l0_in == (160 * nt if pool else 320 * nt) + nt
    ref = {'bn_eps': 1e-3}
    for li in range(len(hidden) + 1):
        name = 'fc_regressor' if li == len(hidden) else f'fc_dense{li}'
        k_ref = ts.glorot(seed, li, widths[li], widths[li + 1])
        k_dev = got[name + '.kernel']
        assert k_dev.shape == k_ref.shape
        ulps = np.abs(k_dev.astype(np.float64) - k_ref.astype(np.float64)) / np.spacing(np.abs(k_ref)).astype(np.float64)
        print(f'{name}.kernel: max distance {ulps.max():.2f} ulp')
        assert ulps.max() <= 2.0, (name, float(ulps.max()))
        assert np.abs(k_dev).max() <= float(ts.glorot_limit(widths[li], widths[li + 1])) * (1 + 2 ** -22)
        assert np.all(got[name + '.bias'] == 0.0)
        ref[name + '.kernel'], ref[name + '.bias'] = k_ref, got[name + '.bias']
        if use_bn and li < len(hidden):
            assert np.all(got[f'bn{li}.gamma'] == 1.0) and np.all(got[f'bn{li}.beta'] == 0.0)
            assert np.all(got[f'bn{li}.moving_mean'] == 0.0) and np.all(got[f'bn{li}.moving_variance'] == 1.0)
            for s in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
                ref[f'bn{li}.{s}'] = got[f'bn{li}.{s}']
    e.train_end('real', commit=True)
    rng = np.random.default_rng(8)
    x = rng.standard_normal((37, 321 * nt)).astype(np.float32)
    L = 320 * nt
    xin = np.concatenate([np.maximum(x[:, 0:L:2], x[:, 1:L:2]), x[:, L:]], axis=1) if pool else x
    assert _rel(e.predict_samples('real', x), oracle.fc_forward(xin, ref, np.float64)) < 1e-4


# ------------------------------------------------------------------------------------ GPU, part C: ranks of a data-parallel fit
@pytest.mark.gpu
def test_ranks_draw_their_own_noise_and_masks(pkg, oracle):
    """Two engines standing for two ranks of a data-parallel fit, equal seeds: different noise, each the replay of its own
    rank's stream, uncorrelated; identical Glorot kernels; rank 0 has the single-process streams (the replay with rank 0 is the
    formula every other test here pins).  A stochastic step of rank 1 follows the oracle under rank 1's noise and masks."""
    nt, B, seed = 4, 64, 77
    K, L = 321 * nt, 320 * nt
    draws, kernels = {}, {}
    for rank in (0, 1, 3):
        e = pkg.CsiEngine(nt, 2, hidden=(96, 40))
        assert e.get_option('train_rank') == 0
        if rank:
            e.set_option('train_rank', rank)
        rng = np.random.default_rng(B)
        x, y = _zero_ltf_rows(rng, B, nt), rng.standard_normal((B, 234)).astype(np.float32)
        e.train_begin('real', lr=1e-4, dropout=0.0, seed=seed)
        kernels[rank] = e.train_weights('real')
        e.train_step('real', x, y, noise_std=1.0)
        z_dev = e.train_staged_input('real', B)
        z_ref, radius = ts.input_noise(seed, 1, B, K, L, rank=rank, with_radius=True)
        ratio = np.abs(z_dev[:, :L].astype(np.float64) - z_ref[:, :L]) / _noise_bound(radius[:, :L])
        assert ratio.max() <= 1.0, (rank, float(ratio.max()))
        np.testing.assert_array_equal(z_dev[:, L:], x[:, L:])
        draws[rank] = z_dev[:, :L]
        e.train_end('real', commit=False)
    for a, b in ((0, 1), (0, 3), (1, 3)):
        assert not np.array_equal(draws[a], draws[b])
        assert abs(_z_corr(draws[a], draws[b])) < Z_MAX, (a, b)
        for k in kernels[a]:
            np.testing.assert_array_equal(kernels[a][k], kernels[b][k])             # initial weights stay identical across ranks
    # the full step on rank 1: its own masks as well
    hidden, p, lr, rank = (100, 72, 24), 0.5, 1e-3, 1
    rng = np.random.default_rng(90)
    w, x, y = _problem(oracle, rng, nt, hidden, B)
    e = pkg.CsiEngine(nt, 2, hidden=hidden)
    e.set_option('train_rank', rank)
    e.train_begin('real', weights=w, lr=lr, dropout=p, seed=seed)
    ref = {k: np.asarray(v, np.float64) for k, v in w.items() if k != 'bn_eps'}
    state = oracle.adam_init(ref)
    for step in (1, 2):
        loss = e.train_step('real', x, y, noise_std=NOISE_STD)
        noise, masks = _replayed_inputs(seed, step, B, nt, hidden, p, NOISE_STD, rank=rank)
        rloss, ref, g = oracle.train_step_reference(ref, state, x, y, lr=lr, noise=noise, masks=masks, dropout=p)
        _assert_step(e, 'real', loss, rloss, g, ref, lr, step, step)
    e.train_end('real', commit=False)
    with pytest.raises(pkg.CsiError):
        e.set_option('train_rank', -1)
