"""GPU tests of the decimated-input models (--decimate_max / --decimate_avg, massiveMIMO_CSI_prediction_DNN.py:30-31,197-205):
MaxPooling1D / AveragePooling1D (pool 2, stride 2) on the LTF before Flatten + Concatenate, csi_set_input_pool.  The reference for
parity is the numpy oracle fed with the LTF columns pooled here, in numpy."""
import os
import sys

import numpy as np
import pytest

from conftest import rel_rows

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TOL = 1e-5
BF16_TOL_IMPL = 4e-3      # vs the bf16-operand emulation (the tolerance of every bf16 kernel, tests/test_gpu_dnn_bf16.py)
MODES = ('max', 'avg')


def pool_np(x, mode):
    """keras MaxPooling1D / AveragePooling1D (pool 2, stride 2, 'valid') over the last axis, in float32."""
    x = np.asarray(x, np.float32)
    a, b = x[..., 0::2], x[..., 1::2]
    return np.maximum(a, b) if mode == 'max' else (np.float32(0.5) * (a + b)).astype(np.float32)


def pool_ltf(ltf, mode):
    """complex preambles [.., len_ltf] -> pooled [.., len_ltf / 2] (each component plane pooled on its own, as the engine does)."""
    ltf = np.asarray(ltf)
    return pool_np(ltf.real, mode).astype(np.float64) + 1j * pool_np(ltf.imag, mode).astype(np.float64)


def _weights(oracle, seed, nt, hidden, use_bn=True):
    rng = np.random.default_rng(seed)
    d_in = 160 * nt + nt
    return (oracle.make_weights(rng, d_in, list(hidden), 234, use_bn=use_bn),
            oracle.make_weights(rng, d_in, list(hidden), 234, use_bn=use_bn))


def _engine(pkg, nt, nr, hidden, w_re, w_im, P, mode, use_bn=True, **kw):
    e = pkg.CsiEngine(nt, nr, hidden=hidden, use_bn=use_bn, input_pool=mode, **kw)
    e.load_weights('real', w_re)
    e.load_weights('imag', w_im)
    e.set_pilot(P)
    return e


def _packets(oracle, seed, nt, nr, npkt):
    rng = np.random.default_rng(seed)
    P = oracle.hadamard(nt) if nt in (4, 8, 16, 32, 64, 128) else rng.integers(-3, 4, (nt, nt)).astype(np.float64)
    ltf, _ = oracle.make_structured_packets(rng, npkt, nr, P, snr_db=10.0)
    return P, ltf.astype(np.complex64)


def _subset(npkt, n=6):
    """packets whose oracle is evaluated (every packet is independent; the fp64 oracle of thousands of packets takes minutes)"""
    return np.unique(np.linspace(0, npkt - 1, min(n, npkt)).astype(int))


# nt, nr, npkt, hidden: every layer-0 route - one-packet gemv (1 / 2 packets = 4 / 8 preambles), the tile kernel of the small path
# (8 packets of Nt = 8), the weight-streaming split-f16 kernel (24 / 64 packets), the split-f16 GEMM (500 packets), config 2 (4000)
F32_CASES = [
    (32, 4, 1, (1024, 1024)),
    (32, 4, 2, (1024, 1024)),
    (8, 2, 8, (64, 64)),
    (32, 4, 24, (1024, 1024)),
    (32, 4, 64, (1024, 1024)),
    (32, 4, 500, (1024, 1024)),
    (32, 4, 4000, (1024, 1024)),
    (4, 2, 3, (64, 64)),
    (12, 2, 7, (40,)),
    (64, 2, 3, (64, 32)),
]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('nt,nr,npkt,hidden', F32_CASES)
def test_pooled_f32_matches_oracle(pkg, oracle, mode, nt, nr, npkt, hidden):
    w_re, w_im = _weights(oracle, nt * 7 + npkt, nt, hidden)
    P, ltf = _packets(oracle, npkt + nt, nt, nr, npkt)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P, mode)
    assert e.get_option('input_pool') == {'max': 1, 'avg': 2}[mode]
    o_re, o_im = e.predict(ltf)
    sel = _subset(npkt)
    r_re, r_im = oracle.predict_packets(pool_ltf(ltf[sel], mode), P, w_re, w_im, np.float64, pkt_batch=len(sel))
    assert rel_rows(o_re[sel], r_re) < TOL and rel_rows(o_im[sel], r_im) < TOL, (rel_rows(o_re[sel], r_re), rel_rows(o_im[sel], r_im))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('npkt', [1, 3, 24])
def test_pooled_f32_graph_replay(pkg, oracle, mode, npkt):
    """use_graph: the pooling pass / the pooled one-packet kernel inside the captured graph, replayed."""
    nt, nr, hidden = 32, 4, (256, 256)
    w_re, w_im = _weights(oracle, 3, nt, hidden)
    P, ltf = _packets(oracle, 4, nt, nr, npkt)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P, mode)
    e.set_option('use_graph', 1)
    d_re, d_im = e.to_device(ltf.real), e.to_device(ltf.imag)
    o_re, o_im = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
    h_re, h_im = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
    r_re, r_im = oracle.predict_packets(pool_ltf(ltf, mode), P, w_re, w_im, np.float64, pkt_batch=npkt)
    r_ls = oracle.ls_estimate(ltf, P)
    for _ in range(4):          # eager, eager, capture, replay
        e.estimate_device(d_re, d_im, npkt, o_re, o_im, h_re, h_im)
        e.synchronize()
        assert rel_rows(o_re.download(), r_re) < TOL and rel_rows(o_im.download(), r_im) < TOL
        h = h_re.download() + 1j * h_im.download()
        assert rel_rows(np.concatenate([h.real, h.imag], -1), np.concatenate([r_ls.real, r_ls.imag], -1)) < TOL, 'LS reads the raw preambles'
    assert e.get_option('graph_replays') >= 1


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('nt,nr,npkt,hidden', [(64, 2, 1, (256, 256)), (64, 4, 64, (1024, 1024)), (64, 4, 500, (1024, 1024)),
                                               (32, 4, 24, (512, 256)), (8, 2, 5, (64, 64))])
def test_pooled_bf16_matches_emulation(pkg, oracle, mode, nt, nr, npkt, hidden):
    w_re, w_im = _weights(oracle, nt + npkt, nt, hidden)
    P, ltf = _packets(oracle, npkt, nt, nr, npkt)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P, mode, dtype='bf16')
    o_re, o_im = e.predict(ltf)
    sel = _subset(npkt)
    b_re, b_im = oracle.predict_packets_bf16(pool_ltf(ltf[sel], mode), P, w_re, w_im)
    assert rel_rows(o_re[sel], b_re) < BF16_TOL_IMPL and rel_rows(o_im[sel], b_im) < BF16_TOL_IMPL


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('mode', MODES)
def test_pooled_predict_samples_takes_raw_rows(pkg, oracle, mode, dtype):
    """csi_predict_samples: raw [B, len_ltf + nt] rows in (keras predict), pooled on the device."""
    nt, hidden = 8, (64, 48)
    w_re, w_im = _weights(oracle, 11, nt, hidden)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((37, 320 * nt + nt)).astype(np.float32)
    xp = np.concatenate([pool_np(x[:, :320 * nt], mode), x[:, 320 * nt:]], axis=1)
    e = pkg.CsiEngine(nt, 1, hidden=hidden, input_pool=mode, dtype=dtype)
    e.load_weights('real', w_re)
    y = e.predict_samples('real', x)
    if dtype == 'f32':
        assert rel_rows(y, oracle.fc_forward(xp, w_re, np.float64)) < TOL
    else:
        assert rel_rows(y, oracle.fc_forward_bf16(xp, w_re)) < BF16_TOL_IMPL


@pytest.mark.parametrize('mode', MODES)
def test_pooled_predictor_c128(pkg, oracle, mode, tmp_path):
    """csi_estimate_c128 through CSIPredictor: the mode comes from the config.json CSIModel.save writes; an explicit argument that
    disagrees raises."""
    nt, nr, npkt, hidden = 8, 2, 6, (64, 64)
    w_re, w_im = _weights(oracle, 21, nt, hidden)
    P, ltf = _packets(oracle, 22, nt, nr, npkt)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P, mode)
    for d, w in (('real', w_re), ('imag', w_im)):
        pkg.CSIModel(e, d).load_weights(w).save(str(tmp_path / f'{d}_keras_model'), pilot=P)
    e.close()
    pred = pkg.CSIPredictor(str(tmp_path), experiment='matlab_maMimo')
    assert pred.engine.input_pool == mode
    out = pred.inference(ltf.astype(np.complex128))
    r_re, r_im = oracle.predict_packets(pool_ltf(ltf, mode), P, w_re, w_im, np.float64, pkt_batch=npkt)
    assert rel_rows(out.real, r_re) < TOL and rel_rows(out.imag, r_im) < TOL
    other = 'avg' if mode == 'max' else 'max'
    with pytest.raises(pkg.CsiError, match='disagrees'):
        pkg.CSIPredictor(str(tmp_path), experiment='matlab_maMimo', input_pool=other)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_mode_none_is_bit_identical(pkg, oracle, dtype):
    """a context that set 'none' computes exactly what a context that never called csi_set_input_pool computes"""
    nt, nr, hidden = 32, 4, (256, 256)
    rng = np.random.default_rng(8)
    d_in = 320 * nt + nt
    w_re, w_im = oracle.make_weights(rng, d_in, list(hidden), 234), oracle.make_weights(rng, d_in, list(hidden), 234)
    for npkt in (1, 3, 40):
        P, ltf = _packets(oracle, npkt, nt, nr, npkt)
        a = _engine(pkg, nt, nr, hidden, w_re, w_im, P, None, dtype=dtype)
        b = pkg.CsiEngine(nt, nr, hidden=hidden, dtype=dtype)
        b._check(b._lib.csi_set_input_pool(b._ctx, 0))
        b.load_weights('real', w_re)
        b.load_weights('imag', w_im)
        b.set_pilot(P)
        assert b.get_option('input_pool') == 0
        for x, y in zip(a.predict(ltf), b.predict(ltf)):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize('npkt', [1, 2])
def test_pooled_one_packet_call_launch_count(pkg, oracle, npkt):
    """the one-packet path pools inside its layer-0 loads: a pooled call launches as many kernels as an unpooled one (three)"""
    nt, nr, hidden = 32, 4, (1024, 1024)
    P, ltf = _packets(oracle, 1, nt, nr, npkt)
    counts = {}
    for mode in (None, 'max', 'avg'):
        rng = np.random.default_rng(2)
        d_in = (160 if mode else 320) * nt + nt
        w = [oracle.make_weights(rng, d_in, list(hidden), 234) for _ in range(2)]
        e = _engine(pkg, nt, nr, hidden, w[0], w[1], P, mode)
        e.predict(ltf)
        e.profile_enable(True)
        e.profile_reset()
        e.predict(ltf)
        prof = e.profile()
        counts[mode] = sum(v['launches'] for v in prof.values())
        assert prof['input_pool']['launches'] == 0, mode
        assert e.get_option('small_calls') >= 1
    assert counts['max'] == counts[None] == counts['avg'] == 3, counts


@pytest.mark.parametrize('mode', MODES)
def test_pooled_training_matches_oracle(pkg, oracle, mode):
    """noise_std = 0: loss and gradient of layer 0 against oracle.train_forward_backward on the pooled rows; Glorot fan-in pooled"""
    nt, hidden, B = 4, (48, 32), 24
    rng = np.random.default_rng(31)
    w = oracle.make_weights(rng, 160 * nt + nt, list(hidden), 234)
    x = rng.standard_normal((B, 320 * nt + nt)).astype(np.float32)
    y = rng.standard_normal((B, 234)).astype(np.float32)
    xp = np.concatenate([pool_np(x[:, :320 * nt], mode), x[:, 320 * nt:]], axis=1)
    e = pkg.CsiEngine(nt, 1, hidden=hidden, input_pool=mode)
    e.train_begin('real', weights=w, lr=1e-4, dropout=0.0, seed=1)
    loss = e.train_step('real', x, y, noise_std=0.0)
    ref_loss, g, _ = oracle.train_forward_backward(w, xp, y)
    assert abs(loss - ref_loss) < 1e-4 * max(1.0, ref_loss)
    for name in ('fc_dense0.kernel', 'fc_dense0.bias', 'fc_regressor.kernel'):
        got = e.train_get('real', 'grad:' + name)
        assert rel_rows(got.reshape(1, -1), g[name].reshape(1, -1)) < 2e-4, name
    np.testing.assert_array_equal(e.train_staged_input('real', B), xp)
    e.train_end('real', commit=False)
    e.train_begin('imag', lr=1e-4, seed=3)          # Glorot-uniform: limit sqrt(6 / (fan_in + fan_out)) with the pooled fan-in
    k0 = e.train_get('imag', 'fc_dense0.kernel')
    assert k0.shape == (160 * nt + nt, hidden[0])
    assert np.max(np.abs(k0)) <= np.sqrt(6.0 / (160 * nt + nt + hidden[0])) * (1 + 1e-6)
    e.train_end('imag', commit=False)


@pytest.mark.parametrize('mode', MODES)
def test_pooled_training_noise_before_pooling(pkg, oracle, mode):
    """same seed and step: the staged input of a pooled context is pool() of the staged input of an unpooled one, bit for bit -
    the noise is drawn per raw sample and added before the pooling (DNN.py:191-203)"""
    nt, hidden, B = 4, (32,), 16
    rng = np.random.default_rng(41)
    x = rng.standard_normal((B, 320 * nt + nt)).astype(np.float32)
    y = rng.standard_normal((B, 234)).astype(np.float32)
    staged = {}
    for m in (None, mode):
        e = pkg.CsiEngine(nt, 1, hidden=hidden, input_pool=m)
        e.train_begin('real', lr=1e-4, dropout=0.0, seed=9)
        e.train_step('real', x, y, noise_std=0.25)
        staged[m] = e.train_staged_input('real', B)
        e.train_end('real', commit=False)
    raw = staged[None]
    assert not np.array_equal(raw, x), 'noise was added'
    np.testing.assert_array_equal(raw[:, 320 * nt:], x[:, 320 * nt:])
    expect = np.concatenate([pool_np(raw[:, :320 * nt], mode), raw[:, 320 * nt:]], axis=1)
    np.testing.assert_array_equal(staged[mode], expect)


def test_pooled_fit_commit_predicts_like_fresh_load(pkg, oracle):
    nt, nr, hidden, B = 8, 2, (64, 64), 32
    rng = np.random.default_rng(51)
    x = rng.standard_normal((B, 320 * nt + nt)).astype(np.float32)
    y = rng.standard_normal((B, 234)).astype(np.float32)
    e = pkg.CsiEngine(nt, nr, hidden=hidden, input_pool='avg')
    for d in ('real', 'imag'):
        e.train_begin(d, lr=1e-3, dropout=0.15, seed=4)
        for _ in range(3):
            e.train_step(d, x, y, noise_std=0.1)
    w = {d: e.train_weights(d) for d in ('real', 'imag')}
    for d in ('real', 'imag'):
        e.train_end(d, commit=True)
    P, ltf = _packets(oracle, 52, nt, nr, 3)
    e.set_pilot(P)
    f = _engine(pkg, nt, nr, hidden, w['real'], w['imag'], P, 'avg')
    for a, b in zip(e.predict(ltf), f.predict(ltf)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(e.predict_samples('real', x), f.predict_samples('real', x))


def test_pooling_refusals(pkg, oracle):
    nt, hidden = 8, (64, 64)
    w_re, w_im = _weights(oracle, 61, nt, hidden)
    rng = np.random.default_rng(62)
    w_full = oracle.make_weights(rng, 320 * nt + nt, list(hidden), 234)
    # a mode after weights
    e = pkg.CsiEngine(nt, 2, hidden=hidden)
    e.load_weights('real', w_full)
    with pytest.raises(pkg.CsiError, match='before csi_load_weights'):
        e._check(e._lib.csi_set_input_pool(e._ctx, 1))
    # a mode while a trainer exists
    t = pkg.CsiEngine(nt, 2, hidden=hidden)
    t.train_begin('imag', lr=1e-4)
    with pytest.raises(pkg.CsiError, match='trainer'):
        t._check(t._lib.csi_set_input_pool(t._ctx, 2))
    # unpooled weights in a pooled context, pooled weights in an unpooled one
    p = pkg.CsiEngine(nt, 2, hidden=hidden, input_pool='max')
    with pytest.raises(pkg.CsiError, match='input pooling max'):
        p.load_weights('real', w_full)
    with pytest.raises(pkg.CsiError, match='decimated model'):
        pkg.CsiEngine(nt, 2, hidden=hidden).load_weights('real', w_re)
    # the single-input model
    with pytest.raises(pkg.CsiError, match='nt > 0'):
        pkg.CsiEngine(0, 1, hidden=(16,), len_ltf=64, input_pool='avg')
    # clones between modes: refused with text, destination left empty
    P, ltf = _packets(oracle, 63, nt, 2, 2)
    src = _engine(pkg, nt, 2, hidden, w_re, w_im, P, 'max')
    for dst_mode in (None, 'avg'):
        dst = pkg.CsiEngine(nt, 2, hidden=hidden, input_pool=dst_mode)
        with pytest.raises(pkg.CsiError, match='input pooling differs'):
            dst.clone_weights_from(src)
        with pytest.raises(pkg.CsiError):
            dst.predict(ltf)
    # pooled -> pooled: bit-identical
    dst = pkg.CsiEngine(nt, 2, hidden=hidden, input_pool='max')
    dst.clone_weights_from(src)
    for a, b in zip(src.predict(ltf), dst.predict(ltf)):
        np.testing.assert_array_equal(a, b)
