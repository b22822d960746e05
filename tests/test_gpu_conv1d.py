"""GPU tests of the CONV1D models (--model CONV1D, massiveMIMO_CSI_prediction_DNN.py:236-270): Conv1D(128, 7, 'same') + relu, its
BatchNormalization, AveragePooling1D (pool 2) and Flatten in front of the FC stack, csi_set_model_type.  The reference for parity is
built here: a float64 numpy statement of the front end produces the features, which go with the P rows into the numpy oracle
(oracle.fc_forward through predict_packets, or its bf16 emulation)."""
import os
import pickle
import sys

import numpy as np
import pytest

from conftest import rel_rows

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TOL = 1e-5
BF16_TOL_IMPL = 4e-3      # vs the bf16-operand emulation (the tolerance of every bf16 kernel, tests/test_gpu_dnn_bf16.py)
BF16_TOL_F64 = 3e-2
BN_EPS = 1e-3


def conv_weights(rng):
    """cnn1d_1 (7 taps x 1 x 128 filters, bias) and its BatchNormalization, with non-trivial statistics."""
    return {'cnn1d_1.kernel': rng.uniform(-0.5, 0.5, (7, 1, 128)).astype(np.float32),
            'cnn1d_1.bias': (0.05 * rng.standard_normal(128)).astype(np.float32),
            'conv_bn.gamma': rng.uniform(0.5, 1.5, 128).astype(np.float32),
            'conv_bn.beta': (0.1 * rng.standard_normal(128)).astype(np.float32),
            'conv_bn.moving_mean': (0.1 * rng.standard_normal(128)).astype(np.float32),
            'conv_bn.moving_variance': rng.uniform(0.5, 1.5, 128).astype(np.float32)}


def features(x, w):
    """float64 front end: x [..., L] -> [..., 64 L] (conv 'same', relu, BN with moving statistics, pool 2, flatten channels last)."""
    x = np.asarray(x, np.float64)
    L = x.shape[-1]
    k = w['cnn1d_1.kernel'].astype(np.float64).reshape(7, 128)
    xp = np.concatenate([np.zeros(x.shape[:-1] + (3,)), x, np.zeros(x.shape[:-1] + (3,))], axis=-1)
    conv = np.zeros(x.shape + (128,))
    for j in range(7):
        conv += xp[..., j:j + L, None] * k[j]
    conv += w['cnn1d_1.bias'].astype(np.float64)
    q = np.maximum(conv, 0.0)
    q = (q - w['conv_bn.moving_mean'].astype(np.float64)) / np.sqrt(w['conv_bn.moving_variance'].astype(np.float64) + BN_EPS) * \
        w['conv_bn.gamma'].astype(np.float64) + w['conv_bn.beta'].astype(np.float64)
    a = (q[..., 0::2, :] + q[..., 1::2, :]) / 2.0
    return a.reshape(x.shape[:-1] + (64 * L,))


def _weights(oracle, seed, nt, hidden, use_bn=True):
    rng = np.random.default_rng(seed)
    d_in = 64 * 320 * nt + nt
    ws = []
    for _ in range(2):
        w = oracle.make_weights(rng, d_in, list(hidden), 234, use_bn=use_bn)
        w.update(conv_weights(rng))
        ws.append(w)
    return ws


def _engine(pkg, nt, nr, hidden, w_re, w_im, P, use_bn=True, **kw):
    e = pkg.CsiEngine(nt, nr, hidden=hidden, use_bn=use_bn, model='CONV1D', **kw)
    e.load_weights('real', w_re)
    e.load_weights('imag', w_im)
    e.set_pilot(P)
    return e


def _packets(oracle, seed, nt, nr, npkt):
    rng = np.random.default_rng(seed)
    P = oracle.hadamard(nt)
    ltf, _ = oracle.make_structured_packets(rng, npkt, nr, P, snr_db=10.0)
    return P, ltf.astype(np.complex64)


def _subset(npkt, n=4):
    return np.unique(np.linspace(0, npkt - 1, min(n, npkt)).astype(int))


def reference(oracle, ltf, P, w_re, w_im, bf16=False):
    """float64 (or bf16-emulation) outputs of packets ltf: the features of each plane through its own model's front end."""
    feat = features(np.asarray(ltf).real, w_re) + 1j * features(np.asarray(ltf).imag, w_im)
    if bf16:
        return oracle.predict_packets_bf16(feat, P, w_re, w_im)
    return oracle.predict_packets(feat, P, w_re, w_im, np.float64, pkt_batch=len(feat))


# (nt, nr, npkt, hidden, options): the one-packet gemv (1 / 2 packets at Nt = 4, Nr = 2), the weight-streaming split-f16 kernel
# (7 ... 300 packets), and by option the skinny gemv (small_fused = 0), the split-f16 GEMM (l0_stream = 0, f32_engine = 1: below
# ~1300 preambles the weight-streaming kernel takes the call) and the fp32 MFMA GEMM
# (f32_engine = 0); Nt = 32: the reference's K0 = 655360
# (dense BN on and off at Nt = 4 / 8; the Nt = 32 shapes with dense BN)
F32_CASES = [(4, 2, n, (64, 32), {}, bn) for n in (1, 2, 7, 37, 300) for bn in (True, False)] + [
    (4, 2, 2, (64, 32), {'small_fused': 0}, True),
    (4, 2, 37, (64, 32), {'l0_stream': 0, 'f32_engine': 1}, True),
    (4, 2, 37, (64, 32), {'f32_engine': 0}, True),
    (4, 2, 300, (64, 32), {'f32_engine': 0}, False),
    (8, 4, 64, (128,), {}, True),
    (8, 4, 64, (128,), {}, False),
    (32, 4, 3, (256, 128), {}, True),
    (32, 4, 64, (256, 128), {}, True),
]


@pytest.mark.parametrize('nt,nr,npkt,hidden,opts,use_bn', F32_CASES)
def test_conv1d_f32_matches_float64(pkg, oracle, nt, nr, npkt, hidden, opts, use_bn):
    w_re, w_im = _weights(oracle, nt * 7 + npkt, nt, hidden, use_bn)
    P, ltf = _packets(oracle, npkt + nt, nt, nr, npkt)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P, use_bn)
    for k, v in opts.items():
        e.set_option(k, v)
    assert e.get_option('model_type') == 1
    n0 = e.get_option('conv_launches')
    o_re, o_im = e.predict(ltf)
    assert e.get_option('conv_launches') > n0
    sel = _subset(npkt)
    r_re, r_im = reference(oracle, ltf[sel], P, w_re, w_im)
    errs = rel_rows(o_re[sel], r_re), rel_rows(o_im[sel], r_im)
    assert max(errs) < TOL, errs


def test_conv1d_f32_routes_taken(pkg, oracle):
    """the call sizes above reach the routes they are meant to: one-packet path, weight-streaming kernel, split-f16 GEMM"""
    nt, nr, hidden = 4, 2, (64, 32)
    w_re, w_im = _weights(oracle, 5, nt, hidden)
    P, ltf = _packets(oracle, 6, nt, nr, 37)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P)
    s0 = e.get_option('small_calls')
    e.predict(ltf[:2])
    assert e.get_option('small_calls') == s0 + 1
    l0 = e.get_option('l0_stream_launches')
    e.predict(ltf)
    assert e.get_option('l0_stream_launches') > l0
    e.set_option('l0_stream', 0)
    e.set_option('f32_engine', 1)
    h0 = e.get_option('hs_launches')
    e.predict(ltf)
    assert e.get_option('hs_launches') > h0


def test_conv1d_f32_several_chunks(pkg, oracle):
    """a small workspace cuts the call into several chunks: the same numbers as one chunk within 1e-6, and the float64 contract"""
    nt, nr, npkt, hidden = 4, 2, 300, (64, 32)
    w_re, w_im = _weights(oracle, 71, nt, hidden)
    P, ltf = _packets(oracle, 72, nt, nr, npkt)
    one = _engine(pkg, nt, nr, hidden, w_re, w_im, P)
    many = _engine(pkg, nt, nr, hidden, w_re, w_im, P, workspace_bytes=48 << 20)
    n0 = many.get_option('conv_launches')
    a, b = one.predict(ltf), many.predict(ltf)
    assert many.get_option('conv_launches') - n0 >= 4, 'expected several chunks per model'
    for x, y in zip(a, b):
        assert rel_rows(y, x) < 1e-6
    sel = _subset(npkt)
    r_re, r_im = reference(oracle, ltf[sel], P, w_re, w_im)
    assert rel_rows(b[0][sel], r_re) < TOL and rel_rows(b[1][sel], r_im) < TOL


@pytest.mark.parametrize('nt,nr,npkt,hidden', [(4, 2, 1, (64, 32)), (4, 2, 37, (64, 32)), (4, 2, 300, (64, 32)),
                                               (8, 4, 64, (128,)), (32, 4, 3, (256, 128)), (32, 4, 64, (256, 128))])
def test_conv1d_bf16_matches_emulation(pkg, oracle, nt, nr, npkt, hidden):
    w_re, w_im = _weights(oracle, nt + npkt, nt, hidden)
    P, ltf = _packets(oracle, npkt, nt, nr, npkt)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P, dtype='bf16')
    o_re, o_im = e.predict(ltf)
    sel = _subset(npkt)
    b_re, b_im = reference(oracle, ltf[sel], P, w_re, w_im, bf16=True)
    errs = rel_rows(o_re[sel], b_re), rel_rows(o_im[sel], b_im)
    assert max(errs) < BF16_TOL_IMPL, errs
    r_re, r_im = reference(oracle, ltf[sel], P, w_re, w_im)
    errs = rel_rows(o_re[sel], r_re), rel_rows(o_im[sel], r_im)
    assert max(errs) < BF16_TOL_F64, errs


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_conv1d_predict_samples_takes_raw_rows(pkg, oracle, dtype):
    """csi_predict_samples: raw [B, len_ltf + nt] rows (keras predict), the front end and the pilot-column copy on the device"""
    nt, hidden = 4, (64, 48)
    w_re, _ = _weights(oracle, 11, nt, hidden)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((37, 320 * nt + nt)).astype(np.float32)
    xf = np.concatenate([features(x[:, :320 * nt], w_re), x[:, 320 * nt:]], axis=1)
    e = pkg.CsiEngine(nt, 1, hidden=hidden, model='CONV1D', dtype=dtype)
    e.load_weights('real', w_re)
    y = e.predict_samples('real', x)
    if dtype == 'f32':
        assert rel_rows(y, oracle.fc_forward(xf, w_re, np.float64)) < TOL
    else:
        assert rel_rows(y, oracle.fc_forward_bf16(xf, w_re)) < BF16_TOL_IMPL


def test_setters_with_defaults_in_either_order(pkg, oracle):
    """csi_set_input_pool(none) after csi_set_model_type(CONV1D), and csi_set_model_type(FC) after csi_set_input_pool(avg), keep the
    layer-0 width the other setting asks for: the context loads its own weights and predicts them right; pooling on a CONV1D context is
    refused in either order"""
    nt, nr, hidden = 4, 2, (64, 32)
    P, ltf = _packets(oracle, 91, nt, nr, 3)
    w_re, w_im = _weights(oracle, 92, nt, hidden)
    e = pkg.CsiEngine(nt, nr, hidden=hidden, model='CONV1D')
    e._check(e._lib.csi_set_input_pool(e._ctx, 0))
    assert e.get_option('model_type') == 1 and e.get_option('input_pool') == 0
    e.load_weights('real', w_re)
    e.load_weights('imag', w_im)
    e.set_pilot(P)
    o_re, o_im = e.predict(ltf)
    r_re, r_im = reference(oracle, ltf, P, w_re, w_im)
    assert rel_rows(o_re, r_re) < TOL and rel_rows(o_im, r_im) < TOL
    rng = np.random.default_rng(93)
    p_re, p_im = (oracle.make_weights(rng, 160 * nt + nt, list(hidden), 234) for _ in range(2))
    f = pkg.CsiEngine(nt, nr, hidden=hidden, input_pool='avg')
    f._check(f._lib.csi_set_model_type(f._ctx, 0))
    assert f.get_option('model_type') == 0 and f.get_option('input_pool') == 2
    f.load_weights('real', p_re)
    f.load_weights('imag', p_im)
    f.set_pilot(P)
    o_re, o_im = f.predict(ltf)
    avg = lambda a: (np.float32(0.5) * (a[..., 0::2] + a[..., 1::2])).astype(np.float64)
    pooled = avg(ltf.real) + 1j * avg(ltf.imag)
    r_re, r_im = oracle.predict_packets(pooled, P, p_re, p_im, np.float64, pkt_batch=3)
    assert rel_rows(o_re, r_re) < TOL and rel_rows(o_im, r_im) < TOL
    g = pkg.CsiEngine(nt, nr, hidden=hidden, model='CONV1D')
    for mode in (1, 2):
        with pytest.raises(pkg.CsiError, match='no input pooling'):
            g._check(g._lib.csi_set_input_pool(g._ctx, mode))
    assert g.get_option('model_type') == 1 and g.get_option('input_pool') == 0
    g.load_weights('real', w_re)                  # still a CONV1D context of 64 len_ltf + nt layer-0 rows


@pytest.mark.parametrize('npkt', [1, 3, 40])
def test_conv1d_graph_replay_bit_identical(pkg, oracle, npkt):
    """use_graph: the front end inside the captured graph (both streams of an fp32 call); replays give the eager bits, LS reads the
    raw preambles"""
    nt, nr, hidden = 4, 2, (64, 32)
    w_re, w_im = _weights(oracle, 3, nt, hidden)
    P, ltf = _packets(oracle, 4, nt, nr, npkt)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P)
    eager = e.predict(ltf)
    e.set_option('use_graph', 1)
    d_re, d_im = e.to_device(ltf.real), e.to_device(ltf.imag)
    o_re, o_im = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
    h_re, h_im = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
    r_ls = oracle.ls_estimate(ltf, P)
    for _ in range(4):          # eager, eager, capture, replay
        e.estimate_device(d_re, d_im, npkt, o_re, o_im, h_re, h_im)
        e.synchronize()
        np.testing.assert_array_equal(o_re.download(), eager[0])
        np.testing.assert_array_equal(o_im.download(), eager[1])
        h = h_re.download() + 1j * h_im.download()
        assert rel_rows(np.concatenate([h.real, h.imag], -1), np.concatenate([r_ls.real, r_ls.imag], -1)) < TOL
    assert e.get_option('graph_replays') >= 1


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_conv1d_repeat_calls_identical(pkg, oracle, dtype):
    nt, nr, npkt, hidden = 4, 2, 37, (64, 32)
    w_re, w_im = _weights(oracle, 13, nt, hidden)
    P, ltf = _packets(oracle, 14, nt, nr, npkt)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P, dtype=dtype)
    a, b = e.predict(ltf), e.predict(ltf)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_conv1d_ls_unaffected(pkg, oracle):
    """LS reads the raw preambles: a CONV1D context's LS estimate is bit-identical to an FC context's"""
    nt, nr, npkt = 4, 2, 5
    w_re, w_im = _weights(oracle, 15, nt, (64, 32))
    P, ltf = _packets(oracle, 16, nt, nr, npkt)
    e = _engine(pkg, nt, nr, (64, 32), w_re, w_im, P)
    f = pkg.CsiEngine(nt, nr, hidden=(64, 32))
    f.set_pilot(P)
    np.testing.assert_array_equal(e.ls_estimate(ltf), f.ls_estimate(ltf))


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_model_type_fc_is_bit_identical(pkg, oracle, dtype):
    """a context that set FC explicitly computes exactly what a default context computes"""
    nt, nr, hidden = 32, 4, (256, 256)
    rng = np.random.default_rng(8)
    d_in = 320 * nt + nt
    w_re, w_im = oracle.make_weights(rng, d_in, list(hidden), 234), oracle.make_weights(rng, d_in, list(hidden), 234)
    for npkt in (1, 3, 40):
        P, ltf = _packets(oracle, npkt, nt, nr, npkt)
        a = pkg.CsiEngine(nt, nr, hidden=hidden, dtype=dtype)
        b = pkg.CsiEngine(nt, nr, hidden=hidden, dtype=dtype, model='FC')
        b._check(b._lib.csi_set_model_type(b._ctx, 0))
        for x in (a, b):
            x.load_weights('real', w_re)
            x.load_weights('imag', w_im)
            x.set_pilot(P)
        assert b.get_option('model_type') == 0
        for x, y in zip(a.predict(ltf), b.predict(ltf)):
            np.testing.assert_array_equal(x, y)


def test_conv1d_clones(pkg, oracle):
    """conv -> conv: bit-identical; conv -> FC and FC -> conv: refused with text, the destination left empty"""
    nt, nr, hidden = 4, 2, (64, 32)
    w_re, w_im = _weights(oracle, 61, nt, hidden)
    P, ltf = _packets(oracle, 63, nt, nr, 9)
    src = _engine(pkg, nt, nr, hidden, w_re, w_im, P)
    dst = pkg.CsiEngine(nt, nr, hidden=hidden, model='CONV1D')
    dst.clone_weights_from(src)
    for a, b in zip(src.predict(ltf), dst.predict(ltf)):
        np.testing.assert_array_equal(a, b)
    fc = pkg.CsiEngine(nt, nr, hidden=hidden)
    with pytest.raises(pkg.CsiError, match='model type differs'):
        fc.clone_weights_from(src)
    with pytest.raises(pkg.CsiError):
        fc.predict(ltf)
    rng = np.random.default_rng(64)
    f_src = pkg.CsiEngine(nt, nr, hidden=hidden)
    for d in ('real', 'imag'):
        f_src.load_weights(d, oracle.make_weights(rng, 320 * nt + nt, list(hidden), 234))
    f_src.set_pilot(P)
    with pytest.raises(pkg.CsiError, match='model type differs'):
        pkg.CsiEngine(nt, nr, hidden=hidden, model='CONV1D').clone_weights_from(f_src)


def test_conv1d_refusals_on_device(pkg, oracle):
    nt, hidden = 4, (64, 32)
    w_re, _ = _weights(oracle, 81, nt, hidden)
    e = pkg.CsiEngine(nt, 2, hidden=hidden, model='CONV1D')
    with pytest.raises(pkg.CsiError, match='CONV1D'):
        e.train_begin('real', lr=1e-4)
    bad = dict(w_re)
    del bad['cnn1d_1.bias']
    with pytest.raises(pkg.CsiError, match='CONV1D'):
        e.load_weights('real', bad)
    with pytest.raises(pkg.CsiError, match='CONV1D'):
        pkg.CsiEngine(nt, 2, hidden=hidden).load_weights('real', w_re)
    with pytest.raises(pkg.CsiError, match='exclude each other'):
        pkg.CsiEngine(nt, 2, hidden=hidden, input_pool='max', model='CONV1D')
    f = pkg.CsiEngine(nt, 2, hidden=hidden)
    f.load_weights('real', oracle.make_weights(np.random.default_rng(1), 320 * nt + nt, list(hidden), 234))
    with pytest.raises(pkg.CsiError, match='before csi_load_weights'):
        f._check(f._lib.csi_set_model_type(f._ctx, 1))


def test_conv1d_predictor_folder_and_hdf5_pair(pkg, oracle, tmp_path):
    """CSIPredictor on the folder CSIModel.save writes (config.json "model") and on a pair of Keras HDF5 files our writer wrote"""
    nt, nr, npkt, hidden = 4, 2, 5, (64, 32)
    w_re, w_im = _weights(oracle, 21, nt, hidden)
    P, ltf = _packets(oracle, 22, nt, nr, npkt)
    r_re, r_im = reference(oracle, ltf, P, w_re, w_im)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P)
    for d, w in (('real', w_re), ('imag', w_im)):
        pkg.CSIModel(e, d).load_weights(w).save(str(tmp_path / 'a' / f'{d}_keras_model'), pilot=P)
        (tmp_path / 'b').mkdir(exist_ok=True)
        pkg.save_weight_file(str(tmp_path / 'b' / f'{d}_keras_model.h5'), w, component=d)
    e.close()
    for sub in ('a', 'b'):
        pred = pkg.CSIPredictor(str(tmp_path / sub), experiment='matlab_maMimo', pilot=P if sub == 'b' else None, nr=nr)
        assert pred.engine.model == 'CONV1D'
        out = pred.inference(ltf.astype(np.complex128))
        assert rel_rows(out.real, r_re) < TOL and rel_rows(out.imag, r_im) < TOL, sub


def test_cli_test_conv1d_end_to_end(pkg, oracle, tmp_path, capsys):
    """--test --model CONV1D: pickle dataset + HDF5 checkpoints in, .mat files out, against the float64 reference"""
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import cli
    rng = np.random.default_rng(77)
    nt, nr, npkt, hidden = 4, 2, 3, (64, 32)
    P = oracle.hadamard(nt)
    ltf, _ = oracle.make_structured_packets(rng, npkt, nr, P, snr_db=3.0)
    y = oracle.ls_estimate(ltf, P).reshape(npkt * nr * nt, 234)
    X = np.zeros((npkt * nr * nt, 2), dtype=int)
    LTF = {}
    for p in range(npkt):
        for r in range(nr):
            key = 500 + p * nr + r
            LTF[key] = {'real': ltf[p, r].real.copy(), 'imag': ltf[p, r].imag.copy()}
            for t in range(nt):
                X[p * nr * nt + r * nt + t] = [key, t]
    ds = {'X': X, 'y': {'real': y.real.copy(), 'imag': y.imag.copy()}, 'LTF': LTF, 'P': P.T.copy(), 'simParams': {'nTX': nt, 'nRX': nr}}
    with open(tmp_path / 'test.b', 'wb') as f:
        pickle.dump(ds, f)
    w_re, w_im = _weights(oracle, 3, nt, hidden)
    model_dir, work = tmp_path / 'model', tmp_path / 'out'
    model_dir.mkdir(); work.mkdir()
    for d, w in (('real', w_re), ('imag', w_im)):
        pkg.save_weight_file(str(model_dir / f'{d}_weights-improvement.hdf5'), w, component=d)
    base = ['--test', '-x', str(tmp_path / 'test.b'), '--modeldir', str(model_dir), '-d', str(work), '--nn', '64', '32', '--useBN',
            '--datasource', 'matlab_maMimo', '--valSameTrain']
    assert cli.main(base + ['--model', 'CONV1D', '--decimate_avg']) == 0
    out = capsys.readouterr().out
    assert 'ignored for --model CONV1D' in out and 'cnn1d_1 (Conv1D relu)' in out
    r_re, r_im = reference(oracle, ltf.astype(np.complex64), P, w_re, w_im)
    for n in range(npkt):
        for d, r in (('real', r_re), ('imag', r_im)):
            m = loadmat(str(work / f'test_csi_predictions_{d}_{n + 1}.mat'))['all_pkts_csi_nn_out'][0, 0]
            assert rel_rows(m['y'], r[n].reshape(nr * nt, 234)) < TOL
    # the folder the run leaves behind loads as a CONV1D model again
    assert pkg.CSIPredictor(str(work), experiment='matlab_maMimo').engine.model == 'CONV1D'
    # --model FC on CONV1D weights aborts with text
    with pytest.raises(SystemExit):
        cli.main(base)
    assert 'CONV1D model' in capsys.readouterr().out
