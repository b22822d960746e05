"""GPU tests (-m gpu; every call through the C-ABI of libcsi_mamimo.so, checked against the numpy oracle on identical seeded inputs at the
1e-5 norm-relative contract of BASELINE.json unless a test states its own): the drop-in surface: CSIPredictor / Keras-model twins (inference.py:6-68), model files, dataset / CLI, host-buffer pipeline, complex entry points, hipGraph replay, profile and metric entry points."""

import os

import numpy as np
import pytest

from conftest import rel_rows

pytestmark = pytest.mark.gpu


TOL = 1e-5


def _weights(oracle, seed, nt, hidden, use_bn=True, n_out=234):
    rng = np.random.default_rng(seed)
    d_in = 320 * nt + nt
    return (oracle.make_weights(rng, d_in, list(hidden), n_out, use_bn=use_bn),
            oracle.make_weights(rng, d_in, list(hidden), n_out, use_bn=use_bn))


def _engine(pkg, nt, nr, hidden, w_re, w_im, P, use_bn=True, n_out=234, **kw):
    e = pkg.CsiEngine(nt, nr, hidden=hidden, n_out=n_out, use_bn=use_bn, **kw)
    e.load_weights('real', w_re)
    e.load_weights('imag', w_im)
    e.set_pilot(P)
    return e


def _pilot(rng, nt, orthogonal=True):
    from oracle import csi_oracle as o
    if orthogonal:
        P = o.hadamard(nt)
        return (P[rng.permutation(nt)] * rng.choice([-1.0, 1.0], nt)[:, None]).astype(np.float64)
    return rng.integers(-3, 4, (nt, nt)).astype(np.float64)


def test_keras_model_surface_with_reference_batches(pkg, oracle, golden_dir):
    """CSIModel.predict driven exactly like DNN.py:339-346: a Sequence yielding
    ([Xsig (B,lenLTF,1), Xp (B,Nt)], y, None) with B = nTX*nRX, batches taken from the golden
    vectors the reference's DataGenerator produced."""
    g = np.load(os.path.join(golden_dir, 'ref_datagen_nt4.npz'))
    nt, nr, npkt = int(g['nt']), int(g['nr']), int(g['npkt'])
    w_re, w_im = _weights(oracle, 4321, nt, (64, 64))
    P_rows = g['P_matlab']
    e = _engine(pkg, nt, nr, (64, 64), w_re, w_im, P_rows)

    class Seq:                                   # stands in for the reference DataGenerator
        def __init__(self, d):
            self.d = d

        def __len__(self):
            return npkt

        def __getitem__(self, b):
            return [g[f'{self.d}_Xsig'][b], g[f'{self.d}_Xp'][b]], g[f'{self.d}_y'][b], None

    ltf = (g['ds_ltf_real'] + 1j * g['ds_ltf_imag']).reshape(npkt, nr, 320 * nt)
    fast_re, fast_im = e.predict(ltf)
    for d, w, fast in (('real', w_re, fast_re), ('imag', w_im, fast_im)):
        model = pkg.CSIModel(e, d).load_weights(w)
        csi_out = model.predict(Seq(d))
        assert csi_out.shape == (npkt * nt * nr, 234) and csi_out.dtype == np.float32
        x = np.concatenate([g[f'{d}_Xsig'][..., 0], g[f'{d}_Xp']], axis=-1).reshape(npkt * nr * nt, -1)
        ref = oracle.fc_forward(x, w, np.float64)
        assert rel_rows(csi_out, ref) < TOL
        assert rel_rows(fast.reshape(csi_out.shape), ref) < TOL      # packet path, same samples


def test_empty_and_error_paths(pkg, oracle):
    nt, nr, hidden = 4, 2, (32, 32)
    e = pkg.CsiEngine(nt, nr, hidden=hidden)
    ltf = pkg.synth.white_packets(np.random.default_rng(1), 2, nr, nt)
    with pytest.raises(pkg.CsiError) as ex:         # nothing loaded yet
        e.predict(ltf)
    assert ex.value.code == -2
    w_re, w_im = _weights(oracle, 9, nt, hidden)
    e.load_weights('real', w_re)
    e.set_pilot(np.eye(nt))
    with pytest.raises(pkg.CsiError) as ex:         # imag model missing
        e.predict(ltf)
    assert ex.value.code == -2
    e.load_weights('imag', w_im)
    o_re, o_im = e.predict(np.zeros((0, nr, 320 * nt), dtype=np.complex64))
    assert o_re.shape == (0, nr, nt, 234)
    bad = dict(w_re)
    bad['fc_dense1.kernel'] = bad['fc_dense1.kernel'][:, :16]
    with pytest.raises(pkg.CsiError) as ex:
        e.load_weights('real', bad)
    assert ex.value.code == -1
    with pytest.raises(pkg.CsiError):
        e.predict(np.zeros((1, nr, 7), dtype=np.complex64))


def test_hip_path_matches_committed_oracle_fixture(pkg, golden_dir):
    """LS and DNN of the committed Nt=4 fixture (tests/golden/oracle_nt4.npz) without running the oracle."""
    import os
    g = np.load(os.path.join(golden_dir, 'oracle_nt4.npz'))
    w = {tag: {k.split('.', 1)[1]: g[k] for k in g.files if k.startswith(f'w_{tag}.')} for tag in ('re', 'im')}
    e = pkg.CsiEngine(int(g['nt']), int(g['nr']), hidden=(64, 64))
    e.load_weights('real', w['re'])
    e.load_weights('imag', w['im'])
    e.set_pilot(g['P'])
    o_re, o_im = e.predict(g['ltf'])
    assert rel_rows(o_re, g['dnn_real']) < TOL and rel_rows(o_im, g['dnn_imag']) < TOL
    h = e.ls_estimate(g['ltf'])
    assert rel_rows(np.concatenate([h.real, h.imag], -1), np.concatenate([g['ls'].real, g['ls'].imag], -1)) < TOL


# ------------------------------------------------------------------------------------ accuracy metric
def test_nmse_metric_matches_oracle(pkg, oracle):
    """NMSE_subk (BER_test_maMIMO_LTF.m:675-686) on the device: host-buffer and device-pointer entry
    points against the oracle; per-link ratios; a ragged link count; determinism."""
    rng = np.random.default_rng(21)
    nt, nr, npkt = 8, 2, 37
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    ref = (rng.standard_normal((npkt, nr, nt, 234)) + 1j * rng.standard_normal((npkt, nr, nt, 234))).astype(np.complex64)
    est = (ref + 0.05 * (rng.standard_normal(ref.shape) + 1j * rng.standard_normal(ref.shape))).astype(np.complex64)
    want = oracle.nmse_subk(ref, est)
    got = e.nmse(ref, est)
    assert abs(got - want) <= 1e-6 * want
    assert e.nmse(ref, est) == got
    assert e.nmse(ref, ref) == 0.0
    # other bin counts (RICE_RENEW has 52 outputs) and a single link
    assert abs(e.nmse(ref[0, 0, 0, :52], est[0, 0, 0, :52]) - oracle.nmse_subk(ref[0, 0, 0, :52], est[0, 0, 0, :52])) <= 1e-6 * want
    d = [e.empty((npkt, nr, nt, 234)) for _ in range(4)]
    for a, h in zip(d, (ref.real, ref.imag, est.real, est.imag)):
        a.upload(np.ascontiguousarray(h, np.float32))
    per = e.empty((npkt * nr * nt,))
    got_d = e.nmse_device(d[0], d[1], d[2], d[3], npkt * nr * nt, 234, per)
    assert got_d == got
    ratios = per.download()
    num = np.sum(np.abs(ref.astype(np.complex128) - est) ** 2, -1).reshape(-1)
    den = np.sum(np.abs(ref.astype(np.complex128)) ** 2, -1).reshape(-1)
    np.testing.assert_allclose(ratios, num / den, rtol=2e-6)
    # the metric the reference reports for a DNN estimate: DNN output against the true channel
    w_re, w_im = _weights(oracle, 5, nt, (8,))
    P = _pilot(rng, nt)
    e.load_weights('real', w_re); e.load_weights('imag', w_im); e.set_pilot(P)
    ltf, H = oracle.make_structured_packets(rng, 6, nr, oracle.hadamard(nt), snr_db=5.0)
    o_re, o_im = e.predict(ltf)
    assert abs(e.nmse(H, o_re + 1j * o_im) - oracle.nmse_subk(H, o_re + 1j * o_im)) <= 1e-5 * oracle.nmse_subk(H, o_re + 1j * o_im)


# ------------------------------------------------------------------------------------ twin
def test_csipredictor_twin_mamimo_end_to_end(pkg, oracle, tmp_path):
    rng = np.random.default_rng(31)
    nt, nr, npkt, hidden = 8, 2, 4, (64, 64)
    w_re, w_im = _weights(oracle, 17, nt, hidden)
    P = _pilot(rng, nt)
    e = pkg.CsiEngine(nt, nr, hidden=hidden)
    for d, w in (('real', w_re), ('imag', w_im)):
        pkg.CSIModel(e, d).load_weights(w).save(str(tmp_path / f'{d}_keras_model'), pilot=P)   # DNN.py:411
    pred = pkg.CSIPredictor(str(tmp_path), experiment='matlab_maMimo')
    ltf, H = oracle.make_structured_packets(rng, npkt, nr, P, snr_db=10.0)
    csi = pred.inference(ltf)
    assert csi.shape == (npkt, nr, nt, 234) and csi.dtype == np.complex64
    r_re, r_im = oracle.predict_packets(ltf.astype(np.complex64), P, w_re, w_im, np.float64, pkt_batch=npkt)
    ref = oracle.recombine(r_re, r_im)
    assert rel_rows(np.concatenate([csi.real, csi.imag], -1), np.concatenate([ref.real, ref.imag], -1)) < TOL
    h_ls = pred.ls_estimate(ltf)
    ref_ls = oracle.ls_estimate(ltf, P)
    assert rel_rows(np.concatenate([h_ls.real, h_ls.imag], -1), np.concatenate([ref_ls.real, ref_ls.imag], -1)) < TOL
    with pytest.raises(SystemExit) as ex:
        pred.inference(ltf.astype(np.complex64))
    assert ex.value.code == -1


def test_reference_model_files_load_and_predict(pkg, oracle, golden_dir, tmp_path):
    """a-10 end to end: ``CSIModel.load_weights('<d>_weights-improvement.hdf5')`` (DNN.py:334) on the
    libhdf5-written Keras checkpoints and ``CSIPredictor(model_path)`` (inference.py:15-16) on SavedModel
    directories ``<d>_keras_model/`` - no h5py / TensorFlow - must predict what the oracle computes from the
    tensors that were written into those files."""
    import shutil
    exp = np.load(os.path.join(golden_dir, 'keras_weights_expected.npz'))
    nt, nr, npkt = int(exp['nt']), 3, 5
    w = {d: {k[len(d) + 1:]: exp[k] for k in exp.files if k.startswith(d + '.')} for d in ('real', 'imag')}
    rng = np.random.default_rng(41)
    P = _pilot(rng, nt)
    ltf = oracle.make_structured_packets(rng, npkt, nr, oracle.hadamard(nt), snr_db=5.0)[0]
    r_re, r_im = oracle.predict_packets(ltf.astype(np.complex64), P, w['real'], w['imag'], np.float64, pkt_batch=npkt)
    # Keras HDF5 checkpoints through the keras-shaped model object
    e = pkg.CsiEngine(nt, nr, hidden=(16, 8))
    for d in ('real', 'imag'):
        shutil.copy(os.path.join(golden_dir, f'keras_weights_{d}.hdf5'), tmp_path / f'{d}_weights-improvement.hdf5')
        pkg.CSIModel(e, d).load_weights(str(tmp_path / f'{d}_weights-improvement.hdf5'))
    e.set_pilot(P)
    o_re, o_im = e.predict(ltf)
    assert rel_rows(o_re, r_re) < TOL and rel_rows(o_im, r_im) < TOL
    x = oracle.samples_from_packets(ltf[:2].astype(np.complex64), P.astype(np.float32), 'imag')
    assert rel_rows(pkg.CSIModel(e, 'imag').load_weights(str(tmp_path / 'imag_weights-improvement.hdf5')).predict(x),
                    oracle.fc_forward(x, w['imag'], np.float64)) < TOL
    # SavedModel directories through the deployment wrapper (no config.json, no pilot, no rx count inside)
    pred = pkg.CSIPredictor(os.path.join(golden_dir, 'savedmodel_fixture'), experiment='matlab_maMimo', pilot=P)
    h = pred.inference(ltf.astype(np.complex128))
    assert h.shape == (npkt, nr, nt, 234)
    assert rel_rows(h.real, r_re) < TOL and rel_rows(h.imag, r_im) < TOL
    h1 = pkg.CSIPredictor(os.path.join(golden_dir, 'savedmodel_fixture'), experiment='matlab_maMimo', pilot=P, nr=nr).inference(ltf.astype(np.complex128))
    np.testing.assert_array_equal(h1, h)


def test_csipredictor_twin_rice_renew_single_input(pkg, oracle, golden_dir, tmp_path):
    """The reference's implemented experiment: single-input FC model, 52 outputs re-inserted
    into 64 bins.  Input/recombination/post-processing behaviour is pinned by the golden
    vectors recorded from the reference class itself."""
    import json
    g = np.load(os.path.join(golden_dir, 'ref_inference_rice.npz'), allow_pickle=True)
    x = g['x']
    n_in = x.shape[1]
    rng = np.random.default_rng(3)
    ws = {}
    for d in ('real', 'imag'):
        w = oracle.make_weights(rng, n_in, [32], 52, use_bn=True)
        ws[d] = w
        p = tmp_path / f'{d}_keras_model'
        p.mkdir()
        pkg.save_weight_file(str(p / 'weights.safetensors'), w)
        (p / 'config.json').write_text(json.dumps(dict(nt=0, nr=1, len_ltf=n_in, hidden=[32], n_out=52, use_bn=True)))
    pred = pkg.CSIPredictor(str(tmp_path))                       # experiment='RICE_RENEW' default
    y = pred.inference(x)
    assert y.shape == (x.shape[0], 64) and y.dtype == np.complex128
    ref = oracle.postprocess_rice_renew(oracle.recombine(oracle.fc_forward(x.real, ws['real'], np.float64),
                                                          oracle.fc_forward(x.imag, ws['imag'], np.float64)))
    np.testing.assert_array_equal(y == 0, g['y'] == 0)            # same null pattern as the reference
    nz = ref[:, 1:27]
    assert rel_rows(np.concatenate([y[:, 1:27].real, y[:, 1:27].imag], -1), np.concatenate([nz.real, nz.imag], -1)) < TOL


def test_dataset_label_self_consistency(pkg, oracle):
    """dataset labels are the LS estimate of the same noisy preamble; a dataset in the
    reference's pickle layout, packed by the host code, must satisfy LS(ltf) == labels on the GPU."""
    rng = np.random.default_rng(12)
    nt, nr, npkt = 8, 2, 3
    P_rows = _pilot(rng, nt)
    ltf, _ = oracle.make_structured_packets(rng, npkt, nr, P_rows, snr_db=3.0)
    y = oracle.ls_estimate(ltf, P_rows).reshape(npkt * nr * nt, 234)          # what MATLAB stores as label
    X = np.zeros((npkt * nr * nt, 2), dtype=int)
    LTF = {}
    for p in range(npkt):
        for r in range(nr):
            key = 1000 + p * nr + r
            LTF[key] = {'real': ltf[p, r].real.copy(), 'imag': ltf[p, r].imag.copy()}
            for t in range(nt):
                X[p * nr * nt + r * nt + t] = [key, t]
    ds = {'X': X, 'y': {'real': y.real.copy(), 'imag': y.imag.copy()}, 'LTF': LTF, 'P': P_rows.T.copy(),
          'simParams': {'nTX': nt, 'nRX': nr}}
    packed = pkg.dataset.packets_from_dataset(ds)
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    assert pkg.dataset.label_consistency(e, packed) < TOL
    packed['pilot'] = packed['pilot'].T.copy()                                # wrong orientation must show
    assert pkg.dataset.label_consistency(e, packed) > 1e-2


def test_cli_test_run_end_to_end(pkg, oracle, tmp_path, capsys):
    """The command-line twin of `DNN.py --test`: pickle dataset + saved models in, evaluate() figure
    and per-packet .mat files out."""
    import pickle
    from scipy.io import loadmat
    rng = np.random.default_rng(77)
    nt, nr, npkt, hidden = 8, 2, 3, (64, 32)
    P_rows = _pilot(rng, nt)
    ltf, _ = oracle.make_structured_packets(rng, npkt, nr, P_rows, snr_db=3.0)
    y = oracle.ls_estimate(ltf, P_rows).reshape(npkt * nr * nt, 234)
    X = np.zeros((npkt * nr * nt, 2), dtype=int)
    LTF = {}
    for p in range(npkt):
        for r in range(nr):
            key = 500 + p * nr + r
            LTF[key] = {'real': ltf[p, r].real.copy(), 'imag': ltf[p, r].imag.copy()}
            for t in range(nt):
                X[p * nr * nt + r * nt + t] = [key, t]
    ds = {'X': X, 'y': {'real': y.real.copy(), 'imag': y.imag.copy()}, 'LTF': LTF, 'P': P_rows.T.copy(),
          'simParams': {'nTX': nt, 'nRX': nr}}
    with open(tmp_path / 'test.b', 'wb') as f:
        pickle.dump(ds, f)
    w_re, w_im = _weights(oracle, 3, nt, hidden)
    model_dir, work = tmp_path / 'model', tmp_path / 'out'
    model_dir.mkdir(); work.mkdir()
    pkg.save_weight_file(str(model_dir / 'real_weights-improvement.safetensors'), w_re)
    pkg.save_weight_file(str(model_dir / 'imag_weights-improvement.safetensors'), w_im)
    from dl_channel_estimation_mamimo_amd import cli
    # the pipeline's own invocation (full_pipeline_maMIMO_DNNEst.sh:47) passes --valSameTrain: every packet is tested
    rc = cli.main(['--test', '-x', str(tmp_path / 'test.b'), '--modeldir', str(model_dir), '-d', str(work), '--nn', '64', '32',
                   '--useBN', '--datasource', 'matlab_maMimo', '--valSameTrain', '--execTime'])
    assert rc == 0
    out = capsys.readouterr().out
    assert 'loss (mse vs labels)' in out and 'LS(GPU) vs stored LS labels' in out and 'pair_dense_gemm' in out
    r_re, r_im = oracle.predict_packets(ltf.astype(np.complex64), P_rows, w_re, w_im, np.float64, pkt_batch=npkt)
    for n in range(npkt):
        m = loadmat(str(work / f'test_csi_predictions_imag_{n + 1}.mat'))['all_pkts_csi_nn_out'][0, 0]
        assert rel_rows(m['y'], r_im[n].reshape(nr * nt, 234)) < TOL
        np.testing.assert_array_equal(m['true_y'], y.imag.reshape(npkt, nr * nt, 234)[n])
    # DNN.py:411: the test run leaves <d>_keras_model/ behind, the folder inference.CSIPredictor loads (inference.py:15-16)
    pred = pkg.CSIPredictor(str(work), experiment='matlab_maMimo')
    h = pred.inference(ltf[:1].astype(np.complex128))
    assert rel_rows(h.real, r_re[:1]) < TOL and rel_rows(h.imag, r_im[:1]) < TOL
    # without --valSameTrain the reference tests the LAST floor(Npkt * valTrainRatio) packets and numbers
    # their files from 1 (DNN.py:125-128, massiveMIMO_dataGenerator.py:46-55)
    work2 = tmp_path / 'out2'
    work2.mkdir()
    rc = cli.main(['--test', '-x', str(tmp_path / 'test.b'), '--modeldir', str(model_dir), '-d', str(work2), '--nn', '64', '32',
                   '--useBN', '--datasource', 'matlab_maMimo', '--valTrainRatio', '0.34'])
    assert rc == 0 and 'Validation separate from Training' in capsys.readouterr().out
    assert sorted(f for f in os.listdir(work2) if f.endswith('.mat')) == ['test_csi_predictions_imag_1.mat', 'test_csi_predictions_real_1.mat']
    m = loadmat(str(work2 / 'test_csi_predictions_real_1.mat'))['all_pkts_csi_nn_out'][0, 0]
    assert rel_rows(m['y'], r_re[npkt - 1].reshape(nr * nt, 234)) < TOL
    np.testing.assert_array_equal(m['true_y'], y.real.reshape(npkt, nr * nt, 234)[npkt - 1])
    # train -> test -> re-train -> test in ONE work directory (round-2 advice): the second test run must evaluate the
    # new checkpoint, not the <d>_keras_model/ folder the first test run left there (DNN.py:279-281,334 always loads
    # <d>_weights-improvement.hdf5)
    work3 = tmp_path / 'out3'
    work3.mkdir()
    pkg.save_weight_file(str(work3 / 'real_weights-improvement.safetensors'), w_re)
    pkg.save_weight_file(str(work3 / 'imag_weights-improvement.safetensors'), w_im)
    args3 = ['--test', '-x', str(tmp_path / 'test.b'), '-d', str(work3), '--nn', '64', '32', '--useBN', '--datasource', 'matlab_maMimo', '--valSameTrain']
    assert cli.main(args3) == 0 and os.path.isdir(work3 / 'real_keras_model')
    w_re2, w_im2 = _weights(oracle, 4, nt, hidden)
    pkg.save_weight_file(str(work3 / 'real_weights-improvement.safetensors'), w_re2)
    pkg.save_weight_file(str(work3 / 'imag_weights-improvement.safetensors'), w_im2)
    assert cli.main(args3) == 0
    capsys.readouterr()
    n_re, n_im = oracle.predict_packets(ltf.astype(np.complex64), P_rows, w_re2, w_im2, np.float64, pkt_batch=npkt)
    m = loadmat(str(work3 / 'test_csi_predictions_real_2.mat'))['all_pkts_csi_nn_out'][0, 0]
    assert rel_rows(m['y'], n_re[1].reshape(nr * nt, 234)) < TOL


def test_host_pipeline_many_chunks_pinned_and_pageable(pkg, oracle):
    """The host-buffer entry points pipeline upload / kernels / download over packet chunks through two
    slots: many chunks (Nt=4, Nr=2: 8192-packet chunks -> use 20000 packets), caller buffers pageable
    or pinned (csi_host_malloc), one or several copy threads - all bit-identical, and right on
    sampled packets."""
    rng = np.random.default_rng(123)
    nt, nr, npkt, hidden = 4, 2, 20000, (32, 16)
    w_re, w_im = _weights(oracle, 77, nt, hidden)
    P = oracle.hadamard(nt)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P)
    re = rng.standard_normal((npkt, nr, 320 * nt), dtype=np.float32)
    im = rng.standard_normal((npkt, nr, 320 * nt), dtype=np.float32)
    o_re, o_im = e.predict(re, im)
    h = e.ls_estimate(re, im)
    sel = np.r_[0:2, 8191:8194, npkt - 2:npkt]
    ltf = (re[sel] + 1j * im[sel]).astype(np.complex64)
    r_re, r_im = oracle.predict_packets(ltf, P, w_re, w_im, np.float64, pkt_batch=len(sel))
    assert rel_rows(o_re[sel], r_re) < TOL and rel_rows(o_im[sel], r_im) < TOL
    ref = oracle.ls_estimate(ltf, P)
    assert rel_rows(np.concatenate([h[sel].real, h[sel].imag], -1), np.concatenate([ref.real, ref.imag], -1)) < TOL
    # pinned caller buffers, and a different number of copy threads
    p_re, p_im = e.pinned_empty(re.shape), e.pinned_empty(im.shape)
    p_re[...] = re
    p_im[...] = im
    out = (e.pinned_empty(o_re.shape), e.pinned_empty(o_im.shape))
    q_re, q_im = e.predict(p_re, p_im, out=out)
    assert q_re is out[0] and np.array_equal(q_re, o_re) and np.array_equal(q_im, o_im)
    e.set_option('host_threads', 1)
    s_re, s_im = e.predict(re, im)
    assert np.array_equal(s_re, o_re) and np.array_equal(s_im, o_im)
    hp = e.ls_estimate(re, im, out=(np.empty(o_re.shape, np.float32), np.empty(o_re.shape, np.float32)))
    assert np.array_equal(hp[0], h.real) and np.array_equal(hp[1], h.imag)


# ------------------------------------------------------------------------------------ device path
def test_estimate_c128_matches_plane_entry_points(pkg, oracle):
    """csi_estimate_c128 - complex128 preambles in, complex64 DNN and LS estimates out, one upload, the real / imag
    split and the complex assembly inside the pipeline's staging copies - must return exactly what csi_predict and
    csi_ls_estimate return for the float32 planes of the same packets: many chunks (Nt=4, Nr=2: 8192-packet chunks),
    a ragged last chunk, either output alone, caller-provided buffers, and the deployment wrapper on top of it."""
    rng = np.random.default_rng(21)
    nt, nr, npkt, hidden = 4, 2, 20011, (64, 32)
    w_re, w_im = _weights(oracle, 21, nt, hidden)
    P = _pilot(rng, nt)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P)
    x = (rng.standard_normal((npkt, nr, 320 * nt)) + 1j * rng.standard_normal((npkt, nr, 320 * nt)))        # complex128
    p_re, p_im = e.predict(x)
    h = e.ls_estimate(x)
    dnn, ls = e.estimate(x)
    assert dnn.dtype == np.complex64 and dnn.shape == (npkt, nr, nt, 234) and ls.dtype == np.complex64
    np.testing.assert_array_equal(dnn.real, p_re)
    np.testing.assert_array_equal(dnn.imag, p_im)
    np.testing.assert_array_equal(ls, h)
    only_ls = e.estimate(x[:700], dnn=False)
    assert only_ls[0] is None
    np.testing.assert_array_equal(only_ls[1], h[:700])
    buf = np.zeros((3, nr, nt, 234), np.complex64)
    got, none = e.estimate(x[5:8], ls=False, out=(buf, None))
    assert got is buf and none is None
    np.testing.assert_array_equal(buf.real, e.predict(x[5:8])[0])        # (a 3-packet call takes other kernels than the big batch)
    r_re, r_im = oracle.predict_packets(x[:4].astype(np.complex64), P, w_re, w_im, np.float64, pkt_batch=4)
    assert rel_rows(dnn[:4].real, r_re) < TOL and rel_rows(dnn[:4].imag, r_im) < TOL
    with pytest.raises(pkg.CsiError):
        e.estimate(x[:2], dnn=False, ls=False)
    with pytest.raises(pkg.CsiError):
        e.estimate(x[:2, :1])


def test_device_resident_path_and_profile(pkg, oracle):
    rng = np.random.default_rng(41)
    nt, nr, npkt, hidden = 8, 2, 16, (64, 64)
    w_re, w_im = _weights(oracle, 23, nt, hidden)
    P = _pilot(rng, nt)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P)
    d_re, d_im = e.empty((npkt, nr, e.len_ltf)), e.empty((npkt, nr, e.len_ltf))
    e.synth_white(2024, 0, npkt, d_re, d_im)
    d_ore, d_oim = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
    d_hre, d_him = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
    e.profile_enable(True)
    e.profile_reset()
    e.predict_device(d_re, d_im, npkt, d_ore, d_oim)
    e.ls_estimate_device(d_re, d_im, npkt, d_hre, d_him)
    e.synchronize()
    prof = e.profile()
    # round 5: a call of 32 preambles / 256 pair rows takes the one-packet path - ONE launch per layer for both component models
    per_layer = 1 if e.get_option('small_calls') == 1 else 2
    assert prof['pair_dense_gemm']['launches'] == per_layer and prof['pair_dense_gemm']['ms'] > 0
    assert prof['ls_estimate']['launches'] == 1 and prof['regressor_gemm']['launches'] == per_layer
    ltf = d_re.download() + 1j * d_im.download()
    # white generator: unit-variance circular Gaussian, reproducible, offset-consistent
    assert abs(np.mean(np.abs(ltf) ** 2) - 1.0) < 0.02 and abs(np.mean(ltf)) < 0.01
    d_re2, d_im2 = e.empty((4, nr, e.len_ltf)), e.empty((4, nr, e.len_ltf))
    e.synth_white(2024, 5, 4, d_re2, d_im2)
    np.testing.assert_array_equal(d_re2.download(), ltf.real[5:9].astype(np.float32))
    r_re, r_im = oracle.predict_packets(ltf, P, w_re, w_im, np.float64, pkt_batch=npkt)
    assert rel_rows(d_ore.download(), r_re) < TOL and rel_rows(d_oim.download(), r_im) < TOL
    ref_ls = oracle.ls_estimate(ltf, P)
    assert rel_rows(d_hre.download(), ref_ls.real) < TOL and rel_rows(d_him.download(), ref_ls.imag) < TOL


def test_hipgraph_replay_matches_eager(pkg, oracle):
    """use_graph: the 2nd identical csi_predict_device call is captured, later ones replay the
    hipGraph.  Results must equal the eager ones bit for bit, follow new input data written into
    the same buffers, and survive a re-allocation (larger batch) and a weight reload."""
    rng = np.random.default_rng(5)
    nt, nr, npkt, hidden = 8, 2, 6, (256, 64)
    w_re, w_im = _weights(oracle, 41, nt, hidden)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, _pilot(rng, nt))
    a = pkg.synth.white_packets(rng, npkt, nr, nt)
    b = pkg.synth.white_packets(rng, npkt, nr, nt)
    d_re, d_im = e.to_device(a.real), e.to_device(a.imag)
    o_re, o_im = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
    e.predict_device(d_re, d_im, npkt, o_re, o_im); e.synchronize()
    eager_a = (o_re.download(), o_im.download())
    eager_b = e.predict(b)
    e.set_option('use_graph', 1)
    for it in range(4):                       # eager, capture, replay, replay
        o_re.upload(np.zeros((npkt, nr, nt, 234), np.float32))
        e.predict_device(d_re, d_im, npkt, o_re, o_im); e.synchronize()
        np.testing.assert_array_equal(o_re.download(), eager_a[0])
        np.testing.assert_array_equal(o_im.download(), eager_a[1])
    d_re.upload(b.real); d_im.upload(b.imag)  # same pointers, new data -> the graph must see it
    e.predict_device(d_re, d_im, npkt, o_re, o_im); e.synchronize()
    np.testing.assert_array_equal(o_re.download(), eager_b[0])
    big = pkg.synth.white_packets(rng, 40, nr, nt)      # forces a workspace re-allocation
    e.predict(big)
    e.predict_device(d_re, d_im, npkt, o_re, o_im); e.synchronize()
    np.testing.assert_array_equal(o_im.download(), eager_b[1])
    w2_re, w2_im = _weights(oracle, 42, nt, hidden)     # new weights drop the cached graphs
    e.load_weights('real', w2_re); e.load_weights('imag', w2_im)
    for it in range(3):
        e.predict_device(d_re, d_im, npkt, o_re, o_im); e.synchronize()
    e.set_option('use_graph', 0)
    ref = e.predict(b)
    np.testing.assert_array_equal(o_re.download(), ref[0])
    np.testing.assert_array_equal(o_im.download(), ref[1])
    with pytest.raises(pkg.CsiError):
        e.set_option('no_such_option', 1)


def test_hipgraph_config5_scale_multi_chunk(pkg, oracle):
    """BASELINE configs[4] shape (Nt=128, Nr=16, shipped model, "hipGraph-captured batched inference"): 520 packets =
    1 064 960 pair rows per component model, more than the 4 GiB workspace holds, so one call is TWO packet chunks
    - LS kernel, range-guard memsets, magnitude sample, layer 0 (K = 40 960), slab sum, per-pair layer, regressor,
    x 2 models x 2 chunks in ONE captured graph (csi_estimate_device).  Replays must reproduce the eager results bit
    for bit, follow new data in the same buffers, keep the split engine's range-guard bookkeeping alive, and the
    sampled packets must meet the contract."""
    nt, nr, npkt, hidden = 128, 16, 520, (1024, 1024)
    w_re, w_im = _weights(oracle, 128, nt, hidden)
    P = oracle.hadamard(nt)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P)
    d_re, d_im = e.empty((npkt, nr, e.len_ltf)), e.empty((npkt, nr, e.len_ltf))
    e.synth_white(55, 0, npkt, d_re, d_im)
    outs = [e.empty((npkt, nr, nt, 234)) for _ in range(4)]            # dnn re, dnn im, ls re, ls im
    e.estimate_device(d_re, d_im, npkt, *outs)
    e.synchronize()
    eager = [o.download() for o in outs]
    n_eager = e.get_option('hs_launches')
    assert n_eager >= 2 * 2 * 2                                          # two chunks x two models x (layer 0, pair layer + regressor [one band kernel])
    e.set_option('use_graph', 1)
    for it in range(4):                                                  # eager, capture, replay, replay
        for o in outs:
            e._check(e._lib.csi_memcpy_h2d(e._ctx, o.ptr, np.zeros(1024, np.float32).ctypes.data, 4096))    # dirty the heads
        before = e.get_option('hs_launches')
        e.estimate_device(d_re, d_im, npkt, *outs)
        e.synchronize()                                                  # range guard checked after replays too
        assert e.get_option('hs_launches') - before == n_eager
        for o, ref in zip(outs, eager):
            np.testing.assert_array_equal(o.download(), ref)
    assert e.get_option('graph_replays') == 2
    # new data in the same buffers: the graph reads it (and the magnitude sample re-derives the input scale)
    e.synth_white(56, 0, npkt, d_re, d_im)
    e.estimate_device(d_re, d_im, npkt, *outs)
    e.synchronize()
    assert e.get_option('graph_replays') == 3
    pick = [0, 259, 260, npkt - 1]                                       # both sides of the chunk boundary
    for p in pick:
        ltf = d_re.download(p, 1) + 1j * d_im.download(p, 1)
        r_re, r_im = oracle.predict_packets_shared(ltf, P, w_re, w_im)
        assert rel_rows(outs[0].download(p, 1), r_re) < TOL and rel_rows(outs[1].download(p, 1), r_im) < TOL, p
        ref = oracle.ls_estimate(ltf, P)
        assert rel_rows(np.concatenate([outs[2].download(p, 1), outs[3].download(p, 1)], -1), np.concatenate([ref.real, ref.imag], -1)) < TOL, p
    # a range-guard hit inside a replayed graph is still reported
    e.set_option('use_graph', 0)
    e.set_option('use_graph', 1)
    big = e.empty((4, nr, e.len_ltf))
    big.upload(np.full((4, nr, e.len_ltf), 3.0e4, np.float32))
    o4 = [e.empty((4, nr, nt, 234)) for _ in range(4)]
    e.set_option('f32_engine', 1)
    hits = 0
    for it in range(3):
        e.estimate_device(big, big, 4, *o4)
        try:
            e.synchronize()
        except pkg.CsiError as err:
            assert err.code == -6
            hits += 1
    assert hits == 3 and e.get_option('graph_replays') == 4


def test_host_pipeline_modes_agree(pkg, oracle):
    """The host-buffer entry points with the staging on side threads (default), inline on the caller (round 3's arrangement) and
    with small pipeline slots: identical bits, on pageable and on caller-pinned buffers, planes and complex128 surface."""
    rng = np.random.default_rng(8)
    nt, nr, npkt, hidden = 8, 2, 3000, (64, 64)            # 3000 packets x 20 KB: several chunks at every slot size
    w_re, w_im = _weights(oracle, 5, nt, hidden)
    P = oracle.hadamard(nt)
    ltf = (rng.standard_normal((npkt, nr, 320 * nt)) + 1j * rng.standard_normal((npkt, nr, 320 * nt))).astype(np.complex128)
    e = pkg.CsiEngine(nt, nr, hidden=hidden)
    e.load_weights('real', w_re)
    e.load_weights('imag', w_im)
    e.set_pilot(P)
    re, im = np.ascontiguousarray(ltf.real, np.float32), np.ascontiguousarray(ltf.imag, np.float32)
    ref_p = e.predict(re, im)
    ref_c = e.estimate(ltf)
    ref_l = e.ls_estimate(re, im)
    by_chunk = {}
    for side, chunk, threads in ((0, 0, 0), (1, 0, 8), (1, 100, 3), (0, 100, 2), (1, 37, 0), (0, 37, 5)):
        e.set_option('hp_side_threads', side)
        e.set_option('hp_chunk_packets', chunk)
        e.set_option('host_threads', threads)
        p = e.predict(re, im)
        assert np.array_equal(p[0], ref_p[0]) and np.array_equal(p[1], ref_p[1]), (side, chunk, threads)     # the plane calls keep their own slot size
        assert np.array_equal(e.ls_estimate(re, im), ref_l)
        c = e.estimate(ltf)
        assert e.get_option('hp_total_us') > 0
        # the slot size decides how many packets one kernel launch sees (engine choice, data-derived input scale): bit-identical for
        # the same slot size whoever does the staging, inside the contract of each other across slot sizes
        if chunk in by_chunk:
            assert np.array_equal(c[0], by_chunk[chunk][0]) and np.array_equal(c[1], by_chunk[chunk][1]), (side, chunk, threads)
        by_chunk[chunk] = c
        if chunk == 0:
            assert np.array_equal(c[0], ref_c[0]) and np.array_equal(c[1], ref_c[1])
        assert np.array_equal(c[1], ref_c[1])                                                            # LS: one kernel whatever the chunk
        cat = lambda z: np.concatenate([z.real, z.imag], -1)
        assert rel_rows(cat(c[0]), cat(ref_c[0])) < 5e-6, (side, chunk, threads)
    pr, pi = e.pinned_empty(re.shape), e.pinned_empty(im.shape)
    pr[...] = re; pi[...] = im
    po = (e.pinned_empty(ref_p[0].shape), e.pinned_empty(ref_p[1].shape))
    e.predict(pr, pi, out=po)
    assert np.array_equal(po[0], ref_p[0]) and np.array_equal(po[1], ref_p[1])
    k = 3
    r_re, r_im = oracle.predict_packets(ltf[:k].astype(np.complex64), P, w_re, w_im, np.float64, pkt_batch=k)
    assert rel_rows(ref_p[0][:k], r_re) < TOL and rel_rows(ref_c[0][:k].imag, r_im) < TOL


def test_profile_entry_points(pkg, oracle):
    """csi_profile_band_skeleton / csi_profile_pcie: plausible numbers, arguments checked, the context still right afterwards."""
    rng = np.random.default_rng(2)
    nt, nr, hidden = 32, 4, (1024, 1024)
    w_re, w_im = _weights(oracle, 77, nt, hidden)
    e = pkg.CsiEngine(nt, nr, hidden=hidden)
    with pytest.raises(pkg.CsiError):
        e.band_skeleton(4096)                                 # nothing loaded
    e.load_weights('real', w_re)
    e.load_weights('imag', w_im)
    e.set_pilot(oracle.hadamard(nt))
    ltf = oracle.make_structured_packets(rng, 40, nr, oracle.hadamard(nt), snr_db=0.0)[0].astype(np.complex64)
    e.set_option('f32_engine', 1)
    a = e.predict(ltf)
    ms, tf = e.band_skeleton(65536, 3)
    assert 0.05 < ms < 5.0 and 300.0 < tf < 2500.0, (ms, tf)   # 512 bands = 2 rounds of 256 CUs: a fraction of a millisecond
    b = e.predict(ltf)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    up, down, both = e.pcie_probe(256 << 20, 128 << 20)
    assert up > 0 and down > 0 and max(up, down) * 0.9 <= both <= (up + down) * 1.2
    assert 10.0 < (256 << 20) / up / 1e6 < 80.0                 # GB/s of a PCIe Gen5 x16 link
    with pytest.raises(pkg.CsiError):
        e.pcie_probe(0, 0)
    e2 = pkg.CsiEngine(8, 2, hidden=(64,))
    with pytest.raises(pkg.CsiError):
        e2.band_skeleton(1024)


def test_engine_close_frees_its_device_arrays(pkg, oracle):
    """A DeviceArray that is still alive when its engine closes is freed by close() (it used to survive as leaked HBM: a probe that made
    a fresh engine per cycle ran a 288 GB part out of memory), and freeing it again afterwards is harmless."""
    e = pkg.CsiEngine(4, 2, hidden=(8,))
    a = e.empty((3, 5))
    b = e.to_device(np.arange(12, dtype=np.float32).reshape(3, 4))
    assert a.ptr and b.ptr
    np.testing.assert_array_equal(b.download(), np.arange(12, dtype=np.float32).reshape(3, 4))
    e.close()
    assert a.ptr == 0 and b.ptr == 0
    a.free()
    e.close()


def test_estimate_c128_into_pinned_result_arrays(pkg, oracle):
    """csi_estimate_c128 with result arrays in pinned host memory (engine.pinned_empty(shape, np.complex64)): the complex values are
    assembled on the device (weave_c64_kernel) and the downloads land in the caller's arrays themselves - same bits as with pageable
    arrays (host threads weave out of the staging buffer), several chunks with the short first / last ones, either estimator alone,
    both pipeline arrangements, and `hp_device_weave` = 0 puts the host weave back."""
    rng = np.random.default_rng(12)
    nt, nr, npkt, hidden = 8, 2, 700, (64, 64)
    w_re, w_im = _weights(oracle, 6, nt, hidden)
    P = oracle.hadamard(nt)
    ltf = (rng.standard_normal((npkt, nr, 320 * nt)) + 1j * rng.standard_normal((npkt, nr, 320 * nt))).astype(np.complex128)
    e = pkg.CsiEngine(nt, nr, hidden=hidden)
    e.load_weights('real', w_re)
    e.load_weights('imag', w_im)
    e.set_pilot(P)
    shape = (npkt, nr, nt, 234)
    assert e.get_option('hp_device_weave') == 1
    for chunk, side in ((0, 1), (96, 1), (96, 0), (37, 1)):
        e.set_option('hp_chunk_packets', chunk)
        e.set_option('hp_side_threads', side)
        ref = e.estimate(ltf)                                                    # pageable result arrays: host weave
        n0 = e.get_option('hp_direct_out_calls')
        po = (e.pinned_empty(shape, np.complex64), e.pinned_empty(shape, np.complex64))
        po[0][...] = np.nan
        po[1][...] = np.nan
        got = e.estimate(ltf, out=po)
        assert got[0] is po[0] and got[1] is po[1]
        assert e.get_option('hp_direct_out_calls') == n0 + 1, (chunk, side)
        assert np.array_equal(po[0], ref[0]) and np.array_equal(po[1], ref[1]), (chunk, side)
        only_dnn = e.pinned_empty(shape, np.complex64)
        e.estimate(ltf, ls=False, out=(only_dnn, None))
        only_ls = e.pinned_empty(shape, np.complex64)
        e.estimate(ltf, dnn=False, out=(None, only_ls))
        assert np.array_equal(only_dnn, ref[0]) and np.array_equal(only_ls, ref[1]), (chunk, side)
        assert e.get_option('hp_direct_out_calls') == n0 + 3
        # one pinned, one pageable array: the host weave serves both
        mixed = (e.pinned_empty(shape, np.complex64), np.empty(shape, np.complex64))
        e.estimate(ltf, out=mixed)
        assert e.get_option('hp_direct_out_calls') == n0 + 3
        assert np.array_equal(mixed[0], ref[0]) and np.array_equal(mixed[1], ref[1])
    e.set_option('hp_device_weave', 0)
    n0 = e.get_option('hp_direct_out_calls')
    po = (e.pinned_empty(shape, np.complex64), e.pinned_empty(shape, np.complex64))
    e.estimate(ltf, out=po)
    assert e.get_option('hp_direct_out_calls') == n0
    assert np.array_equal(po[0], ref[0]) and np.array_equal(po[1], ref[1])
    k = 3
    r_re, r_im = oracle.predict_packets(ltf[:k].astype(np.complex64), P, w_re, w_im, np.float64, pkt_batch=k)
    assert rel_rows(ref[0][:k].real, r_re) < TOL and rel_rows(ref[0][:k].imag, r_im) < TOL


def test_estimate_c64_is_bit_identical_with_the_c128_call(pkg, oracle):
    """csi_estimate_c64 (round-4 verdict, next 7): a complex64 batch uploaded as it is and split on the device.  On values that single
    precision represents it must return the bits of csi_estimate_c128 - pageable and pinned input, pageable and pinned result arrays,
    either estimator alone, several pipeline slot sizes (short first / last chunks) - and both agree with the fp64 oracle."""
    nt, nr, hidden, npkt = 8, 2, (64, 64), 150
    rng = np.random.default_rng(64)
    w_re, w_im = _weights(oracle, 640, nt, hidden)
    P = oracle.hadamard(nt)
    x64 = oracle.make_structured_packets(rng, npkt, nr, P, snr_db=3.0)[0].astype(np.complex64)
    x128 = x64.astype(np.complex128)                                   # the same values, widened
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P)
    r_re, r_im = oracle.predict_packets(x64[:3], P, w_re, w_im, np.float64, pkt_batch=3)
    xp = e.pinned_empty(x64.shape, np.complex64)
    xp[...] = x64
    for chunk in (0, 7, 64, 149):
        e.set_option('hp_chunk_packets', chunk)
        # the complex128 call on the same schedule (a chunk's size picks its kernels - split-K factors, the one-packet path - so the bits
        # of two schedules differ by rounding; the two ENTRY POINTS on one schedule must not differ at all)
        ref_dnn, ref_ls = e.estimate(x128)
        assert rel_rows(ref_dnn[:3].real, r_re) < TOL and rel_rows(ref_dnn[:3].imag, r_im) < TOL
        for src in (x64, xp):
            dnn, ls = e.estimate(src)
            assert dnn.dtype == np.complex64 and np.array_equal(dnn, ref_dnn) and np.array_equal(ls, ref_ls), (chunk, src is xp)
            dnn, ls = e.estimate(src, pinned_results=True)
            assert np.array_equal(dnn, ref_dnn) and np.array_equal(ls, ref_ls), (chunk, src is xp, 'pinned results')
            only, none = e.estimate(src, ls=False)
            assert none is None and np.array_equal(only, ref_dnn)
            none, only = e.estimate(src, dnn=False)
            assert none is None and np.array_equal(only, ref_ls)
    e.set_option('hp_chunk_packets', 0)
    with pytest.raises(pkg.CsiError):
        e.estimate(x64[:, :1])                                          # wrong shape
    # the reference's wrapper keeps its complex128 contract (inference.py:39-43)
    assert e.estimate(x128[:2])[0].dtype == np.complex64


def test_tensorflow_written_model_predicts_what_tensorflow_predicted(pkg):
    """The GPU half of the f-1 landing test: once `tools/make_tf_fixture.py` has been run on a TensorFlow host and its
    output committed under tests/golden/tf_written/, the HIP path loads TensorFlow's OWN checkpoint and SavedModel files and must reproduce
    TensorFlow's OWN `Model.predict` on the recorded batch at the 1e-5 contract - the one place the Dense / BatchNormalization arithmetic
    is pinned to the reference's framework instead of to the oracle's restatement of it.  Skips loudly until then."""
    import os
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'tf_written')
    if not os.path.exists(os.path.join(d, 'expected.npz')):
        pytest.skip('NO TensorFlow-written model files in tests/golden/tf_written/ (f-1 stays "partial"): run '
                    '`python tools/make_tf_fixture.py tests/golden/tf_written` on a TensorFlow 2.x host and commit the output')
    exp = np.load(os.path.join(d, 'expected.npz'))
    x = np.concatenate([exp['x_sig'][:, :, 0], exp['x_p']], axis=1).astype(np.float32)       # [Flatten(seq_in), seq_p], DNN.py:207-208
    nt = exp['x_p'].shape[1]
    for comp in ('real', 'imag'):
        for path in (os.path.join(d, comp + '_weights-improvement.hdf5'), os.path.join(d, comp + '_keras_model')):
            w = pkg.load_weight_file(path)
            hidden = tuple(int(w['fc_dense%d.bias' % i].shape[0]) for i in range(8) if 'fc_dense%d.bias' % i in w)
            e = pkg.CsiEngine(nt, 1, hidden=hidden, n_out=int(w['fc_regressor.bias'].shape[0]), use_bn=True)
            e.load_weights(comp, w)
            y = e.predict_samples(comp, x)
            assert rel_rows(y, exp[comp + '_y']) < TOL, (path, rel_rows(y, exp[comp + '_y']))
            e.close()
