"""On-box fine-tuning: csi_train_* against the oracle's fp64 restatement of the
keras training step, the python fit loop (EarlyStopping / ReduceLROnPlateau / AWGN schedule), and a
small end-to-end learning problem.  GPU tests call through the C-ABI."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_streams      # noqa: E402  (host replay of the trainer's random streams)


def _problem(oracle, rng, nt, hidden, B, n_out=234, use_bn=True):
    d_in = 321 * nt
    w = oracle.make_weights(rng, d_in, hidden, n_out, use_bn=use_bn)
    x = rng.standard_normal((B, d_in)).astype(np.float32)
    y = rng.standard_normal((B, n_out)).astype(np.float32)
    return w, x, y


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ------------------------------------------------------------------------------------ CPU: oracle self-checks
def test_oracle_gradients_match_finite_differences(oracle):
    """The fp64 restatement itself: analytic gradients of the BN(batch statistics) stack against
    central differences of the loss."""
    rng = np.random.default_rng(5)
    w, x, y = _problem(oracle, rng, 1, (12, 10), 16, n_out=6)
    w = {k: (np.asarray(v, np.float64) if k != 'bn_eps' else v) for k, v in w.items()}
    loss, g, _ = oracle.train_forward_backward(w, x, y)
    for name in ('fc_dense0.kernel', 'fc_dense1.bias', 'bn0.gamma', 'bn1.beta', 'fc_regressor.kernel'):
        idx = tuple(rng.integers(0, s) for s in w[name].shape)
        h = 1e-6
        wp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}
        wm = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}
        wp[name][idx] += h
        wm[name][idx] -= h
        fd = (oracle.train_forward_backward(wp, x, y)[0] - oracle.train_forward_backward(wm, x, y)[0]) / (2 * h)
        assert abs(fd - g[name][idx]) < 1e-6 * max(1.0, abs(fd)), (name, fd, g[name][idx])


def test_oracle_forward_backward_match_torch_autograd(oracle):
    """Independent cross-check of the oracle's hand-derived forward / backward (Dense, relu,
    BatchNormalization with batch statistics, dropout mask, mse) against PyTorch autograd in float64,
    and of its inference forward against torch's batch_norm in eval mode.  (PyTorch is a third
    implementation of the published layer definitions, not the reference - the Keras rows stay
    'parity unpinned'.)"""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(17)
    w, x, y = _problem(oracle, rng, 4, (24, 16), 32, n_out=10)
    w = {k: (np.asarray(v, np.float64) if k != 'bn_eps' else v) for k, v in w.items()}
    masks = [rng.random((32, 24)) >= 0.3, None]
    loss, g, stats = oracle.train_forward_backward(w, x, y, masks=masks, dropout=0.3)
    tw = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in w.items() if k != 'bn_eps'}
    h = torch.tensor(x, dtype=torch.float64)
    for i in range(2):
        a = torch.relu(h @ tw[f'fc_dense{i}.kernel'] + tw[f'fc_dense{i}.bias'])
        h = F.batch_norm(a, None, None, tw[f'bn{i}.gamma'], tw[f'bn{i}.beta'], training=True, eps=1e-3)
        if i == 0:
            h = torch.where(torch.tensor(masks[0]), h / (1.0 - 0.3), torch.zeros_like(h))
    out = h @ tw['fc_regressor.kernel'] + tw['fc_regressor.bias']
    tl = torch.mean((out - torch.tensor(y, dtype=torch.float64)) ** 2)
    tl.backward()
    assert abs(tl.item() - loss) < 1e-12 * max(1.0, loss)
    for k, gk in g.items():
        assert _rel(gk, tw[k].grad.numpy()) < 1e-10, k
    # inference mode
    ref = oracle.fc_forward(x.astype(np.float64), w, np.float64)
    h = torch.tensor(x, dtype=torch.float64)
    with torch.no_grad():
        for i in range(2):
            a = torch.relu(h @ tw[f'fc_dense{i}.kernel'] + tw[f'fc_dense{i}.bias'])
            h = F.batch_norm(a, torch.tensor(w[f'bn{i}.moving_mean']), torch.tensor(w[f'bn{i}.moving_variance']),
                             tw[f'bn{i}.gamma'], tw[f'bn{i}.beta'], training=False, eps=1e-3)
        out = h @ tw['fc_regressor.kernel'] + tw['fc_regressor.bias']
    assert _rel(ref, out.numpy()) < 1e-12


def test_trainer_schedule_logic(pkg):
    """noise schedule and batch assembly of the python loop (no GPU): DNN.py:97-100, dataGenerator.py:314."""
    tr = pkg.trainer
    assert abs(tr.noise_std_for(2.0, 0.0) - 1.0) < 1e-12
    assert abs(tr.noise_std_for(2.0, 20.0) - 0.1) < 1e-12
    X = [np.arange(12, dtype=np.float32).reshape(2, 6, 1), np.ones((2, 2), np.float32)]
    rows = tr.rows_from_batch(X)
    assert rows.shape == (2, 8) and rows[1, 0] == 6 and rows[1, 7] == 1

    class Gen:
        def __len__(self):
            return 1

        def __getitem__(self, b):
            return X, np.zeros((2, 3), np.float32), None
    assert abs(tr.average_signal_power(Gen()) - np.mean(np.arange(12.0).reshape(2, 6) ** 2)) < 1e-9


# ------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize('nt,hidden,B,use_bn', [(4, (64, 48), 64, True), (4, (40,), 33, True), (4, (64, 32, 24), 256, False),
                                                (8, (128, 128), 256, True)])
def test_train_step_matches_oracle(pkg, oracle, nt, hidden, B, use_bn):
    """noise and dropout off: loss, every gradient and the Adam update of three consecutive steps
    against the fp64 oracle (batch sizes that are not multiples of 32, widths that are not multiples
    of 32, with and without BatchNormalization)."""
    rng = np.random.default_rng(nt * 100 + B)
    w, x, y = _problem(oracle, rng, nt, hidden, B, use_bn=use_bn)
    e = pkg.CsiEngine(nt, 2, hidden=hidden, use_bn=use_bn)
    lr = 1e-3
    e.train_begin('real', weights=w, lr=lr, dropout=0.0, seed=1)
    ref = {k: np.asarray(v, np.float64) for k, v in w.items() if k != 'bn_eps'}
    state = oracle.adam_init(ref)
    for step in range(3):
        xs = x if step == 0 else (x + 0.1 * step).astype(np.float32)
        loss = e.train_step('real', xs, y, noise_std=0.0)
        rloss, ref_new, g = oracle.train_step_reference(ref, state, xs, y, lr=lr, use_bn=use_bn)
        assert abs(loss - rloss) < 2e-5 * max(1.0, rloss)
        for name, gk in g.items():
            assert _rel(e.train_get('real', 'grad:' + name), gk) < 2e-4, (step, name)
        for name in e.train_tensor_names():
            got = e.train_get('real', name)
            # Adam divides by sqrt(v): where |g| is at the fp32 noise level the update direction is arbitrary,
            # so compare with an absolute tolerance of a fraction of one full step
            assert np.max(np.abs(got - ref_new[name])) < 0.05 * lr * (step + 1) + 1e-6, (step, name)
            assert _rel(got, ref_new[name]) < 1e-4, (step, name)
        ref = ref_new
    # inference-mode loss of the trained parameters
    assert abs(e.train_eval('real', x, y) - oracle.eval_loss_reference(ref, x, y, use_bn=use_bn)) < 1e-4
    # commit: the inference model now predicts with the trained tensors
    e.train_end('real', commit=True)
    out = e.predict_samples('real', x[:8])
    wr = dict(ref)
    wr['bn_eps'] = 1e-3
    assert _rel(out, oracle.fc_forward(x[:8], wr, np.float64)) < 1e-4


@pytest.mark.gpu
def test_train_trajectory_follows_oracle(pkg, oracle):
    """40 consecutive steps from the same initial tensors (noise / dropout off): the loss curve and the
    running BatchNormalization statistics stay on the fp64 oracle's trajectory."""
    rng = np.random.default_rng(33)
    nt, hidden, B = 4, (64, 32), 128
    w, _, _ = _problem(oracle, rng, nt, hidden, B, n_out=16)
    d_in = 321 * nt
    A = (rng.standard_normal((d_in, 16)) / np.sqrt(d_in)).astype(np.float32)
    e = pkg.CsiEngine(nt, 1, hidden=hidden, n_out=16)
    e.train_begin('real', weights=w, lr=1e-3, dropout=0.0, seed=0)
    ref = {k: np.asarray(v, np.float64) for k, v in w.items() if k != 'bn_eps'}
    state = oracle.adam_init(ref)
    for step in range(40):
        x = rng.standard_normal((B, d_in)).astype(np.float32)
        y = (x @ A).astype(np.float32)
        loss = e.train_step('real', x, y)
        rloss, ref, _ = oracle.train_step_reference(ref, state, x, y, lr=1e-3)
        assert abs(loss - rloss) < 2e-4 * max(1.0, rloss), step
    for name in ('bn0.moving_mean', 'bn1.moving_variance', 'fc_regressor.kernel', 'fc_dense0.kernel'):
        assert _rel(e.train_get('real', name), ref[name]) < 2e-3, name
    e.train_end('real', commit=False)


@pytest.mark.gpu
def test_train_noise_and_dropout_statistics(pkg, oracle):
    """AWGN only on the LTF columns with the requested stddev; dropout keeps ~(1-p) of the units and
    the same mask is used forward and backward (gradient of dropped units is exactly zero);
    steps are reproducible for equal seeds.  Noise and masks are held against the host replay of the counter-based streams
    (tests/train_streams.py); tests/test_train_streams.py has the full stochastic step against the fp64 oracle."""
    rng = np.random.default_rng(9)
    nt, hidden, B = 4, (96, 64), 256
    w, x, y = _problem(oracle, rng, nt, hidden, B)
    losses = []
    for rep in range(2):
        e = pkg.CsiEngine(nt, 2, hidden=hidden)
        e.train_begin('imag', weights=w, lr=1e-4, dropout=0.5, seed=77)
        losses.append([e.train_step('imag', x, y, noise_std=0.3) for _ in range(3)])
        if rep == 0:
            g1 = e.train_get('imag', 'grad:fc_dense1.kernel')      # [96, 64]: rows = units of layer 0 after dropout
            dead = np.all(g1 == 0.0, axis=1)
            assert not dead.any()                                   # a unit is dropped per sample, not per batch
        e.train_end('imag', commit=False)
    assert losses[0] == losses[1]
    # the loss moves with the noise ...
    e = pkg.CsiEngine(nt, 2, hidden=hidden)
    e.train_begin('real', weights=w, lr=1e-9, dropout=0.0, seed=3)
    l0 = np.mean([e.train_step('real', x, y, noise_std=0.0) for _ in range(2)])
    l1 = np.mean([e.train_step('real', x, y, noise_std=3.0) for _ in range(2)])
    assert np.isfinite(l0) and np.isfinite(l1) and abs(l1 - l0) > 1e-4 * l0
    # ... which sits on the LTF columns only and has the requested stddev: what layer 0 read in the last step (step 4 of this
    # trainer) minus the rows is 3 x the replayed N(0,1) stream (tests/train_streams.py; its distribution is checked on the
    # host and the device's draws against it element by element in tests/test_train_streams.py)
    staged = e.train_staged_input('real', B).astype(np.float64)
    L = 320 * nt
    np.testing.assert_array_equal(staged[:, L:], x[:, L:])
    added = staged[:, :L] - x[:, :L]
    z_ref, radius = train_streams.input_noise(3, 4, B, 321 * nt, L, with_radius=True)
    z_ref = z_ref[:, :L]
    # 3 x the bound on the device's normal (16 ulp-units of the radius, derived in test_train_streams._noise_bound) + an ulp each for
    # the product and the sum
    tol = (3.0 * 16.0 * 2.0 ** -24 * np.maximum(radius[:, :L], 2.0 ** -10) + np.spacing(np.abs(staged[:, :L]).astype(np.float32))
           + np.spacing(np.abs(3.0 * z_ref).astype(np.float32)))
    assert np.all(np.abs(added - 3.0 * z_ref) <= tol)
    n = added.size
    assert abs(added.mean() / 3.0) * np.sqrt(n) < 4.0 and abs(np.mean((added / 3.0) ** 2) - 1.0) / np.sqrt(2.0 / n) < 4.0
    e.train_end('real', commit=False)
    # dropout, per sample: a batch of two rows without BatchNormalization.  The replayed mask says which units of layer 0 are
    # dropped in both rows (about a quarter at p = 0.5): exactly those (and units whose relu is off in every row where they
    # are kept) have an exactly zero row in grad:fc_dense1.kernel (forward mask) AND an exactly zero column in
    # grad:fc_dense0.kernel / entry in grad:fc_dense0.bias (the backward pass recomputes the same mask)
    wn = {k: v for k, v in w.items() if not k.startswith('bn') or k == 'bn_eps'}
    e = pkg.CsiEngine(nt, 2, hidden=hidden, use_bn=False)
    e.train_begin('real', weights=wn, lr=1e-4, dropout=0.5, seed=77)
    e.train_step('real', x[:2], y[:2], noise_std=0.0)
    keep = train_streams.dropout_masks(77, 1, 2, hidden, 0.5)[0]            # [2, 96]
    assert abs(keep.mean() - 0.5) < 4.0 * np.sqrt(0.25 / keep.size)
    a0 = x[:2].astype(np.float64) @ wn['fc_dense0.kernel'].astype(np.float64) + wn['fc_dense0.bias']
    on = keep & (a0 > 1e-3)                                                # kept and relu clearly on
    off = ~(keep & (a0 > -1e-3))                                           # dropped, or relu clearly off
    g1, g0, gb0 = (e.train_get('real', 'grad:' + k) for k in ('fc_dense1.kernel', 'fc_dense0.kernel', 'fc_dense0.bias'))
    dead, alive = off.all(axis=0), on.any(axis=0)
    assert dead.sum() >= 10 and alive.sum() >= 10 and (~keep).all(axis=0).sum() >= 10
    assert np.all(g1[dead] == 0.0) and np.all(g0[:, dead] == 0.0) and np.all(gb0[dead] == 0.0)
    assert np.all(np.any(g1[alive] != 0.0, axis=1)) and np.all(np.any(g0[:, alive] != 0.0, axis=0)) and np.all(gb0[alive] != 0.0)
    e.train_end('real', commit=False)


@pytest.mark.gpu
def test_fit_learns_a_linear_channel_map(pkg, oracle):
    """End to end: Glorot initialisation, AWGN schedule, EarlyStopping / ReduceLROnPlateau bookkeeping; the
    validation loss of a learnable target falls by more than 5x and the committed model reproduces it."""
    rng = np.random.default_rng(21)
    nt, nr, hidden, n_out = 4, 1, (64, 32), 16
    d_in = 321 * nt
    A = np.zeros((d_in, n_out), np.float32)           # the target depends on 48 of the 1284 inputs
    A[:48] = (rng.standard_normal((48, n_out)) / np.sqrt(48.0)).astype(np.float32)

    class Gen:
        def __init__(self, n, bs, seed):
            r = np.random.default_rng(seed)
            self.x = r.standard_normal((n, d_in)).astype(np.float32)
            self.x[:, 48:] *= 0.02            # weak nuisance columns (the oracle run of this problem learns 15x)
            self.y = (self.x @ A).astype(np.float32)
            self.bs = bs

        def __len__(self):
            return len(self.x) // self.bs

        def __getitem__(self, b):
            s = slice(b * self.bs, (b + 1) * self.bs)
            return [self.x[s, :320 * nt, None], self.x[s, 320 * nt:]], self.y[s], None

    e = pkg.CsiEngine(nt, nr, hidden=hidden, n_out=n_out)
    tr, va = Gen(2048, 256, 1), Gen(512, 256, 2)
    hist = pkg.trainer.fit(e, 'real', tr, va, epochs=60, lr=3e-3, dropout=0.05, method='default_SNR',
                           snr_levels=(40, 30), es_patience=25, rlr_patience=20, seed=4, verbose=False)
    assert min(hist['val_loss']) < 0.2 * hist['val_loss'][0], (hist['val_loss'][0], min(hist['val_loss']))
    assert len(hist['loss']) == len(hist['val_loss']) == len(hist['lr']) <= 60
    assert hist['best_val_loss'] == min(hist['val_loss'])
    rows = pkg.trainer.rows_from_batch(va[0][0])
    out = e.predict_samples('real', rows)
    assert abs(float(np.mean((out - va[0][1]) ** 2)) - hist['best_val_loss']) < 0.25 * hist['best_val_loss'] + 1e-6


@pytest.mark.gpu
def test_train_api_errors(pkg):
    e = pkg.CsiEngine(4, 2, hidden=(32,))
    with pytest.raises(pkg.CsiError):
        e.train_step('real', np.zeros((4, 1284), np.float32), np.zeros((4, 234), np.float32))     # no csi_train_begin
    e.train_begin('real', lr=1e-4)
    with pytest.raises(pkg.CsiError):
        e.train_get('real', 'no_such_tensor.kernel')
    e.train_end('real', commit=False)
    b = pkg.CsiEngine(4, 2, hidden=(32,), dtype='bf16')
    with pytest.raises(pkg.CsiError):
        b.train_begin('real', lr=1e-4)


@pytest.mark.gpu
def test_cli_train_then_test(pkg, oracle, tmp_path, capsys):
    """`--train` (pipe.sh:40) on a small pickle dataset writes <d>_weights-improvement.safetensors that the
    `--test` run (pipe.sh:47) then loads; the printed val_loss history is finite and the test run's loss
    is the mse of the trained model."""
    import pickle
    rng = np.random.default_rng(12)
    nt, nr, npkt, hidden = 4, 2, 24, (32, 16)
    P_rows = oracle.hadamard(nt)
    ltf, _ = oracle.make_structured_packets(rng, npkt, nr, P_rows, snr_db=20.0)
    y = oracle.ls_estimate(ltf, P_rows).reshape(npkt * nr * nt, 234)
    X = np.zeros((npkt * nr * nt, 2), dtype=int)
    LTF = {}
    for p in range(npkt):
        for r in range(nr):
            key = 900 + p * nr + r
            LTF[key] = {'real': ltf[p, r].real.copy(), 'imag': ltf[p, r].imag.copy()}
            for t in range(nt):
                X[p * nr * nt + r * nt + t] = [key, t]
    ds = {'X': X, 'y': {'real': y.real.copy(), 'imag': y.imag.copy()}, 'LTF': LTF, 'P': P_rows.T.copy(),
          'simParams': {'nTX': nt, 'nRX': nr}}
    with open(tmp_path / 'train.b', 'wb') as f:
        pickle.dump(ds, f)
    from dl_channel_estimation_mamimo_amd import cli
    work = tmp_path / 'model'
    rc = cli.main(['--train', '-x', str(tmp_path / 'train.b'), '-d', str(work), '--nn', '32', '16', '--useBN', '--bs', '16',
                   '--epochs', '3', '--method', 'default_SNR', '--valTrainRatio', '0.25', '--datasource', 'matlab_maMimo'])
    assert rc == 0
    out = capsys.readouterr().out
    assert out.count('Epoch 3/3') == 2 and 'val_loss' in out and 'Validation separate from Training' in out
    for d in ('real', 'imag'):
        w = pkg.load_weight_file(str(work / f'{d}_weights-improvement.safetensors'))
        assert w['fc_dense0.kernel'].shape == (321 * nt, 32) and np.isfinite(w['fc_regressor.kernel']).all()
        # ... and, like DNN.py:319, a Keras HDF5 checkpoint with the same tensors
        k = pkg.load_weight_file(str(work / f'{d}_weights-improvement.hdf5'))
        assert set(k) == set(w) and all(np.array_equal(k[n].ravel(), w[n].ravel()) for n in w)
    outdir = tmp_path / 'out'
    outdir.mkdir()
    rc = cli.main(['--test', '-x', str(tmp_path / 'train.b'), '--modeldir', str(work), '-d', str(outdir), '--nn', '32', '16',
                   '--useBN', '--datasource', 'matlab_maMimo'])
    assert rc == 0 and 'loss (mse vs labels)' in capsys.readouterr().out


def _dp_worker(rank, world, port, tmp, repo):
    """One rank of the data-parallel check (2 processes sharing GPU 0, gloo carrying the CUDA all-reduce)."""
    import os
    import sys
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    sys.path.insert(0, repo)
    import numpy as np
    import dl_channel_estimation_mamimo_amd as pkg
    pkg.dist.init_process_group('gloo')
    z = np.load(os.path.join(tmp, 'problem.npz'))
    w = {k: z[k] for k in z.files if k not in ('x', 'y')}
    x, y = z['x'], z['y']
    e = pkg.CsiEngine(4, 2, hidden=(48, 32), use_bn=False)
    e.train_begin('real', weights=w, lr=1e-3, dropout=0.0, seed=5)
    for step in range(2):
        xs = (x + 0.05 * step).astype(np.float32)
        e.train_backward('real', xs[rank::world], y[rank::world])
        e.synchronize()
        pkg.dist.all_reduce_device(*e.train_grads('real'), average=True)
        e.train_apply('real')
    out = e.train_weights('real')
    m = pkg.dist.all_reduce_mean_arrays({'a': np.full(3, float(rank), np.float32)})
    np.savez(os.path.join(tmp, f'rank{rank}.npz'), mean_probe=m['a'], **out)
    e.train_end('real', commit=False)


@pytest.mark.gpu
def test_data_parallel_step_equals_full_batch_step(pkg, oracle, tmp_path):
    """Two ranks, each on half of a batch: backward -> flat gradient all-reduce (mean) -> Adam gives every
    rank the parameters of the single-process step on the whole batch (model without BatchNormalization,
    whose statistics are per rank by design)."""
    import os
    import torch.multiprocessing as mp
    rng = np.random.default_rng(8)
    w, x, y = _problem(oracle, rng, 4, (48, 32), 64, use_bn=False)
    np.savez(tmp_path / 'problem.npz', x=x, y=y, **{k: v for k, v in w.items() if k != 'bn_eps'})
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mp.spawn(_dp_worker, args=(2, 29533, str(tmp_path), repo), nprocs=2, join=True)
    ref = {k: np.asarray(v, np.float64) for k, v in w.items() if k != 'bn_eps'}
    state = oracle.adam_init(ref)
    for step in range(2):
        _, ref, _ = oracle.train_step_reference(ref, state, (x + 0.05 * step).astype(np.float32), y, lr=1e-3, use_bn=False)
    r0, r1 = np.load(tmp_path / 'rank0.npz'), np.load(tmp_path / 'rank1.npz')
    assert np.allclose(r0['mean_probe'], 0.5)
    for k in ref:
        np.testing.assert_array_equal(r0[k], r1[k])            # identical parameters on both ranks
        assert np.max(np.abs(r0[k] - ref[k])) < 0.05 * 1e-3 * 2 + 1e-6 and _rel(r0[k], ref[k]) < 1e-4, k


@pytest.mark.gpu
def test_cli_train_under_torchrun_two_ranks(pkg, oracle, tmp_path):
    """`cli --train` launched the way the driver launches multi-GPU work (torch.distributed.run, one process
    per rank; here both ranks share GPU 0 and gloo carries the collectives): rank 0 writes the weights."""
    import os
    import pickle
    import subprocess
    import sys
    rng = np.random.default_rng(14)
    nt, nr, npkt = 4, 2, 32
    P_rows = oracle.hadamard(nt)
    ltf, _ = oracle.make_structured_packets(rng, npkt, nr, P_rows, snr_db=20.0)
    y = oracle.ls_estimate(ltf, P_rows).reshape(npkt * nr * nt, 234)
    X = np.zeros((npkt * nr * nt, 2), dtype=int)
    LTF = {}
    for p in range(npkt):
        for r in range(nr):
            key = 100 + p * nr + r
            LTF[key] = {'real': ltf[p, r].real.copy(), 'imag': ltf[p, r].imag.copy()}
            for t in range(nt):
                X[p * nr * nt + r * nt + t] = [key, t]
    ds = {'X': X, 'y': {'real': y.real.copy(), 'imag': y.imag.copy()}, 'LTF': LTF, 'P': P_rows.T.copy(),
          'simParams': {'nTX': nt, 'nRX': nr}}
    with open(tmp_path / 'train.b', 'wb') as f:
        pickle.dump(ds, f)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CSI_DIST_BACKEND='gloo', PYTHONPATH=repo)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', '29541', '-m', 'dl_channel_estimation_mamimo_amd.cli', '--train', '-x', str(tmp_path / 'train.b'),
           '-d', str(tmp_path / 'model'), '--nn', '32', '16', '--useBN', '--bs', '16', '--epochs', '2', '--method', 'default_SNR',
           '--valTrainRatio', '0.25', '--datasource', 'matlab_maMimo', '--onlyReal']
    res = subprocess.run(cmd, env=env, cwd=repo, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:]
    assert 'Epoch 2/2' in res.stdout and 'weights saved to' in res.stdout
    w = pkg.load_weight_file(str(tmp_path / 'model' / 'real_weights-improvement.safetensors'))
    assert np.isfinite(w['fc_dense0.kernel']).all()


@pytest.mark.gpu
def test_resident_dataset_steps_equal_host_row_steps(pkg, oracle):
    """The training set uploaded once + batches addressed by sample index (csi_train_set_dataset /
    csi_train_indexed) give bit-identical steps to batches assembled on the host by the generator twin -
    with AWGN and dropout on (the counter-based streams depend only on seed, step and position)."""
    rng = np.random.default_rng(40)
    nt, nr, npkt, hidden = 4, 2, 12, (32, 16)
    P_rows = rng.integers(-2, 3, (nt, nt)).astype(np.float64)           # generic pilot matrix, not symmetric
    n = npkt * nr * nt
    X = np.zeros((n, 2), dtype=int)
    LTF = {}
    for p in range(npkt):
        for r in range(nr):
            key = 7000 + 13 * (p * nr + r)
            LTF[key] = {'real': rng.standard_normal(320 * nt), 'imag': rng.standard_normal(320 * nt)}
            for t in range(nt):
                X[p * nr * nt + r * nt + t] = [key, t]
    ds = {'X': X, 'y': {'real': rng.standard_normal((n, 234)), 'imag': rng.standard_normal((n, 234))}, 'LTF': LTF,
          'P': P_rows.T.copy(), 'simParams': {'nTX': nt, 'nRX': nr}}
    w = oracle.make_weights(rng, 321 * nt, hidden, 234)
    results = []
    for resident in (False, True):
        e = pkg.CsiEngine(nt, nr, hidden=hidden)
        e.set_pilot(P_rows)
        gen = pkg.dataset.SampleGenerator(list(range(n)), ds, 'imag', batch_size=32, shuffle=True, seed=9)
        e.train_begin('imag', weights=w, lr=1e-3, dropout=0.2, seed=11)
        if resident:
            e.train_set_dataset('imag', *pkg.dataset.resident_arrays(ds, 'imag'))
        losses = []
        for b in range(len(gen)):
            if resident:
                losses.append(e.train_step_indexed('imag', gen.batch_ids(b), noise_std=0.3))
            else:
                Xb, yb, _ = gen[b]
                losses.append(e.train_step('imag', pkg.trainer.rows_from_batch(Xb), yb, noise_std=0.3))
        ev = e.train_eval_indexed('imag', gen.batch_ids(0)) if resident else e.train_eval('imag', pkg.trainer.rows_from_batch(gen[0][0]), gen[0][1])
        results.append((losses, ev, e.train_weights('imag')))
        e.train_end('imag', commit=False)
    assert results[0][0] == results[1][0] and results[0][1] == results[1][1]
    for k in results[0][2]:
        np.testing.assert_array_equal(results[0][2][k], results[1][2][k])
    e = pkg.CsiEngine(nt, nr, hidden=hidden)
    e.train_begin('real', lr=1e-3)
    with pytest.raises(pkg.CsiError):
        e.train_step_indexed('real', [0, 1, 2])                  # no dataset uploaded
    with pytest.raises(pkg.CsiError):
        e.train_set_dataset('real', *pkg.dataset.resident_arrays(ds, 'real'))      # pilot not set
