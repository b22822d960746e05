"""GPU tests of the hybrid beamforming weights (csi_hybrid_weights[_device], csrc/hybrid_weights.hip.h): SVD + orthogonal
matching pursuit per (packet, subcarrier) against a dictionary of array responses, BER_test_maMIMO_LTF.m:347-376.

The comparison is a REPLAY, not an index match: the reference's dictionary (random rays on an array whose response depends on
cos(el) sin(az) only) is full of near-duplicate columns, the best and the second-best metric are often within 1e-4 of each other,
and two correct runs in different precisions choose different indices in ~0.2 % of the items.  tests/hybrid_ref.py therefore follows
the GPU's own index sequence in fp64 and reports how far each choice falls short of the best metric, and the fp64 coefficients for
the GPU's index set.  The reference values are computed from the fp32 planes the library receives."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hybrid_ref as R      # noqa: E402

TOL = 1e-5                  # the project's fp32 contract against fp64
GAP_MIN = 3e-3              # items whose singular-value gap at the cut is smaller have no well-defined Fopt
RAY_SEED = 5

# (Nt, Nr, Ns, NtRF, rays, SNR dB, packets)
SHAPES = [(8, 4, 1, 1, 500, 10, 8), (8, 2, 1, 2, 64, -10, 8), (32, 4, 2, 4, 500, 0, 4), (32, 4, 4, 8, 500, -10, 3),
          (16, 4, 3, 5, 333, 0, 6), (64, 8, 4, 16, 256, 10, 2), (128, 16, 2, 4, 500, 10, 1)]
# the widths, antenna counts and caps beyond powers of two (hybrid_ref.NEW_SHAPES says what each row is for).  The context and the
# 64 KiB LDS request of the correlation kernel are accepted at Nt = 256, the stage's own limit, so the row at the cap stands as it is
SHAPES += R.NEW_SHAPES


def dictionary(pkg, nt, rays):
    az, el = pkg.synth.random_rays(np.random.default_rng(RAY_SEED), rays)
    return pkg.synth.steering_ula(nt, az, el).astype(np.complex64)


ls_csi = R.ls_csi           # the Hadamard pilot where Nt is a power of two, a seeded +-1 pilot elsewhere


def engine(pkg, nt, nr, At=None, **kw):
    e = pkg.CsiEngine(nt, nr, hidden=(8,), device=0, **kw)
    if At is not None:
        e.set_dictionary(At)
    return e


def check_items(tag, H, H_eval, At, ns, ntrf, fbb, idx, n_atoms, gain):
    """Checks 1 - 4 of the replay on items H [items][nr][nt] (complex128 of the fp32 input)."""
    At = np.asarray(At, np.complex128)
    rays = At.shape[1]
    # 3. index sanity first: the replay needs valid indices
    assert idx.min() >= 0 and idx.max() < rays, (tag, idx.min(), idx.max())
    srt = np.sort(idx, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), tag + ': an item chose the same column twice'
    assert (n_atoms == ntrf).all(), (tag, np.unique(n_atoms))
    short, fbb_ref = R.replay(H, At, ns, idx)
    # 1. selection: every step of every item
    print('%s: selection shortfall max %.3g (bound %.0e)' % (tag, short.max(), TOL))
    assert short.max() <= TOL, (tag, short.max())
    # 2. weights
    _, sv = R.fopt_of(H, ns)
    g = R.gap_at_cut(sv, ns)
    keep = g >= GAP_MIN
    left_out = 1.0 - keep.mean()
    T = R.weights_matrix(At, idx, fbb)
    T_ref = R.weights_matrix(At, idx, fbb_ref)
    ratio = R.projector_error(T, T_ref) / (TOL * np.maximum(1.0, 0.1 / g))
    print('%s: projector error / bound max %.3g, left out %.4f, smallest gap %.3g' % (tag, ratio[keep].max(), left_out, g.min()))
    assert left_out <= 0.01, (tag, left_out)
    assert ratio[keep].max() <= 1.0, (tag, ratio[keep].max())
    # 3. power
    pw = (np.abs(T) ** 2).sum((1, 2))
    print('%s: | |T|_F^2 - Ns | max %.3g' % (tag, np.abs(pw - ns).max()))
    assert np.abs(pw - ns).max() <= TOL, (tag, np.abs(pw - ns).max())
    # 4. gain from the GPU's own fbb, idx
    g_ref = R.gain(H_eval, T)
    err = np.abs(gain / g_ref - 1.0).max()
    print('%s: gain relative error max %.3g' % (tag, err))
    assert err <= TOL, (tag, err)


@pytest.mark.parametrize('nt,nr,ns,ntrf,rays,snr,npkt', SHAPES)
def test_hybrid_weights_replay(pkg, oracle, nt, nr, ns, ntrf, rays, snr, npkt):
    h = ls_csi(oracle, nt, nr, snr, npkt)
    rng = np.random.default_rng(3)
    h_eval = (h + 0.3 * (rng.standard_normal(h.shape) + 1j * rng.standard_normal(h.shape))).astype(np.complex64)
    At = dictionary(pkg, nt, rays)
    e = engine(pkg, nt, nr, At)
    n0 = e.get_option('hybrid_launches')
    w = e.hybrid_weights(h, ns=ns, ntrf=ntrf, h_eval=h_eval)
    assert e.get_option('hybrid_launches') == n0 + 1 + 2 * ntrf + 2
    assert w.fbb.shape == (npkt, 234, ns, ntrf) and w.idx.shape == (npkt, 234, ntrf) and w.frf_mean.shape == (npkt, ntrf, nt)
    H, He = R.csi_to_items(h), R.csi_to_items(h_eval)
    n = npkt * 234
    tag = 'Nt %d Nr %d Ns %d NtRF %d R %d' % (nt, nr, ns, ntrf, rays)
    check_items(tag, H, He, At, ns, ntrf, w.fbb.reshape(n, ns, ntrf), w.idx.reshape(n, ntrf), w.n_atoms.reshape(n), w.gain.reshape(n))
    # gain with h_eval NULL: against the input itself; nothing else changes
    w2 = e.hybrid_weights(h, ns=ns, ntrf=ntrf)
    assert np.array_equal(w2.fbb, w.fbb) and np.array_equal(w2.idx, w.idx)
    T = R.weights_matrix(At, w2.idx.reshape(n, ntrf), w2.fbb.reshape(n, ns, ntrf))
    err = np.abs(w2.gain.reshape(n) / R.gain(H, T) - 1.0).max()
    print('%s: gain (h_eval NULL) relative error max %.3g' % (tag, err))
    assert err <= TOL
    # frf_mean against the mean of At[:, idx]
    frf = pkg.frf_from_idx(At.astype(np.complex128), w.idx)          # [npkt][234][ntrf][nt]
    err = np.abs(w.frf_mean - frf.mean(axis=1)).max()
    print('%s: frf_mean absolute error max %.3g' % (tag, err))
    assert err <= 1e-6
    if ns == 1 and ntrf == 1:
        # 5. the reference's configuration against the closed form
        fopt, _ = R.fopt_of(H, 1)
        corr = np.abs(np.conj(At.astype(np.complex128)).T @ fopt[:, :, 0].T).T          # [items][rays]
        got = corr[np.arange(n), w.idx.reshape(n)]
        assert (1.0 - got / corr.max(axis=1)).max() <= TOL
        nrm = np.linalg.norm(At.astype(np.complex128)[:, w.idx.reshape(n)], axis=0)
        assert np.abs(np.abs(w.fbb.reshape(n)) * nrm - 1.0).max() <= TOL


def test_full_size_run_across_the_chunk_boundary(pkg, oracle):
    """Nt 32, Nr 4, 4000 packets through the device entry point, (1, 1) and (2, 4); the second needs more than the stage's default
    workspace limit and runs in two packet chunks.  Checked on a seeded sample of 2000 items."""
    nt, nr, npkt, rays = 32, 4, 4000, 500
    h = ls_csi(oracle, nt, nr, 0, npkt)
    At = dictionary(pkg, nt, rays)
    e = engine(pkg, nt, nr, At)
    d_re, d_im = e.to_device(np.ascontiguousarray(h.real)), e.to_device(np.ascontiguousarray(h.imag))
    n = npkt * 234
    pick = np.sort(np.random.default_rng(17).choice(n, 2000, replace=False))
    H = h[pick // 234, :, :, pick % 234].astype(np.complex128)          # [2000][nr][nt]
    for ns, ntrf in ((1, 1), (2, 4)):
        d_f = [e.empty((npkt, 234, ns, ntrf)) for _ in range(2)]
        d_idx, d_na, d_gain = e.empty((npkt, 234, ntrf)), e.empty((npkt, 234)), e.empty((npkt, 234))
        e.hybrid_weights_device(d_re, d_im, npkt, ns, ntrf, d_f[0], d_f[1], d_idx, d_na, d_gain)
        e.synchronize()
        fbb = (d_f[0].download() + 1j * d_f[1].download()).reshape(n, ns, ntrf)
        idx, na, gain = d_idx.download().view(np.int32).reshape(n, ntrf), d_na.download().view(np.int32).reshape(n), d_gain.download().reshape(n)
        assert idx.min() >= 0 and idx.max() < rays and (na == ntrf).all()
        check_items('4000 packets (%d, %d)' % (ns, ntrf), H, H, At, ns, ntrf, fbb[pick], idx[pick], na[pick], gain[pick])
        for d in d_f + [d_idx, d_na, d_gain]:
            d.free()


def test_known_answer_and_early_stop(pkg):
    """H = u a_17^H of rank one over a dictionary without duplicates: the first atom is column 17 and fits exactly, so the
    pursuit stops there (the fp32 residual, ~6e-8, is under the default stop_tol): one atom, the other slots empty."""
    nt, nr, npkt, k = 16, 4, 2, 17
    At = pkg.synth.steering_ula(nt, np.linspace(-80, 80, 64), 0.0).astype(np.complex64)
    rng = np.random.default_rng(2)
    u = rng.standard_normal((npkt, nr, 1, 234)) + 1j * rng.standard_normal((npkt, nr, 1, 234))
    h = (u * np.conj(At[:, k].astype(np.complex128))[None, None, :, None]).astype(np.complex64)
    e = engine(pkg, nt, nr, At)
    w = e.hybrid_weights(h, ns=1, ntrf=3)
    assert (w.idx[..., 0] == k).all()
    assert (w.n_atoms == 1).all()
    assert (w.idx[..., 1:] == -1).all()
    assert (w.fbb[..., 1:] == 0).all()
    hn = (np.abs(h.astype(np.complex128)) ** 2).sum((1, 2))          # |H|_F^2 per (packet, subcarrier)
    assert np.abs(w.gain / hn - 1.0).max() <= TOL
    # the empty slots add nothing to the mean of the analog part
    assert np.abs(w.frf_mean[:, 0] - At[:, k][None, :]).max() <= 1e-6 and (w.frf_mean[:, 1:] == 0).all()


def test_determinism_entry_points_and_call_split(pkg, oracle):
    nt, nr, ns, ntrf, npkt = 32, 4, 2, 4, 600
    rng = np.random.default_rng(23)
    h = (rng.standard_normal((npkt, nr, nt, 234)) + 1j * rng.standard_normal((npkt, nr, nt, 234))).astype(np.complex64)
    At = dictionary(pkg, nt, 500)
    e = engine(pkg, nt, nr, At)
    a = e.hybrid_weights(h, ns=ns, ntrf=ntrf)
    b = e.hybrid_weights(h, ns=ns, ntrf=ntrf)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # device-pointer entry point
    d_re, d_im = e.to_device(np.ascontiguousarray(h.real)), e.to_device(np.ascontiguousarray(h.imag))

    def device_call(first, count):
        d_f = [e.empty((count, 234, ns, ntrf)) for _ in range(2)]
        d_idx, d_na, d_gain = e.empty((count, 234, ntrf)), e.empty((count, 234)), e.empty((count, 234))
        d_m = [e.empty((count, ntrf, nt)) for _ in range(2)]
        s_re, s_im = e.to_device(np.ascontiguousarray(h.real[first:first + count])), e.to_device(np.ascontiguousarray(h.imag[first:first + count]))
        e.hybrid_weights_device(s_re, s_im, count, ns, ntrf, d_f[0], d_f[1], d_idx, d_na, d_gain, d_m[0], d_m[1])
        e.synchronize()
        return (d_f[0].download() + 1j * d_f[1].download()).astype(np.complex64), d_idx.download().view(np.int32), d_na.download().view(np.int32), \
            d_gain.download(), (d_m[0].download() + 1j * d_m[1].download()).astype(np.complex64)
    whole = device_call(0, npkt)
    for x, y in zip(a, whole):
        assert np.array_equal(x, y), 'host-pointer and device-pointer entry points differ'
    lo, hi = device_call(0, 300), device_call(300, 300)
    for x, y, z in zip(whole, lo, hi):
        assert np.array_equal(x, np.concatenate([y, z])), 'one call of 600 packets differs from two calls of 300'


def test_in_the_pipeline_eager_and_captured(pkg, oracle):
    """estimate_device followed by hybrid_weights_device on the DNN planes with h_eval = the LS planes: eager, and both calls
    inside one captured graph, same bits; the DNN and LS outputs are those of a call without the new stage."""
    nt, nr, npkt, hidden, ns, ntrf = 8, 2, 40, (64, 64), 1, 2
    rng = np.random.default_rng(0)
    w_re = oracle.make_weights(rng, 320 * nt + nt, list(hidden), 234)
    w_im = oracle.make_weights(rng, 320 * nt + nt, list(hidden), 234)
    P = oracle.hadamard(nt)
    ltf, _ = oracle.make_structured_packets(rng, npkt, nr, P, snr_db=5.0)
    At = dictionary(pkg, nt, 200)

    def make():
        e = pkg.CsiEngine(nt, nr, hidden=hidden, device=0)
        e.load_weights('real', w_re); e.load_weights('imag', w_im); e.set_pilot(P)
        return e
    e0 = make()
    d_in = [e0.to_device(np.ascontiguousarray(ltf.real, np.float32)), e0.to_device(np.ascontiguousarray(ltf.imag, np.float32))]
    d_o = [e0.empty((npkt, nr, nt, 234)) for _ in range(4)]
    e0.estimate_device(d_in[0], d_in[1], npkt, *d_o)
    e0.synchronize()
    base = [d.download() for d in d_o]

    e = make()
    e.set_dictionary(At)
    d_in = [e.to_device(np.ascontiguousarray(ltf.real, np.float32)), e.to_device(np.ascontiguousarray(ltf.imag, np.float32))]
    d_o = [e.empty((npkt, nr, nt, 234)) for _ in range(4)]
    d_f = [e.empty((npkt, 234, ns, ntrf)) for _ in range(2)]
    d_idx, d_na, d_gain = e.empty((npkt, 234, ntrf)), e.empty((npkt, 234)), e.empty((npkt, 234))
    d_m = [e.empty((npkt, ntrf, nt)) for _ in range(2)]
    outs = d_o + d_f + [d_idx, d_na, d_gain] + d_m

    def calls():
        e.estimate_device(d_in[0], d_in[1], npkt, *d_o)
        e.hybrid_weights_device(d_o[0], d_o[1], npkt, ns, ntrf, d_f[0], d_f[1], d_idx, d_na, d_gain, d_m[0], d_m[1], d_eval_re=d_o[2], d_eval_im=d_o[3])
    calls()
    e.synchronize()
    eager = [d.download() for d in outs]
    for x, y in zip(base, eager[:4]):
        assert np.array_equal(x, y), 'the new stage changed the estimate in front of it'
    assert np.isfinite(eager[4]).all() and (eager[7].view(np.int32) >= 1).all()
    # the eager weights are right (gain against the LS planes from the GPU's own fbb, idx)
    dnn = (eager[0] + 1j * eager[1]).astype(np.complex64)
    ls = (eager[2] + 1j * eager[3]).astype(np.complex64)
    n = npkt * 234
    fbb, idx = (eager[4] + 1j * eager[5]).reshape(n, ns, ntrf), eager[6].view(np.int32).reshape(n, ntrf)
    T = R.weights_matrix(At, idx, fbb)
    assert np.abs(eager[8].reshape(n) / R.gain(R.csi_to_items(ls), T) - 1.0).max() <= TOL
    short, _ = R.replay(R.csi_to_items(dnn), At, ns, idx)
    assert short.max() <= TOL
    for d in outs:
        d.upload(np.zeros(d.shape, np.float32))
    e.capture_begin()
    try:
        calls()
    finally:
        graph = e.capture_end()
    e.synchronize()
    for _ in range(2):
        graph.launch()
    e.synchronize()
    for x, d in zip(eager, outs):
        assert np.array_equal(x, d.download()), 'the captured graph does not reproduce the eager bits'
    graph.free()


def test_refusals(pkg):
    nt, nr = 8, 2
    h = np.ones((1, nr, nt, 234), np.complex64)
    e = engine(pkg, nt, nr)
    with pytest.raises(pkg.CsiError, match='no dictionary set'):
        e.hybrid_weights(h)
    with pytest.raises(pkg.CsiError, match=r'dictionary must be \[Nt=8\]'):
        e.set_dictionary(np.ones((16, 64), np.complex64))
    e.set_dictionary(dictionary(pkg, nt, 64))
    with pytest.raises(pkg.CsiError, match='ns 2 outside 1 .. min'):
        e.hybrid_weights(h, ns=2, ntrf=1)
    with pytest.raises(pkg.CsiError, match='ntrf 17 outside'):
        e.hybrid_weights(h, ns=1, ntrf=17)
    with pytest.raises(pkg.CsiError, match='ns 0 outside'):
        e.hybrid_weights(h, ns=0, ntrf=1)
    e32 = engine(pkg, 32, 4, dictionary(pkg, 32, 64))
    with pytest.raises(pkg.CsiError, match='ntrf 17 outside 1 .. min'):
        e32.hybrid_weights(np.ones((1, 4, 32, 234), np.complex64), ns=1, ntrf=17)
    eb = pkg.CsiEngine(32, 4, hidden=(256, 256), device=0, dtype='bf16')
    eb.set_dictionary(dictionary(pkg, 32, 64))
    with pytest.raises(pkg.CsiError, match='fp32 contexts only'):
        eb.hybrid_weights(np.ones((1, 4, 32, 234), np.complex64))
    ew = engine(pkg, 4, 8)
    ew.set_dictionary(dictionary(pkg, 4, 16))
    with pytest.raises(pkg.CsiError, match='Nr 8 > Nt 4'):
        ew.hybrid_weights(np.ones((1, 8, 4, 234), np.complex64))
    # kernel names of the stage
    lib = pkg.load_library()
    names = [lib.csi_profile_kernel_name(i).decode() for i in range(lib.csi_profile_num_kernels())]
    assert {'hybrid_svd', 'hybrid_corr_argmax', 'hybrid_solve', 'hybrid_finish'} <= set(names)


def test_cli_hybrid_weights(pkg, oracle, tmp_path, capsys):
    """`--test --hybridWeights 64` on a miniature dataset: the per-packet files and the dictionary are written and replay."""
    import pickle
    from scipy.io import loadmat
    rng = np.random.default_rng(77)
    nt, nr, npkt, hidden, ns = 8, 2, 3, (64, 32), 2
    P_rows = oracle.hadamard(nt)
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
    ds = {'X': X, 'y': {'real': y.real.copy(), 'imag': y.imag.copy()}, 'LTF': LTF, 'P': P_rows.T.copy(), 'simParams': {'nTX': nt, 'nRX': nr}}
    with open(tmp_path / 'test.b', 'wb') as f:
        pickle.dump(ds, f)
    w_re = oracle.make_weights(rng, 320 * nt + nt, list(hidden), 234)
    w_im = oracle.make_weights(rng, 320 * nt + nt, list(hidden), 234)
    model_dir, work = tmp_path / 'model', tmp_path / 'out'
    model_dir.mkdir(); work.mkdir()
    pkg.save_weight_file(str(model_dir / 'real_weights-improvement.safetensors'), w_re)
    pkg.save_weight_file(str(model_dir / 'imag_weights-improvement.safetensors'), w_im)
    from dl_channel_estimation_mamimo_amd import cli
    rc = cli.main(['--test', '-x', str(tmp_path / 'test.b'), '--modeldir', str(model_dir), '-d', str(work), '--nn', '64', '32', '--useBN',
                   '--datasource', 'matlab_maMimo', '--valSameTrain', '--hybridWeights', '64', '--numSTS', str(ns)])
    assert rc == 0
    assert 'hybrid weights: 64 rays' in capsys.readouterr().out
    At = loadmat(str(work / 'hybrid_dictionary.mat'))['At']
    assert At.shape == (nt, 64)
    for n in range(npkt):
        assert os.path.exists(str(work / f'test_csi_predictions_real_{n + 1}.mat'))
        m = loadmat(str(work / f'hybrid_weights_{n + 1}.mat'))
        dnn = (loadmat(str(work / f'test_csi_predictions_real_{n + 1}.mat'))['all_pkts_csi_nn_out'][0, 0]['y']
               + 1j * loadmat(str(work / f'test_csi_predictions_imag_{n + 1}.mat'))['all_pkts_csi_nn_out'][0, 0]['y'])
        H = R.csi_to_items(dnn.reshape(1, nr, nt, 234).astype(np.complex64))
        H_ls = R.csi_to_items(oracle.ls_estimate(ltf[n:n + 1], P_rows).astype(np.complex64))
        check_items('cli packet %d' % n, H, H_ls, At, ns, ns, m['fbb'].reshape(234, ns, ns), m['idx'].reshape(234, ns).astype(np.int64),
                    m['n_atoms'].reshape(234), m['gain'].reshape(234))
