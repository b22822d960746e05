"""CPU tests of the NMSE-vs-SNR sweep: the C-ABI surface of csi_synth_structured (header, ctypes table, exported symbol, profile
entry, refusal without a device), the host replay tests/synth_streams.py on its own, and the host functions of the sweep module
(confidence interval, metrics.mat, dataset packing)."""
import ctypes
import os
import pickle
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_streams as ss      # noqa: E402


def test_synth_structured_in_header_table_and_library(pkg):
    pkg.build_library()
    lib = pkg.load_library()
    header = open(os.path.join(REPO, 'include', 'csi_mamimo.h')).read()
    assert re.search(r'generate_maMIMO_LTF\.m:197-342\s+csi_synth_structured', header), 'row of the call-site table'
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(csi_[a-z0-9_]+)\s*\(', header))
    from dl_channel_estimation_mamimo_amd import _lib
    assert 'csi_synth_structured' in declared
    assert 'csi_synth_structured' in _lib.SYMBOLS
    assert hasattr(lib, 'csi_synth_structured')
    assert lib.csi_abi_version() == 1            # the change is additive
    names = [lib.csi_profile_kernel_name(i).decode() for i in range(lib.csi_profile_num_kernels())]
    assert 'synth_structured' in names, names
    assert b'synth_structured_kernel' in open(pkg.library_path(), 'rb').read()
    assert lib.csi_synth_structured(None, 1, 0, 1, None, 8, 1, None, None, None, None, None) == -1
    assert hasattr(pkg.CsiEngine, 'synth_structured') and hasattr(pkg.CsiEngine, 'lmmse_estimate_device')


def _signed_permutation(rng, H):
    n = H.shape[0]
    return (rng.choice([-1.0, 1.0], n)[:, None] * H[rng.permutation(n)][:, rng.permutation(n)]) * rng.choice([-1.0, 1.0], n)[None, :]


def test_replay_known_answer(oracle):
    """oracle.ls_estimate of the replay's noise-free packets is the replay's h, for a Hadamard P and a signed row / column
    permutation of one, with and without the amplitude scale"""
    rng = np.random.default_rng(2)
    for nt, nr in ((4, 2), (16, 3)):
        for P in (oracle.hadamard(nt), _signed_permutation(rng, oracle.hadamard(nt))):
            for amp in (False, True):
                r = ss.replay(9, 3, 2, nr, P, snr_db=None, n_taps=8, amp_scale=amp)
                assert r['ltf'].shape == (2, nr, 320 * nt) and r['h'].shape == (2, nr, nt, 234)
                err = np.abs(oracle.ls_estimate(r['ltf'], P) - r['h']).max()
                assert err < 1e-10, (nt, amp, err)
    # n_taps only adds taps: the first 4 taps of an 8-tap draw are the 4-tap draw
    assert np.array_equal(ss.taps(9, 3, 2, 4, 8)[..., :4], ss.taps(9, 3, 2, 4, 4))


def test_replay_ranges_and_noise_separation(oracle):
    P = oracle.hadamard(4)
    snr = np.linspace(-20, 10, 12)
    full = ss.replay(5, 0, 12, 2, P, snr_db=snr)
    part = ss.replay(5, 5, 5, 2, P, snr_db=snr[5:10])
    for k in ('ltf', 'clean', 'h', 'noise_std', 'z'):
        assert np.array_equal(full[k][5:10], part[k]), k
    clean = ss.replay(5, 0, 12, 2, P, snr_db=None)
    assert np.array_equal(clean['ltf'], full['clean']) and np.array_equal(clean['h'], full['h'])      # noise does not move the channel draws
    assert not np.array_equal(ss.replay(6, 0, 2, 2, P)['h'], clean['h'][:2])
    # per-packet power: every packet's own mean, not the batch mean
    want = np.sqrt(np.mean(np.abs(full['clean'] / ss.AMP) ** 2, axis=(1, 2)) * ss.noise_factor(snr))
    assert np.allclose(full['noise_std'], want, rtol=1e-12)
    assert np.std(full['power']) / np.mean(full['power']) > 0.05


def test_replay_realised_noise_power(oracle):
    """one Nt = 32, Nr = 4 packet: 81 920 real draws; the mean square of a standard normal has standard error sqrt(2 / n)"""
    nt, nr, snr = 32, 4, -5.0
    r = ss.replay(2024, 7, 1, nr, oracle.hadamard(nt), snr_db=snr, amp_scale=True)
    noise = (r['ltf'] - r['clean']) / ss.AMP
    n = 2 * noise.size
    assert n == 81920
    realised = np.mean(np.abs(noise) ** 2)                                          # complex noise power
    requested = r['power'][0] / 10.0 ** (snr / 10.0)
    dev = (realised / requested - 1.0) / np.sqrt(2.0 / n)
    print('realised / requested noise power = %.5f (%.2f standard errors)' % (realised / requested, dev))
    assert abs(dev) < 4.0
    snr_real = 10 * np.log10(np.mean(np.abs(r['clean']) ** 2) / np.mean(np.abs(r['ltf'] - r['clean']) ** 2))
    assert abs(snr_real - snr) < 0.1


def test_confidence_interval(pkg):
    from scipy import stats
    from dl_channel_estimation_mamimo_amd import sweep
    # by hand: x = 1, 2, 3, 4 -> mean 2.5, std (n - 1) = sqrt(5 / 3), t(0.975, 3) = 3.182446305...
    m, lo, hi = sweep.confidence_interval([1.0, 2.0, 3.0, 4.0])
    half = 3.182446305284263 * np.sqrt(5.0 / 3.0) / 2.0
    assert m == 2.5 and abs(lo - (2.5 - half)) < 1e-12 and abs(hi - (2.5 + half)) < 1e-12
    x = np.random.default_rng(0).lognormal(size=500)
    m, lo, hi = sweep.confidence_interval(x)
    ref = stats.t.interval(0.95, x.size - 1, loc=x.mean(), scale=stats.sem(x))
    assert abs(m - x.mean()) < 1e-15 and np.allclose((lo, hi), ref, rtol=1e-12)


def test_metrics_mat_round_trip(pkg, tmp_path):
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    rng = np.random.default_rng(1)
    mse = {'MSE_' + e: rng.random(16) for e in sweep.ESTIMATORS}
    path = sweep.write_metrics(str(tmp_path / 'BS4_SNR-20' / 'metrics.mat'), mse)
    back = loadmat(path)
    assert {k for k in back if not k.startswith('__')} == {'MSE_LS', 'MSE_MMSE', 'MSE_DNN'}
    for k, v in mse.items():
        assert back[k].shape == (1, 16) and back[k].dtype == np.float64 and np.array_equal(back[k][0], v)
    assert np.allclose(sweep.tap_profile(8), np.exp(-0.5 * np.arange(8)) / np.sqrt(2.0), rtol=1e-7)


def test_dataset_from_packets_round_trip(pkg, oracle, tmp_path):
    ds = pkg.dataset
    rng = np.random.default_rng(3)
    nt, nr, npkt = 4, 2, 6
    P = _signed_permutation(rng, oracle.hadamard(nt))           # not symmetric: a transposed P would show
    assert not np.array_equal(P, P.T)
    r = ss.replay(1, 0, npkt, nr, P)
    labels = oracle.ls_estimate(r['ltf'], P)
    data = ds.dataset_from_packets(r['ltf'], labels, P)
    assert sorted(data) == ['LTF', 'P', 'X', 'simParams', 'y'] and np.array_equal(data['P'], P.T)
    assert data['X'].shape == (npkt * nr * nt, 2) and len(data['LTF']) == npkt * nr
    path = str(tmp_path / 'dataset.b')
    with open(path, 'wb') as f:
        pickle.dump(data, f)
    packed = ds.packets_from_dataset(ds.load_dataset(path))
    assert (packed['nt'], packed['nr'], packed['npkt']) == (nt, nr, npkt)
    assert np.array_equal(packed['ltf'], r['ltf']) and np.array_equal(packed['pilot'], P) and np.array_equal(packed['labels'], labels)
    # the training-side readers accept it
    train_ids, val_ids = ds.split_train_val(data, 0.5)
    assert len(train_ids) == len(val_ids) == 3 * nr * nt
    gen = ds.SampleGenerator(train_ids, data, 'real', batch_size=8, shuffle=False)
    (xsig, xp), y, _ = gen[1]
    ids = gen.batch_ids(1)
    assert xsig.shape == (8, 320 * nt, 1) and xp.shape == (8, nt) and y.shape == (8, 234)
    s = int(ids[3])
    p, rx, j = s // (nr * nt), (s // nt) % nr, s % nt
    assert np.array_equal(xsig[3, :, 0], r['ltf'][p, rx].real.astype(np.float32)) and np.array_equal(xp[3], P[j].astype(np.float32))
    assert np.array_equal(y[3], labels[p, rx, j].real.astype(np.float32))
    table, ltf_row, itx, yy = ds.resident_arrays(data, 'imag')
    assert table.shape == (npkt * nr, 320 * nt) and np.array_equal(table[ltf_row[s]], r['ltf'][p, rx].imag.astype(np.float32))
    assert itx[s] == j and np.array_equal(yy[s], labels[p, rx, j].imag.astype(np.float32))
    # complex64 packets (what the device hands back) keep their precision class
    d32 = ds.dataset_from_packets(r['ltf'].astype(np.complex64), labels.astype(np.complex64), P)
    assert d32['LTF'][0]['real'].dtype == np.float32 and d32['y']['imag'].dtype == np.float32
