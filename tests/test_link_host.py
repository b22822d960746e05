"""CPU tests of the link simulation (csrc/link_sim.hip.h): the C-ABI surface (header, ctypes table, exported symbols,
profile names, refusals that need no device), csi_link_frame_bits, and the fp64 / fp32 restatement tests/link_ref.py against known
answers: the encoder's impulse response and free distance, the decoder on clean and sign-flipped frames, the QPSK soft bit in
closed form, and synth.link_noise_var."""
import ctypes
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import link_ref as L      # noqa: E402

NEW = ['csi_link_frame_bits', 'csi_viterbi_decode_device', 'csi_link_sim_device']


def test_new_entry_points_in_header_table_and_library(pkg):
    pkg.build_library()
    lib = pkg.load_library()
    header = open(os.path.join(REPO, 'include', 'csi_mamimo.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(csi_[a-z0-9_]+)\s*\(', header))
    from dl_channel_estimation_mamimo_amd import _lib
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.csi_abi_version() == 1            # the change is additive
    names = [lib.csi_profile_kernel_name(i).decode() for i in range(lib.csi_profile_num_kernels())]
    for k in ('link_txrx', 'link_viterbi'):
        assert k in names, names
    blob = open(pkg.library_path(), 'rb').read()
    for k in (b'link_txrx_kernel', b'link_viterbi_kernel', b'link_encode_kernel'):
        assert k in blob, k


def test_null_context_is_refused_without_a_device(pkg):
    lib = pkg.load_library()
    assert lib.csi_viterbi_decode_device(None, None, 1, 7, None) == -1
    assert lib.csi_link_sim_device(None, *[None] * 7, 0, 0, 1, 1, 1, 1, 2, *[None] * 8) == -1


def test_frame_bits(pkg):
    lib = pkg.load_library()
    n_info, n_coded = ctypes.c_int64(), ctypes.c_int64()
    assert lib.csi_link_frame_bits(1, 10, 2, ctypes.byref(n_info), ctypes.byref(n_coded)) == 0
    assert (n_info.value, n_coded.value) == (1554, 4680) == L.frame_bits(1, 10, 2)
    assert lib.csi_link_frame_bits(4, 3, 4, ctypes.byref(n_info), ctypes.byref(n_coded)) == 0
    assert (n_info.value, n_coded.value) == (4 * 3 * 234 * 4 // 3 - 6, 4 * 3 * 234 * 4) == L.frame_bits(4, 3, 4)
    assert lib.csi_link_frame_bits(2, 1, 2, None, None) == 0
    for bad in ((0, 10, 2), (5, 10, 2), (1, 0, 2), (1, 10, 3), (1, 10, 6), (1, 10, 0)):
        assert lib.csi_link_frame_bits(*bad, ctypes.byref(n_info), ctypes.byref(n_coded)) == -1, bad


def test_encoder_impulse_response_and_free_distance():
    want = [[1, 1, 1], [0, 1, 1], [1, 1, 1], [1, 1, 0], [0, 0, 1], [1, 0, 0], [1, 1, 1]]
    imp = np.array([1, 0, 0, 0, 0, 0, 0], np.uint8)
    assert L.encode_literal(imp).tolist() == want
    assert L.encode(imp, terminate=False).reshape(-1, 3).tolist() == want
    assert L.encode(imp[:1]).reshape(-1, 3).tolist() == want            # one bit and its six tail bits
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2, (3, 200)).astype(np.uint8)
    vec = L.encode(bits, terminate=False)
    for i in range(3):
        assert np.array_equal(vec[i].reshape(-1, 3), L.encode_literal(bits[i]))
    # free distance 15: the lightest terminated codeword over every input of up to 12 bits that starts with a one (the code is linear)
    n = 12
    words = ((np.arange(1 << (n - 1))[:, None] >> np.arange(n - 1)) & 1).astype(np.uint8)
    words = np.concatenate([np.ones((words.shape[0], 1), np.uint8), words], 1)
    assert int(L.encode(words).sum(1).min()) == 15


def test_reference_viterbi_recovers_clean_and_flipped_frames():
    rng = np.random.default_rng(1)
    for n_info in (1, 58, 59, 300):
        bits = rng.integers(0, 2, (4, n_info)).astype(np.uint8)
        llr = 1.0 - 2.0 * L.encode(bits).astype(np.float64)
        for dt in (np.float64, np.float32):
            assert np.array_equal(L.viterbi(llr, dt), bits), (n_info, dt)
        # 7 sign flips anywhere: below half the free distance of 15, so the sent word stays the unique closest one
        bad = llr.copy()
        for i in range(4):
            pos = rng.choice(llr.shape[1], 7, replace=False)
            bad[i, pos] *= -1.0
        for dt in (np.float64, np.float32):
            assert np.array_equal(L.viterbi(bad, dt), bits), (n_info, dt)
        assert (L.path_metric(llr, bits) == llr.shape[1]).all()
    assert np.array_equal(L.viterbi(llr[0]), bits[0])                  # one codeword without the leading axis


def test_qpsk_soft_bit_in_closed_form():
    """Gray QPSK: |x + a|^2 - |x - a|^2 = 4 a x per axis, so llr = 4 a Re(x) csi / noise_var (first bit), 4 a Im(x) csi / noise_var"""
    rng = np.random.default_rng(2)
    ns, n_sym = 2, 3
    x = rng.standard_normal((ns, n_sym, L.N)) + 1j * rng.standard_normal((ns, n_sym, L.N))
    csi = rng.uniform(0.1, 3.0, (ns, L.N))
    nv = 0.37
    llr = L.soft_bits(x, csi, nv, 2).reshape(ns, n_sym, L.N, 2)
    a = L.unit(2)
    assert np.abs(llr[..., 0] - 4 * a * x.real * csi[:, None, :] / nv).max() < 1e-12
    assert np.abs(llr[..., 1] - 4 * a * x.imag * csi[:, None, :] / nv).max() < 1e-12
    # the constellations: unit average power, Gray along both axes, mapper and labels agree
    for bps in (2, 4):
        q, lab = L.constellation(bps)
        assert abs((np.abs(q) ** 2).mean() - 1.0) < 1e-12
        d = np.abs(q[:, None] - q[None, :])
        near = np.isclose(d, 2 * L.unit(bps))
        assert ((lab[:, None, :] != lab[None, :, :]).sum(-1)[near] == 1).all()
        reps = L.N // (1 << bps) + 1
        sym = L.map_bits(np.tile(lab.reshape(-1), reps)[:L.N * bps], 1, 1, bps)        # every label in turn along the subcarriers
        assert sym.shape == (1, 1, L.N) and np.allclose(sym[0, 0, :1 << bps], q)
        # a noiseless symbol demaps to its own label and has no EVM
        hard = L.soft_bits(np.tile(q, reps)[:L.N].reshape(1, 1, L.N), np.ones((1, L.N)), 1.0, bps) < 0
        assert np.array_equal(hard.reshape(L.N, bps)[:1 << bps].astype(np.uint8), lab)
        assert L.evm_rms(q, bps) == 0.0


def test_link_noise_var(pkg):
    amp = float(np.float32(np.sqrt(242.0) / 256.0))
    std = np.array([0.5, 2.0], np.float32)
    assert np.allclose(pkg.synth.link_noise_var(std), 512.0 * amp * amp * std.astype(np.float64) ** 2, rtol=1e-12)
    assert np.allclose(pkg.synth.link_noise_var(std, amp_scale=False), 512.0 * std.astype(np.float64) ** 2, rtol=1e-12)
    assert float(pkg.synth.link_noise_var(0.0)) == 0.0
