"""CPU tests of the hybrid beamforming weights: the C-ABI surface (header, ctypes table, exported symbols, refusals that need no
device), the fp64 restatement tests/hybrid_ref.py against a literal per-item loop, and the dictionary helpers of synth."""
import ctypes
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hybrid_ref as R      # noqa: E402

NEW = ['csi_hybrid_set_dictionary', 'csi_hybrid_weights', 'csi_hybrid_weights_device',
       'csi_capture_begin', 'csi_capture_end', 'csi_capture_launch', 'csi_capture_free']


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
    for k in ('hybrid_svd', 'hybrid_corr_argmax', 'hybrid_solve', 'hybrid_finish'):
        assert k in names, names
    blob = open(pkg.library_path(), 'rb').read()
    for k in (b'hyb_svd_kernel', b'hyb_corr_kernel', b'hyb_solve_kernel', b'hyb_gain_kernel', b'hyb_frf_mean_kernel'):
        assert k in blob, k


def test_null_context_is_refused_without_a_device(pkg):
    lib = pkg.load_library()
    z = np.zeros(4, np.float32)
    p = z.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.csi_hybrid_set_dictionary(None, p, p, 1) == -1
    none7 = [None] * 7
    assert lib.csi_hybrid_weights(None, None, None, None, None, 1, 1, 1, 0.0, *none7) == -1
    assert lib.csi_hybrid_weights_device(None, None, None, None, None, 1, 1, 1, 0.0, *none7) == -1
    assert lib.csi_capture_begin(None) == -1
    g = ctypes.c_void_p()
    assert lib.csi_capture_end(None, ctypes.byref(g)) == -1
    assert lib.csi_capture_launch(None, None) == -1
    lib.csi_capture_free(None, None)             # a no-op


def literal_item(H, At, ns, ntrf, stop_tol):
    """the definition for one item, written out with np.linalg.svd and lstsq"""
    _, _, vh = np.linalg.svd(H)
    fopt = np.conj(vh[:ns]).T
    res, idx, C = fopt.copy(), [], None
    for _ in range(ntrf):
        met = (np.abs(np.conj(At).T @ res) ** 2).sum(1)
        idx.append(int(np.argmax(met)))
        A = At[:, idx]
        C = np.linalg.lstsq(A, fopt, rcond=None)[0]
        T = fopt - A @ C
        e = np.linalg.norm(T)
        if e <= stop_tol:
            break
        res = T / e
    A = At[:, idx]
    fbb = np.zeros((ns, ntrf), np.complex128)
    fbb[:, :len(idx)] = (np.sqrt(ns) * C / np.linalg.norm(A @ C)).T
    return fbb, idx + [-1] * (ntrf - len(idx)), len(idx)


def test_hybrid_ref_against_a_literal_loop(pkg):
    rng = np.random.default_rng(4)
    nt, nr, ns, ntrf, rays, n = 16, 4, 2, 4, 96, 50
    az, el = pkg.synth.random_rays(np.random.default_rng(6), rays)
    At = pkg.synth.steering_ula(nt, az, el)
    H = rng.standard_normal((n, nr, nt)) + 1j * rng.standard_normal((n, nr, nt))
    fbb, idx, n_atoms = R.omp(H, At, ns, ntrf)
    for i in range(n):
        f_i, idx_i, n_i = literal_item(H[i], At, ns, ntrf, 1e-5)
        assert idx[i].tolist() == idx_i and n_atoms[i] == n_i
        assert np.abs(fbb[i] - f_i).max() < 1e-10
    # the replay of the definition's own choices has no shortfall and gives the same coefficients
    short, fbb_r = R.replay(H, At, ns, idx)
    assert np.abs(short).max() < 1e-12 and np.abs(fbb_r - fbb).max() < 1e-10
    T = R.weights_matrix(At, idx, fbb)
    assert np.abs((np.abs(T) ** 2).sum((1, 2)) - ns).max() < 1e-12
    assert R.projector_error(T, T).max() == 0.0
    # early stop: a rank-one channel along a dictionary column is fitted by one atom
    H1 = (rng.standard_normal((3, nr, 1)) + 0j) * np.conj(At[:, 7])[None, None, :]
    fbb1, idx1, n1 = R.omp(H1, At, 1, 3)
    assert (idx1[:, 0] == 7).all() and (idx1[:, 1:] == -1).all() and (n1 == 1).all() and (fbb1[:, :, 1:] == 0).all()
    assert np.allclose(R.gain(H1, R.weights_matrix(At, idx1, fbb1)), (np.abs(H1) ** 2).sum((1, 2)))
    # csi_to_items: [p][i][j][k] -> item (p, k)
    h = rng.standard_normal((2, nr, nt, 234)) + 1j * rng.standard_normal((2, nr, nt, 234))
    items = R.csi_to_items(h)
    assert items.shape == (468, nr, nt) and np.array_equal(items[234 + 5], h[1, :, :, 5])


def test_steering_ula_and_random_rays(pkg):
    nt = 8
    az, el = pkg.synth.random_rays(np.random.default_rng(1), 1000)
    assert az.shape == el.shape == (1000,)
    assert az.min() >= -180 and az.max() <= 180 and el.min() >= -90 and el.max() <= 90
    assert az.min() < -150 and az.max() > 150 and el.min() < -75 and el.max() > 75          # the whole range is drawn
    A = pkg.synth.steering_ula(nt, az, el)
    assert A.shape == (nt, 1000) and A.dtype == np.complex128
    assert np.abs(np.abs(A) - 1.0).max() < 1e-12
    # the array is centred: element n and element nt-1-n are conjugates; broadside is all ones
    assert np.abs(A - np.conj(A[::-1])).max() < 1e-12
    assert np.abs(pkg.synth.steering_ula(nt, 0.0, 0.0)[:, 0] - 1.0).max() < 1e-12
    # a_n = exp(2 pi i y_n cos(el) sin(az)), half-wavelength spacing: neighbours differ by exp(i pi cos(el) sin(az))
    a = pkg.synth.steering_ula(nt, 30.0, 60.0)[:, 0]
    assert np.abs(a[1:] / a[:-1] - np.exp(1j * np.pi * np.cos(np.deg2rad(60.0)) * np.sin(np.deg2rad(30.0)))).max() < 1e-12
    assert np.abs(pkg.synth.steering_ula(nt, -30.0, 0.0) - np.conj(pkg.synth.steering_ula(nt, 30.0, 0.0))).max() < 1e-12


def test_frf_from_idx(pkg):
    At = pkg.synth.steering_ula(4, np.linspace(-60, 60, 5), 0.0)
    idx = np.array([[[2, -1]], [[0, 4]]])
    frf = pkg.frf_from_idx(At, idx)
    assert frf.shape == (2, 1, 2, 4)
    assert np.array_equal(frf[0, 0, 0], At[:, 2]) and (frf[0, 0, 1] == 0).all() and np.array_equal(frf[1, 0, 1], At[:, 4])
    assert np.array_equal(frf, R.frf_from_idx(At, idx))
