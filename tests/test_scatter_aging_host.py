"""CPU tests of channel aging (csi_scatter_channel_at_device, csrc/scatter_aged.hip.h): the fp64 statement
tests/scatter_aging_ref.py against tests/scatter_ref.py at t = 0 and at speed 0, its one-scatterer known answer with the sign of the
Doppler shift, time reversal, the draw of a random heading, and the C-ABI surface (header, ctypes table, exported symbol, profile
entry, a null context)."""
import ctypes
import math
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scatter_aging_ref as ar      # noqa: E402
import scatter_ref as sr      # noqa: E402


def test_t0_and_speed0_are_the_parent_replay(oracle):
    for nt, nr, S, kw in ((4, 2, 3, dict(random_users=True)), (8, 2, 37, dict(range_m=1000.0, amp_scale=False, az_deg=-75.0, el_deg=20.0))):
        P = oracle.hadamard(nt)
        parent = sr.replay(11, 3, 2, nr, P, n_scat=S, **kw)['h']
        moving = ar.replay(11, 3, 2, nr, P, [0.0, 3e-3], speed_mps=2.0, heading_az_deg=40.0, heading_el_deg=-10.0, n_scat=S, **kw)['h']
        static = ar.replay(11, 3, 2, nr, P, [-1.0, 0.0, 0.25], speed_mps=0.0, heading_az_deg=40.0, random_heading=True, n_scat=S, **kw)['h']
        scale = np.abs(parent).max()
        assert np.abs(moving[0] - parent).max() < 1e-13 * scale
        assert np.abs(moving[1] - parent).max() > 1e-3 * scale
        for k in range(3):
            assert np.abs(static[k] - parent).max() < 1e-13 * scale


def test_one_scatterer_known_answer_and_its_sign(oracle):
    """S = 1: h_t = h_0 exp(2 pi i nu t) with nu = speed fc / c cos(angle(m, o)) from the replayed offset; a user that moves towards
    its scatterer (m . o > 0) shortens the path, so the phase ADVANCES: nu > 0"""
    nt, nr, speed, fc, t = 4, 2, 1.5, 28e9, 2e-3
    P = oracle.hadamard(nt)
    for az in (0.0, 77.0, -160.0):
        r = ar.replay(5, 2, 2, nr, P, [0.0, t], speed_mps=speed, heading_az_deg=az, heading_el_deg=15.0, carrier_hz=fc, n_scat=1)
        for p in range(2):
            o_s, m = r['off'][p, 0], r['m'][p]
            cosang = float(np.dot(m, o_s) / np.linalg.norm(o_s))
            nu = speed * fc / sr.C * cosang
            assert abs(np.linalg.norm(m) - 1.0) < 1e-15 and abs(r['nu'][p, 0] - nu) < 1e-9 * abs(nu)
            assert abs(nu) <= speed * fc / sr.C and (nu > 0) == (np.dot(m, o_s) > 0)
            ratio = r['h'][1, p] / r['h'][0, p]
            assert np.abs(ratio - np.exp(2j * np.pi * nu * t)).max() < 1e-9
    # towards the scatterer itself: the full Doppler shift, positive
    uu, u, _ = sr.draws(5, 2, 1)
    off = ar.offsets(u, 100.0, 0.1)[0]
    az, el = math.degrees(math.atan2(off[1], off[0])), math.degrees(math.asin(off[2] / np.linalg.norm(off)))
    nu = ar.doppler(off[None], ar.heading(az, el)[0], speed, fc)[0]
    assert abs(nu / (speed * fc / sr.C) - 1.0) < 1e-6      # az / el pass through fp32


def test_time_reversal_of_one_scatterer(oracle):
    nt, nr, t = 4, 2, 1.25e-3
    r = ar.replay(9, 0, 2, nr, oracle.hadamard(nt), [-t, 0.0, t], speed_mps=3.0, heading_az_deg=-20.0, n_scat=1)['h']
    assert np.abs(r[0] * r[2] - r[1] ** 2).max() < 1e-12 * np.abs(r[1] ** 2).max()      # h_-t h_t = h_0^2
    assert np.abs(r[0] / r[1] - np.conj(r[2] / r[1])).max() < 1e-12


def test_random_heading_reads_index_3_and_moves_nothing_else(oracle):
    import synth_streams as ss
    import train_streams as ts
    nt, nr, S, seed, first = 4, 2, 5, 21, 6
    P = oracle.hadamard(nt)
    fixed = ar.replay(seed, first, 3, nr, P, [0.0, 1e-3], speed_mps=1.0, heading_az_deg=10.0, n_scat=S, random_users=True)
    rnd = ar.replay(seed, first, 3, nr, P, [0.0, 1e-3], speed_mps=1.0, heading_az_deg=10.0, n_scat=S, random_users=True, random_heading=True)
    for i in range(3):
        u3 = float(ts.uniform(ss.key(seed, first + i, 0), np.array([3], np.uint64))[0])
        assert rnd['heading_az'][i] == 180.0 * (2.0 * u3 - 1.0) and -180.0 <= rnd['heading_az'][i] < 180.0
        assert abs(fixed['heading_az'][i] - 10.0) < 1e-6
    assert len(set(rnd['heading_az'].tolist())) == 3
    # the scatterers, the user and the sounding-time channel are those of the fixed heading and of the parent
    for k in ('off', 'g', 'tau_excess'):
        assert np.array_equal(fixed[k], rnd[k])
    assert np.array_equal(fixed['h'][0], rnd['h'][0])
    assert not np.array_equal(fixed['h'][1], rnd['h'][1])
    assert np.abs(rnd['h'][0] - sr.replay(seed, first, 3, nr, P, n_scat=S, random_users=True)['h']).max() < 1e-13


def test_surface_header_table_library_and_profile(pkg):
    pkg.build_library()
    lib = pkg.load_library()
    from dl_channel_estimation_mamimo_amd import _lib
    header = open(os.path.join(REPO, 'include', 'csi_mamimo.h')).read()
    assert 'first order' in header.lower() and 'No pilot matrix is needed' in header
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert 'csi_scatter_channel_at_device' in set(re.findall(r'\b(csi_[a-z0-9_]+)\s*\(', code))
    assert 'csi_scatter_channel_at_device' in _lib.SYMBOLS and hasattr(lib, 'csi_scatter_channel_at_device')
    assert lib.csi_abi_version() == 1            # the change is additive
    fields = re.search(r'typedef struct \{([^}]*)\} csi_motion_config;', code).group(1)
    assert re.findall(r'\b([a-z_]+)\s*[,;]', fields) == [f[0] for f in _lib.CsiMotionConfig._fields_]
    assert ctypes.sizeof(_lib.CsiMotionConfig) == 20
    names = [lib.csi_profile_kernel_name(i).decode() for i in range(lib.csi_profile_num_kernels())]
    assert 'scatter_aged' in names and 'synth_scattering' in names, names
    assert b'scatter_aged_kernel' in open(pkg.library_path(), 'rb').read()
    t = (ctypes.c_double * 1)(0.0)
    assert lib.csi_scatter_channel_at_device(None, 1, 0, 1, None, None, t, 1, None, None) == -1          # a null context
    for m in ('scatter_channel_at', 'scatter_channel_at_device'):
        assert hasattr(pkg.CsiEngine, m)
