"""csi_band4 / csi_band4_cs after the re-cut of their sub-step schedule (csrc/band4_kernel_gen.py RoleH: exchange writes dealt early, counted LDS waits as
generator flags): every path of the main loop at the smallest shapes that reach it.

hidden = (K1, N1):  K1 128 = head + last, 192 = one loop trip, 320 = the loop's back edge;  N1 256 = one column step, 512 = the second-column
path, 1024 = the 2-way column split (csi_band4_cs, each split 512 wide; "band_split" = 2 asks for it, a call this small would take 4 splits
of the 8-wave form otherwise).  Nt 16 and 32, Nr 1.  n_out 234 = the staged epilogue, 233 = the row-per-lane stores.

Rows: one full band (128); a ragged last band; and - K1 128, N1 256 only - 600 bands in one launch, more than the CUs, so that workgroups turn
over.  The ragged count: a call has packets x Nt rows, always a multiple of 16, so "128 k + 40" cannot occur at these Nt; the nearest counts that
exist are taken, 11 packets in both cases: Nt 16 -> 176 = 128 + 48 (row group 1 of the last band half filled), Nt 32 -> 352 = 2 x 128 + 96 (the
last band's fourth row group empty).

Every call goes through the device entry point (one launch per component model).  Each call: against the fp64 oracle at the tolerance of
test_gpu_dnn_f32.py::test_band_kernel_matches_oracle_and_separate_kernels (1e-5 norm-relative per row), three runs bit-identical (a wait that is too short shows as a run-to-run difference), the SHA-256 of the two output planes equal
to the digest the PREVIOUS schedule's build wrote for the same inputs (tests/golden/band4_waits_outputs.json: the arithmetic did not change, so the
bits must not), and "band4_launches" advanced by the two component models."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import rel_rows

pytestmark = pytest.mark.gpu

TOL = 1e-5
K1S, N1S, NTS, NOUTS = (128, 192, 320), (256, 512, 1024), (16, 32), (234, 233)
CASES = [(k1, n1, nt, n_out) for k1 in K1S for n1 in N1S for nt in NTS for n_out in NOUTS]
TURNOVER_BANDS = 600
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'band4_waits_outputs.json')


def packet_counts(k1, n1, nt):
    """(label, packets) of a case: one full band, the ragged count, and the 600-band launch where it is asked for"""
    counts = [('full', 128 // nt), ('ragged', 11)]
    if (k1, n1) == (128, 256):
        counts.append(('turnover', TURNOVER_BANDS * 128 // nt))
    return counts


def key(k1, n1, nt, n_out, label):
    return 'K1=%d N1=%d Nt=%d n_out=%d %s' % (k1, n1, nt, n_out, label)


def run_case(pkg, oracle, k1, n1, nt, n_out, golden=None, counter=True, log=None):
    """runs every row count of one case; returns {key: digest}.  golden = the recorded digests to compare with (None: record only)"""
    seed = ((k1 * 4096 + n1) * 64 + nt) * 256 + n_out
    rng = np.random.default_rng(seed)
    w = [oracle.make_weights(rng, 320 * nt + nt, [k1, n1], n_out) for _ in range(2)]
    P = oracle.hadamard(nt)
    e = pkg.CsiEngine(nt, 1, hidden=(k1, n1), n_out=n_out)
    out = {}
    try:
        e.load_weights('real', w[0])
        e.load_weights('imag', w[1])
        e.set_pilot(P)
        e.set_option('f32_engine', 1)
        e.set_option('small_fused', 0)
        e.set_option('band_split', 2 if n1 == 1024 else 0)
        for label, npkt in packet_counts(k1, n1, nt):
            ltf = (rng.standard_normal((npkt, 1, 320 * nt), np.float32) + 1j * rng.standard_normal((npkt, 1, 320 * nt), np.float32)).astype(np.complex64)
            # the device entry point: the whole call is ONE launch per component model (the host entry point stages a large call in chunks)
            d_re, d_im = e.to_device(np.ascontiguousarray(ltf.real, np.float32)), e.to_device(np.ascontiguousarray(ltf.imag, np.float32))
            d_o = [e.empty((npkt, 1, nt, n_out)) for _ in range(2)]
            runs = []
            for _ in range(3):
                n0 = e.get_option('band4_launches') if counter else 0
                b0, s0 = e.get_option('band_launches'), e.get_option('band_split_launches')
                for d in d_o:
                    d.upload(np.zeros((npkt, 1, nt, n_out), np.float32))
                e.predict_device(d_re, d_im, npkt, d_o[0], d_o[1])
                e.synchronize()
                runs.append((d_o[0].download().copy(), d_o[1].download().copy()))
                assert e.get_option('band_launches') == b0 + 2, 'one band launch per component model'
                if counter:
                    assert e.get_option('band4_launches') == n0 + 2, 'a csi_band4* kernel did not serve both component models'
                assert e.get_option('band_split_launches') - s0 == (2 if n1 == 1024 else 0), 'csi_band4 / csi_band4_cs: the other form served the call'
            assert e.get_option('hs_range_fallbacks') == 0
            for o_re, o_im in runs[1:]:
                assert np.array_equal(o_re, runs[0][0]) and np.array_equal(o_im, runs[0][1]), 'run-to-run difference: %s' % key(k1, n1, nt, n_out, label)
            o_re, o_im = runs[0]
            k = min(npkt, 4)
            sel = np.r_[0:k // 2, npkt - (k - k // 2):npkt]
            r_re, r_im = oracle.predict_packets(ltf[sel], P, w[0], w[1], np.float64, pkt_batch=len(sel))
            err = max(rel_rows(o_re[sel], r_re), rel_rows(o_im[sel], r_im))
            h = hashlib.sha256()
            h.update(np.ascontiguousarray(o_re, np.float32).tobytes())
            h.update(np.ascontiguousarray(o_im, np.float32).tobytes())
            kk = key(k1, n1, nt, n_out, label)
            out[kk] = h.hexdigest()
            if log:
                log('%-44s rows %6d oracle %.2e digest %s' % (kk, npkt * nt, err, out[kk][:16]))
            assert np.isfinite(o_re).all() and np.isfinite(o_im).all() and err < TOL, (kk, err)
            if golden is not None:
                assert out[kk] == golden[kk], 'the output bits differ from the previous schedule\'s: %s' % kk
    finally:
        e.close()
    return out


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)['digests']


@pytest.mark.parametrize('k1,n1,nt,n_out', CASES)
def test_band4_counted_waits(pkg, oracle, golden, k1, n1, nt, n_out):
    run_case(pkg, oracle, k1, n1, nt, n_out, golden=golden, log=print)
