"""GPU tests (-m gpu) of the memory contract and the call history of csi_feedback_compress_device / csi_feedback_expand_device, in the
manner of tests/test_gpu_memory_contract.py (whose both_ways runs a call on plain and on guarded arrays and compares bit for bit).

Part A.  Every array exactly the documented size inside guard bands; the optional outputs present and NULL; the code arrays hold uint16
in arrays of floats, with an odd number of codes so that the documented size ends inside the last word (the rest of that word must
still hold the pre-fill); guards intact, nothing unwritten, inputs unchanged, one launch counted per call.

Part B.  One long-lived engine serves calls of changing shape, bit widths (the tables on the context are replaced), grouping and packet
count (the workspace grows) in changing order; every result equals, bit for bit, the same call on a fresh engine."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feedback_ref as R                                  # noqa: E402
from test_gpu_memory_contract import both_ways, _f32      # noqa: E402

N = R.N


def _pack(codes):
    """uint16 codes -> the float words that hold them (the last word zero-padded)"""
    flat = np.ascontiguousarray(codes, np.uint16).reshape(-1)
    return np.concatenate([flat, np.zeros(flat.size & 1, np.uint16)]).view(np.float32)


# (Nt, Nr, nc, npkt, ng, bits): 3 x 3 x 117 and 1 x 22 x 59 ... codes; the first is odd
A_CASES = [(4, 2, 1, 3, 2, (4, 2)), (8, 4, 4, 1, 4, (9, 7)), (32, 4, 2, 1, 1, (6, 4))]


@pytest.mark.parametrize('outputs', ['all', 'codes_only', 'continuous'])
@pytest.mark.parametrize('nt,nr,nc,npkt,ng,bits', A_CASES)
def test_a_compress(pkg, nt, nr, nc, npkt, ng, bits, outputs):
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    h = R.planes(7 + nt, npkt, nr, nt)
    n_ang, n_rep = R.n_angles(nt, nc), R.n_reports(ng)
    count = npkt * n_ang * n_rep
    ang, words = (npkt, n_ang, n_rep), ((count + 1) // 2,)
    outs, byte_len = {}, {}
    if outputs != 'continuous':
        outs.update(phi_code=words, psi_code=words)
        byte_len = {'phi_code': 2 * count, 'psi_code': 2 * count}
    if outputs != 'codes_only':
        outs.update(phi=ang, psi=ang)
    if outputs == 'all':
        outs.update(sigma=(npkt, nc, n_rep), v_re=(npkt, nc, nt, n_rep), v_im=(npkt, nc, nt, n_rep))
    b = (0, 0) if outputs == 'continuous' else bits

    def call(i, o):
        e.feedback_compress_device(i['h_re'], i['h_im'], npkt, nc, b[0], b[1], ng, o.get('phi_code'), o.get('psi_code'), o.get('phi'), o.get('psi'),
                                   o.get('sigma'), o.get('v_re'), o.get('v_im'))

    got = both_ways(e, call, {'h_re': _f32(h.real), 'h_im': _f32(h.imag)}, outs, {'feedback_launches': 1}, byte_len=byte_len)
    if 'phi_code' in got:
        kp, ks = got['phi_code'].view(np.uint16)[:count], got['psi_code'].view(np.uint16)[:count]
        assert kp.max() < 2 ** bits[0] and ks.max() < 2 ** bits[1]
    if 'phi' in got:
        assert np.isfinite(got['phi']).all() and np.isfinite(got['psi']).all()
    e.close()


@pytest.mark.parametrize('source,layout,with_sigma', [('codes', 'w', False), ('codes', 'csi', True), ('codes', 'csi', False), ('angles', 'w', False),
                                                      ('angles', 'csi', True)])
@pytest.mark.parametrize('nt,nr,nc,npkt,ng,bits', A_CASES)
def test_a_expand(pkg, nt, nr, nc, npkt, ng, bits, source, layout, with_sigma):
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    rng = np.random.default_rng(11 + nt)
    ang = (npkt, R.n_angles(nt, nc), R.n_reports(ng))
    if source == 'codes':
        ins = {'phi_code': _pack(rng.integers(0, 2 ** bits[0], ang)), 'psi_code': _pack(rng.integers(0, 2 ** bits[1], ang))}
    else:
        ins = {'phi': _f32(rng.uniform(0, 2 * np.pi, ang)), 'psi': _f32(rng.uniform(0, np.pi / 2, ang))}
    if with_sigma:
        ins['sigma'] = _f32(rng.uniform(0.5, 2.0, (npkt, nc, ang[2])))
    shape = (npkt, nc if layout == 'w' else nr, nt, N)

    def call(i, o):
        e.feedback_expand_device(npkt, nc, bits[0], bits[1], ng, e.FB_LAYOUT_W if layout == 'w' else e.FB_LAYOUT_CSI, o['out_re'], o['out_im'],
                                 d_phi_code=i.get('phi_code'), d_psi_code=i.get('psi_code'), d_phi=i.get('phi'), d_psi=i.get('psi'), d_sigma=i.get('sigma'))

    got = both_ways(e, call, ins, {'out_re': shape, 'out_im': shape}, {'feedback_launches': 1})
    assert np.isfinite(got['out_re']).all() and np.isfinite(got['out_im']).all()
    if layout == 'w':
        assert np.abs((got['out_re'].astype(np.float64) ** 2 + got['out_im'].astype(np.float64) ** 2).sum((1, 2)) - nt).max() <= 1e-5 * nt
    e.close()


# ====================================================================================================================== part B
B_NT, B_NR = 8, 4
# (nc, bits, ng, npkt)
B_CALLS = [(2, (9, 7), 1, 3), (1, (4, 2), 4, 1), (4, (6, 4), 2, 7), (2, (0, 0), 1, 2)]


def _round_trip(e, call):
    nc, bits, ng, npkt = call
    h = R.planes(300 + npkt, npkt, B_NR, B_NT)
    rep = e.feedback_compress(h, nc, bits[0], bits[1], ng, keep_angles=True, keep_v=True)
    return [a for a in rep[:6] if a is not None] + [e.feedback_expand(rep, 'w'), e.feedback_expand(rep, 'csi')]


def test_b_changing_calls_on_one_engine_equal_fresh_engines(pkg):
    fresh = []
    for call in B_CALLS:
        e = pkg.CsiEngine(B_NT, B_NR, hidden=(8,))
        fresh.append(_round_trip(e, call))
        e.close()
    e = pkg.CsiEngine(B_NT, B_NR, hidden=(8,))
    for j in (0, 1, 2, 3, 2, 0, 3, 1, 0):
        for k, (a, b) in enumerate(zip(_round_trip(e, B_CALLS[j]), fresh[j])):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), 'call %s after other calls: result %d differs' % (B_CALLS[j], k)
    e.close()
