"""GPU tests (-m gpu) of the memory contract and the call history of csi_rx_combiner_device / csi_rx_apply_combiner_device, in the manner
of tests/test_gpu_feedback_memory.py (both_ways of tests/test_gpu_memory_contract.py runs a call on plain and on guarded arrays and
compares bit for bit).

Part A.  Every array exactly the documented size inside guard bands, sigma present and NULL; guards intact, nothing unwritten, inputs
unchanged, one launch counted per call.  Part B.  Every refusal raises with text that names the argument and leaves "combine_launches"
and the outputs untouched; the context stays usable."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feedback_ref as R                                  # noqa: E402
from test_gpu_memory_contract import both_ways, _f32      # noqa: E402

N = R.N
A_CASES = [(8, 2, 1, 3), (8, 4, 2, 1), (16, 16, 4, 1)]      # (Nt, Nr, ns, npkt)


@pytest.mark.parametrize('with_sigma', [True, False])
@pytest.mark.parametrize('nt,nr,ns,npkt', A_CASES)
def test_a_combiner(pkg, nt, nr, ns, npkt, with_sigma):
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    h = R.planes(7 + nt, npkt, nr, nt)
    outs = {'c_re': (npkt, ns, nr, N), 'c_im': (npkt, ns, nr, N)}
    if with_sigma:
        outs['sigma'] = (npkt, ns, N)

    def call(i, o):
        e.rx_combiner_device(i['h_re'], i['h_im'], npkt, ns, o['c_re'], o['c_im'], o.get('sigma'))

    got = both_ways(e, call, {'h_re': _f32(h.real), 'h_im': _f32(h.imag)}, outs, {'combine_launches': 1})
    assert all(np.isfinite(v).all() for v in got.values())
    e.close()


@pytest.mark.parametrize('nt,nr,ns,npkt', A_CASES)
def test_a_apply(pkg, nt, nr, ns, npkt):
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    h = R.planes(9 + nt, npkt, nr, nt)
    rng = np.random.default_rng(3 + nr)
    c = rng.standard_normal((2, npkt, ns, nr, N)).astype(np.float32)
    shape = (npkt, nr, nt, N)

    def call(i, o):
        e.rx_apply_combiner_device(i['c_re'], i['c_im'], i['h_re'], i['h_im'], npkt, ns, o['e_re'], o['e_im'])

    got = both_ways(e, call, {'c_re': c[0], 'c_im': c[1], 'h_re': _f32(h.real), 'h_im': _f32(h.imag)}, {'e_re': shape, 'e_im': shape},
                    {'combine_launches': 1})
    assert np.isfinite(got['e_re']).all() and np.isfinite(got['e_im']).all() and not got['e_re'][:, ns:].any()
    e.close()


class _At:
    def __init__(self, ptr):
        self.ptr = ptr


def test_b_refusals(pkg):
    nt, nr, npkt = 8, 4, 2
    e = pkg.CsiEngine(nt, nr, hidden=(8,), device=0)
    big = [e.to_device(np.zeros((npkt, nr, nt, N + 8), np.float32)) for _ in range(7)]
    n0 = e.get_option('combine_launches')

    def comb(text, ns=2, n=npkt, eng=e, **kw):
        a = dict(h_re=big[0], h_im=big[1], c_re=big[2], c_im=big[3], sigma=big[4])
        a.update(kw)
        with pytest.raises(pkg.CsiError) as err:
            eng.rx_combiner_device(a['h_re'], a['h_im'], n, ns, a['c_re'], a['c_im'], a['sigma'])
        assert err.value.code == -1 and text in str(err.value), (text, str(err.value))

    def app(text, ns=2, n=npkt, eng=e, **kw):
        a = dict(c_re=big[2], c_im=big[3], h_re=big[0], h_im=big[1], e_re=big[5], e_im=big[6])
        a.update(kw)
        with pytest.raises(pkg.CsiError) as err:
            eng.rx_apply_combiner_device(a['c_re'], a['c_im'], a['h_re'], a['h_im'], n, ns, a['e_re'], a['e_im'])
        assert err.value.code == -1 and text in str(err.value), (text, str(err.value))

    for f in (comb, app):
        f('ns 0 outside', ns=0)
        f('ns 5 outside 1 .. min(4, Nr 4)', ns=5)
        f('npkt -1', n=-1)
        f('the c planes come as a pair', c_im=_At(None))
        f('null required pointer (c_re, c_im)', c_re=_At(None), c_im=_At(None))
        f('d_c_re must start on a 16-byte boundary', c_re=_At(big[2].ptr + 4))
        f('d_c_im must start on a 16-byte boundary', c_im=_At(big[3].ptr + 8))
    comb('null required pointer (hest_re, hest_im)', h_re=_At(None))
    comb('d_hest_re must start on a 16-byte boundary', h_re=_At(big[0].ptr + 4))
    comb('d_hest_im must start on a 16-byte boundary', h_im=_At(big[1].ptr + 4))
    comb('d_sigma must be aligned', sigma=_At(big[4].ptr + 2))
    app('the h planes come as a pair', h_im=_At(None))
    app('the e planes come as a pair', e_re=_At(None))
    app('null required pointer (h_re, h_im)', h_re=_At(None), h_im=_At(None))
    app('null required pointer (e_re, e_im)', e_re=_At(None), e_im=_At(None))
    app('d_h_re must start on a 16-byte boundary', h_re=_At(big[0].ptr + 4))
    app('d_e_im must start on a 16-byte boundary', e_im=_At(big[6].ptr + 4))
    e.synchronize()
    assert e.get_option('combine_launches') == n0
    assert all(not a.download().any() for a in big), 'a refused call wrote'
    # npkt == 0 returns 0 and launches nothing
    e.rx_combiner_device(big[0], big[1], 0, 2, big[2], big[3])
    e.rx_apply_combiner_device(big[2], big[3], big[0], big[1], 0, 2, big[5], big[6])
    assert e.get_option('combine_launches') == n0
    # shapes of the context: ns above Nr, Nr above 16, a single-input context
    two = pkg.CsiEngine(4, 2, hidden=(8,), device=0)
    comb('ns 3 outside 1 .. min(4, Nr 2)', ns=3, eng=two)
    many = pkg.CsiEngine(32, 32, hidden=(8,), device=0)
    comb('Nr 32 > 16', eng=many)
    app('Nr 32 > 16', eng=many)
    one = pkg.CsiEngine(0, 1, hidden=(16,), len_ltf=64)
    comb('single-input context', ns=1, eng=one)
    app('single-input context', ns=1, eng=one)
    for x in (two, many, one):
        assert x.get_option('combine_launches') == 0
        x.close()
    # the context stays usable
    c = e.rx_combiner(R.planes(1, 1, nr, nt), 2)
    assert e.get_option('combine_launches') == n0 + 1 and c.shape == (1, 2, nr, N)
    e.close()
