"""GPU tests of the delay-subspace smoother (csi_subspace_set_basis, csi_subspace_smooth[_device]; csrc/subspace_smooth.hip.h) against
tests/subspace_ref.py: accuracy beside the same statement in numpy complex64, the projection property, weights per (packet, rx),
bit-for-bit identity across call sizes / chunks / aliasing / graph replay, guard bands around every array, refusals, what the
estimator gains over LS on known-channel packets, and the sweep's --delayTaps switch."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subspace_ref as sr      # noqa: E402
from guarded import Guarded       # noqa: E402

pytestmark = pytest.mark.gpu

N = 234
ORDER = 4.0      # the kernel sums in another order than numpy's complex64 products: the factor test_d_ml_shortfall_on_real_llrs uses for that
# (Nt, Nr, npkt, basis): 4 rows, the smallest call; odd rank, 24 rows, less than any tile; 592 rows: several workgroups and a partial
# last tile (two rank tiles, carriers in halves); top rank (four rank tiles); 1152 rows; a basis without delay structure; ranks that
# fill no whole number of tiles: 33 (two rank tiles, carriers in halves, the second tile one column), 65 and 96 (three rank tiles:
# the fourth wave idles through stage 1; 65 leaves the third tile one column)
CASES = {
    'rows4_rank1': (4, 1, 1, ('delay', 1, 0)),
    'rows24_rank13': (4, 2, 3, ('delay', 13, 0)),
    'rows592_rank64': (8, 2, 37, ('delay', 64, 8)),
    'rows20_rank128': (4, 1, 5, ('delay', 128, 16)),
    'rows1152_rank16': (32, 4, 9, ('delay', 16, 0)),
    'rows24_random13': (4, 2, 3, ('random', 13)),
    'rows24_rank33': (4, 2, 3, ('delay', 33, 4)),
    'rows40_random65': (4, 2, 5, ('random', 65)),
    'rows36_rank96': (4, 3, 3, ('delay', 96, 12)),
}


def _planes(rng, shape):
    return (rng.standard_normal(shape, dtype=np.float32) + 1j * rng.standard_normal(shape, dtype=np.float32)).astype(np.complex64)


def _basis(pkg, spec):
    if spec[0] == 'delay':
        Q, lam = pkg.subspace.delay_basis(spec[1], spec[2])
        assert Q.shape[1] == spec[1]
        return Q
    return sr.random_basis(np.random.default_rng(spec[1]), spec[1])


def _cplx(re, im):
    out = np.empty(re.shape, np.complex64)
    out.real, out.imag = re, im
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(e, x, w=None):
    """one device call on fresh arrays -> complex64 result"""
    npkt = x.shape[0]
    i_re, i_im = e.to_device(x.real), e.to_device(x.imag)
    o_re, o_im = e.empty(x.shape), e.empty(x.shape)
    d_w = e.to_device(w) if w is not None else None
    e.subspace_smooth_device(i_re, i_im, npkt, o_re, o_im, d_w)
    e.synchronize()
    out = _cplx(o_re.download(), o_im.download())
    for a in (i_re, i_im, o_re, o_im) + ((d_w,) if d_w is not None else ()):
        a.free()
    return out


_CASES = {}


def _case(pkg, name):
    """One device run of a case without weights and its references, computed once and shared: the engine (basis set), Q, the input x,
    the device result `out`, the complex128 reference `ref` and the worst row errors of the device and of the complex64 statement."""
    if name in _CASES:
        return _CASES[name]
    nt, nr, npkt, spec = CASES[name]
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    Q = _basis(pkg, spec)
    e.subspace_set_basis(Q)
    x = _planes(np.random.default_rng(len(name) + 7 * npkt), (npkt, nr, nt, N))
    out = _run(e, x)
    ref = sr.smooth(x, Q)
    c = dict(e=e, Q=Q, x=x, out=out, ref=ref, nt=nt, nr=nr, npkt=npkt, rank=Q.shape[1],
             dev_err=float(sr.row_err(out, ref, x).max()), np_err=float(sr.row_err(sr.smooth(x, Q, None, np.complex64), ref, x).max()))
    _CASES[name] = c
    return c


# ---------------------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize('name', list(CASES))
def test_a_accuracy_beside_the_complex64_statement(pkg, name):
    """max over rows of |dev - fp64| / |x_row| against the same quantity of the numpy complex64 statement on the same inputs: at most
    ORDER times as large.  Both carry the rounding of Q to float32.  Measured on the MI355X: profiles/subspace_smooth.txt."""
    k = _case(pkg, name)
    print('%s: device %.3e, numpy complex64 %.3e (ratio %.2f)' % (name, k['dev_err'], k['np_err'], k['dev_err'] / k['np_err']))
    assert np.isfinite(k['out'].view(np.float32)).all()
    assert k['dev_err'] <= ORDER * k['np_err']


@pytest.mark.parametrize('name', ['rows24_rank13', 'rows592_rank64', 'rows24_random13'])
def test_b_projection(pkg, name):
    """Rows inside the subspace come back, rows orthogonal to it come back as zero - each within the bound of test_a for these inputs,
    beside what rounding the rows to float32 leaves outside / inside the subspace (taken from the complex128 reference: 1e-7 at most)."""
    k = _case(pkg, name)
    e, Q, shape = k['e'], k['Q'], k['x'].shape
    rng = np.random.default_rng(41)
    coef = rng.standard_normal(shape[:3] + (k['rank'],)) + 1j * rng.standard_normal(shape[:3] + (k['rank'],))
    inside = (coef @ Q.T).astype(np.complex64)
    z = _planes(rng, shape).astype(np.complex128)
    outside = (z - (z @ Q.conj()) @ Q.T).astype(np.complex64)
    for what, x, want in (('inside', inside, inside), ('orthogonal', outside, np.zeros_like(outside))):
        ref = sr.smooth(x, Q)
        bound = ORDER * sr.row_err(sr.smooth(x, Q, None, np.complex64), ref, x).max()
        left = sr.row_err(ref, want, x).max()
        got = sr.row_err(_run(e, x), want, x).max()
        print('%s %s: device off by %.3e of |x|, bound %.3e + rounding of the rows %.3e' % (name, what, got, bound, left))
        assert left <= 1e-7
        assert got <= bound + left


# ---------------------------------------------------------------------------------------------------------------- weights
@pytest.mark.parametrize('name', ['rows24_rank13', 'rows592_rank64', 'rows24_rank33'])
def test_c_weights(pkg, name):
    k = _case(pkg, name)
    e, Q, x = k['e'], k['Q'], k['x']
    wshape = (k['npkt'], k['nr'], k['rank'])
    assert np.array_equal(_bits(_run(e, x, np.ones(wshape, np.float32))), _bits(k['out'])), 'all ones = NULL'
    assert not _run(e, x, np.zeros(wshape, np.float32)).view(np.float32).any(), 'all zeros'
    w = np.random.default_rng(9).random(wshape, dtype=np.float32)
    got, ref = _run(e, x, w), sr.smooth(x, Q, w)
    err = sr.row_err(got, ref, x).max()
    np_err = sr.row_err(sr.smooth(x, Q, w, np.complex64), ref, x).max()
    print('%s weights per (packet, rx): device %.3e, numpy complex64 %.3e' % (name, err, np_err))
    assert err <= ORDER * np_err
    # a swapped rx or packet index would show
    assert sr.row_err(got, sr.smooth(x, Q, w[:, ::-1]), x).max() > 1e-2
    assert sr.row_err(got, sr.smooth(x, Q, w[::-1]), x).max() > 1e-2
    # the host entry point takes them too
    assert np.array_equal(_bits(e.subspace_smooth(x, w)), _bits(got))
    # robust weights of the delay window, one nu per (packet, rx)
    if name == 'rows592_rank64':
        _, lam = pkg.subspace.delay_basis(64, 8)
        wr = pkg.subspace.robust_weights(lam, np.random.default_rng(2).random(wshape[:2] + (1,)) + 0.01).astype(np.float32)
        ref = sr.smooth(x, Q, wr)
        assert sr.row_err(e.subspace_smooth(x, wr), ref, x).max() <= ORDER * sr.row_err(sr.smooth(x, Q, wr, np.complex64), ref, x).max()


# ---------------------------------------------------------------------------------------------------------------- batch independence
def test_d_bit_for_bit_identity(pkg):
    """The 592-row case: packets [a, b) alone (cuts at 5 - odd, 80 rows = 2.5 tiles -, 12 and 20), a second call, out aliasing in, a
    captured graph, and the host entry point of a context whose workspace_bytes holds 5 packets per chunk (8 chunks) all give the
    bits of the first call."""
    k = _case(pkg, 'rows592_rank64')
    e, x, want, npkt = k['e'], k['x'], _bits(k['out']), k['npkt']
    n0 = e.get_option('subspace_launches')
    for a, b in ((0, 5), (5, npkt), (12, 20)):
        assert np.array_equal(_bits(_run(e, x[a:b])), want[a:b]), (a, b)
    assert np.array_equal(_bits(_run(e, x)), want)
    assert e.get_option('subspace_launches') == n0 + 4, 'one launch per device call'
    # exact aliasing
    a_re, a_im = e.to_device(x.real), e.to_device(x.imag)
    e.subspace_smooth_device(a_re, a_im, npkt, a_re, a_im)
    e.synchronize()
    assert np.array_equal(_bits(_cplx(a_re.download(), a_im.download())), want)
    # a captured graph: nothing runs at capture, the replay gives the eager bits
    a_re.upload(x.real); a_im.upload(x.imag)
    o_re, o_im = e.to_device(np.zeros(x.shape, np.float32)), e.to_device(np.zeros(x.shape, np.float32))
    e.capture_begin()
    try:
        e.subspace_smooth_device(a_re, a_im, npkt, o_re, o_im)
    finally:
        g = e.capture_end()
    assert not o_re.download().any(), 'a captured call must not run'
    g.launch()
    e.synchronize()
    assert np.array_equal(_bits(_cplx(o_re.download(), o_im.download())), want)
    for a in (a_re, a_im, o_re, o_im):
        a.free()
    # host entry point, one chunk and several
    assert np.array_equal(_bits(e.subspace_smooth(x)), want)
    small = pkg.CsiEngine(k['nt'], k['nr'], hidden=(8,), workspace_bytes=5 * 4 * k['nr'] * k['nt'] * N * 4)
    small.subspace_set_basis(k['Q'])
    assert np.array_equal(_bits(small.subspace_smooth(x)), want)
    assert small.get_option('subspace_launches') == 8


def test_d_second_basis_replaces_the_first(pkg):
    k = _case(pkg, 'rows24_rank13')
    other = _case(pkg, 'rows24_random13')
    e = pkg.CsiEngine(k['nt'], k['nr'], hidden=(8,))
    e.subspace_set_basis(_basis(pkg, ('delay', 128, 16)))
    e.subspace_set_basis(k['Q'])
    assert np.array_equal(_bits(_run(e, k['x'])), _bits(k['out']))
    e.subspace_set_basis(other['Q'])
    assert np.array_equal(_bits(_run(e, other['x'])), _bits(other['out']))


# ---------------------------------------------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize('name', ['rows24_rank13', 'rows592_rank64', 'rows36_rank96'])
def test_e_guard_bands(pkg, name):
    """Every plane and w as exact-size slices between NaN / 3e38 guards: no guard word damaged, every output word written, nothing of
    an input guard in a result, inputs unchanged, and the bits of the call on plain arrays."""
    k = _case(pkg, name)
    e, x, npkt = k['e'], k['x'], k['npkt']
    w = np.random.default_rng(5).random((npkt, k['nr'], k['rank']), dtype=np.float32)
    plain = _run(e, x, w)
    g_in = dict(h_re=Guarded(e, x.shape, 'in', np.ascontiguousarray(x.real), name='h_re'),
                h_im=Guarded(e, x.shape, 'in', np.ascontiguousarray(x.imag), name='h_im'), w=Guarded(e, w.shape, 'in', w, name='w'))
    g_out = dict(out_re=Guarded(e, x.shape, 'out', name='out_re'), out_im=Guarded(e, x.shape, 'out', name='out_im'))
    e.subspace_smooth_device(g_in['h_re'], g_in['h_im'], npkt, g_out['out_re'], g_out['out_im'], g_in['w'])
    e.synchronize()
    for a in list(g_in.values()) + list(g_out.values()):
        a.check()
    for n, a in g_out.items():
        assert a.count_unwritten() == 0, n
        assert np.isfinite(a.download()).all(), n
    assert all(a.unchanged() for a in g_in.values())
    assert np.array_equal(_bits(_cplx(g_out['out_re'].download(), g_out['out_im'].download())), _bits(plain))
    # in place between guards
    e.subspace_smooth_device(g_in['h_re'], g_in['h_im'], npkt, g_in['h_re'], g_in['h_im'], g_in['w'])
    e.synchronize()
    for a in g_in.values():
        a.check()
    assert np.array_equal(_bits(_cplx(g_in['h_re'].download(), g_in['h_im'].download())), _bits(plain))
    for a in list(g_in.values()) + list(g_out.values()):
        a.free()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_f_refusals_carry_text(pkg):
    nt, nr, npkt = 4, 2, 2
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    lib, ctx = e._lib, e._ctx
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    h, o = [e.empty((npkt + 1, nr, nt, N)) for _ in range(2)], [e.empty((npkt + 1, nr, nt, N)) for _ in range(2)]
    host = np.zeros(npkt * nr * nt * N, np.float32)
    ok = (h[0].ptr, h[1].ptr, npkt, None, o[0].ptr, o[1].ptr)

    def refused(text, *args, code=-1, fn=lib.csi_subspace_smooth_device):
        assert fn(ctx, *args) == code, (text, args)
        assert text in lib.csi_last_error(ctx).decode(), lib.csi_last_error(ctx)
        assert e.get_option('subspace_launches') == launches

    launches = 0
    refused('no basis set', *ok, code=-2)
    refused('no basis set', fp(host), fp(host), npkt, None, fp(host), fp(host), code=-2, fn=lib.csi_subspace_smooth)
    Q, _ = pkg.subspace.delay_basis(8)
    q_re, q_im = np.ascontiguousarray(Q.real, np.float32), np.ascontiguousarray(Q.imag, np.float32)
    set_basis = lib.csi_subspace_set_basis
    refused('rank 0 outside 1 .. 128', fp(q_re), fp(q_im), 0, fn=set_basis)
    refused('rank 129 outside 1 .. 128', fp(q_re), fp(q_im), 129, fn=set_basis)
    refused('null basis planes', None, fp(q_im), 8, fn=set_basis)
    bad = q_re.copy(); bad[3, 2] = np.nan
    refused('non-finite basis entry at [3][2]', fp(bad), fp(q_im), 8, fn=set_basis)
    bad = q_re.copy(); bad[:, 1] = q_re[:, 0]
    skew = q_im.copy(); skew[:, 1] = q_im[:, 0]
    refused('not orthonormal', fp(bad), fp(skew), 8, fn=set_basis)
    refused('not orthonormal', fp(np.ascontiguousarray(1.001 * q_re)), fp(np.ascontiguousarray(1.001 * q_im)), 8, fn=set_basis)
    refused('no basis set', *ok, code=-2)          # a refused basis sets nothing
    e.subspace_set_basis(Q)
    refused('must not be negative', *(ok[:2] + (-1,) + ok[3:]))
    for i in (0, 1, 4, 5):
        refused('null required pointer', *(ok[:i] + (None,) + ok[i + 1:]))
    for i, name in ((0, 'd_h_re'), (1, 'd_h_im'), (4, 'd_out_re'), (5, 'd_out_im')):
        refused('%s must start on a 16-byte boundary' % name, *(ok[:i] + (ok[i] + 4,) + ok[i + 1:]))
    one_pkt = nr * nt * N * 4
    refused('overlap', h[0].ptr, h[1].ptr, npkt, None, h[0].ptr + one_pkt, o[1].ptr)          # out_re one packet into h_re
    refused('overlap', h[0].ptr, h[1].ptr, npkt, None, o[0].ptr, h[1].ptr + one_pkt)
    refused('overlap', h[0].ptr, h[1].ptr, npkt, None, h[1].ptr, h[0].ptr)                    # re and im crossed
    refused('overlap', h[0].ptr, h[1].ptr, npkt, None, o[0].ptr, o[0].ptr)                    # one output plane twice
    refused('must not be negative', fp(host), fp(host), -1, None, fp(host), fp(host), fn=lib.csi_subspace_smooth)
    refused('null required pointer', None, fp(host), npkt, None, fp(host), fp(host), fn=lib.csi_subspace_smooth)
    # npkt = 0 is no error and no launch; then one launch per device call
    assert lib.csi_subspace_smooth_device(ctx, *(ok[:2] + (0,) + ok[3:])) == 0 and e.get_option('subspace_launches') == 0
    for n in (1, 2):
        assert lib.csi_subspace_smooth_device(ctx, *ok) == 0
        assert e.get_option('subspace_launches') == n
    e.synchronize()
    with pytest.raises(pkg.CsiError, match='h must be'):
        e.subspace_smooth(np.zeros((1, nr, nt, 7), np.complex64))
    with pytest.raises(pkg.CsiError, match='weights must be'):
        e.subspace_smooth(np.zeros((1, nr, nt, N), np.complex64), np.ones((1, nr, 7), np.float32))
    with pytest.raises(pkg.CsiError, match='basis must be'):
        e.subspace_set_basis(np.zeros((7, 3)))
    one = pkg.CsiEngine(0, 1, hidden=(16,), len_ltf=64)
    assert one._lib.csi_subspace_smooth_device(one._ctx, *ok) == -1
    assert 'single-input context' in one._lib.csi_last_error(one._ctx).decode()
    assert one._lib.csi_subspace_set_basis(one._ctx, fp(q_re), fp(q_im), 8) == -1
    assert 'single-input context' in one._lib.csi_last_error(one._ctx).decode()


# ---------------------------------------------------------------------------------------------------------------- end to end
_LINKS = {}


def _links(pkg, oracle, snr):
    """Nt = 8, Nr = 2, 64 packets of synth_structured with the 8-tap profile: true channel, LS estimate and its projection onto the
    window (8, 0), complex64 [64, 2, 8, 234] each"""
    if snr in _LINKS:
        return _LINKS[snr]
    nt, nr, npkt = 8, 2, 64
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(oracle.hadamard(nt))
    e.subspace_set_basis(pkg.subspace.delay_basis(8, 0)[0])
    d_re, d_im, h_re, h_im, _ = e.synth_structured(21, 0, npkt, snr_db=snr, n_taps=8, want_noise_std=False)
    shape = (npkt, nr, nt, N)
    ls_re, ls_im, o_re, o_im = (e.empty(shape) for _ in range(4))
    e.ls_estimate_device(d_re, d_im, npkt, ls_re, ls_im)
    e.subspace_smooth_device(ls_re, ls_im, npkt, o_re, o_im)
    e.synchronize()
    _LINKS[snr] = tuple(_cplx(a.download(), b.download()) for a, b in ((h_re, h_im), (ls_re, ls_im), (o_re, o_im)))
    e.close()
    return _LINKS[snr]


def test_g_noise_free_channel_is_kept(pkg, oracle):
    h, ls, dly = _links(pkg, oracle, None)
    n_ls, n_dly = sr.nmse(ls, h), sr.nmse(dly, h)
    print('noise-free: NMSE LS %.4e, DLY %.4e' % (n_ls, n_dly))
    assert n_dly <= 2.0 * n_ls


@pytest.mark.parametrize('snr', [-10.0, 10.0])
def test_g_gain_over_ls_is_rank_over_carriers(pkg, oracle, snr):
    """NMSE(DLY) / NMSE(LS) within 10 % of r / 234 = 8 / 234: the expected value for white LS error and a channel inside the window.
    1024 links of 8 taps: the spread of the ratio is under 1 %.  In numpy fp64 the ratio was 0.0337 and 0.0340 against 0.0342."""
    h, ls, dly = _links(pkg, oracle, snr)
    n_ls, n_dly = sr.nmse(ls, h), sr.nmse(dly, h)
    want = 8.0 / N
    print('snr %g: NMSE LS %.4e, DLY %.4e, ratio %.5f against r / 234 = %.5f' % (snr, n_ls, n_dly, n_dly / n_ls, want))
    assert abs(n_dly / n_ls - want) <= 0.1 * want


# ---------------------------------------------------------------------------------------------------------------- sweep
def test_h_sweep_with_the_delay_estimator(pkg, oracle, tmp_path):
    """A miniature sweep (Nt 4, Nr 2, hidden (16, 16), random weights from a model folder, two levels of 6 packets) with and without
    delay_taps=8: the option adds MSE_DLY, below MSE_LS at both levels, and leaves MSE_LS, MSE_MMSE and MSE_DNN bit-identical."""
    import json
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    from dl_channel_estimation_mamimo_amd.model import save_weight_file
    nt, nr, hidden, levels = 4, 2, (16, 16), (-10.0, 10.0)
    rng = np.random.default_rng(8)
    models = str(tmp_path / 'models')
    os.makedirs(models)
    for d in ('real', 'imag'):
        w = {n: v for n, v in oracle.make_weights(rng, 321 * nt, list(hidden), 234).items() if isinstance(v, np.ndarray)}
        save_weight_file(os.path.join(models, d + '_weights-improvement.safetensors'), w)
    res = {}
    for taps in (None, 8):
        e = pkg.CsiEngine(nt, nr, hidden=hidden)
        e.set_pilot(oracle.hadamard(nt))
        out = str(tmp_path / ('delay' if taps else 'plain'))
        res[taps] = sweep.run_sweep(e, out, levels=levels, n_train=8, n_test=6, seed=3, modeldir=models, verbose=False, delay_taps=taps)
        res[taps]['dir'] = out
    for snr in levels:
        a, b = (loadmat(os.path.join(res[t]['dir'], 'BS%d_SNR%g' % (nt, snr), 'metrics.mat')) for t in (None, 8))
        assert {k for k in a if not k.startswith('__')} == {'MSE_LS', 'MSE_MMSE', 'MSE_DNN'}
        assert {k for k in b if not k.startswith('__')} == {'MSE_LS', 'MSE_MMSE', 'MSE_DNN', 'MSE_DLY'}
        for f in ('MSE_LS', 'MSE_MMSE', 'MSE_DNN'):
            assert np.array_equal(a[f].view(np.uint64), b[f].view(np.uint64)), (snr, f)
        assert b['MSE_DLY'].shape == (1, 6) and np.isfinite(b['MSE_DLY']).all()
        print('snr %g: LS %.4e, MMSE %.4e, DLY %.4e' % (snr, b['MSE_LS'].mean(), b['MSE_MMSE'].mean(), b['MSE_DLY'].mean()))
        assert b['MSE_DLY'].mean() < b['MSE_LS'].mean()
    plain = json.load(open(os.path.join(res[None]['dir'], 'sweep.json')))
    with_d = json.load(open(os.path.join(res[8]['dir'], 'sweep.json')))
    assert 'delay' not in plain and all('DLY' not in lv for lv in plain['levels'])
    assert with_d['delay'] == dict(taps=8, pre=0, rank=8) and all('DLY' in lv for lv in with_d['levels'])
