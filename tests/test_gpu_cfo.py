"""GPU tests of the carrier-frequency-offset stage (csi_cfo_estimate_device, csi_cfo_rotate_device, csi_cfo_correct[_device];
csrc/cfo.hip.h) against the fp64 statement tests/cfo_ref.py on the downloaded float32 inputs.

Tolerances, each fixed before the first device run (measured ratios: profiles/cfo.txt):
  estimate  |eps_hat_dev - eps_hat_ref| modulo 1 <= 8 2^-24 / (2 pi quality_ref): a product of fp32 inputs carries at most four
            roundings relative to |a| |b|, sum |a| |b| <= E, the fp64 sums add nothing, a factor 2 of slack; an error d of gamma turns
            its angle by at most d / |gamma| = d / (E quality).  quality: 8 2^-24.  The all-zero packet returns exactly (0, 0).
  rotate    per sample |y_dev - y_ref| <= 2^-20 |x|: the rounding of the reduced turn count (2 pi 2^-25), the sine and cosine and the
            complex product come to about 8 2^-24, doubled.  The eps = 0 packet is bit-identical to the input.
  through LS: the corrected packets get 4 times the rel_rows figure of the unrotated packets on the same engine (two rotations add
            rounding of the order of the transform's own); the uncorrected ones must stand above 1000 times it."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfo_ref as cr      # noqa: E402
import guarded as G      # noqa: E402
from conftest import rel_rows      # noqa: E402

U = 2.0 ** -24
EPS_BOUND = 8.0 * U / (2.0 * np.pi)      # over quality_ref
Q_BOUND = 8.0 * U
ROT_BOUND = 2.0 ** -20
SHAPES = [(4, 1, 5), (8, 2, 3), (128, 1, 2)]
_cache = {}


def _engine(pkg, nt, nr, **kw):
    return pkg.CsiEngine(nt, nr, hidden=(8,), **kw)


def _packets(oracle, nt, nr, npkt, snr_db):
    """float32 planes of oracle packets under offsets |eps| <= 0.45 (the first +0.45, the next -0.45), the last packet all zero;
    computed once per case"""
    key = (nt, nr, npkt, snr_db)
    if key not in _cache:
        rng = np.random.default_rng(1000 * nt + 10 * nr + npkt)
        ltf, _ = oracle.make_structured_packets(rng, npkt, nr, oracle.hadamard(nt), snr_db=snr_db)
        eps = np.concatenate([[0.45, -0.45], rng.uniform(-0.45, 0.45, npkt)])[:npkt]
        y = cr.rotate(ltf, eps)
        y[-1] = 0.0
        re, im = np.ascontiguousarray(y.real, np.float32), np.ascontiguousarray(y.imag, np.float32)
        _cache[key] = (re, im, eps)
    return _cache[key]


def _f64(d):
    """a DeviceArray [n, 2] of float32 words as float64 [n]"""
    return d.download().view(np.float64)[..., 0].copy()


def _eps_up(e, eps):
    return e.to_device(np.ascontiguousarray(eps, np.float64).view(np.float32).reshape(-1, 2))


def _estimate(e, re, im, cp_skip):
    npkt = re.shape[0]
    d_re, d_im, d_eps, d_q = e.to_device(re), e.to_device(im), e.empty((npkt, 2)), e.empty((npkt,))
    e.cfo_estimate_device(d_re, d_im, npkt, d_eps, cp_skip=cp_skip, d_quality=d_q)
    e.synchronize()
    out = _f64(d_eps), d_q.download()
    for a in (d_re, d_im, d_eps, d_q):
        a.free()
    return out


@pytest.mark.parametrize('snr_db', [None, -10.0], ids=['noise-free', '-10dB'])
@pytest.mark.parametrize('cp_skip', [0, 16, 63])
@pytest.mark.parametrize('nt,nr,npkt', SHAPES)
def test_a_estimate_against_the_fp64_statement(pkg, oracle, nt, nr, npkt, cp_skip, snr_db):
    re, im, eps = _packets(oracle, nt, nr, npkt, snr_db)
    e = _engine(pkg, nt, nr)
    got, quality = _estimate(e, re, im, cp_skip)
    want, q_ref = cr.estimate(re.astype(np.float64) + 1j * im.astype(np.float64), cp_skip)
    live = slice(0, npkt - 1)
    err = np.abs(cr.wrap(got - want))[live]
    bound = EPS_BOUND / q_ref[live]
    print(f'Nt {nt} Nr {nr} npkt {npkt} cp_skip {cp_skip} {"noise-free" if snr_db is None else "%g dB" % snr_db}: eps_hat error / bound '
          f'{(err / bound).max():.3f} (quality {q_ref[live].min():.3f} .. {q_ref[live].max():.3f}), quality error / bound '
          f'{np.abs(quality[live] - q_ref[live]).max() / Q_BOUND:.3f}')
    assert (err <= bound).all(), (err, bound)
    assert np.abs(quality - q_ref).max() <= Q_BOUND
    if snr_db is None:
        assert np.abs(cr.wrap(got[live] - eps[live])).max() < 1e-6          # the offset itself came back
    assert got[-1] == 0.0 and not np.signbit(got[-1]) and quality[-1] == 0.0      # the all-zero packet


def _rotate_case(nt, nr, npkt):
    rng = np.random.default_rng(nt)
    shape = (npkt, nr, 320 * nt)
    re, im = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    eps = np.array([0.49999, 0.0, -0.49999][:npkt])
    return re, im, eps


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
@pytest.mark.parametrize('scale', [1.0, -1.0])
@pytest.mark.parametrize('nt,nr,npkt', [(4, 1, 3), (128, 1, 2)])
def test_b_rotate_against_the_fp64_statement(pkg, nt, nr, npkt, scale, in_place):
    re, im, eps = _rotate_case(nt, nr, npkt)
    e = _engine(pkg, nt, nr)
    d_re, d_im, d_eps = e.to_device(re), e.to_device(im), _eps_up(e, eps)
    o_re, o_im = (d_re, d_im) if in_place else (e.empty(re.shape), e.empty(re.shape))
    e.cfo_rotate_device(d_re, d_im, npkt, d_eps, scale, *(() if in_place else (o_re, o_im)))
    e.synchronize()
    y_re, y_im = o_re.download(), o_im.download()
    if not in_place:
        assert np.array_equal(d_re.download().view(np.uint32), re.view(np.uint32)) and np.array_equal(d_im.download().view(np.uint32), im.view(np.uint32))
    x = re.astype(np.float64) + 1j * im.astype(np.float64)
    want = cr.rotate(x, eps, scale)
    ratio = np.abs((y_re.astype(np.float64) + 1j * y_im.astype(np.float64)) - want) / (ROT_BOUND * np.abs(x))
    print(f'Nt {nt} npkt {npkt} scale {scale:+g} {"in place" if in_place else "out of place"}: |y_dev - y_ref| / (2^-20 |x|) <= {ratio.max():.3f} '
          f'({80 * nt * 0.49999 / 64:.1f} turns at the end of a packet)')
    assert ratio.max() <= 1.0
    assert np.array_equal(y_re[1].view(np.uint32), re[1].view(np.uint32)) and np.array_equal(y_im[1].view(np.uint32), im[1].view(np.uint32))      # eps = 0


@pytest.mark.parametrize('cp_skip', [0, 63])
@pytest.mark.parametrize('nt,nr,npkt', [(8, 2, 3), (128, 1, 2)])
def test_c_correct_is_estimate_then_rotate(pkg, oracle, nt, nr, npkt, cp_skip):
    re, im, _ = _packets(oracle, nt, nr, npkt, -10.0)
    e = _engine(pkg, nt, nr)
    d_re, d_im = e.to_device(re), e.to_device(im)
    d_eps, d_q, a_re, a_im = e.empty((npkt, 2)), e.empty((npkt,)), e.empty(re.shape), e.empty(re.shape)
    n0 = e.get_option('cfo_launches')
    e.cfo_estimate_device(d_re, d_im, npkt, d_eps, cp_skip=cp_skip, d_quality=d_q)
    e.cfo_rotate_device(d_re, d_im, npkt, d_eps, -1.0, a_re, a_im)
    assert e.get_option('cfo_launches') == n0 + 2
    c_eps, c_q, b_re, b_im = e.empty((npkt, 2)), e.empty((npkt,)), e.empty(re.shape), e.empty(re.shape)
    e.cfo_correct_device(d_re, d_im, npkt, b_re, b_im, cp_skip=cp_skip, d_eps=c_eps, d_quality=c_q)
    assert e.get_option('cfo_launches') == n0 + 4                     # at most two launches
    k_re, k_im = e.empty(re.shape), e.empty(re.shape)
    e.cfo_correct_device(d_re, d_im, npkt, k_re, k_im, cp_skip=cp_skip)      # eps kept by the engine
    e.synchronize()
    bits = lambda a: a.download().view(np.uint32)      # noqa: E731
    assert np.array_equal(bits(c_eps), bits(d_eps)) and np.array_equal(bits(c_q), bits(d_q))
    for x, y in ((b_re, a_re), (b_im, a_im), (k_re, a_re), (k_im, a_im)):
        assert np.array_equal(bits(x), bits(y))
    # the host twin: the device path's bits
    out, h_eps, h_q = e.cfo_correct(re + 1j * im, cp_skip=cp_skip, details=True)
    assert np.array_equal(out.real.view(np.uint32), bits(a_re)) and np.array_equal(out.imag.view(np.uint32), bits(a_im))
    assert np.array_equal(h_eps.view(np.uint64), _f64(d_eps).view(np.uint64)) and np.array_equal(h_q.view(np.uint32), bits(d_q))
    # ... and in chunks of one packet
    small = _engine(pkg, nt, nr, workspace_bytes=2 * nr * 320 * nt * 4)
    out1, eps1, q1 = small.cfo_correct(re + 1j * im, cp_skip=cp_skip, details=True)
    assert np.array_equal(out1.view(np.uint64), out.view(np.uint64)) and np.array_equal(eps1.view(np.uint64), h_eps.view(np.uint64))
    assert np.array_equal(q1.view(np.uint32), h_q.view(np.uint32))


def test_d_same_bits_whatever_the_call(pkg, oracle):
    nt, nr, npkt = 8, 2, 5
    re, im, _ = _packets(oracle, nt, nr, npkt, -10.0)
    e = _engine(pkg, nt, nr)
    first = _estimate(e, re, im, 16)
    again = _estimate(e, re, im, 16)
    assert np.array_equal(first[0].view(np.uint64), again[0].view(np.uint64)) and np.array_equal(first[1].view(np.uint32), again[1].view(np.uint32))
    part = _estimate(e, re[1:3], im[1:3], 16)
    assert np.array_equal(part[0].view(np.uint64), first[0][1:3].view(np.uint64)) and np.array_equal(part[1].view(np.uint32), first[1][1:3].view(np.uint32))

    def fixed(r, i):
        d = e.to_device(r), e.to_device(i)
        e.cfo_correct_device(d[0], d[1], r.shape[0])
        e.synchronize()
        return d[0].download().view(np.uint32), d[1].download().view(np.uint32)
    whole, whole2, sub = fixed(re, im), fixed(re, im), fixed(re[1:3], im[1:3])
    assert np.array_equal(whole[0], whole2[0]) and np.array_equal(whole[1], whole2[1])
    assert np.array_equal(sub[0], whole[0][1:3]) and np.array_equal(sub[1], whole[1][1:3])


def test_e_through_the_ls_estimate(pkg, oracle):
    """synth_structured noise-free at (8, 2, 4) -> rotate(+eps) -> correct -> ls_estimate_device against the generator's h"""
    nt, nr, npkt = 8, 2, 4
    e = _engine(pkg, nt, nr)
    e.set_pilot(oracle.hadamard(nt))
    d_re, d_im, h_re, h_im, _ = e.synth_structured(5, 0, npkt, snr_db=None, want_noise_std=False)
    eps = np.array([0.4, -0.4, 0.013, -0.27])
    d_eps = _eps_up(e, eps)
    r_re, r_im, c_re, c_im = (e.empty((npkt, nr, 320 * nt)) for _ in range(4))
    e.cfo_rotate_device(d_re, d_im, npkt, d_eps, 1.0, r_re, r_im)
    e.cfo_correct_device(r_re, r_im, npkt, c_re, c_im)
    l_re, l_im = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
    truth = np.concatenate([h_re.download(), h_im.download()], -1)

    def ls(a_re, a_im):
        e.ls_estimate_device(a_re, a_im, npkt, l_re, l_im)
        e.synchronize()
        return rel_rows(np.concatenate([l_re.download(), l_im.download()], -1), truth)
    clean, offset, fixed = ls(d_re, d_im), ls(r_re, r_im), ls(c_re, c_im)
    print(f'LS rows against the generator\'s h: unrotated {clean:.3e}, under the offset {offset:.3e} ({offset / clean:.3g} x), corrected {fixed:.3e} '
          f'({fixed / clean:.3f} x)')
    assert fixed <= 4.0 * clean, (fixed, clean)
    assert offset > 1000.0 * clean, (offset, clean)


def test_f_guard_bands_on_every_output(pkg, oracle):
    nt, nr, npkt = 8, 2, 3
    re, im, _ = _packets(oracle, nt, nr, npkt, -10.0)
    e = _engine(pkg, nt, nr)
    shape = re.shape
    g_re, g_im = G.Guarded(e, shape, 'in', re, 'ltf_re'), G.Guarded(e, shape, 'in', im, 'ltf_im')
    for cp_skip in (0, 63):
        g_eps, g_q = G.Guarded(e, (npkt, 2), 'out', name='eps'), G.Guarded(e, (npkt,), 'out', name='quality')
        e.cfo_estimate_device(g_re, g_im, npkt, g_eps, cp_skip=cp_skip, d_quality=g_q)
        e.synchronize()
        for g in (g_re, g_im, g_eps, g_q):
            g.check()
        assert g_eps.count_unwritten() == 0 and g_q.count_unwritten() == 0 and g_re.unchanged() and g_im.unchanged()
        want = _estimate(e, re, im, cp_skip)
        assert np.array_equal(g_eps.download().view(np.float64)[..., 0].view(np.uint64), want[0].view(np.uint64))      # the guards' values reached nothing
        assert np.array_equal(g_q.download().view(np.uint32), want[1].view(np.uint32))
        o_re, o_im = G.Guarded(e, shape, 'out', name='out_re'), G.Guarded(e, shape, 'out', name='out_im')
        e.cfo_rotate_device(g_re, g_im, npkt, g_eps, -1.0, o_re, o_im)
        e.synchronize()
        k_re, k_im = G.Guarded(e, shape, 'out', name='cor_re'), G.Guarded(e, shape, 'out', name='cor_im')
        k_eps, k_q = G.Guarded(e, (npkt, 2), 'out', name='cor_eps'), G.Guarded(e, (npkt,), 'out', name='cor_quality')
        e.cfo_correct_device(g_re, g_im, npkt, k_re, k_im, cp_skip=cp_skip, d_eps=k_eps, d_quality=k_q)
        e.synchronize()
        for g in (g_re, g_im, g_eps, o_re, o_im, k_re, k_im, k_eps, k_q):
            g.check()
            assert g.fill == 'in' or g.count_unwritten() == 0, g.name
        assert g_re.unchanged() and g_im.unchanged()
        assert np.array_equal(k_re.download().view(np.uint32), o_re.download().view(np.uint32))
        assert np.array_equal(k_im.download().view(np.uint32), o_im.download().view(np.uint32))
        for g in (g_eps, g_q, o_re, o_im, k_re, k_im, k_eps, k_q):
            g.free()
    # in place: the payload is the input and the output
    i_re, i_im = G.Guarded(e, shape, 'out', name='inplace_re').upload(re), G.Guarded(e, shape, 'out', name='inplace_im').upload(im)
    e.cfo_correct_device(i_re, i_im, npkt)
    e.synchronize()
    i_re.check(), i_im.check()
    fixed = e.cfo_correct(re + 1j * im)
    assert np.array_equal(i_re.download().view(np.uint32), fixed.real.view(np.uint32)) and np.array_equal(i_im.download().view(np.uint32), fixed.imag.view(np.uint32))


def test_g_refusals_carry_text_and_write_nothing(pkg):
    nt, nr, npkt = 4, 2, 2
    e = _engine(pkg, nt, nr)
    lib, ctx = e._lib, e._ctx
    shape = (npkt + 1, nr, 320 * nt)
    x = [G.Guarded(e, shape, 'out', name='x%d' % i).upload(np.ones(shape, np.float32)) for i in range(2)]
    y = [G.Guarded(e, shape, 'out', name='y%d' % i) for i in range(2)]
    eps, q = G.Guarded(e, (npkt + 1, 2), 'out', name='eps'), G.Guarded(e, (npkt + 1,), 'out', name='quality')
    est, rot, cor = lib.csi_cfo_estimate_device, lib.csi_cfo_rotate_device, lib.csi_cfo_correct_device
    ok_est = (x[0].ptr, x[1].ptr, npkt, 0, eps.ptr, q.ptr)
    ok_rot = (x[0].ptr, x[1].ptr, npkt, eps.ptr, 1.0, y[0].ptr, y[1].ptr)
    ok_cor = (x[0].ptr, x[1].ptr, npkt, 0, y[0].ptr, y[1].ptr, eps.ptr, q.ptr)
    sub = lambda ok, i, val: ok[:i] + (val,) + ok[i + 1:]      # noqa: E731
    pkt = nr * 320 * nt * 4

    def refused(text, fn, *args):
        assert fn(ctx, *args) == -1, (text, args)
        assert text in lib.csi_last_error(ctx).decode(), (text, lib.csi_last_error(ctx))
        assert e.get_option('cfo_launches') == 0

    for fn, ok in ((est, ok_est), (rot, ok_rot), (cor, ok_cor)):
        name = 'd_in' if fn is rot else 'd_ltf'
        refused('npkt 0 must be at least 1', fn, *sub(ok, 2, 0))
        refused('npkt -3 must be at least 1', fn, *sub(ok, 2, -3))
        refused('exceed one launch', fn, *sub(ok, 2, 2 ** 31))
        for i in (0, 1):
            refused('null required pointer (%s_re, %s_im)' % (name, name), fn, *sub(ok, i, None))
            refused('must start on a 16-byte boundary', fn, *sub(ok, i, ok[i] + 8))
    for fn, ok in ((est, ok_est), (cor, ok_cor)):
        refused('cp_skip -1 outside 0 .. 63', fn, *sub(ok, 3, -1))
        refused('cp_skip 64 outside 0 .. 63', fn, *sub(ok, 3, 64))
    refused('null required pointer (d_eps)', est, *sub(ok_est, 4, None))
    refused('null required pointer (d_eps)', rot, *sub(ok_rot, 3, None))
    refused('d_eps must be aligned for 8-byte words', est, *sub(ok_est, 4, eps.ptr + 4))
    refused('d_eps must be aligned for 8-byte words', rot, *sub(ok_rot, 3, eps.ptr + 4))
    refused('d_quality for 4-byte words', cor, *sub(ok_cor, 7, q.ptr + 2))
    refused('d_eps / d_quality overlap a plane or each other', est, *sub(ok_est, 4, x[1].ptr + 64))
    refused('d_eps / d_quality overlap a plane or each other', est, *sub(ok_est, 5, eps.ptr + 8))
    refused('d_eps / d_quality overlap a plane or each other', rot, *sub(ok_rot, 3, y[0].ptr))
    refused('scale nan must be finite', rot, *sub(ok_rot, 4, float('nan')))
    for fn, ok, i in ((rot, ok_rot, 5), (cor, ok_cor, 4)):
        for j in (i, i + 1):
            refused('null required pointer (d_out_re, d_out_im)', fn, *sub(ok, j, None))
            refused('must start on a 16-byte boundary', fn, *sub(ok, j, ok[j] + 4))
        refused('any other overlap of the planes is refused', fn, *sub(ok, i, x[0].ptr + pkt))          # partial overlap with its own input
        refused('any other overlap of the planes is refused', fn, *sub(ok, i, x[1].ptr))                # re onto im
        refused('any other overlap of the planes is refused', fn, *sub(ok, i + 1, ok[i] + 16))           # the outputs onto each other
    hp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))      # noqa: E731
    host = np.ones(2 * (npkt + 1) * nr * 320 * nt, np.float32)
    half = host.size // 2
    kept = host.copy()
    twin = lib.csi_cfo_correct
    refused('npkt 0 must be at least 1', twin, hp(host), hp(host[half:]), 0, 0, hp(host), hp(host[half:]), None, None)
    refused('cp_skip 64 outside 0 .. 63', twin, hp(host), hp(host[half:]), npkt, 64, hp(host), hp(host[half:]), None, None)
    refused('null required pointer (ltf_re, ltf_im, out_re, out_im)', twin, hp(host), None, npkt, 0, hp(host), hp(host[half:]), None, None)
    refused('any other overlap of the planes is refused', twin, hp(host), hp(host[half:]), npkt, 0, hp(host[4:]), hp(host[half:]), None, None)
    assert np.array_equal(host, kept)
    e.synchronize()
    for g in x + y + [eps, q]:            # nothing was written
        g.check()
    assert all(g.count_unwritten() == g.n for g in y + [eps, q])
    with pytest.raises(pkg.CsiError, match='preambles must be'):
        e.cfo_correct(np.zeros((1, nr, 7), np.complex64))
    # the launches of every entry
    for fn, ok, n in ((est, ok_est, 1), (rot, ok_rot, 2), (cor, ok_cor, 4)):
        assert fn(ctx, *ok) == 0, lib.csi_last_error(ctx)
        assert e.get_option('cfo_launches') == n
    # an open capture: correct without d_eps needs an eager call of its shape in front
    e.capture_begin()
    try:
        assert est(ctx, *ok_est) == 0                       # recorded, counted, not run
        assert cor(ctx, *sub(sub(ok_cor, 6, None), 7, None)) == -1 and 'sized by an eager call' in lib.csi_last_error(ctx).decode()
        assert e.get_option('cfo_launches') == 5
    finally:
        e.capture_end()
    e.synchronize()
    names = [lib.csi_profile_kernel_name(i).decode() for i in range(lib.csi_profile_num_kernels())]
    assert 'cfo_corr' in names and 'cfo_rotate' in names
    one = pkg.CsiEngine(0, 1, hidden=(16,), len_ltf=64)
    for fn, ok in ((est, ok_est), (rot, ok_rot), (cor, ok_cor)):
        assert fn(one._ctx, *ok) == -1 and 'single-input context' in lib.csi_last_error(one._ctx).decode()
