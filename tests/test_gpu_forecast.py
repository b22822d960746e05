"""GPU tests of the channel forecast (csi_forecast_gram / fit / apply_device, csi_forecast[_device], csi_sounding_noise_device;
csrc/forecast.hip.h) against the fp64 statement tests/forecast_ref.py.

Tolerances, each fixed before the first device run (measured ratios: profiles/forecast.txt):
  gram   per entry |T_dev - T_fp64| / sqrt(T_ii T_qq) against the same quantity of the plain complex64 statement of the sum (products and
         a running sum in numpy complex64, np.cumsum: one chain of K terms).  The kernel sums K / 4 terms per wave in another order, so
         it gets ORDER = 4 times that yardstick, the factor tests/test_gpu_subspace.py and tests/test_gpu_beam.py grant for that.
  fit    |c_dev - c_ref| / max |c_ref| against 2^-24 + M^2 cond_2(G + ridge trace / M) 2^-52 (fp32 rounding of the result plus a
         backward-stable fp64 Cholesky); forecast_ref solves the device's own T in another order of the sums, so FIT = 4 times it.
         fit_err (formed from the fp64 c, rounded once): 2^-24 + FIT M^2 cond 2^-52 sum_a |c_a| |rhs_a| / energy.
  apply  per element (M + 2) 2^-24 sum_m |c_m| |x_m|, with the device's c.
  noise  one ulp of the result (np.spacing of the replayed value) per component: half an ulp of the fused multiply-add plus the few
         ulps of the device's logf / cosf in n, which |x| >= 2 |s n| in the test data keeps below the other half.
  end to end: the forecast NMSE of the device against forecast_ref on the downloaded inputs, relative: the device's figures were
         measured (2.4e-4 noise-free at cond 3.8e5, 2.2e-7 at 20 dB at cond 641; profiles/forecast.txt) and about four times each is
         granted, E2E = 1e-3 and 1e-6 (float32 rounding of T alone moves the noise-free figure by 2e-4)."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forecast_ref as fr      # noqa: E402

N = 234
NPKT = 3
ORDER = 4.0
FIT = 4.0
E2E = {'noise-free': 1e-3, '20 dB': 1e-6}


def _engine(pkg, nt, nr, **kw):
    return pkg.CsiEngine(nt, nr, hidden=(8,), **kw)


def _soundings(rng, P, shape, rho=0.97):
    """P correlated soundings (a first-order autoregression per element plus white noise), float32 planes as complex128"""
    x = np.empty((P,) + shape, np.complex128)
    cur = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    for i in range(P):
        x[i] = cur + 0.05 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
        cur = rho * np.exp(0.3j) * cur + np.sqrt(1 - rho * rho) * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    return x.astype(np.complex64).astype(np.complex128)


def _up(e, x):
    """lists of DeviceArrays (re, im) of the soundings x [P, ...]"""
    return [e.to_device(x[i].real) for i in range(x.shape[0])], [e.to_device(x[i].imag) for i in range(x.shape[0])]


def _dl(re, im):
    return re.download().astype(np.float64) + 1j * im.download().astype(np.float64)


def _info(d):
    return d.download().view(np.int32)


def _gram_dev(e, x, blocks, kf):
    """T of the blocks form: x [P, blocks, kf] -> complex128 [blocks, P, P]"""
    P = x.shape[0]
    re, im = _up(e, x)
    t = [e.empty((blocks, P, P)) for _ in range(2)]
    e.forecast_gram_blocks_device(re, im, blocks, kf, t[0], t[1])
    e.synchronize()
    out = (t[0].download(), t[1].download())
    for a in re + im + t:
        a.free()
    return out


def _gram_c64(x):
    """the plain complex64 statement: products and one running sum per entry in complex64; x [P, blocks, kf] -> [blocks, P, P]"""
    f = x.astype(np.complex64)
    P = f.shape[0]
    out = np.empty((f.shape[1], P, P), np.complex128)
    for i in range(P):
        for q in range(P):
            out[:, i, q] = np.cumsum(np.conj(f[i]) * f[q], axis=-1, dtype=np.complex64)[:, -1]
    return out


# (Nt, Nr, P): one block of one row; odd blocks off 16 bytes; the issue's flagship; two full tiles of rows; 16 rows and an odd block size.
# A context needs Nt % 4 == 0, so every shape runs through the blocks entry (3 Nr blocks of 234 Nt floats), the kernel of
# csi_forecast_gram_device; the shapes a context can have run through that entry too
GRAM_SHAPES = [(1, 1, 2), (3, 2, 5), (8, 2, 12), (32, 1, 16), (33, 2, 16)]


@pytest.mark.parametrize('nt,nr,P', GRAM_SHAPES)
def test_a_gram(pkg, nt, nr, P):
    rng = np.random.default_rng(100 + nt + P)
    e = _engine(pkg, 4, 1)
    blocks, kf = NPKT * nr, nt * N
    x = _soundings(rng, P, (blocks, kf))
    t_re, t_im = _gram_dev(e, x, blocks, kf)
    got = t_re.astype(np.float64) + 1j * t_im.astype(np.float64)
    ref = np.einsum('ibk,qbk->biq', x.conj(), x)
    scale = np.sqrt(np.einsum('bii,bqq->biq', ref.real, ref.real))
    err, yard = (np.abs(got - ref) / scale).max(), (np.abs(_gram_c64(x) - ref) / scale).max()
    print(f'gram nt {nt} nr {nr} P {P}: device {err:.3e}, complex64 running sum {yard:.3e} (ratio {err / yard:.3f}, granted {ORDER})')
    assert err < ORDER * yard, (err, yard)
    # Hermitian to the bit, the diagonal real
    assert np.array_equal(t_re, np.swapaxes(t_re, -1, -2)) and np.array_equal(t_im, -np.swapaxes(t_im, -1, -2))
    assert not t_im[:, np.arange(P), np.arange(P)].any()
    # a packet alone against the same packet inside the batch
    for p in (0, NPKT - 1):
        a_re, a_im = _gram_dev(e, x[:, p * nr:(p + 1) * nr], nr, kf)
        assert np.array_equal(a_re, t_re[p * nr:(p + 1) * nr]) and np.array_equal(a_im, t_im[p * nr:(p + 1) * nr]), p
    if nt % 4 == 0:      # the context's entry is that kernel
        c = _engine(pkg, nt, nr)
        re, im = _up(c, x.reshape(P, NPKT, nr, nt, N))
        t = [c.empty((NPKT, nr, P, P)) for _ in range(2)]
        c.forecast_gram_device(re, im, NPKT, t[0], t[1])
        c.synchronize()
        assert np.array_equal(t[0].download().reshape(blocks, P, P), t_re) and np.array_equal(t[1].download().reshape(blocks, P, P), t_im)
        assert c.get_option('forecast_launches') == 1 and 'forecast_gram' in c.profile()


def _fit_dev(e, T, M, d, ridge, pool):
    npkt, nr, P = T.shape[:3]
    t = [e.to_device(np.ascontiguousarray(T.real, np.float32)), e.to_device(np.ascontiguousarray(T.imag, np.float32))]
    c = [e.empty((npkt, nr, M)) for _ in range(2)]
    fe, info = e.empty((npkt, nr)), e.empty((npkt, nr))
    e.forecast_fit_device(t[0], t[1], P, npkt, M, d, c[0], c[1], ridge=ridge, pool_rx=pool, d_fit_err=fe, d_info=info)
    e.synchronize()
    return _dl(c[0], c[1]), fe.download(), _info(info)


# (P, M, d, ridge, pooled): the issue's flagship, M = 1, M = 8, M + d = P (one equation), ridge 0, pooled
FIT_CASES = [(12, 4, 4, 1e-5, False), (5, 1, 2, 1e-5, False), (16, 8, 4, 1e-5, False), (6, 3, 3, 1e-3, False), (9, 2, 1, 0.0, False),
             (12, 4, 4, 1e-5, True), (16, 8, 8, 1e-4, True)]


@pytest.mark.parametrize('P,M,d,ridge,pool', FIT_CASES)
def test_b_fit_on_the_devices_own_gram(pkg, P, M, d, ridge, pool):
    nt, nr = 8, 2
    rng = np.random.default_rng(200 + P + M)
    e = _engine(pkg, nt, nr)
    x = _soundings(rng, P, (NPKT, nr, nt, N))
    x[:, 1, 0] = 0.0                                   # one (packet, rx) of zero planes: the fallback, unless pooled
    re, im = _up(e, x)
    t = [e.empty((NPKT, nr, P, P)) for _ in range(2)]
    e.forecast_gram_device(re, im, NPKT, t[0], t[1])
    e.synchronize()
    T = _dl(t[0], t[1])
    got_c, got_fe, got_info = _fit_dev(e, T, M, d, ridge, pool)
    ref = fr.fit(T, M, d, ridge, pool)
    assert np.array_equal(got_info, ref['info']), (got_info, ref['info'])
    assert got_info[1, 0] == (0 if pool else 1) and got_info.sum() == (0 if pool else 1)
    if not pool:
        assert np.array_equal(got_c[1, 0], np.eye(1, M)[0]) and got_fe[1, 0] == 0.0
    worst = 0.0
    for p in range(NPKT):
        for r in range(nr):
            if ref['info'][p, r]:
                continue
            yard = 2.0 ** -24 + M * M * ref['cond'][p, r] * 2.0 ** -52
            err = np.abs(got_c[p, r] - ref['c'][p, r]).max() / np.abs(ref['c'][p, r]).max()
            worst = max(worst, err / yard)
            assert err < FIT * yard, (p, r, err, yard, ref['cond'][p, r])
    # fit_err = 1 - Re(c^H rhs) / energy from the fp64 c on both sides, rounded once to fp32: the yardstick of c on terms of size amp
    cond = np.where(np.isfinite(ref['cond']), ref['cond'], 0.0)
    fe_tol = 2.0 ** -24 + FIT * M * M * cond * 2.0 ** -52 * ref['amp']
    assert (np.abs(got_fe - ref['fit_err']) <= fe_tol).all(), (np.abs(got_fe - ref['fit_err']), fe_tol)
    if pool:
        assert np.array_equal(got_c[:, 0], got_c[:, 1]) and np.array_equal(got_fe[:, 0], got_fe[:, 1])
    print(f'fit P {P} M {M} d {d} ridge {ridge:g} pooled {pool}: worst |dc| / yardstick {worst:.3f} (granted {FIT}), cond up to {cond.max():.3g}, '
          f'fit_err within {np.abs(got_fe - ref["fit_err"]).max():.2e}')


@pytest.mark.parametrize('nt,nr,P,M', [(8, 2, 12, 4), (4, 3, 3, 1), (36, 1, 16, 8)])
def test_c_apply(pkg, nt, nr, P, M):
    rng = np.random.default_rng(300 + nt)
    e = _engine(pkg, nt, nr)
    x = _soundings(rng, P, (NPKT, nr, nt, N))
    c = (rng.standard_normal((NPKT, nr, M)) + 1j * rng.standard_normal((NPKT, nr, M))).astype(np.complex64)
    re, im = _up(e, x)
    d_c = [e.to_device(c.real), e.to_device(c.imag)]
    out = [e.empty((NPKT, nr, nt, N)) for _ in range(2)]
    e.forecast_apply_device(re, im, NPKT, M, d_c[0], d_c[1], out[0], out[1])
    e.synchronize()
    got = _dl(out[0], out[1])
    cd = c.astype(np.complex128)
    ref = fr.apply(x, cd)
    bound = (M + 2) * 2.0 ** -24 * sum(np.abs(cd[:, :, m, None, None]) * np.abs(x[P - 1 - m]) for m in range(M))
    ratio = (np.abs(got - ref) / bound).max()
    print(f'apply nt {nt} nr {nr} P {P} M {M}: worst |dy| / bound {ratio:.3f}')
    assert ratio < 1.0, ratio


def test_d_sequence_host_entry_and_capture(pkg):
    """csi_forecast_device = the three calls, csi_forecast = the device entry with a chunk smaller than the call, a captured replay"""
    nt, nr, P, M, d, npkt = 8, 2, 12, 4, 4, 5
    rng = np.random.default_rng(400)
    e = _engine(pkg, nt, nr)
    x = _soundings(rng, P, (npkt, nr, nt, N))
    re, im = _up(e, x)
    for pool in (False, True):
        t = [e.empty((npkt, nr, P, P)) for _ in range(2)]
        c = [e.empty((npkt, nr, M)) for _ in range(2)]
        y = [e.empty((npkt, nr, nt, N)) for _ in range(2)]
        fe, info = e.empty((npkt, nr)), e.empty((npkt, nr))
        e.forecast_gram_device(re, im, npkt, t[0], t[1])
        e.forecast_fit_device(t[0], t[1], P, npkt, M, d, c[0], c[1], pool_rx=pool, d_fit_err=fe, d_info=info)
        e.forecast_apply_device(re, im, npkt, M, c[0], c[1], y[0], y[1])
        e.synchronize()
        want = [a.download() for a in y + c + [fe, info]]
        n0 = e.get_option('forecast_launches')
        y2 = [e.empty((npkt, nr, nt, N)) for _ in range(2)]
        c2 = [e.empty((npkt, nr, M)) for _ in range(2)]
        fe2, info2 = e.empty((npkt, nr)), e.empty((npkt, nr))
        e.forecast_device(re, im, npkt, M, d, y2[0], y2[1], pool_rx=pool, d_c_re=c2[0], d_c_im=c2[1], d_fit_err=fe2, d_info=info2)
        e.synchronize()
        assert e.get_option('forecast_launches') == n0 + 3
        for a, w in zip(y2 + c2 + [fe2, info2], want):
            assert np.array_equal(a.download().view(np.int32), w.view(np.int32))
        # without the optional planes: c lives in the workspace
        y3 = [e.empty((npkt, nr, nt, N)) for _ in range(2)]
        e.forecast_device(re, im, npkt, M, d, y3[0], y3[1], pool_rx=pool)
        e.synchronize()
        assert np.array_equal(y3[0].download(), want[0]) and np.array_equal(y3[1].download(), want[1])
        # the host entry, one chunk and chunks of two packets
        out, hc, hfe, hinfo = e.forecast(x, M, d, pool_rx=pool, details=True)
        small = _engine(pkg, nt, nr, workspace_bytes=2 * (2 * P + 2) * nr * nt * N * 4)
        out_s, hc_s, hfe_s, hinfo_s = small.forecast(x, M, d, pool_rx=pool, details=True)
        assert small.get_option('forecast_launches') == 3 * 3
        small.close()
        for o, oc, ofe, oinfo in ((out, hc, hfe, hinfo), (out_s, hc_s, hfe_s, hinfo_s)):
            assert np.array_equal(o.real, want[0]) and np.array_equal(o.imag, want[1])
            assert np.array_equal(oc.real, want[2]) and np.array_equal(oc.imag, want[3])
            assert np.array_equal(ofe, want[4]) and np.array_equal(oinfo, want[5].view(np.int32))
        assert np.array_equal(e.forecast(x, M, d, pool_rx=pool), out)
    # one captured replay after the eager calls above (they sized the workspace)
    zero = np.zeros((npkt, nr, nt, N), np.float32)
    g_re, g_im = e.to_device(zero), e.to_device(zero)
    n0 = e.get_option('forecast_launches')
    e.capture_begin()
    try:
        e.forecast_device(re, im, npkt, M, d, g_re, g_im, pool_rx=True)
    finally:
        g = e.capture_end()
    assert not g_re.download().any(), 'a captured call must not run'
    assert e.get_option('forecast_launches') == n0 + 3
    g.launch()
    e.synchronize()
    assert np.array_equal(g_re.download(), want[0]) and np.array_equal(g_im.download(), want[1])
    # against fp64 end to end, loosely: the forecast of the statement from the same soundings
    ref_y = fr.forecast(x, M, d, 1e-5, True)[0]
    assert fr.nmse(want[0].astype(np.float64) + 1j * want[1], ref_y) < 1e-8


def test_e_noise(pkg):
    nt, nr, npkt, seed, first = 8, 2, 3, 91, 5
    rng = np.random.default_rng(500)
    e = _engine(pkg, nt, nr)
    shape = (npkt, nr, nt, N)
    mag = lambda: rng.uniform(0.5, 2.0, shape) * rng.choice([-1.0, 1.0], shape)      # noqa: E731
    x = (mag() + 1j * mag()).astype(np.complex64)
    v = np.array([[2e-3, 0.0], [1e-3, 5e-4], [0.0, 2e-3]], np.float32)
    d_x, d_v = [e.to_device(x.real), e.to_device(x.imag)], e.to_device(v)
    out = [e.empty(shape) for _ in range(2)]
    e.sounding_noise_device(seed, first, npkt, d_v, d_x[0], d_x[1], out[0], out[1])
    e.synchronize()
    got_re, got_im = out[0].download(), out[1].download()
    s = np.sqrt(np.float32(0.5) * v, dtype=np.float32).astype(np.float64)[:, :, None, None]
    n = fr.noise_normals(seed, first, npkt, nr, nt)
    ref = fr.sounding_noise(x.astype(np.complex128), v, seed, first)
    worst = 0.0
    for g, r, xx, nn in ((got_re, ref.real, x.real, n.real), (got_im, ref.imag, x.imag, n.imag)):
        assert (np.abs(xx) >= 2.0 * np.abs(s * nn)).all()                  # the premise of the tolerance
        worst = max(worst, (np.abs(g.astype(np.float64) - r) / np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)).max())
    print(f'noise: worst error {worst:.3f} ulp of the result')
    assert worst <= 1.0
    # v = 0 returns the input bits; the others moved
    for p, r in ((0, 1), (2, 0)):
        assert np.array_equal(got_re[p, r].view(np.int32), x.real[p, r].view(np.int32)) and np.array_equal(got_im[p, r].view(np.int32), x.imag[p, r].view(np.int32))
    assert not np.array_equal(got_re[1], x.real[1])
    rel = ((got_re[1, 0] - x.real[1, 0]).astype(np.float64) ** 2).mean() / (0.5 * 1e-3)
    assert abs(rel - 1.0) < 0.1, rel                                           # variance v / 2 per component
    # in place equals out of place; a packet's noise does not depend on the call
    e.sounding_noise_device(seed, first, npkt, d_v, d_x[0], d_x[1])
    e.synchronize()
    assert np.array_equal(d_x[0].download(), got_re) and np.array_equal(d_x[1].download(), got_im)
    d_x[0].upload(x.real); d_x[1].upload(x.imag)
    one = [e.empty((1,) + shape[1:]) for _ in range(2)]
    e.sounding_noise_device(seed, first + 1, 1, e.to_device(v[1:2]), e.to_device(x.real[1:2]), e.to_device(x.imag[1:2]), one[0], one[1])
    e.synchronize()
    assert np.array_equal(one[0].download()[0], got_re[1]) and np.array_equal(one[1].download()[0], got_im[1])
    assert 'sounding_noise' in e.profile()


def test_f_end_to_end_on_the_ageing_channel(pkg):
    """Nt = 8, Nr = 2, (P, M, d) = (12, 4, 4), 0.5 ms, 1 m/s: the planes of scatter_channel_at_device, the LS case with white error at
    20 dB; the device's forecast NMSE against forecast_ref on the downloaded inputs, and the conditions of use of the CPU test"""
    nt, nr, npkt, P, M, d, dt, seed = 8, 2, 2, 12, 4, 4, 0.5e-3, 31
    e = _engine(pkg, nt, nr)
    times = [-(P - 1 - i) * dt for i in range(P)] + [d * dt]
    h_re, h_im = e.scatter_channel_at(seed, 0, npkt, times, speed_mps=1.0, heading_az_deg=20.0, n_scat=100)
    re, im = [e.view(h_re, i) for i in range(P)], [e.view(h_im, i) for i in range(P)]
    e.synchronize()
    truth = _dl(e.view(h_re, P), e.view(h_im, P))
    y = [e.empty((npkt, nr, nt, N)) for _ in range(2)]

    def run(tag, hold_min):
        x = np.stack([_dl(a, b) for a, b in zip(re, im)])
        info = e.empty((npkt, nr))
        e.forecast_device(re, im, npkt, M, d, y[0], y[1], d_info=info)
        e.synchronize()
        got = _dl(y[0], y[1])
        ref_y, f = fr.forecast(x, M, d, 1e-5)
        dev, ref, hold = fr.nmse(got, truth), fr.nmse(ref_y, truth), fr.nmse(x[-1], truth)
        print(f'{tag}: hold {hold:.4f}, forecast device {dev:.6f}, fp64 {ref:.6f} (relative difference {abs(dev - ref) / ref:.2e}, granted {E2E[tag]}), '
              f'cond {f["cond"].max():.3g}')
        assert not _info(info).any() and not f['info'].any()
        assert abs(dev - ref) < E2E[tag] * ref, (dev, ref)
        return dev, hold

    dev, hold = run('noise-free', 0.4)
    assert dev <= 0.02 and hold >= 0.4, (dev, hold)
    # 20 dB: white error of 10^-2 x the mean element power on the P - 1 earlier soundings and on the newest (an LS estimate has it too)
    v = np.full((npkt, nr), 1e-2 * np.mean(np.abs(_dl(re[-1], im[-1])) ** 2), np.float32)
    d_v = e.to_device(v)
    for i in range(P):
        e.sounding_noise_device(seed ^ ((i + 1) << 32), 0, npkt, d_v, re[i], im[i])
    dev_n, hold_n = run('20 dB', 0.4)
    assert dev_n < 0.5 * hold_n, (dev_n, hold_n)


def test_g_refusals_carry_text(pkg):
    nt, nr, npkt, P, M = 4, 2, 2, 4, 2
    e = _engine(pkg, nt, nr)
    lib, ctx = e._lib, e._ctx
    x = [[e.empty((npkt + 1, nr, nt, N)) for _ in range(P)] for _ in range(2)]
    t, c, y = [e.empty((npkt, nr, P, P)) for _ in range(2)], [e.empty((npkt, nr, M)) for _ in range(2)], [e.empty((npkt + 1, nr, nt, N)) for _ in range(2)]
    fe, info, v = e.empty((npkt, nr)), e.empty((npkt, nr)), e.to_device(np.ones((npkt, nr), np.float32))
    arr = lambda planes, **kw: (ctypes.c_void_p * len(planes))(*[kw.get('at%d' % i, a.ptr) for i, a in enumerate(planes)])      # noqa: E731
    xr, xi = arr(x[0]), arr(x[1])
    launches = 0

    def refused(text, fn, *args):
        assert fn(ctx, *args) == -1, (text, args)
        assert text in lib.csi_last_error(ctx).decode(), (text, lib.csi_last_error(ctx))
        assert e.get_option('forecast_launches') == launches

    gram, fit, app, seq, noise = (lib.csi_forecast_gram_device, lib.csi_forecast_fit_device, lib.csi_forecast_apply_device, lib.csi_forecast_device,
                                  lib.csi_sounding_noise_device)
    ok_gram = (xr, xi, P, npkt, t[0].ptr, t[1].ptr)
    ok_fit = (t[0].ptr, t[1].ptr, P, npkt, M, 1, 1e-5, 0, c[0].ptr, c[1].ptr, fe.ptr, info.ptr)
    ok_app = (xr, xi, P, npkt, M, c[0].ptr, c[1].ptr, y[0].ptr, y[1].ptr)
    ok_seq = (xr, xi, P, npkt, M, 1, 1e-5, 0, y[0].ptr, y[1].ptr, c[0].ptr, c[1].ptr, fe.ptr, info.ptr)
    ok_noise = (7, 0, npkt, v.ptr, x[0][0].ptr, x[1][0].ptr, y[0].ptr, y[1].ptr)
    sub = lambda ok, i, val: ok[:i] + (val,) + ok[i + 1:]      # noqa: E731
    for fn, ok in ((gram, ok_gram), (app, ok_app), (seq, ok_seq)):
        refused('n_snd 1 outside 2 .. 16', fn, *sub(ok, 2, 1))
        refused('n_snd 17 outside 2 .. 16', fn, *sub(ok, 2, 17))
        refused('npkt -1 must not be negative', fn, *sub(ok, 3, -1))
        refused('exceed one launch', fn, *sub(ok, 3, 2 ** 31))
        refused('null required pointer (d_x_re)', fn, *sub(ok, 0, None))
        refused('null required pointer (d_x_im[1])', fn, *sub(ok, 1, arr(x[1], at1=None)))
        refused('d_x_re[2] must start on a 16-byte boundary', fn, *sub(ok, 0, arr(x[0], at2=x[0][2].ptr + 8)))
    refused('n_snd 1 outside 2 .. 16', fit, *sub(ok_fit, 2, 1))
    refused('npkt -1 must not be negative', fit, *sub(ok_fit, 3, -1))
    for fn, ok, i in ((fit, ok_fit, 4), (seq, ok_seq, 4)):
        refused('order 0 outside 1 .. 8', fn, *sub(ok, i, 0))
        refused('order 9 outside 1 .. 8', fn, *sub(ok, i, 9))
        refused('steps 0 must be at least 1', fn, *sub(ok, i + 1, 0))
        refused('order 2 + steps 3 exceed n_snd 4', fn, *sub(ok, i + 1, 3))
        refused('must be finite and not negative', fn, *sub(ok, i + 2, -1e-3))
        refused('must be finite and not negative', fn, *sub(ok, i + 2, float('nan')))
        refused('must be finite and not negative', fn, *sub(ok, i + 2, float('inf')))
        refused('unknown flag bits 0x2', fn, *sub(ok, i + 3, 2))
    refused('order 0 outside 1 .. min(8, n_snd 4)', app, *sub(ok_app, 4, 0))
    refused('order 5 outside 1 .. min(8, n_snd 4)', app, *sub(ok_app, 4, 5))
    for i in (4, 5):
        refused('null required pointer (d_t_re, d_t_im)', gram, *sub(ok_gram, i, None))
        refused('must start on a 16-byte boundary', gram, *sub(ok_gram, i, ok_gram[i] + 4))
    refused('the output d_t_re overlaps the input d_x_re[1]', gram, *sub(ok_gram, 4, x[0][1].ptr + 16))
    refused('the outputs d_t_re and d_t_im overlap', gram, *sub(ok_gram, 5, t[0].ptr))
    for i in (0, 1, 8, 9):
        refused('null required pointer (d_t_re, d_t_im, d_c_re, d_c_im)', fit, *sub(ok_fit, i, None))
    refused('d_t_im must start on a 16-byte boundary', fit, *sub(ok_fit, 1, t[1].ptr + 4))
    refused('d_c_re must be aligned for 4-byte words', fit, *sub(ok_fit, 8, c[0].ptr + 2))
    refused('d_info must be aligned for 4-byte words', fit, *sub(ok_fit, 11, info.ptr + 1))
    refused('the output d_c_re overlaps the input d_t_im', fit, *sub(ok_fit, 8, t[1].ptr))
    refused('the outputs d_c_re and d_c_im overlap', fit, *sub(ok_fit, 9, c[0].ptr))
    for i in (5, 6):
        refused('null required pointer (d_c_re, d_c_im)', app, *sub(ok_app, i, None))
    refused('d_c_im must be aligned for 4-byte words', app, *sub(ok_app, 6, c[1].ptr + 2))
    for fn, ok, i in ((app, ok_app, 7), (seq, ok_seq, 8)):
        refused('null required pointer (d_out_re, d_out_im)', fn, *sub(ok, i, None))
        refused('d_out_im must start on a 16-byte boundary', fn, *sub(ok, i + 1, ok[i + 1] + 4))
        refused('the output d_out_re overlaps the input d_x_re[3]', fn, *sub(ok, i, x[0][3].ptr))             # in place is refused too
        refused('the output d_out_im overlaps the input d_x_re[0]', fn, *sub(ok, i + 1, x[0][0].ptr + nr * nt * N * 4))
        refused('the outputs d_out_re and d_out_im overlap', fn, *sub(ok, i + 1, ok[i]))
    refused('the output d_out_re overlaps the input d_c_re', app, *sub(ok_app, 5, y[0].ptr + 64))
    refused('the c planes come as a pair', seq, *sub(ok_seq, 10, None))
    refused('d_fit_err must be aligned for 4-byte words', seq, *sub(ok_seq, 12, fe.ptr + 2))
    refused('the outputs d_c_re and d_fit_err overlap', seq, *sub(ok_seq, 12, c[0].ptr))
    refused('must not be negative', noise, *sub(ok_noise, 2, -1))
    refused('must not be negative', noise, *sub(ok_noise, 1, -1))
    for i in (3, 4, 5, 6, 7):
        refused('null required pointer (d_err_var, d_x_re, d_x_im, d_out_re, d_out_im)', noise, *sub(ok_noise, i, None))
    for i, name in ((4, 'd_x_re'), (5, 'd_x_im'), (6, 'd_out_re'), (7, 'd_out_im')):
        refused(name + ' must start on a 16-byte boundary', noise, *sub(ok_noise, i, ok_noise[i] + 8))
    refused('d_err_var must be aligned for 4-byte words', noise, *sub(ok_noise, 3, v.ptr + 2))
    refused('any other overlap of the planes is refused', noise, *sub(ok_noise, 6, x[0][0].ptr + 16))
    refused('any other overlap of the planes is refused', noise, *sub(ok_noise, 6, x[1][0].ptr))
    refused('the output d_out_im overlaps the input d_err_var', noise, 7, 0, npkt, y[1].ptr + 32, x[0][0].ptr, x[1][0].ptr, y[0].ptr, y[1].ptr)
    blocks = lib.csi_forecast_gram_blocks_device
    refused('blocks outside 0 .. 2^31 - 1', blocks, xr, xi, P, -1, 2 * N, t[0].ptr, t[1].ptr)
    refused('block_floats 3 must be even', blocks, xr, xi, P, 2, 3, t[0].ptr, t[1].ptr)
    refused('block_floats 0 must be even and at least 2', blocks, xr, xi, P, 2, 0, t[0].ptr, t[1].ptr)
    hp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))      # noqa: E731
    host = np.zeros(npkt * nr * nt * N, np.float32)
    hx = (ctypes.c_void_p * P)(*[host.ctypes.data] * P)
    refused('n_snd 1 outside 2 .. 16', lib.csi_forecast, hx, hx, 1, npkt, M, 1, 1e-5, 0, hp(host), hp(host), None, None, None, None)
    refused('order 2 + steps 3 exceed n_snd 4', lib.csi_forecast, hx, hx, P, npkt, M, 3, 1e-5, 0, hp(host), hp(host), None, None, None, None)
    refused('null required pointer (x_re, x_im, out_re, out_im)', lib.csi_forecast, hx, hx, P, npkt, M, 1, 1e-5, 0, None, hp(host), None, None, None, None)
    refused('null required pointer (x_re[2] / x_im[2])', lib.csi_forecast, (ctypes.c_void_p * P)(host.ctypes.data, host.ctypes.data, None, host.ctypes.data), hx,
            P, npkt, M, 1, 1e-5, 0, hp(host), hp(host), None, None, None, None)
    big = np.zeros((P + 2) * npkt * nr * nt * N, np.float32)
    at = lambda i: big[i * host.size:].ctypes.data      # noqa: E731
    hx_re, hx_im = (ctypes.c_void_p * P)(*[at(i) for i in range(P)]), (ctypes.c_void_p * P)(*[at(0)] * P)
    refused('the output out_re overlaps the input x_re[1]', lib.csi_forecast, hx_re, hx_im, P, npkt, M, 1, 1e-5, 0, hp(big[host.size + 4:]), hp(big[P * host.size:]),
            None, None, None, None)
    refused('the outputs out_re and out_im overlap', lib.csi_forecast, hx_re, hx_im, P, npkt, M, 1, 1e-5, 0, hp(big[P * host.size:]), hp(big[P * host.size:]),
            None, None, None, None)
    refused('the outputs c_re and c_im overlap', lib.csi_forecast, hx_re, hx_im, P, npkt, M, 1, 1e-5, 0, hp(big[P * host.size:]), hp(big[(P + 1) * host.size:]),
            hp(host), hp(host), None, None)
    # npkt = 0 is no error and no launch, whatever the pointers
    assert gram(ctx, None, None, P, 0, None, None) == 0 and fit(ctx, None, None, P, 0, M, 1, 1e-5, 0, None, None, None, None) == 0
    assert app(ctx, None, None, P, 0, M, None, None, None, None) == 0 and seq(ctx, None, None, P, 0, M, 1, 1e-5, 0, None, None, None, None, None, None) == 0
    assert noise(ctx, 7, 0, 0, None, None, None, None, None) == 0 and blocks(ctx, None, None, P, 0, 2, None, None) == 0
    assert lib.csi_forecast(ctx, None, None, P, 0, M, 1, 1e-5, 0, hp(host), hp(host), None, None, None, None) == 0
    assert e.get_option('forecast_launches') == 0
    # an open capture: the sequence needs an eager call of its shape in front
    e.capture_begin()
    try:
        assert gram(ctx, *ok_gram) == 0                     # recorded, counted, not run
        launches = 1
        refused('sized by an eager call', seq, *ok_seq)
    finally:
        e.capture_end()
    # the launches of every entry
    for fn, ok, n in ((gram, ok_gram, 2), (fit, ok_fit, 3), (app, ok_app, 4), (seq, ok_seq, 7), (noise, ok_noise, 8)):
        assert fn(ctx, *ok) == 0, lib.csi_last_error(ctx)
        assert e.get_option('forecast_launches') == n
    e.synchronize()
    v0 = e.view(y[0], 1)
    assert v0.shape == (nr, nt, N) and v0.ptr == y[0].ptr + nr * nt * N * 4
    with pytest.raises(IndexError):
        e.view(y[0], npkt + 1)
    with pytest.raises(pkg.CsiError, match='x must be'):
        e.forecast(np.zeros((P, 1, nr, nt, 7), np.complex64), M, 1)
    one = pkg.CsiEngine(0, 1, hidden=(16,), len_ltf=64)
    for fn, ok in ((gram, ok_gram), (fit, ok_fit), (app, ok_app), (seq, ok_seq), (noise, ok_noise)):
        assert fn(one._ctx, *ok) == -1 and 'single-input context' in lib.csi_last_error(one._ctx).decode()


def test_h_miniature_sweep_with_the_forecast(pkg, oracle, tmp_path):
    """Nt = 8, Nr = 2, one level, two users, sweep --forecast 12 4: the new fields are there and finite, MSEF_perfect is the NMSE of the
    forecast this file tests (CsiEngine.forecast on the downloaded history) against the aged truth, and it beats MSEA_perfect"""
    from scipy.io import loadmat
    from dl_channel_estimation_mamimo_amd import sweep
    nt, nr, n_train, n_test, P, M, D, ms = 8, 2, 24, 6, 12, 4, 4, 2.0
    out = str(tmp_path / 'sweep')
    assert sweep.main(['-d', out, '--nTX', str(nt), '--nRX', str(nr), '--nn', '16', '--trainPkts', str(n_train), '--testPkts', str(n_test), '--snr', '20',
                       '--quiet', '--epochs', '2', '--bs', '32', '--channel', 'scattering', '--ber', '--numSTS', '1', '--users', '2', '--rays', '64',
                       '--dataSymbols', '2', '--aging', str(ms), '--speed', '1', '--forecast', str(P), str(M)]) == 0
    m = loadmat(os.path.join(out, 'BS8_SNR20', 'metrics.mat'))
    new = [k for k in m if any(k.startswith(f) for f in sweep.MSEF_FIELDS + sweep.MUF_FIELDS)]
    assert sorted(new) == sorted(f + x for x in ('LS', 'perfect') for f in sweep.MSEF_FIELDS + sweep.MUF_FIELDS)
    assert [k for k in m if not k.startswith('__')][-8:] == ['MSEF_LS', 'MSEF_perfect'] + [f + x for x in ('LS', 'perfect') for f in sweep.MUF_FIELDS]
    for k in new:
        assert m[k].shape == (1, n_test) and np.isfinite(m[k]).all(), k
    e = _engine(pkg, nt, nr)
    times = [-1e-3 * (P - 1 - i) * ms / D for i in range(P - 1)] + [0.0, 1e-3 * ms]
    h = _dl(*e.scatter_channel_at(1, n_train, n_test, times, speed_mps=1.0))
    y = e.forecast(h[:P], M, D)
    want = np.array([oracle.nmse_subk(h[-1][p], y[p]) for p in range(n_test)])
    err = np.abs(m['MSEF_perfect'][0] / want - 1.0).max()
    print(f'miniature sweep at 20 dB, 2 ms, 1 m/s, (12, 4, 4): MSEA_perfect {m["MSEA_perfect"][0].mean():.4e} -> MSEF_perfect {m["MSEF_perfect"][0].mean():.4e} '
          f'(against CsiEngine.forecast on the downloaded history: relative difference {err:.2e}), MSEA_LS {m["MSEA_LS"][0].mean():.4e} -> MSEF_LS '
          f'{m["MSEF_LS"][0].mean():.4e}; sinrMUA_perfect {m["sinrMUA_perfect"][0].mean():.2f} -> sinrMUF_perfect {m["sinrMUF_perfect"][0].mean():.2f} dB')
    assert err < 1e-6                                     # tests/test_gpu_eval_kernels.py, the metric
    assert m['MSEF_perfect'][0].mean() < 0.1 * m['MSEA_perfect'][0].mean()
