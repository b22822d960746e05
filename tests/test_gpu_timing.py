"""GPU tests of the symbol-timing stage (csi_sync_embed_device, csi_sync_estimate_device, csi_sync_extract_device,
csi_sync_correct[_device]; csrc/sync.hip.h) against the fp64 statement tests/timing_ref.py on the downloaded float32
captures.

Tolerances, each fixed before the first device run (measured ratios: profiles/timing.txt):
  metric    |Lambda_dev - Lambda_ref| <= 8 2^-24 Phi_ref(theta) for every theta: each product carries two roundings relative to
            |a| |b| <= (|a|^2 + |b|^2) / 2, that is 2 sqrt 2 for |gamma| plus 2 rho for Phi, below 4.83; 8 is granted.  The fp64 sums
            add nothing.
  theta_hat exactly the lowest argmax of the device's own d_metric; equal to the reference's argmax for every packet whose reference
            runner-up gap exceeds 100 x 8 2^-24 max_theta Phi_ref.  No packet may fall under that exemption noise-free and at 20 dB;
            the 0 dB case may exempt 2 of its 16 packets.
  eps_hat / quality   the CFO test's bounds, 8 2^-24 / (2 pi quality_ref) and 8 2^-24, where theta_hat agrees.  The zero packet
            returns exactly (0, 0, 0).
  margins   the draw z = margin / std against the host replay: the bound derived for tr_normal in tests/test_train_streams.py
            (16 ulp-units of the Box-Muller radius) plus one fp32 spacing of the product std z.
  through LS: the corrected capture gets 4 times the rel_rows figure of the un-embedded packets on the same engine (the allowance of
            the CFO test); the cut at span / 2 must stand above 1000 times it.
Everything else is compared bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfo_ref as cr         # noqa: E402
import guarded as G          # noqa: E402
import timing_ref as tr      # noqa: E402
from conftest import rel_rows      # noqa: E402
from test_train_streams import _noise_bound      # noqa: E402  (the bound derived there for the same tr_normal draw)

U = 2.0 ** -24
LAM_BOUND = 8.0 * U                        # times Phi_ref(theta)
GAP_UNITS = 100.0 * 8.0 * U                # times max_theta Phi_ref
EPS_BOUND = 8.0 * U / (2.0 * np.pi)        # over quality_ref
Q_BOUND = 8.0 * U
SHAPES = [(4, 1, 5, 4), (4, 2, 4, 64), (8, 2, 3, 128), (4, 1, 3, 256), (128, 1, 2, 64)]
SEED = 21
_cache = {}


def _engine(pkg, nt, nr, **kw):
    return pkg.CsiEngine(nt, nr, hidden=(8,), **kw)


def _thetas(npkt, span, roll=0):
    """0 and span first, then starts of the residues 1, 2, 3 mod 4 (in an order that differs between the shapes), span - 1, ..."""
    low = [[3, 2, 1], [2, 1, 3], [1, 3, 2]][roll % 3]
    return np.array(([0, span] + low + [span - 1, span // 2 + 1])[:npkt], np.int32)


def _case(oracle, nt, nr, npkt, span, snr_db, zero_last=True, seed=None):
    """float32 planes of oracle packets under offsets |eps| <= 0.45, their starts, the deviation of their margins; the last packet
    all zero (margins included) when zero_last; computed once per case"""
    key = (nt, nr, npkt, span, snr_db, zero_last, seed)
    if key not in _cache:
        rng = np.random.default_rng(1000 * nt + 10 * nr + span if seed is None else seed)
        ltf, _ = oracle.make_structured_packets(rng, npkt, nr, oracle.hadamard(nt), snr_db=snr_db)
        eps = np.concatenate([[0.45, -0.45], rng.uniform(-0.45, 0.45, npkt)])[:npkt]
        x = cr.rotate(ltf, eps)
        roll = nt // 4 + nr
        theta = _thetas(npkt, span, roll) if npkt <= 7 else np.concatenate([_thetas(7, span, roll), rng.integers(0, span + 1, npkt - 7).astype(np.int32)])
        std = np.zeros(npkt, np.float32)
        if snr_db is not None:
            snr = 10.0 ** (snr_db / 10.0)
            std[:] = np.sqrt(0.5 * np.mean(np.abs(ltf) ** 2) / (1.0 + snr))
        if zero_last:
            x[-1] = 0.0
            std[-1] = 0.0
        _cache[key] = (np.ascontiguousarray(x.real, np.float32), np.ascontiguousarray(x.imag, np.float32), theta, std, eps)
    return _cache[key]


def _i32_up(e, a):
    return e.to_device(np.ascontiguousarray(a, np.int32).view(np.float32))


def _f64_up(e, a):
    return e.to_device(np.ascontiguousarray(a, np.float64).view(np.float32).reshape(-1, 2))


def _i32(d):
    return d.download().view(np.int32).copy()


def _f64(d):
    """a DeviceArray [..., 2] of float32 words as float64 [...]"""
    return d.download().view(np.float64)[..., 0].copy()


def _bits(d):
    return d.download().view(np.uint32)


def _embed(e, re, im, theta, std, span, first_pkt=0):
    """device capture planes of the case"""
    npkt, nr, ln = re.shape
    d = dict(x_re=e.to_device(re), x_im=e.to_device(im), theta=_i32_up(e, theta), std=e.to_device(std),
             c_re=e.empty((npkt, nr, ln + span)), c_im=e.empty((npkt, nr, ln + span)))
    e.sync_embed_device(SEED, first_pkt, npkt, span, d['theta'], d['x_re'], d['x_im'], d['c_re'], d['c_im'], d_margin_std=d['std'])
    e.synchronize()
    return d


def _estimate(e, c_re, c_im, npkt, span, rho=1.0):
    d_th, d_eps, d_q, d_m = e.empty((npkt,)), e.empty((npkt, 2)), e.empty((npkt,)), e.empty((npkt, span + 1, 2))
    e.sync_estimate_device(c_re, c_im, npkt, span, d_th, rho=rho, d_eps=d_eps, d_quality=d_q, d_metric=d_m)
    e.synchronize()
    return _i32(d_th), _f64(d_eps), d_q.download(), _f64(d_m)


@pytest.mark.parametrize('snr_db', [None, 20.0], ids=['noise-free', '20dB'])
@pytest.mark.parametrize('nt,nr,npkt,span', SHAPES)
def test_a_embed_and_cut_out_return_the_bits(pkg, oracle, nt, nr, npkt, span, snr_db):
    re, im, theta, std, _ = _case(oracle, nt, nr, npkt, span, snr_db, zero_last=False)
    e = _engine(pkg, nt, nr)
    d = _embed(e, re, im, theta, std, span, first_pkt=3)
    c_re, c_im = d['c_re'].download(), d['c_im'].download()
    cap = c_re.astype(np.float64) + 1j * c_im.astype(np.float64)
    L = 320 * nt + span
    worst = 0.0
    for p in range(npkt):
        inside = np.zeros(L, bool)
        inside[theta[p]:theta[p] + 320 * nt] = True
        assert np.array_equal(c_re[p][:, inside].view(np.uint32), re[p].view(np.uint32))
        assert np.array_equal(c_im[p][:, inside].view(np.uint32), im[p].view(np.uint32))
        m = cap[p][:, ~inside]
        if std[p] == 0.0:
            assert not m.any()
            continue
        z, rad = tr.margin_normals(SEED, 3 + p, nr, L)
        for part in (lambda v: v.real, lambda v: v.imag):
            got = part(m)
            bound = _noise_bound(part(rad[:, ~inside])) + np.spacing(np.abs(got).astype(np.float32)).astype(np.float64) / std[p]
            worst = max(worst, float((np.abs(got / std[p] - part(z[:, ~inside])) / bound).max()))
    print(f'Nt {nt} Nr {nr} npkt {npkt} span {span}: margin |z_dev - z_ref| / bound <= {worst:.3f}')
    assert worst <= 1.0
    o_re, o_im = e.empty(re.shape), e.empty(re.shape)
    e.sync_extract_device(d['c_re'], d['c_im'], npkt, span, d['theta'], o_re, o_im)
    e.synchronize()
    assert np.array_equal(_bits(o_re), re.view(np.uint32)) and np.array_equal(_bits(o_im), im.view(np.uint32))


def _check_estimate(e, d, npkt, span, rho, theta, live, max_exempt, tag):
    th, eps, quality, lam = _estimate(e, d['c_re'], d['c_im'], npkt, span, rho)
    cap = d['c_re'].download().astype(np.float64) + 1j * d['c_im'].download().astype(np.float64)
    th_ref, eps_ref, q_ref, lam_ref, phi_ref = tr.estimate(cap, span, rho)
    ratio = np.abs(lam - lam_ref)[live] / (LAM_BOUND * phi_ref[live])
    gap = tr.runner_up_gap(lam_ref)[live] / (GAP_UNITS * phi_ref[live].max(axis=1))
    sure = gap > 1.0
    agree = th[live] == th_ref[live]
    print(f'{tag} rho {rho}: |Lambda_dev - Lambda_ref| / bound <= {ratio.max():.3f}, smallest runner-up gap {gap.min():.1f} units, '
          f'{int((~sure).sum())} packets exempt, theta_hat agrees for {int(agree.sum())} of {agree.size}, equals the embedded start for '
          f'{int((th[live] == theta[live]).sum())}')
    assert ratio.max() <= 1.0
    assert np.array_equal(th, np.argmax(lam, axis=1))                  # the lowest argmax of the values the device compared
    assert (~sure).sum() <= max_exempt
    assert agree[sure].all()
    ok = np.flatnonzero(agree)
    e_err = np.abs(cr.wrap(eps[live][ok] - eps_ref[live][ok])) / (EPS_BOUND / q_ref[live][ok])
    q_err = np.abs(quality[live][ok] - q_ref[live][ok]) / Q_BOUND
    print(f'{tag} rho {rho}: eps_hat error / bound {e_err.max():.3f}, quality error / bound {q_err.max():.3f} '
          f'(quality {q_ref[live].min():.3f} .. {q_ref[live].max():.3f})')
    assert e_err.max() <= 1.0 and q_err.max() <= 1.0
    return th, eps, quality


@pytest.mark.parametrize('snr_db', [None, 20.0], ids=['noise-free', '20dB'])
@pytest.mark.parametrize('nt,nr,npkt,span', SHAPES)
def test_b_estimate_against_the_fp64_statement(pkg, oracle, nt, nr, npkt, span, snr_db):
    re, im, theta, std, eps_true = _case(oracle, nt, nr, npkt, span, snr_db)
    e = _engine(pkg, nt, nr)
    d = _embed(e, re, im, theta, std, span)
    live = slice(0, npkt - 1)
    for rho in (1.0, 0.5):
        th, eps, quality = _check_estimate(e, d, npkt, span, rho, theta, live, 0, f'Nt {nt} Nr {nr} npkt {npkt} span {span} '
                                           f'{"noise-free" if snr_db is None else "%g dB" % snr_db}')
        assert np.array_equal(th[live], theta[live])                    # every start came back
        if snr_db is None:
            assert np.abs(cr.wrap(eps[live] - eps_true[live])).max() < 1e-6
        assert th[-1] == 0 and eps[-1] == 0.0 and not np.signbit(eps[-1]) and quality[-1] == 0.0      # the all-zero capture


def test_c_estimate_at_0_db(pkg, oracle):
    """(4, 2, 16 packets, span 64) at 0 dB; the seed was chosen on the CPU so that the reference alone (host replay of the margins)
    leaves at most 2 packets under the exemption: seeds 7 .. 11 left 0, 0, 0, 1, 0; seed 8 has the widest smallest gap, 7.2 units"""
    nt, nr, npkt, span = 4, 2, 16, 64
    re, im, theta, std, _ = _case(oracle, nt, nr, npkt, span, 0.0, zero_last=False, seed=8)
    e = _engine(pkg, nt, nr)
    d = _embed(e, re, im, theta, std, span)
    _check_estimate(e, d, npkt, span, 1.0, theta, slice(0, npkt), 2, 'Nt 4 Nr 2 npkt 16 span 64 0 dB')


@pytest.mark.parametrize('nt,nr,npkt,span', [(8, 2, 3, 128), (128, 1, 2, 64)])
def test_d_same_bits_whatever_the_route(pkg, oracle, nt, nr, npkt, span):
    re, im, theta, std, _ = _case(oracle, nt, nr, npkt, span, 20.0, zero_last=False)
    e = _engine(pkg, nt, nr)
    d = _embed(e, re, im, theta, std, span)
    c_re, c_im = d['c_re'], d['c_im']
    n0 = e.get_option('sync_launches')
    # extract with eps == extract, then cfo_rotate_device(-1); an eps of 0 copies
    eps = np.array([0.3, 0.0, -0.45][:npkt])
    d_eps = _f64_up(e, eps)
    a_re, a_im, b_re, b_im = (e.empty(re.shape) for _ in range(4))
    e.sync_extract_device(c_re, c_im, npkt, span, d['theta'], a_re, a_im, d_eps=d_eps)
    e.sync_extract_device(c_re, c_im, npkt, span, d['theta'], b_re, b_im)
    assert e.get_option('sync_launches') == n0 + 2
    e.cfo_rotate_device(b_re, b_im, npkt, d_eps, -1.0)
    e.synchronize()
    assert np.array_equal(_bits(a_re), _bits(b_re)) and np.array_equal(_bits(a_im), _bits(b_im))
    assert np.array_equal(_bits(a_re)[1], re[1].view(np.uint32)) and np.array_equal(_bits(a_im)[1], im[1].view(np.uint32))
    assert not np.array_equal(_bits(a_re)[0], re[0].view(np.uint32))
    # correct == estimate + extract, with and without the offset removed, with and without the caller's arrays
    for remove in (True, False):
        t1, e1, q1, o_re, o_im = e.empty((npkt,)), e.empty((npkt, 2)), e.empty((npkt,)), e.empty(re.shape), e.empty(re.shape)
        n0 = e.get_option('sync_launches')
        e.sync_estimate_device(c_re, c_im, npkt, span, t1, rho=0.75, d_eps=e1, d_quality=q1)
        e.sync_extract_device(c_re, c_im, npkt, span, t1, o_re, o_im, d_eps=e1 if remove else None)
        t2, e2, q2, p_re, p_im = e.empty((npkt,)), e.empty((npkt, 2)), e.empty((npkt,)), e.empty(re.shape), e.empty(re.shape)
        e.sync_correct_device(c_re, c_im, npkt, span, p_re, p_im, rho=0.75, remove_cfo=remove, d_theta=t2, d_eps=e2, d_quality=q2)
        k_re, k_im = e.empty(re.shape), e.empty(re.shape)
        e.sync_correct_device(c_re, c_im, npkt, span, k_re, k_im, rho=0.75, remove_cfo=remove)      # theta and eps kept by the engine
        assert e.get_option('sync_launches') == n0 + 6
        e.synchronize()
        assert np.array_equal(_i32(t1), theta)
        for x, y in ((t2, t1), (e2, e1), (q2, q1), (p_re, o_re), (p_im, o_im), (k_re, o_re), (k_im, o_im)):
            assert np.array_equal(_bits(x), _bits(y))
        if not remove:
            assert np.array_equal(_bits(o_re), re.view(np.uint32)) and np.array_equal(_bits(o_im), im.view(np.uint32))
        # a captured replay and a repeated call
        r_re, r_im = e.empty(re.shape), e.empty(re.shape)
        e.capture_begin()
        try:
            e.sync_correct_device(c_re, c_im, npkt, span, r_re, r_im, rho=0.75, remove_cfo=remove)
        finally:
            graph = e.capture_end()
        for _ in range(2):
            graph.launch()
            e.synchronize()
            assert np.array_equal(_bits(r_re), _bits(o_re)) and np.array_equal(_bits(r_im), _bits(o_im))
        graph.free()
        # the host twin, whole and in chunks of one packet
        cap = c_re.download() + 1j * c_im.download()
        out, h_th, h_eps, h_q = e.sync_correct(cap, span, rho=0.75, remove_cfo=remove, details=True)
        small = _engine(pkg, nt, nr, workspace_bytes=2 * nr * (640 * nt + span) * 4)
        out1, th1, eps1, q1h = small.sync_correct(cap, span, rho=0.75, remove_cfo=remove, details=True)
        for o, t, ee, q in ((out, h_th, h_eps, h_q), (out1, th1, eps1, q1h)):
            assert np.array_equal(o.real.view(np.uint32), _bits(o_re)) and np.array_equal(o.imag.view(np.uint32), _bits(o_im))
            assert np.array_equal(t, _i32(t1)) and np.array_equal(ee.view(np.uint64), _f64(e1).view(np.uint64))
            assert np.array_equal(q.view(np.uint32), _bits(q1))
    # a packet's results do not depend on the call: a sub-range gives the same bits
    s_th, s_eps, s_q, s_lam = _estimate(e, e.view(c_re, 1), e.view(c_im, 1), 1, span)
    w_th, w_eps, w_q, w_lam = _estimate(e, c_re, c_im, npkt, span)
    assert s_th[0] == w_th[1] and s_eps.view(np.uint64)[0] == w_eps.view(np.uint64)[1] and s_q.view(np.uint32)[0] == w_q.view(np.uint32)[1]
    assert np.array_equal(s_lam[0].view(np.uint64), w_lam[1].view(np.uint64))


def test_e_through_the_ls_estimate(pkg, oracle):
    """synth_structured noise-free at (8, 2, 4, 64) -> embed -> correct -> ls_estimate_device against the generator's h"""
    nt, nr, npkt, span = 8, 2, 4, 64
    e = _engine(pkg, nt, nr)
    e.set_pilot(oracle.hadamard(nt))
    d_re, d_im, h_re, h_im, _ = e.synth_structured(5, 0, npkt, snr_db=None, want_noise_std=False)
    theta = np.array([0, 64, 33, 7], np.int32)
    d_theta = _i32_up(e, theta)
    shape = (npkt, nr, 320 * nt)
    c_re, c_im = e.empty((npkt, nr, 320 * nt + span)), e.empty((npkt, nr, 320 * nt + span))
    e.sync_embed_device(5, 0, npkt, span, d_theta, d_re, d_im, c_re, c_im)
    f_re, f_im, k_re, k_im, t_hat = e.empty(shape), e.empty(shape), e.empty(shape), e.empty(shape), e.empty((npkt,))
    e.sync_extract_device(c_re, c_im, npkt, span, _i32_up(e, np.full(npkt, span // 2)), f_re, f_im)
    e.sync_correct_device(c_re, c_im, npkt, span, k_re, k_im, d_theta=t_hat)
    l_re, l_im = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
    truth = np.concatenate([h_re.download(), h_im.download()], -1)

    def ls(a_re, a_im):
        e.ls_estimate_device(a_re, a_im, npkt, l_re, l_im)
        e.synchronize()
        return rel_rows(np.concatenate([l_re.download(), l_im.download()], -1), truth)
    clean, fixed, found = ls(d_re, d_im), ls(f_re, f_im), ls(k_re, k_im)
    print(f'LS rows against the generator\'s h: un-embedded {clean:.3e}, cut at span / 2 {fixed:.3e} ({fixed / clean:.3g} x), corrected {found:.3e} '
          f'({found / clean:.3f} x); theta_hat {_i32(t_hat).tolist()}')
    assert np.array_equal(_i32(t_hat), theta)
    assert found <= 4.0 * clean, (found, clean)
    assert fixed > 1000.0 * clean, (fixed, clean)


def test_f_guard_bands_on_every_entry(pkg, oracle):
    nt, nr, npkt, span = 4, 2, 4, 64
    re, im, theta, std, _ = _case(oracle, nt, nr, npkt, span, 20.0)
    e = _engine(pkg, nt, nr)
    wild = np.array([-7, span + 9, 2 ** 31 - 1, -2 ** 31], np.int32)            # out of range: clamped to 0, span, span, 0
    kept = np.array([0, span, span, 0], np.int32)
    cshape = (npkt, nr, 320 * nt + span)
    g_re, g_im = G.Guarded(e, re.shape, 'in', re, 'x_re'), G.Guarded(e, re.shape, 'in', im, 'x_im')
    g_std = G.Guarded(e, (npkt,), 'in', std, 'std')
    caps = {}
    for name, th in (('given', theta), ('wild', wild), ('kept', kept)):
        g_th = G.Guarded(e, (npkt,), 'in', th.view(np.float32), 'theta')
        c_re, c_im = G.Guarded(e, cshape, 'out', name='cap_re'), G.Guarded(e, cshape, 'out', name='cap_im')
        e.sync_embed_device(SEED, 0, npkt, span, g_th, g_re, g_im, c_re, c_im, d_margin_std=g_std)
        e.synchronize()
        for g in (g_re, g_im, g_std, g_th, c_re, c_im):
            g.check()
        assert c_re.count_unwritten() == 0 and c_im.count_unwritten() == 0
        assert g_re.unchanged() and g_im.unchanged() and g_std.unchanged() and g_th.unchanged()
        caps[name] = (c_re.download(), c_im.download())
        for g in (g_th, c_re, c_im):
            g.free()
    assert np.array_equal(caps['wild'][0].view(np.uint32), caps['kept'][0].view(np.uint32))
    assert np.array_equal(caps['wild'][1].view(np.uint32), caps['kept'][1].view(np.uint32))
    plain = _embed(e, re, im, theta, std, span)                      # the guards' values reached nothing
    assert np.array_equal(caps['given'][0].view(np.uint32), _bits(plain['c_re'])) and np.array_equal(caps['given'][1].view(np.uint32), _bits(plain['c_im']))
    # the capture as an input between NaN and 3e38
    i_re, i_im = G.Guarded(e, cshape, 'in', caps['given'][0], 'cap_re'), G.Guarded(e, cshape, 'in', caps['given'][1], 'cap_im')
    o_th, o_eps, o_q = G.Guarded(e, (npkt,), 'out', name='theta'), G.Guarded(e, (npkt, 2), 'out', name='eps'), G.Guarded(e, (npkt,), 'out', name='quality')
    o_m = G.Guarded(e, (npkt, span + 1, 2), 'out', name='metric')
    e.sync_estimate_device(i_re, i_im, npkt, span, o_th, d_eps=o_eps, d_quality=o_q, d_metric=o_m)
    e.synchronize()
    for g in (i_re, i_im, o_th, o_eps, o_q, o_m):
        g.check()
        assert g.fill == 'in' or g.count_unwritten() == 0, g.name
    assert i_re.unchanged() and i_im.unchanged()
    want = _estimate(e, plain['c_re'], plain['c_im'], npkt, span)
    assert np.array_equal(o_th.download().view(np.int32), want[0])
    assert np.array_equal(o_eps.download().view(np.float64)[..., 0].view(np.uint64), want[1].view(np.uint64))
    assert np.array_equal(o_q.download().view(np.uint32), want[2].view(np.uint32))
    assert np.array_equal(o_m.download().view(np.float64)[..., 0].view(np.uint64), want[3].view(np.uint64))
    assert np.array_equal(want[0][:-1], theta[:-1])
    for th, ref_th, with_eps in ((theta, theta, False), (theta, theta, True), (wild, kept, True)):
        g_th = G.Guarded(e, (npkt,), 'in', th.view(np.float32), 'theta')
        y_re, y_im = G.Guarded(e, re.shape, 'out', name='out_re'), G.Guarded(e, re.shape, 'out', name='out_im')
        e.sync_extract_device(i_re, i_im, npkt, span, g_th, y_re, y_im, d_eps=o_eps if with_eps else None)
        e.synchronize()
        for g in (i_re, i_im, g_th, o_eps, y_re, y_im):
            g.check()
        assert y_re.count_unwritten() == 0 and y_im.count_unwritten() == 0 and i_re.unchanged() and i_im.unchanged() and g_th.unchanged()
        w_re, w_im = e.empty(re.shape), e.empty(re.shape)
        e.sync_extract_device(plain['c_re'], plain['c_im'], npkt, span, _i32_up(e, ref_th), w_re, w_im, d_eps=o_eps if with_eps else None)
        e.synchronize()
        assert np.array_equal(y_re.download().view(np.uint32), _bits(w_re)) and np.array_equal(y_im.download().view(np.uint32), _bits(w_im))
        if not with_eps:
            assert np.array_equal(y_re.download().view(np.uint32), re.view(np.uint32))
        for g in (g_th, y_re, y_im):
            g.free()
    k_re, k_im = G.Guarded(e, re.shape, 'out', name='cor_re'), G.Guarded(e, re.shape, 'out', name='cor_im')
    k_th, k_eps, k_q = G.Guarded(e, (npkt,), 'out', name='cor_theta'), G.Guarded(e, (npkt, 2), 'out', name='cor_eps'), G.Guarded(e, (npkt,), 'out', name='cor_q')
    e.sync_correct_device(i_re, i_im, npkt, span, k_re, k_im, d_theta=k_th, d_eps=k_eps, d_quality=k_q)
    e.synchronize()
    for g in (i_re, i_im, k_re, k_im, k_th, k_eps, k_q):
        g.check()
        assert g.fill == 'in' or g.count_unwritten() == 0, g.name
    assert i_re.unchanged() and i_im.unchanged()
    assert np.array_equal(k_th.download().view(np.int32), want[0]) and np.array_equal(k_q.download().view(np.uint32), want[2].view(np.uint32))


def test_g_refusals_carry_text_and_write_nothing(pkg):
    nt, nr, npkt, span = 4, 2, 2, 8
    e = _engine(pkg, nt, nr)
    lib, ctx = e._lib, e._ctx
    xshape, cshape = (npkt + 1, nr, 320 * nt), (npkt + 1, nr, 320 * nt + span)
    x = [G.Guarded(e, xshape, 'out', name='x%d' % i).upload(np.ones(xshape, np.float32)) for i in range(2)]
    cap = [G.Guarded(e, cshape, 'out', name='cap%d' % i).upload(np.ones(cshape, np.float32)) for i in range(2)]
    cout = [G.Guarded(e, cshape, 'out', name='cout%d' % i) for i in range(2)]
    y = [G.Guarded(e, xshape, 'out', name='y%d' % i) for i in range(2)]
    th_in = G.Guarded(e, (npkt + 1,), 'out', name='theta_in').upload(np.zeros(npkt + 1, np.int32).view(np.float32))
    std = G.Guarded(e, (npkt + 1,), 'out', name='std').upload(np.ones(npkt + 1, np.float32))
    eps_in = G.Guarded(e, (npkt + 1, 2), 'out', name='eps_in').upload(np.zeros((npkt + 1, 2), np.float32))
    th, eps, q = G.Guarded(e, (npkt + 1,), 'out', name='theta'), G.Guarded(e, (npkt + 1, 2), 'out', name='eps'), G.Guarded(e, (npkt + 1,), 'out', name='quality')
    met = G.Guarded(e, (npkt + 1, span + 1, 2), 'out', name='metric')
    emb, est, ext, cor = lib.csi_sync_embed_device, lib.csi_sync_estimate_device, lib.csi_sync_extract_device, lib.csi_sync_correct_device
    ok_emb = (1, 0, npkt, span, th_in.ptr, std.ptr, x[0].ptr, x[1].ptr, cout[0].ptr, cout[1].ptr)
    ok_est = (cap[0].ptr, cap[1].ptr, npkt, span, 1.0, th.ptr, eps.ptr, q.ptr, met.ptr)
    ok_ext = (cap[0].ptr, cap[1].ptr, npkt, span, th_in.ptr, eps_in.ptr, y[0].ptr, y[1].ptr)
    ok_cor = (cap[0].ptr, cap[1].ptr, npkt, span, 1.0, 1, y[0].ptr, y[1].ptr, th.ptr, eps.ptr, q.ptr)
    sub = lambda ok, i, val: ok[:i] + (val,) + ok[i + 1:]      # noqa: E731

    def refused(text, fn, *args):
        assert fn(ctx, *args) == -1, (text, args)
        assert text in lib.csi_last_error(ctx).decode(), (text, lib.csi_last_error(ctx))
        assert e.get_option('sync_launches') == 0

    # (entry, valid arguments, index of npkt, indices of the input planes, of the output planes, name of the input planes)
    entries = ((emb, ok_emb, 2, (6, 7), (8, 9), 'd_x'), (est, ok_est, 2, (0, 1), (), 'd_cap'), (ext, ok_ext, 2, (0, 1), (6, 7), 'd_cap'),
               (cor, ok_cor, 2, (0, 1), (6, 7), 'd_cap'))
    for fn, ok, i_n, ins, outs, name in entries:
        refused('npkt 0 must be at least 1', fn, *sub(ok, i_n, 0))
        refused('npkt -3 must be at least 1', fn, *sub(ok, i_n, -3))
        refused('exceed one launch', fn, *sub(ok, i_n, 2 ** 31))
        for bad in (0, 2, 6, 260, 320, -4):
            refused('span %d must be a multiple of 4 in 4 .. 256' % bad, fn, *sub(ok, i_n + 1, bad))
        for i in ins:
            refused('null required pointer (%s_re, %s_im)' % (name, name), fn, *sub(ok, i, None))
            refused('%s_re / %s_im must start on a 16-byte boundary' % (name, name), fn, *sub(ok, i, ok[i] + 8))
        out_name = 'd_cap' if fn is emb else 'd_out'
        for i in outs:
            refused('null required pointer (%s_re, %s_im)' % (out_name, out_name), fn, *sub(ok, i, None))
            refused('%s_re / %s_im must start on a 16-byte boundary' % (out_name, out_name), fn, *sub(ok, i, ok[i] + 4))
        if outs:
            refused('shares a byte with', fn, *sub(ok, outs[0], ok[ins[0]] + 16))          # an output onto an input plane
            refused('shares a byte with', fn, *sub(ok, outs[0], ok[ins[1]]))
            refused('shares a byte with', fn, *sub(ok, outs[1], ok[outs[0]] + 16))         # the outputs onto each other
    for fn, ok in ((est, ok_est), (cor, ok_cor)):
        for bad, shown in ((float('nan'), 'nan'), (float('inf'), 'inf'), (-0.25, '-0.25'), (1.5, '1.5')):
            refused('rho %s must be finite and in [0, 1]' % shown, fn, *sub(ok, 4, bad))
    refused('unknown flag bits 0x2', cor, *sub(ok_cor, 5, 3))
    refused('unknown flag bits 0x80000000', cor, *sub(ok_cor, 5, 0x80000000))
    refused('first_pkt -1 must not be negative', emb, *sub(ok_emb, 1, -1))
    refused('null required pointer (d_theta)', emb, *sub(ok_emb, 4, None))
    refused('null required pointer (d_theta)', est, *sub(ok_est, 5, None))
    refused('null required pointer (d_theta)', ext, *sub(ok_ext, 4, None))
    refused('d_theta must be aligned for 4-byte words', emb, *sub(ok_emb, 4, th_in.ptr + 2))
    refused('d_margin_std must be aligned for 4-byte words', emb, *sub(ok_emb, 5, std.ptr + 1))
    refused('d_theta must be aligned for 4-byte words', est, *sub(ok_est, 5, th.ptr + 2))
    refused('d_eps must be aligned for 8-byte words', est, *sub(ok_est, 6, eps.ptr + 4))
    refused('d_quality must be aligned for 4-byte words', est, *sub(ok_est, 7, q.ptr + 2))
    refused('d_metric must be aligned for 8-byte words', est, *sub(ok_est, 8, met.ptr + 4))
    refused('d_theta must be aligned for 4-byte words', ext, *sub(ok_ext, 4, th_in.ptr + 2))
    refused('d_eps must be aligned for 8-byte words', ext, *sub(ok_ext, 5, eps_in.ptr + 4))
    refused('d_theta must be aligned for 4-byte words', cor, *sub(ok_cor, 8, th.ptr + 2))
    refused('d_eps must be aligned for 8-byte words', cor, *sub(ok_cor, 9, eps.ptr + 4))
    refused('d_quality must be aligned for 4-byte words', cor, *sub(ok_cor, 10, q.ptr + 2))
    refused('d_theta shares a byte with d_cap_im', est, *sub(ok_est, 5, cap[1].ptr + 64))
    refused('d_quality shares a byte with d_eps', est, *sub(ok_est, 7, eps.ptr + 8))
    refused('d_metric shares a byte with d_theta', est, *sub(ok_est, 8, th.ptr))
    refused('d_out_re shares a byte with d_theta', ext, *sub(ok_ext, 4, y[0].ptr + 32))
    refused('d_out_im shares a byte with d_eps', ext, *sub(ok_ext, 5, y[1].ptr))
    refused('d_cap_re shares a byte with d_margin_std', emb, *sub(ok_emb, 5, cout[0].ptr))
    refused('d_eps shares a byte with d_out_re', cor, *sub(ok_cor, 9, y[0].ptr + 8))
    hp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))      # noqa: E731
    h_cap = np.ones(2 * (npkt + 1) * nr * (320 * nt + span), np.float32)
    h_out = np.ones(2 * (npkt + 1) * nr * 320 * nt, np.float32)
    hc, ho = h_cap.size // 2, h_out.size // 2
    kept = h_out.copy()
    twin = lib.csi_sync_correct
    ok_twin = (hp(h_cap), hp(h_cap[hc:]), npkt, span, 1.0, 0, hp(h_out), hp(h_out[ho:]), None, None, None)
    refused('npkt 0 must be at least 1', twin, *sub(ok_twin, 2, 0))
    refused('span 12345 must be a multiple of 4 in 4 .. 256', twin, *sub(ok_twin, 3, 12345))
    refused('rho 2 must be finite and in [0, 1]', twin, *sub(ok_twin, 4, 2.0))
    refused('unknown flag bits 0x4', twin, *sub(ok_twin, 5, 4))
    refused('null required pointer (cap_re, cap_im, out_re, out_im)', twin, *sub(ok_twin, 7, None))
    refused('out_re shares a byte with cap_re', twin, *sub(ok_twin, 6, hp(h_cap[8:])))
    refused('out_im shares a byte with out_re', twin, *sub(ok_twin, 7, hp(h_out[4:])))
    assert np.array_equal(h_out, kept)
    e.synchronize()
    for g in x + cap + cout + y + [th_in, std, eps_in, th, eps, q, met]:            # nothing was written
        g.check()
    assert all(g.count_unwritten() == g.n for g in cout + y + [th, eps, q, met])
    with pytest.raises(pkg.CsiError, match='captures must be'):
        e.sync_correct(np.zeros((1, nr, 320 * nt), np.complex64), span)
    # the launches of every entry
    for fn, ok, n in ((emb, ok_emb, 1), (est, ok_est, 2), (ext, ok_ext, 3), (cor, ok_cor, 5)):
        assert fn(ctx, *ok) == 0, lib.csi_last_error(ctx)
        assert e.get_option('sync_launches') == n
    # an open capture: correct without d_theta / d_eps needs an eager call of its shape in front
    e.capture_begin()
    try:
        assert est(ctx, *ok_est) == 0                       # recorded, counted, not run
        assert cor(ctx, *sub(sub(ok_cor, 8, None), 9, None)) == -1 and 'sized by an eager call' in lib.csi_last_error(ctx).decode()
        assert e.get_option('sync_launches') == 6
    finally:
        e.capture_end()
    e.synchronize()
    one = pkg.CsiEngine(0, 1, hidden=(16,), len_ltf=64)
    for fn, ok in ((emb, ok_emb), (est, ok_est), (ext, ok_ext), (cor, ok_cor)):
        assert fn(one._ctx, *ok) == -1 and 'single-input context' in lib.csi_last_error(one._ctx).decode()
