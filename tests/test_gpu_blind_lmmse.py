"""GPU tests of the blind LMMSE smoother (csi_lmmse_blind[_device], csrc/lmmse.hip.h) against tests/blind_lmmse_ref.py: the two
statistics, the smoothed rows, what the smoother gains over LS, bit-for-bit identity across entry points / call sizes / chunks /
graph replay / aliasing, guard bands around every array, degenerate and refused inputs, and the sweep's --blind switch.
Packets come from engine.synth_structured; the reference is evaluated on the SAME fp32 planes the device call read."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blind_lmmse_ref as br      # noqa: E402
from guarded import Guarded       # noqa: E402

pytestmark = pytest.mark.gpu

N = 234
LEVELS = (-10.0, 10.0, 40.0, None)
# (Nt, Nr, packets): one workgroup; several; two tx chunks, the second with 4 valid right-hand sides (a generic pilot); two full chunks
SHAPES = ((4, 1, 1), (8, 4, 3), (36, 2, 2), (64, 2, 2))
STAT_TOL = 1e-10        # fp64 sums of exact products against fp64 numpy; an fp32 accumulation would sit at 1e-7
ROW_TOL = 1e-6          # the existing smoother's contract up to 40 dB; condition numbers here stay near 1e5 at most


def _pilot(oracle, nt):
    if nt & (nt - 1) == 0:
        return oracle.hadamard(nt)
    q, _ = np.linalg.qr(np.random.default_rng(nt).standard_normal((nt, nt)))      # generic real P with P P^T = Nt I
    return q * np.sqrt(nt)


def _f64(dev):
    """a DeviceArray / Guarded of float32 words that holds doubles -> float64 array"""
    return dev.download().reshape(-1).view(np.float64)


def _cplx(re, im):
    out = np.empty(re.shape, np.complex64)
    out.real, out.imag = re, im
    return out


_CASES = {}


def _case(pkg, oracle, nt, nr, npkt, snr, seed=5):
    """One device run of a shape and level and its reference, computed once and shared: dict with the engine, the device arrays of
    the inputs (ltf_re, ltf_im, ls_re, ls_im), host copies, the device results (out, nv, c) and the reference's (r_out, r_nv, r_c)."""
    key = (nt, nr, npkt, snr, seed)
    if key in _CASES:
        return _CASES[key]
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(_pilot(oracle, nt))
    d_re, d_im, h_re, h_im, _ = e.synth_structured(seed, 0, npkt, snr_db=snr, want_noise_std=False)
    shape = (npkt, nr, nt, N)
    ls_re, ls_im, o_re, o_im = (e.empty(shape) for _ in range(4))
    d_nv, d_c = e.empty((npkt, nr, 2)), e.empty((npkt, nr, N, 4))
    e.ls_estimate_device(d_re, d_im, npkt, ls_re, ls_im)
    e.lmmse_blind_device(d_re, d_im, ls_re, ls_im, npkt, o_re, o_im, d_nv, d_c)
    e.synchronize()
    c = dict(e=e, nt=nt, nr=nr, npkt=npkt, d_re=d_re, d_im=d_im, ls_re=ls_re, ls_im=ls_im,
             ltf=_cplx(d_re.download(), d_im.download()), ls=_cplx(ls_re.download(), ls_im.download()),
             h=_cplx(h_re.download(), h_im.download()), out=_cplx(o_re.download(), o_im.download()),
             nv=_f64(d_nv).reshape(npkt, nr), c=_f64(d_c).reshape(npkt, nr, N, 2))
    c['c'] = c['c'][..., 0] + 1j * c['c'][..., 1]
    c['r_out'], c['r_nv'], c['r_c'] = br.blind_ref(c['ltf'], c['ls'])
    for a in (h_re, h_im, o_re, o_im, d_nv, d_c):
        a.free()
    _CASES[key] = c
    return c


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- (a), (b)
@pytest.mark.parametrize('snr', LEVELS, ids=lambda s: 'noise_free' if s is None else '%gdB' % s)
@pytest.mark.parametrize('nt,nr,npkt', SHAPES, ids=['%dx%dx%d' % s for s in SHAPES])
def test_a_corr_against_the_reference(pkg, oracle, nt, nr, npkt, snr):
    """corr against the fp64 reference on the same fp32 planes: 1e-10 relative to |c[0]|.  An fp64 sum of at most 234 * 128 exact
    products errs by about 3e-12, an fp32 accumulation by about 1e-7.  Measured on the MI355X: 1.7e-15 ... 4.5e-14."""
    k = _case(pkg, oracle, nt, nr, npkt, snr)
    e_c = float(np.max(np.abs(k['c'] - k['r_c']) / np.abs(k['r_c'][..., :1])))
    print('Nt %d Nr %d npkt %d snr %s: corr err / |c[0]| %.3e' % (nt, nr, npkt, snr, e_c))
    assert np.all(k['c'][..., 0].imag == 0.0) and np.all(k['c'][..., 0].real > 0.0)
    assert e_c <= STAT_TOL, e_c


@pytest.mark.parametrize('snr', LEVELS, ids=lambda s: 'noise_free' if s is None else '%gdB' % s)
@pytest.mark.parametrize('nt,nr,npkt', SHAPES, ids=['%dx%dx%d' % s for s in SHAPES])
def test_a_noise_var_against_the_reference(pkg, oracle, nt, nr, npkt, snr):
    """noise_var against the reference on the same fp32 planes: 1e-10 relative, noise-free packets included.

    There the null carriers hold only the fp32 generator's rounding residue (nv = 2e-16 ... 3e-15 against 3e-6 at 40 dB): the 256 terms
    of a Y[s][b] cancel to 1e-8 of their size, and a plain fp64 sum - the kernel's first form and numpy's complex128 alike - is left
    with 1e-8 ... 3e-7 of error.  So the kernel sums in fp64 pairs with 106-bit twiddles and the reference evaluates the sums exactly
    (blind_lmmse_ref.noise_var).  Measured on the MI355X: at most 3.6e-16 at every shape and level (plain fp64 sums: 7.6e-9 ... 4.9e-8
    noise-free)."""
    k = _case(pkg, oracle, nt, nr, npkt, snr)
    e_nv = float(np.max(np.abs(k['nv'] - k['r_nv']) / k['r_nv']))
    print('Nt %d Nr %d npkt %d snr %s: noise_var %.3e .. %.3e rel err %.3e' % (nt, nr, npkt, snr, k['nv'].min(), k['nv'].max(), e_nv))
    assert e_nv <= STAT_TOL, e_nv


@pytest.mark.parametrize('snr', LEVELS, ids=lambda s: 'noise_free' if s is None else '%gdB' % s)
@pytest.mark.parametrize('nt,nr,npkt', SHAPES, ids=['%dx%dx%d' % s for s in SHAPES])
def test_b_output_against_the_reference(pkg, oracle, nt, nr, npkt, snr):
    """The smoothed rows against np.linalg.solve in complex128 on the same planes: row-relative error at most 1e-6.  Measured maximum
    over the grid: 3.0e-08 (profiles/lmmse_blind.txt).  The condition number of T on these inputs is printed, not gated - it is a
    property of the packets: 20 ... 54 at -10 dB, up to 1.06e5 at 40 dB and noise-free (the (8, 4, 3) case)."""
    k = _case(pkg, oracle, nt, nr, npkt, snr)
    err = float(br.rel_rows_c(k['out'], k['r_out']).max())
    cond = max(np.linalg.cond(br.toeplitz(k['r_c'][p, r])) for p in range(npkt) for r in range(nr))
    print('Nt %d Nr %d npkt %d snr %s: row-relative error %.3e, largest condition number %.3g' % (nt, nr, npkt, snr, err, cond))
    assert k['e'].get_option('lmmse_blind_fallbacks') == 0
    assert err <= ROW_TOL, err


def test_b_second_staging_chunk_of_the_host_entry_point(pkg, oracle):
    """(128, 16, 37) through csi_lmmse_blind only: the host entry point stages 35 packets of this shape per chunk, so packets 35 and 36
    are its second chunk.  The reference is evaluated on packets 0, 34, 35 and 36 (both sides of the boundary); the whole result must
    be finite and all four tx chunks of every (packet, rx) written."""
    nt, nr, npkt = 128, 16, 37
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(oracle.hadamard(nt))
    d_re, d_im, _, _, _ = e.synth_structured(11, 0, npkt, snr_db=10.0, want_channel=False, want_noise_std=False)
    ltf_re, ltf_im = d_re.download(), d_im.download()
    d_re.free(); d_im.free()
    ls_re, ls_im = e.ls_estimate(ltf_re, ltf_im, out=(np.empty((npkt, nr, nt, N), np.float32), np.empty((npkt, nr, nt, N), np.float32)))
    ls = _cplx(ls_re, ls_im)
    out, nv, c = e.lmmse_blind(_cplx(ltf_re, ltf_im), ls, details=True)
    assert np.isfinite(out.view(np.float32)).all() and np.isfinite(nv).all() and np.isfinite(c.view(np.float64)).all()
    pk = [0, 34, 35, 36]
    r_out, r_nv, r_c = br.blind_ref(_cplx(ltf_re[pk], ltf_im[pk]), ls[pk], exact=False)      # 10 dB: the plain null-carrier sums do (1e-14 of their own)
    e_nv = float(np.max(np.abs(nv[pk] - r_nv) / r_nv))
    e_c = float(np.max(np.abs(c[pk] - r_c) / np.abs(r_c[..., :1])))
    err = float(br.rel_rows_c(out[pk], r_out).max())
    print('Nt 128 Nr 16, packets %s of 37: noise_var rel err %.3e, corr err / |c[0]| %.3e, row-relative error %.3e' % (pk, e_nv, e_c, err))
    assert e_nv <= STAT_TOL and e_c <= STAT_TOL and err <= ROW_TOL
    # a packet's bits do not depend on the chunk that holds it: the last two packets alone
    tail = e.lmmse_blind(_cplx(ltf_re[35:], ltf_im[35:]), ls[35:])
    assert np.array_equal(_bits(tail), _bits(out[35:]))
    # every other (packet, rx) moved away from LS, i.e. was smoothed
    assert np.all(np.abs(out - ls).reshape(npkt * nr, -1).max(axis=1) > 0)
    assert e.get_option('lmmse_blind_fallbacks') == 0


# ---------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize('snr', [-10.0, 10.0])
def test_c_gain_over_ls(pkg, oracle, snr):
    """(8, 2, 16) from synth_structured, seed 77: NMSE of the smoothed estimate below half the NMSE of LS.  With the fp64 reference alone
    on the host twin of these packets (tests/synth_streams.py, same seed): 14.25 -> 1.470 (ratio 0.103) at -10 dB, 0.1425 -> 0.02244
    (0.158) at 10 dB; at 40 dB the gain is 4 % and nothing is asserted."""
    k = _case(pkg, oracle, 8, 2, 16, snr, seed=77)
    ls, sm = br.nmse(k['ls'], k['h']), br.nmse(k['out'], k['h'])
    print('snr %g: NMSE LS %.4e -> blind LMMSE %.4e (ratio %.3f; reference on the same planes %.4e)' % (snr, ls, sm, sm / ls, br.nmse(k['r_out'], k['h'])))
    assert sm < 0.5 * ls


# ---------------------------------------------------------------------------------------------------------------- (d)
def test_d_bit_for_bit_identity(pkg, oracle):
    """(36, 2, 2) at 10 dB: the host entry point, a second call, each packet alone, `out` aliasing `h`, and a captured graph all return
    the bits of the first device call."""
    k = _case(pkg, oracle, 36, 2, 2, 10.0)
    e, nt, nr, npkt = k['e'], 36, 2, 2
    want = _bits(k['out'])
    # host entry point, statistics included
    out, nv, c = e.lmmse_blind(k['ltf'], k['ls'], details=True)
    assert np.array_equal(_bits(out), want)
    assert np.array_equal(nv.view(np.uint64), k['nv'].view(np.uint64)) and np.array_equal(c.view(np.uint64), k['c'].view(np.uint64))
    # two calls in a row, the second without the optional outputs (statistics in the context's workspace)
    shape = (npkt, nr, nt, N)
    o_re, o_im = e.empty(shape), e.empty(shape)
    for _ in range(2):
        e.lmmse_blind_device(k['d_re'], k['d_im'], k['ls_re'], k['ls_im'], npkt, o_re, o_im)
        e.synchronize()
        assert np.array_equal(_bits(_cplx(o_re.download(), o_im.download())), want)
    # each packet alone
    for p in range(npkt):
        one = e.lmmse_blind(k['ltf'][p:p + 1], k['ls'][p:p + 1])
        assert np.array_equal(_bits(one), want[p:p + 1]), p
    # a captured graph replays the eager bits (the eager calls above sized the workspace)
    o_re.upload(np.zeros(shape, np.float32)); o_im.upload(np.zeros(shape, np.float32))
    e.capture_begin()
    try:
        e.lmmse_blind_device(k['d_re'], k['d_im'], k['ls_re'], k['ls_im'], npkt, o_re, o_im)
    finally:
        g = e.capture_end()
    assert not o_re.download().any(), 'a captured call must not run'
    g.launch()
    e.synchronize()
    assert np.array_equal(_bits(_cplx(o_re.download(), o_im.download())), want)
    # out aliasing h
    a_re, a_im = e.to_device(k['ls'].real), e.to_device(k['ls'].imag)
    e.lmmse_blind_device(k['d_re'], k['d_im'], a_re, a_im, npkt, a_re, a_im)
    e.synchronize()
    assert np.array_equal(_bits(_cplx(a_re.download(), a_im.download())), want)
    assert e.get_option('lmmse_blind_fallbacks') == 0


def test_d_packet_inside_a_larger_call(pkg, oracle):
    """packets 0 ... 2 of the (8, 4, 3) case as part of one call and one by one through the device entry point"""
    k = _case(pkg, oracle, 8, 4, 3, -10.0)
    e = k['e']
    for p in range(3):
        i = [e.to_device(a) for a in (k['ltf'].real[p:p + 1], k['ltf'].imag[p:p + 1], k['ls'].real[p:p + 1], k['ls'].imag[p:p + 1])]
        o = [e.empty((1, 4, 8, N)) for _ in range(2)]
        s = [e.empty((1, 4, 2)), e.empty((1, 4, N, 4))]
        e.lmmse_blind_device(i[0], i[1], i[2], i[3], 1, o[0], o[1], s[0], s[1])
        e.synchronize()
        assert np.array_equal(_bits(_cplx(o[0].download(), o[1].download())), _bits(k['out'][p:p + 1])), p
        assert np.array_equal(_f64(s[0]).view(np.uint64), k['nv'][p].reshape(-1).view(np.uint64))
        for a in i + o + s:
            a.free()


# ---------------------------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize('nt,nr,npkt', [(4, 1, 1), (36, 2, 3)])
def test_e_guard_bands(pkg, oracle, nt, nr, npkt):
    """Guard bands around all four inputs and all four outputs (diagnostics included): no guard word damaged, every payload word written,
    no NaN from an input guard in any result, inputs unchanged, and the bits of the run on plain arrays."""
    k = _case(pkg, oracle, nt, nr, npkt, 10.0)
    e = k['e']
    ins = dict(ltf_re=k['ltf'].real, ltf_im=k['ltf'].imag, h_re=k['ls'].real, h_im=k['ls'].imag)
    g_in = {n: Guarded(e, v.shape, 'in', np.ascontiguousarray(v, np.float32), name=n) for n, v in ins.items()}
    shape = (npkt, nr, nt, N)
    g_out = dict(out_re=Guarded(e, shape, 'out', name='out_re'), out_im=Guarded(e, shape, 'out', name='out_im'),
                 noise_var=Guarded(e, (npkt, nr, 2), 'out', name='noise_var'), corr=Guarded(e, (npkt, nr, N, 4), 'out', name='corr'))
    e.lmmse_blind_device(g_in['ltf_re'], g_in['ltf_im'], g_in['h_re'], g_in['h_im'], npkt, g_out['out_re'], g_out['out_im'],
                         g_out['noise_var'], g_out['corr'])
    e.synchronize()
    for a in list(g_in.values()) + list(g_out.values()):
        a.check()
    for n, a in g_out.items():
        assert a.count_unwritten() == 0, n
        assert np.isfinite(a.download()).all() if n.startswith('out') else np.isfinite(_f64(a)).all(), n
    assert all(a.unchanged() for a in g_in.values())
    assert np.array_equal(_bits(_cplx(g_out['out_re'].download(), g_out['out_im'].download())), _bits(k['out']))
    assert np.array_equal(_f64(g_out['noise_var']).view(np.uint64), k['nv'].reshape(-1).view(np.uint64))
    assert np.array_equal(_f64(g_out['corr']).view(np.uint64), np.ascontiguousarray(k['c']).view(np.float64).reshape(-1).view(np.uint64))
    for a in list(g_in.values()) + list(g_out.values()):
        a.free()


# ---------------------------------------------------------------------------------------------------------------- (f)
def test_f_degenerate_inputs_and_the_fallback(pkg, oracle):
    k = _case(pkg, oracle, 8, 4, 3, 10.0)
    nt, nr, npkt = 8, 4, 3
    e = pkg.CsiEngine(nt, nr, hidden=(8,))          # a context of its own: the counter starts at 0
    e.set_pilot(oracle.hadamard(nt))
    zero_ltf, zero_h = np.zeros((npkt, nr, 320 * nt), np.complex64), np.zeros((npkt, nr, nt, N), np.complex64)
    out, nv, c = e.lmmse_blind(zero_ltf, zero_h, details=True)
    assert not out.view(np.float32).any() and not nv.any() and not c.view(np.float64).any()
    assert e.get_option('lmmse_blind_fallbacks') == 0
    # zero LS rows under a noisy preamble: still zeros out (c[0] == 0), the noise estimate is the preamble's
    out, nv, _ = e.lmmse_blind(k['ltf'], zero_h, details=True)
    assert not out.view(np.float32).any() and np.array_equal(nv.view(np.uint64), k['nv'].view(np.uint64))
    assert e.get_option('lmmse_blind_fallbacks') == 0
    # the constructed input: (packet 1, rx 2) cannot be smoothed and comes back as it went in; every other pair as in the clean call
    bad = br.break_input(k['ls'], 1, 2)
    out = e.lmmse_blind(k['ltf'], bad)
    assert e.get_option('lmmse_blind_fallbacks') == 1
    assert np.array_equal(_bits(out[1, 2]), _bits(bad[1, 2]))
    keep = np.ones((npkt, nr), bool)
    keep[1, 2] = False
    assert np.array_equal(_bits(out[keep]), _bits(k['out'][keep]))
    out = e.lmmse_blind(k['ltf'], bad)
    assert e.get_option('lmmse_blind_fallbacks') == 2          # the counter accumulates over calls


def test_f_refusals_carry_text(pkg, oracle):
    nt, nr = 4, 2
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(oracle.hadamard(nt))
    lib, ctx = e._lib, e._ctx
    ltf, h = e.empty((2, nr, 320 * nt)), e.empty((2, nr, nt, N))
    host = np.zeros(2 * nr * nt * N, np.float32)
    fp = lambda a: a.ctypes.data_as(lib.csi_lmmse_blind.argtypes[1])

    def refused(text, *args):
        assert lib.csi_lmmse_blind_device(ctx, *args) == -1
        assert text in lib.csi_last_error(ctx).decode(), lib.csi_last_error(ctx)

    ok = (ltf.ptr, ltf.ptr, h.ptr, h.ptr, 1, h.ptr, h.ptr, None, None)
    refused('must be positive', *(ok[:4] + (0,) + ok[5:]))
    refused('must be positive', *(ok[:4] + (-3,) + ok[5:]))
    for i in (0, 1, 2, 3, 5, 6):
        refused('null required pointer', *(ok[:i] + (None,) + ok[i + 1:]))
    for i, name in ((0, 'd_ltf_re'), (1, 'd_ltf_im'), (2, 'd_h_re'), (3, 'd_h_im'), (5, 'd_out_re'), (6, 'd_out_im')):
        refused('%s must start on a 16-byte boundary' % name, *(ok[:i] + (ok[i] + 4,) + ok[i + 1:]))
    refused('aligned for doubles', *(ok[:7] + (h.ptr + 4, None)))
    assert lib.csi_lmmse_blind(ctx, fp(host), fp(host), fp(host), fp(host), 0, fp(host), fp(host), None, None) == -1
    assert 'must be positive' in lib.csi_last_error(ctx).decode()
    assert lib.csi_lmmse_blind(ctx, None, fp(host), fp(host), fp(host), 1, fp(host), fp(host), None, None) == -1
    assert 'null required pointer' in lib.csi_last_error(ctx).decode()
    assert e.get_option('lmmse_blind_fallbacks') == 0
    with pytest.raises(pkg.CsiError, match='h_ls must be'):
        e.lmmse_blind(np.zeros((1, nr, 320 * nt), np.complex64), np.zeros((1, nr, nt, 7), np.complex64))
    # h_ls=None runs the LS estimate first
    d_re, d_im, _, _, _ = e.synth_structured(3, 0, 2, snr_db=0.0, want_channel=False, want_noise_std=False)
    x = _cplx(d_re.download(), d_im.download())
    assert np.array_equal(_bits(e.lmmse_blind(x)), _bits(e.lmmse_blind(x, e.ls_estimate(x))))


# ---------------------------------------------------------------------------------------------------------------- (g)
def test_g_sweep_with_the_blind_estimator(pkg, oracle, tmp_path):
    """A miniature sweep (Nt 4, Nr 2, hidden (16, 16), random weights from a model folder, two levels of 6 packets) with and without
    blind=True: the flag adds MSE_MMSEb and leaves MSE_LS, MSE_MMSE and MSE_DNN bit-identical."""
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
    for blind in (False, True):
        e = pkg.CsiEngine(nt, nr, hidden=hidden)
        e.set_pilot(oracle.hadamard(nt))
        out = str(tmp_path / ('blind' if blind else 'plain'))
        res[blind] = sweep.run_sweep(e, out, levels=levels, n_train=8, n_test=6, seed=3, modeldir=models, verbose=False, blind=blind)
        res[blind]['dir'] = out
    for snr in levels:
        a, b = (loadmat(os.path.join(res[f]['dir'], 'BS%d_SNR%g' % (nt, snr), 'metrics.mat')) for f in (False, True))
        assert {k for k in a if not k.startswith('__')} == {'MSE_LS', 'MSE_MMSE', 'MSE_DNN'}
        assert {k for k in b if not k.startswith('__')} == {'MSE_LS', 'MSE_MMSE', 'MSE_DNN', 'MSE_MMSEb'}
        for f in ('MSE_LS', 'MSE_MMSE', 'MSE_DNN'):
            assert np.array_equal(a[f].view(np.uint64), b[f].view(np.uint64)), (snr, f)
        assert b['MSE_MMSEb'].shape == (1, 6) and np.isfinite(b['MSE_MMSEb']).all()
        print('snr %g: LS %.4e, MMSE %.4e, MMSEb %.4e' % (snr, b['MSE_LS'].mean(), b['MSE_MMSE'].mean(), b['MSE_MMSEb'].mean()))
    plain = json.load(open(os.path.join(res[False]['dir'], 'sweep.json')))
    with_b = json.load(open(os.path.join(res[True]['dir'], 'sweep.json')))
    assert 'blind' not in plain and all('MMSEb' not in lv for lv in plain['levels'])
    assert with_b['blind'] is True and all('MMSEb' in lv for lv in with_b['levels'])
