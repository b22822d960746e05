"""GPU tests of the 16x16x32 form of the split-f16 layer-0 kernel ("hs_l0_mfma" = 16, gemm_hs.hip.h hs_cast_mfma16_body): the same
terms as the 32x32x16 form in another order of the fp32 sums.  Both forms run in the same context on the same inputs and are held to the
project's own bounds: 1e-5 norm-relative per row against the fp64 oracle (the contract), 5e-6 between the two forms (what
test_gpu_dnn_f32.py demands of two engines).  'f32_engine' = 1 and 'l0_stream' = 0 force the kernel at test sizes."""
import os
import sys

import numpy as np
import pytest

from conftest import rel_rows

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_dnn_f32 import _weights, _pilot, _engine        # noqa: E402

TOL = 1e-5
FORMS = 5e-6


def _force(e):
    e.set_option('f32_engine', 1)
    e.set_option('l0_stream', 0)
    assert e.get_option('hs_vm_cast') == 2


def _both(e, ltf):
    """(outputs of the 32 form, outputs of the 16 form, launches of the 16 form during the second call)"""
    e.set_option('hs_l0_mfma', 32)
    n0 = e.get_option('hs_l0_mfma16_launches')
    a = e.predict(ltf)
    assert e.get_option('hs_l0_mfma16_launches') == n0, 'the 32 form must not count'
    e.set_option('hs_l0_mfma', 16)
    assert e.get_option('hs_l0_mfma') == 16
    b = e.predict(ltf)
    return a, b, e.get_option('hs_l0_mfma16_launches') - n0


# nt, nr, npkt, hidden
CASES = [
    (8, 2, 70, (64, 48)),            # 140 rows: one ragged row tile; N = 64; K = 2560 in several k ranges
    (4, 3, 100, (80, 48)),           # 300 rows: a full and a ragged row tile; N = 80: a partly filled 16-column tile group; two k ranges
    (32, 2, 150, (320, 64)),         # Nt = 32; N = 320: a full and a ragged column tile; 300 rows
    (32, 4, 9, (1024, 1024)),        # the shipped model at 36 rows: four column tiles, split-K
    (4, 2, 300, (256, 64)),          # 600 rows: three row tiles, the last ragged
    (16, 1, 30, (48,)),              # one hidden layer
]


@pytest.mark.parametrize('nt,nr,npkt,hidden', CASES)
def test_forms_agree_and_meet_the_contract(pkg, oracle, nt, nr, npkt, hidden):
    rng = np.random.default_rng(nt * 131 + npkt)
    w_re, w_im = _weights(oracle, 700 + nt, nt, hidden)
    P = _pilot(rng, nt)
    ltf = oracle.make_structured_packets(rng, npkt, nr, oracle.hadamard(nt), snr_db=3.0)[0]
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P)
    _force(e)
    (a_re, a_im), (b_re, b_im), moved = _both(e, ltf)
    assert moved == 2, 'one layer-0 launch per component model'
    sel = np.unique(np.linspace(0, npkt - 1, min(npkt, 12)).astype(int))
    r_re, r_im = oracle.predict_packets(ltf[sel].astype(np.complex64), P, w_re, w_im, np.float64, pkt_batch=len(sel))
    errs = dict(f16_re=rel_rows(b_re[sel], r_re), f16_im=rel_rows(b_im[sel], r_im), f32_re=rel_rows(a_re[sel], r_re),
                forms_re=rel_rows(b_re, a_re), forms_im=rel_rows(b_im, a_im))
    print('hs_l0_mfma', (nt, nr, npkt, hidden), errs)
    assert errs['f16_re'] < TOL and errs['f16_im'] < TOL and errs['f32_re'] < TOL, errs
    assert errs['forms_re'] < FORMS and errs['forms_im'] < FORMS, errs
    assert np.all(np.isfinite(b_re)) and np.all(np.isfinite(b_im))
    assert not np.array_equal(a_re, b_re), 'the option did not switch forms'
    c_re, c_im = e.predict(ltf)                                   # run-to-run identical
    np.testing.assert_array_equal(c_re, b_re)
    np.testing.assert_array_equal(c_im, b_im)
    assert e.get_option('hs_range_fallbacks') == 0


def test_other_vector_memory_schedules_keep_the_32_form(pkg, oracle):
    """the 16 form replaces the default schedule ('hs_vm_cast' = 2) only: the counter stays where it is under the others"""
    rng = np.random.default_rng(21)
    nt, nr, npkt, hidden = 8, 2, 40, (64, 48)
    w_re, w_im = _weights(oracle, 31, nt, hidden)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, _pilot(rng, nt))
    _force(e)
    ltf = oracle.make_structured_packets(rng, npkt, nr, oracle.hadamard(nt), snr_db=3.0)[0]
    e.set_option('hs_l0_mfma', 16)
    ref = e.predict(ltf)
    n0 = e.get_option('hs_l0_mfma16_launches')
    assert n0 == 2
    e.set_option('hs_l0_mfma', 32)
    base = e.predict(ltf)
    e.set_option('hs_l0_mfma', 16)
    for vm in (0, 1, 3):
        e.set_option('hs_vm_cast', vm)
        o = e.predict(ltf)
        assert e.get_option('hs_l0_mfma16_launches') == n0, vm
        np.testing.assert_array_equal(o[0], base[0])               # those schedules are bit-identical to each other
    e.set_option('hs_vm_cast', 2)
    o = e.predict(ltf)
    assert e.get_option('hs_l0_mfma16_launches') == n0 + 2
    np.testing.assert_array_equal(o[0], ref[0])
    with pytest.raises(pkg.CsiError):
        e.set_option('hs_l0_mfma', 8)


@pytest.mark.parametrize('mode', ['max', 'avg'])
def test_pooled_context(pkg, oracle, mode):
    import test_gpu_input_pool as tp
    nt, nr, npkt, hidden = 8, 2, 60, (64, 32)
    w_re, w_im = tp._weights(oracle, 55, nt, hidden)
    P, ltf = tp._packets(oracle, 56, nt, nr, npkt)
    e = tp._engine(pkg, nt, nr, hidden, w_re, w_im, P, mode)
    _force(e)
    (a_re, a_im), (b_re, b_im), moved = _both(e, ltf)
    assert moved == 2                                              # 160 Nt / 16 sub-tiles: even in every k range
    sel = tp._subset(npkt)
    r_re, r_im = oracle.predict_packets(tp.pool_ltf(ltf[sel], mode), P, w_re, w_im, np.float64, pkt_batch=len(sel))
    errs = rel_rows(b_re[sel], r_re), rel_rows(b_im[sel], r_im), rel_rows(b_re, a_re), rel_rows(b_im, a_im)
    print('hs_l0_mfma pooled', mode, errs)
    assert errs[0] < TOL and errs[1] < TOL and errs[2] < FORMS and errs[3] < FORMS, errs


def test_conv1d_context(pkg, oracle):
    """CONV1D: K0 = 64 len_ltf, a multiple of 64 in every k range - the 16 form takes its layer 0"""
    import test_gpu_conv1d as tc
    nt, nr, npkt, hidden = 4, 2, 37, (64, 32)
    w_re, w_im = tc._weights(oracle, 65, nt, hidden)
    P, ltf = tc._packets(oracle, 66, nt, nr, npkt)
    e = tc._engine(pkg, nt, nr, hidden, w_re, w_im, P)
    _force(e)
    (a_re, a_im), (b_re, b_im), moved = _both(e, ltf)
    assert moved >= 2 and moved % 2 == 0, moved
    sel = tc._subset(npkt)
    r_re, r_im = tc.reference(oracle, ltf[sel], P, w_re, w_im)
    errs = rel_rows(b_re[sel], r_re), rel_rows(b_im[sel], r_im), rel_rows(b_re, a_re), rel_rows(b_im, a_im)
    print('hs_l0_mfma conv1d', errs)
    assert errs[0] < TOL and errs[1] < TOL and errs[2] < FORMS and errs[3] < FORMS, errs


def test_range_guard_is_the_same_for_both_forms(pkg, oracle):
    """Heavy-tailed input: a few preambles far above the sampled magnitude trip the guard; both forms report it and the repeated
    call (fp32 MFMA kernels) hands back the same bits.  Preambles that overflow the hidden activations likewise."""
    rng = np.random.default_rng(3)
    nt, nr, npkt, hidden = 8, 2, 40, (64, 64)
    w_re, w_im = _weights(oracle, 17, nt, hidden)
    P = _pilot(rng, nt)
    base = oracle.make_structured_packets(rng, npkt, nr, oracle.hadamard(nt), snr_db=10.0)[0]
    tails = base * (1.0 + 1.0e6 * (rng.random((npkt, nr, 1)) < 0.05))            # ~5 % of the preambles 1e6 times the rest
    assert np.abs(tails).max() > 1e5 * np.median(np.abs(tails))
    for ltf in (tails, 3.0e4 * base):
        outs, falls = [], []
        for form in (32, 16):
            e = _engine(pkg, nt, nr, hidden, w_re, w_im, P)
            _force(e)
            e.set_option('hs_l0_mfma', form)
            outs.append(e.predict(ltf))
            falls.append(e.get_option('hs_range_fallbacks'))
            assert e.get_option('hs_l0_mfma16_launches') == (2 if form == 16 else 0)
        print('hs_l0_mfma range guard: fallbacks', falls)
        assert falls[0] == falls[1] and falls[0] >= 1, falls
        np.testing.assert_array_equal(outs[0][0], outs[1][0])
        np.testing.assert_array_equal(outs[0][1], outs[1][1])
        r_re, r_im = oracle.predict_packets(ltf.astype(np.complex64), P, w_re, w_im, np.float64, pkt_batch=npkt)
        assert rel_rows(outs[1][0], r_re) < TOL and rel_rows(outs[1][1], r_im) < TOL


def test_graph_replay_runs_the_16_form(pkg, oracle):
    rng = np.random.default_rng(12)
    nt, nr, npkt, hidden = 16, 4, 200, (128, 64)
    w_re, w_im = _weights(oracle, 8, nt, hidden)
    P = _pilot(rng, nt)
    e = _engine(pkg, nt, nr, hidden, w_re, w_im, P)
    _force(e)
    d_re, d_im = e.empty((npkt, nr, e.len_ltf)), e.empty((npkt, nr, e.len_ltf))
    e.synth_white(5, 0, npkt, d_re, d_im)
    o_re, o_im = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
    e.set_option('hs_l0_mfma', 32)
    e.predict_device(d_re, d_im, npkt, o_re, o_im); e.synchronize()
    eager32 = o_re.download()
    e.set_option('hs_l0_mfma', 16)
    n0 = e.get_option('hs_l0_mfma16_launches')
    e.predict_device(d_re, d_im, npkt, o_re, o_im); e.synchronize()
    eager16 = o_re.download()
    assert e.get_option('hs_l0_mfma16_launches') == n0 + 2
    assert not np.array_equal(eager16, eager32) and rel_rows(eager16, eager32) < FORMS
    e.set_option('use_graph', 1)
    r0 = e.get_option('graph_replays')
    for _ in range(4):                                   # eager, eager, capture, replay
        o_re.upload(np.zeros((npkt, nr, nt, 234), np.float32))
        e.predict_device(d_re, d_im, npkt, o_re, o_im); e.synchronize()
        assert np.array_equal(o_re.download(), eager16)
    assert e.get_option('graph_replays') > r0 and e.get_option('hs_l0_mfma') == 16
    assert e.get_option('hs_l0_mfma16_launches') > n0 + 2       # the launches that were captured went through the 16 route
    ltf = d_re.download(0, 4) + 1j * d_im.download(0, 4)
    r_re, _ = oracle.predict_packets(ltf, P, w_re, w_im, np.float64, pkt_batch=4)
    assert rel_rows(eager16[:4], r_re) < TOL


def test_headline_shape(pkg, oracle):
    """Nt = 32, Nr = 4, 4000 packets of the benchmark's mixed-SNR input (500 at each of 8 levels), the shipped model, automatic engine
    choice: both forms against each other over the whole batch, the 16 form against the fp64 oracle on one packet per level."""
    nt, nr, npkt, hidden = 32, 4, 4000, (1024, 1024)
    rng = np.random.default_rng(1234)
    w_re, w_im = pkg.synth.make_weights(rng, nt, hidden), pkg.synth.make_weights(rng, nt, hidden)
    P = pkg.synth.hadamard(nt)
    e = pkg.CsiEngine(nt, nr, hidden=hidden, n_out=234, use_bn=True)
    e.load_weights('real', w_re)
    e.load_weights('imag', w_im)
    e.set_pilot(P)
    d_re, d_im = e.empty((npkt, nr, e.len_ltf)), e.empty((npkt, nr, e.len_ltf))
    for p0, snr, blk in pkg.synth.mixed_snr_batch(2025, nr, P, per_level=npkt // 8):
        d_re.upload(np.ascontiguousarray(blk.real), first=p0)
        d_im.upload(np.ascontiguousarray(blk.imag), first=p0)
    outs = {f: (e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))) for f in (32, 16)}
    n0 = e.get_option('hs_l0_mfma16_launches')
    for f in (32, 16):
        e.set_option('hs_l0_mfma', f)
        e.predict_device(d_re, d_im, npkt, outs[f][0], outs[f][1])
        e.synchronize()
        assert e.get_option('hs_l0_mfma16_launches') - n0 == (2 if f == 16 else 0)
    assert e.get_option('hs_range_fallbacks') == 0
    worst, worst_abs, step = 0.0, 0.0, 250
    for p0 in range(0, npkt, step):
        for k in (0, 1):
            a, b = outs[32][k].download(p0, step), outs[16][k].download(p0, step)
            worst = max(worst, rel_rows(b, a))
            worst_abs = max(worst_abs, float(np.max(np.abs(b.astype(np.float64) - a))))
    sel = [i * (npkt // 8) + 7 * i for i in range(8)]              # one packet per SNR level
    got_re = np.concatenate([outs[16][0].download(p, 1) for p in sel])
    got_im = np.concatenate([outs[16][1].download(p, 1) for p in sel])
    ltf = np.concatenate([d_re.download(p, 1) + 1j * d_im.download(p, 1) for p in sel])
    r_re, r_im = oracle.predict_packets(ltf.astype(np.complex64), P, w_re, w_im, np.float64, pkt_batch=len(sel))
    errs = rel_rows(got_re, r_re), rel_rows(got_im, r_im)
    print('hs_l0_mfma headline: largest norm-relative row difference between the forms %.3e (largest absolute %.3e); '
          '16 form against the fp64 oracle %.3e / %.3e' % (worst, worst_abs, errs[0], errs[1]))
    assert worst < FORMS, worst
    assert errs[0] < TOL and errs[1] < TOL, errs
