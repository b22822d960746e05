"""GPU tests (-m gpu) of what the value tests cannot see: the memory contract of the device-pointer entry points and their
independence from the calls a context served before.

Part A.  Every case runs one call twice on one engine: on plain, exactly-sized DeviceArrays, and on tests/guarded.py arrays - each
array a slice of a larger allocation whose neighbourhood holds NaN and +-3e38 (inputs) or NaN and a finite word (outputs), the output
payloads pre-filled with another NaN.  Asserted: every output plane bit-identical between the two runs (with such guards, the proof that no value outside
the inputs reaches a result), every guard intact, no output element left unwritten, every input bit-unchanged, and the counter or
option that names the kernel route moved as the case intends.  The shapes are the smallest of the suite's case tables at which each
route keeps its ragged edge.

Part B.  estimate_device of 1 / 4 / 21 / 150 packets on ONE long-lived engine - in changing order, under hipGraph replay, behind a
range-guard recovery, behind a call with NaN / Inf preambles, behind option toggles that drop cached state - against the same calls on
fresh engines, bit for bit.

Part C.  The pointer contract of include/csi_mamimo.h: a plane that does not start on a 16-byte boundary is refused on the host, with
text, before anything is launched or counted.  (Nothing is ever launched with such a pointer.)"""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import rel_rows

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import Guarded, GuardDamage, UNWRITTEN      # noqa: E402

N = 234
TOL = 1e-5                 # the fp32 contract against the fp64 oracle (BASELINE.json)
BF16_TOL_FMT = 3e-2        # a bf16 context against the fp64 oracle: the format error of 8-bit-mantissa operands (test_gpu_dnn_bf16.py)
P_VHT4 = np.array([[1, -1, 1, 1], [1, 1, -1, 1], [1, 1, 1, -1], [-1, 1, 1, 1]], np.float64)
ROUTE_COUNTERS = ('small_calls', 'l0_stream_launches', 'band_launches', 'band_split_launches', 'hs_range_fallbacks')


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _planes(ltf):
    ltf = np.asarray(ltf)
    return _f32(ltf.real), _f32(ltf.imag)


def both_ways(e, call, ins, outs, route=None, byte_len=None):
    """call(i, o) enqueues one library call on the dicts of arrays i (inputs) and o (outputs).  Runs it on plain DeviceArrays, then on
    Guarded ones; `route` maps a counter to the change EACH run must produce (an int, or '+' for any advance).  `byte_len` names outputs
    of BYTES whose documented size ends inside the last word of the float array that holds them: the two runs are compared on those
    bytes, and the rest of the word must still hold the pre-fill.  Every violation of the case is collected and reported together.
    Returns the plain outputs (host arrays)."""
    route, byte_len = route or {}, byte_len or {}
    bad = []

    def run(i, o, tag):
        before = {k: e.get_option(k) for k in route}
        call(i, o)
        e.synchronize()
        for k, want in route.items():
            d = e.get_option(k) - before[k]
            if (d <= 0) if want == '+' else (d != want):
                bad.append('%s run: counter %s moved by %d, the case intends %s' % (tag, k, d, want))

    p_in = {k: e.to_device(v) for k, v in ins.items()}
    p_out = {k: e.empty(s) for k, s in outs.items()}
    run(p_in, p_out, 'plain')
    want = {k: a.download() for k, a in p_out.items()}
    g_in = {k: Guarded(e, v.shape, 'in', v, name=k) for k, v in ins.items()}
    g_out = {k: Guarded(e, s, 'out', name=k) for k, s in outs.items()}
    run(g_in, g_out, 'guarded')
    for k, a in g_out.items():
        got = a.download()
        if k in byte_len:
            nb = byte_len[k]
            if not np.array_equal(got.view(np.uint8)[:nb], want[k].view(np.uint8)[:nb]):
                bad.append('output %s: the %d bytes differ between the plain and the guarded run' % (k, nb))
            if not np.array_equal(got.view(np.uint8)[nb:], np.full(got.size, UNWRITTEN, np.uint32).view(np.uint8)[nb:]):
                bad.append('output %s: bytes behind its %d documented ones were written' % (k, nb))
        elif not _same(got, want[k]):
            diff = np.flatnonzero(_bits(got) != _bits(want[k]))
            bad.append('output %s: %d of %d words differ between the plain and the guarded run, first at %d (%r against %r)'
                       % (k, diff.size, got.size, diff[0], got.reshape(-1)[diff[0]], want[k].reshape(-1)[diff[0]]))
        holes = a.count_unwritten()
        if holes:
            bad.append('output %s: %d of %d elements were never written' % (k, holes, a.n))
    for k, a in list(g_out.items()) + list(g_in.items()):
        try:
            a.check()
        except GuardDamage as err:
            bad.append(str(err))
    for k, a in g_in.items():
        if not a.unchanged():
            bad.append('input %s was modified by the call' % k)
    for k, a in p_in.items():
        if not _same(a.download(), ins[k]):
            bad.append('input %s (plain run) was modified by the call' % k)
    for a in list(p_in.values()) + list(p_out.values()) + list(g_in.values()) + list(g_out.values()):
        a.free()
    assert not bad, '\n'.join(bad)
    return want


# ====================================================================================================================== part A: LS
def _ls_pilot(oracle, rng, nt, kind):
    if kind == 'generic':
        return rng.integers(-2, 3, (nt, nt)).astype(np.float64)
    if kind == 'pm1':                                       # +-1 entries, not Hadamard: one bf16 piece
        return rng.choice([-1.0, 1.0], (nt, nt))
    if kind == 'vht':                                       # kron(H4, P_VHT4): Hadamard, not in the Sylvester order
        return np.kron(oracle.hadamard(nt // 4), P_VHT4)
    return oracle.hadamard(nt)


# id, nt, nr, npkt, pilot, options, the ls_mode the call must run (LsMode of csrc/csi_ls.hpp: 1 FFT-first, 2 chunked, 3 despread-first, 4 / 5 Walsh-Hadamard
# register prefetch / LDS-DMA ring, 6 generic P on the ring, 7 generic P with the bf16-split despread)
LS_CASES = [
    ('fft_first_generic_partial_tile', 12, 2, 2, 'generic', {}, 1),
    ('chunked', 40, 2, 3, 'generic', {'ls_kernel': 2}, 2),
    ('ring', 40, 2, 3, 'generic', {'ls_kernel': 6}, 6),
    ('chunked_partial_last_chunk', 72, 1, 2, 'generic', {'ls_kernel': 2}, 2),
    ('ring_partial_last_chunk', 72, 1, 2, 'generic', {'ls_kernel': 6}, 6),
    ('despread_first', 160, 1, 1, 'generic', {'ls_kernel': 3}, 3),
    ('fwht_register_prefetch', 16, 2, 5, 'sylvester', {'ls_kernel': 4}, 4),
    ('fwht_ring', 16, 2, 5, 'sylvester', {'ls_kernel': 5}, 5),
    ('fwht_ring_v2', 16, 2, 5, 'sylvester', {'ls_kernel': 5, 'ls_v2': 1}, 5),
    ('fwht_table_vht_pilot', 16, 4, 40, 'vht', {}, 5),
    ('bf16_split_despread', 16, 2, 5, 'pm1', {'ls_kernel': 7}, 7),
    ('persistent_walk', 32, 3, 300, 'generic', {}, 6),
]


@pytest.mark.parametrize('name,nt,nr,npkt,pilot,opts,mode', LS_CASES, ids=[c[0] for c in LS_CASES])
def test_a_ls_estimate_device(pkg, oracle, name, nt, nr, npkt, pilot, opts, mode):
    rng = np.random.default_rng(1000 + nt + npkt)
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_pilot(_ls_pilot(oracle, rng, nt, pilot))
    assert e.get_option('ls_mode') == mode, 'the case no longer reaches its kernel'
    if pilot == 'vht':
        assert e.get_option('ls_pilot_fast') == 2
    if name == 'persistent_walk':
        assert npkt * nr > 256 * e.get_option('ls_per_cu'), 'more items than resident workgroups'
        re, im = _planes(pkg.synth.white_packets(rng, npkt, nr, nt))
    else:
        re, im = _f32(rng.standard_normal((npkt, nr, 320 * nt))), _f32(rng.standard_normal((npkt, nr, 320 * nt)))
    shape = (npkt, nr, nt, N)
    got = both_ways(e, lambda i, o: e.ls_estimate_device(i['ltf_re'], i['ltf_im'], npkt, o['h_re'], o['h_im']),
                    {'ltf_re': re, 'ltf_im': im}, {'h_re': shape, 'h_im': shape})
    assert e.get_option('ls_mode') == mode
    assert np.isfinite(got['h_re']).all() and np.isfinite(got['h_im']).all()
    e.close()


# ====================================================================================================================== part A: DNN
def _conv_weights(rng):
    """cnn1d_1 (7 taps x 1 x 128 filters, bias) and its BatchNormalization (as tests/test_gpu_conv1d.py builds them)"""
    return {'cnn1d_1.kernel': rng.uniform(-0.5, 0.5, (7, 1, 128)).astype(np.float32),
            'cnn1d_1.bias': (0.05 * rng.standard_normal(128)).astype(np.float32),
            'conv_bn.gamma': rng.uniform(0.5, 1.5, 128).astype(np.float32),
            'conv_bn.beta': (0.1 * rng.standard_normal(128)).astype(np.float32),
            'conv_bn.moving_mean': (0.1 * rng.standard_normal(128)).astype(np.float32),
            'conv_bn.moving_variance': rng.uniform(0.5, 1.5, 128).astype(np.float32)}


def _model(pkg, oracle, seed, nt, nr, hidden, n_out=N, opts=None, **kw):
    """engine with both component models and a pilot matrix (Hadamard where Nt is a power of two, small integers elsewhere)"""
    rng = np.random.default_rng(seed)
    e = pkg.CsiEngine(nt, nr, hidden=hidden, n_out=n_out, **kw)
    ws = []
    for d in ('real', 'imag'):
        w = oracle.make_weights(rng, e.l0_in, list(hidden), n_out)
        if e.model == 'CONV1D':
            w.update(_conv_weights(rng))
        e.load_weights(d, w)
        ws.append(w)
    P = oracle.hadamard(nt) if nt & (nt - 1) == 0 else rng.integers(-2, 3, (nt, nt)).astype(np.float64)
    e.set_pilot(P)
    for k, v in (opts or {}).items():
        e.set_option(k, v)
    return e, ws, P


def _packets(oracle, seed, nt, nr, npkt, snr_db=5.0):
    """complex64 preambles: structured packets where Nt is a power of two, white ones elsewhere (as the suite's case tables do)"""
    rng = np.random.default_rng(seed)
    if nt & (nt - 1) == 0:
        return oracle.make_structured_packets(rng, npkt, nr, oracle.hadamard(nt), snr_db=snr_db)[0].astype(np.complex64)
    return (rng.standard_normal((npkt, nr, 320 * nt)) + 1j * rng.standard_normal((npkt, nr, 320 * nt))).astype(np.complex64)


FP32_MFMA = {'f32_engine': 0, 'small_fused': 0}             # (small_fused 0: the general kernels also where the call is a small one - their split-K form)
NO_SPLIT_ENGINE = {'small_calls': 0, 'hs_launches': 0, 'l0_stream_launches': 0, 'band_launches': 0}
SEPARATE = {'f32_engine': 1, 'hs_band': 0}
SEPARATE_ROUTE = {'small_calls': 0, 'hs_launches': '+', 'band_launches': 0, 'hs_range_fallbacks': 0}
BAND = {'f32_engine': 1, 'band_split': 0}
BAND_ROUTE = {'small_calls': 0, 'band_launches': 2, 'band_split_launches': 0, 'hs_range_fallbacks': 0}
STREAM = {'small_rows_band': 0, 'small_fused': 0}
STREAM_ROUTE = {'small_calls': 0, 'l0_stream_launches': 2, 'hs_range_fallbacks': 0}
SPLIT_ROUTE = {'small_calls': 0, 'band_split_launches': 2, 'hs_range_fallbacks': 0}

# id, (nt, nr, npkt, hidden), engine keywords, options, counters -> change per call
PREDICT_CASES = [
    ('fp32_mfma_ragged_rows', (4, 2, 37, (64, 64)), {}, FP32_MFMA, NO_SPLIT_ENGINE),
    ('fp32_mfma_ragged_widths', (8, 3, 5, (100, 36)), {}, FP32_MFMA, NO_SPLIT_ENGINE),
    ('fp32_mfma_one_layer_nt12', (12, 2, 7, (40,)), {}, FP32_MFMA, NO_SPLIT_ENGINE),
    ('fp32_mfma_three_layers', (4, 1, 6, (32, 48, 40)), {}, FP32_MFMA, NO_SPLIT_ENGINE),
    ('split_separate_nt12', (12, 3, 11, (48, 80)), {}, SEPARATE, SEPARATE_ROUTE),
    ('split_separate_narrow', (4, 1, 30, (16, 16)), {}, SEPARATE, SEPARATE_ROUTE),
    ('split_separate_one_layer', (4, 1, 70, (128,)), {}, SEPARATE, SEPARATE_ROUTE),
    ('band_ragged_last_band', (8, 2, 70, (128, 256)), {}, BAND, BAND_ROUTE),
    ('band_staged_nt16', (16, 2, 41, (128, 256)), {}, BAND, BAND_ROUTE),
    ('band_table_slab_nt100', (100, 1, 5, (128, 256)), {}, BAND, BAND_ROUTE),
    ('band_column_split_2', (16, 2, 9, (128, 512)), {}, {'f32_engine': 1, 'band_split': 2}, SPLIT_ROUTE),
    ('band_column_split_4', (16, 2, 9, (128, 512)), {}, {'f32_engine': 1, 'band_split': 4}, SPLIT_ROUTE),
    ('l0_stream_in_kernel_row_pass', (16, 2, 21, (208, 512)), {}, STREAM, STREAM_ROUTE),
    ('l0_stream_row_max_three_blocks', (16, 3, 183, (128, 512)), {}, STREAM, STREAM_ROUTE),
    ('bf16_general', (8, 2, 37, (64, 64)), {'dtype': 'bf16'}, {'force_tile': 128, 'l0_stream': 0},
     {'small_calls': 0, 'l0_stream_launches': 0, 'band_launches': 0}),
    ('bf16_band4', (32, 1, 3, (256, 256)), {'dtype': 'bf16', 'n_out': 52}, {'force_tile': 256}, {'small_calls': 0, 'band_launches': 2}),
    ('bf16_l0_stream', (16, 2, 70, (128, 64)), {'dtype': 'bf16'}, {}, {'small_calls': 0, 'l0_stream_launches': 2}),
    ('conv1d', (4, 2, 1, (64, 32)), {'model': 'CONV1D'}, {}, {'conv_launches': '+', 'small_calls': 1}),
    ('input_pool_max', (4, 2, 3, (64, 64)), {'input_pool': 'max'}, {}, {'small_calls': 1}),
    ('input_pool_avg', (4, 2, 3, (64, 64)), {'input_pool': 'avg'}, {}, {'small_calls': 1}),
]


@pytest.mark.parametrize('name,shape,kw,opts,route', PREDICT_CASES, ids=[c[0] for c in PREDICT_CASES])
def test_a_predict_device(pkg, oracle, name, shape, kw, opts, route):
    nt, nr, npkt, hidden = shape
    kw = dict(kw)
    n_out = kw.pop('n_out', N)
    e, _, _ = _model(pkg, oracle, 2000 + nt + npkt, nt, nr, hidden, n_out=n_out, opts=opts, **kw)
    if 'input_pool' in kw:
        assert e.get_option('input_pool') == {'max': 1, 'avg': 2}[kw['input_pool']]
    if name == 'conv1d':
        assert e.get_option('model_type') == 1
    re, im = _planes(_packets(oracle, 3000 + nt + npkt, nt, nr, npkt))
    out = (npkt, nr, nt, n_out)
    got = both_ways(e, lambda i, o: e.predict_device(i['ltf_re'], i['ltf_im'], npkt, o['out_re'], o['out_im']),
                    {'ltf_re': re, 'ltf_im': im}, {'out_re': out, 'out_im': out}, route)
    assert np.isfinite(got['out_re']).all() and np.isfinite(got['out_im']).all()
    if name == 'bf16_band4':
        assert e.get_option('band4') == 1 and e.get_option('band4_available') == 1, 'the register-blocked form did not serve the call'
    e.close()


@pytest.mark.parametrize('nt,nr,npkt,hidden', [(16, 2, 1, (256, 256)), (16, 1, 7, (128,))])
@pytest.mark.parametrize('fused', [1, 0])
def test_a_estimate_device_one_packet_path(pkg, oracle, fused, nt, nr, npkt, hidden):
    """LS + DNN of at most 8 preambles: the LS estimate inside the layer-0 launch (`small_ls_fused` 1) and as its own launch (0)"""
    e, _, _ = _model(pkg, oracle, 2100 + nt + npkt, nt, nr, hidden, opts={'small_ls_fused': fused})
    re, im = _planes(_packets(oracle, 3100 + nt + npkt, nt, nr, npkt, snr_db=3.0))
    out = (npkt, nr, nt, N)
    both_ways(e, lambda i, o: e.estimate_device(i['ltf_re'], i['ltf_im'], npkt, o['out_re'], o['out_im'], o['h_re'], o['h_im']),
              {'ltf_re': re, 'ltf_im': im}, {'out_re': out, 'out_im': out, 'h_re': out, 'h_im': out},
              {'small_calls': 1, 'small_ls_launches': fused})
    e.close()


def test_a_estimate_device_under_graph_replay(pkg, oracle):
    """`use_graph`: the first call runs eagerly, the second is captured, the following ones replay the captured hipGraph on the guarded
    arrays.  Every call bit-identical with the eager call on plain arrays; guards, inputs and the unwritten count checked after the
    last replay (a replay that wrote outside its arrays would have done so on every one of them)."""
    nt, nr, npkt, hidden = 8, 2, 4, (64, 64)
    e, _, _ = _model(pkg, oracle, 2200, nt, nr, hidden)
    re, im = _planes(_packets(oracle, 3200, nt, nr, npkt))
    out = (npkt, nr, nt, N)
    names = ('out_re', 'out_im', 'h_re', 'h_im')
    d_re, d_im = e.to_device(re), e.to_device(im)
    plain = [e.empty(out) for _ in names]
    s0 = e.get_option('small_calls')
    e.estimate_device(d_re, d_im, npkt, *plain)
    e.synchronize()
    assert e.get_option('small_calls') == s0 + 1
    eager = [a.download() for a in plain]
    g_in = [Guarded(e, re.shape, 'in', re, name='ltf_re'), Guarded(e, im.shape, 'in', im, name='ltf_im')]
    g_out = [Guarded(e, out, 'out', name=k) for k in names]
    e.set_option('use_graph', 1)
    r0, calls = e.get_option('graph_replays'), 0
    while e.get_option('graph_replays') < r0 + 2:
        calls += 1
        assert calls <= 8, 'the call never replayed'
        e.estimate_device(g_in[0], g_in[1], npkt, *g_out)
        e.synchronize()
        for k, a, want in zip(names, g_out, eager):
            assert _same(a.download(), want), 'call %d under use_graph (%d replays so far): %s differs from the eager call' \
                % (calls, e.get_option('graph_replays') - r0, k)
    assert calls >= 3, 'eager, capture, two replays'
    for a in g_in + g_out:
        a.check()
    assert all(a.count_unwritten() == 0 for a in g_out) and all(a.unchanged() for a in g_in)
    e.set_option('use_graph', 0)
    e.close()


# ====================================================================================================================== part A: the other device calls
def _cplx(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


@pytest.mark.parametrize('nt,nr,npkt,L', [(4, 2, 2, 100), (12, 1, 3, 1)])
def test_a_lmmse_estimate_device(pkg, nt, nr, npkt, L):
    """hvec and snr_db are inputs inside guards too: [npkt][L] and [npkt][nr] floats, far smaller than a guard word run"""
    rng = np.random.default_rng(40 + nt)
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    h = _cplx(rng, (npkt, nr, nt, N))
    hvec = _f32(np.sort(np.abs(rng.standard_normal((npkt, L)))) * (1e-7 if L > 1 else 1.0))
    snr = _f32(rng.choice([-10.0, 0.0, 10.0, 25.0], size=(npkt, nr)))
    got = both_ways(e, lambda i, o: e.lmmse_estimate_device(i['h_re'], i['h_im'], npkt, i['hvec'], L, i['snr_db'], o['out_re'], o['out_im']),
                    {'h_re': _f32(h.real), 'h_im': _f32(h.imag), 'hvec': hvec, 'snr_db': snr}, {'out_re': h.shape, 'out_im': h.shape})
    assert np.isfinite(got['out_re']).all() and np.isfinite(got['out_im']).all()
    e.close()


@pytest.mark.parametrize('nlinks,n_bins', [(37, N), (5, 7)])
def test_a_nmse_device_with_per_link(pkg, nlinks, n_bins):
    """the mean (returned on the host) and the per-link ratios; n_bins = 7: rows that are no multiple of 16 bytes"""
    rng = np.random.default_rng(50 + n_bins)
    e = pkg.CsiEngine(4, 2, hidden=(8,))
    ref, est = _cplx(rng, (nlinks, n_bins)), _cplx(rng, (nlinks, n_bins))
    means = []
    ins = {'ref_re': _f32(ref.real), 'ref_im': _f32(ref.imag), 'est_re': _f32(est.real), 'est_im': _f32(est.imag)}
    got = both_ways(e, lambda i, o: means.append(e.nmse_device(i['ref_re'], i['ref_im'], i['est_re'], i['est_im'], nlinks, n_bins, d_per_link=o['per_link'])),
                    ins, {'per_link': (nlinks,)})
    assert len(means) == 2 and np.isfinite(means[0]) and np.float64(means[0]).tobytes() == np.float64(means[1]).tobytes()
    assert abs(float(got['per_link'].astype(np.float64).mean()) - means[0]) <= 1e-6 * means[0]
    e.close()


def test_a_hybrid_weights_device(pkg):
    """every output: fbb, idx, n_atoms, gain, frf_mean; h_eval given (read-only like h)"""
    nt, nr, ns, ntrf, rays, npkt = 8, 2, 1, 2, 64, 2
    rng = np.random.default_rng(60)
    az, el = pkg.synth.random_rays(np.random.default_rng(5), rays)
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_dictionary(pkg.synth.steering_ula(nt, az, el).astype(np.complex64))
    h = _cplx(rng, (npkt, nr, nt, N))
    he = (h + 0.3 * _cplx(rng, h.shape)).astype(np.complex64)
    fbb, mean = (npkt, N, ns, ntrf), (npkt, ntrf, nt)

    def call(i, o):
        e.hybrid_weights_device(i['h_re'], i['h_im'], npkt, ns, ntrf, o['fbb_re'], o['fbb_im'], o['idx'], d_n_atoms=o['n_atoms'], d_gain=o['gain'],
                                d_frf_mean_re=o['frf_mean_re'], d_frf_mean_im=o['frf_mean_im'], d_eval_re=i['eval_re'], d_eval_im=i['eval_im'])

    got = both_ways(e, call, {'h_re': _f32(h.real), 'h_im': _f32(h.imag), 'eval_re': _f32(he.real), 'eval_im': _f32(he.imag)},
                    {'fbb_re': fbb, 'fbb_im': fbb, 'idx': (npkt, N, ntrf), 'n_atoms': (npkt, N), 'gain': (npkt, N), 'frf_mean_re': mean, 'frf_mean_im': mean},
                    {'hybrid_launches': 1 + 2 * ntrf + 2})
    idx = got['idx'].view(np.int32)
    assert idx.min() >= 0 and idx.max() < rays and (got['n_atoms'].view(np.int32) == ntrf).all() and (got['gain'] > 0).all()
    e.close()


def test_a_link_sim_device(pkg, oracle):
    """all five optional outputs; bit_errors holds int32 and bits holds bytes in arrays of floats (the last word partly written)"""
    nt, nr, ns, ntrf, bps, n_sym, npkt = 8, 4, 1, 1, 2, 2, 3
    rng = np.random.default_rng(70)
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(oracle.hadamard(nt))
    n_info, n_coded = e.link_frame_bits(ns, n_sym, bps)
    h, fbb = _cplx(rng, (npkt, nr, nt, N)), _cplx(rng, (npkt, N, ns, ntrf))
    frf = np.exp(2j * np.pi * rng.random((npkt, ntrf, nt))).astype(np.complex64)
    ins = {'h_re': _f32(h.real), 'h_im': _f32(h.imag), 'fbb_re': _f32(fbb.real), 'fbb_im': _f32(fbb.imag), 'frf_re': _f32(frf.real),
           'frf_im': _f32(frf.imag), 'noise_var': _f32(np.full(npkt, 0.05))}
    xeq = (npkt, ns, n_sym, N)
    outs = {'bit_errors': (npkt,), 'evm_rms': (npkt,), 'dt_snr_db': (npkt,), 'xeq_re': xeq, 'xeq_im': xeq, 'csi': (npkt, ns, N),
            'llr': (npkt, n_coded), 'bits': ((npkt * n_info + 3) // 4,)}

    def call(i, o):
        e.link_sim_device(i['h_re'], i['h_im'], i['fbb_re'], i['fbb_im'], i['frf_re'], i['frf_im'], i['noise_var'], 21, 4, npkt, ns, ntrf,
                          o['bit_errors'], o['evm_rms'], o['dt_snr_db'], n_sym=n_sym, bps=bps, d_xeq_re=o['xeq_re'], d_xeq_im=o['xeq_im'],
                          d_csi=o['csi'], d_llr=o['llr'], d_bits=o['bits'])

    got = both_ways(e, call, ins, outs, {'link_launches': 3}, byte_len={'bits': npkt * n_info})
    assert np.isfinite(got['llr']).all() and (got['bits'].view(np.uint8)[:npkt * n_info] <= 1).all()
    e.close()


@pytest.mark.parametrize('ncw,n_steps', [(3, 64), (1, 7)])
def test_a_viterbi_decode_device(pkg, ncw, n_steps):
    rng = np.random.default_rng(80 + n_steps)
    e = pkg.CsiEngine(4, 2, hidden=(8,))
    llr = _f32(rng.standard_normal((ncw, 3 * n_steps)))
    n_info = n_steps - 6

    def call(i, o):
        e._check(e._lib.csi_viterbi_decode_device(e._ctx, i['llr'].ptr, ncw, n_steps, o['bits'].ptr))

    got = both_ways(e, call, {'llr': llr}, {'bits': ((ncw * n_info + 3) // 4,)}, {'link_launches': 1}, byte_len={'bits': ncw * n_info})
    assert (got['bits'].view(np.uint8)[:ncw * n_info] <= 1).all()
    e.close()


def _ptr(a):
    return None if a is None else a.ptr


@pytest.mark.parametrize('kind', ['white', 'structured', 'scattering'])
def test_a_synth_packets_from_a_later_first_packet(pkg, oracle, kind):
    """the generators write only: preamble planes, and for the known-channel kinds the channel planes, noise_std and (scattering) tau"""
    from dl_channel_estimation_mamimo_amd._lib import CsiScatterConfig
    nt, nr, npkt, first, n_scat = 4, 2, 3, 5, 10
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(oracle.hadamard(nt))
    ltf, h = (npkt, nr, 320 * nt), (npkt, nr, nt, N)
    snr = (ctypes.c_float * npkt)(0.0, 10.0, -5.0)
    if kind == 'white':
        outs = {'ltf_re': ltf, 'ltf_im': ltf}
        call = lambda i, o: e.synth_white(9, first, npkt, o['ltf_re'], o['ltf_im'])      # noqa: E731
    elif kind == 'structured':
        outs = {'ltf_re': ltf, 'ltf_im': ltf, 'h_re': h, 'h_im': h, 'noise_std': (npkt,)}
        call = lambda i, o: e._check(e._lib.csi_synth_structured(e._ctx, 9, first, npkt, snr, 8, 1, o['ltf_re'].ptr, o['ltf_im'].ptr,      # noqa: E731
                                                                 o['h_re'].ptr, o['h_im'].ptr, o['noise_std'].ptr))
    else:
        outs = {'ltf_re': ltf, 'ltf_im': ltf, 'h_re': h, 'h_im': h, 'noise_std': (npkt,), 'tau': (npkt, n_scat)}
        cfg = CsiScatterConfig(n_scat=n_scat, flags=1, range_m=100.0, az_deg=30.0, el_deg=0.0, box_frac=0.1, sample_rate_hz=100e6)
        call = lambda i, o: e._check(e._lib.csi_synth_scattering(e._ctx, 9, first, npkt, snr, ctypes.byref(cfg), o['ltf_re'].ptr, o['ltf_im'].ptr,      # noqa: E731
                                                                 o['h_re'].ptr, o['h_im'].ptr, o['noise_std'].ptr, o['tau'].ptr))
    got = both_ways(e, call, {}, outs)
    assert all(np.isfinite(v).all() for v in got.values()) and np.abs(got['ltf_re']).sum(axis=-1).min() > 0
    e.close()


# ====================================================================================================================== part B
B_NT, B_NR, B_HIDDEN = 16, 2, (128, 512)
B_SIZES = (1, 4, 21, 150)
B_NAMES = ('out_re', 'out_im', 'h_re', 'h_im')


class _World:
    """One dtype: the model, 150 packets, the planes of every size on FRESH engines (eager, and under hipGraph replay), and the ONE
    long-lived engine the steps below share.  Built once per dtype (module scope)."""

    def __init__(self, pkg, oracle, dtype):
        self.pkg, self.oracle, self.dtype = pkg, oracle, dtype
        rng = np.random.default_rng(4000)
        self.P = oracle.hadamard(B_NT)
        self.w = [oracle.make_weights(rng, 320 * B_NT + B_NT, list(B_HIDDEN), N) for _ in range(2)]
        self.ltf = oracle.make_structured_packets(rng, max(B_SIZES), B_NR, self.P, snr_db=5.0)[0].astype(np.complex64)
        self.fresh, self.fresh_graph, self.route = {}, {}, {}
        for n in B_SIZES:
            e = self.engine()
            before = self.counters(e)
            self.fresh[n] = self.call(e, n)
            self.route[n] = tuple(a - b for a, b in zip(self.counters(e), before))
            e.close()
            e = self.engine()
            e.set_option('use_graph', 1)
            self.fresh_graph[n] = self.replayed(e, n)
            e.close()
        self.e = self.engine()

    def engine(self):
        e = self.pkg.CsiEngine(B_NT, B_NR, hidden=B_HIDDEN, dtype=self.dtype)
        e.load_weights('real', self.w[0])
        e.load_weights('imag', self.w[1])
        e.set_pilot(self.P)
        return e

    @staticmethod
    def counters(e):
        return tuple(e.get_option(k) for k in ROUTE_COUNTERS)

    def arrays(self, e, n, ltf=None):
        """device arrays of an n-packet call on engine e: inputs uploaded, outputs pre-filled with the UNWRITTEN pattern"""
        bufs = e.__dict__.setdefault('_part_b_arrays', {})
        if n not in bufs:
            bufs[n] = [e.empty((n, B_NR, 320 * B_NT)) for _ in range(2)] + [e.empty((n, B_NR, B_NT, N)) for _ in range(4)]
        b = bufs[n]
        re, im = _planes(self.ltf[:n] if ltf is None else ltf)
        b[0].upload(re)
        b[1].upload(im)
        for o in b[2:]:
            o.upload(np.full(o.shape, UNWRITTEN, np.uint32).view(np.float32))
        return b

    def call(self, e, n, ltf=None, checked=False):
        b = self.arrays(e, n, ltf)
        served = e.estimate_device(b[0], b[1], n, *b[2:], checked=checked)
        e.synchronize()
        self.served = served
        return [a.download() for a in b[2:]]

    def replayed(self, e, n):
        """under `use_graph`: call until the call has been served by a replay; every call's planes must equal the first one's"""
        r0, first = e.get_option('graph_replays'), None
        for it in range(8):
            got = self.call(e, n)
            first = first or got
            assert all(_same(a, b) for a, b in zip(got, first)), '%d packets under use_graph: call %d differs from the first' % (n, it)
            if e.get_option('graph_replays') > r0:
                return got
        raise AssertionError('%d packets: no replay in 8 calls' % n)

    def same_as_fresh(self, n, got, where, ref=None):
        ref = ref or self.fresh[n]
        for k, a, b in zip(B_NAMES, got, ref):
            assert not (_bits(a) == UNWRITTEN).any(), '%s: %d packets, %s has unwritten elements' % (where, n, k)
            if not _same(a, b):
                diff = np.flatnonzero(_bits(a) != _bits(b))
                raise AssertionError('%s: %d packets, %s differs from the fresh engine in %d of %d words (rel_rows %.3g)'
                                     % (where, n, k, diff.size, a.size, rel_rows(a, b)))

    def eager(self, n, where):
        before = self.counters(self.e)
        got = self.call(self.e, n)
        moved = tuple(a - b for a, b in zip(self.counters(self.e), before))
        assert moved == self.route[n], '%s: %d packets took another route than on a fresh engine: %s against %s (%s)' \
            % (where, n, moved, self.route[n], ROUTE_COUNTERS)
        self.same_as_fresh(n, got, where)


@pytest.fixture(scope='module', params=['f32', 'bf16'])
def world(request, pkg, oracle):
    w = _World(pkg, oracle, request.param)
    yield w
    w.e.close()


def test_b0_the_sizes_reach_their_routes_and_the_contract(world):
    """The fresh-engine references themselves: one packet on the one-packet path (fp32 contexts), 21 on the streaming layer 0 with the
    column-split band kernel, 150 beyond the one-packet path; every plane inside the contract of its dtype against the fp64 oracle."""
    o, w = world.oracle, world
    r = dict(zip(B_SIZES, (dict(zip(ROUTE_COUNTERS, w.route[n])) for n in B_SIZES)))
    print('\n%s routes %s: %s' % (w.dtype, ROUTE_COUNTERS, w.route))
    if w.dtype == 'f32':
        assert r[1]['small_calls'] == 1 and r[4]['small_calls'] == 1
        assert r[21]['l0_stream_launches'] == 2 and r[21]['band_split_launches'] == 2
    assert r[21]['small_calls'] == 0
    assert r[150]['small_calls'] == 0 and r[150]['hs_range_fallbacks'] == 0
    tol = TOL if w.dtype == 'f32' else BF16_TOL_FMT
    r_re, r_im = o.predict_packets(w.ltf, w.P, w.w[0], w.w[1], np.float64, pkt_batch=50)
    r_ls = o.ls_estimate(w.ltf, w.P)
    for n in B_SIZES:
        f = w.fresh[n]
        assert rel_rows(f[0], r_re[:n]) < tol and rel_rows(f[1], r_im[:n]) < tol, n
        assert rel_rows(f[2], r_ls[:n].real) < TOL and rel_rows(f[3], r_ls[:n].imag) < TOL, n


def test_b1_changing_sizes_on_one_engine(world):
    """workspace, split-K slabs, row maxima and guard words are reused across calls of different size and route"""
    for n in (150, 21, 1, 4, 150, 1):
        world.eager(n, 'after calls of other sizes')


def test_b2_hipgraph_replays_of_changing_sizes(world):
    """`use_graph` on: each size until it has replayed, in the order of step 1, on the engine that holds the eager state of step 1;
    then graphs off again and the eager calls once more.  A replay is held, bit for bit, to the EAGER call of a fresh engine and to the
    replay of a fresh engine: at these shapes (N1 = 512: two column splits at most) a captured call, which runs both component models
    on one stream, takes the kernels and the summation order of the eager one.  (Where it does not - four column splits instead of
    two at N1 = 1024 - test_mid_size_call_under_a_small_workspace_and_under_graph_replay holds the pair to 2e-6.)"""
    w = world
    for n in B_SIZES:
        w.same_as_fresh(n, w.fresh_graph[n], 'hipGraph replay on a fresh engine against its eager call')
    w.e.set_option('use_graph', 1)
    try:
        for n in (150, 21, 1, 4, 150, 1):
            r0 = w.e.get_option('graph_replays')
            got = w.replayed(w.e, n)
            assert w.e.get_option('graph_replays') > r0
            w.same_as_fresh(n, got, 'hipGraph replay on the long-lived engine')
    finally:
        w.e.set_option('use_graph', 0)
    for n in (21, 1, 150, 4):
        w.eager(n, 'after graphs were captured, replayed and dropped')


def test_b3_behind_a_range_guard_recovery(world):
    """64 packets, one of them scaled by 2^20 (HOT_CASES of test_gpu_dnn_f32.py): an fp32 context's split-f16 engine reports, the
    checked call repeats on the fp32 MFMA kernels with `f32_engine` set and put back (cached graphs dropped).  bf16 contexts have no
    range guard: the same call is simply another size.  Then 21 and 1."""
    w = world
    hot = w.ltf[:64].copy()
    hot[40] *= np.float32(2.0 ** 20)
    got = w.call(w.e, 64, ltf=hot, checked=True)
    assert all(np.isfinite(a).all() for a in got)
    if w.dtype == 'f32':
        assert w.served == 'fp32' and w.e.get_option('f32_engine') == -1, w.served
        r_re, r_im = w.oracle.predict_packets(hot, w.P, w.w[0], w.w[1], np.float64, pkt_batch=64)
        assert rel_rows(got[0], r_re) < TOL and rel_rows(got[1], r_im) < TOL
    for n in (21, 1):
        w.eager(n, 'after a range-guard recovery')


def test_b4_behind_a_call_with_nan_and_inf_preambles(world):
    """21 packets, one with a NaN in its preamble and one with an Inf, checked: the call may return or raise CsiError.  If it returns,
    the finite packets are held to the contract; nothing is asserted about the poisoned packets' own outputs.  Then 21, 150 and 1."""
    w = world
    bad = w.ltf[:21].copy()
    bad[5, 0, 100] = np.nan
    bad[13, 1, 7] = np.complex64(np.inf)
    try:
        got = w.call(w.e, 21, ltf=bad, checked=True)
    except w.pkg.CsiError as err:
        print('%s: the poisoned call raised %r' % (w.dtype, err))
        got = None
        try:
            w.e.synchronize()
        except w.pkg.CsiError:
            pass
    if got is not None:
        keep = [p for p in range(21) if p not in (5, 13)]
        tol = TOL if w.dtype == 'f32' else BF16_TOL_FMT
        r_re, r_im = w.oracle.predict_packets(w.ltf[:21], w.P, w.w[0], w.w[1], np.float64, pkt_batch=21)
        r_ls = w.oracle.ls_estimate(w.ltf[:21], w.P)
        assert rel_rows(got[0][keep], r_re[keep]) < tol and rel_rows(got[1][keep], r_im[keep]) < tol, 'finite packets beside a NaN / Inf packet'
        assert rel_rows(got[2][keep], r_ls[keep].real) < TOL and rel_rows(got[3][keep], r_ls[keep].imag) < TOL
    assert w.e.get_option('f32_engine') == -1
    for n in (21, 150, 1):
        w.eager(n, 'after a call with NaN / Inf preambles')


def test_b5_behind_option_toggles_that_drop_cached_state(world):
    w = world
    for name, off, on in (('l0_stream', 0, 1), ('band_split', 0, -1), ('small_fused', 0, 1)):
        assert w.e.get_option(name) == on, name
        w.e.set_option(name, off)
        w.call(w.e, 21)                      # a call in the other configuration: its scratch and cached plans are what must not linger
        w.call(w.e, 1)
        w.e.set_option(name, on)
    for n in (21, 1):
        w.eager(n, 'after option toggles')


# ====================================================================================================================== part C
class _At:
    """a pointer into somebody's allocation"""

    def __init__(self, ptr):
        self.ptr = ptr


def test_c_misaligned_planes_are_refused_before_anything_runs(pkg, oracle):
    """A plane 4 bytes into a live allocation: CsiError with the argument's name, and no counter moves - the check sits in front of every
    launch.  (The generators' own refusals are in test_gpu_sweep.py / test_gpu_scatter.py.)"""
    nt, nr, npkt, ns, ntrf = 8, 2, 2, 1, 1
    e, _, _ = _model(pkg, oracle, 5000, nt, nr, (64, 64))
    big = [e.to_device(np.zeros((npkt + 1, nr, nt, 320), np.float32)) for _ in range(8)]      # live, and larger than any plane below
    ok = lambda k: big[k]                     # noqa: E731
    off = lambda k: _At(big[k].ptr + 4)       # noqa: E731
    counters = ROUTE_COUNTERS + ('hs_launches', 'graph_replays', 'hybrid_launches', 'link_launches', 'small_ls_launches')
    before = {k: e.get_option(k) for k in counters}

    def refused(who, arg, fn):
        with pytest.raises(pkg.CsiError) as err:
            fn()
        assert err.value.code == -1 and '%s: %s must start on a 16-byte boundary' % (who, arg) in str(err.value), (who, arg, str(err.value))

    def each(who, names, launch):
        """launch(arrays) with every plane argument in turn moved 4 bytes in"""
        for j, arg in enumerate(names):
            refused(who, arg, lambda: launch([off(k) if k == j else ok(k) for k in range(len(names))]))

    each('csi_predict_device', ('d_ltf_re', 'd_ltf_im', 'd_out_re', 'd_out_im'), lambda a: e.predict_device(a[0], a[1], npkt, a[2], a[3]))
    each('csi_ls_estimate_device', ('d_ltf_re', 'd_ltf_im', 'd_h_re', 'd_h_im'), lambda a: e.ls_estimate_device(a[0], a[1], npkt, a[2], a[3]))
    each('csi_estimate_device', ('d_ltf_re', 'd_ltf_im', 'd_out_re', 'd_out_im', 'd_h_re', 'd_h_im'), lambda a: e.estimate_device(a[0], a[1], npkt, *a[2:]))
    e.set_option('use_graph', 1)
    each('csi_estimate_device', ('d_ltf_re', 'd_ltf_im', 'd_out_re', 'd_out_im', 'd_h_re', 'd_h_im'), lambda a: e.estimate_device(a[0], a[1], npkt, *a[2:]))
    e.set_option('use_graph', 0)
    each('csi_lmmse_estimate_device', ('d_h_re', 'd_h_im', 'd_out_re', 'd_out_im'),
         lambda a: e.lmmse_estimate_device(a[0], a[1], npkt, big[6], 4, big[7], a[2], a[3]))
    each('csi_hybrid_weights_device', ('d_h_re', 'd_h_im', 'd_eval_re', 'd_eval_im', 'd_fbb_re', 'd_fbb_im', 'd_frf_mean_re', 'd_frf_mean_im'),
         lambda a: e.hybrid_weights_device(a[0], a[1], npkt, ns, ntrf, a[4], a[5], big[0], d_frf_mean_re=a[6], d_frf_mean_im=a[7], d_eval_re=a[2], d_eval_im=a[3]))
    each('csi_link_sim_device', ('d_h_re', 'd_h_im', 'd_fbb_re', 'd_fbb_im', 'd_frf_re', 'd_frf_im', 'd_xeq_re', 'd_xeq_im'),
         lambda a: e.link_sim_device(a[0], a[1], a[2], a[3], a[4], a[5], big[0], 1, 0, npkt, ns, ntrf, big[1], big[2], big[3], n_sym=1, bps=2,
                                     d_xeq_re=a[6], d_xeq_im=a[7]))
    each('csi_synth_white', ('d_re', 'd_im'), lambda a: e.synth_white(1, 0, npkt, a[0], a[1]))
    e.synchronize()
    assert {k: e.get_option(k) for k in counters} == before, 'a refused call moved a counter'
    assert all(not a.download().any() for a in big), 'a refused call wrote'
    # the context stays usable, and an aligned slice of a larger allocation (a later packet range) is served
    rng = np.random.default_rng(1)
    re, im = _f32(rng.standard_normal((3, nr, 320 * nt))), _f32(rng.standard_normal((3, nr, 320 * nt)))
    d_re, d_im, h = e.to_device(re), e.to_device(im), [e.empty((3, nr, nt, N)) for _ in range(4)]
    e.ls_estimate_device(d_re, d_im, 3, h[0], h[1])
    pkt_in, pkt_out = 4 * nr * 320 * nt, 4 * nr * nt * N
    e.ls_estimate_device(_At(d_re.ptr + pkt_in), _At(d_im.ptr + pkt_in), 2, _At(h[2].ptr + pkt_out), _At(h[3].ptr + pkt_out))
    e.synchronize()
    assert _same(h[2].download(1, 2), h[0].download(1, 2)) and _same(h[3].download(1, 2), h[1].download(1, 2))
    e.close()
