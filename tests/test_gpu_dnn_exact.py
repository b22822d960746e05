"""GPU tests (-m gpu) of every DNN kernel route on the integer-lattice fixtures of tests/lattice_cases.py: no operand and no sum needs
rounding in bf16, in split f16 or in fp32 (tests/test_lattice_host.py proves that for every shape used here), so the device output must
EQUAL the fp64 oracle, element for element, on every route and in every arithmetic mode.  A norm-relative tolerance is a rounding budget
that an addressing error can hide in; here a mismatch is an indexing fact, reported with its coordinates.

Every route is forced with the options and confirmed with the launch counters the tolerance tests use (test_gpu_dnn_bf16.py,
test_gpu_dnn_f32.py, test_gpu_l0_mfma16.py, test_gpu_small_calls.py); a case that did not run the intended kernel fails.  Every case
predicts twice and the two runs must be equal as well.  The reference is oracle.predict_packets_shared for every shape: the host module
shows it equal to the literal oracle.predict_packets on these fixtures, and the literal form of the large batches would take minutes.

The CONV1D models (conv_frontend_kernel and a layer 0 of K0 = 64 len_ltf) run on the fixtures of lc.conv_lattice_case: integer samples, taps of
+-1, a conv BatchNormalization whose scale is gamma exactly, so every feature is a multiple of 1/2 that bf16 holds.  'zero_rest' (shift folded
to 0, bias <= 0: features only around the samples, so layer 0's sum stays inside bf16's 8 bits; both context types), 'full' (every feature
non-zero; fp32 contexts) and 'tie' (features half way between two bf16 numbers, against the bf16 emulation - still equality) cover the
one-packet gemv, the skinny gemv + range sum, l0_hs_stream, the split-f16 and the fp32 MFMA GEMM, the bf16 GEMM, 256 k ranges, the
grid-stride loop of the front end, several chunks, the rows form and graph replay.

Routes that are not bit-exact: none."""
import numpy as np
import pytest

import lattice_cases as lc

pytestmark = pytest.mark.gpu

_REF = {}


def _case(case, dense=False, pool=None):
    c = lc.lattice_case(*case, dense=dense, pool=pool)
    key = (case, dense, pool)
    if key not in _REF:
        if len(_REF) > 3:
            _REF.clear()
        from oracle import csi_oracle
        r_re, r_im = csi_oracle.predict_packets_shared(c.ltf_in, c.P, c.w_re, c.w_im)
        _REF[key] = (r_re.astype(np.float32), r_im.astype(np.float32))
        assert np.array_equal(_REF[key][0], r_re) and np.array_equal(_REF[key][1], r_im)          # lattice points: exact as float32
    return c, _REF[key]


def _engine(pkg, c, dtype='f32', **kw):
    e = pkg.CsiEngine(c.nt, c.nr, hidden=c.hidden, n_out=c.n_out, bn_eps=c.bn_eps, dtype=dtype, input_pool=c.pool,
                      model='CONV1D' if getattr(c, 'conv', None) else 'FC', **kw)
    e.load_weights('real', c.w_re)
    e.load_weights('imag', c.w_im)
    e.set_pilot(c.P)
    return e


def assert_exact(got, ref, what):
    """got, ref [npkt, nr, nt, n_out]: equal element for element, or a report of where they differ."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float32, (what, got.shape, ref.shape, got.dtype)
    if np.array_equal(got, ref):
        return
    npkt, nr, nt, n_out = ref.shape
    bad = np.argwhere(~(got == ref))
    rows = (bad[:, 0] * nr + bad[:, 1]) * nt + bad[:, 2]
    first = ['(packet %d, rx %d, tx %d, column %d): got %r, ref %r' % (p, r, t, n, float(got[p, r, t, n]), float(ref[p, r, t, n]))
             for p, r, t, n in bad[:8]]
    sets = {'row % 128': rows % 128, 'row % 32': rows % 32, 'column % 32': bad[:, 3] % 32, 'column % 16': bad[:, 3] % 16}
    raise AssertionError('%s: %d of %d elements differ (%d of %d rows, %d of %d columns)\n  %s\n  %s' % (
        what, len(bad), ref.size, len(np.unique(rows)), npkt * nr * nt, len(np.unique(bad[:, 3])), n_out, '\n  '.join(first),
        '\n  '.join('%s in %s' % (k, sorted(set(v.tolist()))) for k, v in sets.items())))


def _predict_exact(e, c, ref, what):
    o_re, o_im = e.predict(c.ltf)
    assert_exact(o_re, ref[0], what + ', real model')
    assert_exact(o_im, ref[1], what + ', imag model')
    p_re, p_im = e.predict(c.ltf)
    assert np.array_equal(o_re, p_re) and np.array_equal(o_im, p_im), what + ': two runs differ'


def _samples_exact(oracle, e, c, ref, what, npkt=3):
    """the literal network (predict_samples) on the rows of the first packets"""
    n = min(npkt, c.npkt)
    for i, d in enumerate(('real', 'imag')):
        x = oracle.samples_from_packets(c.ltf[:n], c.P.astype(np.float32), d)
        y = e.predict_samples(d, x)
        assert_exact(np.asarray(y).reshape(n, c.nr, c.nt, c.n_out), ref[i][:n], what + ', predict_samples ' + d)


def _counters(e, *names):
    return tuple(e.get_option(n) for n in names)


BF16_ROUTE_COUNTERS = ('band_launches', 'band_split_launches', 'l0_stream_launches', 'bf16_l0_fused_split_launches')


# ---------------------------------------------------------------------------------------------------------------- bf16 contexts
@pytest.mark.parametrize('case', lc.BF16_TILE_CASES, ids=lc.case_id)
def test_bf16_tile_kernels(pkg, oracle, case):
    """gemm_bf16: the 128 x 128 lock-step and the 256 x 256 ping-pong kernel, h1 materialised or generated inside the first per-pair GEMM"""
    c, ref = _case(case)
    e = _engine(pkg, c, 'bf16')
    for tile in (128, 256):
        for fused in (0, 1):
            e.set_option('force_tile', tile)
            e.set_option('bf16_fused_h1', fused)
            n0 = _counters(e, *BF16_ROUTE_COUNTERS)
            _predict_exact(e, c, ref, 'bf16 force_tile %d bf16_fused_h1 %d' % (tile, fused))
            assert _counters(e, *BF16_ROUTE_COUNTERS) == n0, 'another route than the tile kernels served the call'
    if case == lc.BF16_TILE_CASES[0]:
        _samples_exact(oracle, e, c, ref, 'bf16 tile kernels')
    e.close()


@pytest.mark.parametrize('case', lc.BF16_BAND_CASES, ids=lc.case_id)
def test_bf16_band_kernels(pkg, oracle, case):
    """csi_band4_bf16 / csi_band8_bf16 ("hs_band" = 2: also the per-lane form of Nt < 32), ragged last bands, bands over three pair rows"""
    c, ref = _case(case)
    e = _engine(pkg, c, 'bf16')
    e.set_option('force_tile', 256)
    e.set_option('hs_band', 2)
    for band4 in (1, 0):
        e.set_option('band4', band4)
        n0 = e.get_option('band_launches')
        _predict_exact(e, c, ref, 'bf16 hs_band 2 band4 %d' % band4)
        assert e.get_option('band_launches') == n0 + 4, 'the band kernel did not serve both models of both calls'
        assert e.get_option('band4_available') == 1
    if case == lc.BF16_BAND_CASES[0]:
        _samples_exact(oracle, e, c, ref, 'bf16 band kernels')
    e.close()


@pytest.mark.parametrize('case', lc.BF16_SPLIT_CASES, ids=lc.case_id)
def test_bf16_column_split_band_kernel(pkg, oracle, case):
    """csi_band8_bf16_cs: automatic, 2 and 4 column splits"""
    c, ref = _case(case)
    e = _engine(pkg, c, 'bf16')
    for split in (-1, 2, 4):
        e.set_option('band_split', split)
        n0 = e.get_option('band_split_launches')
        _predict_exact(e, c, ref, 'bf16 band_split %d' % split)
        assert e.get_option('band_split_launches') == n0 + 4, 'the column-split band kernel did not serve both models of both calls'
    if case == lc.BF16_SPLIT_CASES[0]:
        _samples_exact(oracle, e, c, ref, 'bf16 column split')
    e.close()


@pytest.mark.parametrize('case', lc.BF16_L0_STREAM_CASES, ids=lc.case_id)
def test_bf16_layer0_weight_streaming_kernel(pkg, oracle, case):
    c, ref = _case(case)
    e = _engine(pkg, c, 'bf16')
    n0 = e.get_option('l0_stream_launches')
    _predict_exact(e, c, ref, 'bf16 l0_stream')
    assert e.get_option('l0_stream_launches') == n0 + 4
    e.set_option('l0_stream', 0)                                   # the kernels it replaces, on the same context
    _predict_exact(e, c, ref, 'bf16 l0_stream 0')
    assert e.get_option('l0_stream_launches') == n0 + 4
    if case == lc.BF16_L0_STREAM_CASES[0]:
        _samples_exact(oracle, e, c, ref, 'bf16 l0_stream')
    e.close()


@pytest.mark.parametrize('case', lc.BF16_L0_FUSED_CASES, ids=lc.case_id)
def test_bf16_layer0_fused_kernel_with_k_ranges(pkg, oracle, case):
    c, ref = _case(case)
    e = _engine(pkg, c, 'bf16')
    n0, s0 = _counters(e, 'bf16_l0_fused_split_launches', 'l0_stream_launches')
    _predict_exact(e, c, ref, 'bf16 bf16_l0_fused_split')
    assert _counters(e, 'bf16_l0_fused_split_launches', 'l0_stream_launches') == (n0 + 4, s0)
    e.set_option('bf16_l0_fused_split', 0)
    _predict_exact(e, c, ref, 'bf16 bf16_l0_fused_split 0')
    assert e.get_option('bf16_l0_fused_split_launches') == n0 + 4
    _samples_exact(oracle, e, c, ref, 'bf16 bf16_l0_fused_split')
    e.close()


# ---------------------------------------------------------------------------------------------------------------- fp32 contexts
FIXTURE_IDS = {False: 'sparse', True: 'dense'}
HS_GUARDS = ('hs_range_fallbacks', 'hs_weight_pins')


def _fit_activation_scale(e, dense):
    """The activation scale the library derives from a small model (up to 2^7) times the dense fixture's |h| < 2^10 leaves f16: the range guard
    then repeats a host call on the fp32 kernels ("hs_range_fallbacks" moves) and fails a device-pointer call with CSI_ERR_RANGE, as documented.
    2^4 is a scale the option allows and the host module walks; the sparse fixture stays on the automatic scale."""
    if dense:
        e.set_option('hs_act_shift', 4)


def _split_engine_served(e, h0, g0, what):
    """a split-f16 case: the engine launched, and neither the range guard nor a pinned weight copy handed work to the fp32 kernels"""
    assert e.get_option('hs_launches') > h0, what + ': the split-f16 engine did not run'
    assert _counters(e, *HS_GUARDS) == g0, what + ': the fp32 kernels were measured, not the split ones'


@pytest.mark.parametrize('dense', [False, True], ids=FIXTURE_IDS.get)
@pytest.mark.parametrize('case', lc.F32_TILE_CASES, ids=lc.case_id)
def test_f32_pair_tile_kernels(pkg, oracle, monkeypatch, case, dense):
    """gemm_f32 / gemm_hs: the 128-row and the 256-row tile kernels of every GEMM, fp32 MFMA and split f16"""
    c, ref = _case(case, dense)
    # ("force_tile" = 128 excludes the split engine by design - csi_dnn_hs.hpp hs_tail_wanted - so that tile height is an fp32 MFMA case only)
    for tile, engines in (('128', (0,)), ('256', (0, 1))):
        monkeypatch.setenv('CSI_FORCE_PAIR_TILE', tile)
        e = _engine(pkg, c)
        assert e.get_option('force_tile') == int(tile)
        for engine in engines:
            e.set_option('f32_engine', engine)
            if engine:
                _fit_activation_scale(e, dense)
            h0, g0 = e.get_option('hs_launches'), _counters(e, *HS_GUARDS)
            what = 'f32 pair tile %s f32_engine %d %s' % (tile, engine, FIXTURE_IDS[dense])
            _predict_exact(e, c, ref, what)
            if engine:
                _split_engine_served(e, h0, g0, what)
            else:
                assert e.get_option('hs_launches') == h0, what
        if tile == '256' and case == lc.F32_TILE_CASES[0]:
            _samples_exact(oracle, e, c, ref, 'f32 pair tile kernels')
        e.close()


@pytest.mark.parametrize('dense', [False, True], ids=FIXTURE_IDS.get)
@pytest.mark.parametrize('case', lc.F32_FUSE_REG_CASES, ids=lc.case_id)
def test_f32_split_engine_fused_regressor(pkg, oracle, case, dense):
    c, ref = _case(case, dense)
    e = _engine(pkg, c)
    e.set_option('f32_engine', 1)
    for fuse in (0, 1):
        e.set_option('hs_fuse_regressor', fuse)
        assert e.get_option('hs_fuse_regressor') == fuse
        h0, g0 = e.get_option('hs_launches'), _counters(e, *HS_GUARDS)
        what = 'split f16 hs_fuse_regressor %d %s' % (fuse, FIXTURE_IDS[dense])
        _predict_exact(e, c, ref, what)
        _split_engine_served(e, h0, g0, what)
    e.close()


@pytest.mark.parametrize('dense', [False, True], ids=FIXTURE_IDS.get)
@pytest.mark.parametrize('case', lc.F32_BAND_CASES, ids=lc.case_id)
def test_f32_band_kernels(pkg, oracle, case, dense):
    """csi_band4 / csi_band8 (LDS-staged, "hs_band" = 1) and the form with per-lane loads of L0 / T ("hs_band" = 3)"""
    c, ref = _case(case, dense)
    e = _engine(pkg, c)
    e.set_option('f32_engine', 1)
    e.set_option('band_split', 0)
    for hs_band in (1, 3):
        for band4 in (1, 0):
            e.set_option('hs_band', hs_band)
            e.set_option('band4', band4)
            n0, g0 = e.get_option('band_launches'), _counters(e, *HS_GUARDS)
            what = 'split f16 hs_band %d band4 %d %s' % (hs_band, band4, FIXTURE_IDS[dense])
            _predict_exact(e, c, ref, what)
            assert e.get_option('band_launches') == n0 + 4, what + ': the band kernel did not serve both models of both calls'
            assert e.get_option('band4_available') == 1
            assert _counters(e, *HS_GUARDS) == g0, what
    if not dense and case == lc.F32_BAND_CASES[0]:
        _samples_exact(oracle, e, c, ref, 'split f16 band kernels')
    e.close()


@pytest.mark.parametrize('dense', [False, True], ids=FIXTURE_IDS.get)
@pytest.mark.parametrize('case', lc.F32_BAND_TAIL_CASES, ids=lc.case_id)
def test_f32_band_tail_split(pkg, oracle, case, dense):
    """552 bands on one stream: the nearly empty last round of band workgroups runs in column splits on shifted operand pointers"""
    c, ref = _case(case, dense)
    e = _engine(pkg, c)
    e.set_option('f32_engine', 1)
    e.set_option('small_call_overlap', 0)
    d_re, d_im = e.to_device(np.ascontiguousarray(c.ltf.real)), e.to_device(np.ascontiguousarray(c.ltf.imag))
    outs = [e.empty((c.npkt, c.nr, c.nt, c.n_out)) for _ in range(2)]

    def run():
        e.predict_device(d_re, d_im, c.npkt, *outs)
        e.synchronize()
        return [x.download() for x in outs]
    for tail, moved in ((1, 2), (0, 0)):
        e.set_option('band_tail_split', tail)
        n0, g0 = e.get_option('band_tail_launches'), _counters(e, *HS_GUARDS)
        what = 'split f16 band_tail_split %d %s' % (tail, FIXTURE_IDS[dense])
        a = run()
        assert e.get_option('band_tail_launches') == n0 + moved, what
        assert_exact(a[0], ref[0], what + ', real model')
        assert_exact(a[1], ref[1], what + ', imag model')
        b = run()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what + ': two runs differ'
        assert _counters(e, *HS_GUARDS) == g0, what
    e.close()


@pytest.mark.parametrize('dense', [False, True], ids=FIXTURE_IDS.get)
@pytest.mark.parametrize('case', lc.F32_BAND_SPLIT_CASES, ids=lc.case_id)
def test_f32_column_split_band_kernel(pkg, oracle, case, dense):
    c, ref = _case(case, dense)
    e = _engine(pkg, c)
    e.set_option('f32_engine', 1)
    for split in (2, 4, -1):
        e.set_option('band_split', split)
        n0, g0 = e.get_option('band_split_launches'), _counters(e, *HS_GUARDS)
        what = 'split f16 band_split %d %s' % (split, FIXTURE_IDS[dense])
        _predict_exact(e, c, ref, what)
        assert e.get_option('band_split_launches') == n0 + 4, what + ': the column-split kernel did not serve both models of both calls'
        assert _counters(e, *HS_GUARDS) == g0, what
    e.close()


@pytest.mark.parametrize('dense', [False, True], ids=FIXTURE_IDS.get)
@pytest.mark.parametrize('case', lc.F32_L0_STREAM_CASES, ids=lc.case_id)
def test_f32_layer0_weight_streaming_kernel(pkg, oracle, case, dense):
    c, ref = _case(case, dense)
    e = _engine(pkg, c)
    e.set_option('small_rows_band', 0)
    e.set_option('small_fused', 0)
    n0, g0 = e.get_option('l0_stream_launches'), _counters(e, *HS_GUARDS)
    what = 'l0_hs_stream %s' % FIXTURE_IDS[dense]
    _predict_exact(e, c, ref, what)
    assert e.get_option('l0_stream_launches') == n0 + 4, what + ': the streaming kernel did not serve both models of both calls'
    assert _counters(e, *HS_GUARDS) == g0, what
    e.set_option('l0_stream', 0)
    _predict_exact(e, c, ref, what + ', l0_stream 0')
    assert e.get_option('l0_stream_launches') == n0 + 4
    e.close()


@pytest.mark.parametrize('dense', [False, True], ids=FIXTURE_IDS.get)
@pytest.mark.parametrize('case', lc.F32_L0_MFMA_CASES, ids=lc.case_id)
def test_f32_split_layer0_both_mfma_forms(pkg, oracle, case, dense):
    """gemm_hs layer 0 on 32x32x16 and on 16x16x32 MFMAs ("hs_l0_mfma")"""
    c, ref = _case(case, dense)
    e = _engine(pkg, c)
    e.set_option('f32_engine', 1)
    e.set_option('l0_stream', 0)
    assert e.get_option('hs_vm_cast') == 2
    for form, moved in ((32, 0), (16, 4)):
        e.set_option('hs_l0_mfma', form)
        n0, h0, g0 = e.get_option('hs_l0_mfma16_launches'), e.get_option('hs_launches'), _counters(e, *HS_GUARDS)
        what = 'split f16 hs_l0_mfma %d %s' % (form, FIXTURE_IDS[dense])
        _predict_exact(e, c, ref, what)
        assert e.get_option('hs_l0_mfma16_launches') == n0 + moved, what
        _split_engine_served(e, h0, g0, what)
    e.close()


@pytest.mark.parametrize('dense', [False, True], ids=FIXTURE_IDS.get)
@pytest.mark.parametrize('case', lc.F32_SMALL_CASES, ids=lc.case_id)
def test_f32_small_call_route(pkg, oracle, case, dense):
    """small_l0_gemv_kernel + small_tile_gemm_kernel, and the general kernels on the same call ("small_fused" = 0)"""
    c, ref = _case(case, dense)
    e = _engine(pkg, c)
    e.set_option('small_rows_band', 65536)
    assert e.get_option('small_fused') == 1
    n0 = e.get_option('small_calls')
    _predict_exact(e, c, ref, 'small call %s' % FIXTURE_IDS[dense])
    assert e.get_option('small_calls') == n0 + 2, 'the one-packet path did not take the calls'
    e.set_option('small_fused', 0)
    _predict_exact(e, c, ref, 'small call, small_fused 0, %s' % FIXTURE_IDS[dense])
    assert e.get_option('small_calls') == n0 + 2, 'the general kernels were asked for'
    e.close()


@pytest.mark.parametrize('dense', [False, True], ids=FIXTURE_IDS.get)
@pytest.mark.parametrize('case', lc.F32_GRAPH_CASES, ids=lc.case_id)
def test_f32_split_engine_under_graph_replay(pkg, oracle, case, dense):
    c, ref = _case(case, dense)
    e = _engine(pkg, c)
    e.set_option('f32_engine', 1)
    _fit_activation_scale(e, dense)
    d_re, d_im = e.to_device(np.ascontiguousarray(c.ltf.real)), e.to_device(np.ascontiguousarray(c.ltf.imag))
    outs = [e.empty((c.npkt, c.nr, c.nt, c.n_out)) for _ in range(2)]
    h0, g0 = e.get_option('hs_launches'), _counters(e, *HS_GUARDS)
    for use_graph, runs in ((0, 1), (1, 4)):
        e.set_option('use_graph', use_graph)
        for it in range(runs):
            e.predict_device(d_re, d_im, c.npkt, *outs)
            e.synchronize()
            what = 'split f16 use_graph %d run %d %s' % (use_graph, it, FIXTURE_IDS[dense])
            assert_exact(outs[0].download(), ref[0], what + ', real model')
            assert_exact(outs[1].download(), ref[1], what + ', imag model')
    assert e.get_option('graph_replays') >= 1
    _split_engine_served(e, h0, g0, 'split f16 under graph replay')
    e.close()


# ---------------------------------------------------------------------------------------------------------------- decimated-input models
@pytest.mark.parametrize('mode', ['max', 'avg'])
@pytest.mark.parametrize('case', lc.POOL_CASES, ids=lc.case_id)
def test_pooled_input_models(pkg, oracle, case, mode):
    """input_pool.hip.h in front of layer 0: the pooled samples of these preambles are max(v, 0) or v / 2, exact in every format"""
    for dtype, dense, engines in (('bf16', False, (-1,)), ('f32', False, (0, 1)), ('f32', True, (0, 1))):
        c, ref = _case(case, dense, mode)
        e = _engine(pkg, c, dtype)
        assert e.get_option('input_pool') == {'max': 1, 'avg': 2}[mode]
        for engine in engines:
            what = 'input_pool %s %s f32_engine %d %s' % (mode, dtype, engine, FIXTURE_IDS[dense])
            h0, g0 = e.get_option('hs_launches'), _counters(e, *HS_GUARDS)
            if dtype == 'f32':
                e.set_option('f32_engine', engine)
            if engine == 1:
                _fit_activation_scale(e, dense)
            _predict_exact(e, c, ref, what)
            if engine == 1:
                _split_engine_served(e, h0, g0, what)
        e.close()


# ---------------------------------------------------------------------------------------------------------------- CONV1D models
def _conv_case(case):
    """the fixture and its reference: the fp64 oracle on the features layer 0 reads ('tie': the bf16 emulation, which rounds them to nearest even)"""
    c = lc.conv_lattice_case(*case)
    key = (case, 'conv')
    if key not in _REF:
        if len(_REF) > 3:
            _REF.clear()
        from oracle import csi_oracle
        if c.conv == 'tie':
            _REF[key] = csi_oracle.predict_packets_bf16(c.ltf_in, c.P, c.w_re, c.w_im)
            assert _REF[key][0].dtype == np.float32
        else:
            r_re, r_im = csi_oracle.predict_packets_shared(c.ltf_in, c.P, c.w_re, c.w_im)
            _REF[key] = (r_re.astype(np.float32), r_im.astype(np.float32))
            assert np.array_equal(_REF[key][0], r_re) and np.array_equal(_REF[key][1], r_im)
    return c, _REF[key]


def _conv_engine(pkg, c, dtype='f32', **kw):
    e = _engine(pkg, c, dtype, **kw)
    assert e.get_option('model_type') == 1
    if c.conv == 'full':
        e.set_option('hs_act_shift', 4)          # |h1 scale + shift| reaches 3200: the automatic scale of a small model (up to 2^7) leaves f16
    return e


@pytest.mark.parametrize('case', lc.CONV_F32_SMALL_CASES, ids=lc.conv_id)
def test_conv_f32_one_packet_route(pkg, oracle, case):
    """at most 8 preambles: ONE front-end launch for both planes (each with its own model's constants) + small_l0_gemv_kernel; with
    "small_fused" = 0 one launch per model + layer0_skinny_kernel + splitk_reduce"""
    c, ref = _conv_case(case)
    e = _conv_engine(pkg, c)
    n0, v0 = _counters(e, 'small_calls', 'conv_launches')
    _predict_exact(e, c, ref, 'conv one-packet route %s' % c.conv)
    assert _counters(e, 'small_calls', 'conv_launches') == (n0 + 2, v0 + 2), 'the one-packet path (one two-plane front-end launch per call) did not take the calls'
    e.set_option('small_fused', 0)
    _predict_exact(e, c, ref, 'conv small_fused 0 %s' % c.conv)
    assert _counters(e, 'small_calls', 'conv_launches', 'l0_stream_launches') == (n0 + 2, v0 + 6, 0), 'the general path with the skinny layer 0 was asked for'
    e.close()


@pytest.mark.parametrize('case', lc.CONV_F32_MID_CASES, ids=lc.conv_id)
def test_conv_f32_layer0_routes(pkg, oracle, case):
    """74 preambles: l0_hs_stream, the split-f16 GEMM ("l0_stream" 0, "f32_engine" 1) and the fp32 MFMA GEMM ("f32_engine" 0) over the feature slab"""
    c, ref = _conv_case(case)
    e = _conv_engine(pkg, c)
    v0, s0, g0 = e.get_option('conv_launches'), e.get_option('l0_stream_launches'), _counters(e, *HS_GUARDS)
    _predict_exact(e, c, ref, 'conv l0_hs_stream %s' % c.conv)
    assert _counters(e, 'conv_launches', 'l0_stream_launches') == (v0 + 4, s0 + 4), 'the streaming kernel did not serve both models of both calls'
    e.set_option('l0_stream', 0)
    e.set_option('f32_engine', 1)
    h0 = e.get_option('hs_launches')
    _predict_exact(e, c, ref, 'conv split-f16 GEMM %s' % c.conv)
    _split_engine_served(e, h0, g0, 'conv split-f16 GEMM %s' % c.conv)
    e.set_option('f32_engine', 0)
    h0 = e.get_option('hs_launches')
    _predict_exact(e, c, ref, 'conv fp32 MFMA GEMM %s' % c.conv)
    assert _counters(e, 'hs_launches', 'l0_stream_launches', 'conv_launches') == (h0, s0 + 4, v0 + 12)
    assert _counters(e, *HS_GUARDS) == g0
    e.close()


@pytest.mark.parametrize('case', lc.CONV_F32_STRIDE_CASES, ids=lc.conv_id)
def test_conv_front_end_grid_stride_and_chunks(pkg, oracle, case):
    """220 preambles x 10 tiles: more tiles than the n_cu x 8 workgroups of a launch, so workgroups loop and their prefetched window crosses
    rows; a small workspace cuts the same batch into several chunks (feature slab behind each chunk's buffers), which must change nothing"""
    c, ref = _conv_case(case)
    assert c.npkt * c.nr * (320 * c.nt // lc.CONV_TILE) > 256 * 8
    one = _conv_engine(pkg, c)
    v0 = one.get_option('conv_launches')
    _predict_exact(one, c, ref, 'conv one chunk %s' % c.conv)
    assert one.get_option('conv_launches') == v0 + 4, 'one front-end launch per model and call expected'
    one.close()
    many = _conv_engine(pkg, c, workspace_bytes=32 << 20)
    v0 = many.get_option('conv_launches')
    _predict_exact(many, c, ref, 'conv several chunks %s' % c.conv)
    assert many.get_option('conv_launches') >= v0 + 2 * 4, 'expected several chunks per call'
    many.close()


@pytest.mark.parametrize('case', lc.CONV_RANGES_CASES, ids=lc.conv_id)
def test_conv_layer0_many_k_ranges(pkg, oracle, case):
    """Nt = 16, 9 preambles: K0 = 327680 over one output tile - the fp32 MFMA GEMM and the bf16 GEMM cut it into L0_CONV_MAX_SPLITS = 256
    ranges (slabs beyond BF16_L0_MAX_SPLITS in the split-K scratch), the split-f16 GEMM into 32"""
    c, ref = _conv_case(case)
    assert c.npkt * c.nr > 8 and 64 * 320 * c.nt // 1024 >= 256
    e = _conv_engine(pkg, c)
    e.set_option('l0_stream', 0)
    for engine in (0, 1):
        e.set_option('f32_engine', engine)
        h0, g0 = e.get_option('hs_launches'), _counters(e, *HS_GUARDS)
        _predict_exact(e, c, ref, 'conv k ranges f32_engine %d' % engine)
        if engine:
            _split_engine_served(e, h0, g0, 'conv k ranges split f16')
        else:
            assert e.get_option('hs_launches') == h0
        assert e.get_option('l0_stream_launches') == 0
    e.close()
    e = _conv_engine(pkg, c, 'bf16')
    v0 = e.get_option('conv_launches')
    _predict_exact(e, c, ref, 'conv k ranges bf16')
    assert e.get_option('conv_launches') == v0 + 4
    e.close()


@pytest.mark.parametrize('case', lc.CONV_BF16_CASES, ids=lc.conv_id)
def test_conv_bf16_contexts(pkg, oracle, case):
    """bf16 features (16-byte stores of 8 channels) into xb, then gemm_bf16 over k ranges"""
    c, ref = _conv_case(case)
    e = _conv_engine(pkg, c, 'bf16')
    v0 = e.get_option('conv_launches')
    _predict_exact(e, c, ref, 'conv bf16')
    assert e.get_option('conv_launches') == v0 + 4
    e.close()


@pytest.mark.parametrize('case', lc.CONV_TIE_CASES, ids=lc.conv_id)
def test_conv_bf16_store_rounds_ties_to_even(pkg, oracle, case):
    """features of 128.5 / 129.5: a truncating or a half-up store gives other outputs (host module); the reference is the bf16 emulation, all of whose sums are exact"""
    c, ref = _conv_case(case)
    e = _conv_engine(pkg, c, 'bf16')
    _predict_exact(e, c, ref, 'conv bf16 tie fixture')
    e.close()


@pytest.mark.parametrize('dtype,case', [('f32', lc.CONV_F32_MID_CASES[0]), ('f32', lc.CONV_F32_MID_CASES[1]), ('bf16', lc.CONV_BF16_CASES[1])],
                         ids=lambda v: v if isinstance(v, str) else lc.conv_id(v))
def test_conv_rows_form(pkg, oracle, dtype, case):
    """csi_predict_samples on raw rows [B, 320 nt + nt]: feature rows of pitch K0 + nt, the pilot columns copied behind the features"""
    c, ref = _conv_case(case)
    e = _conv_engine(pkg, c, dtype)
    v0 = e.get_option('conv_launches')
    _samples_exact(oracle, e, c, ref, 'conv rows form %s %s' % (dtype, c.conv))
    assert e.get_option('conv_launches') == v0 + 2
    e.close()


def test_conv_f32_under_graph_replay(pkg, oracle):
    c, ref = _conv_case(lc.CONV_F32_MID_CASES[0])
    e = _conv_engine(pkg, c)
    d_re, d_im = e.to_device(np.ascontiguousarray(c.ltf.real)), e.to_device(np.ascontiguousarray(c.ltf.imag))
    outs = [e.empty((c.npkt, c.nr, c.nt, c.n_out)) for _ in range(2)]
    v0, g0 = e.get_option('conv_launches'), _counters(e, *HS_GUARDS)
    for use_graph, runs in ((0, 1), (1, 4)):
        e.set_option('use_graph', use_graph)
        for it in range(runs):
            e.predict_device(d_re, d_im, c.npkt, *outs)
            e.synchronize()
            what = 'conv use_graph %d run %d' % (use_graph, it)
            assert_exact(outs[0].download(), ref[0], what + ', real model')
            assert_exact(outs[1].download(), ref[1], what + ', imag model')
    assert e.get_option('graph_replays') >= 1 and e.get_option('conv_launches') > v0
    assert _counters(e, *HS_GUARDS) == g0
    e.close()
