"""Host tests (no GPU) of the integer-lattice fixtures of tests/lattice_cases.py, for every shape tests/test_gpu_dnn_exact.py runs:
the fixture stays on the lattice (every emulation of a device arithmetic EQUALS the fp64 oracle), it reaches what it claims to reach
(conditions, not measurements), and it is sensitive: mutants of the emulation - each one an indexing or rounding-mode error of the kind a
kernel port makes - change the output, while the norm-relative tolerance of the bf16 tests lets some of them through.  The CONV1D fixtures
(last section) get the same three proofs for the front end in front of layer 0, and a tie fixture for its bf16 store."""
import numpy as np
import pytest

from conftest import rel_rows
import lattice_cases as lc

BF16_TOL_IMPL = 4e-3            # tests/test_gpu_dnn_bf16.py: what every bf16 kernel is held to against the bf16-operand emulation

FIXTURES = ([(c, False, True) for c in lc.BF16_CASES]                                   # (case, dense, a bf16 context runs it)
            + [(c, False, False) for c in lc.F32_CASES if c not in lc.BF16_CASES] + [(c, True, False) for c in lc.F32_CASES])
IDS = [lc.case_id(c) + ('-dense' if dense else '-sparse') for c, dense, _ in FIXTURES]
# decimated-input models: (case, pooling mode, dense, a bf16 context runs it)
POOLED = [(c, mode, dense, dense is False) for c in lc.POOL_CASES for mode in ('max', 'avg') for dense in (False, True)]
POOLED_IDS = [lc.case_id(c) + '-' + mode + ('-dense' if dense else '-sparse') for c, mode, dense, _ in POOLED]


def _subset(c, n_each=2):
    """first and last packets: they hold the pinned preamble columns (first / last k, last k tile)"""
    return sorted(set(list(range(min(n_each, c.npkt))) + list(range(max(0, c.npkt - n_each), c.npkt))))


def _literal_is_cheap(c, npkt, limit=1e9):
    """multiply-adds of layer 0 of the literal network over npkt packets"""
    return npkt * c.nr * c.nt * (321.0 * c.nt) * c.hidden[0] < limit


def _shifts(limit, all_of_them):
    """values of "hs_in_shift" / "hs_act_shift" the library accepts (-8 .. 14) under which `limit` stays inside f16"""
    ok = [s for s in range(-8, 15) if limit * 2.0 ** s < 65504.0]
    return ok if all_of_them else [ok[0], ok[len(ok) // 2], ok[-1]]


@pytest.mark.parametrize('case,mode,dense,bf16', POOLED, ids=POOLED_IDS)
def test_pooled_fixture_is_on_the_lattice_and_reaches_every_k(oracle, case, mode, dense, bf16):
    """input_pool max / avg: the pooled samples are max(v, 0) or v / 2, still exact everywhere"""
    import test_gpu_input_pool as tp
    c = lc.lattice_case(*case, dense=dense, pool=mode)
    assert np.array_equal(c.ltf_in, tp.pool_ltf(c.ltf, mode)), 'the pooling of the builder is not the one the pooled tests state'
    assert np.array_equal(2 * c.ltf_in.real, np.rint(2 * c.ltf_in.real)) and np.abs(c.ltf_in.real).max() <= 2
    test_fixture_is_on_the_lattice(oracle, case, dense, bf16, pool=mode)
    test_fixture_reaches_what_it_claims(case, dense, bf16, pool=mode)


@pytest.mark.parametrize('case,dense,bf16', FIXTURES, ids=IDS)
def test_fixture_is_on_the_lattice(oracle, case, dense, bf16, pool=None):
    c = lc.lattice_case(*case, dense=dense, pool=pool)
    # the whole batch: the builder's own fp64 forward, the oracle's shared-layer-0 form and (where affordable) the literal loop are ONE array
    s_re, s_im = oracle.predict_packets_shared(c.ltf_in, c.P, c.w_re, c.w_im)
    assert np.array_equal(s_re, c.trace('real').out) and np.array_equal(s_im, c.trace('imag').out)
    sel = _subset(c)
    cheap = _literal_is_cheap(c, len(sel), 1e8)         # every shift the library accepts, or the two ends and the middle of the range
    if not cheap:
        sel = sel[:1]
    lit = sel if not _literal_is_cheap(c, c.npkt) else list(range(c.npkt))
    l_re, l_im = oracle.predict_packets(c.ltf_in[lit], c.P, c.w_re, c.w_im, np.float64, pkt_batch=len(lit))
    assert np.array_equal(l_re, s_re[lit]) and np.array_equal(l_im, s_im[lit]), 'shared form != literal form'
    for d, w, ref in (('real', c.w_re, s_re), ('imag', c.w_im, s_im)):
        t = c.trace(d)
        nr = c.nr if cheap else 1                        # (a large shape: the pairs of the first rx antenna of one packet)
        x = oracle.samples_from_packets(c.ltf_in[sel][:, :nr], c.P.astype(np.float32), d)
        want = ref[sel][:, :nr].reshape(x.shape[0], -1)
        assert np.array_equal(oracle.fc_forward(x, w, np.float32), want), 'fp32 arithmetic leaves the lattice'
        for s_in in _shifts(t.max_in, cheap):
            assert np.array_equal(oracle.fc_forward_split_f16(x, w, in_shift=s_in, act_shift=0), want), ('hs_in_shift', s_in)
        for s_act in _shifts(t.max_act, cheap):
            assert np.array_equal(oracle.fc_forward_split_f16(x, w, in_shift=4, act_shift=s_act), want), ('hs_act_shift', s_act)
        if bf16:
            assert np.array_equal(oracle.fc_forward_bf16(x, w), want), 'bf16 operands leave the lattice'
            assert np.array_equal(lc.forward_bf16_hooked(x, w), want)


@pytest.mark.parametrize('case,dense,bf16', FIXTURES, ids=IDS)
def test_fixture_reaches_what_it_claims(case, dense, bf16, pool=None):
    c = lc.lattice_case(*case, dense=dense, pool=pool)
    k_cover, nonzero = c.cover()
    assert k_cover == 1.0, 'a k index of some layer never meets a non-zero activation and a non-zero weight'
    assert nonzero >= 0.90
    for d in ('real', 'imag'):
        t = c.trace(d)
        # the 16 M1 non-zeros of the batch lie at different preamble columns (three pinned ones may coincide with others) and meet a weight
        if not pool:
            assert t.l0_cover == t.l0_want >= min(1.0, (lc.L0_NNZ * c.npkt * c.nr - 3) / (320.0 * c.nt))
        assert t.max_abs_sum < lc.SUM_LIMIT
        if bf16:
            assert t.act_bf16_exact, 'a hidden activation needs more than 8 significand bits'
    rows = c.trace('real').out.reshape(-1, c.n_out)
    assert len(np.unique(rows, axis=0)) > 0.9 * len(rows) or len(rows) > 20000       # (row-distinctness of the large batches: not worth the sort)


def _layers(w):
    names = []
    i = 0
    while f'fc_dense{i}.kernel' in w:
        names.append(f'fc_dense{i}')
        i += 1
    return names + ['fc_regressor']


def _with(w, name, kernel=None, bias=None):
    m = dict(w)
    if kernel is not None:
        m[name + '.kernel'] = kernel
    if bias is not None:
        m[name + '.bias'] = bias
    return m


def _relu_outputs(x, w):
    """fp64 relu outputs [h1, h2, ...] of the literal network for the rows x"""
    hs, a, i = [], np.asarray(x, dtype=np.float64), 0
    while f'fc_dense{i}.kernel' in w:
        hs.append(np.maximum(a @ w[f'fc_dense{i}.kernel'].astype(np.float64) + w[f'fc_dense{i}.bias'], 0.0))
        sc, sh = lc.bn_fold(w, i)
        a = hs[-1] * sc + sh
        i += 1
    return hs


def _mutants(oracle, c, d, sel, forward):
    """(label, mutant output) for the weight / input mutants of one emulation `forward(x, w)`"""
    w = c.w_re if d == 'real' else c.w_im
    len_ltf = 320 * c.nt
    x = oracle.samples_from_packets(c.ltf[sel], c.P.astype(np.float32), d)
    for name in _layers(w):
        k = w[name + '.kernel']
        K = len_ltf if name == 'fc_dense0' else k.shape[0]
        picks = {0, K - 1, K - 64 if name == 'fc_dense0' else max(0, K - 64) + min(3, K - 1)}
        if name == 'fc_dense0':
            picks |= {len_ltf, len_ltf + c.nt - 1}                       # the pilot rows behind the preamble columns
        for row in sorted(picks):
            km = k.copy()
            km[row] = 0
            yield 'zero k = %d of %s' % (row, name), forward(x, _with(w, name, km))
    # two 8-element k chunks of one kernel row (one output column's weights along k) swapped
    live = _relu_outputs(x[:1], w)
    for li, name in enumerate(_layers(w)):
        k = w[name + '.kernel']
        # (a hidden layer: the row of the unit that is most active in sample 0, so that the swap reaches a live unit)
        n = int(np.argmax(live[li][0])) if li < len(live) else k.shape[1] // 2
        if name == 'fc_dense0':
            a, b = 0, next(j for j in range(1, len_ltf // 8) if k[8 * j, n] != k[0, n])
        else:
            a = int(np.flatnonzero(k[:, n])[0]) // 8                     # the first chunk that holds a weight, and the next one that differs from it
            b = next(j % (k.shape[0] // 8) for j in range(a + 1, a + k.shape[0] // 8) if not np.array_equal(
                k[8 * (j % (k.shape[0] // 8)):8 * (j % (k.shape[0] // 8)) + 8, n], k[8 * a:8 * a + 8, n]))
        km = k.copy()
        km[8 * a:8 * a + 8, n], km[8 * b:8 * b + 8, n] = k[8 * b:8 * b + 8, n], k[8 * a:8 * a + 8, n]
        yield 'k chunks %d and %d of row %d of %s swapped' % (a, b, n, name), forward(x, _with(w, name, km))
    km = w['fc_dense0.kernel'].copy()
    km[len_ltf - 64:len_ltf] = 0
    yield 'last k tile of layer 0 dropped', forward(x, _with(w, 'fc_dense0', km))
    xp = oracle.samples_from_packets(c.ltf[sel], np.roll(c.P, -1, axis=0).astype(np.float32), d)
    yield 'pilot row t + 1 for pair t', forward(xp, w)


@pytest.mark.parametrize('case,dense,bf16', FIXTURES, ids=IDS)
def test_mutants_of_the_emulation_change_the_output(oracle, case, dense, bf16):
    """Every mutant must move at least one output element of the subset it runs on - the exact comparison sees it."""
    c = lc.lattice_case(*case, dense=dense)
    sel = list(range(c.npkt)) if _literal_is_cheap(c, c.npkt) else _subset(c, 4)
    if not _literal_is_cheap(c, len(sel)):
        sel = [0, c.npkt - 1] if c.npkt > 1 else [0]
    forward = oracle.fc_forward_bf16 if bf16 else (lambda x, w: oracle.fc_forward(x, w, np.float32))
    d = 'real'
    w = c.w_re
    x = oracle.samples_from_packets(c.ltf[sel], c.P.astype(np.float32), d)
    ref = forward(x, w)
    assert np.array_equal(ref, c.trace(d).out[sel].reshape(ref.shape))
    for label, got in _mutants(oracle, c, d, sel, forward):
        assert not np.array_equal(got, ref), label
    if not bf16:
        return
    # two adjacent h1 rows across a pair-row boundary (the last pair of one preamble, the first of the next)
    def swap(h):
        h = h.copy()
        h[[c.nt - 1, c.nt]] = h[[c.nt, c.nt - 1]]
        return h
    if x.shape[0] > c.nt:
        assert not np.array_equal(lc.forward_bf16_hooked(x, w, h1_hook=swap), ref), 'h1 rows swapped'
    # truncation in place of round-to-nearest-even: one bias moved to 160.5, where bf16 steps by 1 and every h1 of that column is a tie
    # (of a unit that some unit of the next layer reads with a positive folded weight: that reader is then live in every row)
    n = 0
    if len(c.hidden) > 1:
        n = int(np.flatnonzero(((w['fc_dense1.kernel'] * lc.bn_fold(w, 0)[0][:, None]) > 0).any(1))[0])
    b = w['fc_dense0.bias'].copy()
    b[n] += 160.5
    wt = _with(w, 'fc_dense0', bias=b)
    rne = lc.forward_bf16_hooked(x, wt)
    assert np.array_equal(rne, oracle.fc_forward_bf16(x, wt))
    trunc = lc.forward_bf16_hooked(x, wt, round_h1=lc.bf16_truncate)
    assert not np.array_equal(trunc, rne), 'truncation of h1'


def test_the_norm_relative_bf16_tolerance_lets_such_errors_pass(oracle):
    """THE GAP the lattice tests close, shown on the kind of fixture the tolerance tests use (test_gpu_dnn_bf16.py::test_band_kernel_bf16_mode:
    glorot weights, structured packets, Nt = 8, hidden 256 x 256): one weight element of layer 0, or of the regressor, fetched from the
    neighbouring 8-element k chunk stays inside BF16_TOL_IMPL = 4e-3 per row (1.8e-3 and 1.9e-4 here) - a rounding budget has room for it.
    On the lattice the same mutants change elements of an array that must be EQUAL (test_mutants_of_the_emulation_change_the_output).
    (Truncation of h1 in place of round-to-nearest-even lands at 4.6e-3 on this fixture: just outside, printed, not asserted.)"""
    nt, nr, npkt, hidden = 8, 2, 4, (256, 256)
    rng = np.random.default_rng(7 * nt + 37)
    w = oracle.make_weights(np.random.default_rng(900 + nt), 320 * nt + nt, list(hidden), 234)
    P = oracle.hadamard(nt)
    ltf = oracle.make_structured_packets(rng, npkt, nr, P, snr_db=8.0)[0].astype(np.complex64)
    x = oracle.samples_from_packets(ltf, P.astype(np.float32), 'real')
    ref = lc.forward_bf16_hooked(x, w)
    assert np.array_equal(ref, oracle.fc_forward_bf16(x, w))
    for name, (row, col) in (('fc_dense0', (1000, 10)), ('fc_regressor', (3, 100))):
        km = w[name + '.kernel'].copy()
        km[row, col] = km[row + 8, col]
        got = lc.forward_bf16_hooked(x, _with(w, name, km))
        err = rel_rows(got, ref)
        print('one weight of %s from the neighbouring k chunk:' % name, err)
        assert not np.array_equal(got, ref) and 0 < err < BF16_TOL_IMPL, (name, err)
    print('truncation of h1:', rel_rows(lc.forward_bf16_hooked(x, w, round_h1=lc.bf16_truncate), ref))


def test_assert_exact_reports_where_the_arrays_differ():
    """the helper of the GPU module: silent on equal arrays; on a mismatch the count, the first coordinates and the residue sets a lane map shows in"""
    from test_gpu_dnn_exact import assert_exact
    ref = np.arange(2 * 2 * 4 * 40, dtype=np.float32).reshape(2, 2, 4, 40)
    assert_exact(ref.copy(), ref, 'same')
    got = ref.copy()
    got[1, 0, 3, 33] += 1
    got[1, 1, 3, 17] = np.nan
    with pytest.raises(AssertionError) as ex:
        assert_exact(got, ref, 'route x')
    msg = str(ex.value)
    assert 'route x: 2 of 640 elements differ (2 of 16 rows, 2 of 40 columns)' in msg
    assert '(packet 1, rx 0, tx 3, column 33): got %r, ref %r' % (float(got[1, 0, 3, 33]), float(ref[1, 0, 3, 33])) in msg
    assert 'row % 128 in [11, 15]' in msg and 'column % 32 in [1, 17]' in msg and 'column % 16 in [1]' in msg
    with pytest.raises(AssertionError):
        assert_exact(ref.astype(np.float64), ref, 'dtype')


# ---------------------------------------------------------------------------------------------------------------- CONV1D models
CONV_FIXTURES = [(c, c in lc.CONV_BF16_CASES or c in lc.CONV_RANGES_CASES) for c in lc.CONV_CASES]        # (case, a bf16 context runs it)
CONV_IDS = [lc.conv_id(c) for c, _ in CONV_FIXTURES]


def _conv_parts(c):
    """(component, weights, other model's weights, raw rows [M1, L], feature rows [M1, 64 L]) of both models"""
    m1 = c.npkt * c.nr
    yield 'real', c.w_re, c.w_im, c.ltf.real.reshape(m1, -1), c.ltf_in.real.reshape(m1, -1)
    yield 'imag', c.w_im, c.w_re, c.ltf.imag.reshape(m1, -1), c.ltf_in.imag.reshape(m1, -1)


def _pin_rows(c, part):
    """the preambles that hold pinned samples, at most the first 16"""
    return sorted({m for m, _, _, _ in c.pins[part]})[:16]


@pytest.mark.parametrize('case,bf16', CONV_FIXTURES, ids=CONV_IDS, scope='module')      # (module scope: the tests of one fixture run in a row and share its build)
def test_conv_fixture_is_on_the_lattice(oracle, monkeypatch, case, bf16):
    """the front end: the builder's fp64 statement is the one tests/test_gpu_conv1d.py states (with the lattice's eps) and the float32
    restatement in the kernel's operation order; every feature is a multiple of 1/2 that bf16 holds; behind it every forward form is ONE array"""
    import test_gpu_conv1d as tc
    monkeypatch.setattr(tc, 'BN_EPS', lc.BN_EPS)
    c = lc.conv_lattice_case(*case)
    assert c.ltf.shape == (c.npkt, c.nr, 320 * c.nt) and c.ltf_in.shape == (c.npkt, c.nr, 64 * 320 * c.nt)
    for d, w, _, x, f in _conv_parts(c):
        some = sorted(set(_pin_rows(c, d == 'imag')) | set(range(len(x) - 2, len(x))))       # (the dense fp64 statement: the pinned preambles and the last two)
        assert np.array_equal(tc.features(x[some], w), f[some]), 'the builder\'s front end is not the one the CONV1D tests state'
        for r0 in range(0, len(x), 32):
            assert np.array_equal(lc.frontend_f32(x[r0:r0 + 32], w), f[r0:r0 + 32]), 'the float32 front end leaves the lattice'
        assert np.array_equal(2 * f, np.rint(2 * f))
        assert np.array_equal(oracle.bf16_round(f), f), 'a feature needs more than 8 significand bits'
        sc, sh = lc.conv_fold(w)
        assert np.array_equal(sc, w['conv_bn.gamma']) and np.array_equal(sh, np.rint(sh))
        if c.conv == 'zero_rest':
            assert not sh.any() and w['conv_bn.moving_mean'].any() and (w['cnn1d_1.bias'] <= 0).all() and not lc.conv_rest(w).any()
        else:
            assert (sh != 0).sum() > 64 and (w['cnn1d_1.bias'] > 0).any() and (w['cnn1d_1.bias'] < 0).any() and (f != 0).mean() > 0.8
        k = w['cnn1d_1.kernel'].reshape(7, 128)
        assert set(np.unique(k)) == {-1.0, 0.0, 1.0} and ((k != 0).sum(1) >= 8).all() and ((k != 0).sum(0) >= 1).all()
    s_re, s_im = oracle.predict_packets_shared(c.ltf_in, c.P, c.w_re, c.w_im)
    assert np.array_equal(s_re, c.trace('real').out) and np.array_equal(s_im, c.trace('imag').out)
    sel = _subset(c, 1) if c.nt <= 4 else [0]          # (K0 = 327680 at Nt = 16: the rows of the first packet, first rx antenna)
    nr = c.nr if c.nt <= 4 else 1
    l_re, l_im = oracle.predict_packets(c.ltf_in[sel][:, :nr], c.P, c.w_re, c.w_im, np.float64, pkt_batch=len(sel))
    assert np.array_equal(l_re, s_re[sel][:, :nr]) and np.array_equal(l_im, s_im[sel][:, :nr]), 'shared form != literal form'
    for d, w, ref in (('real', c.w_re, s_re), ('imag', c.w_im, s_im)):
        t = c.trace(d)
        x = oracle.samples_from_packets(c.ltf_in[sel][:, :nr], c.P.astype(np.float32), d)
        want = ref[sel][:, :nr].reshape(x.shape[0], -1)
        assert np.array_equal(lc.forward_shared(x[::c.nt, :-c.nt], c.P, w), want)
        assert np.array_equal(oracle.fc_forward(x, w, np.float32), want), 'fp32 arithmetic leaves the lattice'
        step = 1 if c.nt <= 4 else 2                                   # the two ends and the middle of the accepted range (Nt = 16: the ends)
        for s_in in _shifts(t.max_in, False)[::step]:
            assert np.array_equal(oracle.fc_forward_split_f16(x, w, in_shift=s_in, act_shift=0), want), ('hs_in_shift', s_in)
        for s_act in _shifts(t.max_act, False)[::step]:
            assert np.array_equal(oracle.fc_forward_split_f16(x, w, in_shift=4, act_shift=s_act), want), ('hs_act_shift', s_act)
        if bf16:
            assert np.array_equal(oracle.fc_forward_bf16(x, w), want), 'bf16 operands leave the lattice'
            assert np.array_equal(lc.forward_bf16_hooked(x, w), want)


@pytest.mark.parametrize('case,bf16', CONV_FIXTURES, ids=CONV_IDS, scope='module')      # (module scope: the tests of one fixture run in a row and share its build)
def test_conv_fixture_reaches_what_it_claims(case, bf16):
    c = lc.conv_lattice_case(*case)
    k_cover, nonzero = c.cover()
    assert k_cover == 1.0, 'a k index behind layer 0 never meets a non-zero activation and a non-zero weight'
    assert nonzero >= 0.90
    L, m1 = 320 * c.nt, c.npkt * c.nr
    for part, (d, w, _, x, f) in enumerate(_conv_parts(c)):
        t = c.trace(d)
        assert 2 * t.max_abs_sum < lc.SUM_LIMIT                       # (the features are multiples of 1/2)
        if bf16:
            assert c.conv == 'zero_rest' and t.act_bf16_exact, 'a hidden activation needs more than 8 significand bits'
        # the cover is what the sample list reaches, derived without the dense forward
        cover = lc.conv_feat_cover(c, d)
        assert cover == lc.conv_feat_want(c, d)
        if m1 >= 64:
            assert cover >= 0.5
        # the pinned samples are where the builder says, and each one moves a feature that layer 0 weighs: the row-end pins the first /
        # last pooled position, an edge pin a position of the NEIGHBOURING tile (reached through that tile's halo only)
        pins = c.pins[part]
        assert {(m, tt) for m, _, tt, e in pins if e is None} == {(m, tt) for m in (0, 1) for tt in (0, 1, 2, L - 3, L - 2, L - 1)}
        assert {(tt - e, e) for _, _, tt, e in pins if e is not None} == {(off, e) for off in range(-3, 3) for e in lc.conv_edges(c.nt)}
        assert len(lc.conv_edges(c.nt)) >= 2 and all(e % lc.CONV_TILE == 0 and 0 < e < L for e in lc.conv_edges(c.nt))
        rest = lc.conv_rest(w)
        used = (np.abs(w['fc_dense0.kernel'][:64 * L]).sum(1) > 0).reshape(L // 2, 128)
        k = w['cnn1d_1.kernel'].reshape(7, 128)
        b = w['cnn1d_1.bias']
        for m, _, tt, e in pins:
            v = x[m, tt]
            assert v != 0 and (e is None or abs(v) == 2)
            if e is None:
                us = [0] if tt < 3 else [L // 2 - 1]
            else:
                us = [e // 2 - 1] if tt >= e else [e // 2]
            # derived for the sample alone: tap j of channel ch carries it to output sample tt + 3 - j
            alone = [(u, ch) for u in us for j in range(7) for ch in np.flatnonzero(k[j]) if (tt + 3 - j) // 2 == u
                     and max(b[ch] + k[j, ch] * v, 0) != max(b[ch], 0)]
            assert alone, ('no channel answers the pinned sample', m, tt)
            moved = (f[m].reshape(L // 2, 128)[us] != rest) & used[us]
            assert moved.any(), ('the pinned sample moves no weighed feature', m, tt)
        # both parities of the output sample for every tap: both members of a pooled pair see every tap
        mm, ts = np.nonzero(x)
        for j in range(7):
            to = ts + 3 - j
            to = to[(to >= 0) & (to < L)]
            assert (to % 2 == 0).any() and (to % 2 == 1).any(), j


@pytest.mark.parametrize('case,bf16', CONV_FIXTURES, ids=CONV_IDS, scope='module')      # (module scope: the tests of one fixture run in a row and share its build)
def test_mutants_of_the_front_end_change_the_output(oracle, case, bf16):
    """every mutant of the front-end emulation moves at least one OUTPUT element of the preambles that hold the pinned samples"""
    c = lc.conv_lattice_case(*case)
    for part, (d, w, other, x, f) in enumerate(_conv_parts(c)):
        rows = _pin_rows(c, part)
        rows = list(range(min(rows), max(rows) + 1))                  # consecutive: the neighbouring-row mutant needs the neighbours
        ref = lc.forward_shared(lc.frontend_f32(x[rows], w), c.P, w)
        assert np.array_equal(ref, c.trace(d).out.reshape(c.npkt * c.nr, c.nt, -1)[rows].reshape(ref.shape))
        for mutant in lc.CONV_MUTANTS:
            got = lc.forward_shared(lc.frontend_f32(x[rows], w, mutant, other), c.P, w)
            assert not np.array_equal(got, ref), (d, mutant)
        if part == 0 and bf16:
            break                                                     # (the imag model of the bf16 shapes: nothing the real one does not show)


@pytest.mark.parametrize('case', lc.CONV_TIE_CASES, ids=lc.conv_id)
def test_conv_tie_fixture_tells_the_rounding_modes_apart(oracle, case):
    """the bf16 store of the front end: pooled features of 128.5 / 129.5 (and 257 / 259 behind gamma = +-2) lie half way between two bf16
    numbers.  Nearest-even, truncation and half-up give three feature arrays and three outputs; the emulation's sums are exact, so the
    device must EQUAL oracle.predict_packets_bf16 on the unrounded features (it rounds them to nearest even itself)."""
    c = lc.conv_lattice_case(*case)
    assert len(c.hidden) == 1
    for d, w, _, x, f in _conv_parts(c):
        assert np.array_equal(lc.frontend_f32(x, w), f)
        stores = [oracle.bf16_round(f), lc.bf16_truncate(f), lc.bf16_half_up(f)]
        ties = stores[1] != stores[2]
        assert ties.sum() >= 64 and {128.5, 129.5} <= set(np.abs(f[ties]).tolist())
        assert (stores[0] != stores[1]).any() and (stores[0] != stores[2]).any()
        P32 = c.P.astype(np.float32)
        rows = lambda feat: np.concatenate([np.repeat(feat, c.nt, 0), np.tile(P32, (len(feat), 1))], axis=1)
        outs = [oracle.fc_forward_bf16(rows(s), w) for s in stores]
        assert np.array_equal(outs[0], oracle.fc_forward_bf16(rows(f), w)), 'the emulation rounds the features to nearest even itself'
        assert not np.array_equal(outs[1], outs[0]), 'truncating store'
        assert not np.array_equal(outs[2], outs[0]), 'half-up store'
        assert not np.array_equal(outs[1], outs[2])
        # every fp32 sum of the emulation is exact whatever its order: operands are multiples of 1/2 (features, h1 after rounding ...)
        k0 = np.abs(w['fc_dense0.kernel'].astype(np.float64))
        h_max = (np.abs(stores[0].astype(np.float64)) @ k0[:f.shape[1]]).max() + np.abs(c.P).sum(1).max() + 3
        assert 2 * h_max < lc.SUM_LIMIT
        sc, sh = lc.bn_fold(w, 0)
        assert 2 * (h_max * np.abs(sc).max() + np.abs(sh).max()) * np.abs(w['fc_regressor.kernel']).sum(0).max() < lc.SUM_LIMIT
