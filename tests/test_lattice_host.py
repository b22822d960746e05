"""Host tests (no GPU) of the integer-lattice fixtures of tests/lattice_cases.py, for every shape tests/test_gpu_dnn_exact.py runs:
the fixture stays on the lattice (every emulation of a device arithmetic EQUALS the fp64 oracle), it reaches what it claims to reach
(conditions, not measurements), and it is sensitive: mutants of the emulation - each one an indexing or rounding-mode error of the kind a
kernel port makes - change the output, while the norm-relative tolerance of the bf16 tests lets some of them through."""
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
