"""The case table of tests/test_gpu_ls_rows.py (tests/ls_rows.py) and the comparison it makes - on a machine without a GPU.

The table must reach every kernel instantiation the recording tests/golden/ls_routes.json knows (58, per family as FAMILIES of
tests/test_ls_routes_host.py counts them), with cases that are reproducible and inside what the GPU test can afford; its pilot builders must
produce the classes they are named after; and `conftest.rel_rows` against `oracle.ls_estimate` at the 1e-5 LS contract must reject an estimate
that is wrong in one sign of P, in the order of two LTF symbols, in the order of the data bins, or by 2^-12 in one antenna row - each by a
factor of ten at least."""
import numpy as np

from conftest import rel_rows

import ls_rows
from test_ls_routes_host import FAMILIES


def test_every_recorded_instantiation_has_a_case():
    table = ls_rows.load()
    cases = ls_rows.cases(table)
    recorded = ls_rows.recorded_kernels(table)
    have = [c.kernel for c in cases]
    missing = sorted(set(recorded) - set(have))
    print('\n%d of %d recorded instantiations have a case' % (len(set(recorded) & set(have)), len(recorded)))
    for c in cases:
        print('  %-62s nt=%3d %-9s ls_kernel=%d ls_v2=%d -> mode %d, %d per CU' % (ls_rows.short_name(c.kernel), c.nt, c.kind, c.ls_kernel, c.ls_v2, c.ls_mode, c.ls_per_cu))
    assert not missing, 'recorded instantiations no grid case launches: %s' % missing
    assert len(have) == len(set(have)) == 58 and have == sorted(recorded)
    per_family = {f: sum(1 for k in have if ls_rows.family(k) == f) for f in FAMILIES}
    assert per_family == FAMILIES, per_family
    assert len({ls_rows.short_name(k) for k in have}) == 58           # the test ids are distinct


def test_the_cases_are_stable_and_follow_the_preference():
    table = ls_rows.load()
    cases = ls_rows.cases(table)
    assert cases == ls_rows.cases(table) == ls_rows.cases()
    by_name = {}
    for key, by_kernel in table['grid'].items():
        nt, kind = key.split('/')
        for k, by_v2 in enumerate(by_kernel):
            for v2, rec in zip(ls_rows.V2S, by_v2):
                by_name.setdefault(ls_rows.launched(rec, table)[0], []).append((int(nt), kind, k, v2, rec))
    for c in cases:
        cells = by_name[c.kernel]
        rec = [r for nt, kind, k, v2, r in cells if (nt, kind, k, v2) == (c.nt, c.kind, c.ls_kernel, c.ls_v2)]
        assert len(rec) == 1 and tuple(table['records'][rec[0]][:4]) == tuple(c[5:]), c
        assert c.ls_kernel != 0 or all(k == 0 for _, _, k, _, _ in cells), c                       # an explicit "ls_kernel" wherever one reaches the row
        if any(k != 0 and 0 <= v2 <= 3 for _, _, k, v2, _ in cells):
            assert 0 <= c.ls_v2 <= 3, c                                                           # ... and an "ls_v2" the families know
        assert c.kind in ls_rows.pilots(c.nt), c
        assert c.ls_per_cu >= 1 and 1 <= c.ls_mode <= 7
        # what the persistent walk of the GPU test costs: items beyond the resident grid, no multiple of it, planes of a few hundred MB at most
        npkt = ls_rows.walk_packets(c.ls_per_cu)
        items, grid = 3 * npkt, 256 * c.ls_per_cu
        assert items > grid + 2 and 3 * (npkt - 1) <= grid + 2 and items % grid != 0, c
        sel = ls_rows.walk_items(c.ls_per_cu, items)
        assert sel == sorted(set(sel)) and sel[-1] == items - 1 and grid + 1 < items - 1
        assert items * c.nt * (320 + 234) * 8 < 600e6, (c, items)


def test_the_pilot_builders_make_the_classes_they_are_named_after():
    """'sylvester' the Sylvester matrix, 'vht' a Hadamard matrix in another order, 'pm1' / 'two' / 'floats' no Hadamard matrix with 1 / 2 / 3 bf16
    pieces - what csi_set_pilot reports as "ls_pilot_fast" 1 / 2 / 0 and "ls_pilot_pieces"; every recorded (Nt, class) is built"""
    table = ls_rows.load()
    want = {'sylvester': 'sylvester', 'vht': 'hadamard', 'pm1': 1, 'two': 2, 'floats': 3}
    for key in table['grid']:
        nt, kind = key.split('/')
        P = ls_rows.pilots(int(nt))[kind]
        assert P.dtype == np.float32 and P.shape == (int(nt), int(nt))
        assert ls_rows.pilot_class(P) == want[kind], key
    assert sorted('%d/%s' % (nt, k) for nt in {int(key.split('/')[0]) for key in table['grid']} for k in ls_rows.pilots(nt)) == sorted(table['grid'])
    fast = {'sylvester': 1, 'vht': 2}
    for c in ls_rows.cases(table):          # the recorded options of a case agree with the class of its pilot
        assert c.ls_pilot_fast == fast.get(c.kind, 0) and (c.kind not in ('pm1', 'two', 'floats') or c.ls_pilot_pieces == want[c.kind]), c


def test_the_comparison_rejects_four_wrong_estimates(oracle):
    """One Nt = 16 item, `oracle.ls_estimate` as the truth: each wrong variant exceeds the tolerance of the GPU test tenfold at least.
    The smallest one, an antenna row off by 2^-12, sets the margin: 2^-12 / 1e-5 = 24."""
    nt = 16
    rng = np.random.default_rng(16)
    P = np.float64(ls_rows.pilots(nt)['pm1'])
    ltf = (rng.standard_normal((1, 1, 320 * nt)) + 1j * rng.standard_normal((1, 1, 320 * nt))).astype(np.complex64)
    truth = oracle.ls_estimate(ltf, P)
    assert truth.shape == (1, 1, nt, 234)
    assert rel_rows(ls_rows.cat(truth.astype(np.complex64)), ls_rows.cat(truth)) < ls_rows.TOL / 10          # fp32 storage alone is far inside it

    flipped = P.copy()
    flipped[5, 9] = -flipped[5, 9]
    swapped = ltf.copy().reshape(1, 1, nt, 320)
    swapped[:, :, [3, 11]] = swapped[:, :, [11, 3]]
    assert not np.array_equal(P[:, 3], P[:, 11])
    scaled = truth.copy()
    scaled[0, 0, 7] *= 1 + 2.0 ** -12
    wrong = {'one sign of P flipped': oracle.ls_estimate(ltf, flipped),
             'two LTF symbols swapped': oracle.ls_estimate(swapped.reshape(1, 1, 320 * nt), P),
             'the data bins shifted by one': np.roll(truth, 1, axis=-1),
             'one antenna row scaled by 1 + 2^-12': scaled}
    errs = {k: rel_rows(ls_rows.cat(v), ls_rows.cat(truth)) for k, v in wrong.items()}
    print('\nrel_rows of the wrong variants (tolerance %.0e): %s' % (ls_rows.TOL, errs))
    assert all(e >= 10 * ls_rows.TOL for e in errs.values()), errs
    assert abs(errs['one antenna row scaled by 1 + 2^-12'] - 2.0 ** -12) < 1e-9
