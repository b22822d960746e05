"""GPU tests (-m gpu): EVERY LS kernel instantiation of csrc/csi_ls.hpp (LS_KERNELS) runs on the device, against the fp64 oracle.

tests/test_ls_routes_host.py pins on a model of the HIP runtime which options reach which instantiation; the value tests reach the instantiations
their hand-picked shapes happen to hit.  This file walks the list between the two: tests/ls_rows.py derives one case (Nt, pilot class, "ls_kernel",
"ls_v2") per kernel name of the recording, and each case makes three calls on ONE context whose options are set as the recording's driver set
them ("ls_v2", then "ls_kernel", then the pilot), after asserting that the four recorded options read back - the case still reaches its row:

  one item        one packet of standard-normal planes through the guard bands of tests/guarded.py (both_ways of
                  tests/test_gpu_memory_contract.py: guards intact, inputs unmodified, every output word written, plain and guarded run
                  bit-identical), the result against the oracle;
  persistent walk white packets for nr = 3 rx antennas, the smallest packet count with more than 256 x ls_per_cu + 2 items - more items than
                  resident workgroups, no multiple of the grid - every item finite and non-zero; items 0, 1, grid - 1, grid, grid + 1 and the
                  last (first and second item of a workgroup) against the oracle; a second run bit-identical.  The one-antenna-tile rows of the
                  bf16-split kernel walk their loop here too (DESIGN.md 4.12 closed what kept them out of tests);
  back            the default options ("ls_v2" 0, "ls_kernel" 0) on the same context and the one-item call again against the oracle: the
                  dynamic-LDS attribute, which only a real device enforces, follows the plan in both directions.

The contexts have nr = 1 like the recording's (the four options are compared with it); the walk hands them the [npkt, 3, 320 Nt] planes of an
nr = 3 call as 3 npkt one-antenna packets - the same bytes and the same item count: an LS item is a (packet, rx) pair and no LS kernel sees nr.

Tolerance: rel_rows < 1e-5, the LS contract of BASELINE.json (TOL of tests/test_gpu_ls.py).  The worst error per family is printed by the last
test of the file (run with -s to see it)."""
import os
import sys
import time

import numpy as np
import pytest

from conftest import rel_rows

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ls_rows                                              # noqa: E402
from test_gpu_memory_contract import both_ways              # noqa: E402

N = 234
NR_WALK = 3
CASES = ls_rows.cases()
WORST = {}          # family -> [worst rel_rows against the oracle, the kernel it came from]; filled by the cases, reported by the last test
T0 = time.time()


def _note(kernel, err):
    w = WORST.setdefault(ls_rows.family(kernel), [0.0, ''])
    if err >= w[0]:
        w[:] = [err, ls_rows.short_name(kernel)]


def _one_item(e, oracle, P, rng, nt):
    re = rng.standard_normal((1, 1, 320 * nt)).astype(np.float32)
    im = rng.standard_normal((1, 1, 320 * nt)).astype(np.float32)
    shape = (1, 1, nt, N)
    got = both_ways(e, lambda i, o: e.ls_estimate_device(i['ltf_re'], i['ltf_im'], 1, o['h_re'], o['h_im']),
                    {'ltf_re': re, 'ltf_im': im}, {'h_re': shape, 'h_im': shape})
    ref = oracle.ls_estimate(re.astype(np.float64) + 1j * im.astype(np.float64), P)
    return rel_rows(np.concatenate([got['h_re'], got['h_im']], -1), ls_rows.cat(ref))


@pytest.mark.parametrize('case', CASES, ids=[ls_rows.short_name(c.kernel) for c in CASES])
def test_ls_row_on_the_device(pkg, oracle, case):
    c = case
    rng = np.random.default_rng(sum(map(ord, c.kernel)))
    P32 = ls_rows.pilots(c.nt)[c.kind]
    P = P32.astype(np.float64)
    e = pkg.CsiEngine(c.nt, 1, hidden=(8,))
    e.set_option('ls_v2', c.ls_v2)
    e.set_option('ls_kernel', c.ls_kernel)
    e.set_pilot(P32)
    got = tuple(e.get_option(k) for k in ls_rows.OPTIONS)
    assert got == tuple(c[5:]), 'the case no longer reaches its row: %s read back as %s, recorded %s' % (ls_rows.OPTIONS, got, tuple(c[5:]))

    # one item, inside guard bands
    err = _one_item(e, oracle, P, rng, c.nt)
    print('\n%s one item: rel_rows %.3g' % (ls_rows.short_name(c.kernel), err))
    _note(c.kernel, err)
    assert err < ls_rows.TOL, ('one item', err)

    # persistent walk
    npkt = ls_rows.walk_packets(c.ls_per_cu, NR_WALK)
    items = npkt * NR_WALK
    assert items > 256 * c.ls_per_cu + 2
    ltf = pkg.synth.white_packets(rng, npkt, NR_WALK, c.nt).reshape(items, 1, 320 * c.nt)
    h = e.ls_estimate(ltf)
    assert h.shape == (items, 1, c.nt, N)
    assert tuple(e.get_option(k) for k in ls_rows.OPTIONS) == tuple(c[5:])
    finite = np.isfinite(h.view(np.float32)).all(axis=(1, 2, 3))
    power = np.abs(h).sum(axis=(1, 2, 3))
    assert finite.all() and power.min() > 0, ('walk: items not finite %s, items all zero %s' % (np.flatnonzero(~finite)[:20], np.flatnonzero(power == 0)[:20]))
    sel = ls_rows.walk_items(c.ls_per_cu, items)
    ref = oracle.ls_estimate(ltf[sel], P)
    per_item = [rel_rows(ls_rows.cat(h[i]), ls_rows.cat(r)) for i, r in zip(sel, ref)]
    print('%s walk of %d items, per item %s: rel_rows %s' % (ls_rows.short_name(c.kernel), items, sel, ' '.join('%.3g' % v for v in per_item)))
    _note(c.kernel, max(per_item))
    assert max(per_item) < ls_rows.TOL, ('walk', dict(zip(sel, per_item)))
    again = e.ls_estimate(ltf)
    differ = np.flatnonzero((h.view(np.uint32) != again.view(np.uint32)).any(axis=(1, 2, 3)))
    assert differ.size == 0, 'walk: %d items differ on the second run, the first %s' % (differ.size, differ[:20])
    del h, again, ltf

    # back to the default plan on the same context
    e.set_option('ls_v2', 0)
    e.set_option('ls_kernel', 0)
    err = _one_item(e, oracle, P, rng, c.nt)
    print('%s back on the default plan (mode %d): rel_rows %.3g' % (ls_rows.short_name(c.kernel), e.get_option('ls_mode'), err))
    assert err < ls_rows.TOL, ('default plan behind the row', e.get_option('ls_mode'), err)
    e.close()


def test_zz_worst_error_per_family():
    """the figures a later tightening of the contract can start from (nothing new is asserted: every case has asserted its own)"""
    print('\nworst rel_rows against the fp64 oracle per LS kernel family (tolerance %.0e), %.1f s since the file was imported:' % (ls_rows.TOL, time.time() - T0))
    for f in sorted(WORST):
        print('  %-28s %.3g  (%s)' % (f, WORST[f][0], WORST[f][1]))
    assert all(w[0] < ls_rows.TOL for w in WORST.values())
