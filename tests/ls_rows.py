"""One GPU case per LS kernel instantiation, derived from the host recording (test helper, no test collects from here).

tests/golden/ls_routes.json (tests/test_ls_routes_host.py) holds, per (Nt, pilot class, "ls_kernel", "ls_v2") of its `grid` section, the number
of a record: the four options the context read back ("ls_mode", "ls_per_cu", "ls_pilot_fast", "ls_pilot_pieces") and the log lines of its two
launches.  `cases()` turns that into the list tests/test_gpu_ls_rows.py walks: for every distinct kernel name of a `launch` line ONE case, the same
one on every run, chosen by a fixed order of preference among the grid cells that launch that kernel:

  1. an explicit "ls_kernel" before 0 (the row is reached because it was asked for, not because of today's automatic choice), and among the
     explicit ones the value that names the family itself (it reads back as "ls_mode") before one that falls through to it;
  2. "ls_v2" in 0 ... 3 before -1 and 4 (the values a family knows before the out-of-range ones that fall to its default shape);
  3. an Nt that is no multiple of 32 before one that is (a partial antenna tile and, for the 16-symbol chunks, a partial last chunk), then the
     smaller Nt (the cheaper case), then the most general pilot class the row admits (PILOT_KINDS from its end: arbitrary floats first), then
     the smaller "ls_kernel", then the smaller "ls_v2".

No kernel name and no case is written out here: a row added to LS_KERNELS gets its case by being recorded.

`pilots(nt)` builds a pilot matrix of every recorded class with the definitions of the recording's driver (only the class has to match, the
GPU test asserts it through "ls_pilot_fast" / "ls_pilot_pieces"); `pilot_pieces` / `pilot_class` restate the host's classification in numpy for
the device-less check of those builders."""
import collections
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ls_routes.json')
TOL = 1e-5                      # the LS contract of BASELINE.json: rel_rows against the fp64 oracle (TOL of tests/test_gpu_ls.py)
V2S = (-1, 0, 1, 2, 3, 4)       # the "ls_v2" axis of the recording's grid, in its order; the "ls_kernel" axis is 0 ... 7
PILOT_KINDS = ('sylvester', 'vht', 'pm1', 'two', 'floats')
OPTIONS = ('ls_mode', 'ls_per_cu', 'ls_pilot_fast', 'ls_pilot_pieces')
VHT4 = np.array([[1, -1, 1, 1], [1, 1, -1, 1], [1, 1, 1, -1], [-1, 1, 1, 1]], np.float32)

Case = collections.namedtuple('Case', ('kernel', 'nt', 'kind', 'ls_kernel', 'ls_v2') + OPTIONS)


def hadamard(n):
    h = np.ones((1, 1), np.float32)
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h.astype(np.float32)


def pilots(nt):
    """the pilot classes Nt admits, as the driver of tests/test_ls_routes_host.py defines them"""
    rng = np.random.default_rng(1000 + nt)
    pow2 = nt & (nt - 1) == 0
    out = {}
    if pow2:
        out['sylvester'] = hadamard(nt)
    if pow2 and nt >= 16:
        out['vht'] = np.kron(hadamard(nt // 4), VHT4).astype(np.float32)      # Hadamard-equivalent, not in the Sylvester order
    out['pm1'] = rng.choice(np.float32([-1, 1]), (nt, nt))                               # one bf16 piece
    out['two'] = (rng.choice(np.float32([-1, 1]), (nt, nt)) * (1 + rng.integers(0, 128, (nt, nt)) / 256)).astype(np.float32)      # 9 significant bits: two pieces
    out['floats'] = rng.standard_normal((nt, nt)).astype(np.float32)                    # three
    return out


def _bf16_piece(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def pilot_pieces(P):
    """bf16 pieces (truncation) the entries of P need, at most 3: pilot_pieces of csrc/csi_ls.hpp"""
    r1 = np.float32(P) - _bf16_piece(P)
    if not r1.any():
        return 1
    return 3 if (r1 - _bf16_piece(r1)).any() else 2


def pilot_class(P):
    """'sylvester', 'hadamard' (+-1, P P^T = Nt I, another order: what the recording's 'vht' is) or the number of bf16 pieces"""
    nt = P.shape[0]
    if nt & (nt - 1) == 0 and np.array_equal(P, hadamard(nt)):
        return 'sylvester'
    if np.isin(P, (-1, 1)).all() and np.array_equal(np.float64(P) @ np.float64(P).T, nt * np.eye(nt)):
        return 'hadamard'
    return pilot_pieces(P)


def load():
    with open(GOLDEN) as f:
        return json.load(f)


def launched(rec, table):
    """kernel names in the launch lines of a record (every LS call of the recording runs one kernel: one name)"""
    lines = [table['lines'][i] for i in table['records'][rec][len(OPTIONS):]]
    return sorted({l.split(' kernel=')[1] for l in lines if l.startswith('launch') and ' kernel=ls_' in l})


def family(kernel):
    return kernel.split('<')[0].split('(')[0]


def recorded_kernels(table=None):
    """every LS kernel name in a launch line of the recording, whichever section it came from"""
    table = table or load()
    return sorted({l.split(' kernel=')[1] for l in table['lines'] if l.startswith('launch') and ' kernel=ls_' in l})


def _preference(c):
    return (c.ls_kernel == 0, c.ls_kernel != c.ls_mode, not 0 <= c.ls_v2 <= 3, c.nt % 32 == 0, c.nt, -PILOT_KINDS.index(c.kind), c.ls_kernel, c.ls_v2)


def cases(table=None):
    """[Case], one per kernel name the grid of the recording launches, sorted by name"""
    table = table or load()
    best = {}
    for key, by_kernel in table['grid'].items():
        nt, kind = key.split('/')
        for k, by_v2 in enumerate(by_kernel):
            for v2, rec in zip(V2S, by_v2):
                names = launched(rec, table)
                assert len(names) == 1, (key, k, v2, names)
                c = Case(names[0], int(nt), kind, k, v2, *table['records'][rec][:len(OPTIONS)])
                if names[0] not in best or _preference(c) < _preference(best[names[0]]):
                    best[names[0]] = c
    return [best[n] for n in sorted(best)]


def short_name(kernel):
    """the instantiation without its parameter list: the test id"""
    return kernel.split('(')[0].replace(' ', '')


def walk_packets(per_cu, nr=3):
    """smallest packet count with more items than resident workgroups (256 CUs x per_cu) and no multiple of that grid"""
    return (256 * per_cu + 2) // nr + 1


def walk_items(per_cu, nitems):
    """items the walk compares with the oracle: the first items a workgroup handles, and the second ones"""
    grid = 256 * per_cu
    return [0, 1, grid - 1, grid, grid + 1, nitems - 1]


def cat(z):
    """complex [..., 234] as the rows rel_rows compares: real parts, then imaginary parts"""
    z = np.asarray(z)
    return np.concatenate([z.real, z.imag], -1)
