"""Which LS kernel serves a call, in which launch shape, and what csi_set_pilot uploads - on a machine without a GPU.

The LS estimator has 58 kernel instantiations behind one plan (csrc/csi_ls.hpp: LS_KERNELS, ls_plan): seven families, picked from Nt, the
class of the pilot matrix and five options, two of which ("ls_kernel", "ls_v2") exist for A/B runs and tests only.  Which form runs is a
correctness property of this kernel family, and the library's counters cannot tell the forms apart.  The model of the HIP
runtime can: tests/mock_hip.hpp hands every hipLaunchKernel (function handle, grid, workgroup size, dynamic LDS bytes) and every
hipFuncSetAttribute to tests/mock_library.cpp, which names the kernel through the dynamic linker (dladdr + demangling - the product table holds
no name strings) and keeps one text line per attribute call and launch of an LS kernel.  A further test-only entry point returns the four
buffers csi_set_pilot uploaded ("device" memory is host memory on the mock).

tests/golden/ls_routes.json is that log per case, RECORDED ON THE HOST CODE AS IT WAS BEFORE csrc/csi_ls.hpp EXISTED: this file, the mock
extension and the log were run on the csrc/ and include/ of the parent of the change that introduced csi_ls.hpp - plan, pilot analysis and
launch loop inside csi_mamimo.hip - by `python tests/test_ls_routes_host.py <tree with that csrc/> <output file>`.  It is the contract a change
of the plan keeps: same instantiations, same grids, same workgroup sizes, same LDS requests, same attribute calls, same uploaded bytes.  Never
re-record it from code under test.  To check it: restore that parent's csrc/ and include/ under these tests - all of them pass.

Cases (all contexts nr 1, fp32; the launches are dropped by the mock, so every LS call gets one small buffer for all four planes):
  grid      nt 8 ... 160 x the pilot classes the nt admits x "ls_kernel" 0 ... 7 x "ls_v2" -1 ... 4 ("ls_v2" has no range check: anything but the
            values a family knows is its default shape - part of the contract);
  sweep     "ls_fast_perm" 0 / 1 x "ls_fft_first_max" 0 / default / 64 x "ls_ringb_min" 0 / 16 / default x "ls_kernel" 0 / 1 / 5 / 7, every nt up
            to 128, the pilot classes without the Sylvester matrix (which none of the three options touches);
  per case  the options are set ("ls_kernel" last), then two calls: 3 packets, and 1100 - more items than 256 x ls_per_cu of every kernel, so
            the cap of the persistent grids and the one-workgroup-per-item grid of the despread-first kernel are both pinned.  Kept: "ls_mode",
            "ls_per_cu", "ls_pilot_fast", "ls_pilot_pieces", and the log from the attribute line of the last option on;
  estimate  one-packet csi_estimate_device at nt 16 / 32 / 64, Sylvester and VHT pilots, "ls_kernel" 0 / 5 x "ls_v2" 0 / 1 x "small_ls_fused"
            0 / 1: the "small_ls_launches" the call added and its LS log - one small_l0_ls_kernel launch when the estimate rides in layer 0;
  failures  csi_pilot_classify of a +-1 matrix that is no Hadamard matrix and of an nt that is no power of two; csi_ls_estimate_device
            before csi_set_pilot.
The file stores every distinct log line once ("lines"), every distinct outcome once ("records": the four options, then the line numbers
of the log) and per case the number of its record.  All 58 instantiations the parent's plan can return are reached by the cases.
The count is taken from the recording against per-family numbers written out below, not from LS_KERNELS: a row added to the table later that no
option reaches would not fail here - whoever adds a row adds the case that reaches it."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden', 'ls_routes.json')

# the instantiations per family, as counted in the parent's plan (ls_ringb_shape / ls_plan of csi_mamimo.hip)
FAMILIES = {'ls_estimate_ringb_kernel': 24, 'ls_estimate_fwht2_kernel': 16, 'ls_estimate_ring_kernel': 7, 'ls_estimate_fwht_kernel': 4,
            'ls_estimate_chunked_kernel': 4, 'ls_estimate_kernel': 2, 'ls_despread_first_kernel': 1}

# the child process: argv = repository, mock library; prints the recording as one "RECORDING <json>" line
DRIVER = r'''
import ctypes, hashlib, json, sys
import numpy as np
REPO, SO = sys.argv[1], sys.argv[2]
sys.path.insert(0, REPO)
import dl_channel_estimation_mamimo_amd as pkg
from dl_channel_estimation_mamimo_amd import _lib
_lib._SO = SO
lib = _lib.load_library()
raw = ctypes.CDLL(SO)                      # the test-only entry points of tests/mock_library.cpp
raw.csi_mock_ls_log_read.restype = ctypes.c_int64
raw.csi_mock_ls_log_read.argtypes = [ctypes.c_char_p, ctypes.c_int64]
raw.csi_mock_ls_log_clear.restype = None
raw.csi_mock_pilot_buffer.restype = ctypes.c_int64
raw.csi_mock_pilot_buffer.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]

NTS = (8, 12, 16, 24, 32, 40, 48, 64, 96, 128, 160)
V2S = (-1, 0, 1, 2, 3, 4)
VHT4 = np.array([[1, -1, 1, 1], [1, 1, -1, 1], [1, 1, 1, -1], [-1, 1, 1, 1]], np.float32)


def pilots(nt):
    rng = np.random.default_rng(1000 + nt)
    pow2 = nt & (nt - 1) == 0
    out = {}
    if pow2:
        out['sylvester'] = pkg.synth.hadamard(nt)
    if pow2 and nt >= 16:
        out['vht'] = np.kron(pkg.synth.hadamard(nt // 4), VHT4).astype(np.float32)      # Hadamard-equivalent, not in the Sylvester order
    out['pm1'] = rng.choice(np.float32([-1, 1]), (nt, nt))                               # one bf16 piece
    out['two'] = (rng.choice(np.float32([-1, 1]), (nt, nt)) * (1 + rng.integers(0, 128, (nt, nt)) / 256)).astype(np.float32)      # 9 significant bits: two pieces
    out['floats'] = rng.standard_normal((nt, nt)).astype(np.float32)                    # three
    return out


lines, records = [], []


def intern(table, item):
    if item not in table:
        table.append(item)
    return table.index(item)


def read_log():
    need = raw.csi_mock_ls_log_read(None, 0)
    buf = ctypes.create_string_buffer(need)
    raw.csi_mock_ls_log_read(buf, need)
    return buf.value.decode().splitlines()


def ls_case(e, scratch, **options):
    """options in the order given (callers put ls_kernel last), 3 and 1100 packets; the record's number"""
    raw.csi_mock_ls_log_clear()
    for k, v in options.items():
        e.set_option(k, v)
    for npkt in (3, 1100):
        e.ls_estimate_device(scratch, scratch, npkt, scratch, scratch)
    log = read_log()
    first_launch = min(i for i, l in enumerate(log) if l.startswith('launch'))
    log = log[max(i for i in range(first_launch) if log[i].startswith('attr')):]
    rec = [e.get_option(k) for k in ('ls_mode', 'ls_per_cu', 'ls_pilot_fast', 'ls_pilot_pieces')] + [intern(lines, l) for l in log]
    return intern(records, rec)


out = {'grid': {}, 'sweep': {}, 'buffers': {}, 'estimate': {}, 'failures': {}}
for nt in NTS:
    for kind, P in pilots(nt).items():
        e = pkg.CsiEngine(nt, 1, hidden=(64, 64), n_out=52)
        scratch = e.empty((64,))
        e.set_pilot(P)
        sha = []
        for which in range(4):
            ptr = ctypes.c_void_p()
            n = raw.csi_mock_pilot_buffer(e._ctx, which, ctypes.byref(ptr))
            sha.append('%d:%s' % (n, hashlib.sha256(ctypes.string_at(ptr, n)).hexdigest() if n else ''))
        out['buffers']['%d/%s' % (nt, kind)] = sha
        out['grid']['%d/%s' % (nt, kind)] = [[ls_case(e, scratch, ls_v2=v2, ls_kernel=k) for v2 in V2S] for k in range(8)]
        e.set_option('ls_v2', 0)
        if nt <= 128 and kind != 'sylvester':
            fm_default, rm_default = e.get_option('ls_fft_first_max'), e.get_option('ls_ringb_min')
            out['sweep']['%d/%s' % (nt, kind)] = [[[[ls_case(e, scratch, ls_fast_perm=fp, ls_fft_first_max=fm, ls_ringb_min=rm, ls_kernel=k) for k in (0, 1, 5, 7)]
                                                    for rm in (0, 16, rm_default)] for fm in (0, fm_default, 64)] for fp in (0, 1)]
        e.close()

for nt in (16, 32, 64):
    for kind in ('sylvester', 'vht'):
        e = pkg.CsiEngine(nt, 1, hidden=(64, 64), n_out=52)
        w = pkg.synth.make_weights(np.random.default_rng(0), nt, (64, 64), n_out=52)
        e.load_weights('real', w); e.load_weights('imag', w); e.set_pilot(pilots(nt)[kind])
        x = e.to_device(np.zeros((1, 1, 320 * nt), np.float32))
        o_re, o_im, h_re, h_im = e.empty((1, 1, nt, 52)), e.empty((1, 1, nt, 52)), e.empty((1, 1, nt, 234)), e.empty((1, 1, nt, 234))
        for k in (0, 5):
            for v2 in (0, 1):
                for fused in (0, 1):
                    e.set_option('small_ls_fused', fused); e.set_option('ls_v2', v2); e.set_option('ls_kernel', k)
                    raw.csi_mock_ls_log_clear()
                    before = e.get_option('small_ls_launches')
                    e.estimate_device(x, x, 1, o_re, o_im, h_re, h_im)
                    e.synchronize()
                    out['estimate']['%d/%s/ls_kernel=%d/ls_v2=%d/small_ls_fused=%d' % (nt, kind, k, v2, fused)] = \
                        [e.get_option('small_ls_launches') - before] + [intern(lines, l) for l in read_log()]
        e.close()


def classify(P):
    P = np.ascontiguousarray(P, np.float32)
    a, b = np.full(P.shape[0], -7, np.int32), np.full(P.shape[0], -7, np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    rc = lib.csi_pilot_classify(P.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), P.shape[0], a.ctypes.data_as(i32p), b.ctypes.data_as(i32p))
    return [rc, bool((a == -7).all() and (b == -7).all())]      # return code; the tables untouched


notH = pkg.synth.hadamard(16).copy()
notH[5, 9] = -notH[5, 9]
out['failures']['classify: +-1, no Hadamard matrix'] = classify(notH)
out['failures']['classify: nt 12'] = classify(np.ones((12, 12)))
e = pkg.CsiEngine(16, 1, hidden=(64, 64), n_out=52)
scratch = e.empty((64,))
try:
    e.ls_estimate_device(scratch, scratch, 1, scratch, scratch)
    out['failures']['ls_estimate_device before set_pilot'] = [0, '']
except pkg.CsiError as err:
    out['failures']['ls_estimate_device before set_pilot'] = [err.code, str(err)]
e.close()
out['lines'], out['records'] = lines, records
print('RECORDING ' + json.dumps(out, separators=(',', ':')), flush=True)
'''


def _build_mock(repo, so):
    sys.path.insert(0, repo)
    from dl_channel_estimation_mamimo_amd import _lib
    _lib.build_band_kernel()
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    res = subprocess.run([hipcc, '--offload-arch=gfx950', '-O1', '-std=c++17', '-shared', '-fPIC', '-Wno-unused-value', '-pthread',
                          os.path.join(repo, 'tests', 'mock_library.cpp'), '-o', so], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert res.returncode == 0, res.stdout[-3000:]
    return so


def _run_driver(repo, so):
    env = {k: v for k, v in os.environ.items() if not k.startswith('CSI_')}
    run = subprocess.run([sys.executable, '-c', DRIVER, repo, so], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600, env=env)
    got = [l for l in run.stdout.splitlines() if l.startswith('RECORDING ')]
    assert run.returncode == 0 and got, run.stdout[-3000:]
    return json.loads(got[-1][len('RECORDING '):])


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def seen(tmp_path_factory):
    """every case on tests/mock_library.cpp (built as tests/test_band_routes_host.py builds it), in one child process"""
    return _run_driver(REPO, _build_mock(REPO, str(tmp_path_factory.mktemp('mocklib') / 'libcsi_mock.so')))


def _resolve(rec, table):
    """a record with its log lines written out"""
    opts, log = table['records'][rec][:4], [table['lines'][i] for i in table['records'][rec][4:]]
    return dict(zip(('ls_mode', 'ls_per_cu', 'ls_pilot_fast', 'ls_pilot_pieces'), opts), log=log)


def _flat(x):
    return [v for y in x for v in _flat(y)] if isinstance(x, list) else [x]


def test_the_recording_reaches_every_instantiation_of_the_plan(golden):
    """58 kernels in the launch lines of the recording, per family as counted in the parent's plan; every launch of an LS kernel of its own
    follows an attribute call for that kernel and those bytes (the fused layer-0 launch keeps its attribute per thread: it may not)."""
    launches = [l for l in golden['lines'] if l.startswith('launch')]
    names = {l.split(' kernel=')[1] for l in launches if ' kernel=ls_' in l}
    per_family = {f: sum(1 for n in names if n.split('<')[0].split('(')[0] == f) for f in FAMILIES}
    assert per_family == FAMILIES and len(names) == 58, (per_family, len(names))
    assert all(' attr=1 ' in l for l in launches if ' kernel=ls_' in l)
    # and the cases are the full grid
    assert len(golden['grid']) == 42 and all(len(g) == 8 and all(len(r) == 6 for r in g) for g in golden['grid'].values())
    assert len(golden['sweep']) == 34 and all(len(_flat(s)) == 72 for s in golden['sweep'].values())
    assert len(golden['estimate']) == 48 and len(golden['failures']) == 3


def test_every_ls_call_takes_the_kernel_and_launch_shape_of_the_recording(golden, seen):
    """ls_mode / ls_per_cu / ls_pilot_fast / ls_pilot_pieces, the attribute call of the last option and the two launches - kernel, grid,
    workgroup size, dynamic LDS bytes - of every case of the grid and of the sweep."""
    wrong = []
    for part in ('grid', 'sweep'):
        assert set(seen[part]) == set(golden[part])
        for key in golden[part]:
            want, got = _flat(golden[part][key]), _flat(seen[part][key])
            assert len(want) == len(got)
            wrong += [(part, key, i, _resolve(g, seen), _resolve(w, golden)) for i, (w, g) in enumerate(zip(want, got)) if _resolve(g, seen) != _resolve(w, golden)]
    assert not wrong, '%d cases differ, the first:\n' % len(wrong) + '\n'.join('%s %s #%d: got %s, recorded %s' % w for w in wrong[:5])


def test_set_pilot_uploads_the_recorded_bytes(golden, seen):
    """length and sha256 of P, its zero-padded copy, its bf16 pieces in MFMA operand order and the tables of the permuted Walsh-Hadamard
    kernel, per (nt, pilot class)"""
    assert seen['buffers'] == golden['buffers']


def test_one_packet_estimate_calls_take_the_recorded_ls_route(golden, seen):
    """csi_estimate_device of one packet: the LS estimate inside the layer-0 launch where the recording has it there, the LS kernel of its
    own (and no small_ls_launches) everywhere else"""
    def resolve(table):
        return {k: (v[0], [table['lines'][i] for i in v[1:]]) for k, v in table['estimate'].items()}
    got, want = resolve(seen), resolve(golden)
    assert got == want, [(k, got.get(k), want[k]) for k in want if got.get(k) != want[k]][:5]
    assert any(v[0] == 1 and 'small_l0_ls_kernel' in v[1][-1] for v in want.values()) and any(v[0] == 0 for v in want.values())


def test_the_failure_cases_return_the_recorded_codes_and_texts(golden, seen):
    assert seen['failures'] == golden['failures']
    assert golden['failures']['classify: +-1, no Hadamard matrix'] == [0, True] and golden['failures']['classify: nt 12'] == [0, True]
    code, text = golden['failures']['ls_estimate_device before set_pilot']
    assert code == -2 and 'csi_set_pilot has not been called' in text


if __name__ == '__main__':          # python tests/test_ls_routes_host.py <tree> <output file>: the recording of <tree> (see the module docstring)
    tree, target = os.path.abspath(sys.argv[1]), sys.argv[2]
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        rec = _run_driver(tree, _build_mock(tree, os.path.join(tmp, 'libcsi_mock.so')))
    with open(target, 'w') as f:
        json.dump(rec, f, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    print('%s: %d bytes, sha256 %s' % (target, os.path.getsize(target), hashlib.sha256(open(target, 'rb').read()).hexdigest()))
