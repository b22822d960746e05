"""Which band kernel serves a call, on a machine without a GPU.

The fused band kernel (first per-pair layer + regressor) exists in ten launchable forms - csi_band8 / csi_band4, split-f16 / bf16,
unsplit / column-split / without the staged streams - and the host picks one per call from the shape, the models in flight and five
options.  The launch counters of the library cannot tell the forms apart; the model of the HIP runtime can: tests/mock_hip.hpp hands
every module launch, with the name its function was looked up by, to tests/mock_library.cpp, which keeps one text line per band launch
(kernel name, grid, block, bytes of the argument record, M / N1 / nt of the record, tiled or plain weights, partial-sum buffer).

ROUTES below is that log per case, RECORDED ON THE DISPATCHER AS IT WAS BEFORE csrc/csi_band.hpp EXISTED: this file and the mock extension
were run on the csi_dnn_hs.hpp / csi_dnn_bf16.hpp of the parent of the change that introduced csi_band.hpp, and the output was pasted
here (to check it: restore that parent's csrc/ and include/ under these tests - both tests pass).  It is the contract a change of the
dispatcher keeps: same kernels, same grids, same records, same order.  Never re-record it from code under test.

All cases: n_out 52, zero input, f32_engine 1 on fp32 contexts, both component models (two streams unless small_call_overlap is 0) -
every case logs its per-model sequence twice.  Bands = ceil(npkt nr nt / 128).  Packet counts that differ from the first sketch of the
cases, because that sketch's count does not reach the named route on the old dispatcher:
  6   2208 packets (552 bands = 2 x 256 + 40), not 1184 (296 bands): a one-stream call of 257 ... 320 bands takes the automatic 2 splits
      (band8_splits), so the smallest call with full rounds AND a 40-band tail has two full rounds;
  10  128 packets (64 bands per model, 128 in flight), not 64 (32 bands, 64 in flight: 4 splits fit the 256 CUs, and 4 splits are
      always the 8-wave form);
  11  321 packets: 161 bands per model = 322 in flight, the first count beyond the 257 ... 320 window ('11/320' is its last);
  12  512 packets: nt 16 is outside the column-split small-call route of bf16 contexts, so the band kernel needs the 256 tiles of
      the fused pair kernel's regime (16 384 rows x 1024 columns);
  hook  the hooked name runs with band4 = 0, as the tools/*.sh that use the hook set it; with band4 = 1 the product's csi_band4 takes
      the staged unsplit launch in its place ('hook/band4=1').
One case more than the routes: 'load fails' - the code object does not load (the mock refuses it and keeps the error as the thread's last
HIP error, as the runtime does).  That is not fatal: no band launch, and the separate kernels serve the call without tripping over the
error the load left behind."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F16 = dict(dtype='f32', nt=16, nr=2, hidden=[256, 1024])
F16N = dict(F16, hidden=[128, 1024])
F32 = dict(dtype='f32', nt=32, nr=1, hidden=[256, 1024])
F8 = dict(dtype='f32', nt=8, nr=2, hidden=[256, 512])
B32 = dict(dtype='bf16', nt=32, nr=2, hidden=[256, 1024])
B32R1 = dict(B32, nr=1)
B16 = dict(dtype='bf16', nt=16, nr=2, hidden=[256, 1024])
HOOK = {'CSI_DEBUG_HOOKS': '1', 'CSI_BAND8_HSACO': os.devnull, 'CSI_BAND8_NAME': 'csi_band4_nopk'}


def _case(cid, ctx, npkt, env=None, **options):
    return dict(ctx, id=cid, npkt=npkt, options=options, env=env or {})


CASES = [
    _case('1', F16, 8), _case('2', F16, 160), _case('2/band4=0', F16, 160, band4=0), _case('3', F16, 700), _case('3/band4=0', F16, 700, band4=0),
    _case('4', F16, 8, band_split=1), _case('5', F16, 700, band_split=4),
    _case('6', F16N, 2208, small_call_overlap=0), _case('6/band_tail_split=0', F16N, 2208, small_call_overlap=0, band_tail_split=0),
    _case('6/band4=0', F16N, 2208, small_call_overlap=0, band4=0),
    _case('7', F32, 1360, small_call_overlap=0), _case('7/band4=0', F32, 1360, small_call_overlap=0, band4=0),
    _case('8', F8, 2100), _case('8b', F16, 700, hs_band=3),
    _case('9', B32, 4), _case('10', B32, 128), _case('10/band4=0', B32, 128, band4=0),
    _case('11/320', B32, 320), _case('11', B32, 321), _case('11/band4=0', B32, 321, band4=0), _case('11/tail', B32R1, 1360, small_call_overlap=0),
    _case('12', B16, 512, hs_band=2),
    _case('13/hs_band=0', F16, 700, hs_band=0), _case('13/hs_fuse_regressor=1', F16, 700, hs_fuse_regressor=1),
    _case('hook', F16, 700, env=HOOK, band4=0), _case('hook/band4=1', F16, 700, env=HOOK), _case('hook/2 splits', F16, 160, env=HOOK, band4=0),
    _case('hook/tail', F32, 1360, env=HOOK, small_call_overlap=0, band4=0),
    _case('load fails', F16, 700, env={'MOCK_HIP_FAIL_MODULE_LOAD': '1'}), _case('load fails/bf16', B32, 321, env={'MOCK_HIP_FAIL_MODULE_LOAD': '1'}),
]

# case -> ((band_launches, band_split_launches, band_tail_launches) the call added, the launches of ONE component model in order)
ROUTES = {
    '1': ((2, 2, 0), ['csi_band8_cs grid=2,4 block=512 bytes=144 M=256 N1=256 nt=16 tiled=0 part=1']),
    '2': ((2, 2, 0), ['csi_band4_cs grid=40,2 block=256 bytes=144 M=5120 N1=512 nt=16 tiled=1 part=1']),
    '2/band4=0': ((2, 2, 0), ['csi_band8_cs grid=40,2 block=512 bytes=144 M=5120 N1=512 nt=16 tiled=0 part=1']),
    '3': ((2, 0, 0), ['csi_band4 grid=175,1 block=256 bytes=128 M=22400 N1=1024 nt=16 tiled=1']),
    '3/band4=0': ((2, 0, 0), ['csi_band8 grid=175,1 block=512 bytes=128 M=22400 N1=1024 nt=16 tiled=0']),
    '4': ((2, 0, 0), ['csi_band4 grid=2,1 block=256 bytes=128 M=256 N1=1024 nt=16 tiled=1']),
    '5': ((2, 2, 0), ['csi_band8_cs grid=175,4 block=512 bytes=144 M=22400 N1=256 nt=16 tiled=0 part=1']),
    '6': ((4, 2, 2), ['csi_band4 grid=512,1 block=256 bytes=128 M=65536 N1=1024 nt=16 tiled=1',
                      'csi_band8_cs grid=40,4 block=512 bytes=144 M=5120 N1=256 nt=16 tiled=0 part=1']),
    '6/band_tail_split=0': ((2, 0, 0), ['csi_band4 grid=552,1 block=256 bytes=128 M=70656 N1=1024 nt=16 tiled=1']),
    '6/band4=0': ((4, 2, 2), ['csi_band8 grid=512,1 block=512 bytes=128 M=65536 N1=1024 nt=16 tiled=0',
                              'csi_band8_cs grid=40,4 block=512 bytes=144 M=5120 N1=256 nt=16 tiled=0 part=1']),
    '7': ((4, 2, 2), ['csi_band4 grid=256,1 block=256 bytes=128 M=32768 N1=1024 nt=32 tiled=1',
                      'csi_band4_cs grid=84,2 block=256 bytes=144 M=10752 N1=512 nt=32 tiled=1 part=1']),
    '7/band4=0': ((4, 2, 2), ['csi_band8 grid=256,1 block=512 bytes=128 M=32768 N1=1024 nt=32 tiled=0',
                              'csi_band8_cs grid=84,2 block=512 bytes=144 M=10752 N1=512 nt=32 tiled=0 part=1']),
    '8': ((2, 0, 0), ['csi_band8_nostage grid=263,1 block=512 bytes=128 M=33600 N1=512 nt=8 tiled=0']),
    '8b': ((2, 0, 0), ['csi_band8_nostage grid=175,1 block=512 bytes=128 M=22400 N1=1024 nt=16 tiled=0']),
    '9': ((2, 2, 0), ['csi_band8_bf16_cs grid=2,4 block=512 bytes=144 M=256 N1=256 nt=32 tiled=0 part=1']),
    '10': ((2, 2, 0), ['csi_band4_bf16_cs grid=64,2 block=256 bytes=144 M=8192 N1=512 nt=32 tiled=1 part=1']),
    '10/band4=0': ((2, 2, 0), ['csi_band8_bf16_cs grid=64,2 block=512 bytes=144 M=8192 N1=512 nt=32 tiled=0 part=1']),
    '11/320': ((2, 2, 0), ['csi_band4_bf16_cs grid=160,2 block=256 bytes=144 M=20480 N1=512 nt=32 tiled=1 part=1']),
    '11': ((2, 0, 0), ['csi_band4_bf16 grid=161,1 block=256 bytes=128 M=20544 N1=1024 nt=32 tiled=1']),
    '11/band4=0': ((2, 0, 0), ['csi_band8_bf16 grid=161,1 block=512 bytes=128 M=20544 N1=1024 nt=32 tiled=0']),
    '11/tail': ((2, 0, 0), ['csi_band4_bf16 grid=340,1 block=256 bytes=128 M=43520 N1=1024 nt=32 tiled=1']),      # (case 7's 340 bands: never a tail launch)
    '12': ((2, 0, 0), ['csi_band8_bf16_nostage grid=128,1 block=512 bytes=128 M=16384 N1=1024 nt=16 tiled=0']),
    '13/hs_band=0': ((0, 0, 0), []),
    '13/hs_fuse_regressor=1': ((0, 0, 0), []),
    'hook': ((2, 0, 0), ['csi_band4_nopk grid=175,1 block=256 bytes=128 M=22400 N1=1024 nt=16 tiled=1']),
    'hook/band4=1': ((2, 0, 0), ['csi_band4 grid=175,1 block=256 bytes=128 M=22400 N1=1024 nt=16 tiled=1']),
    'hook/2 splits': ((2, 2, 0), ['csi_band8_cs grid=40,2 block=512 bytes=144 M=5120 N1=512 nt=16 tiled=0 part=1']),
    'hook/tail': ((4, 2, 2), ['csi_band4_nopk grid=256,1 block=256 bytes=128 M=32768 N1=1024 nt=32 tiled=1',
                              'csi_band8_cs grid=84,2 block=512 bytes=144 M=10752 N1=512 nt=32 tiled=0 part=1']),
    'load fails': ((0, 0, 0), []),
    'load fails/bf16': ((0, 0, 0), []),
}

PRODUCT_KERNELS = {'csi_band8', 'csi_band8_cs', 'csi_band8_nostage', 'csi_band8_bf16', 'csi_band8_bf16_cs', 'csi_band8_bf16_nostage',
                   'csi_band4', 'csi_band4_cs', 'csi_band4_bf16', 'csi_band4_bf16_cs'}

# the child process: argv = repository, mock library, the cases as JSON; prints one "ROUTE <id> <json>" line per case
DRIVER = r'''
import ctypes, json, os, sys
import numpy as np
REPO, SO, CASES = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
sys.path.insert(0, REPO)
import dl_channel_estimation_mamimo_amd as pkg
from dl_channel_estimation_mamimo_amd import _lib
_lib._SO = SO
_lib.load_library()
raw = ctypes.CDLL(SO)                      # the two test-only entry points of tests/mock_library.cpp
raw.csi_mock_band_log_read.restype = ctypes.c_int64
raw.csi_mock_band_log_read.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]
raw.csi_mock_band_log_clear.restype = None
COUNTERS = ('band_launches', 'band_split_launches', 'band_tail_launches')
engines = {}


def engine(case):
    # one context per shape - and per environment: the debug hooks are read when a context first loads the code object
    key = (case['dtype'], case['nt'], case['nr'], tuple(case['hidden']), tuple(sorted(case['env'].items())))
    if key not in engines:
        e = pkg.CsiEngine(case['nt'], case['nr'], hidden=tuple(case['hidden']), n_out=52, dtype=case['dtype'])
        w = pkg.synth.make_weights(np.random.default_rng(0), case['nt'], tuple(case['hidden']), n_out=52)
        e.load_weights('real', w); e.load_weights('imag', w); e.set_pilot(pkg.synth.hadamard(case['nt']))
        engines[key] = (e, {})
    return engines[key]


for case in CASES:
    os.environ.update(case['env'])
    e, defaults = engine(case)
    opts = dict(case['options'])
    if case['dtype'] == 'f32':
        opts.setdefault('f32_engine', 1)
    for k in opts:
        defaults.setdefault(k, e.get_option(k))
    for k, v in defaults.items():           # every option an earlier case of this context touched goes back to its default
        e.set_option(k, opts.get(k, v))
    npkt, nt, nr = case['npkt'], case['nt'], case['nr']
    x = e.to_device(np.zeros((npkt, nr, 320 * nt), np.float32))
    o_re, o_im = e.empty((npkt, nr, nt, 52)), e.empty((npkt, nr, nt, 52))
    raw.csi_mock_band_log_clear()
    before = [e.get_option(k) for k in COUNTERS]
    e.predict_device(x, x, npkt, o_re, o_im)
    e.synchronize()
    need = raw.csi_mock_band_log_read(e._ctx, None, 0)
    buf = ctypes.create_string_buffer(need)
    raw.csi_mock_band_log_read(e._ctx, buf, need)
    print('ROUTE %s %s' % (case['id'], json.dumps({'launches': buf.value.decode().splitlines(),
                                                   'counters': [e.get_option(k) - b for k, b in zip(COUNTERS, before)]})), flush=True)
    del x, o_re, o_im
    for k in case['env']:
        del os.environ[k]
print('band routes: done')
'''


@pytest.fixture(scope='module')
def mock_so(tmp_path_factory):
    """tests/mock_library.cpp built as tests/test_host_round4.py builds it, after the band kernels' code object (band8_hsaco.inc: a build without
    it has no band route to log)."""
    sys.path.insert(0, REPO)
    from dl_channel_estimation_mamimo_amd import _lib
    _lib.build_band_kernel()
    so = str(tmp_path_factory.mktemp('mocklib') / 'libcsi_mock.so')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    res = subprocess.run([hipcc, '--offload-arch=gfx950', '-O1', '-std=c++17', '-shared', '-fPIC', '-Wno-unused-value', '-pthread',
                          os.path.join(REPO, 'tests', 'mock_library.cpp'), '-o', so], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert res.returncode == 0, res.stdout[-3000:]
    return so


def test_the_route_table_names_every_product_kernel():
    named = {line.split()[0] for _, seq in ROUTES.values() for line in seq}
    assert PRODUCT_KERNELS <= named, sorted(PRODUCT_KERNELS - named)
    assert {c['id'] for c in CASES} == set(ROUTES)
    assert all(seq for cid, (_, seq) in ROUTES.items() if not cid.startswith(('13', 'load fails')))


def test_every_call_takes_the_band_kernel_the_table_names(mock_so):
    """csi_predict_device of every case on the mock runtime, in one child process: the band launches it logs and the three launch counters
    are those of ROUTES - kernel name, grid, workgroup size, record size, M / N1 / nt of the record, tiled or plain weights - per component
    model, in order."""
    env = {k: v for k, v in os.environ.items() if not k.startswith('CSI_')}
    run = subprocess.run([sys.executable, '-c', DRIVER, REPO, mock_so, json.dumps(CASES)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, timeout=600, env=env)
    print(run.stdout[-20000:])
    assert run.returncode == 0 and 'band routes: done' in run.stdout, run.stdout[-3000:]
    seen = {}
    for line in run.stdout.splitlines():
        if line.startswith('ROUTE '):
            cid, _, text = line[6:].partition(' {')
            seen[cid] = json.loads('{' + text)
    wrong = []
    for case in CASES:
        counters, per_model = ROUTES[case['id']]
        got = seen.get(case['id'])
        if got is None or got['launches'] != per_model * 2 or tuple(got['counters']) != counters:
            wrong.append((case['id'], got, per_model * 2, counters))
    assert not wrong, '\n'.join('case %s: logged %s, recorded %s %s' % w for w in wrong)
