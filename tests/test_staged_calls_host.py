"""What the staged host entry points do to the HIP runtime, call by call - on a machine without a GPU.

Seven entry points take host pointers and run their device form over packets (links, for the metric) in chunks through the context's staging
buffer: csi_lmmse_estimate, csi_lmmse_blind, csi_nmse, csi_hybrid_weights, csi_subspace_smooth, csi_beam_smooth and csi_beam_wiener.  What
they ask of the runtime is their contract: the size of the staging buffer, where each plane lies in it, which bytes of which host array go up
and come down per chunk and in which order, the launches between them, and the synchronisations.  The model of the HIP runtime can see all
of it: tests/mock_hip.hpp hands every hipMalloc, hipMemcpyAsync / hipMemcpy, hipLaunchKernel and hipStreamSynchronize to
tests/mock_library.cpp, which keeps one text line per event while a context is named -
  malloc bytes=<requested>
  copy H2D|D2H bytes=<> dev=<context buffer>+<offset> host=<the caller's array>+<offset>
  launch grid=<x>,<y>,<z> block=<x>,<y>,<z> lds=<dynamic bytes> kernel=<demangled name>
  sync
(a device address is named by the context's buffer that holds it - stage, skbuf, lmb_ws, hyb_ws, beam_ws, sub_q, beam_a -, a host address
by the array this file handed over; "local" is a variable of the library's own).

tests/golden/staged_calls.json is that log per case, RECORDED ON THE HOST CODE AS IT WAS BEFORE csrc/csi_stage.hpp EXISTED: this file, the
mock extension and the log were run on the csrc/ and include/ of the parent of the change that introduced csi_stage.hpp - six hand-written
chunk loops in csi_mamimo.hip, csi_hybrid.hpp, csi_subspace.hpp and csi_beam.hpp - by
`python tests/test_staged_calls_host.py <tree with that csrc/> <output file>`.  It is the contract a change of the staging code keeps.  Never
re-record it from code under test.  To check it: restore that parent's csrc/ and include/ under these tests - all of them pass.

Cases (fp32 contexts, a fresh one per call of a host entry point, so that the first line of its log is the allocation of the staging buffer;
all inputs zero - the mock drops the launches):
  one chunk   nt 8, nr 2, a few packets, every optional pointer present and absent: noise_var / corr of csi_lmmse_blind, w of the two
              smoothers, w_out of csi_beam_wiener, and all 16 combinations of eval_*, n_atoms, gain and frf_mean_* of csi_hybrid_weights;
  two chunks  a short last chunk.  The smoothers on a context whose workspace_bytes holds two packets, five packets.  The other four chunk
              on 256 MiB alone: nt 128, nr 16 stages 35 packets (34 of csi_hybrid_weights), so 37 (36) packets; csi_nmse at 2^22 bins stages
              4 links, so 5 links;
  device      the device forms whose host side moved with the staging code (csi_lmmse_estimate_device, csi_lmmse_blind_device,
              csi_null_noise_device), the two *_set_basis calls, and an in-place call of each smoother's device form;
  refusals    code and csi_last_error text of every refusal of these entry points, of their device forms' own checks (alignment, overlap of
              the planes) and of the two *_set_basis calls.  Addresses in a text are replaced by <ptr>.
Not covered: csi_lmmse_estimate on a context with nt = 0 divides by the packet size before the device form refuses the context; the case
is left out.
The file stores every distinct log line once ("lines") and per case the return code, the error text, the three launch counters
(hybrid_launches, subspace_launches, beam_launches) and the line numbers of the log."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden', 'staged_calls.json')

ENTRY_POINTS = ('csi_lmmse_estimate', 'csi_lmmse_blind', 'csi_nmse', 'csi_hybrid_weights', 'csi_subspace_smooth', 'csi_beam_smooth', 'csi_beam_wiener')
SMOOTHERS = ('csi_subspace_smooth', 'csi_beam_smooth', 'csi_beam_wiener')          # their two-chunk case has three chunks: 2 + 2 + 1 packets

# the child process: argv = repository, mock library; prints the recording as one "RECORDING <json>" line
DRIVER = r'''
import ctypes, itertools, json, re, sys
import numpy as np
REPO, SO = sys.argv[1], sys.argv[2]
sys.path.insert(0, REPO)
import dl_channel_estimation_mamimo_amd as pkg
from dl_channel_estimation_mamimo_amd import _lib
_lib._SO = SO
lib = _lib.load_library()
raw = ctypes.CDLL(SO)                      # the test-only entry points of tests/mock_library.cpp
raw.csi_mock_stage_log_read.restype = ctypes.c_int64
raw.csi_mock_stage_log_read.argtypes = [ctypes.c_char_p, ctypes.c_int64]
raw.csi_mock_stage_log_clear.restype = None
raw.csi_mock_stage_log_clear.argtypes = [ctypes.c_void_p]
raw.csi_mock_stage_log_name.restype = None
raw.csi_mock_stage_log_name.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int64]

N = 234
lines, out = [], {}


def zeros(shape, dtype=np.float32):
    """zeroed, on a 64-byte boundary (the device forms take these arrays as device planes on the mock)"""
    n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    buf = np.zeros(n + 64, np.uint8)
    off = -buf.ctypes.data % 64
    return buf[off:off + n].view(dtype).reshape(shape)


class Raw:
    """an address handed over as it is (a misaligned plane)"""
    def __init__(self, addr):
        self.addr = addr


def engine(nt=8, nr=2, **kw):
    return pkg.CsiEngine(nt, nr, hidden=(8,), **kw)


def trace(key, e, fn, *args):
    """args: scalars, None, Raw, or (name, array) - the array is named in the log.  Keeps return code, error text, counters and log."""
    f = getattr(lib, fn)
    call = [e._ctx]
    for a, t in zip(args, f.argtypes[1:]):
        if isinstance(a, tuple):
            raw.csi_mock_stage_log_name(a[0].encode(), a[1].ctypes.data, a[1].nbytes)
            a = Raw(a[1].ctypes.data)
        call.append(ctypes.cast(ctypes.c_void_p(a.addr), t) if isinstance(a, Raw) else a)
    assert len(call) == len(f.argtypes), fn
    raw.csi_mock_stage_log_clear(e._ctx)
    rc = f(*call)
    need = raw.csi_mock_stage_log_read(None, 0)
    buf = ctypes.create_string_buffer(need)
    raw.csi_mock_stage_log_read(buf, need)
    raw.csi_mock_stage_log_clear(None)
    raw.csi_mock_stage_log_name(None, None, 0)
    log = []
    for l in buf.value.decode().splitlines():
        if l not in lines:
            lines.append(l)
        log.append(lines.index(l))
    err = re.sub(r'0x[0-9a-f]+|\(nil\)', '<ptr>', (lib.csi_last_error(e._ctx) or b'').decode()) if rc else ''
    assert key not in out, key
    out[key] = [rc, err, [e.get_option(k) for k in ('hybrid_launches', 'subspace_launches', 'beam_launches')], log]
    return rc


def planes(npkt, nr, nt, *names):
    return [(n, zeros((npkt, nr, nt, N))) for n in names]


# ---------------------------------------------------------------- csi_lmmse_estimate
def lmmse_estimate(key, nt, nr, npkt, L=8):
    e = engine(nt, nr)
    h_re, h_im, out_re, out_im = planes(npkt, nr, nt, 'h_re', 'h_im', 'out_re', 'out_im')
    trace(key, e, 'csi_lmmse_estimate', h_re, h_im, npkt, ('hvec', zeros((npkt, L))), L, ('snr_db', zeros((npkt, nr))), out_re, out_im)
    e.close()


lmmse_estimate('csi_lmmse_estimate/one chunk', 8, 2, 3)
lmmse_estimate('csi_lmmse_estimate/two chunks', 128, 16, 37)


# ---------------------------------------------------------------- csi_lmmse_blind
def lmmse_blind(key, nt, nr, npkt, nv, corr, fn='csi_lmmse_blind'):
    e = engine(nt, nr)
    ltf = [(n, zeros((npkt, nr, 320 * nt))) for n in ('ltf_re', 'ltf_im')]
    h_re, h_im, out_re, out_im = planes(npkt, nr, nt, 'h_re', 'h_im', 'out_re', 'out_im')
    trace(key, e, fn, ltf[0], ltf[1], h_re, h_im, npkt, out_re, out_im,
          ('noise_var', zeros((npkt, nr), np.float64)) if nv else None, ('corr', zeros((npkt, nr, N, 2), np.float64)) if corr else None)
    e.close()


for nv, corr in itertools.product((0, 1), (0, 1)):
    lmmse_blind('csi_lmmse_blind/one chunk/noise_var=%d/corr=%d' % (nv, corr), 8, 2, 3, nv, corr)
    lmmse_blind('csi_lmmse_blind_device/noise_var=%d/corr=%d' % (nv, corr), 8, 2, 3, nv, corr, fn='csi_lmmse_blind_device')
lmmse_blind('csi_lmmse_blind/two chunks/noise_var=1/corr=1', 128, 16, 37, 1, 1)


# ---------------------------------------------------------------- csi_nmse
def nmse(key, nlinks, n_bins):
    e = engine()
    p = [(n, zeros((nlinks, n_bins))) for n in ('ref_re', 'ref_im', 'est_re', 'est_im')]
    mean = ctypes.c_double(0.0)
    trace(key, e, 'csi_nmse', p[0], p[1], p[2], p[3], nlinks, n_bins, ctypes.byref(mean))
    e.close()


nmse('csi_nmse/one chunk', 10, N)
nmse('csi_nmse/two chunks', 5, 1 << 22)


# ---------------------------------------------------------------- csi_hybrid_weights
def dictionary(e, nt, rays=4):
    d = np.zeros((nt, rays), np.float32)
    assert lib.csi_hybrid_set_dictionary(e._ctx, d.ctypes.data_as(_lib._fp), d.ctypes.data_as(_lib._fp), rays) == 0


def hybrid(key, nt, nr, npkt, ns, ntrf, ev, na, gain, mean):
    e = engine(nt, nr)
    dictionary(e, nt)
    h_re, h_im, e_re, e_im = planes(npkt, nr, nt, 'h_re', 'h_im', 'eval_re', 'eval_im')
    trace(key, e, 'csi_hybrid_weights', h_re, h_im, e_re if ev else None, e_im if ev else None, npkt, ns, ntrf, ctypes.c_float(0.0),
          ('fbb_re', zeros((npkt, N, ns, ntrf))), ('fbb_im', zeros((npkt, N, ns, ntrf))), ('idx', zeros((npkt, N, ntrf), np.int32)),
          ('n_atoms', zeros((npkt, N), np.int32)) if na else None, ('gain', zeros((npkt, N))) if gain else None,
          ('frf_mean_re', zeros((npkt, ntrf, nt))) if mean else None, ('frf_mean_im', zeros((npkt, ntrf, nt))) if mean else None)
    e.close()


for ev, na, gain, mean in itertools.product((0, 1), repeat=4):
    hybrid('csi_hybrid_weights/one chunk/eval=%d/n_atoms=%d/gain=%d/frf_mean=%d' % (ev, na, gain, mean), 8, 2, 2, 1, 2, ev, na, gain, mean)
hybrid('csi_hybrid_weights/two chunks/eval=1/n_atoms=1/gain=1/frf_mean=1', 128, 16, 36, 1, 1, 1, 1, 1, 1)


# ---------------------------------------------------------------- the two smoothers
TWO_PACKETS = 150000          # workspace_bytes: two packets of four planes at nt 8, nr 2 (59904 bytes each)


def basis(rows, cols):
    return np.ascontiguousarray(np.eye(rows, cols, dtype=np.float32)), np.zeros((rows, cols), np.float32)


def set_basis(e, fn, rows, cols):
    q_re, q_im = basis(rows, cols)
    assert getattr(lib, fn)(e._ctx, q_re.ctypes.data_as(_lib._fp), q_im.ctypes.data_as(_lib._fp), cols) == 0


def subspace(key, npkt, w, rank=5, fn='csi_subspace_smooth', inplace=False, **kw):
    e = engine(**kw)
    set_basis(e, 'csi_subspace_set_basis', N, rank)
    h_re, h_im, out_re, out_im = planes(npkt, 2, 8, 'h_re', 'h_im', 'out_re', 'out_im')
    trace(key, e, fn, h_re, h_im, npkt, ('w', zeros((npkt, 2, rank))) if w else None, h_re if inplace else out_re, h_im if inplace else out_im)
    e.close()


def beam(key, npkt, w, nb=3, fn='csi_beam_smooth', inplace=False, **kw):
    """w: the weights of csi_beam_smooth, w_out of csi_beam_wiener"""
    e = engine(**kw)
    set_basis(e, 'csi_beam_set_basis', 8, nb)
    h_re, h_im, out_re, out_im = planes(npkt, 2, 8, 'h_re', 'h_im', 'out_re', 'out_im')
    o = (h_re if inplace else out_re, h_im if inplace else out_im)
    if 'wiener' in fn:
        trace(key, e, fn, h_re, h_im, npkt, ('err_var', zeros((npkt, 2))), o[0], o[1], ('w_out', zeros((npkt, 2, nb))) if w else None)
    else:
        trace(key, e, fn, h_re, h_im, npkt, ('w', zeros((npkt, 2, nb))) if w else None, o[0], o[1])
    e.close()


for w in (0, 1):
    subspace('csi_subspace_smooth/one chunk/w=%d' % w, 3, w)
    beam('csi_beam_smooth/one chunk/w=%d' % w, 3, w)
    beam('csi_beam_wiener/one chunk/w_out=%d' % w, 3, w, fn='csi_beam_wiener')
subspace('csi_subspace_smooth/two chunks/w=1', 5, 1, workspace_bytes=TWO_PACKETS)
beam('csi_beam_smooth/two chunks/w=1', 5, 1, workspace_bytes=TWO_PACKETS)
beam('csi_beam_wiener/two chunks/w_out=1', 5, 1, fn='csi_beam_wiener', workspace_bytes=TWO_PACKETS)
subspace('csi_subspace_smooth_device/in place', 3, 1, fn='csi_subspace_smooth_device', inplace=True)
beam('csi_beam_smooth_device/in place', 3, 1, fn='csi_beam_smooth_device', inplace=True)
beam('csi_beam_wiener_device/in place', 3, 1, fn='csi_beam_wiener_device', inplace=True)

# ---------------------------------------------------------------- device forms and *_set_basis
e = engine()
h_re, h_im, out_re, out_im = planes(3, 2, 8, 'h_re', 'h_im', 'out_re', 'out_im')
ltf_re, ltf_im = [(n, zeros((3, 2, 320 * 8))) for n in ('ltf_re', 'ltf_im')]
hvec, snr, nv = ('hvec', zeros((3, 8))), ('snr_db', zeros((3, 2))), ('noise_var', zeros((3, 2), np.float64))
trace('csi_lmmse_estimate_device', e, 'csi_lmmse_estimate_device', h_re, h_im, 3, hvec, 8, snr, out_re, out_im)
trace('csi_null_noise_device', e, 'csi_null_noise_device', ltf_re, ltf_im, 3, nv)
q = [(n, a) for n, a in zip(('q_re', 'q_im'), basis(N, 5))]
a = [(n, a) for n, a in zip(('a_re', 'a_im'), basis(8, 3))]
trace('csi_subspace_set_basis', e, 'csi_subspace_set_basis', q[0], q[1], 5)
trace('csi_subspace_set_basis/again', e, 'csi_subspace_set_basis', q[0], q[1], 5)
trace('csi_beam_set_basis', e, 'csi_beam_set_basis', a[0], a[1], 3)
trace('csi_beam_set_basis/again', e, 'csi_beam_set_basis', a[0], a[1], 3)
e.close()

# ---------------------------------------------------------------- refusals
def off(p, nbytes):
    return Raw(p[1].ctypes.data + nbytes)


mean = ctypes.byref(ctypes.c_double(0.0))
w5, w3, ev = ('w', zeros((3, 2, 5))), ('w', zeros((3, 2, 3))), ('err_var', zeros((3, 2)))
power = ('power', zeros((3, 2, 3)))
fbb_re, fbb_im, idx = ('fbb_re', zeros((3, N, 1, 2))), ('fbb_im', zeros((3, N, 1, 2))), ('idx', zeros((3, N, 2), np.int32))
zf = ctypes.c_float(0.0)


def hyb_args(npkt=3, ns=1, ntrf=2, h=h_re, e_re=None, e_im=None, m_re=None, m_im=None):
    return (h, h_im, e_re, e_im, npkt, ns, ntrf, zf, fbb_re, fbb_im, idx, None, None, m_re, m_im)


def common_refusals(tag, e):
    """what a context refuses whatever its state: null pointers and bad counts"""
    R = lambda name, fn, *args: trace('refusal/%s/%s/%s' % (tag, fn, name), e, fn, *args)
    R('null h_re', 'csi_lmmse_estimate', None, h_im, 3, hvec, 8, snr, out_re, out_im)
    R('null out_im', 'csi_lmmse_estimate', h_re, h_im, 3, hvec, 8, snr, out_re, None)
    R('npkt -1', 'csi_lmmse_estimate', h_re, h_im, -1, hvec, 8, snr, out_re, out_im)
    R('L 0', 'csi_lmmse_estimate', h_re, h_im, 3, hvec, 0, snr, out_re, out_im)
    R('null d_hvec', 'csi_lmmse_estimate_device', h_re, h_im, 3, None, 8, snr, out_re, out_im)
    for fn in ('csi_lmmse_blind', 'csi_lmmse_blind_device'):
        R('null ltf_im', fn, ltf_re, None, h_re, h_im, 3, out_re, out_im, None, None)
        R('npkt 0', fn, ltf_re, ltf_im, h_re, h_im, 0, out_re, out_im, None, None)
        R('npkt -1', fn, ltf_re, ltf_im, h_re, h_im, -1, out_re, out_im, None, None)
    R('null noise_var', 'csi_null_noise_device', ltf_re, ltf_im, 3, None)
    R('npkt -1', 'csi_null_noise_device', ltf_re, ltf_im, -1, nv)
    R('null est_im', 'csi_nmse', h_re, h_im, out_re, None, 10, N, mean)
    R('null mean', 'csi_nmse', h_re, h_im, out_re, out_im, 10, N, None)
    R('nlinks 0', 'csi_nmse', h_re, h_im, out_re, out_im, 0, N, mean)
    R('n_bins 0', 'csi_nmse', h_re, h_im, out_re, out_im, 10, 0, mean)
    for fn in ('csi_hybrid_weights', 'csi_hybrid_weights_device'):
        R('npkt -1', fn, *hyb_args(npkt=-1))
        R('ntrf 0', fn, *hyb_args(ntrf=0))
        R('ns 3', fn, *hyb_args(ns=3))
        R('null h_re', fn, *hyb_args(h=None))
        R('eval_re alone', fn, *hyb_args(e_re=out_re))
        R('frf_mean_im alone', fn, *hyb_args(m_im=('frf_mean_im', zeros((3, 2, 8)))))
    for fn in ('csi_subspace_smooth', 'csi_subspace_smooth_device', 'csi_beam_smooth', 'csi_beam_smooth_device'):
        w = w5 if 'subspace' in fn else w3
        R('npkt -1', fn, h_re, h_im, -1, w, out_re, out_im)
        R('null h_im', fn, h_re, None, 3, w, out_re, out_im)
        R('null out_re', fn, h_re, h_im, 3, w, None, out_im)
    for fn in ('csi_beam_wiener', 'csi_beam_wiener_device'):
        R('npkt -1', fn, h_re, h_im, -1, ev, out_re, out_im, None)
        R('null err_var', fn, h_re, h_im, 3, None, out_re, out_im, None)
        R('null out_im', fn, h_re, h_im, 3, ev, out_re, None, None)
    R('npkt -1', 'csi_beam_power_device', h_re, h_im, -1, power)
    R('null power', 'csi_beam_power_device', h_re, h_im, 3, None)
    return R


# a context without dictionary and bases
e = engine()
R = common_refusals('bare context', e)
R('no dictionary', 'csi_hybrid_weights', *hyb_args())
R('no dictionary', 'csi_hybrid_weights_device', *hyb_args())
for fn in ('csi_subspace_smooth', 'csi_subspace_smooth_device', 'csi_beam_smooth', 'csi_beam_smooth_device'):
    R('no basis', fn, h_re, h_im, 3, None, out_re, out_im)
for fn in ('csi_beam_wiener', 'csi_beam_wiener_device'):
    R('no basis', fn, h_re, h_im, 3, ev, out_re, out_im, None)
R('no basis', 'csi_beam_power_device', h_re, h_im, 3, power)
# the two *_set_basis calls
for fn, rows, cols, names in (('csi_subspace_set_basis', N, 5, ('q_re', 'q_im')), ('csi_beam_set_basis', 8, 3, ('a_re', 'a_im'))):
    b_re, b_im = basis(rows, cols)
    B = lambda re, im: [(names[0], re), (names[1], im)]
    R('rank 0', fn, *B(b_re, b_im), 0)
    R('rank 129', fn, *B(*basis(rows, 129)), 129)
    R('null re', fn, None, (names[1], b_im), cols)
    R('null im', fn, (names[0], b_re), None, cols)
    bad = b_im.copy(); bad[rows - 1, 1] = np.inf
    R('non-finite im', fn, *B(b_re, bad), cols)
    bad = b_re.copy(); bad[2, 4 % cols] = np.nan
    R('non-finite re', fn, *B(bad, b_im), cols)
    bad = b_re.copy(); bad[1, 1] = 1.25
    R('column 1 too long', fn, *B(bad, b_im), cols)
    bad = b_re.copy(); bad[0, 2] = 0.5; bad[2, 2] = np.sqrt(0.75)
    R('columns 0 and 2 not orthogonal', fn, *B(bad, b_im), cols)
    bad = b_im.copy(); bad[1, 2] = 0.00015
    R('just over the tolerance', fn, *B(b_re, bad), cols)
e.close()
e = engine(132, 1)
R = lambda name, fn, *args: trace('refusal/nt 132/%s/%s' % (fn, name), e, fn, *args)
b_re, b_im = basis(132, 3)
R('more than 128 antennas', 'csi_beam_set_basis', ('a_re', b_re), ('a_im', b_im), 3)
e.close()

# a context with everything set: the device forms' own checks
e = engine()
dictionary(e, 8)
set_basis(e, 'csi_subspace_set_basis', N, 5)
set_basis(e, 'csi_beam_set_basis', 8, 3)
R = common_refusals('ready context', e)
R('ntrf 5 of 4 rays', 'csi_hybrid_weights', *hyb_args(ntrf=5))
R('misaligned d_h_re', 'csi_lmmse_estimate_device', off(h_re, 4), h_im, 2, hvec, 8, snr, out_re, out_im)
R('misaligned d_ltf_im', 'csi_lmmse_blind_device', ltf_re, off(ltf_im, 8), h_re, h_im, 2, out_re, out_im, None, None)
R('misaligned d_noise_var', 'csi_lmmse_blind_device', ltf_re, ltf_im, h_re, h_im, 2, out_re, out_im, off(nv, 4), None)
R('misaligned d_ltf_re', 'csi_null_noise_device', off(ltf_re, 4), ltf_im, 2, nv)
R('misaligned d_noise_var', 'csi_null_noise_device', ltf_re, ltf_im, 2, off(nv, 4))
R('misaligned d_eval_re', 'csi_hybrid_weights_device', *hyb_args(npkt=2, e_re=off(out_re, 4), e_im=out_im))
R('misaligned d_power', 'csi_beam_power_device', h_re, h_im, 3, off(power, 2))
R('misaligned d_h_im', 'csi_beam_power_device', h_re, off(h_im, 4), 2, power)
plane = 3 * 2 * 8 * N * 4
for fn in ('csi_subspace_smooth_device', 'csi_beam_smooth_device', 'csi_beam_wiener_device'):
    third = ev if 'wiener' in fn else (w5 if 'subspace' in fn else w3)
    tail = (None,) if 'wiener' in fn else ()
    S = lambda name, npkt, i_re, i_im, o_re, o_im, x=third: R(name, fn, i_re, i_im, npkt, x, o_re, o_im, *tail)
    S('misaligned d_out_re', 2, h_re, h_im, off(out_re, 4), out_im)
    S('misaligned d_h_im', 2, h_re, off(h_im, 8), out_re, out_im)
    S('misaligned ' + ('d_err_var' if 'wiener' in fn else 'd_w'), 3, h_re, h_im, out_re, out_im, off(third, 2))
    S('out_re is h_im', 3, h_re, h_im, h_im, out_im)
    S('out_im is h_re', 3, h_re, h_im, out_re, h_re)
    S('out_re is out_im', 3, h_re, h_im, out_re, out_re)
    S('out_re inside h_re', 2, h_re, h_im, off(h_re, 16), out_im)
    S('out_im ends inside h_im', 2, h_re, off(h_im, plane // 3), out_re, h_im)
    S('out_re ends on h_re', 1, off(h_re, plane // 3), h_im, h_re, out_im)          # shares no byte: accepted
R('misaligned d_w_out', 'csi_beam_wiener_device', h_re, h_im, 3, ev, out_re, out_im, off(w3, 2))
e.close()

# single-input contexts
e = pkg.CsiEngine(0, 2, hidden=(8,), len_ltf=320)
R = lambda fn, *args: trace('refusal/nt 0/%s' % fn, e, fn, *args)
R('csi_lmmse_estimate_device', h_re, h_im, 3, hvec, 8, snr, out_re, out_im)
R('csi_lmmse_blind', ltf_re, ltf_im, h_re, h_im, 3, out_re, out_im, None, None)
R('csi_lmmse_blind_device', ltf_re, ltf_im, h_re, h_im, 3, out_re, out_im, None, None)
R('csi_null_noise_device', ltf_re, ltf_im, 3, nv)
R('csi_hybrid_weights', *hyb_args())
R('csi_hybrid_weights_device', *hyb_args())
for fn in ('csi_subspace_smooth', 'csi_subspace_smooth_device', 'csi_beam_smooth', 'csi_beam_smooth_device'):
    R(fn, h_re, h_im, 3, None, out_re, out_im)
for fn in ('csi_beam_wiener', 'csi_beam_wiener_device'):
    R(fn, h_re, h_im, 3, ev, out_re, out_im, None)
R('csi_beam_power_device', h_re, h_im, 3, power)
R('csi_subspace_set_basis', q[0], q[1], 5)
R('csi_beam_set_basis', a[0], a[1], 3)
e.close()

print('RECORDING ' + json.dumps({'lines': lines, 'cases': out}, separators=(',', ':')), flush=True)
'''


def _build_mock(repo, so):
    sys.path.insert(0, repo)
    from dl_channel_estimation_mamimo_amd import _lib
    _lib.build_band_kernel()
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    res = subprocess.run([hipcc, '--offload-arch=gfx950', '-O1', '-std=c++17', '-shared', '-fPIC', '-Wno-unused-value', '-pthread',
                          os.path.join(repo, 'tests', 'mock_library.cpp'), '-o', so],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
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
    """every case on tests/mock_library.cpp (built as tests/test_ls_routes_host.py builds it), in one child process"""
    return _run_driver(REPO, _build_mock(REPO, str(tmp_path_factory.mktemp('mocklib') / 'libcsi_mock.so')))


def _resolve(table):
    """every case with its log lines written out"""
    return {k: dict(rc=v[0], err=v[1], counters=v[2], log=[table['lines'][i] for i in v[3]]) for k, v in table['cases'].items()}


def _traced(table):
    return {k: v for k, v in _resolve(table).items() if not k.startswith('refusal/')}


def test_the_recording_holds_the_cases_it_is_meant_to(golden):
    """every entry point in one chunk and across a chunk boundary with a short last chunk; every optional pointer there and not; and the
    properties of the recorded calls that do not depend on who wrote the loop"""
    cases = _traced(golden)
    assert all(v['rc'] == 0 and v['err'] == '' for v in cases.values())
    for fn in ENTRY_POINTS:
        one = [v for k, v in cases.items() if k.startswith(fn + '/one chunk')]
        two = [v for k, v in cases.items() if k.startswith(fn + '/two chunks')]
        assert one and len(two) == 1, fn
        for v in one + two:
            assert v['log'][0].startswith('malloc bytes='), (fn, v['log'][:2])           # a fresh context: the staging buffer first
            ups = [l for l in v['log'] if l.startswith('copy H2D') and ' dev=stage+' in l]
            chunks = 1 if v in one else (3 if fn in SMOOTHERS else 2)                     # the first plane goes up once per chunk
            assert len([l for l in ups if ' dev=stage+0 ' in l]) == chunks and ' host=local' not in ''.join(ups), (fn, ups)
            # one synchronisation per chunk: the helper's, or csi_nmse_device's own (behind its nmse_sum_kernel) and then no second one
            assert v['log'].count('sync') == chunks and (fn == 'csi_nmse') == any('kernel=nmse_sum_kernel(' in l for l in v['log']), fn
    assert len([k for k in cases if k.startswith('csi_hybrid_weights/one chunk')]) == 16
    assert len([k for k in cases if k.startswith('csi_lmmse_blind/one chunk')]) == 4
    for fn in SMOOTHERS:
        assert len([k for k in cases if k.startswith(fn + '/one chunk')]) == 2
    # an absent optional pointer costs its copies and nothing else: the staging buffer and the planes' places stay
    full, bare = cases['csi_lmmse_blind/one chunk/noise_var=1/corr=1']['log'], cases['csi_lmmse_blind/one chunk/noise_var=0/corr=0']['log']
    assert [l for l in full if ' host=noise_var+' not in l and ' host=corr+' not in l] == bare and len(full) == len(bare) + 2


def test_every_staged_call_asks_the_runtime_for_what_the_recording_holds(golden, seen):
    """allocation sizes, copies (direction, bytes, place in the staging buffer, place in the caller's array), launches (kernel, grid,
    workgroup size, dynamic LDS bytes) and synchronisations, in order; return code and launch counters"""
    got, want = _traced(seen), _traced(golden)
    assert set(got) == set(want)
    wrong = [k for k in want if got[k] != want[k]]
    for k in wrong[:3]:
        n = next((i for i, (a, b) in enumerate(zip(got[k]['log'], want[k]['log'])) if a != b), min(len(got[k]['log']), len(want[k]['log'])))
        print('%s: rc %s / %s, counters %s / %s, %d / %d lines, first difference at line %d:\n  got      %s\n  recorded %s' % (
            k, got[k]['rc'], want[k]['rc'], got[k]['counters'], want[k]['counters'], len(got[k]['log']), len(want[k]['log']), n,
            got[k]['log'][n:n + 3], want[k]['log'][n:n + 3]))
    assert not wrong, '%d cases differ: %s' % (len(wrong), wrong[:10])


def test_every_refusal_returns_the_recorded_code_and_text(golden, seen):
    """and does so before anything is allocated, copied or launched"""
    pick = lambda t: {k: v for k, v in _resolve(t).items() if k.startswith('refusal/')}
    got, want = pick(seen), pick(golden)
    assert set(got) == set(want)
    wrong = [(k, got[k], want[k]) for k in want if got[k] != want[k]]
    assert not wrong, '%d refusals differ, the first:\n' % len(wrong) + '\n'.join('%s: got %s, recorded %s' % w for w in wrong[:5])
    accepted = {k for k, v in want.items() if v['rc'] == 0}
    assert accepted and all(k.endswith('out_re ends on h_re') for k in accepted), accepted
    assert all(v['log'] == [] for k, v in want.items() if k not in accepted)
    texts = ' | '.join(v['err'] for v in want.values())
    for part in ('an output plane may be its own input plane (re with re, im with im); any other overlap of the planes is refused',
                 'non-finite basis entry at [233][1]', 'non-finite basis entry at [7][1]', 'basis is not orthonormal: |Q^H Q - I| = ',
                 'basis is not orthonormal: |A^H A - I| = ', 'no basis set (csi_subspace_set_basis)', 'no basis set (csi_beam_set_basis)',
                 'must start on a 16-byte boundary (got <ptr>)', 'single-input context (nt=0)', 'no dictionary set'):
        assert part in texts, part


if __name__ == '__main__':          # python tests/test_staged_calls_host.py <tree> <output file>: the recording of <tree> (see the module docstring)
    tree, target = os.path.abspath(sys.argv[1]), sys.argv[2]
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        rec = _run_driver(tree, _build_mock(tree, os.path.join(tmp, 'libcsi_mock.so')))
    with open(target, 'w') as f:
        json.dump(rec, f, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    print('%s: %d bytes, sha256 %s' % (target, os.path.getsize(target), hashlib.sha256(open(target, 'rb').read()).hexdigest()))
