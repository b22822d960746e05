#!/usr/bin/env python3
"""beam_probe.py - device time of the beam-space Wiener smoother (csi_beam_wiener_device) per launch, beside a float4 copy of the same
session and the fp32 matrix peak, and the whole ANG step (csi_null_noise_device + csi_beam_wiener_device) beside the LS + DNN step of
bench.py (csi_ls_estimate_device + csi_predict_device, hidden 1024 x 1024, white preambles) in the same process.
usage: beam_probe.py [--nt 32 64] [--nr 4] [--packets 4000] [--runs 11] [--warmup 3] [--peak-tflops 157.3] [--no-dnn] [-o out.txt]
Per launch: HIP events of the library's profile (one call per run, median over the runs).  Whole calls: a host clock around the call
and csi_synchronize, median over the runs.  A probe only: no test runs it."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import dl_channel_estimation_mamimo_amd as pkg      # noqa: E402


def copy_ms(n_floats, runs, warmup):
    """device-to-device copy of n_floats with torch (a float4 copy kernel of the runtime), HIP events, median"""
    import torch
    src = torch.empty(n_floats, dtype=torch.float32, device='cuda').normal_()
    dst = torch.empty_like(src)
    ms = []
    for i in range(warmup + runs):
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        beg.record()
        dst.copy_(src)
        end.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(beg.elapsed_time(end))
    return float(np.median(ms))


def wall_ms(e, call, runs, warmup):
    ms = []
    for i in range(warmup + runs):
        e.synchronize()
        t0 = time.perf_counter()
        call()
        e.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def measure(nt, nr, npkt, runs, warmup, peak, dnn):
    e = pkg.CsiEngine(nt, nr, hidden=(1024, 1024) if dnn else (8,), use_bn=True)
    rng = np.random.default_rng(1)
    e.set_pilot(pkg.synth.hadamard(nt))
    e.beam_set_basis(pkg.beamspace.dft_basis(nt))
    shape = (npkt, nr, nt, 234)
    d_re, d_im = e.empty((npkt, nr, e.len_ltf)), e.empty((npkt, nr, e.len_ltf))
    e.synth_white(7, 0, npkt, d_re, d_im)
    ls_re, ls_im, o_re, o_im = (e.empty(shape) for _ in range(4))
    d_nv, d_w = e.empty((npkt, nr, 2)), e.empty((npkt, nr, nt))
    e.ls_estimate_device(d_re, d_im, npkt, ls_re, ls_im)
    e.null_noise_device(d_re, d_im, npkt, d_nv)
    v = (d_nv.download().view(np.float64)[..., 0] / nt).astype(np.float32)
    d_v = e.to_device(v)
    planes_gb = npkt * nr * nt * 234 * 8 / 1e9              # both planes of the tensor, once
    c_ms = copy_ms(npkt * nr * nt * 234 * 2, runs, warmup)    # reads them and writes them: 2 planes_gb
    copy_rate = 2 * planes_gb / c_ms
    lines = ['Nt %d Nr %d, %d packets: both planes %.3f GB; float4 copy of them (read + write) %.3f ms = %.2f TB/s' % (nt, nr, npkt, planes_gb, c_ms, copy_rate)]
    wiener = lambda: e.beam_wiener_device(ls_re, ls_im, npkt, d_v, o_re, o_im, d_w)
    for _ in range(warmup):
        wiener()
    e.synchronize()
    per = {'beam_power': [], 'beam_smooth': []}
    stats = {}
    e.profile_enable(True)
    for _ in range(runs):
        e.profile_reset()
        wiener()
        e.synchronize()
        p = e.profile()
        for k in per:
            per[k].append(p[k]['ms'] / p[k]['launches'])
            stats[k] = (p[k]['flops'] / p[k]['launches'], p[k]['bytes'] / p[k]['launches'])
    e.profile_enable(False)
    for k in ('beam_power', 'beam_smooth'):
        ms = float(np.median(per[k]))
        flops, nbytes = stats[k]
        lines.append('  %-11s %8.3f ms (min %.3f, max %.3f of %d runs)  %6.2f TB/s = %.2f of the copy rate  %6.2f TFLOP/s = %.3f of the fp32 matrix peak (%.1f)' % (
            k, ms, min(per[k]), max(per[k]), runs, nbytes / ms / 1e9, nbytes / ms / 1e9 / copy_rate, flops / ms / 1e9, flops / ms / 1e9 / peak, peak))
    w_ms = wall_ms(e, wiener, runs, warmup)
    rest = w_ms[0] - float(np.median(per['beam_power'])) - float(np.median(per['beam_smooth']))
    lines.append('  csi_beam_wiener_device, call + synchronize: %.3f ms (min %.3f, max %.3f); the weight pass, two launch gaps and the synchronize: %.3f ms' % (w_ms + (rest,)))
    ang = lambda: (e.null_noise_device(d_re, d_im, npkt, d_nv), wiener())
    a_ms = wall_ms(e, ang, runs, warmup)
    lines.append('  ANG step (csi_null_noise_device + csi_beam_wiener_device), call + synchronize: %.3f ms (min %.3f, max %.3f)' % a_ms)
    smooth_only = wall_ms(e, lambda: e.beam_smooth_device(ls_re, ls_im, npkt, o_re, o_im, d_w), runs, warmup)
    lines.append('  csi_beam_smooth_device alone, call + synchronize: %.3f ms (min %.3f, max %.3f)' % smooth_only)
    if dnn:
        e.load_weights('real', pkg.synth.make_weights(rng, nt, (1024, 1024)))
        e.load_weights('imag', pkg.synth.make_weights(rng, nt, (1024, 1024)))
        step = lambda: (e.ls_estimate_device(d_re, d_im, npkt, ls_re, ls_im), e.predict_device(d_re, d_im, npkt, o_re, o_im))
        s_ms = wall_ms(e, step, runs, warmup)
        lines.append('  LS + DNN step of bench.py (csi_ls_estimate_device + csi_predict_device, hidden 1024 x 1024), call + synchronize: %.3f ms (min %.3f, max %.3f): '
                     'the ANG step is %.2f of it' % (s_ms + (a_ms[0] / s_ms[0],)))
    e.close()
    return lines


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--nt', type=int, nargs='+', default=[32, 64])
    ap.add_argument('--nr', type=int, default=4)
    ap.add_argument('--packets', type=int, default=4000)
    ap.add_argument('--runs', type=int, default=11)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--peak-tflops', type=float, default=157.3, help='v_mfma_f32_32x32x2_f32 peak of the part (DESIGN.md 4.7)')
    ap.add_argument('--no-dnn', action='store_true')
    ap.add_argument('-o', '--out', default='')
    a = ap.parse_args()
    import torch      # before the library: whichever HIP runtime is loaded first serves both (_lib.load_library)
    torch.zeros(1, device='cuda')
    text = ['beam-space Wiener smoother (csi_beam_wiener_device), DFT beams, LS planes of white preambles; warm-up %d, median of %d runs' % (a.warmup, a.runs)]
    for nt in a.nt:
        text += measure(nt, a.nr, a.packets, a.runs, a.warmup, a.peak_tflops, not a.no_dnn)
    print('\n'.join(text))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(text) + '\n')
