#!/usr/bin/env python3
"""subspace_probe.py - HIP-event time of the delay-subspace smoother (csi_subspace_smooth_device) per rank, beside a float4 copy of the
same bytes (x_re, x_im in, y_re, y_im out: a device-to-device copy of both planes) and beside the fp32 matrix peak.
usage: subspace_probe.py [--nt 32] [--nr 4] [--packets 4000] [--rank 8 32 64 128] [--pre 0] [--reps 5] [--peak-tflops 157.3] [-o out.txt]
(default output profiles/subspace_smooth.txt is NOT written unless -o is given: the accuracy lines of that file come from the GPU tests)"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import dl_channel_estimation_mamimo_amd as pkg      # noqa: E402


def copy_ms(e, planes, reps):
    """device-to-device copy of both planes with torch (a float4 copy kernel of the runtime), HIP events"""
    import torch
    n = int(np.prod(planes))
    src = [torch.empty(n, dtype=torch.float32, device='cuda').normal_() for _ in range(2)]
    dst = [torch.empty_like(s) for s in src]
    for s, d in zip(src, dst):
        d.copy_(s)
    torch.cuda.synchronize()
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(reps):
        for s, d in zip(src, dst):
            d.copy_(s)
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / reps


def measure(nt, nr, npkt, ranks, pre, reps, peak):
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    shape = (npkt, nr, nt, 234)
    rng = np.random.default_rng(1)
    x_re, x_im = (e.to_device(rng.standard_normal(shape, dtype=np.float32)) for _ in range(2))
    o_re, o_im = e.empty(shape), e.empty(shape)
    rows = npkt * nr * nt
    gbytes = rows * 234 * 16 / 1e9
    c_ms = copy_ms(e, shape, reps)
    lines = ['Nt %d Nr %d, %d packets = %d rows, %.3f GB in + out; float4 copy of the same bytes %.3f ms (%.2f TB/s)' % (
        nt, nr, npkt, rows, gbytes, c_ms, gbytes / c_ms)]
    for rank in ranks:
        Q, _ = pkg.subspace.delay_basis(rank, min(pre, rank))
        e.subspace_set_basis(Q)
        e.subspace_smooth_device(x_re, x_im, npkt, o_re, o_im)      # loads the code
        e.synchronize()
        e.profile_enable(True)
        e.profile_reset()
        for _ in range(reps):
            e.subspace_smooth_device(x_re, x_im, npkt, o_re, o_im)
        e.synchronize()
        p = e.profile()['subspace_smooth']
        e.profile_enable(False)
        ms = p['ms'] / p['launches']
        tf = p['flops'] / p['launches'] / ms / 1e9
        lines.append('  rank %3d: %8.3f ms  %7.2f TFLOP/s = %.3f of the fp32 matrix peak (%.1f)  copy / kernel = %.3f  %.2f TB/s' % (
            Q.shape[1], ms, tf, tf / peak, peak, c_ms / ms, gbytes / ms))
    return lines


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--nt', type=int, default=32)
    ap.add_argument('--nr', type=int, default=4)
    ap.add_argument('--packets', type=int, default=4000)
    ap.add_argument('--rank', type=int, nargs='+', default=[8, 32, 64, 128])
    ap.add_argument('--pre', type=int, default=0)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--peak-tflops', type=float, default=157.3, help='v_mfma_f32_32x32x2_f32 peak of the part (DESIGN.md 4.7)')
    ap.add_argument('-o', '--out', default='')
    a = ap.parse_args()
    text = ['delay-subspace smoother (csi_subspace_smooth_device), w = none, random planes; HIP-event time, mean of %d calls' % a.reps]
    text += measure(a.nt, a.nr, a.packets, a.rank, a.pre, a.reps, a.peak_tflops)
    print('\n'.join(text))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(text) + '\n')
