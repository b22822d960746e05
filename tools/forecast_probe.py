#!/usr/bin/env python3
"""forecast_probe.py - the measurements behind profiles/forecast.txt (GPU box; not part of a test or of bench.py).

    python tools/forecast_probe.py [timing] [level] [> profiles/forecast.txt]        (default: both)

  timing   the channel forecast (csi_forecast_device) at Nt = 32, Nr = 4, 4000 packets for (P, M, d) = (8, 4, 2) and (16, 8, 4): device
           time of the Gram, the fit and the apply kernel from the library's HIP events after warm-up and of the whole call (wall clock
           around call + synchronize); the Gram kernel against a device-to-device float4 copy (torch, timed in this process) of the
           8 P Nt 234 bytes per (packet, rx) it reads - as a fraction of the bytes per second the copy moves, read plus write - and against the fp32 matrix peak for the 1536 flop per float of its three 16x16x4
           products; the apply pass against the copy rate of the bytes it moves; csi_sounding_noise_device on one plane pair
  level    the default sweep's packets of one level at 10 dB (Nt = 32, Nr = 4, S = 100), two users 15 degrees apart, 2 ms at 1 m/s,
           (P, M, d) = (12, 4, 4): the NMSE against the aged truth of the sounding-time planes (MSEA) and of their forecast (MSEF), and
           sinrMUA beside the same data phase with the forecast planes as estimates (MUF), for the sources perfect and LS - the steps of sweep --forecast
           (sweep.forecast_planes, sweep.aged_truth, sweep.mu_level with the family MUF) on LS and true planes, without the fitted models"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scatter_aging_probe import copy_rate      # noqa: E402

MATRIX_PEAK_TF = 157.3


def timing(nt=32, nr=4, npkt=4000, calls=5):
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import dl_channel_estimation_mamimo_amd as pkg
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    plane = npkt * nr * nt * 234
    host = np.random.default_rng(0).standard_normal((2, npkt, nr, nt, 234), dtype=np.float32)      # the time does not depend on the values
    for P, M, d in ((8, 4, 2), (16, 8, 4)):
        x = [[e.to_device(host[(i + c) % 2]) for i in range(P)] for c in range(2)]
        y = [e.empty((npkt, nr, nt, 234)) for _ in range(2)]
        rate = copy_rate(8 * P * plane)
        run = lambda: (e.forecast_device(x[0], x[1], npkt, M, d, y[0], y[1]), e.synchronize())      # noqa: E731
        run()
        run()
        e.profile_enable(True)
        e.profile_reset()
        for _ in range(calls):
            run()
        prof = e.profile()
        e.profile_enable(False)
        wall = []
        for _ in range(calls):
            t0 = time.perf_counter()
            run()
            wall.append(1e3 * (time.perf_counter() - t0))
        g, f, a = (prof[k]['ms'] / calls for k in ('forecast_gram', 'forecast_fit', 'forecast_apply'))
        read = 8.0 * P * plane
        print(f'== Nt={nt} Nr={nr} {npkt} packets, (P, M, d) = ({P}, {M}, {d}); a device-to-device copy of {read / 1e9:.2f} GB writes {rate:.2f} TB/s here, '
              f'so it moves {2 * rate:.2f} TB/s (read + write)')
        print(f'   forecast_gram   {g:8.3f} ms: reads {read / (g * 1e-3) / 1e12:.2f} TB/s = {read / (g * 1e-3) / 1e12 / (2 * rate):.3f} of what the copy moves; '
              f'{1536.0 * plane / (g * 1e-3) / 1e12:.1f} TFLOP/s = {1536.0 * plane / (g * 1e-3) / 1e12 / MATRIX_PEAK_TF:.3f} of the fp32 matrix peak')
        print(f'   forecast_fit    {f:8.3f} ms')
        moved = 8.0 * (M + 1) * plane
        print(f'   forecast_apply  {a:8.3f} ms: moves {moved / (a * 1e-3) / 1e12:.2f} TB/s = {moved / (a * 1e-3) / 1e12 / (2 * rate):.3f} of what the copy moves')
        print(f'   csi_forecast_device, call + synchronize: {np.median(wall):.3f} ms (min {min(wall):.3f}, max {max(wall):.3f}); the three kernels {g + f + a:.3f} ms')
        for arr in x[0] + x[1] + y:
            arr.free()
    x = [e.to_device(host[c]) for c in range(2)]
    v = e.to_device(np.full((npkt, nr), 0.01, np.float32))
    run = lambda: (e.sounding_noise_device(1, 0, npkt, v, x[0], x[1]), e.synchronize())      # noqa: E731
    run()
    e.profile_enable(True)
    e.profile_reset()
    for _ in range(calls):
        run()
    print(f'   sounding_noise  {e.profile()["sounding_noise"]["ms"] / calls:8.3f} ms per plane pair, in place')
    e.close()


def level(npkt=500, snr=10.0, delay_ms=2.0, speed=1.0, P=12, M=4, d=4):
    import dl_channel_estimation_mamimo_amd as pkg
    from dl_channel_estimation_mamimo_amd import sweep
    nt, nr, seed, first, spacing = 32, 4, 1, 3000, 15.0
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(pkg.synth.hadamard(nt))
    aging = dict(delay_ms=delay_ms, speed_mps=speed)
    forecast = dict(soundings=P, order=M, steps=d)
    planes, fplanes, nv, aged, msea, msef = [], [], [], [], {}, {}
    d_link = e.empty((npkt * nr * nt,))
    for u in range(2):
        d_re, d_im, h_re, h_im, d_std, _ = e.synth_scattering(seed + u, first, npkt, snr_db=snr, az_deg=30.0 + u * spacing)
        ls = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
        e.ls_estimate_device(d_re, d_im, npkt, ls[0], ls[1])
        src = dict(LS=ls, perfect=(h_re, h_im))
        planes.append(src)
        nv.append(pkg.synth.link_noise_var(d_std.download(), True))
        aged.append(sweep.aged_truth(e, npkt, seed + u, first, {}, aging, az_offset=u * spacing))
        # the sweep's own step: the history, its LS noise and the forecast of both sources
        out = sweep.forecast_planes(e, dict(planes=src, ltf=(d_re, d_im)), npkt, seed + u, first, {}, aging, forecast, az_offset=u * spacing)
        if u == 0:
            for name in sweep.FORECAST_SOURCES:
                msea[name] = e.nmse_device(aged[0][0], aged[0][1], src[name][0], src[name][1], npkt * nr * nt, 234, d_per_link=d_link)
                msef[name] = e.nmse_device(aged[0][0], aged[0][1], out[name][0], out[name][1], npkt * nr * nt, 234, d_per_link=d_link)
        fplanes.append(out)
    later = sweep.mu_level(e, planes, np.stack(nv), npkt, seed, first, true=aged, family='MUA')
    ahead = sweep.mu_level(e, fplanes, np.stack(nv), npkt, seed, first, true=aged, family='MUF')
    print(f'== the default sweep\'s level at {snr:g} dB (Nt={nt} Nr={nr} S=100, packets {first} .. of stream {seed}), 2 users {spacing:g} degrees apart, '
          f'zero forcing, QPSK, 10 symbols; {delay_ms:g} ms at {speed:g} m/s, heading 0; forecast (P, M, d) = ({P}, {M}, {d}), ridge 1e-5')
    for x in ('perfect', 'LS'):
        print(f'   {x:8s} MSEA {msea[x]:.4e} -> MSEF {msef[x]:.4e}   sinrMUA {later["sinrMUA_" + x].mean():7.2f} dB -> sinrMUF {ahead["sinrMUF_" + x].mean():7.2f} dB   '
              f'bersMUA {later["bersMUA_" + x].mean():.3e} -> bersMUF {ahead["bersMUF_" + x].mean():.3e}')
    e.close()


if __name__ == '__main__':
    what = sys.argv[1:] or ['timing', 'level']
    if not set(what) <= {'timing', 'level'}:
        raise SystemExit(__doc__)
    if 'timing' in what:
        timing()
    if 'level' in what:
        level()
