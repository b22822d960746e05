#!/usr/bin/env python3
"""scatter_aging_probe.py - the measurements behind profiles/scatter_aging.txt (GPU box; not part of a test or of bench.py).

    python tools/scatter_aging_probe.py [timing] [floor] [level]        (default: all three)

  timing   csi_scatter_channel_at_device (S = 100, 1 m/s) at Nt = 32 and Nt = 64, Nr = 4, 4000 packets with 1, 4 and 16 times: device
           time per call from the library's HIP events after warm-up; in the same process the parent's noise-free call with channel
           planes (csi_synth_scattering, the yardstick); the time per added slice and the bytes it stores over that time against a
           device-to-device float4 copy of one slice timed in this process (torch)
  floor    MSEA_perfect - the NMSE of the sounding-time truth against the aged truth - against the delay, 0.25 .. 8 ms, at 1 and 10 m/s,
           on the default sweep's channel (Nt = 32, Nr = 4, S = 100, 100 m, azimuth 30, heading 0), 500 packets
  level    the default sweep's packets of one level at 10 dB, two users 15 degrees apart, aged 2 ms at 1 m/s: sinrMU beside sinrMUA for
           the sources perfect and LS (sweep.mu_level on the sounding-time planes and on sweep.aged_truth)"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def copy_rate(nbytes):
    """device-to-device copy in TB/s of bytes written, for nbytes of output, timed with events in this process"""
    import torch
    a = torch.ones(nbytes // 4, dtype=torch.float32, device='cuda')
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(20):
        b.copy_(a)
    end.record()
    torch.cuda.synchronize()
    rate = nbytes / (beg.elapsed_time(end) / 20 * 1e-3) / 1e12
    del a, b
    torch.cuda.empty_cache()
    return rate


def _device_ms(e, entry, run, calls=5):
    run()
    run()
    e.profile_enable(True)
    e.profile_reset()
    for _ in range(calls):
        run()
    p = e.profile()[entry]
    e.profile_enable(False)
    return p['ms'] / calls


def timing(nt, nr=4, npkt=4000, n_scat=100):
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import dl_channel_estimation_mamimo_amd as pkg
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(pkg.synth.hadamard(nt))
    slice_bytes = 8 * npkt * nr * nt * 234
    rate = copy_rate(slice_bytes)
    print(f'== Nt={nt} Nr={nr} {npkt} packets, S={n_scat}: one slice (a plane pair) {slice_bytes / 1e9:.3f} GB; a device-to-device copy of that size writes {rate:.2f} TB/s here')

    def parent():
        arrs = e.synth_scattering(1, 0, npkt, snr_db=None, n_scat=n_scat)
        e.synchronize()
        for a in arrs:
            if a is not None:
                a.free()
    ms_parent = _device_ms(e, 'synth_scattering', parent)
    print(f'   csi_synth_scattering, noise-free, ltf + channel planes (one launch)   {ms_parent:9.3f} ms device time per call')
    ms = {}
    for n_times in (1, 4, 16):
        planes = [e.empty((n_times, npkt, nr, nt, 234)) for _ in range(2)]
        times = [1e-3 * k for k in range(n_times)]

        def aged():
            e.scatter_channel_at_device(1, 0, npkt, times, planes[0], planes[1], speed_mps=1.0, n_scat=n_scat)
            e.synchronize()
        ms[n_times] = _device_ms(e, 'scatter_aged', aged)
        print(f'   csi_scatter_channel_at_device, {n_times:2d} times                              {ms[n_times]:9.3f} ms device time per call = '
              f'{ms[n_times] / n_times:8.3f} ms per slice = {ms[n_times] / ms_parent:.3f} of the parent\'s call')
        for a in planes:
            a.free()
    per = (ms[16] - ms[1]) / 15.0
    stored = slice_bytes / (per * 1e-3) / 1e12
    print(f'   per added slice ((16 times - 1 time) / 15)                              {per:9.3f} ms; it stores {stored:.3f} TB/s = {stored / rate:.3f} of the copy rate')
    e.close()


def floor(npkt=500):
    import dl_channel_estimation_mamimo_amd as pkg
    nt, nr = 32, 4
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    delays = [0.25, 0.5, 1.0, 2.0, 4.0, 8.0]
    print(f'== MSEA_perfect (NMSE of the sounding-time truth against the aged truth, mean over {npkt} packets x {nr * nt} links), Nt={nt} Nr={nr} S=100, '
          f'100 m, azimuth 30, heading 0, 28 GHz')
    print('   delay ms   ' + ''.join('%12g' % d for d in delays))
    d_link = e.empty((npkt * nr * nt,))
    for speed in (1.0, 10.0):
        h = e.scatter_channel_at(1, 3000, npkt, [0.0] + [1e-3 * d for d in delays], speed_mps=speed)
        re, im = h[0].download(), h[1].download()
        row = []
        for k in range(1, len(delays) + 1):
            t_re, t_im, s_re, s_im = (e.to_device(x) for x in (re[k], im[k], re[0], im[0]))
            row.append(e.nmse_device(t_re, t_im, s_re, s_im, npkt * nr * nt, 234, d_per_link=d_link))
            for a in (t_re, t_im, s_re, s_im):
                a.free()
        print('   %4g m/s   ' % speed + ''.join('%12.4e' % v for v in row))
    e.close()


def level(npkt=500, snr=10.0, delay_ms=2.0, speed=1.0):
    import dl_channel_estimation_mamimo_amd as pkg
    from dl_channel_estimation_mamimo_amd import sweep
    nt, nr, seed, first, spacing = 32, 4, 1, 3000, 15.0
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(pkg.synth.hadamard(nt))
    aging = dict(delay_ms=delay_ms, speed_mps=speed)
    planes, nv, aged = [], [], []
    for u in range(2):
        d_re, d_im, h_re, h_im, d_std, _ = e.synth_scattering(seed + u, first, npkt, snr_db=snr, az_deg=30.0 + u * spacing)
        ls = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
        e.ls_estimate_device(d_re, d_im, npkt, ls[0], ls[1])
        planes.append(dict(LS=ls, perfect=(h_re, h_im)))
        nv.append(pkg.synth.link_noise_var(d_std.download(), True))
        aged.append(sweep.aged_truth(e, npkt, seed + u, first, {}, aging, az_offset=u * spacing))
    now = sweep.mu_level(e, planes, np.stack(nv), npkt, seed, first)
    later = sweep.mu_level(e, planes, np.stack(nv), npkt, seed, first, true=aged, family='MUA')
    print(f'== the default sweep\'s level at {snr:g} dB (Nt={nt} Nr={nr} S=100, packets {first} .. of stream {seed}), 2 users {spacing:g} degrees apart, '
          f'zero forcing, QPSK, 10 symbols; aged {delay_ms:g} ms at {speed:g} m/s, heading 0')
    for x in ('perfect', 'LS'):
        print(f'   {x:8s} sinrMU {now["sinrMU_" + x].mean():7.2f} dB   sinrMUA {later["sinrMUA_" + x].mean():7.2f} dB   '
              f'bersMU {now["bersMU_" + x].mean():.3e}   bersMUA {later["bersMUA_" + x].mean():.3e}')
    e.close()


if __name__ == '__main__':
    what = sys.argv[1:] or ['timing', 'floor', 'level']
    if not set(what) <= {'timing', 'floor', 'level'}:
        raise SystemExit(__doc__)
    if 'timing' in what:
        timing(32)
        timing(64)
    if 'floor' in what:
        floor()
    if 'level' in what:
        level()
