#!/usr/bin/env python3
"""timing_probe.py - the measurements behind profiles/timing.txt (GPU box; not part of a test or of bench.py).

    python tools/timing_probe.py [timing] [table] [> profiles/timing.txt]        (default: both)

  timing   the symbol-timing stage at Nt = 32, Nr = 4, 4000 packets for span 64 and 256: device time of csi_sync_estimate_device
           (kernel sync_metric), csi_sync_extract_device with and without eps (sync_extract), csi_sync_embed_device (sync_embed) and
           csi_sync_correct_device (metric + extract) from the library's HIP events, 5 calls after warm-up, and of each call with its
           synchronize on the wall clock; beside csi_cfo_estimate_device (cfo_corr) and csi_cfo_rotate_device (cfo_rotate) on the
           packets and a device-to-device float4 copy (torch, timed in this process) - each as a fraction of the bytes per second the
           copy moves, read plus write, for the bytes the entry must move: 16 per folded pair of samples read by the metric, 16 per
           packet sample cut out (8 in, 8 out), 8 per packet sample in and 8 per capture sample out for the embedding
  table    the LS NMSE of the generator's packets (csi_synth_structured, 500 packets a level) at 0 / 10 / 20 / 40 dB, span 64, for
           (Nt, Nr) = (8, 2) and (32, 4): as they are, embedded at synth.timing_offsets with margins at the level's noise deviation and
           cut out at the fixed start 32, and after csi_sync_correct_device, with the share of exact starts and the mean quality"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scatter_aging_probe import copy_rate      # noqa: E402


def _i32_up(e, a):
    return e.to_device(np.ascontiguousarray(a, np.int32).view(np.float32))


def _f64_up(e, a):
    return e.to_device(np.ascontiguousarray(a, np.float64).view(np.float32).reshape(-1, 2))


def timing(nt=32, nr=4, npkt=4000, calls=5):
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import dl_channel_estimation_mamimo_amd as pkg
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    ln = 320 * nt
    samples = npkt * nr * ln
    host = np.random.default_rng(0).standard_normal((2, npkt, nr, ln), dtype=np.float32)      # the time does not depend on the values
    x = [e.to_device(host[c]) for c in range(2)]
    y = [e.empty((npkt, nr, ln)) for _ in range(2)]
    d_eps, d_hat, d_q, d_th = _f64_up(e, pkg.synth.cfo_offsets(1, 0, npkt, 0.4)), e.empty((npkt, 2)), e.empty((npkt,)), e.empty((npkt,))
    d_std = e.to_device(np.full(npkt, 0.1, np.float32))
    rate = copy_rate(8 * samples)
    print(f'== Nt={nt} Nr={nr} {npkt} packets: {8 * samples / 1e9:.2f} GB in the two preamble planes; a device-to-device copy of them writes {rate:.2f} TB/s '
          f'here, so it moves {2 * rate:.2f} TB/s (read + write)')

    def measure(run, kernels):
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
        return [prof[k]['ms'] / calls for k in kernels], wall

    share = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12 / (2 * rate)      # noqa: E731

    def line(entry, kernel, ms, nbytes, wall, verb='moves'):
        print(f'     {entry:26s} {kernel:13s} {ms:7.3f} ms: {verb} {nbytes / 1e9:.3f} GB at {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = '
              f'{share(nbytes, ms):.3f} of what the copy moves; call + synchronize {np.median(wall):.3f} ms')

    (c_ms,), c_wall = measure(lambda: (e.cfo_estimate_device(x[0], x[1], npkt, d_hat, d_quality=d_q), e.synchronize()), ['cfo_corr'])
    (r_ms,), r_wall = measure(lambda: (e.cfo_rotate_device(x[0], x[1], npkt, d_eps, -1.0, y[0], y[1]), e.synchronize()), ['cfo_rotate'])
    print('   on the packets themselves (the CFO stage, cp_skip 0):')
    line('csi_cfo_estimate_device', 'cfo_corr', c_ms, 16.0 * npkt * nr * nt * 64, c_wall, 'reads')
    line('csi_cfo_rotate_device', 'cfo_rotate', r_ms, 16.0 * samples, r_wall)
    for span in (64, 256):
        cap = [e.empty((npkt, nr, ln + span)) for _ in range(2)]
        theta = _i32_up(e, pkg.synth.timing_offsets(1, 0, npkt, span))
        pairs = npkt * nr * nt * (span + 64)
        cap_samples = npkt * nr * (ln + span)
        (b_ms,), b_wall = measure(lambda: (e.sync_embed_device(1, 0, npkt, span, theta, x[0], x[1], cap[0], cap[1], d_margin_std=d_std), e.synchronize()),
                                  ['sync_embed'])
        (m_ms,), m_wall = measure(lambda: (e.sync_estimate_device(cap[0], cap[1], npkt, span, d_th, d_eps=d_hat, d_quality=d_q), e.synchronize()),
                                  ['sync_metric'])
        (x_ms,), x_wall = measure(lambda: (e.sync_extract_device(cap[0], cap[1], npkt, span, theta, y[0], y[1]), e.synchronize()), ['sync_extract'])
        (z_ms,), z_wall = measure(lambda: (e.sync_extract_device(cap[0], cap[1], npkt, span, theta, y[0], y[1], d_eps=d_eps), e.synchronize()),
                                  ['sync_extract'])
        (k_ms, q_ms), k_wall = measure(lambda: (e.sync_correct_device(cap[0], cap[1], npkt, span, y[0], y[1], d_theta=d_th, d_eps=d_hat, d_quality=d_q),
                                                e.synchronize()), ['sync_metric', 'sync_extract'])
        print(f'   span {span}:')
        line('csi_sync_embed_device', 'sync_embed', b_ms, 8.0 * samples + 8.0 * cap_samples, b_wall)
        line('csi_sync_estimate_device', 'sync_metric', m_ms, 16.0 * pairs, m_wall, 'reads')
        line('csi_sync_extract_device', 'sync_extract', x_ms, 16.0 * samples, x_wall)
        line('  ... with eps', 'sync_extract', z_ms, 16.0 * samples, z_wall)
        print(f'     the cut-out against cfo_rotate: {r_ms / x_ms:.3f} of its rate without eps, {r_ms / z_ms:.3f} with; the metric against cfo_corr: '
              f'{(16.0 * pairs / m_ms) / (16.0 * npkt * nr * nt * 64 / c_ms):.3f} of its bytes per second')
        moved = 16.0 * pairs + 16.0 * samples
        line('csi_sync_correct_device', 'both', k_ms + q_ms, moved, k_wall)
        print(f'       ({k_ms:.3f} + {q_ms:.3f} ms)')
        for a in cap + [theta]:
            a.free()
    e.close()


def table(npkt=500, span=64):
    import dl_channel_estimation_mamimo_amd as pkg
    for nt, nr in ((8, 2), (32, 4)):
        e = pkg.CsiEngine(nt, nr, hidden=(8,))
        e.set_pilot(pkg.synth.hadamard(nt))
        print(f'== LS NMSE of the generator\'s packets (Nt={nt} Nr={nr}, {npkt} packets a level), start uniform in 0 .. {span}, margins at the noise deviation')
        print('   SNR dB   clean        cut at the fixed start   cut at theta_hat   timing_exact   timing_rmse   quality')
        ls = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
        d_link = e.empty((npkt * nr * nt,))
        amp = np.float32(pkg.synth.AMP_SCALE)
        for i, snr in enumerate((0.0, 10.0, 20.0, 40.0)):
            first = i * npkt
            d_re, d_im, h_re, h_im, d_std = e.synth_structured(3, first, npkt, snr_db=snr, want_noise_std=True)
            theta = pkg.synth.timing_offsets(3, first, npkt, span)
            d_theta, d_half, d_hat, d_q = _i32_up(e, theta), _i32_up(e, np.full(npkt, span // 2)), e.empty((npkt,)), e.empty((npkt,))
            d_margin = e.to_device(d_std.download() * amp)
            cap = e.empty((npkt, nr, 320 * nt + span)), e.empty((npkt, nr, 320 * nt + span))
            cut = e.empty((npkt, nr, 320 * nt)), e.empty((npkt, nr, 320 * nt))
            e.sync_embed_device(3, first, npkt, span, d_theta, d_re, d_im, cap[0], cap[1], d_margin_std=d_margin)

            def nmse(planes):
                e.ls_estimate_device(planes[0], planes[1], npkt, ls[0], ls[1])
                return e.nmse_device(h_re, h_im, ls[0], ls[1], npkt * nr * nt, 234, d_per_link=d_link)
            row = [nmse((d_re, d_im))]
            e.sync_extract_device(cap[0], cap[1], npkt, span, d_half, cut[0], cut[1])
            row.append(nmse(cut))
            e.sync_correct_device(cap[0], cap[1], npkt, span, cut[0], cut[1], remove_cfo=False, d_theta=d_hat, d_quality=d_q)
            row.append(nmse(cut))
            err = d_hat.download().view(np.int32).astype(np.int64) - theta
            print(f'   {snr:6g}   {row[0]:.4e}   {row[1]:.4e}               {row[2]:.4e}         {np.mean(err == 0):.4f}         '
                  f'{np.sqrt(np.mean(err.astype(np.float64) ** 2)):.3f}         {d_q.download().mean():.4f}')
            for a in (d_re, d_im, h_re, h_im, d_std, d_theta, d_half, d_hat, d_q, d_margin) + cap + cut:
                a.free()
        e.close()


if __name__ == '__main__':
    what = sys.argv[1:] or ['timing', 'table']
    if not set(what) <= {'timing', 'table'}:
        raise SystemExit(__doc__)
    if 'timing' in what:
        timing()
    if 'table' in what:
        table()
