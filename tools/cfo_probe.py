#!/usr/bin/env python3
"""cfo_probe.py - the measurements behind profiles/cfo.txt (GPU box; not part of a test or of bench.py).

    python tools/cfo_probe.py [timing] [table] [> profiles/cfo.txt]        (default: both)

  timing   the carrier-frequency-offset stage at Nt = 32, Nr = 4, 4000 packets for cp_skip 0 and 16: device time of
           csi_cfo_estimate_device (kernel cfo_corr), csi_cfo_rotate_device (cfo_rotate) and csi_cfo_correct_device (both) from the
           library's HIP events after warm-up, and of each call with its synchronize on the wall clock; each against a device-to-device
           float4 copy (torch, timed in this process) - as a fraction of the bytes per second the copy moves, read plus write - for the
           bytes the entry must move: 16 per correlated pair of samples read, 16 per sample rotated (8 in, 8 out)
  table    the LS NMSE of the generator's packets (csi_synth_structured, Nt = 32, Nr = 4, 500 packets a level) at 0 / 10 / 20 / 40 dB:
           as they are, under offsets uniform in +-0.01 subcarrier spacings (synth.cfo_offsets, csi_cfo_rotate_device) and after
           csi_cfo_correct_device, with the rms error of the offset estimate and the mean quality"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scatter_aging_probe import copy_rate      # noqa: E402


def _eps_up(e, eps):
    return e.to_device(np.ascontiguousarray(eps, np.float64).view(np.float32).reshape(-1, 2))


def timing(nt=32, nr=4, npkt=4000, calls=5):
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import dl_channel_estimation_mamimo_amd as pkg
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    samples = npkt * nr * 320 * nt
    host = np.random.default_rng(0).standard_normal((2, npkt, nr, 320 * nt), dtype=np.float32)      # the time does not depend on the values
    x = [e.to_device(host[c]) for c in range(2)]
    y = [e.empty((npkt, nr, 320 * nt)) for _ in range(2)]
    d_eps, d_hat, d_q = _eps_up(e, pkg.synth.cfo_offsets(1, 0, npkt, 0.4)), e.empty((npkt, 2)), e.empty((npkt,))
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

    for cp_skip in (0, 16):
        pairs = npkt * nr * nt * (64 - cp_skip)
        (c_ms,), c_wall = measure(lambda: (e.cfo_estimate_device(x[0], x[1], npkt, d_hat, cp_skip=cp_skip, d_quality=d_q), e.synchronize()), ['cfo_corr'])
        (r_ms,), r_wall = measure(lambda: (e.cfo_rotate_device(x[0], x[1], npkt, d_eps, 1.0, y[0], y[1]), e.synchronize()), ['cfo_rotate'])
        (k_ms, q_ms), k_wall = measure(lambda: (e.cfo_correct_device(x[0], x[1], npkt, y[0], y[1], cp_skip=cp_skip, d_eps=d_hat, d_quality=d_q),
                                                e.synchronize()), ['cfo_corr', 'cfo_rotate'])
        share = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12 / (2 * rate)      # noqa: E731
        print(f'   cp_skip {cp_skip}:')
        print(f'     csi_cfo_estimate_device  cfo_corr   {c_ms:7.3f} ms: reads {16.0 * pairs / 1e9:.3f} GB at {16.0 * pairs / (c_ms * 1e-3) / 1e12:.2f} TB/s = '
              f'{share(16.0 * pairs, c_ms):.3f} of what the copy moves; call + synchronize {np.median(c_wall):.3f} ms')
        print(f'     csi_cfo_rotate_device    cfo_rotate {r_ms:7.3f} ms: moves {16.0 * samples / 1e9:.3f} GB at {16.0 * samples / (r_ms * 1e-3) / 1e12:.2f} TB/s = '
              f'{share(16.0 * samples, r_ms):.3f} of what the copy moves; call + synchronize {np.median(r_wall):.3f} ms')
        moved = 16.0 * pairs + 16.0 * samples
        print(f'     csi_cfo_correct_device   both       {k_ms + q_ms:7.3f} ms ({k_ms:.3f} + {q_ms:.3f}): moves {moved / 1e9:.3f} GB at '
              f'{moved / ((k_ms + q_ms) * 1e-3) / 1e12:.2f} TB/s = {share(moved, k_ms + q_ms):.3f} of what the copy moves; call + synchronize '
              f'{np.median(k_wall):.3f} ms')
    e.close()


def table(nt=32, nr=4, npkt=500, max_eps=0.01):
    import dl_channel_estimation_mamimo_amd as pkg
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(pkg.synth.hadamard(nt))
    print(f'== LS NMSE of the generator\'s packets (Nt={nt} Nr={nr}, {npkt} packets a level), offsets uniform in +-{max_eps:g} subcarrier spacings, cp_skip 0 / 16')
    print('   SNR dB   clean        with the offset   corrected (0)   corrected (16)   eps rmse (0)   eps rmse (16)   quality (0)')
    ls = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
    d_link = e.empty((npkt * nr * nt,))
    for i, snr in enumerate((0.0, 10.0, 20.0, 40.0)):
        first = i * npkt
        d_re, d_im, h_re, h_im, _ = e.synth_structured(3, first, npkt, snr_db=snr, want_noise_std=False)
        eps = pkg.synth.cfo_offsets(3, first, npkt, max_eps)
        d_eps, d_hat, d_q = _eps_up(e, eps), e.empty((npkt, 2)), e.empty((npkt,))
        off = e.empty((npkt, nr, 320 * nt)), e.empty((npkt, nr, 320 * nt))
        fix = e.empty((npkt, nr, 320 * nt)), e.empty((npkt, nr, 320 * nt))
        e.cfo_rotate_device(d_re, d_im, npkt, d_eps, 1.0, off[0], off[1])

        def nmse(planes):
            e.ls_estimate_device(planes[0], planes[1], npkt, ls[0], ls[1])
            return e.nmse_device(h_re, h_im, ls[0], ls[1], npkt * nr * nt, 234, d_per_link=d_link)
        row = [nmse((d_re, d_im)), nmse(off)]
        rmse, quality = [], []
        for cp_skip in (0, 16):
            e.cfo_correct_device(off[0], off[1], npkt, fix[0], fix[1], cp_skip=cp_skip, d_eps=d_hat, d_quality=d_q)
            row.append(nmse(fix))
            err = d_hat.download().view(np.float64)[..., 0] - eps
            rmse.append(float(np.sqrt(np.mean((err - np.rint(err)) ** 2))))
            quality.append(float(d_q.download().mean()))
        print(f'   {snr:6g}   {row[0]:.4e}   {row[1]:.4e}        {row[2]:.4e}      {row[3]:.4e}       {rmse[0]:.3e}      {rmse[1]:.3e}       {quality[0]:.4f}')
        for a in (d_re, d_im, h_re, h_im, d_eps, d_hat, d_q) + off + fix:
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
