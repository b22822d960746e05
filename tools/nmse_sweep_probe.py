#!/usr/bin/env python3
"""nmse_sweep_probe.py - the measurements behind profiles/nmse_sweep.txt (GPU box; not part of a test or of bench.py).
  generator            csi_synth_structured at config 2 (Nt = 32, Nr = 4, 4000 packets) and at Nt = 128, Nr = 16 (400 packets): device time
                       per call from the library's HIP events after warm-up (noise-free / noisy, with / without the channel planes), bytes
                       written over that time against a write-only fill and a float4 copy of the same size timed in this process (torch),
                       and beside it the wall time of the host route to such packets (synth.mixed_snr_batch + upload), config 2 only
  once NT NR NPKT      one warm-up and one noisy call (for a kernel trace)
  oracle OUT [N]       the weights a sweep saved in OUT, N (20) packets at -20 and 0 dB: evaluate_level beside the fp64 oracle's NMSE of the
                       same downloaded packets"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def device_rates(nbytes):
    """(write-only fill, copy) in TB/s for nbytes of output, timed with events in this process"""
    import torch
    n = nbytes // 4
    a, b = torch.empty(n, dtype=torch.float32, device='cuda'), torch.empty(n, dtype=torch.float32, device='cuda')
    out = []
    for fn, moved in ((lambda: a.fill_(1.0), nbytes), (lambda: b.copy_(a), 2 * nbytes)):
        for _ in range(3):
            fn()
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        beg.record()
        for _ in range(10):
            fn()
        end.record()
        torch.cuda.synchronize()
        out.append(moved / (beg.elapsed_time(end) / 10 * 1e-3) / 1e12)
    del a, b
    torch.cuda.empty_cache()
    return out


def generator(nt, nr, npkt, host_route):
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import dl_channel_estimation_mamimo_amd as pkg
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    P = pkg.synth.hadamard(nt)
    e.set_pilot(P)
    snr = np.repeat(np.asarray(pkg.synth.SNR_LEVELS_DB, np.float32), (npkt + 7) // 8)[:npkt]
    ltf_bytes, h_bytes = 8 * npkt * nr * 320 * nt, 8 * npkt * nr * nt * 234
    fill, copy = device_rates(ltf_bytes + h_bytes)
    print(f'== Nt={nt} Nr={nr} {npkt} packets: ltf planes {ltf_bytes / 1e9:.3f} GB, channel planes {h_bytes / 1e9:.3f} GB; '
          f'in this process a write-only fill reaches {fill:.2f} TB/s, a float4 copy {copy:.2f} TB/s (read + write)')
    for label, kw in (('noise-free, ltf only', dict(snr_db=None, want_channel=False)), ('noise-free, ltf + channel', dict(snr_db=None)),
                      ('noisy (power pass + packet pass), ltf only', dict(snr_db=snr, want_channel=False)),
                      ('noisy (power pass + packet pass), ltf + channel', dict(snr_db=snr))):
        for _ in range(2):
            arrs = e.synth_structured(1, 0, npkt, **kw)
            e.synchronize()
            for a in arrs:
                if a is not None:
                    a.free()
        e.profile_enable(True)
        e.profile_reset()
        calls = 5
        t0 = time.perf_counter()
        for _ in range(calls):
            arrs = e.synth_structured(1, 0, npkt, **kw)
            e.synchronize()
            for a in arrs:
                if a is not None:
                    a.free()
        wall = (time.perf_counter() - t0) / calls * 1e3
        p = e.profile()['synth_structured']
        e.profile_enable(False)
        ms = p['ms'] / p['launches']
        rate = p['bytes'] / p['launches'] / (ms * 1e-3) / 1e12
        print(f'   {label:48s} {ms:8.3f} ms device time per call ({wall:8.3f} ms wall incl. allocation)   {rate:6.3f} TB/s written = '
              f'{rate / fill:.2f} of the fill rate, {rate / copy:.2f} of the copy rate')
    if host_route:
        t0 = time.perf_counter()
        d_re, d_im = e.empty((npkt, nr, 320 * nt)), e.empty((npkt, nr, 320 * nt))
        for first, _, blk in pkg.synth.mixed_snr_batch(3, nr, P, per_level=npkt // 8, threads=8):
            d_re.upload(np.ascontiguousarray(blk.real), first=first)
            d_im.upload(np.ascontiguousarray(blk.imag), first=first)
        e.synchronize()
        print(f'   host route (synth.mixed_snr_batch, 8 threads, + upload; no channel returned)   {(time.perf_counter() - t0) * 1e3:10.1f} ms wall')
    e.close()


def once(nt, nr, npkt):
    import dl_channel_estimation_mamimo_amd as pkg
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(pkg.synth.hadamard(nt))
    for _ in range(2):
        e.synth_structured(1, 0, npkt, snr_db=0.0)
        e.synchronize()
    e.close()


def oracle_check(out, n):
    import dl_channel_estimation_mamimo_amd as pkg
    from dl_channel_estimation_mamimo_amd import sweep
    from dl_channel_estimation_mamimo_amd.cli import _find_weights
    from oracle import csi_oracle as o
    import json
    with open(os.path.join(out, 'sweep.json')) as f:
        cfg = json.load(f)
    nt, nr = cfg['nt'], cfg['nr']
    w = {d: pkg.load_weight_file(_find_weights(out, d)) for d in ('real', 'imag')}
    hidden = [w['real'][f'fc_dense{i}.bias'].shape[0] for i in range(8) if f'fc_dense{i}.bias' in w['real']]
    e = pkg.CsiEngine(nt, nr, hidden=hidden, use_bn='bn0.gamma' in w['real'])
    P = pkg.synth.hadamard(nt)
    e.set_pilot(P)
    for d in ('real', 'imag'):
        e.load_weights(d, w[d])
    for snr in (-20.0, 0.0):
        got = sweep.evaluate_level(e, snr, n, cfg['seed'] + 1, 10 ** 6, cfg['n_taps'], cfg['amp_scale'], keep=True)
        d_re, d_im, h_re, h_im, ls_re, ls_im = got['arrays']
        ltf = d_re.download().astype(np.float64) + 1j * d_im.download()
        h = h_re.download().astype(np.float64) + 1j * h_im.download()
        r_re, r_im = o.predict_packets(ltf, P, w['real'], w['imag'], np.float64, pkt_batch=n)
        ref = dict(LS=o.ls_estimate(ltf, P), DNN=r_re + 1j * r_im)
        for name, est in ref.items():
            want = np.mean([o.nmse_subk(h[p], est[p]) for p in range(n)])
            print(f'   {snr:+5.0f} dB {name:4s}: device {got["MSE_" + name].mean():.6e}   fp64 oracle {want:.6e}   relative difference {abs(got["MSE_" + name].mean() / want - 1):.2e}')
        for a in got['arrays']:
            a.free()
    e.close()


if __name__ == '__main__':
    cmd = sys.argv[1] if len(sys.argv) > 1 else 'generator'
    if cmd == 'generator':
        generator(32, 4, 4000, True)
        generator(128, 16, 400, False)
    elif cmd == 'once':
        once(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    elif cmd == 'oracle':
        oracle_check(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 20)
    else:
        raise SystemExit(__doc__)
