#!/usr/bin/env python3
"""link_probe.py - the measurements behind profiles/link_sim.txt and the timings of profiles/link_rx.txt (GPU box; not part of a test or
of bench.py).

    python tools/link_probe.py [NPKT ...]        (default 500 4000)

Nt = 32, Nr = 4, QPSK, 10 data symbols, (ns, ntrf) = (1, 1) and (2, 4), 500 rays: known-channel packets at 0 dB (csi_synth_structured),
the hybrid weights of the true planes, then csi_link_sim_device.  Device time per call of the two profile entries from the library's HIP
events after warm-up, the decoder's codewords/s, the h bytes link_txrx reads over its time against a float4 copy timed in this process
(torch), and the wall time of the 4-source data phase of one sweep level (4 x (hybrid weights + link)) beside the LS + DNN step.
Then csi_link_sim_rx_device (the receiver that estimates the effective channel from a precoded preamble) on the same arrays in the same
process, timed the same way, and the ratio of its two profile entries to those of csi_link_sim_device."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def copy_rate(nbytes):
    """float4 copy in TB/s (read + write) of nbytes, timed with events in this process"""
    import torch
    n = nbytes // 4
    a, b = torch.empty(n, dtype=torch.float32, device='cuda'), torch.empty(n, dtype=torch.float32, device='cuda')
    for _ in range(3):
        b.copy_(a)
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(10):
        b.copy_(a)
    end.record()
    torch.cuda.synchronize()
    rate = 2 * nbytes / (beg.elapsed_time(end) / 10 * 1e-3) / 1e12
    del a, b
    torch.cuda.empty_cache()
    return rate


def main(argv):
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import dl_channel_estimation_mamimo_amd as pkg
    from dl_channel_estimation_mamimo_amd import sweep
    nt, nr, n_sym, bps, rays = 32, 4, 10, 2, 500
    e = pkg.CsiEngine(nt, nr, hidden=(1024, 1024))
    rng = np.random.default_rng(0)
    for m in ('real', 'imag'):
        e.load_weights(m, pkg.synth.make_weights(rng, nt))
    e.set_pilot(pkg.synth.hadamard(nt))
    az, el = pkg.synth.random_rays(np.random.default_rng(0), rays)
    e.set_dictionary(pkg.synth.steering_ula(nt, az, el))
    for npkt in [int(a) for a in argv] or [500, 4000]:
        d_re, d_im, h_re, h_im, d_std = e.synth_structured(1, 0, npkt, snr_db=0.0)
        d_nv = e.to_device(pkg.synth.link_noise_var(d_std.download()))
        h_bytes = 8 * npkt * nr * nt * 234
        copy = copy_rate(h_bytes)
        print(f'== Nt={nt} Nr={nr} {npkt} packets, QPSK, {n_sym} symbols: h planes {h_bytes / 1e6:.1f} MB; a float4 copy of that size reaches {copy:.2f} TB/s here')
        for ns, ntrf in ((1, 1), (2, 4)):
            n_info, n_coded = e.link_frame_bits(ns, n_sym, bps)
            fbb = [e.empty((npkt, 234, ns, ntrf)) for _ in range(2)]
            frf = [e.empty((npkt, ntrf, nt)) for _ in range(2)]
            d_idx = e.empty((npkt, 234, ntrf))
            outs = [e.empty((npkt,)) for _ in range(3)]
            e.hybrid_weights_device(h_re, h_im, npkt, ns, ntrf, fbb[0], fbb[1], d_idx, d_frf_mean_re=frf[0], d_frf_mean_im=frf[1])
            calls = 5

            def timed(call):
                """device ms per call of (link_txrx, link_viterbi) after two warm-up calls"""
                for _ in range(2):
                    call()
                e.synchronize()
                e.profile_enable(True)
                e.profile_reset()
                for _ in range(calls):
                    call()
                e.synchronize()
                prof = e.profile()
                e.profile_enable(False)
                return prof['link_txrx']['ms'] / calls, prof['link_viterbi']['ms'] / calls

            tx, vit = timed(lambda: e.link_sim_device(h_re, h_im, fbb[0], fbb[1], frf[0], frf[1], d_nv, 1, 0, npkt, ns, ntrf, *outs, n_sym=n_sym, bps=bps))
            rate = h_bytes / (tx * 1e-3) / 1e12
            errs = outs[0].download().view(np.int32)
            print(f'   (ns, ntrf) = ({ns}, {ntrf}), n_info {n_info}: link_txrx {tx:7.3f} ms per call (h read at {rate:.3f} TB/s = {rate / (copy / 2):.2f} of the '
                  f'copy\'s read half), link_viterbi {vit:7.3f} ms = {npkt / (vit * 1e-3) / 1e6:.2f} M codewords/s; BER {errs.sum() / (npkt * n_info):.3e}, '
                  f'EVM {outs[1].download().mean():.1f} %, dtSNR {outs[2].download().mean():.2f} dB')
            # the receiver that estimates its channel, on the same arrays
            rx_outs = [e.empty((npkt,)) for _ in range(4)]
            rtx, rvit = timed(lambda: e.link_sim_rx_device(h_re, h_im, fbb[0], fbb[1], frf[0], frf[1], d_nv, 1, 0, npkt, ns, ntrf, *rx_outs, n_sym=n_sym, bps=bps))
            rerrs = rx_outs[0].download().view(np.int32)
            print(f'      csi_link_sim_rx_device ({e.link_preamble_symbols(ns)} preamble symbols): link_txrx {rtx:7.3f} ms per call = {rtx / tx:.3f} of the genie entry\'s, '
                  f'link_viterbi {rvit:7.3f} ms = {rvit / vit:.3f}; both entries {(rtx + rvit) / (tx + vit):.3f}; BER {rerrs.sum() / (npkt * n_info):.3e}, '
                  f'EVM {rx_outs[1].download().mean():.1f} %, gNMSE {rx_outs[3].download().mean():.3e}')
            for a in rx_outs:
                a.free()
            # the 4-source data phase of a sweep level beside the LS + DNN step
            est = [e.empty((npkt, nr, nt, 234)) for _ in range(4)]
            planes = dict(LS=(est[2], est[3]), MMSE=(est[2], est[3]), DNN=(est[0], est[1]), perfect=(h_re, h_im))
            for rep in range(2):
                t0 = time.perf_counter()
                e.estimate_device(d_re, d_im, npkt, *est)
                e.synchronize()
                t1 = time.perf_counter()
                sweep.link_level(e, planes, h_re, h_im, d_std, npkt, 1, 0, ns=ns, ntrf=ntrf, n_sym=n_sym, bps=bps)
                e.synchronize()
                t2 = time.perf_counter()
            print(f'      LS + DNN step {1e3 * (t1 - t0):7.2f} ms wall; 4 sources x (hybrid weights + link), with the result downloads {1e3 * (t2 - t1):7.2f} ms wall')
            for a in fbb + frf + [d_idx] + outs + est:
                a.free()
        for a in (d_re, d_im, h_re, h_im, d_std, d_nv):
            a.free()
    e.close()


if __name__ == '__main__':
    main(sys.argv[1:])
