#!/usr/bin/env python3
"""mu_link_probe.py - the timings of profiles/mu_link.txt (GPU box; not part of a test or of bench.py).

    python tools/mu_link_probe.py [-o OUT.txt] [NPKT ...]        (default 500 4000)

Nt = 32, Nr = 4, QPSK, 10 data symbols, (U, ns) = (4, 1), (4, 4) and (8, 2): known-channel packets at 10 dB per user (csi_synth_structured,
stream 1 + u), the zero-forcing precoder of the true planes (csi_mu_precoder_device), then csi_mu_link_sim_device.  Device time per call
of the profile entries mu_precoder, mu_txrx and link_viterbi from the library's HIP events after warm-up; the bytes each kernel has to
read (the addressed rows of h for the precoder; those and W for mu_txrx) over its time against the read half of a float4 copy of the
users' h planes timed in this process (torch) - the yardstick of profiles/link_sim.txt; and the wall time of the 4-source multi-user
data phase of one sweep level (sweep.mu_level) beside U times the single-user phase (sweep.link_level: hybrid weights + link)."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from link_probe import copy_rate      # noqa: E402


def main(argv):
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import dl_channel_estimation_mamimo_amd as pkg
    from dl_channel_estimation_mamimo_amd import sweep
    out = None
    if argv[:1] == ['-o']:
        out, argv = argv[1], argv[2:]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nt, nr, n_sym, bps, rays, calls = 32, 4, 10, 2, 500, 5
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(pkg.synth.hadamard(nt))
    az, el = pkg.synth.random_rays(np.random.default_rng(0), rays)
    e.set_dictionary(pkg.synth.steering_ula(nt, az, el))
    say('multi-user downlink (csi_mu_precoder_device, csi_mu_link_sim_device): HIP-event time per call, mean of %d calls after two warm-up calls' % calls)
    for npkt in [int(a) for a in argv] or [500, 4000]:
        users = []
        for u in range(8):
            d_re, d_im, h_re, h_im, d_std = e.synth_structured(1 + u, 0, npkt, snr_db=10.0)
            d_re.free(); d_im.free()
            users.append((h_re, h_im, d_std))
        plane_bytes = 8 * npkt * nr * nt * 234
        say('== Nt=%d Nr=%d %d packets, QPSK, %d symbols: one user\'s h planes %.1f MB' % (nt, nr, npkt, n_sym, plane_bytes / 1e6))
        for nu, ns in ((4, 1), (4, 4), (8, 2)):
            m = nu * ns
            n_info, n_coded = e.link_frame_bits(ns, n_sym, bps)
            h_re, h_im = [x[0] for x in users[:nu]], [x[1] for x in users[:nu]]
            nv = np.stack([pkg.synth.link_noise_var(x[2].download()) for x in users[:nu]])
            d_nv = e.to_device(nv)
            w = [e.empty((npkt, m, nt, 234)) for _ in range(2)]
            outs = [e.empty((nu, npkt)) for _ in range(3)]
            copy = copy_rate(nu * plane_bytes)

            def both():
                e.mu_precoder_device(h_re, h_im, npkt, ns, w[0], w[1])
                e.mu_link_sim_device(h_re, h_im, w[0], w[1], d_nv, 1, 0, npkt, ns, *outs, n_sym=n_sym, bps=bps)

            for _ in range(2):
                both()
            e.synchronize()
            e.profile_enable(True)
            e.profile_reset()
            for _ in range(calls):
                both()
            e.synchronize()
            prof = e.profile()
            e.profile_enable(False)
            pre, tx, vit = (prof[k]['ms'] / calls for k in ('mu_precoder', 'mu_txrx', 'link_viterbi'))
            pre_bytes = 8.0 * npkt * m * nt * 234                      # the addressed rows, once
            tx_bytes = 8.0 * npkt * nu * (ns + m) * nt * 234           # per (packet, user): its ns rows of h and the M rows of W
            r_pre, r_tx = pre_bytes / (pre * 1e-3) / 1e12, tx_bytes / (tx * 1e-3) / 1e12
            errs = outs[0].download().view(np.int32)
            say('   (U, ns) = (%d, %d), M = %d, n_info %d; a float4 copy of the U users\' h planes reaches %.2f TB/s (read + write)' % (nu, ns, m, n_info, copy))
            say('      mu_precoder %8.3f ms per call: %.1f MB of addressed h rows at %.3f TB/s = %.3f of the copy\'s read half (the kernel reads them twice)'
                % (pre, pre_bytes / 1e6, r_pre, r_pre / (copy / 2)))
            say('      mu_txrx     %8.3f ms per call: %.1f MB of h rows and W at %.3f TB/s = %.3f of the copy\'s read half; link_viterbi %8.3f ms = %.2f M codewords/s'
                % (tx, tx_bytes / 1e6, r_tx, r_tx / (copy / 2), vit, nu * npkt / (vit * 1e-3) / 1e6))
            say('      BER %.3e, EVM %.1f %%, SINR %.2f dB (perfect CSI, 10 dB)' % (errs.sum() / (nu * npkt * n_info), outs[1].download().mean(), outs[2].download().mean()))
            # one sweep level: the 4-source multi-user phase beside U times the 4-source single-user phase
            planes = [dict(LS=(a, b), MMSE=(a, b), DNN=(a, b), perfect=(a, b)) for a, b in zip(h_re, h_im)]
            for rep in range(2):
                t0 = time.perf_counter()
                sweep.mu_level(e, planes, nv, npkt, 1, 0, ns=ns, n_sym=n_sym, bps=bps)
                e.synchronize()
                t1 = time.perf_counter()
                for u in range(nu):
                    sweep.link_level(e, planes[u], h_re[u], h_im[u], users[u][2], npkt, 1, 0, ns=ns, ntrf=ns, n_sym=n_sym, bps=bps)
                e.synchronize()
                t2 = time.perf_counter()
            say('      sweep level, 4 sources, with the result downloads: multi-user phase %8.2f ms wall; %d x single-user (hybrid weights + link) %8.2f ms wall'
                % (1e3 * (t1 - t0), nu, 1e3 * (t2 - t1)))
            for a in w + outs + [d_nv]:
                a.free()
        for x in users:
            for a in x:
                a.free()
    e.close()
    if out:
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
