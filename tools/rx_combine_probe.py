#!/usr/bin/env python3
"""rx_combine_probe.py - the timings of profiles/rx_combine.txt (GPU box; not part of a test or of bench.py).

    python tools/rx_combine_probe.py [-o OUT.txt] [NPKT ...]        (default 4000)

Nt = 32, Nr = 4, ns = 1 and 2: known-channel packets at 10 dB (csi_synth_structured), then csi_rx_combiner_device (C and sigma) beside
csi_feedback_compress_device at nc = ns (continuous angles and sigma), and csi_rx_apply_combiner_device.  Device time per call of the
profile entries rx_combiner, fb_compress and rx_combine from the library's HIP events, the mean of 5 calls after two warm-up calls, and
the bytes the apply kernel must move - 8 Nr Nt 234 bytes per packet read and the same written - over that time against the float4 copy
rate (read + write) of as many bytes measured in the same process."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from link_probe import copy_rate      # noqa: E402


def main(argv):
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import dl_channel_estimation_mamimo_amd as pkg
    fb = pkg.feedback
    out = None
    if argv[:1] == ['-o']:
        out, argv = argv[1], argv[2:]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nt, nr, calls = 32, 4, 5
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(pkg.synth.hadamard(nt))
    say('receive combining (csi_rx_combiner_device / csi_rx_apply_combiner_device): HIP-event time per call, mean of %d calls after two warm-up calls' % calls)
    for npkt in [int(a) for a in argv] or [4000]:
        d_re, d_im, h_re, h_im, d_std = e.synth_structured(1, 0, npkt, snr_db=10.0)
        for a in (d_re, d_im, d_std):
            a.free()
        h_bytes = 8.0 * nr * nt * 234 * npkt
        copy = copy_rate(int(h_bytes))
        say('== Nt=%d Nr=%d %d packets; a float4 copy of the CSI planes reaches %.2f TB/s (read + write)' % (nt, nr, npkt, copy))
        for ns in (1, 2):
            n_ang = fb.n_angles(nt, ns)
            c = [e.empty((npkt, ns, nr, 234)) for _ in range(2)]
            sigma = e.empty((npkt, ns, 234))
            ang = [e.empty((npkt, n_ang, 234)) for _ in range(2)]
            eo = [e.empty((npkt, nr, nt, 234)) for _ in range(2)]
            t = {}
            jobs = (('rx_combiner', 'combiner', lambda: e.rx_combiner_device(h_re, h_im, npkt, ns, c[0], c[1], sigma)),
                    ('fb_compress', 'compress', lambda: e.feedback_compress_device(h_re, h_im, npkt, ns, 0, 0, 1, d_phi=ang[0], d_psi=ang[1], d_sigma=sigma)),
                    ('rx_combine', 'apply', lambda: e.rx_apply_combiner_device(c[0], c[1], h_re, h_im, npkt, ns, eo[0], eo[1])))
            for entry, key, job in jobs:
                for _ in range(2):
                    job()
                e.synchronize()
                e.profile_enable(True)
                e.profile_reset()
                for _ in range(calls):
                    job()
                e.synchronize()
                t[key] = e.profile()[entry]['ms'] / calls
                e.profile_enable(False)
            rate = 2.0 * h_bytes / (t['apply'] * 1e-3) / 1e12
            say('   ns %d: combiner %.3f ms = %.2f of fb_compress at nc = ns (%.3f ms); apply %.3f ms (%.2f TB/s read + written = %.2f of the copy rate)'
                % (ns, t['combiner'], t['combiner'] / t['compress'], t['compress'], t['apply'], rate, rate / copy))
            for a in c + [sigma] + ang + eo:
                a.free()
        h_re.free(); h_im.free()
    if out:
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
