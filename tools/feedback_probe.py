#!/usr/bin/env python3
"""feedback_probe.py - the timings of profiles/feedback.txt (GPU box; not part of a test or of bench.py).

    python tools/feedback_probe.py [-o OUT.txt] [NPKT ...]        (default 4000)

Nt = 32, Nr = 4, nc = 1 and 2, bits (9, 7) and (6, 4), ng = 1 and 4: known-channel packets at 10 dB (csi_synth_structured), then
csi_feedback_compress_device (codes and sigma) and csi_feedback_expand_device in both layouts.  Device time per call of the profile
entries fb_compress and fb_expand from the library's HIP events, the mean of 5 calls after two warm-up calls, and the bytes each kernel
must move - compress reads 8 Nr Nt 234 bytes per packet once, expand writes 8 nc Nt 234 (W) or 8 Nr Nt 234 (CSI) - over that time against
the float4 copy rate (read + write) measured in the same process."""
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
    say('quantised CSI feedback (csi_feedback_compress_device / csi_feedback_expand_device): HIP-event time per call, mean of %d calls after two warm-up calls' % calls)
    for npkt in [int(a) for a in argv] or [4000]:
        d_re, d_im, h_re, h_im, d_std = e.synth_structured(1, 0, npkt, snr_db=10.0)
        for a in (d_re, d_im, d_std):
            a.free()
        h_bytes = 8.0 * nr * nt * 234 * npkt
        copy = copy_rate(int(h_bytes))
        say('== Nt=%d Nr=%d %d packets; a float4 copy of the CSI planes reaches %.2f TB/s (read + write)' % (nt, nr, npkt, copy))
        for nc in (1, 2):
            for bits in ((9, 7), (6, 4)):
                for ng in (1, 4):
                    n_ang, n_rep = fb.n_angles(nt, nc), fb.n_reports(ng)
                    codes = [e.empty(((npkt * n_ang * n_rep + 1) // 2,)) for _ in range(2)]
                    sigma = e.empty((npkt, nc, n_rep))
                    w = [e.empty((npkt, nc, nt, 234)) for _ in range(2)]
                    csi = [e.empty((npkt, nr, nt, 234)) for _ in range(2)]
                    t = {}
                    jobs = (('fb_compress', 'compress', lambda: e.feedback_compress_device(h_re, h_im, npkt, nc, bits[0], bits[1], ng, codes[0], codes[1], d_sigma=sigma)),
                            ('fb_expand', 'expand_w', lambda: e.feedback_expand_device(npkt, nc, bits[0], bits[1], ng, e.FB_LAYOUT_W, w[0], w[1],
                                                                                        d_phi_code=codes[0], d_psi_code=codes[1])),
                            ('fb_expand', 'expand_csi', lambda: e.feedback_expand_device(npkt, nc, bits[0], bits[1], ng, e.FB_LAYOUT_CSI, csi[0], csi[1],
                                                                                          d_phi_code=codes[0], d_psi_code=codes[1], d_sigma=sigma)))
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
                    moved = dict(compress=h_bytes, expand_w=8.0 * nc * nt * 234 * npkt, expand_csi=h_bytes)
                    rate = {k: moved[k] / (t[k] * 1e-3) / 1e12 for k in t}
                    say('   nc %d bits %s ng %d (%d bits per packet): compress %.3f ms (%.2f TB/s read = %.2f of the copy rate), expand W %.3f ms '
                        '(%.2f TB/s written = %.2f), expand CSI %.3f ms (%.2f TB/s written = %.2f)'
                        % (nc, bits, ng, fb.report_bits(nt, nc, bits[0], bits[1], ng), t['compress'], rate['compress'], rate['compress'] / copy,
                           t['expand_w'], rate['expand_w'], rate['expand_w'] / copy, t['expand_csi'], rate['expand_csi'], rate['expand_csi'] / copy))
                    for a in codes + [sigma] + w + csi:
                        a.free()
        h_re.free(); h_im.free()
    if out:
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
