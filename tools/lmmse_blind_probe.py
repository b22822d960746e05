#!/usr/bin/env python3
"""lmmse_blind_probe.py - HIP-event time per kernel of the blind LMMSE smoother (csi_lmmse_blind_device) at the bench shape
(Nt = 32, Nr = 4; 500 and 4000 packets at 10 dB), beside csi_lmmse_estimate_device on the same LS planes in the same process.
usage: lmmse_blind_probe.py [out.txt]    (default profiles/lmmse_blind.txt; the accuracy lines of that file come from the GPU tests)"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import dl_channel_estimation_mamimo_amd as pkg      # noqa: E402

KERNELS = ('lmmse_null_noise', 'lmmse_freq_corr', 'lmmse_blind', 'lmmse_levinson')


def measure(npkt, nt=32, nr=4, reps=5):
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(pkg.synth.hadamard(nt))
    d_re, d_im, _, _, _ = e.synth_structured(3, 0, npkt, snr_db=10.0, want_channel=False, want_noise_std=False)
    shape = (npkt, nr, nt, 234)
    h_re, h_im, o_re, o_im = (e.empty(shape) for _ in range(4))
    e.ls_estimate_device(d_re, d_im, npkt, h_re, h_im)
    from dl_channel_estimation_mamimo_amd import sweep
    prof = sweep.tap_profile(8)
    hv = e.to_device(np.tile(prof, (npkt, 1)))
    snr = e.to_device(np.full((npkt, nr), 10.0, np.float32))

    def run():
        e.lmmse_blind_device(d_re, d_im, h_re, h_im, npkt, o_re, o_im)
        e.lmmse_estimate_device(h_re, h_im, npkt, hv, prof.size, snr, o_re, o_im)
    run()                                            # sizes the workspace, loads the code
    e.synchronize()
    e.profile_enable(True)
    e.profile_reset()
    for _ in range(reps):
        run()
    e.synchronize()
    p = e.profile()
    e.profile_enable(False)
    lines = []
    for k in KERNELS:
        ms = p[k]['ms'] / p[k]['launches']
        lines.append('  %-18s %9.3f ms per call  %7.3f us per packet  %6.2f TFLOP/s fp64 (counted flops)' % (
            k, ms, ms / npkt * 1e3, p[k]['flops'] / p[k]['launches'] / ms / 1e9))
    stats = (p['lmmse_null_noise']['ms'] + p['lmmse_freq_corr']['ms']) / reps
    blind = p['lmmse_blind']['ms'] / reps
    lines.append('  statistics kernels together %.3f ms = %.2f x the blind recursion (%.3f ms); blind total %.3f ms = %.2f x csi_lmmse_estimate_device' % (
        stats, stats / blind, blind, stats + blind, (stats + blind) / (p['lmmse_levinson']['ms'] / reps)))
    lines.append('  fallbacks counted: %d' % e.get_option('lmmse_blind_fallbacks'))
    return lines


if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, 'profiles', 'lmmse_blind.txt')
    text = ['blind LMMSE smoother, Nt = 32, Nr = 4, 10 dB packets of csi_synth_structured; HIP-event time per kernel, mean of 5 calls',
            '(lmmse_blind includes the one-workgroup fallback count behind it; lmmse_levinson = csi_lmmse_estimate_device, the yardstick)']
    for npkt in (500, 4000):
        text.append('%d packets:' % npkt)
        text += measure(npkt)
    print('\n'.join(text))
    with open(out, 'w') as f:
        f.write('\n'.join(text) + '\n')
