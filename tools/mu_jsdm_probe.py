#!/usr/bin/env python3
"""mu_jsdm_probe.py - the timings of profiles/mu_jsdm.txt (GPU box; not part of a test or of bench.py).

    python tools/mu_jsdm_probe.py [-o OUT.txt] [NPKT ...]        (default 4000)

Nt = 32, Nr = 4, (U, ns, r_star, b) = (4, 1, 4, 2) and (4, 2, 4, 4), every user its own group, rank_tol 0.05, per-group processing:
known-channel packets at 10 dB per user (csi_synth_structured, stream 1 + u), then csi_mu_jsdm_precoder_device and, on the same true
planes with the same number of RF chains and 500 random rays, csi_mu_hybrid_precoder_device.  Device time per call of the profile
entries mu_cov, mu_jsdm_eig (both launches), mu_jsdm_baseband and mu_hybrid_precoder from the library's HIP events after warm-up; for
the covariance kernel the rate of the definition's flops (8 Nt^2 Nr 234 per packet and user) against the fp32 matrix peak (157.3
Tflop/s), beside mu_beam_score's 0.47 - 0.48 (profiles/mu_hybrid.txt); for the eigen kernel the time per matrix."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
FP32_MATRIX_PEAK = 157.3e12


def main(argv):
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import dl_channel_estimation_mamimo_amd as pkg
    out = None
    if argv[:1] == ['-o']:
        out, argv = argv[1], argv[2:]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nt, nr, rays, calls = 32, 4, 500, 5
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(pkg.synth.hadamard(nt))
    az, el = pkg.synth.random_rays(np.random.default_rng(0), rays)
    e.set_dictionary(pkg.synth.steering_ula(nt, az, el))
    say('multi-user JSDM precoder (csi_mu_jsdm_precoder_device) beside csi_mu_hybrid_precoder_device: HIP-event time per call, mean of %d calls after two warm-up calls' % calls)
    for npkt in [int(a) for a in argv] or [4000]:
        users = []
        for u in range(4):
            d_re, d_im, h_re, h_im, d_std = e.synth_structured(1 + u, 0, npkt, snr_db=10.0)
            for a in (d_re, d_im, d_std):
                a.free()
            users.append((h_re, h_im))
        say('== Nt=%d Nr=%d %d packets' % (nt, nr, npkt))
        for nu, ns, r_star, b in ((4, 1, 4, 2), (4, 2, 4, 4)):
            m, n_rf = nu * ns, nu * b
            h_re, h_im = [x[0] for x in users[:nu]], [x[1] for x in users[:nu]]
            w = [e.empty((npkt, m, nt, 234)) for _ in range(2)]
            d_idx, d_rank = e.empty((npkt, n_rf)), e.empty((npkt, nu, 2))

            def both():
                e.mu_jsdm_precoder_device(h_re, h_im, npkt, ns, r_star, b, w[0], w[1], rank_tol=0.05, flags=e.JSDM_PGP, d_rank=d_rank)
                e.mu_hybrid_precoder_device(h_re, h_im, npkt, ns, n_rf, w[0], w[1], d_idx)

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
            t = {k: prof[k]['ms'] / calls for k in ('mu_cov', 'mu_jsdm_eig', 'mu_jsdm_baseband', 'mu_hybrid_precoder')}
            flops = npkt * nu * 8.0 * nt * nt * nr * 234.0
            rank = d_rank.download().view(np.int32)
            say('   (U, ns, r_star, b) = (%d, %d, %d, %d), n_rf = %d: mu_cov %.3f ms (%.3f Tflop of the definition: %.1f Tflop/s = %.2f of the fp32 matrix peak), '
                'mu_jsdm_eig %.3f ms for %d matrices of both stages (%.2f us per matrix), mu_jsdm_baseband %.3f ms; mu_hybrid_precoder (same planes, '
                'same n_rf) %.3f ms; mean r_g %.2f, q_g %.2f'
                % (nu, ns, r_star, b, n_rf, t['mu_cov'], flops / 1e12, flops / (t['mu_cov'] * 1e-3) / 1e12, flops / (t['mu_cov'] * 1e-3) / FP32_MATRIX_PEAK,
                   t['mu_jsdm_eig'], 2 * npkt * nu, t['mu_jsdm_eig'] * 1e3 / (2 * npkt * nu), t['mu_jsdm_baseband'], t['mu_hybrid_precoder'],
                   rank[..., 0].mean(), rank[..., 1].mean()))
            for a in w + [d_idx, d_rank]:
                a.free()
        for h_re, h_im in users:
            h_re.free(); h_im.free()
    if out:
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
