#!/usr/bin/env python3
"""A / B / A' of the split-f16 layer-0 kernel's MFMA shape ("hs_l0_mfma": 32 = v_mfma_f32_32x32x16_f16, 16 = the 16x16x32 form on pairs
of sub-tiles, gemm_hs.hip.h) in ONE process on one device: the headline shape and input as bench.py builds them (Nt = 32, Nr = 4, 4000
packets, 500 at each of 8 SNR levels, the shipped model, fp32 context, automatic engine choice).

Arms are interleaved per round: A = 32, B = 16, A' = 32 again.  Per arm and round
  * the whole step (ls_estimate_device + predict_device, then synchronize) by the host clock, per-kernel events OFF, `--steps` steps;
  * layer 0's time per launch from the library's own HIP events (profile()['layer0_ltf_gemm']), events ON, `--steps` steps.
Reported: median and minimum over the rounds.  The noise of the measurement is the larger of |median(A) - median(A')| and the
interquartile range of A's rounds.  Rule for the default: B below A by more than THREE times the noise on the kernel time AND the step
time moving the same way by more than its own noise.

    python tools/l0_shape_ab.py [--rounds 10] [--steps 20] [--nt 32 --nr 4 --packets 4000 --input mixed-snr|white]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--nt', type=int, default=32)
    ap.add_argument('--nr', type=int, default=4)
    ap.add_argument('--packets', type=int, default=4000)
    ap.add_argument('--hidden', type=int, nargs='+', default=[1024, 1024])
    ap.add_argument('--input', default='mixed-snr', choices=['mixed-snr', 'white'])
    args = ap.parse_args()
    import dl_channel_estimation_mamimo_amd as pkg

    nt, nr, npkt, hidden = args.nt, args.nr, args.packets, tuple(args.hidden)
    eng = pkg.CsiEngine(nt, nr, hidden=hidden, n_out=234, use_bn=True, dtype='f32')
    rng = np.random.default_rng(1234)
    eng.load_weights('real', pkg.synth.make_weights(rng, nt, hidden))
    eng.load_weights('imag', pkg.synth.make_weights(rng, nt, hidden))
    P = pkg.synth.hadamard(nt)
    eng.set_pilot(P)
    d_re, d_im = eng.empty((npkt, nr, eng.len_ltf)), eng.empty((npkt, nr, eng.len_ltf))
    if args.input == 'mixed-snr':
        assert npkt % 8 == 0
        for p0, snr, blk in pkg.synth.mixed_snr_batch(2024 + 1, nr, P, per_level=npkt // 8):
            d_re.upload(np.ascontiguousarray(blk.real), first=p0)
            d_im.upload(np.ascontiguousarray(blk.imag), first=p0)
    else:
        eng.synth_white(2024 + 1, 0, npkt, d_re, d_im)
    d_ore, d_oim = eng.empty((npkt, nr, nt, 234)), eng.empty((npkt, nr, nt, 234))
    d_hre, d_him = eng.empty((npkt, nr, nt, 234)), eng.empty((npkt, nr, nt, 234))
    eng.synchronize()

    def step():
        eng.ls_estimate_device(d_re, d_im, npkt, d_hre, d_him)
        eng.predict_device(d_re, d_im, npkt, d_ore, d_oim)

    arms = [('A  32', 32), ('B  16', 16), ("A' 32", 32)]
    for _, form in arms[:2]:
        eng.set_option('hs_l0_mfma', form)
        for _ in range(args.warmup):
            step()
        eng.synchronize()
    n16 = eng.get_option('hs_l0_mfma16_launches')
    assert n16 > 0, 'the 16 form was not taken at this shape'

    step_ms = {a: [] for a, _ in arms}
    l0_ms = {a: [] for a, _ in arms}
    for rd in range(args.rounds):
        for name, form in arms:
            eng.set_option('hs_l0_mfma', form)
            c0 = eng.get_option('hs_l0_mfma16_launches')
            step(); eng.synchronize()
            eng.profile_enable(False)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            eng.synchronize()
            step_ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
            eng.profile_enable(True)
            eng.profile_reset()
            for _ in range(args.steps):
                step()
            eng.synchronize()
            p = eng.profile()['layer0_ltf_gemm']
            eng.profile_enable(False)
            l0_ms[name].append(p['ms'] / max(p['launches'], 1))
            took16 = eng.get_option('hs_l0_mfma16_launches') > c0
            assert took16 == (form == 16), (name, form)

    def stats(v):
        v = np.asarray(v)
        return float(np.median(v)), float(v.min()), float(np.percentile(v, 75) - np.percentile(v, 25))

    print('l0_shape_ab: nt %d nr %d packets %d (%s) hidden %s, %d rounds of %d steps, arms interleaved per round' % (
        nt, nr, npkt, args.input, 'x'.join(map(str, hidden)), args.rounds, args.steps))
    print('%-6s | layer 0 ms per launch: median   min     iqr   | step ms: median   min     iqr' % 'arm')
    res = {}
    for name, _ in arms:
        k, s = stats(l0_ms[name]), stats(step_ms[name])
        res[name] = (k, s)
        print('%-6s |                      %8.4f %7.4f %7.4f |        %8.4f %7.4f %7.4f' % ((name,) + k + s))
    for name, _ in arms:
        print('%-6s rounds  layer 0: %s' % (name, ' '.join('%.4f' % x for x in l0_ms[name])))
        print('%-6s rounds  step:    %s' % (name, ' '.join('%.4f' % x for x in step_ms[name])))
    (ka, sa), (kb, sb), (kc, sc) = res['A  32'], res['B  16'], res["A' 32"]
    k_noise = max(abs(ka[0] - kc[0]), ka[2])
    s_noise = max(abs(sa[0] - sc[0]), sa[2])
    k_gain, s_gain = ka[0] - kb[0], sa[0] - sb[0]
    print('noise: layer 0 %.4f ms (|A - A\'| %.4f, iqr(A) %.4f), step %.4f ms (|A - A\'| %.4f, iqr(A) %.4f)' % (
        k_noise, abs(ka[0] - kc[0]), ka[2], s_noise, abs(sa[0] - sc[0]), sa[2]))
    print('gain of 16 over 32: layer 0 %.4f ms per launch (%.1f %%, %.1f x noise), step %.4f ms (%.2f %%, %.1f x noise)' % (
        k_gain, 100 * k_gain / ka[0], k_gain / max(k_noise, 1e-9), s_gain, 100 * s_gain / sa[0], s_gain / max(s_noise, 1e-9)))
    ok = k_gain > 3 * k_noise and s_gain > s_noise
    print('rule (layer 0 gain > 3 x noise and step gain > its noise): %s' % ('16 qualifies as the default' if ok else '32 stays the default'))


if __name__ == '__main__':
    main()
