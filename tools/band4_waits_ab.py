#!/usr/bin/env python3
"""A / B / A' of the split-f16 band kernel's LDS-wait schedule (csrc/band4_kernel_gen.py RoleH, flags 'lw' / 'ex') in ONE process on one device, at the
headline shape and input as bench.py builds them (Nt = 32, Nr = 4, 4000 packets, 500 at each of 8 SNR levels, the shipped model, fp32 context).

Three contexts, every one through the library's code-object hook (CSI_DEBUG_HOOKS / CSI_BAND8_HSACO / CSI_BAND8_NAME, read when a context first loads its
band kernels; "band4" = 0 routes the call to the hooked slot, a name csi_band4* makes it a 256-thread launch on tiled weights):
    A  = csi_band4_oldwaits (no flag: the schedule with three full LDS drains per sub-step - the yardstick),  B = --b (default csi_band4),  A' = A again.
Arms are interleaved per round.  Per arm and round: the whole step (ls_estimate_device + predict_device, then synchronize) by the host clock with the
per-kernel events off, and the band launch from the library's own HIP events (profile()['pair_dense_gemm']) with them on.  "band4_launches" must advance
in every arm, and B's outputs must equal A's bit for bit (the flags move waits, not arithmetic).
Noise = the A / A' spread: |median(A) - median(A')|.  A flag is kept only if B beats A by at least FIVE times that spread on the launch AND on the step.

    tools/build_band8.sh && python tools/band4_waits_ab.py [--b csi_band4_lw] [--rounds 10] [--steps 20]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--a', default='csi_band4_oldwaits')
    ap.add_argument('--b', default='csi_band4')
    ap.add_argument('--hsaco', default=os.path.join(REPO, 'tools', 'band8.hsaco'))
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--nt', type=int, default=32)
    ap.add_argument('--nr', type=int, default=4)
    ap.add_argument('--packets', type=int, default=4000)
    ap.add_argument('--hidden', type=int, nargs='+', default=[1024, 1024])
    args = ap.parse_args()
    os.environ['CSI_DEBUG_HOOKS'] = '1'
    os.environ['CSI_BAND8_HSACO'] = os.path.abspath(args.hsaco)
    assert os.path.exists(args.hsaco), 'build the code object of every variant first: tools/build_band8.sh'
    import dl_channel_estimation_mamimo_amd as pkg

    nt, nr, npkt, hidden = args.nt, args.nr, args.packets, tuple(args.hidden)
    assert npkt % 8 == 0
    P = pkg.synth.hadamard(nt)
    blocks = list(pkg.synth.mixed_snr_batch(2024 + 1, nr, P, per_level=npkt // 8))
    arms = []
    for label, kname in (('A ', args.a), ('B ', args.b), ("A'", args.a)):
        os.environ['CSI_BAND8_NAME'] = kname               # read by this context's first band call (the warm-up below)
        eng = pkg.CsiEngine(nt, nr, hidden=hidden, n_out=234, use_bn=True, dtype='f32')
        rng = np.random.default_rng(1234)
        eng.load_weights('real', pkg.synth.make_weights(rng, nt, hidden))
        eng.load_weights('imag', pkg.synth.make_weights(rng, nt, hidden))
        eng.set_pilot(P)
        eng.set_option('band4', 0)
        d_re, d_im = eng.empty((npkt, nr, eng.len_ltf)), eng.empty((npkt, nr, eng.len_ltf))
        for p0, snr, blk in blocks:
            d_re.upload(np.ascontiguousarray(blk.real), first=p0)
            d_im.upload(np.ascontiguousarray(blk.imag), first=p0)
        outs = [eng.empty((npkt, nr, nt, 234)) for _ in range(4)]

        def step(eng=eng, d_re=d_re, d_im=d_im, outs=outs):
            eng.ls_estimate_device(d_re, d_im, npkt, outs[2], outs[3])
            eng.predict_device(d_re, d_im, npkt, outs[0], outs[1])

        n0 = eng.get_option('band4_launches')
        for _ in range(args.warmup):
            step()
        eng.synchronize()
        assert eng.get_option('band4_launches') == n0 + 2 * args.warmup, '%s: %s did not serve the call as a csi_band4* launch' % (label, kname)
        arms.append(dict(label=label, kernel=kname, eng=eng, step=step, outs=outs, step_ms=[], launch_ms=[]))

    pick = list(range(0, npkt, max(npkt // 16, 1)))
    ref = [np.concatenate([arms[0]['outs'][k].download(p, 1) for p in pick]) for k in range(2)]
    for arm in arms[1:]:
        for k in range(2):
            got = np.concatenate([arm['outs'][k].download(p, 1) for p in pick])
            assert np.array_equal(got, ref[k]), '%s (%s): outputs differ from A\'s' % (arm['label'], arm['kernel'])

    for rd in range(args.rounds):
        for arm in arms:
            eng, step = arm['eng'], arm['step']
            c0 = eng.get_option('band4_launches')
            step(); eng.synchronize()
            eng.profile_enable(False)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            eng.synchronize()
            arm['step_ms'].append((time.perf_counter() - t0) / args.steps * 1e3)
            eng.profile_enable(True)
            eng.profile_reset()
            for _ in range(args.steps):
                step()
            eng.synchronize()
            p = eng.profile()['pair_dense_gemm']
            eng.profile_enable(False)
            arm['launch_ms'].append(p['ms'] / max(p['launches'], 1))
            assert eng.get_option('band4_launches') == c0 + 2 * (2 * args.steps + 1), arm['label']

    def stats(v):
        v = np.asarray(v)
        return float(np.median(v)), float(v.min()), float(np.percentile(v, 75) - np.percentile(v, 25))

    print('band4_waits_ab: A = %s, B = %s; nt %d nr %d packets %d hidden %s, %d rounds of %d steps, arms interleaved per round' % (
        args.a, args.b, nt, nr, npkt, 'x'.join(map(str, hidden)), args.rounds, args.steps))
    print('%-3s | band launch ms: median   min     iqr   | step ms: median   min     iqr' % 'arm')
    res = []
    for arm in arms:
        k, s = stats(arm['launch_ms']), stats(arm['step_ms'])
        res.append((k, s))
        print('%-3s |               %8.4f %7.4f %7.4f |        %8.4f %7.4f %7.4f' % ((arm['label'],) + k + s))
    for arm in arms:
        print('%-3s rounds  launch: %s' % (arm['label'], ' '.join('%.4f' % x for x in arm['launch_ms'])))
        print('%-3s rounds  step:   %s' % (arm['label'], ' '.join('%.4f' % x for x in arm['step_ms'])))
    (ka, sa), (kb, sb), (kc, sc) = res
    k_noise, s_noise = abs(ka[0] - kc[0]), abs(sa[0] - sc[0])
    k_gain, s_gain = ka[0] - kb[0], sa[0] - sb[0]
    print('A / A\' spread: launch %.4f ms, step %.4f ms' % (k_noise, s_noise))
    print('gain of B over A: launch %.4f ms (%.2f %%, %.1f x spread), step %.4f ms (%.2f %%, %.1f x spread)' % (
        k_gain, 100 * k_gain / ka[0], k_gain / max(k_noise, 1e-9), s_gain, 100 * s_gain / sa[0], s_gain / max(s_noise, 1e-9)))
    ok = k_gain >= 5 * k_noise and s_gain >= 5 * s_noise and k_gain > 0 and s_gain > 0
    print('rule (B below A by >= 5 x the A / A\' spread on the launch and on the step): %s' % ('B qualifies' if ok else 'A stays'))


if __name__ == '__main__':
    main()
