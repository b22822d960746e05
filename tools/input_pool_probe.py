#!/usr/bin/env python3
"""Decimated-input models (csi_set_input_pool) on the part: per-step time of none / max / avg, measured interleaved in ONE process
(rounds of none, max, avg, none, ... on the same device-resident preambles), then one profiled call per mode for the pooling
pass (ms, GB/s) and the layer-0 kernels.  Shapes: config 2 (fp32, Nt=32 Nr=4, 4000 packets, LS + both DNNs as one
csi_estimate_device call), configs[2] (bf16, Nt=64 Nr=4, 5000 packets) and the one-packet call of config 2's model (queued calls).
usage: input_pool_probe.py [rounds]   (env CONFIGS=c2,c3,one to pick)"""
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dl_channel_estimation_mamimo_amd as pkg

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
MODES = (None, 'max', 'avg')


def weights(rng, nt, hidden, mode):
    w = pkg.synth.make_weights(rng, nt, hidden)
    if mode:
        k = w['fc_dense0.kernel']
        w['fc_dense0.kernel'] = np.ascontiguousarray(np.concatenate([k[:160 * nt], k[320 * nt:]], axis=0))
    return w


def engines(nt, nr, hidden, dtype):
    out = {}
    for mode in MODES:
        rng = np.random.default_rng(0)
        e = pkg.CsiEngine(nt, nr, hidden=hidden, dtype=dtype, input_pool=mode)
        e.load_weights('real', weights(rng, nt, hidden, mode))
        e.load_weights('imag', weights(rng, nt, hidden, mode))
        e.set_pilot(pkg.synth.hadamard(nt))
        out[mode] = e
    return out


def run(name, nt, nr, npkt, hidden, dtype, calls):
    es = engines(nt, nr, hidden, dtype)
    bufs = {}
    for mode, e in es.items():
        d_re, d_im = e.empty((npkt, nr, e.len_ltf)), e.empty((npkt, nr, e.len_ltf))
        e.synth_white(1, 0, npkt, d_re, d_im)
        o = [e.empty((npkt, nr, nt, 234)) for _ in range(4)]
        bufs[mode] = (d_re, d_im, o)
        for _ in range(3):
            e.estimate_device(d_re, d_im, npkt, *o)
        e.synchronize()
    ts = {m: [] for m in MODES}
    for _ in range(ROUNDS):
        for mode, e in es.items():
            d_re, d_im, o = bufs[mode]
            e.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                e.estimate_device(d_re, d_im, npkt, *o)
            e.synchronize()
            ts[mode].append((time.perf_counter() - t0) / calls * 1e3)
    base = np.median(ts[None])
    print(f'== {name}: Nt={nt} Nr={nr} {npkt} packets, hidden {hidden}, {dtype}; {ROUNDS} interleaved rounds of {calls} queued calls')
    for mode in MODES:
        med = np.median(ts[mode])
        print(f'   {mode or "none":5s} {med * (1e3 if npkt == 1 else 1):10.3f} {"us" if npkt == 1 else "ms"} per call   '
              f'(min {min(ts[mode]):.4f} max {max(ts[mode]):.4f} ms)   ratio to none {med / base:.4f}')
    for mode, e in es.items():
        d_re, d_im, o = bufs[mode]
        e.profile_enable(True)
        e.profile_reset()
        e.estimate_device(d_re, d_im, npkt, *o)
        e.synchronize()
        prof = e.profile()
        e.profile_enable(False)
        pool = prof['input_pool']
        l0 = prof['layer0_ltf_gemm']
        gbs = pool['bytes'] / (pool['ms'] * 1e-3) / 1e9 if pool['ms'] > 0 else 0.0
        print(f'   {mode or "none":5s} profiled: input_pool {pool["launches"]} launches {pool["ms"]:.4f} ms {gbs:8.1f} GB/s   '
              f'layer0_ltf_gemm {l0["launches"]} launches {l0["ms"]:.4f} ms   cast_bf16 {prof["cast_bf16"]["ms"]:.4f} ms   '
              f'all kernels {sum(v["ms"] for v in prof.values()):.4f} ms ({sum(v["launches"] for v in prof.values())} launches)')
        top = sorted(((v['ms'], k) for k, v in prof.items() if v['ms'] > 0), reverse=True)[:6]
        print('         ' + '  '.join(f'{k} {ms:.3f}' for ms, k in top))
    for e in es.values():
        e.close()


if __name__ == '__main__':
    want = os.environ.get('CONFIGS', 'c2,c3,one').split(',')
    if 'c2' in want:
        run('config 2', 32, 4, 4000, (1024, 1024), 'f32', 5)
    if 'c3' in want:
        run('configs[2]', 64, 4, 5000, (1024, 1024), 'bf16', 3)
    if 'one' in want:
        run('one-packet call', 32, 4, 1, (1024, 1024), 'f32', 200)
