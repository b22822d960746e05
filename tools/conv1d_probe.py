#!/usr/bin/env python3
"""CONV1D models (csi_set_model_type, conv_frontend.hip.h) on the part: FC and CONV1D contexts of the same shape measured interleaved in
ONE process (rounds of FC, CONV1D, FC, ... on device-resident preambles, csi_predict_device), then one profiled call of each for the
per-kernel split: the front end's write rate against the 6.29 TB/s float4-copy rate, and layer 0's rate per flop against the FC
model's layer 0.  Nt = 32, Nr = 4.
usage: conv1d_probe.py [--hidden 256,128] [--dtype f32|bf16] [--packets 1,64,500,4000] [--rounds 3]"""
import argparse
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dl_channel_estimation_mamimo_amd as pkg

NT, NR = 32, 4
COPY_TBS = 6.29


def weights(rng, nt, hidden, conv):
    """glorot-like random weights of either model (float32, no BN: the shape of the work is what counts here)"""
    d_in = (64 if conv else 1) * 320 * nt + nt
    w, fan = {}, d_in
    for i, h in enumerate(hidden):
        lim = np.float32(np.sqrt(6.0 / (fan + h)))
        w[f'fc_dense{i}.kernel'] = (rng.random((fan, h), dtype=np.float32) * 2 - 1) * lim
        w[f'fc_dense{i}.bias'] = (0.01 * rng.standard_normal(h)).astype(np.float32)
        fan = h
    w['fc_regressor.kernel'] = ((rng.random((fan, 234), dtype=np.float32) * 2 - 1) * np.float32(np.sqrt(6.0 / (fan + 234))))
    w['fc_regressor.bias'] = np.zeros(234, np.float32)
    if conv:
        w['cnn1d_1.kernel'] = rng.uniform(-0.3, 0.3, (7, 1, 128)).astype(np.float32)
        w['cnn1d_1.bias'] = (0.05 * rng.standard_normal(128)).astype(np.float32)
        w['conv_bn.gamma'] = rng.uniform(0.5, 1.5, 128).astype(np.float32)
        w['conv_bn.beta'] = (0.1 * rng.standard_normal(128)).astype(np.float32)
        w['conv_bn.moving_mean'] = (0.1 * rng.standard_normal(128)).astype(np.float32)
        w['conv_bn.moving_variance'] = rng.uniform(0.5, 1.5, 128).astype(np.float32)
    return w


def engine(hidden, dtype, model):
    rng = np.random.default_rng(0)
    e = pkg.CsiEngine(NT, NR, hidden=hidden, use_bn=False, dtype=dtype, model=model)
    for d in ('real', 'imag'):
        e.load_weights(d, weights(rng, NT, hidden, model == 'CONV1D'))
    e.set_pilot(pkg.synth.hadamard(NT))
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hidden', default='256,128')
    ap.add_argument('--dtype', default='f32')
    ap.add_argument('--packets', default='1,64,500,4000')
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    hidden = tuple(int(h) for h in a.hidden.split(','))
    t0 = time.perf_counter()
    es = {m: engine(hidden, a.dtype, m) for m in ('FC', 'CONV1D')}
    print(f'== Nt={NT} Nr={NR} hidden {hidden} {a.dtype}: contexts ready in {time.perf_counter() - t0:.1f} s', flush=True)
    for npkt in (int(p) for p in a.packets.split(',')):
        calls = 20 if npkt <= 64 else (4 if npkt <= 500 else 2)
        bufs = {}
        for m, e in es.items():
            d_re, d_im = e.empty((npkt, NR, e.len_ltf)), e.empty((npkt, NR, e.len_ltf))
            e.synth_white(1, 0, npkt, d_re, d_im)
            o = [e.empty((npkt, NR, NT, 234)) for _ in range(2)]
            bufs[m] = (d_re, d_im, o)
            for _ in range(2):
                e.predict_device(d_re, d_im, npkt, *o)
            e.synchronize()
        ts = {m: [] for m in es}
        for _ in range(a.rounds):
            for m, e in es.items():
                d_re, d_im, o = bufs[m]
                e.synchronize()
                t1 = time.perf_counter()
                for _ in range(calls):
                    e.predict_device(d_re, d_im, npkt, *o)
                e.synchronize()
                ts[m].append((time.perf_counter() - t1) / calls * 1e3)
        fc_ms = float(np.median(ts['FC']))
        print(f'-- {npkt} packets ({npkt * NR} preambles), {a.rounds} interleaved rounds of {calls} queued calls', flush=True)
        for m in es:
            med = float(np.median(ts[m]))
            print(f'   {m:6s} {med:10.4f} ms per call (min {min(ts[m]):.4f} max {max(ts[m]):.4f})   ratio to FC {med / fc_ms:8.2f}')
        l0_rate = {}
        for m, e in es.items():
            d_re, d_im, o = bufs[m]
            e.profile_enable(True)
            e.profile_reset()
            e.predict_device(d_re, d_im, npkt, *o)
            e.synchronize()
            prof = e.profile()
            e.profile_enable(False)
            l0 = prof['layer0_ltf_gemm']
            l0_rate[m] = l0['flops'] / (l0['ms'] * 1e-3) / 1e12 if l0['ms'] > 0 else 0.0
            total = sum(v['ms'] for v in prof.values())
            print(f'   {m:6s} profiled: all kernels {total:.4f} ms ({sum(v["launches"] for v in prof.values())} launches); '
                  f'layer0_ltf_gemm {l0["launches"]} launches {l0["ms"]:.4f} ms {l0_rate[m]:.2f} TFLOP/s', flush=True)
            if m == 'CONV1D':
                cf = prof['conv_frontend']
                feat_bytes = 2 * npkt * NR * 64 * e.len_ltf * (2 if a.dtype == 'bf16' else 4)        # both models' features
                tbs = feat_bytes / (cf['ms'] * 1e-3) / 1e12 if cf['ms'] > 0 else 0.0
                print(f'          conv_frontend {cf["launches"]} launches {cf["ms"]:.4f} ms: {feat_bytes / 1e9:.3f} GB of features written = '
                      f'{tbs:.2f} TB/s = {tbs / COPY_TBS:.2f} of the {COPY_TBS} TB/s copy rate; front end {cf["ms"] / total:.2f} of the '
                      f'kernel time, layer 0 {l0["ms"] / total:.2f}')
            top = sorted(((v['ms'], k, v['launches']) for k, v in prof.items() if v['ms'] > 0), reverse=True)[:7]
            print('          ' + '  '.join(f'{k} {ms:.3f} ({n})' for ms, k, n in top))
        if l0_rate['FC'] > 0:
            print(f'   layer 0 rate per flop CONV1D / FC: {l0_rate["CONV1D"] / l0_rate["FC"]:.2f}', flush=True)
        for m in es:
            d_re, d_im, o = bufs[m]
            for b in (d_re, d_im, *o):
                b.free()
    for e in es.values():
        e.close()


if __name__ == '__main__':
    main()
