#!/usr/bin/env python3
"""Hybrid beamforming weights (csi_hybrid_weights_device) on the part: time per call and per kernel at Nt 32, Nr 4, 4000 packets,
500 rays for (Ns, NtRF) = (1, 1) and (2, 4); the correlation kernel's rate against the fp32 matrix peak, the singular-vector kernel's
read rate; beside them the same call stated in torch on the same GPU (torch.linalg.svd, batched matmul, argmax, linalg.solve).
Warm-up, then CALLS timed calls (HIP events of the library's per-kernel profile for the kernels, host clock around queued calls
for the whole call).
usage: hybrid_probe.py [calls] [--no-torch] [--packets N]
   rocprofv3 --kernel-trace --stats -d OUT -- python tools/hybrid_probe.py 3 --no-torch       (kernel trace, a run of its own)
   rocprofv3 --pmc SQ_WAVES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES ... -- python tools/hybrid_probe.py 1 --no-torch   (counters, a run of their own)"""
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dl_channel_estimation_mamimo_amd as pkg

ARGS = [a for a in sys.argv[1:] if not a.startswith('--')]
CALLS = int(ARGS[0]) if ARGS else 20
NPKT = int(sys.argv[sys.argv.index('--packets') + 1]) if '--packets' in sys.argv else 4000
NT, NR, RAYS = 32, 4, 500
PEAK_F32_MATRIX = 157.3e12
KERNELS = ('hybrid_svd', 'hybrid_corr_argmax', 'hybrid_solve', 'hybrid_finish')


def torch_statement(h_re, h_im, At, ns, ntrf, calls):
    """the same computation in torch on the same GPU, in packet blocks that fit; returns ms per call"""
    import torch
    dev = torch.device('cuda:0')
    H = torch.complex(torch.from_numpy(h_re), torch.from_numpy(h_im)).to(dev).permute(0, 3, 1, 2).reshape(-1, NR, NT).contiguous()
    A = torch.from_numpy(At).to(dev)
    Ah = A.conj().T.contiguous()
    block = 234 * 500

    def once():
        for i0 in range(0, H.shape[0], block):
            Hb = H[i0:i0 + block]
            _, _, vh = torch.linalg.svd(Hb, full_matrices=False)
            fopt = vh[:, :ns, :].conj().transpose(1, 2).contiguous()
            res = fopt
            idx = []
            for m in range(ntrf):
                psi = Ah @ res
                idx.append((psi.real ** 2 + psi.imag ** 2).sum(-1).argmax(-1))
                Am = A.T[torch.stack(idx, 1)].transpose(1, 2)
                Amh = Am.conj().transpose(1, 2)
                C = torch.linalg.solve(Amh @ Am, Amh @ fopt)
                T = fopt - Am @ C
                res = T / torch.linalg.norm(T, dim=(1, 2), keepdim=True)
            fbb = (ns ** 0.5) * C / torch.linalg.norm(Am @ C, dim=(1, 2), keepdim=True)
        return fbb
    once()
    torch.cuda.synchronize()
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(calls):
        once()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / calls


def main():
    if '--no-torch' not in sys.argv:
        import torch                                  # before the library: one HIP runtime per process, torch's goes first
        torch.cuda.init()
    P = pkg.synth.hadamard(NT)
    az, el = pkg.synth.random_rays(np.random.default_rng(5), RAYS)
    At = pkg.synth.steering_ula(NT, az, el).astype(np.complex64)
    e = pkg.CsiEngine(NT, NR, hidden=(8,), device=0)
    e.set_pilot(P)
    e.set_dictionary(At)
    # the CSI planes are the LS estimates of structured packets at 0 dB, computed where they stay: on the device
    d_re, d_im = e.empty((NPKT, NR, NT, 234)), e.empty((NPKT, NR, NT, 234))
    h_re, h_im = np.empty((NPKT, NR, NT, 234), np.float32), np.empty((NPKT, NR, NT, 234), np.float32)
    for s, p0 in enumerate(range(0, NPKT, 500)):
        n = min(500, NPKT - p0)
        ltf = pkg.synth.structured_packets(np.random.default_rng(s), n, NR, P, 0.0)
        l_re, l_im = e.to_device(np.ascontiguousarray(ltf.real)), e.to_device(np.ascontiguousarray(ltf.imag))
        o_re, o_im = e.empty((n, NR, NT, 234)), e.empty((n, NR, NT, 234))
        e.ls_estimate_device(l_re, l_im, n, o_re, o_im)
        e.synchronize()
        h_re[p0:p0 + n], h_im[p0:p0 + n] = o_re.download(), o_im.download()
        for d in (l_re, l_im, o_re, o_im):
            d.free()
    d_re.upload(h_re)
    d_im.upload(h_im)
    items = NPKT * 234
    print(f'== hybrid weights: Nt={NT} Nr={NR} {NPKT} packets ({items} items), {RAYS} rays; {CALLS} timed calls')
    for ns, ntrf in ((1, 1), (2, 4)):
        d_f = [e.empty((NPKT, 234, ns, ntrf)) for _ in range(2)]
        d_idx, d_na, d_gain = e.empty((NPKT, 234, ntrf)), e.empty((NPKT, 234)), e.empty((NPKT, 234))
        d_m = [e.empty((NPKT, ntrf, NT)) for _ in range(2)]

        def call():
            e.hybrid_weights_device(d_re, d_im, NPKT, ns, ntrf, d_f[0], d_f[1], d_idx, d_na, d_gain, d_m[0], d_m[1])
        for _ in range(3):
            call()
        e.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        e.synchronize()
        ms = (time.perf_counter() - t0) / CALLS * 1e3
        e.profile_enable(True)
        e.profile_reset()
        for _ in range(CALLS):
            call()
        e.synchronize()
        prof = e.profile()
        e.profile_enable(False)
        print(f'   (Ns, NtRF) = ({ns}, {ntrf}): {ms:.3f} ms per call ({items / ms / 1e3:.1f} M items/s)')
        for k in KERNELS:
            p = prof[k]
            per = p['ms'] / CALLS
            extra = ''
            if k == 'hybrid_corr_argmax' and per > 0:
                tf = p['flops'] / CALLS / (per * 1e-3)
                extra = f'   {tf / 1e12:.1f} Tflop/s = {100 * tf / PEAK_F32_MATRIX:.1f} % of the fp32 matrix peak'
            if k == 'hybrid_svd' and per > 0:
                extra = f'   reads H at {items * NR * NT * 8 / (per * 1e-3) / 1e9:.0f} GB/s (one pass over the CSI planes)'
            print(f'      {k:20s} {p["launches"] // CALLS:3d} launches {per:8.3f} ms per call{extra}')
        if '--no-torch' not in sys.argv:
            t_ms = torch_statement(h_re, h_im, At, ns, ntrf, max(1, CALLS // 10))
            print(f'      the same call stated in torch (linalg.svd, matmul, argmax, linalg.solve): {t_ms:.1f} ms per call = {t_ms / ms:.1f} x')
        for d in d_f + [d_idx, d_na, d_gain] + d_m:
            d.free()
    e.close()


if __name__ == '__main__':
    main()
