#!/usr/bin/env python3
"""scatter_probe.py - the measurements behind profiles/synth_scattering.txt (GPU box; not part of a test or of bench.py).

    python tools/scatter_probe.py [timing] [gain]        (default: both)

  timing   csi_synth_scattering (S = 100) at Nt = 32, Nr = 4, 4000 packets and at Nt = 128, Nr = 16, 400 packets: device time per call
           from the library's HIP events after warm-up, noise-free and noisy, ltf + channel planes; csi_synth_structured at the same
           shapes in the same process (the yardstick); bytes written over that time against a write-only float4 fill of the same size
           timed in this process (torch)
  gain     Nt = 32, Nr = 4, 500 packets at 0 dB, 500 rays, (ns, ntrf) = (1, 1): dtSNR of the hybrid weights of the true planes
           ("perfect") and of the LS estimate, for the tap channel and for the scattering channel"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def fill_rate(nbytes):
    """write-only fill in TB/s for nbytes of output, timed with events in this process"""
    import torch
    a = torch.empty(nbytes // 4, dtype=torch.float32, device='cuda')
    for _ in range(3):
        a.fill_(1.0)
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(10):
        a.fill_(1.0)
    end.record()
    torch.cuda.synchronize()
    rate = nbytes / (beg.elapsed_time(end) / 10 * 1e-3) / 1e12
    del a
    torch.cuda.empty_cache()
    return rate


def timing(nt, nr, npkt, n_scat=100):
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import dl_channel_estimation_mamimo_amd as pkg
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(pkg.synth.hadamard(nt))
    snr = np.repeat(np.asarray(pkg.synth.SNR_LEVELS_DB, np.float32), (npkt + 7) // 8)[:npkt]
    nbytes = 8 * npkt * nr * (320 * nt + nt * 234)
    fill = fill_rate(nbytes)
    print(f'== Nt={nt} Nr={nr} {npkt} packets, S={n_scat}: ltf + channel planes {nbytes / 1e9:.3f} GB; a write-only fill of that size reaches {fill:.2f} TB/s here')
    for entry, call in (('synth_structured', lambda s: e.synth_structured(1, 0, npkt, snr_db=s)),
                        ('synth_scattering', lambda s: e.synth_scattering(1, 0, npkt, snr_db=s, n_scat=n_scat))):
        for label, s in (('noise-free', None), ('noisy (power pass + packet pass)', snr)):
            def run():
                arrs = call(s)
                e.synchronize()
                for a in arrs:
                    if a is not None:
                        a.free()
            run()
            run()
            e.profile_enable(True)
            e.profile_reset()
            calls = 5
            for _ in range(calls):
                run()
            p = e.profile()[entry]
            e.profile_enable(False)
            ms = p['ms'] / calls
            rate = p['bytes'] / calls / (ms * 1e-3) / 1e12
            print(f'   {entry:18s} {label:34s} {ms:9.3f} ms device time per call   {rate:6.3f} TB/s written = {rate / fill:.3f} of the fill rate')
    e.close()


def gain(npkt=500, rays=500):
    import dl_channel_estimation_mamimo_amd as pkg
    from dl_channel_estimation_mamimo_amd import sweep
    nt, nr = 32, 4
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(pkg.synth.hadamard(nt))
    az, el = pkg.synth.random_rays(np.random.default_rng(0), rays)
    e.set_dictionary(pkg.synth.steering_ula(nt, az, el))
    print(f'== Nt={nt} Nr={nr} {npkt} packets at 0 dB, {rays} rays, (ns, ntrf) = (1, 1), QPSK, 10 symbols')
    for name, arrs in (('taps (csi_synth_structured)', e.synth_structured(1, 0, npkt, snr_db=0.0)),
                       ('scattering (csi_synth_scattering, S = 100, range 100 m)', e.synth_scattering(1, 0, npkt, snr_db=0.0)[:5])):
        d_re, d_im, h_re, h_im, d_std = arrs
        l_re, l_im = e.empty((npkt, nr, nt, 234)), e.empty((npkt, nr, nt, 234))
        e.ls_estimate_device(d_re, d_im, npkt, l_re, l_im)
        out = sweep.link_level(e, dict(LS=(l_re, l_im), perfect=(h_re, h_im)), h_re, h_im, d_std, npkt, 1, 0, ns=1, ntrf=1)
        print(f'   {name:58s} dtSNR_perfect {out["dtSNR_perfect"].mean():6.2f} dB ({out["dtSNR_perfect"].min():.2f} .. {out["dtSNR_perfect"].max():.2f}), '
              f'dtSNR_LS {out["dtSNR_LS"].mean():6.2f} dB, BER perfect {out["bers_perfect"].mean():.3e}, BER LS {out["bers_LS"].mean():.3e}   '
              f'(array gain 10 log10({nt}) = {10 * np.log10(nt):.2f} dB)')
        for a in arrs + (l_re, l_im):
            a.free()
    e.close()


if __name__ == '__main__':
    what = sys.argv[1:] or ['timing', 'gain']
    if not set(what) <= {'timing', 'gain'}:
        raise SystemExit(__doc__)
    if 'timing' in what:
        timing(32, 4, 4000)
        timing(128, 16, 400)
    if 'gain' in what:
        gain()
