#!/usr/bin/env python3
"""sweep_fp64_check.py - the miniature sweep of tests/test_gpu_sweep.py::test_miniature_pipeline_end_to_end without a device: the
replayed packets of csi_synth_structured (tests/synth_streams.py, per-packet noise), LS labels from the fp64 oracle, both component
models trained by the fp64 oracle trainer (Glorot start, Adam, BatchNormalization, AWGN on the LTF columns at a random level of
trainer.SNR_LEVELS_MAMIMO per batch relative to the first batch's power, best validation weights kept), then NMSE_subk of LS and of the
DNN per level.  Says whether the orderings the GPU test gates (DNN below LS at -20 and -10 dB) hold in exact arithmetic.
usage: sweep_fp64_check.py [seed ...]"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import synth_streams as ss                      # noqa: E402
from oracle import csi_oracle as o              # noqa: E402

NT, NR, HIDDEN, N_TRAIN, N_TEST, BS, LR, EPOCHS = 4, 2, (64, 32), 96, 16, 64, 1e-3, 30
LEVELS = (-20.0, -10.0, 10.0)
SNR_TRAIN = (30, 20, 10, 0, -10, -20)


def glorot(rng, d_in):
    w = o.make_weights(rng, d_in, list(HIDDEN), 234, dtype=np.float64)
    for k in list(w):
        if k.endswith('.bias') or k.endswith('.beta') or k.endswith('moving_mean'):
            w[k] = np.zeros_like(w[k])
        elif k.endswith('.gamma') or k.endswith('moving_variance'):
            w[k] = np.ones_like(w[k])
    return w


def fit(rng, x, y, n_val):
    xt, yt, xv, yv = x[:-n_val], y[:-n_val], x[-n_val:], y[-n_val:]
    w = glorot(rng, x.shape[1])
    w.pop('bn_eps')
    state = o.adam_init(w)
    L = o.SYM_LEN * NT
    avg_pow = float(np.mean(np.mean(xt[:BS, :L] ** 2, axis=1)))
    best, best_w = np.inf, None
    for _ in range(EPOCHS):
        order = rng.permutation(xt.shape[0])
        for b in range(xt.shape[0] // BS):
            ids = order[b * BS:(b + 1) * BS]
            std = np.sqrt(avg_pow / 10.0 ** (rng.choice(SNR_TRAIN) / 10.0)) / np.sqrt(2.0)
            noise = np.zeros((BS, x.shape[1]))
            noise[:, :L] = std * rng.standard_normal((BS, L))
            _, w, _ = o.train_step_reference(w, state, xt[ids], yt[ids], lr=LR, noise=noise)
        val = o.eval_loss_reference(w, xv, yv)
        if val < best:
            best, best_w = val, dict(w)
    return best_w


def main(seeds):
    P = o.hadamard(NT)
    for seed in seeds:
        tr = ss.replay(seed, 0, N_TRAIN, NR, P, snr_db=None)
        labels = o.ls_estimate(tr['ltf'], P)
        n_val = int(np.floor(N_TRAIN * 0.15)) * NR * NT
        rng = np.random.default_rng(seed)
        w = {}
        for d in ('real', 'imag'):
            x = o.samples_from_packets(tr['ltf'], P, d)
            y = (labels.real if d == 'real' else labels.imag).reshape(-1, 234)
            w[d] = fit(rng, x, y, n_val)
        for i, snr in enumerate(LEVELS):
            te = ss.replay(seed + 1, N_TRAIN + i * N_TEST, N_TEST, NR, P, snr_db=snr)
            ls = o.ls_estimate(te['ltf'], P)
            r_re, r_im = o.predict_packets(te['ltf'], P, w['real'], w['imag'], np.float64, pkt_batch=N_TEST)
            m_ls = np.mean([o.nmse_subk(te['h'][p], ls[p]) for p in range(N_TEST)])
            m_dnn = np.mean([o.nmse_subk(te['h'][p], (r_re + 1j * r_im)[p]) for p in range(N_TEST)])
            print('seed %d  %+4.0f dB: LS %.4g  DNN %.4g  (%s)' % (seed, snr, m_ls, m_dnn, 'DNN below LS' if m_dnn < m_ls else 'LS below DNN'))


if __name__ == '__main__':
    main([int(a) for a in sys.argv[1:]] or [1, 2, 3])
