"""The fp64 statement of the symbol-timing stage (csrc/sync.hip.h): the embedding of a packet at theta inside a
capture (with the replayed margin draws), the cyclic-prefix timing metric, the estimate and the cut-out.  x complex
[npkt, nr, 320 nt]; captures complex [npkt, nr, 320 nt + span]; theta in 0 .. span and eps in subcarrier spacings, one per packet."""
import numpy as np

import cfo_ref as cr
import synth_streams as st
import train_streams as ts

SYM, CP, FFT = cr.SYM, cr.CP, cr.FFT
MARGIN_TAG = 0x53594E43


def clamp(theta, span):
    return np.clip(np.asarray(theta, np.int64), 0, int(span))


def margin_key(seed, pkt):
    """km = splitmix64(kn ^ tag), kn the kind-1 noise key of the absolute packet index"""
    return int(ts.splitmix64(np.uint64(st.key(seed, pkt, 1) ^ MARGIN_TAG)))


def margin_normals(seed, pkt, nr, L):
    """(z complex128 [nr, L], radius complex128 [nr, L]): the standard normals per real component of every capture sample of one
    packet (only the samples outside the packet are used) and their Box-Muller radii"""
    pos = (np.arange(nr * L, dtype=np.uint64) * np.uint64(2)).reshape(nr, L)
    k = margin_key(seed, pkt)
    re, rre = ts.normal(k, pos)
    im, rim = ts.normal(k, pos + np.uint64(1))
    return re + 1j * im, rre + 1j * rim


def embed(x, theta, span, seed=0, first_pkt=0, std=None):
    """c[p, r, theta[p] + n] = x[p, r, n]; every other sample std[p] z[p, r, n] (zero without std).  Returns (capture, inside) with
    inside bool [npkt, L] true on the packet's samples."""
    x = np.asarray(x)
    npkt, nr, ln = x.shape
    L = ln + int(span)
    th = clamp(theta, span)
    cap = np.zeros((npkt, nr, L), np.complex128)
    inside = np.zeros((npkt, L), bool)
    for p in range(npkt):
        if std is not None and std[p] != 0:
            cap[p] = float(std[p]) * margin_normals(seed, first_pkt + p, nr, L)[0]
        cap[p, :, th[p]:th[p] + ln] = x[p]
        inside[p, th[p]:th[p] + ln] = True
    return cap, inside


def metric(cap, span, rho=1.0):
    """(Lambda float64 [npkt, span + 1], gamma complex128 [npkt, span + 1], Phi float64 [npkt, span + 1])"""
    cap = np.asarray(cap, np.complex128)
    npkt, nr, L = cap.shape
    span = int(span)
    nt = (L - span) // SYM
    J = span + CP
    sym = np.stack([cap[..., SYM * s:SYM * s + J + FFT] for s in range(nt)], axis=2)      # [p, r, s, J + 256]
    a, b = sym[..., :J], sym[..., FFT:FFT + J]
    q = np.sum(np.conj(a) * b, axis=(1, 2))                                               # [p, J]
    e = 0.5 * np.sum(np.abs(a) ** 2 + np.abs(b) ** 2, axis=(1, 2))
    win = np.arange(span + 1)[:, None] + np.arange(CP)[None, :]                           # [theta, m]
    gamma, phi = q[:, win].sum(-1), e[:, win].sum(-1)
    return np.abs(gamma) - float(rho) * phi, gamma, phi


def estimate(cap, span, rho=1.0):
    """(theta_hat int64 [npkt], eps_hat float64, quality float64, Lambda, Phi); Phi == 0 at theta_hat gives eps_hat = quality = 0"""
    lam, gamma, phi = metric(cap, span, rho)
    th = np.argmax(lam, axis=1)                       # the lowest index of the largest value
    idx = np.arange(lam.shape[0])
    g, f = gamma[idx, th], phi[idx, th]
    some = f > 0
    eps = np.where(some, np.arctan2(g.imag, g.real) / (2.0 * np.pi), 0.0)
    quality = np.where(some, np.abs(g) / np.where(some, f, 1.0), 0.0)
    return th, eps, quality, lam, phi


def extract(cap, theta, span, eps=None):
    """y[p, r, n] = c[p, r, theta[p] + n] exp(-2 pi i eps[p] n / 256), n < L - span"""
    cap = np.asarray(cap)
    ln = cap.shape[-1] - int(span)
    th = clamp(theta, span)
    y = np.stack([cap[p, :, th[p]:th[p] + ln] for p in range(cap.shape[0])])
    return y if eps is None else cr.rotate(y, eps, -1.0)


def runner_up_gap(lam):
    """the largest Lambda minus the largest of the others, per packet"""
    s = np.sort(lam, axis=1)
    return s[:, -1] - s[:, -2]
