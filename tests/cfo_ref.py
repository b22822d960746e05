"""The fp64 statement of the carrier-frequency-offset stage (csrc/cfo.hip.h): the rotation that impairs or corrects a
sounding preamble and the cyclic-prefix estimator.  x complex [npkt, nr, 320 nt], n = 320 s + m (64 samples of prefix, 256 of body);
eps in subcarrier spacings (cycles per 256 samples), one per packet."""
import numpy as np

SYM, CP, FFT = 320, 64, 256


def rotate(x, eps, scale=1.0):
    """y[p, r, n] = x[p, r, n] exp(2 pi i scale eps[p] n / 256), complex128."""
    x = np.asarray(x, np.complex128)
    n = np.arange(x.shape[-1], dtype=np.float64)
    turns = (float(scale) * np.asarray(eps, np.float64))[:, None] * n[None, :] / FFT
    return x * np.exp(2j * np.pi * (turns - np.rint(turns)))[:, None, :]


def correlate(x, cp_skip=0):
    """(gamma complex128 [npkt], E float64 [npkt]) over the samples cp_skip .. 63 of every prefix and their twins 256 samples on."""
    x = np.asarray(x, np.complex128)
    npkt, nr, ln = x.shape
    sym = x.reshape(npkt, nr, ln // SYM, SYM)
    a, b = sym[..., cp_skip:CP], sym[..., FFT + cp_skip:FFT + CP]
    gamma = np.sum(np.conj(a) * b, axis=(1, 2, 3))
    energy = 0.5 * np.sum(np.abs(a) ** 2 + np.abs(b) ** 2, axis=(1, 2, 3))
    return gamma, energy


def estimate(x, cp_skip=0):
    """(eps_hat float64 [npkt], quality float64 [npkt]); a packet without energy gives (0, 0)."""
    gamma, energy = correlate(x, cp_skip)
    some = energy > 0
    eps = np.where(some, np.arctan2(gamma.imag, gamma.real) / (2.0 * np.pi), 0.0)
    quality = np.where(some, np.abs(gamma) / np.where(some, energy, 1.0), 0.0)
    return eps, quality


def correct(x, cp_skip=0):
    """(rotate(x, eps_hat, -1), eps_hat, quality)."""
    eps, quality = estimate(x, cp_skip)
    return rotate(x, eps, -1.0), eps, quality


def wrap(d):
    """d modulo 1 into [-1/2, 1/2]."""
    d = np.asarray(d, np.float64)
    return d - np.rint(d)
