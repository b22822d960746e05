"""Host replay of csi_synth_structured (csrc/synth_structured.hip.h), numpy only.  Written from the formulas in that header, not
from a device run; the hash and the normal draw are tests/train_streams.py's (the device's tr_normal), everything else is fp64.

    key(p, kind) = splitmix64(seed ^ splitmix64(2 p + kind))            p = absolute packet index, kind 0 = taps, 1 = noise
    tap   (r, j, t) = normal(key(p, 0), ((r Nt + j) 64 + t) 2 + {0, 1}) * decay[t],   decay[t] = fp32(exp(-t / 2) / sqrt(2))
    noise (r, n)    = normal(key(p, 1), (r len_ltf + n) 2 + {0, 1})
    H[j][f] = sum_t c[j][t] exp(-2 pi i f t / 256);  X[s][f] = ltf[f] sum_j H[j][f] P[j][s];  x[s] = ifft(X[s]);  symbol = x[192:] | x
    pow = mean |x|^2 over the packet;  noise_std = sqrt(pow * fp32(0.5 * 10^(-snr / 10)));  out = amp (x + noise_std z)
    h[j][q] = amp H[j][f(q)] on the 234 data bins;  amp = fp32(sqrt(242) / 256) or 1"""
import numpy as np

import train_streams as ts
from oracle import csi_oracle as o

MAX_TAPS = 64
AMP = float(np.float32(np.sqrt(242.0) / 256.0))


def key(seed, pkt, kind):
    inner = int(ts.splitmix64(np.uint64((2 * int(pkt) + kind) & ts.MASK64)))
    return int(ts.splitmix64(np.uint64((int(seed) & ts.MASK64) ^ inner)))


def decay(n_taps):
    return (np.exp(-0.5 * np.arange(n_taps)) / np.sqrt(2.0)).astype(np.float32).astype(np.float64)


def noise_factor(snr_db):
    """0.5 * 10^(-snr/10) as the library hands it to the device: from the fp32 level, in double, rounded to fp32"""
    s = np.asarray(snr_db, np.float32).astype(np.float64)
    return (0.5 * 10.0 ** (-0.1 * s)).astype(np.float32).astype(np.float64)


def taps(seed, pkt, nr, nt, n_taps):
    """complex128 [nr, nt, n_taps]"""
    r, j, t = np.meshgrid(np.arange(nr), np.arange(nt), np.arange(n_taps), indexing='ij')
    pos = (((r * nt + j) * MAX_TAPS + t) * 2).astype(np.uint64)
    k = key(seed, pkt, 0)
    re, _ = ts.normal(k, pos)
    im, _ = ts.normal(k, pos + np.uint64(1))
    return (re + 1j * im) * decay(n_taps)


def noise_normals(seed, pkt, nr, len_ltf, with_radius=False):
    """complex128 [nr, len_ltf] standard normals per real component (and their Box-Muller radii, same layout)"""
    pos = (np.arange(nr * len_ltf, dtype=np.uint64) * np.uint64(2)).reshape(nr, len_ltf)
    k = key(seed, pkt, 1)
    re, rre = ts.normal(k, pos)
    im, rim = ts.normal(k, pos + np.uint64(1))
    return (re + 1j * im, rre + 1j * rim) if with_radius else re + 1j * im


def replay(seed, first_pkt, npkt, nr, P, snr_db=None, n_taps=8, amp_scale=True):
    """The packets [first_pkt, first_pkt + npkt) of stream `seed`.  Returns a dict:
    ltf complex128 [npkt, nr, 320 nt], clean (the same without noise), h complex128 [npkt, nr, nt, 234], noise_std [npkt] (before the
    amplitude scale), z / radius complex128 [npkt, nr, 320 nt] (the normals and radii of the noise draw; None when noise-free)."""
    P = np.asarray(P, np.float32).astype(np.float64)
    nt = P.shape[0]
    len_ltf = o.SYM_LEN * nt
    amp = AMP if amp_scale else 1.0
    ltf_seq = np.fft.ifftshift(o.vht_ltf_256())                       # FFT bin order
    fbin = (o.data_carrier_indices() - 1 + o.FFT_LEN // 2) % o.FFT_LEN
    clean = np.empty((npkt, nr, len_ltf), np.complex128)
    h = np.empty((npkt, nr, nt, o.N_DATA), np.complex128)
    z = rad = None
    if snr_db is not None:
        fac = noise_factor(np.broadcast_to(np.asarray(snr_db, np.float32), (npkt,)))
        z, rad = np.empty_like(clean), np.empty_like(clean)
    for i in range(npkt):
        c = taps(seed, first_pkt + i, nr, nt, n_taps)
        H = np.fft.fft(c, n=o.FFT_LEN, axis=-1)                       # [r, j, f]
        X = np.einsum('rjf,js->rsf', H, P) * ltf_seq
        x = np.fft.ifft(X, axis=-1)
        clean[i] = np.concatenate([x[..., -o.CP_LEN:], x], axis=-1).reshape(nr, len_ltf)
        h[i] = amp * H[..., fbin]
        if z is not None:
            z[i], rad[i] = noise_normals(seed, first_pkt + i, nr, len_ltf, with_radius=True)
    power = np.mean(np.abs(clean) ** 2, axis=(1, 2))
    if z is None:
        return dict(ltf=amp * clean, clean=amp * clean, h=h, noise_std=np.zeros(npkt), z=None, radius=None, power=power)
    std = np.sqrt(power * fac)
    return dict(ltf=amp * (clean + std[:, None, None] * z), clean=amp * clean, h=h, noise_std=std, z=z, radius=rad, power=power)
