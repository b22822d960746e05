"""Host replay of csi_synth_scattering (csrc/synth_scattering.hip.h), numpy only.  Written from the model as include/csi_mamimo.h
states it, not from a device run and not from synth.scattering_channel (which the CPU tests compare with this file): scatterer by
scatterer, in plain loops.  The draws are the device's fp32 values (tests/train_streams.py uniform / normal under the key function of
tests/synth_streams.py) and the configuration is rounded to fp32 as the library receives it; all further arithmetic is fp64.

    kc = key(seed, p, 0);  user (random_users): u0..u2 = uniform(kc, 0..2), R = 1 + (range - 1) u0, az = 180 (2 u1 - 1), el = 90 (2 u2 - 1)
    scatterer s, b = 8 (s + 1):  o_s[i] = box_frac R (2 uniform(kc, b + i) - 1),  g_s = (normal(kc, b + 3) + i normal(kc, b + 4)) / sqrt(2)
    q = R e + o;  x = (2 R e.o + |o|^2) / (|q| + R) + |o|;  tau_s = (x_s - min x) fs / c;  tau_abs = (R + x) fs / c;  v = q_y / |q|;  w = o_y / |o|
    H[r][j][f] = S^(-1/2) sum_s g_s exp(2 pi i z_r w_s) exp(-2 pi i y_j v_s) exp(-2 pi i f tau_s / 256),  f signed
    packets, noise and h exactly as tests/synth_streams.py builds them from H"""
import math

import numpy as np

import synth_streams as ss
import train_streams as ts
from oracle import csi_oracle as o

C = 299792458.0


def _f32(x):
    return float(np.float32(x))


def draws(seed, pkt, n_scat):
    """(user uniforms [3], box uniforms [S][3], g complex [S]) of packet `pkt`: the device's fp32 draws as float64"""
    kc = ss.key(seed, pkt, 0)
    uu = ts.uniform(kc, np.arange(3, dtype=np.uint64)).astype(np.float64)
    base = 8 * (np.arange(n_scat, dtype=np.uint64) + np.uint64(1))
    u = np.stack([ts.uniform(kc, base + np.uint64(i)).astype(np.float64) for i in range(3)], axis=1)
    gr, _ = ts.normal(kc, base + np.uint64(3))
    gi, _ = ts.normal(kc, base + np.uint64(4))
    return uu, u, (gr + 1j * gi) / math.sqrt(2.0)


def user(uu, range_m, az_deg, el_deg, random_users):
    if random_users:
        return 1.0 + (_f32(range_m) - 1.0) * uu[0], 180.0 * (2.0 * uu[1] - 1.0), 90.0 * (2.0 * uu[2] - 1.0)
    return _f32(range_m), _f32(az_deg), _f32(el_deg)


def geometry(u, R, az_deg, el_deg, box_frac, sample_rate_hz):
    """per scatterer: x (excess path, stable form), tau (excess delay, samples), tau_abs, v, w"""
    az, el = math.radians(az_deg), math.radians(el_deg)
    e = (math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el))
    spm = _f32(sample_rate_hz) / C
    S = u.shape[0]
    x, v, w = np.empty(S), np.empty(S), np.empty(S)
    for s in range(S):
        off = [_f32(box_frac) * R * (2.0 * u[s, i] - 1.0) for i in range(3)]
        q = [R * e[i] + off[i] for i in range(3)]
        on = math.sqrt(sum(c * c for c in off))
        qn = math.sqrt(sum(c * c for c in q))
        x[s] = (2.0 * R * sum(e[i] * off[i] for i in range(3)) + on * on) / (qn + R) + on
        v[s] = q[1] / qn
        w[s] = off[1] / on if on > 0 else 0.0
    return dict(x=x, tau=(x - x.min()) * spm, tau_abs=(R + x) * spm, v=v, w=w)


def response(g, geo, nr, nt):
    """H complex128 [nr][nt][256] in FFT bin order"""
    S = g.size
    f = np.concatenate([np.arange(128), np.arange(-128, 0)]).astype(np.float64)
    y = (np.arange(nt) - (nt - 1) / 2.0) / 2.0
    H = np.zeros((nr, nt, o.FFT_LEN), np.complex128)
    for s in range(S):
        delay = np.exp(-2j * np.pi * f * geo['tau'][s] / 256.0)
        for r in range(nr):
            zr = (r - (nr - 1) / 2.0) / 2.0
            a = g[s] * np.exp(2j * np.pi * zr * geo['w'][s])
            H[r] += (a * np.exp(-2j * np.pi * y * geo['v'][s]))[:, None] * delay[None, :]
    return H / math.sqrt(S)


def replay(seed, first_pkt, npkt, nr, P, snr_db=None, n_scat=100, range_m=100.0, az_deg=30.0, el_deg=0.0, box_frac=0.1,
           random_users=False, amp_scale=True, sample_rate_hz=100e6):
    """The packets [first_pkt, first_pkt + npkt) of stream `seed`.  The dict of synth_streams.replay (ltf, clean, h, noise_std, z,
    radius, power) plus H [npkt, nr, nt, 256], tau [npkt, S] (absolute, samples), tau_excess, v, w [npkt, S], g [npkt, S]."""
    P = np.asarray(P, np.float32).astype(np.float64)
    nt = P.shape[0]
    len_ltf = o.SYM_LEN * nt
    amp = ss.AMP if amp_scale else 1.0
    ltf_seq = np.fft.ifftshift(o.vht_ltf_256())
    fbin = (o.data_carrier_indices() - 1 + o.FFT_LEN // 2) % o.FFT_LEN
    clean = np.empty((npkt, nr, len_ltf), np.complex128)
    h = np.empty((npkt, nr, nt, o.N_DATA), np.complex128)
    Hs = np.empty((npkt, nr, nt, o.FFT_LEN), np.complex128)
    per = {k: np.empty((npkt, n_scat)) for k in ('tau_abs', 'tau', 'v', 'w')}
    gs = np.empty((npkt, n_scat), np.complex128)
    z = rad = None
    if snr_db is not None:
        fac = ss.noise_factor(np.broadcast_to(np.asarray(snr_db, np.float32), (npkt,)))
        z, rad = np.empty_like(clean), np.empty_like(clean)
    for i in range(npkt):
        uu, u, g = draws(seed, first_pkt + i, n_scat)
        R, az, el = user(uu, range_m, az_deg, el_deg, random_users)
        geo = geometry(u, R, az, el, box_frac, sample_rate_hz)
        H = response(g, geo, nr, nt)
        X = np.einsum('rjf,js->rsf', H, P) * ltf_seq
        x = np.fft.ifft(X, axis=-1)
        clean[i] = np.concatenate([x[..., -o.CP_LEN:], x], axis=-1).reshape(nr, len_ltf)
        h[i] = amp * H[..., fbin]
        Hs[i], gs[i] = H, g
        for k in per:
            per[k][i] = geo[k]
        if z is not None:
            z[i], rad[i] = ss.noise_normals(seed, first_pkt + i, nr, len_ltf, with_radius=True)
    power = np.mean(np.abs(clean) ** 2, axis=(1, 2))
    out = dict(clean=amp * clean, h=h, H=Hs, tau=per['tau_abs'], tau_excess=per['tau'], v=per['v'], w=per['w'], g=gs, power=power)
    if z is None:
        return dict(out, ltf=amp * clean, noise_std=np.zeros(npkt), z=None, radius=None)
    std = np.sqrt(power * fac)
    return dict(out, ltf=amp * (clean + std[:, None, None] * z), noise_std=std, z=z, radius=rad)
