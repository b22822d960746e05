"""Host replay of csi_scatter_channel_at_device (csrc/scatter_aged.hip.h), numpy only: the fp64 statement of the aged
scattering channel, built on the draws, the user and the geometry of tests/scatter_ref.py (imported, not copied) and written from the
model as include/csi_mamimo.h states it, scatterer by scatterer.

    m = (cos el cos az, cos el sin az, sin el) of the heading; random heading: az = 180 (2 uniform(kc, 3) - 1) degrees per packet
    o_s = box_frac R (2 u_s - 1);  nu_s = speed carrier / c  (m . o_s) / |o_s|   (0 for a zero offset)
    H_t[r][j][f] = S^(-1/2) sum_s g_s exp(+2 pi i nu_s t) exp(2 pi i z_r w_s) exp(-2 pi i y_j v_s) exp(-2 pi i f tau_s / 256)
    h_t = amp H_t on the 234 data bins

The configured floats are rounded to fp32 as the library receives them (scatter_ref._f32); the times stay double."""
import math

import numpy as np

import scatter_ref as sr
import synth_streams as ss
import train_streams as ts
from oracle import csi_oracle as o


def heading_uniform(seed, pkt):
    """index 3 of the channel stream of packet `pkt`: the draw of a random heading, as float64"""
    return float(ts.uniform(ss.key(seed, pkt, 0), np.arange(4, dtype=np.uint64))[3])


def heading(heading_az_deg, heading_el_deg, random_heading=False, u3=None):
    """(m, azimuth in degrees): the unit vector of the motion in the transmitter's frame"""
    az = 180.0 * (2.0 * u3 - 1.0) if random_heading else sr._f32(heading_az_deg)
    a, e = math.radians(az), math.radians(sr._f32(heading_el_deg))
    return np.array([math.cos(e) * math.cos(a), math.cos(e) * math.sin(a), math.sin(e)]), az


def offsets(u, R, box_frac):
    """o_s [S][3]: the scatterers' offsets from the receiver, as scatter_ref.geometry forms them"""
    return np.array([[sr._f32(box_frac) * R * (2.0 * u[s, i] - 1.0) for i in range(3)] for s in range(u.shape[0])])


def doppler(off, m, speed_mps, carrier_hz):
    """nu_s [S] in Hz: the last leg of path s shortens at speed (m . o_s) / |o_s| metres per second"""
    nu = np.zeros(off.shape[0])
    for s in range(off.shape[0]):
        on = math.sqrt(sum(c * c for c in off[s]))
        if on > 0:
            nu[s] = sr._f32(speed_mps) * sr._f32(carrier_hz) / sr.C * sum(m[i] * off[s, i] for i in range(3)) / on
    return nu


def response_at(g, geo, nu, t, nr, nt):
    """H_t complex128 [nr][nt][256] in FFT bin order: scatter_ref.response with g_s exp(2 pi i nu_s t) in the place of g_s"""
    turns = nu * float(t)
    return sr.response(g * np.exp(2j * np.pi * (turns - np.rint(turns))), geo, nr, nt)


def replay(seed, first_pkt, npkt, nr, P, times_s, speed_mps=0.0, heading_az_deg=0.0, heading_el_deg=0.0, carrier_hz=28e9, random_heading=False,
           n_scat=100, range_m=100.0, az_deg=30.0, el_deg=0.0, box_frac=0.1, random_users=False, amp_scale=True, sample_rate_hz=100e6):
    """The packets [first_pkt, first_pkt + npkt) of stream `seed` at the times times_s: dict of h [n_times, npkt, nr, nt, 234],
    nu [npkt, S] (Hz), off [npkt, S, 3], m [npkt, 3], heading_az [npkt] (degrees), tau_excess [npkt, S] and g [npkt, S].  P only gives Nt."""
    nt = np.asarray(P).shape[0]
    times = np.atleast_1d(np.asarray(times_s, np.float64))
    amp = ss.AMP if amp_scale else 1.0
    fbin = (o.data_carrier_indices() - 1 + o.FFT_LEN // 2) % o.FFT_LEN
    h = np.empty((times.size, npkt, nr, nt, o.N_DATA), np.complex128)
    out = dict(h=h, nu=np.empty((npkt, n_scat)), off=np.empty((npkt, n_scat, 3)), m=np.empty((npkt, 3)), heading_az=np.empty(npkt),
               tau_excess=np.empty((npkt, n_scat)), g=np.empty((npkt, n_scat), np.complex128))
    for i in range(npkt):
        uu, u, g = sr.draws(seed, first_pkt + i, n_scat)
        R, az, el = sr.user(uu, range_m, az_deg, el_deg, random_users)
        geo = sr.geometry(u, R, az, el, box_frac, sample_rate_hz)
        m, maz = heading(heading_az_deg, heading_el_deg, random_heading, heading_uniform(seed, first_pkt + i))
        off = offsets(u, R, box_frac)
        nu = doppler(off, m, speed_mps, carrier_hz)
        for k, t in enumerate(times):
            h[k, i] = amp * response_at(g, geo, nu, t, nr, nt)[..., fbin]
        out['nu'][i], out['off'][i], out['m'][i], out['heading_az'][i], out['tau_excess'][i], out['g'][i] = nu, off, m, maz, geo['tau'], g
    return out
