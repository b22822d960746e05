// scatter_aged.hip.h - the true channel of csi_synth_scattering's packets at later (or earlier) times, for a user that moves
// (csi_scatter_channel_at_device).
//
// Packet p of stream `seed` keeps the scatterers, coefficients g_s, delays tau_s and direction cosines v_s, w_s of
// synth_scattering.hip.h: the same draws of kc = ss_key(seed, p, 0), nothing moved.  The transmitter and the scatterers stand still; the
// user moves with speed_mps along the unit vector m = (cos el cos az, cos el sin az, sin el) of heading_az_deg / heading_el_deg in the
// transmitter's frame (the frame of az_deg / el_deg).  Only the last leg of path s changes: with o_s the scatterer's offset from the
// receiver it shortens at speed (m . o_s / |o_s|) metres per second, so
//   nu_s = speed_mps carrier_hz / c  (m . o_s) / |o_s|      (0 for a zero offset; c = 299792458)
//   H_t[r][j][f] = S^(-1/2) sum_s g_s exp(+2 pi i nu_s t) exp(2 pi i z_r w_s) exp(-2 pi i y_j v_s) exp(-2 pi i f tau_s / 256)
//   h_t = amp H_t on the 234 data bins in the LS layout; h_0 is what csi_synth_scattering returns, bit for bit.
// The model is FIRST ORDER: delays and direction cosines are frozen at their t = 0 values.  That is good while speed |t| is small
// against the scatterer box box_frac R (millimetres against metres for walking speed and milliseconds); nothing is refused on it.
// Random heading (motion flag bit 0): the azimuth of m is 180 (2 tr_uniform(kc, 3) - 1) degrees per packet, the elevation stays as
// configured.  Index 3 of the channel stream is otherwise unused (the user takes 0 .. 2, scatterer s starts at 8 (s + 1)).
//
// One workgroup of 256 lanes per (packet, rx), one launch per call, no symbol spectra, no inverse transform, no noise, no power pass.
//   setup    once, synth_scattering_kernel's restated operation for operation (that file stays as it is, so that its kernels stay the
//            same machine code): lane s draws scatterer s, fp64 geometry, c_s = g_s exp(2 pi i z_r w_s) / sqrt(S), the 16 phasors
//            B[b] = exp(-2 pi i y_b v_s), tl[s] = tau_s / 256 - and nu_s in fp64
//   per chunk of 16 antennas and per time t:
//            d_s(t) = exp(2 pi i nu_s t): the product nu_s t in fp64, reduced in fp64 (x - rint(x)), rounded once to fp32 for sincospif
//            table T_t[s][b] = ((c_s d_s(t)) exp(-2 pi i (j0 / 2) v_s)) B[b]; lane q sums T_t[s][.] exp(-2 pi i f(q) tau_s / 256) over s
//            (sc_accumulate); the chunk goes through LDS times amp and leaves as 16-byte vectors
// At t = 0 the phasor is exactly (1, 0) (a static user has none), c_s passes through unchanged and every later operation is the parent's.
// The times are kernel arguments (no upload: the call can be captured).  Planar re / im, no complex types, compiled without packed
// fp32, no scratch.
#pragma once
#include "synth_scattering.hip.h"      // SC_DEV, SC_ROW, sc_sync, sc_phasor, sc_accumulate

namespace csi {

constexpr int SA_MAX_TIMES = 16;

struct ScatterAgedArgs {
    const int* bin_pos;      // [234] FFT bin of data bin q
    float* h_re;             // [n_times][npkt][nr][nt][234]
    float* h_im;
    uint64_t seed;
    int64_t first_pkt;
    int nt, nr, n_scat, n_times;
    int random_users, random_heading;
    float amp;
    float range_m, box_frac;
    float ex, ey, ez;        // user direction of the configured az / el (fixed users)
    float spm;               // samples per metre fs / c
    float gscale;            // 1 / sqrt(2 n_scat)
    double dop;              // speed carrier / c: the Doppler shift of a path that shortens at the full speed, Hz
    double mx, my, mz;       // heading m (fixed heading); with a random heading mz = sin el and mce = cos el are used
    double mce;
    double t[SA_MAX_TIMES];  // seconds
};

__host__ __device__ inline size_t scatter_aged_lds_floats(int n_scat) {
    return (size_t)LS_FFT + (size_t)2 * SS_CH * LS_NDATA + (size_t)((n_scat + 3) & ~3) + (size_t)n_scat * SC_ROW;
}

// MOVING = false serves a static user (speed 0): no Doppler phasor at all, the channel block is the parent's as it stands.  The kernel is a
// template also for where that puts it: instantiations are emitted behind every plain kernel of the translation unit, so adding this
// one moves no existing kernel and no pc-relative address inside one (tools/device_code_diff.py).
template <bool MOVING>
__global__ SC_NO_PK __launch_bounds__(SS_THREADS) void scatter_aged_kernel(const ScatterAgedArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int nt = a.nt, S = a.n_scat;
    int* binp = reinterpret_cast<int*>(smem);             // [256] data-bin table
    float* F = smem + LS_FFT;                             // [2][SS_CH][234] the channel chunk on its way out; the excess paths (fp64) during the setup
    float* tl = F + 2 * SS_CH * LS_NDATA;                 // [S] tau_s / 256
    float* tab = tl + ((S + 3) & ~3);                     // [S][SC_ROW] chunk table T_t
    double* xs = reinterpret_cast<double*>(F);

    const int tid = threadIdx.x;
    const size_t blk = blockIdx.x;
    const int64_t pl = (int64_t)(blk / a.nr);             // packet of this call
    const int r = (int)(blk - (size_t)pl * a.nr);
    const uint64_t pkt = (uint64_t)(a.first_pkt + pl);

    if (tid < LS_NDATA) binp[tid] = a.bin_pos[tid];

    // ---- scatterer tid: draws and geometry (synth_scattering_kernel's), and its Doppler shift
    const uint64_t kc = ss_key(a.seed, pkt, 0);
    double R = (double)a.range_m, ex = (double)a.ex, ey = (double)a.ey, ez = (double)a.ez;
    if (a.random_users) {
        const double u0 = (double)tr_uniform(kc, 0), u1 = (double)tr_uniform(kc, 1), u2 = (double)tr_uniform(kc, 2);
        R = 1.0 + ((double)a.range_m - 1.0) * u0;
        double sa, ca, se, ce;
        sincospi(2.0 * u1 - 1.0, &sa, &ca);              // az = 180 (2 u1 - 1) degrees
        sincospi(u2 - 0.5, &se, &ce);                    // el = 90 (2 u2 - 1) degrees
        ex = ce * ca; ey = ce * sa; ez = se;
    }
    double mx = a.mx, my = a.my;
    const double mz = a.mz;
    if (MOVING && a.random_heading) {
        double sa, ca;
        sincospi(2.0 * (double)tr_uniform(kc, 3) - 1.0, &sa, &ca);      // heading azimuth 180 (2 u3 - 1) degrees
        mx = a.mce * ca; my = a.mce * sa;
    }
    const bool mine = tid < S;
    double x = 0.0, nu = 0.0;
    float v = 0.f, cre = 0.f, cim = 0.f;
    if (mine) {
        const uint64_t b = 8 * (uint64_t)(tid + 1);
        const double bR = (double)a.box_frac * R;
        const double ox = bR * (2.0 * (double)tr_uniform(kc, b) - 1.0);
        const double oy = bR * (2.0 * (double)tr_uniform(kc, b + 1) - 1.0);
        const double oz = bR * (2.0 * (double)tr_uniform(kc, b + 2) - 1.0);
        const double o2 = ox * ox + oy * oy + oz * oz, on = sqrt(o2);
        const double qx = R * ex + ox, qy = R * ey + oy, qz = R * ez + oz;
        const double qn = sqrt(qx * qx + qy * qy + qz * qz);
        x = (2.0 * R * (ex * ox + ey * oy + ez * oz) + o2) / (qn + R) + on;
        v = (float)(qy / qn);
        const float w = on > 0.0 ? (float)(oy / on) : 0.f;
        if (MOVING) nu = on > 0.0 ? a.dop * (mx * ox + my * oy + mz * oz) / on : 0.0;
        const float gr = tr_normal(kc, b + 3) * a.gscale, gi = tr_normal(kc, b + 4) * a.gscale;
        float c, s;
        sc_phasor(0.5f * ((float)r - 0.5f * (float)(a.nr - 1)), w, c, s);       // exp(+2 pi i z_r w)
        cre = gr * c - gi * s;
        cim = gr * s + gi * c;
        xs[tid] = x;
    }
    sc_sync();
    if (mine) {
        double m = xs[0];
        for (int s = 1; s < S; ++s) m = fmin(m, xs[s]);
        tl[tid] = (float)((x - m) * (double)a.spm) * (1.0f / LS_FFT);
    }
    // B[b] = exp(-2 pi i y_b v) of antennas 0 .. 15
    float bre[SS_CH], bim[SS_CH];
    const float y0 = -0.25f * (float)(nt - 1);
#pragma unroll
    for (int b = 0; b < SS_CH; ++b) {
        float c, s;
        sc_phasor(y0 + 0.5f * (float)b, v, c, s);
        bre[b] = c;
        bim[b] = -s;
    }
    sc_sync();          // xs (in F) is free, tl is complete

    float ar[SS_CH], ai[SS_CH];
    const int fq = binp[tid < LS_NDATA ? tid : 0];
    const float fsig = (float)(fq < LS_FFT / 2 ? fq : fq - LS_FFT);
    const size_t plane = (size_t)nt * LS_NDATA;           // floats of one (packet, rx) item
    const size_t slice = (size_t)gridDim.x * plane;       // floats of one time
    float* ore = F;                                       // [nj][234] of the chunk
    float* oim = F + SS_CH * LS_NDATA;
    for (int j0 = 0; j0 < nt; j0 += SS_CH) {
        const int nj = min(SS_CH, nt - j0);
        float pc = 1.f, psn = 0.f;
        if (mine) sc_phasor((float)(j0 / 2), v, pc, psn);  // exp(-2 pi i (j0 / 2) v): antennas j0 + b sit j0 / 2 wavelengths behind antennas b
        for (int ti = 0; ti < a.n_times; ++ti) {
            if (mine) {
                float ctr = cre, cti = cim;
                if (MOVING) {
                    const double turns = nu * a.t[ti];
                    const float fr = (float)(turns - rint(turns));
                    float dc, ds;
                    sincospif(2.0f * fr, &ds, &dc);       // d_s(t) = exp(2 pi i nu_s t); exactly (1, 0) at t = 0
                    ctr = cre * dc - cim * ds;
                    cti = cre * ds + cim * dc;
                }
                const float er = ctr * pc + cti * psn, ei = cti * pc - ctr * psn;
                float* row = tab + (size_t)tid * SC_ROW;
#pragma unroll
                for (int b = 0; b < SS_CH; ++b) {
                    row[b] = er * bre[b] - ei * bim[b];
                    row[SS_CH + b] = er * bim[b] + ei * bre[b];
                }
            }
            sc_sync();
            sc_accumulate(tl, tab, S, fsig, ar, ai);
            if (tid < LS_NDATA) {
#pragma unroll
                for (int b = 0; b < SS_CH; ++b) {
                    if (b < nj) {
                        ore[b * LS_NDATA + tid] = ar[b] * a.amp;
                        oim[b * LS_NDATA + tid] = ai[b] * a.amp;
                    }
                }
            }
            sc_sync();
            // nt is a multiple of 4 (csi_create), so a chunk of nj antennas is a whole number of 16-byte vectors on a 16-byte boundary
            float* gre = a.h_re + (size_t)ti * slice + blk * plane + (size_t)j0 * LS_NDATA;
            float* gim = a.h_im + (size_t)ti * slice + blk * plane + (size_t)j0 * LS_NDATA;
            for (int i = tid; i < nj * LS_NDATA / 4; i += SS_THREADS) {
                *reinterpret_cast<f32x4*>(gre + 4 * i) = *reinterpret_cast<const f32x4*>(ore + 4 * i);
                *reinterpret_cast<f32x4*>(gim + 4 * i) = *reinterpret_cast<const f32x4*>(oim + 4 * i);
            }
            sc_sync();          // tab and the chunk image are rewritten
        }
    }
}

}  // namespace csi
