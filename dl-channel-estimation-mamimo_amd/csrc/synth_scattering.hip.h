// synth_scattering.hip.h - sounding packets with a KNOWN channel from a geometric single-bounce scattering model, generated on the device.
//
// The second generator beside synth_structured.hip.h: the same outputs, noise model, draw discipline and LS-inverse contract, another
// channel.  The reference's channel is phased.ScatteringMIMOChannel (helperApplyMUChannel.m:44-143): 100 scatterers in a box around the
// receiver, seen from half-wavelength arrays.  The toolbox object is not part of the reference tree, so its random stream and its sign
// conventions cannot be pinned; the model below is restated from the physics.
//
// Per packet p (absolute index), with kc = ss_key(seed, p, 0), the channel stream (no tap is drawn in this mode):
//   user     flag bit 1:  u0..u2 = tr_uniform(kc, 0..2),  R = 1 + (range_m - 1) u0,  az = 180 (2 u1 - 1),  el = 90 (2 u2 - 1)  degrees
//            otherwise R, az, el are the configured values;   e = (cos el cos az, cos el sin az, sin el)
//   scatterer s, base index b = 8 (s + 1):
//            offset from the receiver  o_s[i] = box_frac R (2 tr_uniform(kc, b + i) - 1),  i = 0, 1, 2
//            reflection coefficient    g_s = (tr_normal(kc, b + 3) + i tr_normal(kc, b + 4)) / sqrt(2)   (the carrier phase is absorbed)
//   geometry q_s = R e + o_s
//            excess path   x_s = (2 R (e . o_s) + |o_s|^2) / (|q_s| + R) + |o_s|        ( = |q_s| - R + |o_s| without the cancellation)
//            excess delay  tau_s = (x_s - min_s' x_s') fs / c  samples,  c = 299792458   (the first path sits at delay 0)
//            reported      tau[p][s] = (R + x_s) fs / c                                  (the absolute path delay in samples)
//            direction cosines along the array axis y:  v_s = q_s,y / |q_s| (transmitter),  w_s = o_s,y / |o_s| (receiver; 0 for o = 0)
//   arrays   ULAs along y, half a wavelength apart:  y_j = (j - (Nt - 1) / 2) / 2,  z_r = (r - (Nr - 1) / 2) / 2
//   response H[r][j][f] = S^(-1/2) sum_s g_s exp(2 pi i z_r w_s) exp(-2 pi i y_j v_s) exp(-2 pi i f tau_s / 256)
//            f = the SIGNED bin index -128 .. 127 (FFT bins 128 .. 255 are f - 256): the delays are fractional, so the sign matters.
//            The transmit factor is the conjugate of synth.steering_ula, so the dominant right singular vector of a one-scatterer H is
//            steering_ula at that scatterer's direction.  E|H|^2 = 1.
// Everything behind H is synth_structured.hip.h's: X[sym][f] = ltf[f] sum_j H[j][f] P[j][sym] on the 242 non-null bins, the 256-point
// inverse transform (ls_fft256_wave with the planes swapped), the 64-sample prefix, amp, noise relative to the packet's own power from
// key(p, 1) at (r len_ltf + n) 2 + {0, 1}, h = amp H on the 234 data bins in the LS layout.
//
// One workgroup of 256 lanes per (packet, rx), a power pass and a packet pass.
//   setup    lane s: the draws and the geometry of scatterer s in fp64 (a few dozen operations once per workgroup; every later value is
//            fp32), c_s = g_s exp(2 pi i z_r w_s) / sqrt(S), the 16 phasors B[b] = exp(-2 pi i y_b v_s) of its first 16 antennas
//   table    antennas 16 a + b:  exp(-2 pi i y_j v_s) = exp(-2 pi i 8 a v_s) B[b]: one sincos per 16 antennas, one complex product each
//   channel  per chunk of 16 antennas lane s writes T[s][b] = c_s exp(-2 pi i y_j v_s); lane q sums T[s][.] exp(-2 pi i f(q) tau_s / 256)
//            over s into 16 complex accumulators; the chunk goes through LDS and leaves as 16-byte vectors
//   symbols  per chunk of 16 LTF symbols lane s writes D[s][sym] = c_s sum_j P[j][sym] exp(-2 pi i y_j v_s); lane f sums over s the same way
// Every phase is reduced in turns before sincos: a product x y is split into its rounded value p and the exact remainder fma(x, y, -p),
// and (p - rint(p)) + remainder goes to sincospif.  Planar re / im, no complex types, compiled without packed fp32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "ls_estimate.hip.h"
#include "rng.hip.h"
#include "synth_structured.hip.h"      // ss_key, SS_CH, SS_THREADS

namespace csi {

constexpr int SC_MAX_SCAT = 256;
constexpr int SC_ROW = 2 * SS_CH + 4;      // floats per scatterer in the chunk table: 16 re, 16 im, 4 pad (rows 16-byte aligned, 16 banks apart)
constexpr double SC_LIGHT = 299792458.0;

#if defined(__HIP_DEVICE_COMPILE__)
#define SC_NO_PK __attribute__((target("no-packed-fp32-ops")))
#else
#define SC_NO_PK
#endif
#define SC_DEV __device__ __forceinline__ SC_NO_PK

struct ScatterArgs {
    const float* P;          // [nt][nt] row j = pilot sequence of tx j
    const float* tw;         // [2][256] exp(-2 pi i u / 256)
    const float* ltf_nat;    // [256] LTF sequence in FFT bin order (0 on the null bins)
    const int* bin_pos;      // [234] FFT bin of data bin q
    const float* fac;        // [npkt] 0.5 * 10^(-snr/10); null = noise-free
    float* part;             // [npkt * nr] sum |x|^2 of every item (written by the POWER launch, read by the other)
    float* ltf_re;           // [npkt][nr][len_ltf]
    float* ltf_im;
    float* h_re;             // [npkt][nr][nt][234] or null
    float* h_im;
    float* noise_std;        // [npkt] or null
    float* tau;              // [npkt][n_scat] or null
    uint64_t seed;
    int64_t first_pkt;
    int nt, nr, len_ltf, n_scat;
    int random_users;
    float amp;
    float range_m, box_frac;
    float ex, ey, ez;        // user direction of the configured az / el (fixed users)
    float spm;               // samples per metre fs / c
    float gscale;            // 1 / sqrt(2 n_scat)
};

__host__ __device__ inline size_t scatter_lds_floats(int nt, int n_scat) {
    return (size_t)4 * LS_FFT + (size_t)SS_CH * 2 * LS_PLANE + (size_t)nt * SS_CH + (size_t)((n_scat + 3) & ~3) + (size_t)n_scat * SC_ROW;
}

// __syncthreads of a function compiled without packed fp32: the library's own is not inlined across the differing target attribute
SC_DEV void sc_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// cos and sin of 2 pi x y, the product reduced exactly in turns
SC_DEV void sc_phasor(float x, float y, float& c, float& s) {
    const float p = x * y;
    const float rem = fmaf(x, y, -p);
    const float fr = (p - rintf(p)) + rem;
    sincospif(2.0f * fr, &s, &c);
}

// acc[k] += (tab[s][k] + i tab[s][16 + k]) exp(-2 pi i f tl[s]) over the scatterers
SC_DEV void sc_accumulate(const float* tl, const float* tab, int n_scat, float f, float (&ar)[SS_CH], float (&ai)[SS_CH]) {
#pragma unroll
    for (int k = 0; k < SS_CH; ++k) ar[k] = ai[k] = 0.f;
    for (int s = 0; s < n_scat; ++s) {
        float c, sn;
        sc_phasor(f, tl[s], c, sn);
        const f32x4* row = reinterpret_cast<const f32x4*>(tab + (size_t)s * SC_ROW);
#pragma unroll
        for (int k4 = 0; k4 < SS_CH / 4; ++k4) {
            const f32x4 dr = row[k4], di = row[SS_CH / 4 + k4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ar[4 * k4 + e] = fmaf(dr[e], c, fmaf(di[e], sn, ar[4 * k4 + e]));
                ai[4 * k4 + e] = fmaf(di[e], c, fmaf(-dr[e], sn, ai[4 * k4 + e]));
            }
        }
    }
}

template <bool POWER>
__global__ SC_NO_PK __launch_bounds__(SS_THREADS) void synth_scattering_kernel(const ScatterArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int nt = a.nt, S = a.n_scat;
    float* tw_re = smem;                                  // [256]
    float* tw_im = smem + LS_FFT;                         // [256]
    float* lt = smem + 2 * LS_FFT;                        // [256] ltf / 256 in FFT bin order
    float* red = smem + 3 * LS_FFT;                       // [256] power reduction (POWER) / data-bin table as ints (otherwise)
    float* F = smem + 4 * LS_FFT;                         // [SS_CH][2][LS_PLANE]; the excess paths (fp64) during the setup; the channel chunk on its way out
    float* Pc = F + SS_CH * 2 * LS_PLANE;                 // [nt][SS_CH] pilot columns of the chunk
    float* tl = Pc + (size_t)nt * SS_CH;                  // [S] tau_s / 256
    float* tab = tl + ((S + 3) & ~3);                     // [S][SC_ROW] chunk table: T (antennas) or D (symbols)
    int* binp = reinterpret_cast<int*>(red);
    double* xs = reinterpret_cast<double*>(F);

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const size_t blk = blockIdx.x;
    const int64_t pl = (int64_t)(blk / a.nr);             // packet of this call
    const int r = (int)(blk - (size_t)pl * a.nr);
    const uint64_t pkt = (uint64_t)(a.first_pkt + pl);

    tw_re[tid] = a.tw[tid];
    tw_im[tid] = a.tw[LS_FFT + tid];
    lt[tid] = a.ltf_nat[tid] * (1.0f / LS_FFT);
    if (!POWER && tid < LS_NDATA) binp[tid] = a.bin_pos[tid];

    // ---- scatterer tid: draws and geometry
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
    const bool mine = tid < S;
    double x = 0.0;
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
        const float gr = tr_normal(kc, b + 3) * a.gscale, gi = tr_normal(kc, b + 4) * a.gscale;
        float c, s;
        sc_phasor(0.5f * ((float)r - 0.5f * (float)(a.nr - 1)), w, c, s);       // exp(+2 pi i z_r w)
        cre = gr * c - gi * s;
        cim = gr * s + gi * c;
        xs[tid] = x;
        if (!POWER && a.tau && r == 0) a.tau[(size_t)pl * S + tid] = (float)((R + x) * (double)a.spm);
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

    // ---- noise level of the packet: its nr item sums in rx order
    float nstd = 0.f;
    if (!POWER) {
        if (a.fac) {
            float s = 0.f;
            for (int i = 0; i < a.nr; ++i) s += a.part[(size_t)pl * a.nr + i];
            nstd = sqrtf(s / ((float)a.nr * (float)a.len_ltf) * a.fac[pl]);
        }
        if (a.noise_std && r == 0 && tid == 0) a.noise_std[pl] = nstd;
    }
    const float nstd_s = nstd * a.amp;

    float ar[SS_CH], ai[SS_CH];

    // ---- true channel on the data bins: h[j][q] = amp H[j][f(q)], 16 antennas at a time
    if (!POWER && a.h_re) {
        const int fq = binp[tid < LS_NDATA ? tid : 0];
        const float fsig = (float)(fq < LS_FFT / 2 ? fq : fq - LS_FFT);
        float* gre = a.h_re + blk * (size_t)nt * LS_NDATA;
        float* gim = a.h_im + blk * (size_t)nt * LS_NDATA;
        float* ore = F;                                   // [nj][234] of the chunk
        float* oim = F + SS_CH * LS_NDATA;
        for (int j0 = 0; j0 < nt; j0 += SS_CH) {
            const int nj = min(SS_CH, nt - j0);
            if (mine) {
                float c, s;
                sc_phasor((float)(j0 / 2), v, c, s);      // exp(-2 pi i (j0 / 2) v): antennas j0 + b sit j0 / 2 wavelengths behind antennas b
                const float er = cre * c + cim * s, ei = cim * c - cre * s;
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
            for (int i = tid; i < nj * LS_NDATA / 4; i += SS_THREADS) {
                *reinterpret_cast<f32x4*>(gre + (size_t)j0 * LS_NDATA + 4 * i) = *reinterpret_cast<const f32x4*>(ore + 4 * i);
                *reinterpret_cast<f32x4*>(gim + (size_t)j0 * LS_NDATA + 4 * i) = *reinterpret_cast<const f32x4*>(oim + 4 * i);
            }
            sc_sync();          // tab and the chunk image are rewritten
        }
    }

    const uint64_t knoise = ss_key(a.seed, pkt, 1);
    const int frev = ((tid & 3) << 6) | (((tid >> 2) & 3) << 4) | (((tid >> 4) & 3) << 2) | (tid >> 6);      // this thread's FFT bin: position tid digit-reversed
    const float fsig = (float)(frev < LS_FFT / 2 ? frev : frev - LS_FFT);
    const float lf = lt[frev];
    const int ppos = ls_phys(tid);
    float acc = 0.f;

    for (int s0 = 0; s0 < nt; s0 += SS_CH) {
        const int ns = min(SS_CH, nt - s0);
        // ---- pilot columns s0 .. s0 + ns - 1 of every tx antenna
        for (int i = tid; i < nt * SS_CH; i += SS_THREADS) {
            const int j = i / SS_CH, sl = i - j * SS_CH;
            Pc[i] = sl < ns ? a.P[(size_t)j * nt + s0 + sl] : 0.f;
        }
        sc_sync();
        // ---- D[s][sym] = c_s sum_j P[j][sym] exp(-2 pi i y_j v_s)
        if (mine) {
#pragma unroll
            for (int k = 0; k < SS_CH; ++k) ar[k] = ai[k] = 0.f;
            for (int j0 = 0; j0 < nt; j0 += SS_CH) {
                float c, s;
                sc_phasor((float)(j0 / 2), v, c, s);
#pragma unroll
                for (int b = 0; b < SS_CH; ++b) {
                    if (j0 + b < nt) {
                        const float er = c * bre[b] + s * bim[b], ei = c * bim[b] - s * bre[b];      // (c - i s) B[b]
                        const f32x4* pr = reinterpret_cast<const f32x4*>(Pc + (size_t)(j0 + b) * SS_CH);
#pragma unroll
                        for (int k4 = 0; k4 < SS_CH / 4; ++k4) {
                            const f32x4 pv = pr[k4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                ar[4 * k4 + e] = fmaf(pv[e], er, ar[4 * k4 + e]);
                                ai[4 * k4 + e] = fmaf(pv[e], ei, ai[4 * k4 + e]);
                            }
                        }
                    }
                }
            }
            float* row = tab + (size_t)tid * SC_ROW;
#pragma unroll
            for (int k = 0; k < SS_CH; ++k) {
                row[k] = cre * ar[k] - cim * ai[k];
                row[SS_CH + k] = cre * ai[k] + cim * ar[k];
            }
        }
        sc_sync();
        // ---- spectra X[sym][f] / 256, planes swapped (the forward FFT of (im, re) is (im, re) of the inverse transform), digit-reversed
        sc_accumulate(tl, tab, S, fsig, ar, ai);
#pragma unroll
        for (int sl = 0; sl < SS_CH; ++sl) {
            if (sl < ns) {
                float* fr = F + (size_t)sl * 2 * LS_PLANE;
                fr[ppos] = ai[sl] * lf;
                fr[LS_PLANE + ppos] = ar[sl] * lf;
            }
        }
        sc_sync();
        ls_fft_rows(F, wave, ns, tw_re, tw_im, lane);
        sc_sync();
        // ---- cyclic prefix + body, 4 samples per lane and plane
        for (int vv = tid; vv < ns * (LS_SYM / 4); vv += SS_THREADS) {
            const int sl = vv / (LS_SYM / 4), i = vv - sl * (LS_SYM / 4);
            const int n = (4 * i + LS_FFT - LS_CP) & (LS_FFT - 1);
            const float* src = F + (size_t)sl * 2 * LS_PLANE + ls_phys(n);
            const f32x4 xi = *reinterpret_cast<const f32x4*>(src);
            const f32x4 xr = *reinterpret_cast<const f32x4*>(src + LS_PLANE);
            if (POWER) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = fmaf(xr[e], xr[e], fmaf(xi[e], xi[e], acc));
            } else {
                const size_t o = (size_t)(s0 + sl) * LS_SYM + 4 * i;       // sample of the rx preamble
                f32x4 yr, yi;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    yr[e] = xr[e] * a.amp;
                    yi[e] = xi[e] * a.amp;
                }
                if (nstd_s != 0.f) {
                    const uint64_t base = ((uint64_t)r * a.len_ltf + o) * 2;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        yr[e] = fmaf(nstd_s, tr_normal(knoise, base + 2 * e), yr[e]);
                        yi[e] = fmaf(nstd_s, tr_normal(knoise, base + 2 * e + 1), yi[e]);
                    }
                }
                *reinterpret_cast<f32x4*>(a.ltf_re + blk * a.len_ltf + o) = yr;
                *reinterpret_cast<f32x4*>(a.ltf_im + blk * a.len_ltf + o) = yi;
            }
        }
        sc_sync();          // F, Pc and the table are rewritten by the next chunk
    }

    if (POWER) {
        red[tid] = acc;
        sc_sync();
        for (int w = SS_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            sc_sync();
        }
        if (tid == 0) a.part[blk] = red[0];
    }
}

}  // namespace csi
