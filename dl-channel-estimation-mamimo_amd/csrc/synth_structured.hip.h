// synth_structured.hip.h - sounding packets with a KNOWN channel, generated on the device: the inverse of the LS kernel.
//
// Device twin of oracle.make_structured_packets / synth.structured_packets, which restate generate_maMIMO_LTF.m:197-342.
// One workgroup of 256 threads per (packet p, rx antenna r):
//   c[j][t]   n_taps complex Gaussian taps per tx antenna j, tap t scaled by decay[t] = exp(-0.5 t) / sqrt(2)
//   H[j][f]   = sum_t c[j][t] exp(-2 pi i f t / 256)                          (the 256-point DFT of the taps, FFT bin order)
//   X[s][f]   = ltf[f] * sum_j H[j][f] P[j][s]                               (ltf: all 242 non-null bins, P as csi_set_pilot holds it)
//   x[s][n]   = 1/256 sum_f X[s][f] exp(+2 pi i f n / 256);  symbol s of the preamble = x[s][192 .. 255] (cyclic prefix) | x[s][0 .. 255]
//   out       = amp * x + (amp * noise_std) * z,   z standard normal per real component
//   h[j][q]   = amp * H[j][f(q)] on the 234 data bins, the layout and bin order of the LS output
// so that csi_ls_estimate_device of the noise-free packet returns h whenever P P^T = Nt I.  amp = sqrt(242) / 256 (:303-304) or 1.
//
// The sum over j is taken on the taps, not on the spectra (d[s][t] = sum_j P[j][s] c[j][t], X[s][f] = ltf[f] DFT(d[s])[f]): Nt x Nt x
// n_taps products instead of Nt x Nt x 256, and the DFT of n_taps terms per bin needs no FFT.  The inverse transform IS the LS kernel's
// one-wave radix-4 FFT (ls_fft256_wave) with the two planes swapped on the way in and out.  The symbols pass through LDS in chunks of
// SS_CH; the pass is bound by its HBM writes (8 len_ltf bytes per item plus the channel planes), stored as 16-byte vectors.
//
// Noise is relative to the packet's OWN power (generate_maMIMO_LTF.m:283-295): pow = mean |x|^2 over the packet's nr * len_ltf complex
// samples before the amplitude scale, noise_std = sqrt(pow * 0.5 * 10^(-snr/10)) per real component.  A first launch (POWER) sums |x|^2
// per item - per thread in element order, then a fixed tree over the 256 threads - and the second launch adds the packet's nr item sums
// in rx order, so a run repeats bit for bit.  Noise-free calls (no SNR array) launch the second pass only.
//
// Draw layout (tests/synth_streams.py replays it).  Every draw is tr_normal(key, index) of rng.hip.h with
//   key(p, kind) = splitmix64(seed ^ splitmix64(2 * p + kind)),   p = ABSOLUTE packet index first_pkt + i,  kind 0 = taps, 1 = noise
//   tap   (r, j, t):  index ((r * Nt + j) * 64 + t) * 2 + {0 re, 1 im}       (64 = the largest n_taps: tap t does not move with n_taps)
//   noise (r, n):     index (r * len_ltf + n) * 2 + {0 re, 1 im}             (n = sample of the rx preamble, 0 .. len_ltf - 1)
// so packets [first, first + n) are the same bits whichever call produces them, and noise never touches the channel draws.
// All arithmetic is fp32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ls_estimate.hip.h"      // ls_fft_rows, ls_phys, LS_*
#include "rng.hip.h"

namespace csi {

constexpr int SS_CH = 16;              // LTF symbols per LDS chunk
constexpr int SS_MAX_TAPS = 64;
constexpr int SS_THREADS = 256;
constexpr int SS_FIXED_FLOATS = 4 * LS_FFT + SS_MAX_TAPS + SS_CH * 2 * LS_PLANE;      // tw_re, tw_im, ltf, reduction / bin table, decay, F

struct SynthArgs {
    const float* P;          // [nt][nt] row j = pilot sequence of tx j
    const float* tw;         // [2][256] exp(-2 pi i u / 256)
    const float* ltf_nat;    // [256] LTF sequence in FFT bin order (0 on the null bins)
    const int* bin_pos;      // [234] FFT bin of data bin q
    const float* decay;      // [64] tap profile
    const float* fac;        // [npkt] 0.5 * 10^(-snr/10); null = noise-free
    float* part;             // [npkt * nr] sum |x|^2 of every item (written by the POWER launch, read by the other)
    float* ltf_re;           // [npkt][nr][len_ltf]
    float* ltf_im;
    float* h_re;             // [npkt][nr][nt][234] or null
    float* h_im;
    float* noise_std;        // [npkt] or null
    uint64_t seed;
    int64_t first_pkt;
    int nt, nr, len_ltf, n_taps;
    float amp;
};

__host__ __device__ inline size_t synth_lds_floats(int nt, int n_taps) {
    return (size_t)SS_FIXED_FLOATS + (size_t)nt * SS_CH + 2 * (size_t)SS_CH * n_taps + 2 * (size_t)nt * n_taps;
}

__device__ __forceinline__ uint64_t ss_key(uint64_t seed, uint64_t pkt, uint64_t kind) { return splitmix64(seed ^ splitmix64(2 * pkt + kind)); }

template <bool POWER>
__global__ __launch_bounds__(SS_THREADS) void synth_structured_kernel(const SynthArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int nt = a.nt, n_taps = a.n_taps;
    float* tw_re = smem;                                  // [256]
    float* tw_im = smem + LS_FFT;                         // [256]
    float* lt = smem + 2 * LS_FFT;                        // [256] ltf / 256 in FFT bin order
    float* red = smem + 3 * LS_FFT;                       // [256] power reduction (POWER) / data-bin table as ints (otherwise)
    float* dec = smem + 4 * LS_FFT;                       // [64]
    float* F = dec + SS_MAX_TAPS;                         // [SS_CH][2][LS_PLANE]
    float* Pc = F + SS_CH * 2 * LS_PLANE;                 // [nt][SS_CH] pilot columns of the chunk
    float* dre = Pc + (size_t)nt * SS_CH;                 // [SS_CH][n_taps] taps of the chunk's symbols
    float* dim = dre + SS_CH * n_taps;
    float* cre = dim + SS_CH * n_taps;                    // [nt][n_taps] taps of the tx antennas
    float* cim = cre + (size_t)nt * n_taps;
    int* binp = reinterpret_cast<int*>(red);

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const size_t blk = blockIdx.x;
    const int64_t pl = (int64_t)(blk / a.nr);             // packet of this call
    const int r = (int)(blk - (size_t)pl * a.nr);
    const uint64_t pkt = (uint64_t)(a.first_pkt + pl);

    tw_re[tid] = a.tw[tid];
    tw_im[tid] = a.tw[LS_FFT + tid];
    lt[tid] = a.ltf_nat[tid] * (1.0f / LS_FFT);
    if (tid < SS_MAX_TAPS) dec[tid] = a.decay[tid];
    if (!POWER && tid < LS_NDATA) binp[tid] = a.bin_pos[tid];
    __syncthreads();

    // ---- taps
    const uint64_t ktap = ss_key(a.seed, pkt, 0);
    for (int i = tid; i < nt * n_taps; i += SS_THREADS) {
        const int j = i / n_taps, t = i - j * n_taps;
        const uint64_t pos = ((uint64_t)(r * nt + j) * SS_MAX_TAPS + t) * 2;
        cre[i] = tr_normal(ktap, pos) * dec[t];
        cim[i] = tr_normal(ktap, pos + 1) * dec[t];
    }
    __syncthreads();

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

    // ---- true channel on the data bins: h[j][q] = amp * sum_t c[j][t] w^(f(q) t)
    if (!POWER && a.h_re) {
        const int total = nt * LS_NDATA;
        auto hval = [&](int idx, float& hr, float& hi) {
            const int j = idx / LS_NDATA, q = idx - j * LS_NDATA;
            const int f = binp[q];
            float sr = 0.f, si = 0.f;
            for (int t = 0; t < n_taps; ++t) {
                const int u = (f * t) & (LS_FFT - 1);
                const float wr = tw_re[u], wi = tw_im[u];
                const float cr = cre[j * n_taps + t], ci = cim[j * n_taps + t];
                sr = fmaf(cr, wr, fmaf(-ci, wi, sr));
                si = fmaf(cr, wi, fmaf(ci, wr, si));
            }
            hr = sr * a.amp;
            hi = si * a.amp;
        };
        float* gre = a.h_re + blk * (size_t)total;
        float* gim = a.h_im + blk * (size_t)total;
        // nt is a multiple of 4 (csi_create), so item blocks start on 16-byte boundaries: one float4 per lane and plane
        for (int v = tid; v < total / 4; v += SS_THREADS) {
            f32x4 vr, vi;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float hr, hi;
                hval(4 * v + e, hr, hi);
                vr[e] = hr;
                vi[e] = hi;
            }
            *reinterpret_cast<f32x4*>(gre + 4 * v) = vr;
            *reinterpret_cast<f32x4*>(gim + 4 * v) = vi;
        }
    }

    const uint64_t knoise = ss_key(a.seed, pkt, 1);
    const int frev = ((tid & 3) << 6) | (((tid >> 2) & 3) << 4) | (((tid >> 4) & 3) << 2) | (tid >> 6);      // this thread's FFT bin: position tid digit-reversed
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
        __syncthreads();
        // ---- taps of the chunk's symbols: d[s][t] = sum_j P[j][s] c[j][t]
        for (int i = tid; i < ns * n_taps; i += SS_THREADS) {
            const int sl = i / n_taps, t = i - sl * n_taps;
            float sr = 0.f, si = 0.f;
            for (int j = 0; j < nt; ++j) {
                const float pv = Pc[j * SS_CH + sl];
                sr = fmaf(pv, cre[j * n_taps + t], sr);
                si = fmaf(pv, cim[j * n_taps + t], si);
            }
            dre[i] = sr;
            dim[i] = si;
        }
        __syncthreads();
        // ---- spectra X[s][f] / 256, planes swapped (the forward FFT of (im, re) is (im, re) of the inverse transform), digit-reversed
        for (int sl = 0; sl < ns; ++sl) {
            float sr = 0.f, si = 0.f;
            for (int t = 0; t < n_taps; ++t) {
                const int u = (frev * t) & (LS_FFT - 1);
                const float wr = tw_re[u], wi = tw_im[u];
                const float dr = dre[sl * n_taps + t], di = dim[sl * n_taps + t];
                sr = fmaf(dr, wr, fmaf(-di, wi, sr));
                si = fmaf(dr, wi, fmaf(di, wr, si));
            }
            float* fr = F + (size_t)sl * 2 * LS_PLANE;
            fr[ppos] = si * lf;
            fr[LS_PLANE + ppos] = sr * lf;
        }
        __syncthreads();
        ls_fft_rows(F, wave, ns, tw_re, tw_im, lane);
        __syncthreads();
        // ---- cyclic prefix + body, 4 samples per lane and plane
        for (int v = tid; v < ns * (LS_SYM / 4); v += SS_THREADS) {
            const int sl = v / (LS_SYM / 4), i = v - sl * (LS_SYM / 4);
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
        __syncthreads();          // F, Pc and d are rewritten by the next chunk
    }

    if (POWER) {
        red[tid] = acc;
        __syncthreads();
        for (int w = SS_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0) a.part[blk] = red[0];
    }
}

}  // namespace csi
