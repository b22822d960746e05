// cfo.hip.h - carrier frequency offset of the sounding preamble: the cyclic-prefix estimator and the rotation that impairs or corrects
// (host side: csi_cfo.hpp).
//
// x[p][r][n] are the planes ltf_re / ltf_im, n = 320 s + m, s < Nt, m < 320 (64 samples of cyclic prefix, 256 of body), len = 320 Nt;
// eps is in subcarrier spacings (cycles per 256 samples), one per packet.
//   y[p][r][n] = x[p][r][n] exp(2 pi i scale eps[p] n / 256)                                          cfo_rotate_kernel
//   gamma[p]   = sum_r sum_s sum_{m = cp_skip}^{63} conj(x[p][r][320 s + m]) x[p][r][320 s + m + 256]
//   E[p]       = 1/2 sum (|x[.. m]|^2 + |x[.. m + 256]|^2) over the same samples
//   eps_hat[p] = atan2(Im gamma, Re gamma) / 2 pi,  quality[p] = |gamma| / E;  E == 0 gives (0, 0)    cfo_corr_kernel
//
// Plan:
//   * cfo_corr_kernel: one workgroup of 4 waves per packet, walking its antennas in order.  An item is four samples of one prefix and
//     their twins 256 samples on: four 16-byte loads (a symbol is 1280 bytes, so every item sits on a 16-byte boundary); the one item a
//     cp_skip that is no multiple of 4 cuts is read sample by sample, so nothing in front of cp_skip is touched.  Lane t takes the items
//     t, t + 256, .. of every antenna.  Products in fp32 (re: fmaf(ai, bi, ar br), im: fmaf(-ai, br, ar bi), |a|^2: fmaf(ar, ar, ai ai)),
//     every sum in fp64: along the lane, then a binary tree over the 256 lanes through LDS.  No atomics; the order of every sum is
//     fixed by (Nt, Nr, cp_skip) alone, so a packet has the same bits whatever the call size or its position.  One fp64 atan2 per packet.
//   * cfo_rotate_kernel: streaming, 16-byte words in and out, a workgroup inside one packet.  Per sample the turn count
//     (scale eps / 256) n in fp64, reduced in fp64 (t - rint(t)), rounded once to fp32 for sincospif (the way of scatter_aged.hip.h);
//     the product on scalar floats: re = fmaf(-xi, s, xr c), im = fmaf(xi, c, xr s).  scale eps == 0 copies the bits.  A lane reads its
//     four samples of both planes before it writes them: in place allowed.
// The kernels are templates compiled without packed fp32 and included behind everything else, so they are emitted behind the earlier ones.
#pragma once
#include "hybrid_weights.hip.h"      // HY_KERNEL

namespace csi {

constexpr int CFO_SYM = 320;                 // samples of a sounding symbol
constexpr int CFO_CP = 64;                   // of them cyclic prefix
constexpr int CFO_FFT = 256;                 // distance of a prefix sample to its twin
constexpr int CFO_THREADS = 256;

struct CfoCorrArgs {
    const float* x_re;                       // [npkt][nr][320 nt], at the call's first packet
    const float* x_im;
    double* eps;                             // [npkt]
    float* quality;                          // [npkt] or null
    int nt, nr, cp_skip;
};

struct CfoRotateArgs {
    const float* x_re;
    const float* x_im;
    float* y_re;
    float* y_im;
    const double* eps;                       // [npkt]
    double scale;
    long long row;                           // samples of one (packet, rx): 320 nt
    long long groups;                        // 16-byte words of a packet and plane: nr 80 nt
    int wg_per_pkt;                          // workgroups of a packet
};

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// UNUSED only makes the kernel a template
template <int UNUSED>
HY_KERNEL __launch_bounds__(CFO_THREADS) void cfo_corr_kernel(const CfoCorrArgs a) {
    __shared__ double cfo_s[3 * CFO_THREADS];
    const int tid = threadIdx.x;
    const int g0 = a.cp_skip >> 2;                       // first item of a prefix; cut when cp_skip & 3
    const int cut = a.cp_skip & 3;
    const int per_sym = CFO_CP / 4 - g0;                 // items of a symbol: 1 .. 16
    const int items = a.nt * per_sym;
    const size_t row = (size_t)CFO_SYM * (size_t)a.nt;
    const size_t pkt = (size_t)blockIdx.x * (size_t)a.nr * row;
    double gr = 0.0, gi = 0.0, en = 0.0;
    for (int r = 0; r < a.nr; ++r) {
        const float* xr = a.x_re + pkt + (size_t)r * row;
        const float* xi = a.x_im + pkt + (size_t)r * row;
        for (int i = tid; i < items; i += CFO_THREADS) {
            const int s = i / per_sym, g = g0 + (i - s * per_sym);
            const size_t o = (size_t)s * CFO_SYM + 4 * (size_t)g;
            float ar[4], ai[4], br[4], bi[4];
            if (g == g0 && cut) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool in = j >= cut;
                    ar[j] = in ? xr[o + j] : 0.0f;
                    ai[j] = in ? xi[o + j] : 0.0f;
                    br[j] = in ? xr[o + j + CFO_FFT] : 0.0f;
                    bi[j] = in ? xi[o + j + CFO_FFT] : 0.0f;
                }
            } else {
                const float4 v0 = *reinterpret_cast<const float4*>(xr + o);
                const float4 v1 = *reinterpret_cast<const float4*>(xi + o);
                const float4 v2 = *reinterpret_cast<const float4*>(xr + o + CFO_FFT);
                const float4 v3 = *reinterpret_cast<const float4*>(xi + o + CFO_FFT);
                ar[0] = v0.x; ar[1] = v0.y; ar[2] = v0.z; ar[3] = v0.w;
                ai[0] = v1.x; ai[1] = v1.y; ai[2] = v1.z; ai[3] = v1.w;
                br[0] = v2.x; br[1] = v2.y; br[2] = v2.z; br[3] = v2.w;
                bi[0] = v3.x; bi[1] = v3.y; bi[2] = v3.z; bi[3] = v3.w;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                gr += (double)fmaf(ai[j], bi[j], ar[j] * br[j]);          // conj(a) b
                gi += (double)fmaf(-ai[j], br[j], ar[j] * bi[j]);
                en += (double)fmaf(ar[j], ar[j], ai[j] * ai[j]);
                en += (double)fmaf(br[j], br[j], bi[j] * bi[j]);
            }
        }
    }
    cfo_s[tid] = gr;
    cfo_s[CFO_THREADS + tid] = gi;
    cfo_s[2 * CFO_THREADS + tid] = en;
    __syncthreads();
    for (int h = CFO_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            cfo_s[tid] += cfo_s[tid + h];
            cfo_s[CFO_THREADS + tid] += cfo_s[CFO_THREADS + tid + h];
            cfo_s[2 * CFO_THREADS + tid] += cfo_s[2 * CFO_THREADS + tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double sr = cfo_s[0], si = cfo_s[CFO_THREADS], e = 0.5 * cfo_s[2 * CFO_THREADS];
        const bool none = e == 0.0;
        a.eps[blockIdx.x] = none ? 0.0 : atan2(si, sr) * 0.15915494309189533577;      // 1 / (2 pi)
        if (a.quality) a.quality[blockIdx.x] = none ? 0.0f : (float)(sqrt(sr * sr + si * si) / e);
    }
}

// UNUSED only makes the kernel a template
template <int UNUSED>
HY_KERNEL __launch_bounds__(CFO_THREADS) void cfo_rotate_kernel(const CfoRotateArgs a) {
    const long long p = blockIdx.x / a.wg_per_pkt;
    const long long q = (long long)(blockIdx.x - p * a.wg_per_pkt) * CFO_THREADS + threadIdx.x;      // 16-byte word of the packet
    if (q >= a.groups) return;
    const size_t o = ((size_t)p * (size_t)a.groups + (size_t)q) * 4;
    const float4 xr = *reinterpret_cast<const float4*>(a.x_re + o);
    const float4 xi = *reinterpret_cast<const float4*>(a.x_im + o);
    float4 yr = xr, yi = xi;
    const double f = a.scale * a.eps[p] * (1.0 / CFO_FFT);      // turns per sample
    if (f != 0.0) {
        const long long n0 = (4 * q) % a.row;
        const float vr[4] = {xr.x, xr.y, xr.z, xr.w}, vi[4] = {xi.x, xi.y, xi.z, xi.w};
        float wr[4], wi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double turns = f * (double)(n0 + j);
            const float fr = (float)(turns - rint(turns));
            float s, c;
            sincospif(2.0f * fr, &s, &c);
            wr[j] = fmaf(-vi[j], s, vr[j] * c);
            wi[j] = fmaf(vi[j], c, vr[j] * s);
        }
        yr = make_float4(wr[0], wr[1], wr[2], wr[3]);
        yi = make_float4(wi[0], wi[1], wi[2], wi[3]);
    }
    *reinterpret_cast<float4*>(a.y_re + o) = yr;
    *reinterpret_cast<float4*>(a.y_im + o) = yi;
}
#endif

}  // namespace csi
