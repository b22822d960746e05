// sync.hip.h - symbol timing of the sounding preamble: the cyclic-prefix timing metric (joint with the carrier frequency offset), the
// cut-out that applies a start and an offset, and the embedding that impairs (host side: csi_sync.hpp).
//
// c[p][r][n] are capture planes [npkt][nr][L], L = 320 nt + span, span a multiple of 4 in 4 .. 256 (every row on a 16-byte boundary);
// the packet of len = 320 nt samples starts at theta[p] in 0 .. span.  For theta = 0 .. span
//   gamma(theta) = sum_r sum_s sum_{m<64} conj(c[p][r][theta + 320 s + m]) c[p][r][theta + 320 s + m + 256]
//   Phi(theta)   = 1/2 sum (|c[.. m]|^2 + |c[.. m + 256]|^2) over the same samples
//   Lambda(theta) = |gamma(theta)| - rho Phi(theta);  theta_hat = the lowest theta of the largest Lambda
//   eps_hat = atan2(Im, Re of gamma(theta_hat)) / 2 pi,  quality = |gamma(theta_hat)| / Phi(theta_hat);  Phi == 0 gives (0, 0)       sync_metric_kernel
//   y[p][r][n] = c[p][r][theta[p] + n] exp(-2 pi i eps[p] n / 256),  n < len                                                    sync_extract_kernel
//   c[p][r][theta[p] + n] = x[p][r][n];  every other sample std[p] (normal(km, 2 e) + i normal(km, 2 e + 1)), e = r L + n         sync_embed_kernel
//
// Plan:
//   * sync_metric_kernel: one workgroup of 4 waves per packet.  The sums over r and s come first: with q[n] = conj(c[n]) c[n + 256] and
//     e[n] = |c[n]|^2 + |c[n + 256]|^2, Q[j] = sum_r sum_s q[320 s + j] and E[j] likewise for the J = span + 64 folded positions j, J / 4
//     items of four positions (17 .. 80).  Lane (item i, stride k), k < K = 256 / (J / 4), takes the rows m = r nt + s = k, k + K, .. of
//     its item: four 16-byte loads per row, the products in fp32 in the forms of cfo_corr_kernel, twelve fp64 sums in registers.  The K
//     strides of a position are then added in order of k through LDS, and lane theta adds the 64 folded positions theta .. theta + 63 in
//     order of m (the direct window sum, no running difference: 3 x 64 LDS reads a lane, and every Lambda carries the rounding of its own
//     64 terms alone).  Argmax by a binary tree that keeps the lower theta on equal values; one fp64 atan2.  No atomics; the order of every
//     sum is fixed by (nt, nr, span) alone, so a packet has the same bits whatever the call size or its position.  Nothing outside
//     [0, L) of a row is read: the last sample read is 320 (nt - 1) + J - 1 + 256 = L - 1.
//   * sync_extract_kernel: streaming, the launch shape of cfo_rotate_kernel on the output planes; a lane writes one 16-byte word of both
//     planes.  Its source starts theta & 3 floats off a 16-byte boundary: four dword loads per plane.  Two aligned 16-byte loads and a
//     select measured 4 % faster without eps and 5 % slower with it, the form the correction runs.  With eps the
//     arithmetic per sample is cfo_rotate_kernel's at scale -1, so the bits are those of a plain cut-out followed by that kernel.
//   * sync_embed_kernel: streaming over the capture's 16-byte words; a sample inside [theta, theta + len) is the packet's, every other the
//     margin draw (zero when std is null or 0).
//   theta outside 0 .. span is clamped into the range by extract and embed: nothing outside the arrays is touched.
// The kernels are templates compiled without packed fp32 and included behind everything else, so they are emitted behind the earlier ones.
#pragma once
#include "cfo.hip.h"                 // CFO_SYM, CFO_CP, CFO_FFT, HY_KERNEL
#include "synth_structured.hip.h"    // ss_key
#include "rng.hip.h"

namespace csi {

constexpr int SYNC_THREADS = 256;
constexpr int SYNC_SPAN_MAX = 256;
constexpr int SYNC_J_MAX = SYNC_SPAN_MAX + CFO_CP;      // folded positions at most: 320
constexpr uint64_t SYNC_MARGIN_TAG = 0x53594E43ull;     // "SYNC": km = splitmix64(kn ^ tag), kn the kind-1 noise key of the packet

struct SyncMetricArgs {
    const float* c_re;                       // [npkt][nr][L], at the call's first packet
    const float* c_im;
    int* theta;                              // [npkt]
    double* eps;                             // [npkt] or null
    float* quality;                          // [npkt] or null
    double* metric;                          // [npkt][span + 1] or null
    double rho;
    int nt, nr, span;
};

struct SyncExtractArgs {
    const float* c_re;                       // [npkt][nr][L]
    const float* c_im;
    float* y_re;                             // [npkt][nr][320 nt]
    float* y_im;
    const int* theta;                        // [npkt]
    const double* eps;                       // [npkt] or null
    long long row;                           // samples of one (packet, rx) of the output: 320 nt
    long long groups;                        // 16-byte words of a packet and plane of the output: nr 80 nt
    int nr, span;
    int wg_per_pkt;
};

struct SyncEmbedArgs {
    const float* x_re;                       // [npkt][nr][320 nt]
    const float* x_im;
    float* c_re;                             // [npkt][nr][L]
    float* c_im;
    const int* theta;                        // [npkt]
    const float* std;                        // [npkt] or null
    uint64_t seed;
    long long first_pkt;
    long long row;                           // 320 nt
    long long cap_row;                       // L
    long long groups;                        // 16-byte words of a packet and plane of the capture: nr L / 4
    int nr, span;
    int wg_per_pkt;
};

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
__device__ __forceinline__ int sync_clamp(int theta, int span) { return theta < 0 ? 0 : (theta > span ? span : theta); }

// UNUSED only makes the kernel a template
template <int UNUSED>
HY_KERNEL __launch_bounds__(SYNC_THREADS) void sync_metric_kernel(const SyncMetricArgs a) {
    // part: the lanes' partial sums [3][K][J] (J K <= 1024); behind the fold it holds the window sums [3][span + 1] and Lambda [span + 1]
    __shared__ double part[3 * 4 * SYNC_THREADS];
    __shared__ double fold[3 * SYNC_J_MAX];
    __shared__ int best[SYNC_THREADS];
    const int tid = threadIdx.x;
    const int J = a.span + CFO_CP;
    const int items = J >> 2;
    const int K = SYNC_THREADS / items;                      // 3 .. 15 strides
    const int rows = a.nr * a.nt;
    const size_t L = (size_t)CFO_SYM * (size_t)a.nt + (size_t)a.span;
    const size_t pkt = (size_t)blockIdx.x * (size_t)a.nr * L;
    const int k = tid / items, i = tid - k * items;
    if (k < K) {
        double qr[4] = {0.0, 0.0, 0.0, 0.0}, qi[4] = {0.0, 0.0, 0.0, 0.0}, en[4] = {0.0, 0.0, 0.0, 0.0};
        for (int m = k; m < rows; m += K) {
            const int r = m / a.nt, s = m - r * a.nt;
            const size_t o = pkt + (size_t)r * L + (size_t)s * CFO_SYM + 4 * (size_t)i;
            const float4 v0 = *reinterpret_cast<const float4*>(a.c_re + o);
            const float4 v1 = *reinterpret_cast<const float4*>(a.c_im + o);
            const float4 v2 = *reinterpret_cast<const float4*>(a.c_re + o + CFO_FFT);
            const float4 v3 = *reinterpret_cast<const float4*>(a.c_im + o + CFO_FFT);
            const float ar[4] = {v0.x, v0.y, v0.z, v0.w}, ai[4] = {v1.x, v1.y, v1.z, v1.w};
            const float br[4] = {v2.x, v2.y, v2.z, v2.w}, bi[4] = {v3.x, v3.y, v3.z, v3.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                qr[j] += (double)fmaf(ai[j], bi[j], ar[j] * br[j]);          // conj(a) b
                qi[j] += (double)fmaf(-ai[j], br[j], ar[j] * bi[j]);
                en[j] += (double)fmaf(ar[j], ar[j], ai[j] * ai[j]);
                en[j] += (double)fmaf(br[j], br[j], bi[j] * bi[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int at = k * J + 4 * i + j;
            part[at] = qr[j];
            part[K * J + at] = qi[j];
            part[2 * K * J + at] = en[j];
        }
    }
    __syncthreads();
    for (int j = tid; j < J; j += SYNC_THREADS) {
        double sr = 0.0, si = 0.0, se = 0.0;
        for (int kk = 0; kk < K; ++kk) {
            sr += part[kk * J + j];
            si += part[K * J + kk * J + j];
            se += part[2 * K * J + kk * J + j];
        }
        fold[j] = sr;
        fold[SYNC_J_MAX + j] = si;
        fold[2 * SYNC_J_MAX + j] = se;
    }
    __syncthreads();
    const int nth = a.span + 1;
    double* const w_r = part;
    double* const w_i = part + nth;
    double* const w_e = part + 2 * nth;
    double* const lam = part + 3 * nth;
    for (int th = tid; th < nth; th += SYNC_THREADS) {
        double sr = 0.0, si = 0.0, se = 0.0;
        for (int m = 0; m < CFO_CP; ++m) {
            sr += fold[th + m];
            si += fold[SYNC_J_MAX + th + m];
            se += fold[2 * SYNC_J_MAX + th + m];
        }
        const double phi = 0.5 * se;
        const double v = sqrt(sr * sr + si * si) - a.rho * phi;
        w_r[th] = sr;
        w_i[th] = si;
        w_e[th] = phi;
        lam[th] = v;
        if (a.metric) a.metric[(size_t)blockIdx.x * (size_t)nth + th] = v;
    }
    __syncthreads();
    // lane t stands for theta = t, lane 0 also for theta = 256; the lower theta stays on equal values
    int mine = tid < nth ? tid : -1;
    if (tid == 0 && nth > SYNC_THREADS && lam[SYNC_THREADS] > lam[0]) mine = SYNC_THREADS;
    best[tid] = mine;
    __syncthreads();
    for (int h = SYNC_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const int p = best[tid], q = best[tid + h];
            if (q >= 0 && p >= 0) {
                const double vp = lam[p], vq = lam[q];
                if (vq > vp || (vq == vp && q < p)) best[tid] = q;
            } else if (p < 0) {
                best[tid] = q;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int th = sync_clamp(best[0], a.span);
        const double sr = w_r[th], si = w_i[th], phi = w_e[th];
        const bool none = phi == 0.0;
        a.theta[blockIdx.x] = th;
        if (a.eps) a.eps[blockIdx.x] = none ? 0.0 : atan2(si, sr) * 0.15915494309189533577;      // 1 / (2 pi)
        if (a.quality) a.quality[blockIdx.x] = none ? 0.0f : (float)(sqrt(sr * sr + si * si) / phi);
    }
}

// UNUSED only makes the kernel a template
template <int UNUSED>
HY_KERNEL __launch_bounds__(SYNC_THREADS) void sync_extract_kernel(const SyncExtractArgs a) {
    const long long p = blockIdx.x / a.wg_per_pkt;
    const long long q = (long long)(blockIdx.x - p * a.wg_per_pkt) * SYNC_THREADS + threadIdx.x;      // 16-byte word of the output packet
    if (q >= a.groups) return;
    const long long r = (4 * q) / a.row, n0 = 4 * q - r * a.row;
    const size_t cap_row = (size_t)a.row + (size_t)a.span;
    const size_t src = ((size_t)p * (size_t)a.nr + (size_t)r) * cap_row + (size_t)sync_clamp(a.theta[p], a.span) + (size_t)n0;
    const size_t o = ((size_t)p * (size_t)a.groups + (size_t)q) * 4;
    float vr[4], vi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        vr[j] = a.c_re[src + j];
        vi[j] = a.c_im[src + j];
    }
    const double f = a.eps ? -1.0 * a.eps[p] * (1.0 / CFO_FFT) : 0.0;      // turns per sample: cfo_rotate_kernel's at scale -1
    if (f != 0.0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double turns = f * (double)(n0 + j);
            const float fr = (float)(turns - rint(turns));
            float s, c;
            sincospif(2.0f * fr, &s, &c);
            const float xr = vr[j], xi = vi[j];
            vr[j] = fmaf(-xi, s, xr * c);
            vi[j] = fmaf(xi, c, xr * s);
        }
    }
    *reinterpret_cast<float4*>(a.y_re + o) = make_float4(vr[0], vr[1], vr[2], vr[3]);
    *reinterpret_cast<float4*>(a.y_im + o) = make_float4(vi[0], vi[1], vi[2], vi[3]);
}

// UNUSED only makes the kernel a template
template <int UNUSED>
HY_KERNEL __launch_bounds__(SYNC_THREADS) void sync_embed_kernel(const SyncEmbedArgs a) {
    const long long p = blockIdx.x / a.wg_per_pkt;
    const long long q = (long long)(blockIdx.x - p * a.wg_per_pkt) * SYNC_THREADS + threadIdx.x;      // 16-byte word of the capture packet
    if (q >= a.groups) return;
    const long long r = (4 * q) / a.cap_row, n0 = 4 * q - r * a.cap_row;
    const long long th = sync_clamp(a.theta[p], a.span);
    const float sd = a.std ? a.std[p] : 0.0f;
    const uint64_t km = splitmix64(ss_key(a.seed, (uint64_t)(a.first_pkt + p), 1) ^ SYNC_MARGIN_TAG);
    const size_t x0 = ((size_t)p * (size_t)a.nr + (size_t)r) * (size_t)a.row;
    float vr[4], vi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long n = n0 + j, k = n - th;
        if (k >= 0 && k < a.row) {
            vr[j] = a.x_re[x0 + (size_t)k];
            vi[j] = a.x_im[x0 + (size_t)k];
        } else if (sd != 0.0f) {
            const uint64_t e = (uint64_t)r * (uint64_t)a.cap_row + (uint64_t)n;
            vr[j] = sd * tr_normal(km, 2 * e);
            vi[j] = sd * tr_normal(km, 2 * e + 1);
        } else {
            vr[j] = 0.0f;
            vi[j] = 0.0f;
        }
    }
    const size_t o = ((size_t)p * (size_t)a.groups + (size_t)q) * 4;
    *reinterpret_cast<float4*>(a.c_re + o) = make_float4(vr[0], vr[1], vr[2], vr[3]);
    *reinterpret_cast<float4*>(a.c_im + o) = make_float4(vi[0], vi[1], vi[2], vi[3]);
}
#endif

}  // namespace csi
