// lmmse.hip.h - LMMSE smoothing of the LS estimate.
//
// Reference: LMMSE_ce.m:23-39, called per link from helperMIMOChannelEstimate.m:37-39 with
// Nfft = Np = 234 and Nps = 1:
//     H_mmse = Rhp * inv(Rpp) * H_ls,   Rhp[a][b] = 1 / (1 + j 2 pi tau_rms (a-b) / 234),
//                                       Rpp = Rhp + I / snr
// where tau_rms is the rms "delay" of the vector h the caller passes and snr = 10^(SNR/10).
// The reference inverts the 234x234 matrix once per (tx, rx) link (its slowest stage: 1.1 s per
// packet at Nt = 32, timing_cpu_vs_gpu_barplot.eps).  Here:
//   * R is Hermitian Toeplitz and identical for the Nt links of an rx antenna, and
//     R (R + s I)^-1 H = H - s (R + s I)^-1 H, so only ONE Hermitian-Toeplitz system with Nt
//     right-hand sides is solved per (packet, rx) - no inverse, no 234x234 matrix in memory.
//   * Levinson recursion (O(n^2) per right-hand side, O(n) storage), in fp64 (the vector fp64
//     rate of gfx950 makes this cheap).  The condition number of R + s I grows with the SNR and
//     as tau_rms shrinks: hundreds for tau_rms of 20-30 bins, but with the sweep's 8-tap profile
//     (tau_rms 0.95) 1.3e3 at 10 dB, 4e4 at 25 dB and 1.3e6 at 40 dB, and 234 / s for one tap
//     (2.3e8 at 60 dB) - fp32 would not do.
//   * one workgroup per (packet, rx, 32 tx antennas): 8 lanes per right-hand side, each lane keeps
//     30 solution entries in registers; the shared forward vector lives in LDS (ping-pong, one
//     barrier per recursion step); the LS columns are staged in LDS and reused for the output.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csi {

constexpr int LM_N = 234;
constexpr int LM_RHS = 32;                 // right-hand sides per workgroup
constexpr int LM_PART = 8;                 // lanes per right-hand side
constexpr int LM_EPL = (LM_N + LM_PART - 1) / LM_PART;     // 30 entries per lane
constexpr int LM_THREADS = LM_RHS * LM_PART;

struct LmmseArgs {
    const float* h_re;      // LS estimate [nblk][nt][234]
    const float* h_im;
    const float* hvec;      // [npkt][L]  the vector LMMSE_ce receives as 'h'
    const float* snr_db;    // [nblk]     SNR(i) per (packet, rx)
    float* o_re;            // [nblk][nt][234]
    float* o_im;
    int nt, nr, L;
};

struct cd {
    double x, y;
};
__device__ __forceinline__ cd cmul(cd a, cd b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cd cfma(cd a, cd b, cd c) {          // a*b + c
    return {fma(a.x, b.x, fma(-a.y, b.y, c.x)), fma(a.x, b.y, fma(a.y, b.x, c.y))};
}
__device__ __forceinline__ cd cconj(cd a) { return {a.x, -a.y}; }
__device__ __forceinline__ cd group_sum(cd v) {                  // over the 8 lanes of a right-hand side
#pragma unroll
    for (int o = 1; o < LM_PART; o <<= 1) {
        v.x += __shfl_xor(v.x, o);
        v.y += __shfl_xor(v.y, o);
    }
    return v;
}

__global__ __launch_bounds__(LM_THREADS) void lmmse_levinson_kernel(const LmmseArgs a, int n_jc) {
    __shared__ cd t[LM_N];                       // first column of the normalised matrix, t[0] = 1
    __shared__ cd f[2][LM_N];                    // forward vector, ping-pong
    __shared__ float2 y[LM_RHS][LM_N];           // LS columns, later the output

    const int tid = threadIdx.x;
    const int jl = tid / LM_PART, e = tid % LM_PART;
    const size_t blk = blockIdx.x / n_jc;
    const int jc = blockIdx.x % n_jc;
    const int p = (int)(blk / a.nr);

    // rms "delay" of h (LMMSE_ce.m:27-30); every thread evaluates it (L is ~100)
    double hh = 0.0, s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < a.L; ++k) {
        const double v = (double)a.hvec[(size_t)p * a.L + k];
        const double w = v * v;
        hh += w;
        s1 += w * k;
        s2 += w * k * (double)k;
    }
    // an all-zero h has no delay spread: tau_rms = 0 (LMMSE_ce.m divides 0 by 0 there and returns NaN)
    double tau_rms = 0.0;
    if (hh > 0.0) {
        const double r = s1 / hh, r2 = s2 / hh;
        tau_rms = sqrt(fmax(r2 - r * r, 0.0));
    }
    const double c = 2.0 * M_PI * tau_rms / LM_N;                       // :31-32, df = 1/Nfft
    const double sig2 = pow(10.0, -0.1 * (double)a.snr_db[blk]);        // 1/snr
    const double t0 = 1.0 + sig2;                                       // diagonal of Rpp

    if (tid < LM_N) {
        const double d = (double)tid;
        const double den = (1.0 + c * c * d * d) * t0;                  // 1/(1 + j c d) = (1 - j c d)/(1 + c^2 d^2)
        t[tid] = tid == 0 ? cd{1.0, 0.0} : cd{1.0 / den, -c * d / den};
    }
    // stage the LS columns of this workgroup's tx antennas
    const int j0 = jc * LM_RHS;
    for (int idx = tid; idx < LM_RHS * LM_N; idx += LM_THREADS) {
        const int jj = idx / LM_N, k = idx - jj * LM_N;
        float2 v = {0.f, 0.f};
        if (j0 + jj < a.nt) {
            const size_t o = (blk * a.nt + j0 + jj) * LM_N + k;
            v = float2{a.h_re[o], a.h_im[o]};
        }
        y[jj][k] = v;
    }
    if (tid == 0) f[0][0] = cd{1.0, 0.0};
    __syncthreads();

    // x[u] <-> solution entry 8u + e of right-hand side jl (normalised system M z = y)
    cd x[LM_EPL];
#pragma unroll
    for (int u = 0; u < LM_EPL; ++u) x[u] = cd{0.0, 0.0};
    if (e == 0) x[0] = cd{(double)y[jl][0].x, (double)y[jl][0].y};

    for (int k = 1; k < LM_N; ++k) {
        const cd* fc = f[(k - 1) & 1];           // length k
        cd* fn = f[k & 1];                       // length k + 1
        // forward error ef = sum_{i<k} t[k-i] fc[i]; error of the solution ex = sum_{i<k} t[k-i] x[i]
        cd ef = {0.0, 0.0}, ex = {0.0, 0.0};
#pragma unroll
        for (int u = 0; u < LM_EPL; ++u) {
            const int i = LM_PART * u + e;
            if (i < k) {
                const cd tk = t[k - i];
                ef = cfma(tk, fc[i], ef);
                ex = cfma(tk, x[u], ex);
            }
        }
        ef = group_sum(ef);
        ex = group_sum(ex);
        const double inv = 1.0 / (1.0 - (ef.x * ef.x + ef.y * ef.y));
        // fn = ([fc; 0] - ef [0; conj(reverse(fc))]) / (1 - |ef|^2)
        if (tid <= k) {
            const cd fe = tid < k ? fc[tid] : cd{0.0, 0.0};
            const cd be = tid > 0 ? cconj(fc[k - tid]) : cd{0.0, 0.0};
            const cd m = cmul(ef, be);
            fn[tid] = cd{(fe.x - m.x) * inv, (fe.y - m.y) * inv};
        }
        __syncthreads();
        // x <- [x; 0] + (y_k - ex) * conj(reverse(fn))
        const float2 yk = y[jl][k];
        const cd coef = {(double)yk.x - ex.x, (double)yk.y - ex.y};
#pragma unroll
        for (int u = 0; u < LM_EPL; ++u) {
            const int i = LM_PART * u + e;
            if (i <= k) x[u] = cfma(coef, cconj(fn[k - i]), x[u]);
        }
    }
    __syncthreads();
    // H_mmse = H_ls - (sig2 / t0) z      (R (R + s I)^-1 H = H - s (R + s I)^-1 H, z solves M z = H)
    const double g = sig2 / t0;
#pragma unroll
    for (int u = 0; u < LM_EPL; ++u) {
        const int i = LM_PART * u + e;
        if (i < LM_N) {
            const float2 v = y[jl][i];
            y[jl][i] = float2{(float)((double)v.x - g * x[u].x), (float)((double)v.y - g * x[u].y)};
        }
    }
    __syncthreads();
    for (int idx = tid; idx < LM_RHS * LM_N; idx += LM_THREADS) {
        const int jj = idx / LM_N, k = idx - jj * LM_N;
        if (j0 + jj < a.nt) {
            const size_t o = (blk * a.nt + j0 + jj) * LM_N + k;
            a.o_re[o] = y[jj][k].x;
            a.o_im[o] = y[jj][k].y;
        }
    }
}

// The smoother with a MEASURED first column (lmmse_blind_kernel below; the model is in the header of the second half of this file)
struct LmmseBlindArgs {
    const float* h_re;      // LS estimate [nblk][nt][234]
    const float* h_im;
    const double* nv;       // [nblk]          noise variance per complex bin of a sounding symbol (lmmse_null_noise_kernel)
    const cd* corr;         // [nblk][234]     sample frequency correlation c[d] (lmmse_freq_corr_kernel)
    float* o_re;            // [nblk][nt][234]
    float* o_im;
    int* fallback;          // [nblk]          1 where the recursion broke down and the LS rows went out unchanged
    int nt, nr;
};

// ---------------------------------------------------------------------------------------------------------------------------------
// LMMSE smoothing from the packet's own statistics (csi_lmmse_blind[_device]): no input that only a simulator has.
//
// Per (packet, rx), in the contiguous-index convention of the smoother above (Nfft = Np = 234, Nps = 1):
//   noise        The VHT-LTF is zero on the 14 null carriers (1-based shifted bins [1:7 129 251:256] = FFT bins 0 and 122 ... 134), so
//                what a sounding symbol carries there is noise:  Y[s][b] = sum_{n<256} x[320 s + 64 + n] exp(-2 pi i b n / 256),
//                nv = sum |Y|^2 / (14 Nt).  The DC bin (b = 0) IS counted: the generators put no offset there, and a receiver that has
//                one would see it in nv.  nv is the variance per complex bin of one symbol in the units of h; an LS row averages Nt
//                symbols (P P^T = Nt I), so its error variance is nv / Nt.
//   correlation  the Nt links of one rx antenna share a delay profile:  c[d] = 1 / (234 Nt) sum_j sum_{k < 234 - d} h[j][k + d] conj(h[j][k]).
//                The BIASED estimate (divisor 234 at every lag): Toeplitz(c) is then positive definite for any non-zero input.
//   smoother     T = Toeplitz(c) estimates R_h + (nv / Nt) I as it stands:  out[j] = h[j] - (nv / Nt) T^-1 h[j], the recursion above on
//                t[d] = c[d] / c[0] with the gain (nv / Nt) / c[0].
//   guards       c[0] == 0 (all-zero rows): out = h.  A recursion step whose 1 - |ef|^2 is not in (0, 1]: out = h for that (packet, rx)
//                and fallback[blk] = 1 (lmmse_blind_count_kernel adds the flags to the context's counter "lmmse_blind_fallbacks").
//                Non-finite inputs are not screened; they end in that fallback.
// fp64 throughout, every sum in a fixed order, no atomics: a packet's bits do not depend on the call or chunk that holds it.  Why fp64
// for the statistics: the smallest eigenvalue of T is 1e-5 ... 1e-4 of 234 c[0]; a c accumulated in fp32 (1e-7 relative) would move
// the output by far more than its fp32 rounding.  Products of two fp32 values are exact in fp64.  The null-carrier sums go one step
// further, fp64 pairs (lmb_pair_fma): on noise-free packets they cancel to rounding residue.

constexpr int LMB_NULLS = 14;
constexpr int LMB_SYMS = 16;                         // sounding symbols staged per pass of lmmse_null_noise_kernel
constexpr int LMB_THREADS = 256;
constexpr int LMB_SYM_PITCH = 257;                   // float2 per staged symbol: rows of different symbols start 2 banks apart
constexpr int LMB_FFT = 256, LMB_CP = 64, LMB_SYM = 320;

// cos(2 pi u / 256), u = 0 .. 64, as unevaluated sums hi + lo of two doubles (106 bits; tests/blind_lmmse_ref.py twiddles_exact
// computes the same values to 60 digits): the quarter wave the fp64-pair twiddle table of lmmse_null_noise_kernel is built from
static const double kLmbQuarterCos[65][2] = {
    {0x1.0000000000000p+0, 0x0.0p+0},
    {0x1.ffd886084cd0dp-1, -0x1.1354d4556e4cbp-55},
    {0x1.ff621e3796d7ep-1, -0x1.c57bc2e24aa15p-57},
    {0x1.fe9cdad01883ap-1, 0x1.521ecd0c67e35p-57},
    {0x1.fd88da3d12526p-1, -0x1.87df6378811c7p-55},
    {0x1.fc26470e19fd3p-1, 0x1.1ec8668ecaceep-55},
    {0x1.fa7557f08a517p-1, -0x1.7a0a8ca13571fp-55},
    {0x1.f8764fa714ba9p-1, 0x1.ab256778ffcb6p-56},
    {0x1.f6297cff75cb0p-1, 0x1.562172a361fd3p-56},
    {0x1.f38f3ac64e589p-1, -0x1.d7bafb51f72e6p-56},
    {0x1.f0a7efb9230d7p-1, 0x1.52c7adc6b4989p-56},
    {0x1.ed740e7684963p-1, 0x1.e82c791f59cc2p-56},
    {0x1.e9f4156c62ddap-1, 0x1.760b1e2e3f81ep-55},
    {0x1.e6288ec48e112p-1, -0x1.16b56f2847754p-57},
    {0x1.e212104f686e5p-1, -0x1.014c76c126527p-55},
    {0x1.ddb13b6ccc23cp-1, 0x1.83c37c6107db3p-55},
    {0x1.d906bcf328d46p-1, 0x1.457e610231ac2p-56},
    {0x1.d4134d14dc93ap-1, -0x1.4ef5295d25af2p-55},
    {0x1.ced7af43cc773p-1, -0x1.e7b6bb5ab58aep-58},
    {0x1.c954b213411f5p-1, -0x1.2fb761e946603p-58},
    {0x1.c38b2f180bdb1p-1, -0x1.6e0b1757c8d07p-56},
    {0x1.bd7c0ac6f952ap-1, -0x1.825a732ac700ap-55},
    {0x1.b728345196e3ep-1, -0x1.bc69f324e6d61p-55},
    {0x1.b090a58150200p-1, -0x1.926da300ffccep-55},
    {0x1.a9b66290ea1a3p-1, 0x1.9f630e8b6dac8p-60},
    {0x1.a29a7a0462782p-1, -0x1.128bb015df175p-56},
    {0x1.9b3e047f38741p-1, -0x1.30ee286712474p-55},
    {0x1.93a22499263fbp-1, 0x1.3d419a920df0bp-55},
    {0x1.8bc806b151741p-1, -0x1.2c5e12ed1336dp-55},
    {0x1.83b0e0bff976ep-1, -0x1.6f420f8ea3475p-56},
    {0x1.7b5df226aafafp-1, -0x1.0f537acdf0ad7p-56},
    {0x1.72d0837efff96p-1, 0x1.0d4ef0f1d915cp-55},
    {0x1.6a09e667f3bcdp-1, -0x1.bdd3413b26456p-55},
    {0x1.610b7551d2cdfp-1, -0x1.251b352ff2a37p-56},
    {0x1.57d69348ceca0p-1, -0x1.75720992bfbb2p-55},
    {0x1.4e6cabbe3e5e9p-1, 0x1.3c293edceb327p-57},
    {0x1.44cf325091dd6p-1, 0x1.8076a2cfdc6b3p-57},
    {0x1.3affa292050b9p-1, 0x1.e3e25e3954964p-56},
    {0x1.30ff7fce17035p-1, -0x1.efcc626f74a6fp-57},
    {0x1.26d054cdd12dfp-1, -0x1.5da743ef3770cp-55},
    {0x1.1c73b39ae68c8p-1, 0x1.b25dd267f6600p-55},
    {0x1.11eb3541b4b23p-1, -0x1.ef23b69abe4f1p-55},
    {0x1.073879922ffeep-1, -0x1.a5a014347406cp-55},
    {0x1.f8ba4dbf89abap-2, -0x1.2ec1fc1b776b8p-60},
    {0x1.e2b5d3806f63bp-2, 0x1.e0d891d3c6841p-58},
    {0x1.cc66e9931c45ep-2, 0x1.6850e59c37f8fp-58},
    {0x1.b5d1009e15cc0p-2, 0x1.5b362cb974183p-57},
    {0x1.9ef7943a8ed8ap-2, 0x1.6da81290bdbabp-57},
    {0x1.87de2a6aea963p-2, -0x1.72cedd3d5a610p-57},
    {0x1.7088530fa459fp-2, -0x1.44b19e0864c5dp-56},
    {0x1.58f9a75ab1fddp-2, -0x1.efdc0d58cf620p-62},
    {0x1.4135c94176601p-2, 0x1.0c97c4afa2518p-56},
    {0x1.294062ed59f06p-2, -0x1.5d28da2c4612dp-56},
    {0x1.111d262b1f677p-2, 0x1.824c20ab7aa9ap-56},
    {0x1.f19f97b215f1bp-3, -0x1.42deef11da2c4p-57},
    {0x1.c0b826a7e4f63p-3, -0x1.af1439e521935p-62},
    {0x1.8f8b83c69a60bp-3, -0x1.26d19b9ff8d82p-57},
    {0x1.5e214448b3fc6p-3, 0x1.531ff779ddac6p-57},
    {0x1.2c8106e8e613ap-3, 0x1.13000a89a11e0p-58},
    {0x1.f564e56a9730ep-4, 0x1.a2704729ae56dp-59},
    {0x1.917a6bc29b42cp-4, -0x1.e2718d26ed688p-60},
    {0x1.2d52092ce19f6p-4, -0x1.9a088a8bf6b2cp-59},
    {0x1.91f65f10dd814p-5, -0x1.912bd0d569a90p-61},
    {0x1.92155f7a3667ep-6, -0x1.b1d63091a0130p-64},
    {0x0.0p+0, 0x0.0p+0},
};

// exp(-2 pi i u / 256) with each component as an unevaluated sum hi + lo of two doubles
struct LmbTwiddle {
    double re_hi, re_lo, im_hi, im_lo;
};

struct LmmseNoiseArgs {
    const float* ltf_re;    // [nblk][len_ltf]
    const float* ltf_im;
    const LmbTwiddle* tw;   // [256] built on the host, once per context (lmb_build_twiddles)
    double* nv;             // [nblk]
    int nt, len_ltf;
};

// acc += x * (w_hi + w_lo) with acc an fp64 pair (hi, lo): the product of the fp32-valued x with w_hi is split exactly by an fma,
// the sum by Knuth's two-sum; what the hi parts lose goes to lo.  A noise-free packet carries only rounding residue on the null
// carriers: the 256 terms of a Y cancel to 1e-8 of their size, and a plain fp64 sum (1e-16 of a term per step) would leave nv with
// 1e-8 of error.  This way Y is good to 1e-30 of a term.
__device__ __forceinline__ void lmb_pair_fma(double x, double w_hi, double w_lo, double& hi, double& lo) {
#pragma clang fp contract(off)                       // hi + p must be the sum of the ROUNDED product: only the two fma() below fuse
    const double p = x * w_hi;
    const double pe = fma(x, w_hi, -p);
    const double s = hi + p;
    const double bb = s - hi;
    const double se = (hi - (s - bb)) + (p - bb);
    hi = s;
    lo += se + fma(x, w_lo, pe);
}

// One workgroup per (packet, rx).  Up to 16 symbols at a time go through LDS (16-byte loads, coalesced); thread (symbol, null bin)
// sums its 256-term dot product in fp64 pairs; the squared magnitudes of a thread's passes add up in pass order, then one tree over
// the workgroup.
__global__ __launch_bounds__(LMB_THREADS) void lmmse_null_noise_kernel(const LmmseNoiseArgs a) {
    __shared__ float2 xs[LMB_SYMS][LMB_SYM_PITCH];
    __shared__ LmbTwiddle tw[LMB_FFT];
    __shared__ double part[LMB_THREADS];

    const int tid = threadIdx.x;
    const size_t blk = blockIdx.x;
    const float* re = a.ltf_re + blk * (size_t)a.len_ltf;
    const float* im = a.ltf_im + blk * (size_t)a.len_ltf;
    tw[tid] = a.tw[tid];
    const int sl = tid / LMB_NULLS, bi = tid - sl * LMB_NULLS;
    const int b = bi == 0 ? 0 : 121 + bi;            // FFT bins 0, 122 ... 134
    double acc = 0.0;
    for (int s0 = 0; s0 < a.nt; s0 += LMB_SYMS) {
        const int ns = min(LMB_SYMS, a.nt - s0);
        __syncthreads();                             // the previous pass has read xs (first pass: tw is complete)
        for (int q = tid; q < ns * (LMB_FFT / 4); q += LMB_THREADS) {
            const int s = q / (LMB_FFT / 4), n4 = q - s * (LMB_FFT / 4);
            const size_t o = (size_t)(s0 + s) * LMB_SYM + LMB_CP + 4 * n4;
            const float4 r = *reinterpret_cast<const float4*>(re + o);
            const float4 m = *reinterpret_cast<const float4*>(im + o);
            xs[s][4 * n4 + 0] = float2{r.x, m.x};
            xs[s][4 * n4 + 1] = float2{r.y, m.y};
            xs[s][4 * n4 + 2] = float2{r.z, m.z};
            xs[s][4 * n4 + 3] = float2{r.w, m.w};
        }
        __syncthreads();
        if (sl < ns) {
            double yr_h = 0.0, yr_l = 0.0, yi_h = 0.0, yi_l = 0.0;
            int u = 0;
            for (int n = 0; n < LMB_FFT; ++n) {
                const float2 v = xs[sl][n];
                const LmbTwiddle w = tw[u];
                const double xr = (double)v.x, xi = (double)v.y;
                lmb_pair_fma(xr, w.re_hi, w.re_lo, yr_h, yr_l);          // (xr + i xi)(wr + i wi)
                lmb_pair_fma(-xi, w.im_hi, w.im_lo, yr_h, yr_l);
                lmb_pair_fma(xr, w.im_hi, w.im_lo, yi_h, yi_l);
                lmb_pair_fma(xi, w.re_hi, w.re_lo, yi_h, yi_l);
                u = (u + b) & (LMB_FFT - 1);
            }
            const double yr = yr_h + yr_l, yi = yi_h + yi_l;
            acc += yr * yr + yi * yi;
        }
    }
    part[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int o = LMB_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
    }
    if (tid == 0) a.nv[blk] = part[0] / (double)(LMB_NULLS * a.nt);
}

struct LmmseCorrArgs {
    const float* h_re;      // LS estimate [nblk][nt][234]
    const float* h_im;
    cd* corr;               // [nblk][234]
    int nt;
};

// One workgroup per (packet, rx); lane = lag d.  The LS rows pass through LDS in groups of at most 32 tx, as the smoother stages
// them (all 128 rows do not fit); y[j][k] is a broadcast read and y[j][k + d] consecutive across the lanes.  The sum runs over the
// rows in order and, inside a row, over k in order.  (Lanes of large lags idle for most of a row: about 2x on a kernel with a
// quarter of the smoother's flops.)
__global__ __launch_bounds__(LMB_THREADS) void lmmse_freq_corr_kernel(const LmmseCorrArgs a) {
    __shared__ float2 y[LM_RHS][LM_N];

    const int tid = threadIdx.x;
    const size_t blk = blockIdx.x;
    cd acc = {0.0, 0.0};
    for (int j0 = 0; j0 < a.nt; j0 += LM_RHS) {
        const int nj = min(LM_RHS, a.nt - j0);
        __syncthreads();
        for (int idx = tid; idx < nj * LM_N; idx += LMB_THREADS) {
            const size_t o = (blk * a.nt + j0) * LM_N + idx;
            (&y[0][0])[idx] = float2{a.h_re[o], a.h_im[o]};
        }
        __syncthreads();
        if (tid < LM_N) {
            for (int jj = 0; jj < nj; ++jj) {
                for (int k = 0; k < LM_N - tid; ++k) {
                    const float2 u = y[jj][k + tid], v = y[jj][k];
                    acc = cfma(cd{(double)u.x, (double)u.y}, cd{(double)v.x, -(double)v.y}, acc);      // h[k + d] conj(h[k])
                }
            }
        }
    }
    if (tid < LM_N) {
        const double s = 1.0 / ((double)LM_N * (double)a.nt);
        a.corr[blk * LM_N + tid] = cd{acc.x * s, acc.y * s};
    }
}

// The recursion of lmmse_levinson_kernel on a measured first column: t[d] = c[d] / c[0], gain (nv / Nt) / c[0], and the two guards.
// Its own kernel, not a shared body: lmmse_levinson_kernel built from a shared template body (set-up and gain under `if constexpr`)
// came out as different machine code (2121 instead of 2361 instructions, tools/device_code_diff.py), and that kernel's results
// are pinned.  Everything between the set-up of t[] and the output step is that kernel's text.
__global__ __launch_bounds__(LM_THREADS) void lmmse_blind_kernel(const LmmseBlindArgs a, int n_jc) {
    __shared__ cd t[LM_N];                       // first column of the normalised matrix, t[0] = 1
    __shared__ cd f[2][LM_N];                    // forward vector, ping-pong
    __shared__ float2 y[LM_RHS][LM_N];           // LS columns, later the output

    const int tid = threadIdx.x;
    const int jl = tid / LM_PART, e = tid % LM_PART;
    const size_t blk = blockIdx.x / n_jc;
    const int jc = blockIdx.x % n_jc;

    // T = Toeplitz(c) is R_h + sig^2 I already; normalised by c[0] (real: a sum of |h|^2)
    const double c0 = a.corr[blk * LM_N].x;
    bool skip = c0 == 0.0;                       // all-zero LS rows: no recursion, out = h_ls (uniform over the workgroup)
    const double g = a.nv[blk] / (double)a.nt / c0;
    if (jc == 0 && tid == 0) a.fallback[blk] = 0;
    if (tid < LM_N) {
        const cd cv = a.corr[blk * LM_N + tid];
        t[tid] = tid == 0 ? cd{1.0, 0.0} : cd{cv.x / c0, cv.y / c0};
    }
    // stage the LS columns of this workgroup's tx antennas
    const int j0 = jc * LM_RHS;
    for (int idx = tid; idx < LM_RHS * LM_N; idx += LM_THREADS) {
        const int jj = idx / LM_N, k = idx - jj * LM_N;
        float2 v = {0.f, 0.f};
        if (j0 + jj < a.nt) {
            const size_t o = (blk * a.nt + j0 + jj) * LM_N + k;
            v = float2{a.h_re[o], a.h_im[o]};
        }
        y[jj][k] = v;
    }
    if (tid == 0) f[0][0] = cd{1.0, 0.0};
    __syncthreads();

    // x[u] <-> solution entry 8u + e of right-hand side jl (normalised system M z = y)
    cd x[LM_EPL];
#pragma unroll
    for (int u = 0; u < LM_EPL; ++u) x[u] = cd{0.0, 0.0};
    if (e == 0) x[0] = cd{(double)y[jl][0].x, (double)y[jl][0].y};

    for (int k = 1; k < LM_N && !skip; ++k) {
        const cd* fc = f[(k - 1) & 1];           // length k
        cd* fn = f[k & 1];                       // length k + 1
        // forward error ef = sum_{i<k} t[k-i] fc[i]; error of the solution ex = sum_{i<k} t[k-i] x[i]
        cd ef = {0.0, 0.0}, ex = {0.0, 0.0};
#pragma unroll
        for (int u = 0; u < LM_EPL; ++u) {
            const int i = LM_PART * u + e;
            if (i < k) {
                const cd tk = t[k - i];
                ef = cfma(tk, fc[i], ef);
                ex = cfma(tk, x[u], ex);
            }
        }
        ef = group_sum(ef);
        ex = group_sum(ex);
        // T is positive definite in exact arithmetic (biased correlation estimate), so 1 - |ef|^2 > 0; a step where rounding or a
        // non-finite input says otherwise ends the recursion.  Every group of 8 lanes sums ef from the same t[] and f[] in the
        // same order: the same bits, so the whole workgroup leaves together, in front of the barrier
        const double den = 1.0 - (ef.x * ef.x + ef.y * ef.y);
        if (!(den > 0.0 && den <= 1.0)) {
            skip = true;
            if (jc == 0 && tid == 0) a.fallback[blk] = 1;
            break;
        }
        const double inv = 1.0 / den;
        // fn = ([fc; 0] - ef [0; conj(reverse(fc))]) / (1 - |ef|^2)
        if (tid <= k) {
            const cd fe = tid < k ? fc[tid] : cd{0.0, 0.0};
            const cd be = tid > 0 ? cconj(fc[k - tid]) : cd{0.0, 0.0};
            const cd m = cmul(ef, be);
            fn[tid] = cd{(fe.x - m.x) * inv, (fe.y - m.y) * inv};
        }
        __syncthreads();
        // x <- [x; 0] + (y_k - ex) * conj(reverse(fn))
        const float2 yk = y[jl][k];
        const cd coef = {(double)yk.x - ex.x, (double)yk.y - ex.y};
#pragma unroll
        for (int u = 0; u < LM_EPL; ++u) {
            const int i = LM_PART * u + e;
            if (i <= k) x[u] = cfma(coef, cconj(fn[k - i]), x[u]);
        }
    }
    __syncthreads();
    // out = H_ls - (nv / Nt) / c[0] z, z the solution of the normalised system; the LS rows as they are after a guard
    if (!skip) {
#pragma unroll
        for (int u = 0; u < LM_EPL; ++u) {
            const int i = LM_PART * u + e;
            if (i < LM_N) {
                const float2 v = y[jl][i];
                y[jl][i] = float2{(float)((double)v.x - g * x[u].x), (float)((double)v.y - g * x[u].y)};
            }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < LM_RHS * LM_N; idx += LM_THREADS) {
        const int jj = idx / LM_N, k = idx - jj * LM_N;
        if (j0 + jj < a.nt) {
            const size_t o = (blk * a.nt + j0 + jj) * LM_N + k;
            a.o_re[o] = y[jj][k].x;
            a.o_im[o] = y[jj][k].y;
        }
    }
}

// the fallback flags of one launch, added to the context's counter word: one workgroup, the stream orders it behind the launch
__global__ __launch_bounds__(LMB_THREADS) void lmmse_blind_count_kernel(const int* fallback, long long nblk, long long* counter) {
    __shared__ long long part[LMB_THREADS];
    const int tid = threadIdx.x;
    long long n = 0;
    for (long long i = tid; i < nblk; i += LMB_THREADS) n += fallback[i] != 0;
    part[tid] = n;
    __syncthreads();
#pragma unroll
    for (int o = LMB_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
    }
    if (tid == 0) *counter += part[0];
}

}  // namespace csi
