// forecast.hip.h - channel forecasting: a linear predictor over several soundings (host side: csi_forecast.hpp).
//
// The soundings x_0 .. x_{P-1} run oldest to newest, equally spaced; each is a CSI plane pair [npkt][Nr][Nt][234].  Per block
// (packet, rx), with K = Nt 234 the contiguous floats of a block in every plane, order M, horizon d (sounding intervals),
// 2 <= P <= 16, 1 <= M <= 8, d >= 1, M + d <= P:
//   T[i][q]  = sum_k conj(x_i[k]) x_q[k]                              P x P, Hermitian                 forecast_gram_kernel
//   G[a][b]  = sum_{p = M+d-1}^{P-1} T[p-d-a][p-d-b]                  M x M
//   rhs[a]   = sum_{p = M+d-1}^{P-1} T[p-d-a][p]
//   (G + ridge trace(G) / M I) c = rhs                                fp64 Cholesky                    forecast_fit_kernel
//   y[k]     = sum_{m < M} c_m x_{P-1-m}[k]                           the forecast of x at index P-1+d  forecast_apply_kernel
// Pooling (flag bit 0): G, rhs and the target energy of a packet's receive antennas are added in ascending rx order before the solve
// and every rx of the packet gets the same c.  A pivot <= 0 or not finite (all-zero planes included) gives c = (1, 0, .., 0): the newest
// sounding is held, info = 1 (0 otherwise).  fit_err = max(0, 1 - Re(c^H rhs) / sum_{p = M+d-1}^{P-1} T[p][p]) with the fp64 c (0 where
// that energy is not positive): the in-sample relative residual.
//
// Plan:
//   * forecast_gram_kernel<PMAX>: one workgroup of 4 waves per block.  The soundings, padded to 16 with zero rows, are the 16 rows of
//     three v_mfma_f32_16x16x4_f32 products per four floats of K: RR = Xr Xr^T, II = Xi Xi^T, RI = Xr Xi^T; re T = RR + II,
//     im T[i][q] = RI[i][q] - RI[q][i].  The A and the B operand of this MFMA form have the same lane map (row or column l & 15,
//     k = l >> 4), so one register serves as both.  K goes through LDS in slabs of 256 floats per sounding and component, read along K
//     one slab ahead into registers as 8-byte words - a block starts on an 8-byte boundary whatever Nt is (936 bytes per row), on a
//     16-byte one only when Nt (p Nr + r) is even, so nothing wider is assumed - and stored with a row stride of 260 floats (16-byte rows,
//     = 4 mod 64 banks).  Wave w takes floats 64 w .. 64 w + 63 of every slab as four 16-byte reads per component (lane: row l & 15,
//     floats 16 j + 4 (l >> 4) .. + 3), each feeding four k steps; the floats past K enter as zeros.  The four partial sums are added in
//     wave order through LDS.  Only i >= q is taken and mirrored, the diagonal's imaginary part is 0: T is Hermitian to the bit.  No
//     atomics; the order of every sum is fixed by (K, P) alone.
//   * forecast_fit_kernel: one lane per block (per packet when pooled), everything in fp64, c rounded once to fp32.
//   * forecast_apply_kernel<MMAX>: streaming, 8-byte words; per element the fp32 complex FMAs run in the order m = 0 .. M-1
//     (re: fma(cr, xr, .), fma(-ci, xi, .); im: fma(cr, xi, .), fma(ci, xr, .)).
//   * sounding_noise_kernel: out = x + s (n_re + i n_im), s = sqrtf(0.5f v[p][r]), n_re / n_im = tr_normal(kn, 2 e) / (kn, 2 e + 1),
//     kn = ss_key(seed, first_pkt + p, 1), e = (r Nt + j) 234 + k; one fmaf per component; s == 0 copies the bits; in place allowed.
// The kernels are templates compiled without packed fp32 and included behind everything else, so they are emitted behind the earlier ones.
#pragma once
#include "hybrid_weights.hip.h"      // HY_KERNEL
#include "synth_structured.hip.h"    // ss_key
#include "rng.hip.h"

namespace csi {

constexpr int FC_MAX_SND = 16;
constexpr int FC_MAX_ORDER = 8;
constexpr int FC_N = 234;
constexpr int FC_THREADS = 256;
constexpr int FC_SLAB = 256;                 // floats of K per slab, sounding and component: 64 per wave
constexpr int FC_STRIDE = FC_SLAB + 4;       // row stride in LDS
constexpr int FC_FIT_THREADS = 64;

struct ForecastGramArgs {
    const float* x_re[FC_MAX_SND];           // sounding i, at the call's first block
    const float* x_im[FC_MAX_SND];
    float* t_re;                             // [blocks][P][P]
    float* t_im;
    long long kf;                            // floats of a block (even)
    int n_snd;
};

struct ForecastFitArgs {
    const float* t_re;
    const float* t_im;
    float* c_re;                             // [blocks][M]
    float* c_im;
    float* fit_err;                          // [blocks] or null
    int32_t* info;                           // [blocks] or null
    double ridge;
    long long items;                         // blocks, or packets when pooled
    int nr, n_snd, order, steps, pooled;
};

struct ForecastApplyArgs {
    const float* x_re[FC_MAX_ORDER];         // x_{P-1-m}, at the call's first block
    const float* x_im[FC_MAX_ORDER];
    const float* c_re;                       // [blocks][M]
    const float* c_im;
    float* y_re;
    float* y_im;
    long long kf;
    int order;
};

struct SoundingNoiseArgs {
    const float* x_re;
    const float* x_im;
    float* y_re;
    float* y_im;
    const float* v;                          // [npkt][nr]
    uint64_t seed;
    long long first_pkt;
    long long kf;                            // floats of a block: Nt 234
    int nr;
};

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
typedef float fc_f32x4 __attribute__((ext_vector_type(4)));

template <int PMAX>
HY_KERNEL __launch_bounds__(FC_THREADS) void forecast_gram_kernel(const ForecastGramArgs a) {
    static_assert(PMAX == 4 || PMAX == 8 || PMAX == 16, "rows fetched per slab");
    __shared__ __attribute__((aligned(16))) float fc_s[2 * FC_MAX_SND * FC_STRIDE];      // [re | im][16 rows][260]; then the partial sums
    float* s_re = fc_s;
    float* s_im = fc_s + FC_MAX_SND * FC_STRIDE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = lane & 15, kq = lane >> 4;
    const int P = a.n_snd;
    const long long kf = a.kf;
    const size_t base = (size_t)blockIdx.x * (size_t)kf;
    for (int i = tid; i < 2 * FC_MAX_SND * FC_STRIDE; i += FC_THREADS) fc_s[i] = 0.0f;      // the rows past P stay zero
    fc_f32x4 rr = {0.0f, 0.0f, 0.0f, 0.0f}, ii = rr, ri = rr;
    // a slab is 128 8-byte words per sounding and component: threads 0 .. 127 fetch the even soundings, 128 .. 255 the odd ones
    const int half = tid >> 7, kl = 2 * (tid & 127);
    float2 vr[PMAX / 2], vi[PMAX / 2];
    const int slabs = (int)((kf + FC_SLAB - 1) / FC_SLAB);
#define FC_FETCH(it)                                                                    \
    {                                                                                   \
        const long long k = (long long)(it) * FC_SLAB + kl;                             \
        const bool in = k < kf;                                                         \
        _Pragma("unroll") for (int x = 0; x < PMAX / 2; ++x) {                          \
            const int p = 2 * x + half;                                                 \
            vr[x] = make_float2(0.0f, 0.0f);                                            \
            vi[x] = make_float2(0.0f, 0.0f);                                            \
            if (p < P && in) {                                                          \
                vr[x] = *reinterpret_cast<const float2*>(a.x_re[p] + base + k);         \
                vi[x] = *reinterpret_cast<const float2*>(a.x_im[p] + base + k);         \
            }                                                                           \
        }                                                                               \
    }
    FC_FETCH(0)
    for (int it = 0; it < slabs; ++it) {
        __syncthreads();                                                 // the waves are through with the slab (first trip: the zeros are in)
#pragma unroll
        for (int x = 0; x < PMAX / 2; ++x)
            if (2 * x + half < P) {
                *reinterpret_cast<float2*>(s_re + (2 * x + half) * FC_STRIDE + kl) = vr[x];
                *reinterpret_cast<float2*>(s_im + (2 * x + half) * FC_STRIDE + kl) = vi[x];
            }
        __syncthreads();
        if (it + 1 < slabs) FC_FETCH(it + 1)                             // in flight behind the MFMAs of this slab
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = row * FC_STRIDE + 64 * wave + 16 * j + 4 * kq;
            const fc_f32x4 xr = *reinterpret_cast<const fc_f32x4*>(s_re + o);
            const fc_f32x4 xi = *reinterpret_cast<const fc_f32x4*>(s_im + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                rr = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[e], xr[e], rr, 0, 0, 0);
                ii = __builtin_amdgcn_mfma_f32_16x16x4f32(xi[e], xi[e], ii, 0, 0, 0);
                ri = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[e], xi[e], ri, 0, 0, 0);      // [i][q] = sum xr_i xi_q
            }
        }
    }
#undef FC_FETCH
    // accumulator register v of this lane: row 4 (l >> 4) + v, column l & 15.  [wave][RR + II | RI][16][16] over the slab area
    __syncthreads();
    for (int v = 0; v < 4; ++v) {
        const int e = (4 * kq + v) * 16 + row;
        fc_s[(wave * 2 + 0) * 256 + e] = rr[v] + ii[v];
        fc_s[(wave * 2 + 1) * 256 + e] = ri[v];
    }
    __syncthreads();
    const int i = tid >> 4, q = tid & 15;
    if (i >= P || q > i) return;
    float re = fc_s[i * 16 + q], m_iq = fc_s[256 + i * 16 + q], m_qi = fc_s[256 + q * 16 + i];
    for (int w = 1; w < FC_THREADS / 64; ++w) {                          // wave 0 + wave 1 + wave 2 + wave 3, in that order
        re += fc_s[(w * 2 + 0) * 256 + i * 16 + q];
        m_iq += fc_s[(w * 2 + 1) * 256 + i * 16 + q];
        m_qi += fc_s[(w * 2 + 1) * 256 + q * 16 + i];
    }
    const float im = i == q ? 0.0f : m_iq - m_qi;
    float* o_re = a.t_re + (size_t)blockIdx.x * P * P;
    float* o_im = a.t_im + (size_t)blockIdx.x * P * P;
    o_re[i * P + q] = re;
    o_im[i * P + q] = im;
    if (i != q) {
        o_re[q * P + i] = re;
        o_im[q * P + i] = -im;
    }
}

// MMAX only makes the kernel a template (emitted behind the plain kernels); the order is a.order
template <int MMAX>
HY_KERNEL __launch_bounds__(FC_FIT_THREADS) void forecast_fit_kernel(const ForecastFitArgs a) {
    const long long idx = (long long)blockIdx.x * FC_FIT_THREADS + threadIdx.x;
    if (idx >= a.items) return;
    const int P = a.n_snd, M = a.order, d = a.steps;
    const int nsum = a.pooled ? a.nr : 1;
    const long long b0 = a.pooled ? idx * a.nr : idx;
    double gr[MMAX][MMAX], gi[MMAX][MMAX], br[MMAX], bi[MMAX], zr[MMAX], zi[MMAX];      // G's lower triangle, then L
    double energy = 0.0;
    for (int x = 0; x < M; ++x) {
        br[x] = 0.0; bi[x] = 0.0;
        for (int y = 0; y <= x; ++y) { gr[x][y] = 0.0; gi[x][y] = 0.0; }
    }
    for (int r = 0; r < nsum; ++r) {
        const float* tr = a.t_re + (size_t)(b0 + r) * P * P;
        const float* ti = a.t_im + (size_t)(b0 + r) * P * P;
        double en = 0.0;
        for (int p = M + d - 1; p < P; ++p) en += (double)tr[p * P + p];
        energy += en;
        for (int x = 0; x < M; ++x) {
            double sr = 0.0, si = 0.0;
            for (int p = M + d - 1; p < P; ++p) { sr += (double)tr[(p - d - x) * P + p]; si += (double)ti[(p - d - x) * P + p]; }
            br[x] += sr; bi[x] += si;
            for (int y = 0; y <= x; ++y) {
                double ur = 0.0, ui = 0.0;
                for (int p = M + d - 1; p < P; ++p) { ur += (double)tr[(p - d - x) * P + (p - d - y)]; ui += (double)ti[(p - d - x) * P + (p - d - y)]; }
                gr[x][y] += ur; gi[x][y] += ui;
            }
        }
    }
    double trace = 0.0;
    for (int x = 0; x < M; ++x) trace += gr[x][x];
    const double lam = a.ridge * trace / (double)M;
    bool bad = false;
    for (int j = 0; j < M && !bad; ++j) {
        double dj = gr[j][j] + lam;
        for (int k = 0; k < j; ++k) dj -= gr[j][k] * gr[j][k] + gi[j][k] * gi[j][k];
        if (!(dj > 0.0) || !isfinite(dj)) { bad = true; break; }
        const double l = sqrt(dj);
        gr[j][j] = l;
        for (int x = j + 1; x < M; ++x) {
            double sr = gr[x][j], si = gi[x][j];
            for (int k = 0; k < j; ++k) {                                // - L[x][k] conj(L[j][k])
                sr -= gr[x][k] * gr[j][k] + gi[x][k] * gi[j][k];
                si -= gi[x][k] * gr[j][k] - gr[x][k] * gi[j][k];
            }
            gr[x][j] = sr / l; gi[x][j] = si / l;
        }
    }
    if (!bad) {
        for (int j = 0; j < M; ++j) {                                    // L z = rhs
            double sr = br[j], si = bi[j];
            for (int k = 0; k < j; ++k) {
                sr -= gr[j][k] * zr[k] - gi[j][k] * zi[k];
                si -= gr[j][k] * zi[k] + gi[j][k] * zr[k];
            }
            zr[j] = sr / gr[j][j]; zi[j] = si / gr[j][j];
        }
        for (int j = M - 1; j >= 0; --j) {                               // L^H c = z, c over z
            double sr = zr[j], si = zi[j];
            for (int k = j + 1; k < M; ++k) {                            // - conj(L[k][j]) c[k]
                sr -= gr[k][j] * zr[k] + gi[k][j] * zi[k];
                si -= gr[k][j] * zi[k] - gi[k][j] * zr[k];
            }
            zr[j] = sr / gr[j][j]; zi[j] = si / gr[j][j];
        }
    } else {
        for (int j = 0; j < M; ++j) { zr[j] = j == 0 ? 1.0 : 0.0; zi[j] = 0.0; }
    }
    double num = 0.0;
    for (int j = 0; j < M; ++j) num += zr[j] * br[j] + zi[j] * bi[j];      // Re(c^H rhs)
    double fe = 0.0;
    if (energy > 0.0) {
        fe = 1.0 - num / energy;
        if (!(fe > 0.0)) fe = 0.0;
    }
    for (int r = 0; r < nsum; ++r) {
        for (int j = 0; j < M; ++j) {
            a.c_re[(size_t)(b0 + r) * M + j] = (float)zr[j];
            a.c_im[(size_t)(b0 + r) * M + j] = (float)zi[j];
        }
        if (a.fit_err) a.fit_err[b0 + r] = (float)fe;
        if (a.info) a.info[b0 + r] = bad ? 1 : 0;
    }
}

template <int MMAX>
HY_KERNEL __launch_bounds__(FC_THREADS) void forecast_apply_kernel(const ForecastApplyArgs a) {
    const int M = a.order;
    const size_t base = (size_t)blockIdx.x * (size_t)a.kf;
    float cr[MMAX], ci[MMAX];
#pragma unroll
    for (int m = 0; m < MMAX; ++m) {
        cr[m] = m < M ? a.c_re[(size_t)blockIdx.x * M + m] : 0.0f;
        ci[m] = m < M ? a.c_im[(size_t)blockIdx.x * M + m] : 0.0f;
    }
    for (long long k = 2 * (long long)threadIdx.x; k < a.kf; k += 2 * FC_THREADS) {
        float yr0 = 0.0f, yr1 = 0.0f, yi0 = 0.0f, yi1 = 0.0f;
#pragma unroll
        for (int m = 0; m < MMAX; ++m)
            if (m < M) {
                const float2 xr = *reinterpret_cast<const float2*>(a.x_re[m] + base + k);
                const float2 xi = *reinterpret_cast<const float2*>(a.x_im[m] + base + k);
                yr0 = fmaf(cr[m], xr.x, yr0); yr0 = fmaf(-ci[m], xi.x, yr0);
                yi0 = fmaf(cr[m], xi.x, yi0); yi0 = fmaf(ci[m], xr.x, yi0);
                yr1 = fmaf(cr[m], xr.y, yr1); yr1 = fmaf(-ci[m], xi.y, yr1);
                yi1 = fmaf(cr[m], xi.y, yi1); yi1 = fmaf(ci[m], xr.y, yi1);
            }
        *reinterpret_cast<float2*>(a.y_re + base + k) = make_float2(yr0, yr1);
        *reinterpret_cast<float2*>(a.y_im + base + k) = make_float2(yi0, yi1);
    }
}

// UNUSED only makes the kernel a template
template <int UNUSED>
HY_KERNEL __launch_bounds__(FC_THREADS) void sounding_noise_kernel(const SoundingNoiseArgs a) {
    const long long blk = blockIdx.x;
    const long long p = blk / a.nr;
    const int r = (int)(blk - p * a.nr);
    const size_t base = (size_t)blk * (size_t)a.kf;
    const float s = sqrtf(0.5f * a.v[blk]);
    const uint64_t kn = ss_key(a.seed, (uint64_t)(a.first_pkt + p), 1);
    for (long long k = 2 * (long long)threadIdx.x; k < a.kf; k += 2 * FC_THREADS) {
        float2 xr = *reinterpret_cast<const float2*>(a.x_re + base + k);
        float2 xi = *reinterpret_cast<const float2*>(a.x_im + base + k);
        if (s != 0.0f) {
            const uint64_t e = (uint64_t)r * (uint64_t)a.kf + (uint64_t)k;
            xr.x = fmaf(s, tr_normal(kn, 2 * e), xr.x);
            xi.x = fmaf(s, tr_normal(kn, 2 * e + 1), xi.x);
            xr.y = fmaf(s, tr_normal(kn, 2 * e + 2), xr.y);
            xi.y = fmaf(s, tr_normal(kn, 2 * e + 3), xi.y);
        }
        *reinterpret_cast<float2*>(a.y_re + base + k) = xr;
        *reinterpret_cast<float2*>(a.y_im + base + k) = xi;
    }
}
#endif

}  // namespace csi
