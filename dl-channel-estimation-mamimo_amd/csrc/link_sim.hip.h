// link_sim.hip.h - link-level simulation of a beamformed data phase: coded QAM through the TRUE channel of a
// synthetic packet, precoded with the hybrid weights of an estimate, then zero forcing, max-log soft bits and a Viterbi decoder.
//
// Reference stage: BER_test_maMIMO_LTF.m:408-646 (bits -> convenc -> qammod -> precoder -> channel -> equaliser -> qamdemod ->
// vitdec -> biterr, EVM :574-578, beamforming gain :585).  The toolbox helpers are not part of the reference tree; the model
// is restated from its definition.  One item = (packet p, subcarrier k of 234, OFDM data symbol n of n_sym):
//   bits      n_info = n_steps - 6 information bits, n_steps = ns n_sym 234 bps / 3;  bit i = splitmix64(key(p, 3) ^ splitmix64(i)) >> 63,
//             key = ss_key of synth_structured.hip.h, p = ABSOLUTE packet index; six zero tail bits follow
//   encoder   rate 1/3, K = 7, generators 133, 171, 165 (octal), terminated.  state = the last 6 inputs, newest in bit 5;
//             reg = (b << 6) | state;  output i = parity(reg & g_i);  next state = reg >> 1
//   mapping   coded bit c = ((s n_sym + n) 234 + k) bps + b  (qammod followed by the reshape of :425-431);  square Gray QAM of
//             unit average power, bps = 2 or 4; the first bps / 2 bits select the in-phase level, the rest the quadrature level.
//             Gray PAM of this file (the project's own labelling - MATLAB's table is not reproduced; BER and EVM do not depend on it):
//               1 bit:  0 -> +a, 1 -> -a                  a = 1 / sqrt(2)
//               2 bits: 00 -> +3a, 01 -> +a, 11 -> -a, 10 -> -3a      a = 1 / sqrt(10)
//   precoder  F_k = frf_mean^T (Nt x ntrf) fbb_k^T (ntrf x ns),  W_k = sqrt(Nt) F_k / |F_k|_F  (0 when |F_k|_F = 0): a data symbol
//             carries the total power of a sounding symbol.  frf_mean [p][ntrf][Nt] and fbb [p][234][ns][ntrf] are the planes
//             csi_hybrid_weights_device writes (:376 uses the subcarrier mean of Frf)
//   channel   y = G_k d + w,  G_k = H_k W_k (Nr x ns),  H = the true planes of csi_synth_structured [p][Nr][Nt][234];
//             w_r = sqrt(noise_var[p] / 2) (tr_normal(key(p, 2), i) + j tr_normal(key(p, 2), i + 1)),  i = ((n 234 + k) Nr + r) 2
//   equaliser x = (G^H G)^-1 G^H y,  csi_s = 1 / [(G^H G)^-1]_ss;  singular G^H G (a Cholesky pivot <= 0 or not finite): x = 0, csi = 0
//   soft bits llr_c = csi_s / noise_var (min_{b=1} |x - q|^2 - min_{b=0} |x - q|^2), positive = 0.  (noise_var = 0: the factor is csi_s.)
//   decoder   Viterbi over the terminated trellis, start and end state 0, fp32 path metrics, no renormalisation.
//             branch metric = ((1-2c_0) llr_0 + (1-2c_1) llr_1) + (1-2c_2) llr_2, new metric = old + branch, in that order;
//             the larger sum survives, on equal sums the predecessor with the lower state number
//   outputs   bit_errors against the information bits; evm_rms = 100 sqrt(mean |x - nearest point|^2) over the packet's
//             ns n_sym 234 symbols; dt_snr_db = 10 log10(sum_k |H_k W_k|_F^2 / sum_k |H_k|_F^2)
//
// Plan:
//   * link_encode_kernel: one thread per trellis step writes the step's three coded bits as bytes (workspace, [p][n_coded]).
//   * link_txrx_kernel: one workgroup of 256 lanes per packet, lane = subcarrier, so every h / fbb / llr / x access runs along
//     the contiguous axis.  Per lane once: F column by column (fbb of the packet staged in LDS, frf_mean wave-uniform), G
//     accumulated in LDS [element][lane], the ns x ns Cholesky factor inverted in registers (NS is a template parameter).  Then
//     the n_sym symbols.  EVM and gain sums: per lane in (n, s) order, then one fixed tree over the 256 lanes - no atomics,
//     a call repeats bit for bit and a packet's result does not depend on the call that holds it.
//   * link_viterbi_kernel: one wavefront per codeword, lane = state j.  The predecessors of j are states 2 (j & 31) and
//     2 (j & 31) + 1 - two ds_bpermute reads per step; all three generators end in 1, so the second branch metric is the
//     negative of the first.  LLRs are fetched 64 steps at a time (lane j holds the three of step t0 + j) and handed out as
//     wave-uniform values (v_readlane).  The 64 decisions of a step are one __ballot word in LDS (8 n_steps bytes); lane 0 traces back from
//     state 0, then all lanes write the bits and count the errors against the regenerated information bits.
// re and im stay in separate registers and planes (no complex types), and the complex arithmetic (link_txrx_kernel) is compiled without packed fp32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "rng.hip.h"
#include "synth_structured.hip.h"      // ss_key

namespace csi {

constexpr int LK_N = 234;                  // data subcarriers
constexpr int LK_THREADS = 256;            // link_txrx_kernel: lanes of a packet (LK_N of them active)
constexpr int LK_MAX_NS = 4;
constexpr int LK_MAX_STEPS = 8190;         // 8 bytes of decisions per step: 65520 bytes of LDS
constexpr int LK_TAIL = 6;
constexpr int LK_KIND_NOISE = 2, LK_KIND_BITS = 3;
constexpr size_t LK_MAX_LDS = 160 * 1024;

#if defined(__HIP_DEVICE_COMPILE__)
#define LK_NO_PK __attribute__((target("no-packed-fp32-ops")))
#else
#define LK_NO_PK
#endif
#define LK_KERNEL __global__ LK_NO_PK
#define LK_DEV __device__ __forceinline__ LK_NO_PK

struct LinkArgs {
    const float* h_re;        // true channel [pkts][nr][nt][234]
    const float* h_im;
    const float* fbb_re;      // [pkts][234][ns][ntrf]
    const float* fbb_im;
    const float* frf_re;      // [pkts][ntrf][nt]
    const float* frf_im;
    const float* noise_var;   // [pkts]
    const uint8_t* coded;     // [pkts][n_coded] coded bits of the chunk (link_encode_kernel)
    float* llr;               // [pkts][n_coded]
    float* xeq_re;            // [pkts][ns][n_sym][234] or null
    float* xeq_im;
    float* csi;               // [pkts][ns][234] or null
    float* evm_rms;           // [pkts]
    float* dt_snr_db;         // [pkts]
    uint64_t seed;
    int64_t first_pkt;        // absolute index of the chunk's first packet
    int nt, nr, ns, ntrf, n_sym, bps;
    int fstride;              // LDS pitch of one subcarrier's fbb block: ns ntrf rounded up to an odd number
};

__host__ __device__ inline size_t link_txrx_lds_bytes(int nr, int ns, int ntrf) {
    const int fstride = (ns * ntrf) | 1;
    return sizeof(float) * ((size_t)2 * nr * ns * LK_THREADS + (size_t)2 * LK_N * fstride + 3 * LK_THREADS);
}

__device__ __forceinline__ int lk_info_bit(uint64_t kbits, uint64_t i) { return (int)(splitmix64(kbits ^ splitmix64(i)) >> 63); }

// ------------------------------------------------------------------------------------------------ encoder
__global__ void link_encode_kernel(uint8_t* coded, uint64_t seed, int64_t first_pkt, int64_t npkt, int n_steps) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= npkt * n_steps) return;
    const int64_t p = gid / n_steps;
    const int t = (int)(gid - p * n_steps);
    const uint64_t kb = ss_key(seed, (uint64_t)(first_pkt + p), LK_KIND_BITS);
    const int n_info = n_steps - LK_TAIL;
    unsigned reg = 0;                       // bit 6 = the input of step t, bit 6 - d = the input of step t - d
#pragma unroll
    for (int d = 0; d <= LK_TAIL; ++d) {
        const int i = t - d;
        const int b = (i >= 0 && i < n_info) ? lk_info_bit(kb, (uint64_t)i) : 0;
        reg |= (unsigned)b << (6 - d);
    }
    uint8_t* o = coded + ((size_t)p * n_steps + t) * 3;
    o[0] = (uint8_t)(__popc(reg & 0133u) & 1);
    o[1] = (uint8_t)(__popc(reg & 0171u) & 1);
    o[2] = (uint8_t)(__popc(reg & 0165u) & 1);
}

// ------------------------------------------------------------------------------------------------ Gray PAM of one axis
// level of the M bits b[0 .. M-1] in units of a: M = 1: +1, -1;  M = 2: +3, +1 (b0 = 0), -3, -1 (b0 = 1)
template <int M>
LK_DEV float lk_pam_level(const int* b) {
    if (M == 1) return b[0] ? -1.f : 1.f;
    const float mag = b[1] ? 1.f : 3.f;
    return b[0] ? -mag : mag;
}

// max-log differences min_{b=1} - min_{b=0} of (x - level)^2 for every bit of the axis, and the squared distance to the nearest level
template <int M>
LK_DEV float lk_pam_soft(float x, float a, float* diff) {
    float m0[M], m1[M], best = INFINITY;
#pragma unroll
    for (int i = 0; i < M; ++i) m0[i] = m1[i] = INFINITY;
#pragma unroll
    for (int v = 0; v < (1 << M); ++v) {
        int b[M];
#pragma unroll
        for (int i = 0; i < M; ++i) b[i] = (v >> (M - 1 - i)) & 1;
        const float e = x - a * lk_pam_level<M>(b);
        const float d2 = e * e;
        best = fminf(best, d2);
#pragma unroll
        for (int i = 0; i < M; ++i) {
            if (b[i]) m1[i] = fminf(m1[i], d2);
            else m0[i] = fminf(m0[i], d2);
        }
    }
#pragma unroll
    for (int i = 0; i < M; ++i) diff[i] = m1[i] - m0[i];
    return best;
}

// ------------------------------------------------------------------------------------------------ transmit, channel, equalise, demap
template <int NS, int M>
LK_KERNEL __launch_bounds__(LK_THREADS) void link_txrx_kernel(const LinkArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lk_smem[];
    const int nt = a.nt, nr = a.nr, ntrf = a.ntrf, n_sym = a.n_sym, fs = a.fstride;
    constexpr int BPS = 2 * M;
    float* G = lk_smem;                                       // [2 (r NS + s) + z][LK_THREADS]
    float* fb_re = G + (size_t)2 * nr * NS * LK_THREADS;      // [234][fs]
    float* fb_im = fb_re + (size_t)LK_N * fs;
    float* red = fb_im + (size_t)LK_N * fs;                   // [3][LK_THREADS]
    const int k = threadIdx.x;
    const bool live = k < LK_N;
    const int kk = live ? k : LK_N - 1;                       // idle lanes repeat the last subcarrier and add nothing
    const size_t p = blockIdx.x;
    const float a_unit = M == 1 ? 0.70710678118654752f : 0.31622776601683794f;

    {   // fbb of the packet -> LDS, pitch fs per subcarrier
        const int per = NS * ntrf;
        const float* gre = a.fbb_re + p * (size_t)LK_N * per;
        const float* gim = a.fbb_im + p * (size_t)LK_N * per;
        for (int i = k; i < LK_N * per; i += LK_THREADS) {
            const int q = i / per, e = i - q * per;
            fb_re[q * fs + e] = gre[i];
            fb_im[q * fs + e] = gim[i];
        }
        for (int i = 0; i < 2 * nr * NS; ++i) G[(size_t)i * LK_THREADS + k] = 0.f;
    }
    __syncthreads();
#define LK_G(r, s, z) G[(size_t)(2 * ((r) * NS + (s)) + (z)) * LK_THREADS + k]

    // ---- G = H F (unscaled), |F|_F^2, |H|_F^2
    const float* hre = a.h_re + p * (size_t)nr * nt * LK_N + kk;
    const float* him = a.h_im + p * (size_t)nr * nt * LK_N + kk;
    const float* qre = a.frf_re + p * (size_t)ntrf * nt;
    const float* qim = a.frf_im + p * (size_t)ntrf * nt;
    const float* mre = fb_re + kk * fs;
    const float* mim = fb_im + kk * fs;
    float f2 = 0.f, h2 = 0.f;
    for (int j = 0; j < nt; ++j) {
        float fr[NS], fi[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) fr[s] = fi[s] = 0.f;
        for (int m = 0; m < ntrf; ++m) {
            const float ur = qre[(size_t)m * nt + j], ui = qim[(size_t)m * nt + j];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float br = mre[s * ntrf + m], bi = mim[s * ntrf + m];
                fr[s] = fmaf(ur, br, fmaf(-ui, bi, fr[s]));
                fi[s] = fmaf(ur, bi, fmaf(ui, br, fi[s]));
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) f2 = fmaf(fr[s], fr[s], fmaf(fi[s], fi[s], f2));
        for (int r = 0; r < nr; ++r) {
            const float xr = hre[((size_t)r * nt + j) * LK_N], xi = him[((size_t)r * nt + j) * LK_N];
            h2 = fmaf(xr, xr, fmaf(xi, xi, h2));
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                LK_G(r, s, 0) = fmaf(xr, fr[s], fmaf(-xi, fi[s], LK_G(r, s, 0)));
                LK_G(r, s, 1) = fmaf(xr, fi[s], fmaf(xi, fr[s], LK_G(r, s, 1)));
            }
        }
    }
    // ---- W = sqrt(Nt) F / |F|_F:  G scaled, A = G^H G (lower triangle), |G|_F^2
    const float wscale = f2 > 0.f ? sqrtf((float)nt / f2) : 0.f;
    float Ar[NS][NS], Ai[NS][NS];
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int c = 0; c < NS; ++c) Ar[i][c] = Ai[i][c] = 0.f;
    float g2 = 0.f;
    for (int r = 0; r < nr; ++r) {
        float gr[NS], gi[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            gr[s] = LK_G(r, s, 0) * wscale;
            gi[s] = LK_G(r, s, 1) * wscale;
            LK_G(r, s, 0) = gr[s];
            LK_G(r, s, 1) = gi[s];
            g2 = fmaf(gr[s], gr[s], fmaf(gi[s], gi[s], g2));
        }
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int c = 0; c <= i; ++c) {                     // A[i][c] += conj(g_i) g_c
                Ar[i][c] = fmaf(gr[i], gr[c], fmaf(gi[i], gi[c], Ar[i][c]));
                Ai[i][c] = fmaf(gr[i], gi[c], fmaf(-gi[i], gr[c], Ai[i][c]));
            }
    }
    // ---- Cholesky A = L L^H in place, then Li = L^-1 (lower); [A^-1]_ss = sum_{i >= s} |Li[i][s]|^2
    bool ok = true;
    float dinv[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        float d = Ar[c][c];
#pragma unroll
        for (int q = 0; q < c; ++q) d -= Ar[c][q] * Ar[c][q] + Ai[c][q] * Ai[c][q];
        if (!(d > 0.f) || !(d <= 3.0e38f)) ok = false;
        const float l = sqrtf(ok ? d : 1.f);
        dinv[c] = 1.f / l;
        Ar[c][c] = l;
        Ai[c][c] = 0.f;
#pragma unroll
        for (int i = c + 1; i < NS; ++i) {
            float sr = Ar[i][c], si = Ai[i][c];
#pragma unroll
            for (int q = 0; q < c; ++q) {                      // - L[i][q] conj(L[c][q])
                sr -= Ar[i][q] * Ar[c][q] + Ai[i][q] * Ai[c][q];
                si -= Ai[i][q] * Ar[c][q] - Ar[i][q] * Ai[c][q];
            }
            Ar[i][c] = sr * dinv[c];
            Ai[i][c] = si * dinv[c];
        }
    }
    float Lr[NS][NS], Lm[NS][NS];                              // Li, lower triangle
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        Lr[c][c] = dinv[c];
        Lm[c][c] = 0.f;
#pragma unroll
        for (int i = c + 1; i < NS; ++i) {                     // Li[i][c] = - (sum_{q = c}^{i - 1} L[i][q] Li[q][c]) / L[i][i]
            float sr = 0.f, si = 0.f;
#pragma unroll
            for (int q = c; q < i; ++q) {
                sr += Ar[i][q] * Lr[q][c] - Ai[i][q] * Lm[q][c];
                si += Ar[i][q] * Lm[q][c] + Ai[i][q] * Lr[q][c];
            }
            Lr[i][c] = -sr * dinv[i];
            Lm[i][c] = -si * dinv[i];
        }
    }
    float csi[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float v = 0.f;
#pragma unroll
        for (int i = s; i < NS; ++i) v += Lr[i][s] * Lr[i][s] + Lm[i][s] * Lm[i][s];
        csi[s] = ok ? 1.f / v : 0.f;
        if (!(csi[s] <= 3.0e38f)) { csi[s] = 0.f; ok = false; }
    }
    if (!ok) {
#pragma unroll
        for (int s = 0; s < NS; ++s) csi[s] = 0.f;
    }
    if (a.csi && live) {
#pragma unroll
        for (int s = 0; s < NS; ++s) a.csi[(p * NS + s) * LK_N + k] = csi[s];
    }

    // ---- the data symbols
    const float nv = a.noise_var[p];
    const float nstd = sqrtf(0.5f * nv);
    float lscale[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) lscale[s] = nv > 0.f ? csi[s] / nv : csi[s];
    const uint64_t kn = ss_key(a.seed, (uint64_t)(a.first_pkt + (int64_t)p), LK_KIND_NOISE);
    const size_t n_coded = (size_t)NS * n_sym * LK_N * BPS;
    const uint8_t* cb = a.coded + p * n_coded;
    float* lo = a.llr + p * n_coded;
    float evm = 0.f;
    for (int n = 0; n < n_sym; ++n) {
        float dr[NS], di[NS], zr[NS], zi[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const uint8_t* c = cb + ((size_t)(s * n_sym + n) * LK_N + kk) * BPS;
            int b[BPS];
#pragma unroll
            for (int i = 0; i < BPS; ++i) b[i] = c[i];
            dr[s] = a_unit * lk_pam_level<M>(b);
            di[s] = a_unit * lk_pam_level<M>(b + M);
            zr[s] = zi[s] = 0.f;
        }
        const uint64_t base = ((uint64_t)(n * LK_N + kk) * nr) * 2;
        for (int r = 0; r < nr; ++r) {
            float yr = nstd * tr_normal(kn, base + 2 * r), yi = nstd * tr_normal(kn, base + 2 * r + 1);
            float gr[NS], gi[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                gr[s] = LK_G(r, s, 0);
                gi[s] = LK_G(r, s, 1);
                yr = fmaf(gr[s], dr[s], fmaf(-gi[s], di[s], yr));
                yi = fmaf(gr[s], di[s], fmaf(gi[s], dr[s], yi));
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {                     // z += conj(g) y
                zr[s] = fmaf(gr[s], yr, fmaf(gi[s], yi, zr[s]));
                zi[s] = fmaf(gr[s], yi, fmaf(-gi[s], yr, zi[s]));
            }
        }
        // x = Li^H (Li z)
        float vr[NS], vi[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            float sr = 0.f, si = 0.f;
#pragma unroll
            for (int c = 0; c <= i; ++c) {
                sr += Lr[i][c] * zr[c] - Lm[i][c] * zi[c];
                si += Lr[i][c] * zi[c] + Lm[i][c] * zr[c];
            }
            vr[i] = sr;
            vi[i] = si;
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float xr = 0.f, xi = 0.f;
#pragma unroll
            for (int i = s; i < NS; ++i) {                     // conj(Li[i][s]) v_i
                xr += Lr[i][s] * vr[i] + Lm[i][s] * vi[i];
                xi += Lr[i][s] * vi[i] - Lm[i][s] * vr[i];
            }
            if (!ok) xr = xi = 0.f;
            float dI[M], dQ[M];
            const float eI = lk_pam_soft<M>(xr, a_unit, dI), eQ = lk_pam_soft<M>(xi, a_unit, dQ);
            if (live) {
                evm += eI + eQ;
                float* l = lo + ((size_t)(s * n_sym + n) * LK_N + k) * BPS;
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    l[i] = lscale[s] * dI[i];
                    l[M + i] = lscale[s] * dQ[i];
                }
                if (a.xeq_re) {
                    const size_t o = ((p * NS + s) * n_sym + n) * LK_N + k;
                    a.xeq_re[o] = xr;
                    a.xeq_im[o] = xi;
                }
            }
        }
    }
#undef LK_G
    // ---- the packet's sums: a fixed tree over the lanes
    red[k] = live ? evm : 0.f;
    red[LK_THREADS + k] = live ? g2 : 0.f;
    red[2 * LK_THREADS + k] = live ? h2 : 0.f;
    __syncthreads();
    for (int w = LK_THREADS / 2; w > 0; w >>= 1) {
        if (k < w) {
            red[k] += red[k + w];
            red[LK_THREADS + k] += red[LK_THREADS + k + w];
            red[2 * LK_THREADS + k] += red[2 * LK_THREADS + k + w];
        }
        __syncthreads();
    }
    if (k == 0) {
        a.evm_rms[p] = 100.f * sqrtf(red[0] / ((float)NS * (float)n_sym * (float)LK_N));
        a.dt_snr_db[p] = 10.f * log10f(red[LK_THREADS] / red[2 * LK_THREADS]);
    }
}

// ------------------------------------------------------------------------------------------------ Viterbi decoder
struct ViterbiArgs {
    const float* llr;         // [ncw][3 n_steps]
    uint8_t* bits;            // [ncw][n_steps - 6] or null
    int32_t* bit_errors;      // [ncw] or null: errors against the regenerated information bits of packet first_pkt + cw
    uint64_t seed;
    int64_t first_pkt;
    int n_steps;
};

// No complex arithmetic here, and the cross-lane helpers (__shfl, __ballot) are inlined only into functions of the default target: this
// kernel and the encoder are compiled without the attribute; the library census of packed fp32 (tests) covers them like any kernel.
__global__ __launch_bounds__(64) void link_viterbi_kernel(const ViterbiArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lk_dec[];      // [n_steps]
    const int j = threadIdx.x;                                                       // state
    const size_t cw = blockIdx.x;
    const int n_steps = a.n_steps, n_info = n_steps - LK_TAIL;
    const float* llr = a.llr + cw * (size_t)3 * n_steps;
    // branch into state j from predecessor 2 (j & 31): reg = (b << 6) | pred with b = j >> 5; the other predecessor flips all three outputs
    const unsigned reg = ((unsigned)(j >> 5) << 6) | (unsigned)((j & 31) << 1);
    const float s0 = (__popc(reg & 0133u) & 1) ? -1.f : 1.f;
    const float s1 = (__popc(reg & 0171u) & 1) ? -1.f : 1.f;
    const float s2 = (__popc(reg & 0165u) & 1) ? -1.f : 1.f;
    const int src = (j & 31) << 1;
    float pm = j == 0 ? 0.f : -INFINITY;
    const int total = 3 * n_steps;
    for (int t0 = 0; t0 < n_steps; t0 += 64) {
        // lane j holds the three LLRs of step t0 + j; a step reads them as wave-uniform values
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        if (t0 + j < n_steps) {
            const float* q = llr + (size_t)3 * (t0 + j);
            v0 = q[0]; v1 = q[1]; v2 = q[2];
        }
        const int cnt = min(64, n_steps - t0);
        for (int tt = 0; tt < cnt; ++tt) {
            const float l0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v0), tt));
            const float l1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v1), tt));
            const float l2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v2), tt));
            const float bm = (s0 * l0 + s1 * l1) + s2 * l2;
            const float p0 = __shfl(pm, src, 64), p1 = __shfl(pm, src + 1, 64);
            const float m0 = p0 + bm, m1 = p1 - bm;
            const bool d = m1 > m0;
            pm = d ? m1 : m0;
            const unsigned long long word = __ballot(d);
            if (j == 0) lk_dec[t0 + tt] = word;
        }
    }
    __syncthreads();
    // traceback from state 0: the input of step t is bit 5 of the state behind it; the slot then holds the decoded bit
    if (j == 0) {
        unsigned st = 0;
        for (int t = n_steps - 1; t >= 0; --t) {
            const unsigned long long word = lk_dec[t];
            const unsigned d = (unsigned)(word >> st) & 1u;
            lk_dec[t] = st >> 5;
            st = ((st & 31u) << 1) | d;
        }
    }
    __syncthreads();
    int errs = 0;
    const uint64_t kb = a.bit_errors ? ss_key(a.seed, (uint64_t)(a.first_pkt + (int64_t)cw), LK_KIND_BITS) : 0;
    for (int t = j; t < n_info; t += 64) {
        const int b = (int)lk_dec[t];
        if (a.bits) a.bits[cw * (size_t)n_info + t] = (uint8_t)b;
        if (a.bit_errors) errs += b ^ lk_info_bit(kb, (uint64_t)t);
    }
    if (a.bit_errors) {
        for (int w = 32; w > 0; w >>= 1) errs += __shfl_xor(errs, w, 64);
        if (j == 0) a.bit_errors[cw] = errs;
    }
}

}  // namespace csi
