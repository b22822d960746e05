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
//
// The receiver that estimates its channel (link_txrx_rx_kernel, csi_link_sim_rx_device; generate_maMIMO_LTF_SINR.m:433-435, 528-533): a
// precoded preamble of n_ltf(ns) = 1, 2, 4, 4 symbols passes through the same G, and the equaliser is built on its LS estimate.
//   pilots    P = P4[0:ns][0:n_ltf],  P4 = [[1,-1,1,1],[1,1,-1,1],[1,1,1,-1],[-1,1,1,1]] (802.11): P P^T = n_ltf I
//   preamble  Ypre[m][r] = sum_s G[r][s] P[s][m] + w[m][r], m < n_ltf.  w continues the data noise stream: preamble symbol m takes the
//             draws of symbol index n_sym + m, i = (((n_sym + m) 234 + k) Nr + r) 2 and i + 1, at the same sqrt(noise_var / 2) scale.
//             The data symbols see the draws they see in link_txrx_kernel: the two receivers are a paired comparison.  The LTF sign
//             of the bin is left out: it cancels in the signal term and only flips the sign of a symmetric draw.
//   estimate  Ghat[r][s] = (1 / n_ltf) sum_m Ypre[m][r] P[s][m]  = G + e,  e ~ CN(0, noise_var / n_ltf)
//   equaliser the same Cholesky path with A = Ghat^H Ghat, z = Ghat^H y, csi_s = 1 / [A^-1]_ss; y is still G d + w.  The singular rule
//             is unchanged.  Soft bits, decoder, evm_rms as above; dt_snr_db is still that of the true G.
//   outputs   g_nmse = sum_{k,r,s} |Ghat - G|^2 / sum_{k,r,s} |G|^2 (per lane in (r, s) order, then the tree over the lanes; 0 when both
//             sums are 0, otherwise the IEEE quotient); optional planes gest [p][234][Nr][ns] (as a pair).
// One body serves both kernels (link_txrx_body.inc, included with LK_RX 0 and 1); LK_RX adds a second [2 Nr ns][256] LDS array for Ghat and a
// fourth row of sums.
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

// the receiver with an estimated channel: the arguments above and its own outputs
struct LinkRxArgs {
    LinkArgs a;
    float* g_nmse;            // [pkts]
    float* gest_re;           // [pkts][234][nr][ns] or null
    float* gest_im;
};

__host__ __device__ inline int link_preamble_symbols(int ns) { return ns == 1 ? 1 : ns == 2 ? 2 : (ns == 3 || ns == 4) ? 4 : -1; }

// link_txrx_rx_kernel: Ghat beside G, and one more row of lane sums
__host__ __device__ inline size_t link_txrx_rx_lds_bytes(int nr, int ns, int ntrf) {
    return link_txrx_lds_bytes(nr, ns, ntrf) + sizeof(float) * ((size_t)2 * nr * ns * LK_THREADS + LK_THREADS);
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
// sign of P4[s][m]: the one -1 of row s stands in column (s + 1) mod 4
LK_DEV float lk_p4(int s, int m) { return m == ((s + 1) & 3) ? -1.f : 1.f; }

template <int NS, int M>
LK_KERNEL __launch_bounds__(LK_THREADS) void link_txrx_kernel(const LinkArgs a) {
#define LK_RX 0
#include "link_txrx_body.inc"
#undef LK_RX
}

// the receiver that estimates G from the preamble: the same body with the LK_RX parts
template <int NS, int M>
LK_KERNEL __launch_bounds__(LK_THREADS) void link_txrx_rx_kernel(const LinkRxArgs b) {
    const LinkArgs& a = b.a;
#define LK_RX 1
#include "link_txrx_body.inc"
#undef LK_RX
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
