// mu_link.hip.h - multi-user downlink: per-subcarrier (regularised) zero-forcing precoding across the addressed receive
// antennas of U users, computed from ESTIMATED CSI, and the coded data phase of link_sim.hip.h through the users' TRUE channels, with
// per-user bit errors, EVM and SINR.
//
// Reference stage: BER_test_maMIMO_LTF.m:110-112, 238-246, 360-385, 417-484 (prm.numUsers).  helperJSDMTransmitWeights is a toolbox
// helper outside the reference tree; the textbook counterpart is stated from its definition.
//   shapes    U users (1 .. 8), user u with CSI planes [p][Nr][Nt][234]; ns streams per user (1 .. min(4, Nr)) addressed to the user's
//             receive antennas 0 .. ns-1; M = U ns <= min(16, Nt) streams, stream m = u ns + s
//   precoder  per item (packet p, subcarrier k):  B[m][j] = hest_u[p][s][j][k] (M x Nt),  A = B B^H + reg[p] I (reg >= 0; none = 0: zero
//             forcing; the regularised form uses reg = M noise_var / Nt),  A = L L^H (a pivot <= 0 or not finite: W = 0 for the item,
//             the singular rule of link_sim.hip.h),  V = B^H A^-1 (Nt x M),  W[:, m] = sqrt(Nt / M) V[:, m] / |V[:, m]|_2 (a zero or
//             non-finite norm: 0).  |W|_F^2 = Nt: a data symbol carries the total power of a sounding symbol, equal power per stream.
//             Planes W [p][M][Nt][234].
//   data      user seed: seed_0 = seed, seed_u = splitmix64(seed ^ splitmix64(u)); bits, encoder, mapper and frame sizes of
//             link_sim.hip.h for (ns, n_sym, bps) on the stream seed_u.  t = sum_m W[:, m] d_m;  at user u, antenna i < ns:
//             y_u[i] = sum_m G_u[i][m] d_m + w,  G_u = H_u[0:ns] W (ns x M), H_u the TRUE planes;  w of variance noise_var[u][p] per
//             complex sample, draws of (seed_u, kind 2) at i = ((n 234 + k) ns + r) 2: user 0 with ns = Nr has the bits and the noise of
//             csi_link_sim_device.
//   equaliser the single-user one on the user's own block G_uu (ns x ns): x = (G_uu^H G_uu)^-1 G_uu^H y, csi_s = 1 / [(G_uu^H G_uu)^-1]_ss,
//             the same singular rule.  Soft bits csi_s / noise_var times the max-log difference: the interference of the other users'
//             streams is NOT in the scale - the receiver does not know it.  Viterbi decoding as in link_sim.hip.h.
//   outputs   [U][npkt]: bit_errors, evm_rms, sinr_db = 10 log10(sum_k |G_uu|_F^2 / (sum_k |G_u,others|_F^2 + 234 ns noise_var)), the
//             IEEE quotient; G_u,others = the columns of the other users.  Optional g [U][p][ns][M][234], xeq [U][p][ns][n_sym][234],
//             csi [U][p][ns][234], llr [U][p][n_coded], bits [U][p][n_info].
//
// Plan:
//   * mu_precoder_kernel: one item per lane, lane = subcarrier, 64 subcarriers per workgroup (4 tiles per packet), so the reads of
//     the U h planes and the stores of W run along the contiguous axis.  The lower triangle of A (then L, 1 / L_ii in the unused
//     imaginary slot of the diagonal), one column of B and the M column norms live in LDS as [element][lane]: (M^2 + 4 M) floats per
//     lane, 80 KiB at M = 16.  Every LDS word belongs to one lane: no barrier.  Gram over j = 0 .. Nt-1 in that order; Cholesky column
//     by column; per column j of B one forward and one backward substitution A x = b_j, W[m][j] = conj(x_m) unscaled, norms
//     accumulated over j in that order; a second pass over the lane's own W elements applies the scale.
//   * mu_txrx_kernel<NS, bits per axis>: one workgroup of 256 lanes per (packet, user), lane = subcarrier.  G_u (ns x M) accumulated in
//     LDS [element][lane] over j in order; the ns x ns normal equations of G_uu in registers as in link_txrx_kernel; per symbol the M
//     streams' symbols are regenerated from the coded bytes of the U codewords, y accumulated over m in order.  EVM and the two SINR
//     sums: per lane in fixed order, then one tree over the 256 lanes.
// The encoder and the decoder are link_encode_kernel and link_viterbi_kernel as they are.  All arithmetic is fp32, no atomics: a call
// repeats bit for bit.  re and im stay in separate registers and planes; the complex arithmetic is compiled without packed fp32.
#pragma once
#include "link_sim.hip.h"

namespace csi {

constexpr int MU_MAX_USERS = 8;
constexpr int MU_MAX_STREAMS = 16;
constexpr int MU_PRE_LANES = 64;                                               // subcarriers of one mu_precoder_kernel workgroup
constexpr int MU_PRE_TILES = (LK_N + MU_PRE_LANES - 1) / MU_PRE_LANES;         // 4

struct MuPrecoderArgs {
    const float* h_re[MU_MAX_USERS];   // estimated planes of user u [pkts][nr][nt][234]
    const float* h_im[MU_MAX_USERS];
    const float* reg;                  // [pkts] or null (0)
    float* w_re;                       // [pkts][M][nt][234]
    float* w_im;
    int nt, nr, ns, n_users;
};

__host__ __device__ inline size_t mu_precoder_lds_bytes(int m) { return sizeof(float) * (size_t)MU_PRE_LANES * ((size_t)m * m + 4 * (size_t)m); }

// A template (LANES = MU_PRE_LANES is its one instance) so that the kernel is emitted with the other instantiations, behind the kernels
// of link_sim.hip.h: a plain kernel would be placed in front of them and move the addresses their calls are relative to.
template <int LANES>
LK_KERNEL __launch_bounds__(LANES) void mu_precoder_kernel(const MuPrecoderArgs a) {
    static_assert(LANES == MU_PRE_LANES, "one tile size");
    extern __shared__ __attribute__((aligned(16))) float mu_pre_smem[];
    const int nt = a.nt, ns = a.ns, nu = a.n_users, M = nu * ns;
    const int lane = threadIdx.x;
    const size_t p = blockIdx.x / MU_PRE_TILES;
    const int k = (int)(blockIdx.x % MU_PRE_TILES) * MU_PRE_LANES + lane;
    const bool live = k < LK_N;
    const int kk = live ? k : LK_N - 1;                       // idle lanes repeat the last subcarrier and store nothing
    float* T = mu_pre_smem + lane;                            // lower triangle [2 (i (i + 1) / 2 + c) + z][lanes]
    float* V = T + (size_t)M * (M + 1) * MU_PRE_LANES;        // one column of B, then the solution [2 m + z][lanes]
    float* NR = V + (size_t)2 * M * MU_PRE_LANES;             // |V[:, m]|^2 [m][lanes]
#define MU_T(i, c, z) T[(size_t)(2 * ((i) * ((i) + 1) / 2 + (c)) + (z)) * MU_PRE_LANES]
#define MU_V(m, z) V[(size_t)(2 * (m) + (z)) * MU_PRE_LANES]
    for (int e = 0; e < M * (M + 1); ++e) T[(size_t)e * MU_PRE_LANES] = 0.f;
    for (int m = 0; m < M; ++m) NR[(size_t)m * MU_PRE_LANES] = 0.f;
    const size_t hoff = p * (size_t)a.nr * nt * LK_N + kk;

    // ---- A = B B^H, lower triangle, over j in order
    for (int j = 0; j < nt; ++j) {
        for (int u = 0, m = 0; u < nu; ++u) {
            const float* hr = a.h_re[u] + hoff + (size_t)j * LK_N;
            const float* hi = a.h_im[u] + hoff + (size_t)j * LK_N;
            for (int s = 0; s < ns; ++s, ++m) {
                MU_V(m, 0) = hr[(size_t)s * nt * LK_N];
                MU_V(m, 1) = hi[(size_t)s * nt * LK_N];
            }
        }
        for (int i = 0; i < M; ++i) {
            const float xr = MU_V(i, 0), xi = MU_V(i, 1);
            for (int c = 0; c < i; ++c) {                      // A[i][c] += b_i conj(b_c)
                const float yr = MU_V(c, 0), yi = MU_V(c, 1);
                MU_T(i, c, 0) = fmaf(xr, yr, fmaf(xi, yi, MU_T(i, c, 0)));
                MU_T(i, c, 1) = fmaf(xi, yr, fmaf(-xr, yi, MU_T(i, c, 1)));
            }
            MU_T(i, i, 0) = fmaf(xr, xr, fmaf(xi, xi, MU_T(i, i, 0)));
        }
    }
    const float reg = a.reg ? a.reg[p] : 0.f;
    for (int i = 0; i < M; ++i) MU_T(i, i, 0) += reg;

    // ---- Cholesky A = L L^H in place; the imaginary slot of a diagonal element holds 1 / L_ii
    bool ok = true;
    for (int c = 0; c < M; ++c) {
        float d = MU_T(c, c, 0);
        for (int q = 0; q < c; ++q) d -= MU_T(c, q, 0) * MU_T(c, q, 0) + MU_T(c, q, 1) * MU_T(c, q, 1);
        if (!(d > 0.f) || !(d <= 3.0e38f)) ok = false;
        const float l = sqrtf(ok ? d : 1.f);
        const float dinv = 1.f / l;
        MU_T(c, c, 0) = l;
        MU_T(c, c, 1) = dinv;
        for (int i = c + 1; i < M; ++i) {
            float sr = MU_T(i, c, 0), si = MU_T(i, c, 1);
            for (int q = 0; q < c; ++q) {                      // - L[i][q] conj(L[c][q])
                const float ar = MU_T(i, q, 0), ai = MU_T(i, q, 1), br = MU_T(c, q, 0), bi = MU_T(c, q, 1);
                sr -= ar * br + ai * bi;
                si -= ai * br - ar * bi;
            }
            MU_T(i, c, 0) = sr * dinv;
            MU_T(i, c, 1) = si * dinv;
        }
    }

    // ---- per column j of B: A x = b_j by two substitutions; V[j][m] = conj(x_m), stored unscaled; norms over j in order
    float* wre = a.w_re + p * (size_t)M * nt * LK_N + k;
    float* wim = a.w_im + p * (size_t)M * nt * LK_N + k;
    for (int j = 0; j < nt; ++j) {
        for (int u = 0, m = 0; u < nu; ++u) {
            const float* hr = a.h_re[u] + hoff + (size_t)j * LK_N;
            const float* hi = a.h_im[u] + hoff + (size_t)j * LK_N;
            for (int s = 0; s < ns; ++s, ++m) {
                MU_V(m, 0) = hr[(size_t)s * nt * LK_N];
                MU_V(m, 1) = hi[(size_t)s * nt * LK_N];
            }
        }
        for (int i = 0; i < M; ++i) {                          // L y = b
            float sr = MU_V(i, 0), si = MU_V(i, 1);
            for (int q = 0; q < i; ++q) {
                const float ar = MU_T(i, q, 0), ai = MU_T(i, q, 1), yr = MU_V(q, 0), yi = MU_V(q, 1);
                sr -= ar * yr - ai * yi;
                si -= ar * yi + ai * yr;
            }
            const float dinv = MU_T(i, i, 1);
            MU_V(i, 0) = sr * dinv;
            MU_V(i, 1) = si * dinv;
        }
        for (int i = M - 1; i >= 0; --i) {                     // L^H x = y
            float sr = MU_V(i, 0), si = MU_V(i, 1);
            for (int q = i + 1; q < M; ++q) {                  // - conj(L[q][i]) x_q
                const float ar = MU_T(q, i, 0), ai = MU_T(q, i, 1), yr = MU_V(q, 0), yi = MU_V(q, 1);
                sr -= ar * yr + ai * yi;
                si -= ar * yi - ai * yr;
            }
            const float dinv = MU_T(i, i, 1);
            sr *= dinv;
            si *= dinv;
            MU_V(i, 0) = sr;
            MU_V(i, 1) = si;
            NR[(size_t)i * MU_PRE_LANES] = fmaf(sr, sr, fmaf(si, si, NR[(size_t)i * MU_PRE_LANES]));
            if (live) {
                wre[((size_t)i * nt + j) * LK_N] = sr;
                wim[((size_t)i * nt + j) * LK_N] = -si;
            }
        }
    }
    // ---- W[:, m] = sqrt(Nt / M) V[:, m] / |V[:, m]|: the lane rescales the elements it stored
    if (live) {
        for (int m = 0; m < M; ++m) {
            const float n2 = NR[(size_t)m * MU_PRE_LANES];
            const float sc = (ok && n2 > 0.f && n2 <= 3.0e38f) ? sqrtf((float)nt / ((float)M * n2)) : 0.f;
            for (int j = 0; j < nt; ++j) {
                const size_t o = ((size_t)m * nt + j) * LK_N;
                const float vr = wre[o], vi = wim[o];
                wre[o] = sc > 0.f ? vr * sc : 0.f;
                wim[o] = sc > 0.f ? vi * sc : 0.f;
            }
        }
    }
#undef MU_T
#undef MU_V
}

// ------------------------------------------------------------------------------------------------ transmit, channels, equalise, demap
struct MuLinkArgs {
    const float* h_re[MU_MAX_USERS];   // TRUE planes of user u [pkts][nr][nt][234], at the chunk's first packet
    const float* h_im[MU_MAX_USERS];
    const float* w_re;                 // [pkts][M][nt][234], at the chunk's first packet
    const float* w_im;
    const float* noise_var;            // [U][out_pkts], at the chunk's first packet
    const uint8_t* coded;              // [U][ws_pkts][coded_stride]: the chunk's coded bits (link_encode_kernel per user)
    float* llr;                        // [U][llr_pkts][n_coded], at the chunk's first packet
    float* g_re;                       // [U][out_pkts][ns][M][234] or null
    float* g_im;
    float* xeq_re;                     // [U][out_pkts][ns][n_sym][234] or null
    float* xeq_im;
    float* csi;                        // [U][out_pkts][ns][234] or null
    float* evm_rms;                    // [U][out_pkts]
    float* sinr_db;                    // [U][out_pkts]
    uint64_t seed[MU_MAX_USERS];       // seed_u
    int64_t first_pkt;                 // absolute index of the chunk's first packet
    int64_t out_pkts;                  // packets of the whole call: the user pitch of the caller's arrays
    int64_t ws_pkts;                   // the user pitch of the coded bits
    int64_t llr_pkts;                  // the user pitch of llr (out_pkts in the caller's array, ws_pkts in the workspace)
    size_t coded_stride;               // bytes of one codeword in the workspace
    int nt, nr, n_users, n_sym;
};

__host__ __device__ inline size_t mu_txrx_lds_bytes(int ns, int m) { return sizeof(float) * ((size_t)2 * ns * m * LK_THREADS + 3 * LK_THREADS); }

template <int NS, int M1>
LK_KERNEL __launch_bounds__(LK_THREADS) void mu_txrx_kernel(const MuLinkArgs a) {
    extern __shared__ __attribute__((aligned(16))) float mu_smem[];
    constexpr int BPS = 2 * M1;
    const int nt = a.nt, nu = a.n_users, n_sym = a.n_sym, M = nu * NS;
    const int k = threadIdx.x;
    const bool live = k < LK_N;
    const int kk = live ? k : LK_N - 1;                       // idle lanes repeat the last subcarrier and add nothing
    const size_t p = blockIdx.x;
    const int u = blockIdx.y;
    const size_t up = (size_t)u * (size_t)a.out_pkts + p;     // (user, packet) in the caller's arrays
    float* G = mu_smem + k;                                   // [2 (i M + m) + z][LK_THREADS]
    float* red = mu_smem + (size_t)2 * NS * M * LK_THREADS;   // [3][LK_THREADS]
    const float a_unit = M1 == 1 ? 0.70710678118654752f : 0.31622776601683794f;
#define MU_G(i, m, z) G[(size_t)(2 * ((i) * M + (m)) + (z)) * LK_THREADS]
    for (int e = 0; e < 2 * NS * M; ++e) G[(size_t)e * LK_THREADS] = 0.f;

    // ---- G_u = H_u[0:ns] W over j in order
    {
        const float* hre = a.h_re[u] + p * (size_t)a.nr * nt * LK_N + kk;
        const float* him = a.h_im[u] + p * (size_t)a.nr * nt * LK_N + kk;
        const float* wre = a.w_re + p * (size_t)M * nt * LK_N + kk;
        const float* wim = a.w_im + p * (size_t)M * nt * LK_N + kk;
        for (int j = 0; j < nt; ++j) {
            float xr[NS], xi[NS];
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                xr[i] = hre[((size_t)i * nt + j) * LK_N];
                xi[i] = him[((size_t)i * nt + j) * LK_N];
            }
            for (int m = 0; m < M; ++m) {
                const float wr = wre[((size_t)m * nt + j) * LK_N], wi = wim[((size_t)m * nt + j) * LK_N];
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    MU_G(i, m, 0) = fmaf(xr[i], wr, fmaf(-xi[i], wi, MU_G(i, m, 0)));
                    MU_G(i, m, 1) = fmaf(xr[i], wi, fmaf(xi[i], wr, MU_G(i, m, 1)));
                }
            }
        }
    }
    // ---- the SINR sums in (i, m) order, the optional g planes
    float sig = 0.f, itf = 0.f;
    const int m0 = u * NS;
#pragma unroll
    for (int i = 0; i < NS; ++i)
        for (int m = 0; m < M; ++m) {
            const float gr = MU_G(i, m, 0), gi = MU_G(i, m, 1);
            if (m >= m0 && m < m0 + NS) sig = fmaf(gr, gr, fmaf(gi, gi, sig));
            else itf = fmaf(gr, gr, fmaf(gi, gi, itf));
            if (a.g_re && live) {
                const size_t o = ((up * NS + i) * M + m) * LK_N + k;
                a.g_re[o] = gr;
                a.g_im[o] = gi;
            }
        }
    // ---- A = G_uu^H G_uu (lower triangle)
    float Ar[NS][NS], Ai[NS][NS];
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int c = 0; c < NS; ++c) Ar[i][c] = Ai[i][c] = 0.f;
#pragma unroll
    for (int r = 0; r < NS; ++r) {
        float gr[NS], gi[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            gr[s] = MU_G(r, m0 + s, 0);
            gi[s] = MU_G(r, m0 + s, 1);
        }
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int c = 0; c <= i; ++c) {                     // A[i][c] += conj(g_i) g_c
                Ar[i][c] = fmaf(gr[i], gr[c], fmaf(gi[i], gi[c], Ar[i][c]));
                Ai[i][c] = fmaf(gr[i], gi[c], fmaf(-gi[i], gr[c], Ai[i][c]));
            }
    }
    // ---- Cholesky A = L L^H in place, then Li = L^-1 (lower); [A^-1]_ss = sum_{i >= s} |Li[i][s]|^2  (as link_txrx_kernel)
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
        for (int s = 0; s < NS; ++s) a.csi[(up * NS + s) * LK_N + k] = csi[s];
    }

    // ---- the data symbols
    const float nv = a.noise_var[up];
    const float nstd = sqrtf(0.5f * nv);
    float lscale[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) lscale[s] = nv > 0.f ? csi[s] / nv : csi[s];
    const uint64_t kn = ss_key(a.seed[u], (uint64_t)(a.first_pkt + (int64_t)p), LK_KIND_NOISE);
    const size_t n_coded = (size_t)NS * n_sym * LK_N * BPS;
    float* lo = a.llr + ((size_t)u * (size_t)a.llr_pkts + p) * n_coded;
    float evm = 0.f;
    for (int n = 0; n < n_sym; ++n) {
        float yr[NS], yi[NS];
        const uint64_t base = ((uint64_t)(n * LK_N + kk) * NS) * 2;
#pragma unroll
        for (int r = 0; r < NS; ++r) {
            yr[r] = nstd * tr_normal(kn, base + 2 * r);
            yi[r] = nstd * tr_normal(kn, base + 2 * r + 1);
        }
        for (int v = 0; v < nu; ++v) {                         // the streams of user v, m = v NS + s in order
            const uint8_t* cb = a.coded + ((size_t)v * (size_t)a.ws_pkts + p) * a.coded_stride;
            float dr[NS], di[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const uint8_t* c = cb + ((size_t)(s * n_sym + n) * LK_N + kk) * BPS;
                int b[BPS];
#pragma unroll
                for (int i = 0; i < BPS; ++i) b[i] = c[i];
                dr[s] = a_unit * lk_pam_level<M1>(b);
                di[s] = a_unit * lk_pam_level<M1>(b + M1);
            }
#pragma unroll
            for (int r = 0; r < NS; ++r)
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const float gr = MU_G(r, v * NS + s, 0), gi = MU_G(r, v * NS + s, 1);
                    yr[r] = fmaf(gr, dr[s], fmaf(-gi, di[s], yr[r]));
                    yi[r] = fmaf(gr, di[s], fmaf(gi, dr[s], yi[r]));
                }
        }
        float zr[NS], zi[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) zr[s] = zi[s] = 0.f;
#pragma unroll
        for (int r = 0; r < NS; ++r)
#pragma unroll
            for (int s = 0; s < NS; ++s) {                     // z += conj(g) y on the user's own block
                const float gr = MU_G(r, m0 + s, 0), gi = MU_G(r, m0 + s, 1);
                zr[s] = fmaf(gr, yr[r], fmaf(gi, yi[r], zr[s]));
                zi[s] = fmaf(gr, yi[r], fmaf(-gi, yr[r], zi[s]));
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
            float dI[M1], dQ[M1];
            const float eI = lk_pam_soft<M1>(xr, a_unit, dI), eQ = lk_pam_soft<M1>(xi, a_unit, dQ);
            if (live) {
                evm += eI + eQ;
                float* l = lo + ((size_t)(s * n_sym + n) * LK_N + k) * BPS;
#pragma unroll
                for (int i = 0; i < M1; ++i) {
                    l[i] = lscale[s] * dI[i];
                    l[M1 + i] = lscale[s] * dQ[i];
                }
                if (a.xeq_re) {
                    const size_t o = ((up * NS + s) * n_sym + n) * LK_N + k;
                    a.xeq_re[o] = xr;
                    a.xeq_im[o] = xi;
                }
            }
        }
    }
#undef MU_G
    // ---- the sums of the (packet, user): a fixed tree over the lanes
    red[k] = live ? evm : 0.f;
    red[LK_THREADS + k] = live ? sig : 0.f;
    red[2 * LK_THREADS + k] = live ? itf : 0.f;
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
        a.evm_rms[up] = 100.f * sqrtf(red[0] / ((float)NS * (float)n_sym * (float)LK_N));
        a.sinr_db[up] = 10.f * log10f(red[LK_THREADS] / (red[2 * LK_THREADS] + (float)LK_N * (float)NS * nv));
    }
}

}  // namespace csi
