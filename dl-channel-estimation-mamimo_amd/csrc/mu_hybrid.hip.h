// mu_hybrid.hip.h - multi-user hybrid precoding: one analog matrix per packet, chosen beam by beam from the ray
// dictionary of csi_hybrid_set_dictionary, and a zero-forcing baseband precoder per subcarrier on the effective channel behind it.
//
// Reference call site: generate_maMIMO_LTF_SINR.m:357-369 (helperJSDMTransmitWeights, a toolbox helper outside the reference tree).  The
// algorithm here is stated on its own: beams from the dictionary instead of covariance eigenvectors plus block diagonalisation.
//   shapes    those of mu_link.hip.h: U users with planes [p][Nr][Nt][234], ns streams per user, M = U ns, stream m = u ns + s,
//             B_k[m][j] = hest_u[p][s][j][k];  dictionary At [Nt][R] (columns as given), n_rf RF chains, M <= n_rf <= min(16, Nt, R)
//   score     S[p][m][r] = sum_k | sum_j B_k[m][j] At[j][r] |^2                                          mu_beam_score_kernel (fp32 MFMA)
//   select    q = 0 .. n_rf-1: stream m = q mod M, idx[p][q] = argmax over the rays not yet taken in this packet of S[p][m][r] (lowest r
//             on a tie, a non-finite score compares as -inf);  Frf[:, q] = At[:, idx[p][q]]              mu_beam_select_kernel
//   baseband  per (p, k): G = B_k Frf (M x n_rf), A = G G^H + reg[p] I, Cholesky A = L L^H (a pivot <= 0 or not finite: W = 0 and Fbb = 0
//             for the item), Vbb = G^H A^-1 (n_rf x M), V = Frf Vbb (Nt x M), c_m = sqrt(Nt / M) / |V[:, m]|_2 (zero or non-finite norm: 0),
//             W[:, m] = c_m V[:, m], Fbb[:, m] = c_m Vbb[:, m]: W = Frf Fbb, |W|_F^2 = Nt               mu_hybrid_precoder_kernel
//             Planes W [p][M][Nt][234] (the layout mu_txrx_kernel reads), Fbb [p][234][n_rf][M].
//
// Plan:
//   * mu_beam_score_kernel: one workgroup of 4 waves per (packet, stream).  Psi = B At as one real product with the complex structure
//     embedded, as hyb_corr_kernel does: per 32 rays x 32 subcarriers two accumulators (re, im) fed by four v_mfma_f32_32x32x2_f32 per two
//     antennas.  The dictionary goes through LDS in tiles of 32 rays, four tiles per round, one per wave (1 KiB per antenna); a wave
//     takes its tile through all 8 subcarrier tiles of 32 (subcarriers past 233 enter as zeros), reading the stream's row of the user's
//     planes along the contiguous axis.  Epilogue, once per (wave, ray tile): re^2 + im^2 added per lane over the 8 subcarrier tiles in
//     order, then a xor butterfly over the 32 subcarrier lanes: only S is written.  The order of every sum depends on Nt, R and the
//     subcarrier index alone; no atomics, and no sum crosses a wave.
//   * mu_beam_select_kernel: one wave per packet; lane l scans the rays l, l + 64, ... in ascending order, a xor butterfly with the
//     (larger score, lower index) rule joins the lanes.
//   * mu_hybrid_precoder_kernel<LANES>: one item per lane, lane = subcarrier, LANES subcarriers per workgroup.  The packet's Frf goes
//     once into LDS (shared, rows of 16 chains, zero past n_rf, read as float4 by every lane at once); G (then the solution A^-1 G, in
//     place) and the lower triangle of A (then L, 1 / L_ii in the unused imaginary slot of the diagonal) live in LDS as [element][lane]:
//     (2 M n_rf + M^2 + M) floats per lane.  64 lanes where that fits 160 KiB, 32 lanes at the caps (M = n_rf = 16: 98 KiB + Frf).  The
//     three long loops - G = B Frf, the Gram matrix, V = Frf Vbb - keep one row of n_rf chains in registers (16 statically indexed
//     pairs, loops over groups of four chains with a uniform exit), so their inner products read Frf only.  Every per-lane word belongs
//     to one lane; the one barrier stands behind the Frf load.  V is formed twice - once for the norms, once scaled for the stores - so
//     nothing written is read back.  The arithmetic of a lane does not depend on LANES.
// All arithmetic is fp32 in fixed order: a packet's bits do not depend on the call, the chunk or its position in the batch.  re and im
// stay in separate registers and planes; the kernels are compiled without packed fp32 (HY_NO_PK).  The kernels are
// templates so that they are emitted behind the kernels of the earlier files and leave their code where it was.
#pragma once
#include "hybrid_weights.hip.h"
#include "mu_link.hip.h"

namespace csi {

constexpr int MH_SCORE_WAVES = 4;          // waves of a score workgroup: each owns one ray tile of a round of four
constexpr int MH_SCORE_THREADS = 64 * MH_SCORE_WAVES;
constexpr int MH_SCORE_CT = (HY_N + 31) / 32;   // 8 subcarrier tiles of 32 (22 lanes of the last one idle)
constexpr int MH_SELECT_THREADS = 64;
constexpr size_t MH_MAX_LDS = 160 * 1024;
constexpr int MH_QP = HY_MAX_RF;           // chains of a row of the baseband kernel's Frf image and of its register rows

struct MuHybridArgs {
    const float* h_re[MU_MAX_USERS];   // estimated planes of user u [pkts][nr][nt][234], at the chunk's first packet
    const float* h_im[MU_MAX_USERS];
    const float* at_re;                // dictionary [nt][rp], rp = rays rounded up to 32, zero padded
    const float* at_im;
    const float* reg;                  // [pkts] or null (0)
    float* score;                      // [pkts][M][rays]
    int32_t* idx;                      // [pkts][n_rf]
    float* w_re;                       // [pkts][M][nt][234]
    float* w_im;
    float* fbb_re;                     // [pkts][234][n_rf][M] or null
    float* fbb_im;
    int nt, nr, ns, n_users, n_rf, rays, rp;
};

__host__ __device__ inline size_t mu_score_lds_bytes(int nt) { return sizeof(float) * (size_t)MH_SCORE_WAVES * 2 * nt * HY_RAY_TILE; }

__host__ __device__ inline size_t mu_hybrid_lds_bytes(int nt, int m, int n_rf, int lanes) {
    return sizeof(float) * ((size_t)2 * nt * MH_QP + (size_t)lanes * ((size_t)2 * m * n_rf + (size_t)m * (m + 1)));
}

// ------------------------------------------------------------------------------------------------ wideband beam score
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
template <int THREADS>
HY_KERNEL __launch_bounds__(THREADS) void mu_beam_score_kernel(const MuHybridArgs a) {
    static_assert(THREADS == MH_SCORE_THREADS && THREADS == 64 * MH_SCORE_WAVES, "four waves");
    extern __shared__ __attribute__((aligned(16))) float mh_tile[];          // [4 waves][2][nt][32]: one dictionary tile per wave
    const int nt = a.nt, rp = a.rp, M = a.n_users * a.ns;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, h = lane >> 5;
    const float* t_re = mh_tile + (size_t)wave * 2 * nt * HY_RAY_TILE;
    const float* t_im = t_re + (size_t)nt * HY_RAY_TILE;
    const size_t p = blockIdx.x / M;
    const int m = (int)(blockIdx.x % M);
    const int u = m / a.ns, s = m - u * a.ns;
    const size_t row = (p * (size_t)a.nr + s) * (size_t)nt * HY_N;           // row s of user u in packet p
    const float* hr = a.h_re[u] + row;
    const float* hi = a.h_im[u] + row;
    float* out = a.score + (p * (size_t)M + m) * (size_t)a.rays;
    for (int r0 = 0; r0 < rp; r0 += MH_SCORE_WAVES * HY_RAY_TILE) {
        // the next four ray tiles (columns r0 .. r0 + 127 of the padded image; columns past rp: zeros nobody reads)
        __syncthreads();
        for (int e = threadIdx.x; e < MH_SCORE_WAVES * nt * HY_RAY_TILE; e += THREADS) {
            const int w = e / (nt * HY_RAY_TILE), f = e - w * (nt * HY_RAY_TILE);
            const int j = f >> 5, r = r0 + w * HY_RAY_TILE + (f & 31);
            const bool in = r < rp;
            mh_tile[(size_t)w * 2 * nt * HY_RAY_TILE + f] = in ? a.at_re[(size_t)j * rp + r] : 0.0f;
            mh_tile[(size_t)(w * 2 + 1) * nt * HY_RAY_TILE + f] = in ? a.at_im[(size_t)j * rp + r] : 0.0f;
        }
        __syncthreads();
        const int rw = r0 + wave * HY_RAY_TILE;                              // this wave's tile
        if (rw >= rp) continue;
        hy_f32x16 met;
        for (int v = 0; v < 16; ++v) met[v] = 0.0f;
        for (int ct = 0; ct < MH_SCORE_CT; ++ct) {
            const int k = ct * 32 + col;
            const bool kin = k < HY_N;
            const int kc = kin ? k : HY_N - 1;                               // subcarriers past the end repeat the last one and enter as zeros
            hy_f32x16 are, aim;
            for (int v = 0; v < 16; ++v) { are[v] = 0.0f; aim[v] = 0.0f; }
            for (int j = 0; j < nt; j += 2) {
                const int jj = j + h;
                const bool in = jj < nt;
                const int jc = in ? jj : nt - 1;
                float ar = t_re[jc * HY_RAY_TILE + col], ai = t_im[jc * HY_RAY_TILE + col];
                float xr = hr[(size_t)jc * HY_N + kc], xi = hi[(size_t)jc * HY_N + kc];
                if (!in) { ar = 0.0f; ai = 0.0f; }
                if (!in || !kin) { xr = 0.0f; xi = 0.0f; }
                // psi = at b:  re = ar xr - ai xi,  im = ar xi + ai xr
                are = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, xr, are, 0, 0, 0);
                aim = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, xi, aim, 0, 0, 0);
                are = __builtin_amdgcn_mfma_f32_32x32x2f32(-ai, xi, are, 0, 0, 0);
                aim = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, xr, aim, 0, 0, 0);
            }
            for (int v = 0; v < 16; ++v) met[v] += are[v] * are[v] + aim[v] * aim[v];
        }
        // accumulator register v of this lane: ray rw + 8 (v / 4) + 4 h + v % 4, subcarrier lane col: sum over the 32 lanes of a half
        for (int v = 0; v < 16; ++v) {
            float x = met[v];
            for (int w = 1; w < 32; w <<= 1) x += __shfl_xor(x, w);
            met[v] = x;
        }
        if (col == 0)
            for (int v = 0; v < 16; ++v) {
                const int ray = rw + 8 * (v >> 2) + 4 * h + (v & 3);
                if (ray < a.rays) out[ray] = met[v];
            }
    }
}
#endif

// ------------------------------------------------------------------------------------------------ greedy selection
template <int THREADS>
HY_KERNEL __launch_bounds__(THREADS) void mu_beam_select_kernel(const MuHybridArgs a) {
    static_assert(THREADS == MH_SELECT_THREADS, "one wave");
    const int M = a.n_users * a.ns, rays = a.rays, n_rf = a.n_rf;
    const int lane = threadIdx.x;
    const size_t p = blockIdx.x;
    const float* S = a.score + p * (size_t)M * rays;
    int taken[HY_MAX_RF];
    for (int q = 0; q < HY_MAX_RF; ++q) taken[q] = -1;
    const float ninf = -__builtin_inff();
    for (int q = 0; q < n_rf; ++q) {
        const float* row = S + (size_t)(q % M) * rays;
        float best = ninf;
        int bidx = 0x7fffffff;
        for (int r = lane; r < rays; r += THREADS) {
            bool free_ = true;
            for (int t = 0; t < HY_MAX_RF; ++t) free_ = free_ && taken[t] != r;
            if (!free_) continue;
            float x = row[r];
            if (!(fabsf(x) <= 3.4028235e38f)) x = ninf;                      // NaN, +-inf
            if (x > best || (x == best && r < bidx)) { best = x; bidx = r; }
        }
        for (int w = 1; w < THREADS; w <<= 1) {
            const float ob = __shfl_xor(best, w);
            const int oi = __shfl_xor(bidx, w);
            if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
        }
        for (int t = 0; t < HY_MAX_RF; ++t)
            if (t == q) taken[t] = bidx;
        if (lane == 0) a.idx[p * (size_t)n_rf + q] = bidx;
    }
}

// ------------------------------------------------------------------------------------------------ baseband stage
// v += f conj(x) over the chains of `groups` groups of four: Fj = row j of the LDS image of Frf (MH_QP complex, zero past n_rf)
#define MH_V_ROW(Fj, vr, vi)                                                                            \
    _Pragma("unroll") for (int g = 0; g < MH_QP / 4; ++g) {                                             \
        if (g >= groups) break;                                                                         \
        const float4 fa = reinterpret_cast<const float4*>(Fj)[2 * g], fb = reinterpret_cast<const float4*>(Fj)[2 * g + 1]; \
        vr = fmaf(fa.x, xr[4 * g], fmaf(fa.y, xi[4 * g], vr));                                          \
        vi = fmaf(fa.y, xr[4 * g], fmaf(-fa.x, xi[4 * g], vi));                                         \
        vr = fmaf(fa.z, xr[4 * g + 1], fmaf(fa.w, xi[4 * g + 1], vr));                                  \
        vi = fmaf(fa.w, xr[4 * g + 1], fmaf(-fa.z, xi[4 * g + 1], vi));                                 \
        vr = fmaf(fb.x, xr[4 * g + 2], fmaf(fb.y, xi[4 * g + 2], vr));                                  \
        vi = fmaf(fb.y, xr[4 * g + 2], fmaf(-fb.x, xi[4 * g + 2], vi));                                 \
        vr = fmaf(fb.z, xr[4 * g + 3], fmaf(fb.w, xi[4 * g + 3], vr));                                  \
        vi = fmaf(fb.w, xr[4 * g + 3], fmaf(-fb.z, xi[4 * g + 3], vi));                                 \
    }
// g_q += b f_q for the same groups
#define MH_G_ONE(f_re, f_im, q)                                                                         \
    gr[q] = fmaf(br, f_re, fmaf(-bi, f_im, gr[q]));                                                     \
    gi[q] = fmaf(br, f_im, fmaf(bi, f_re, gi[q]));

template <int LANES>
HY_KERNEL __launch_bounds__(LANES) void mu_hybrid_precoder_kernel(const MuHybridArgs a) {
    static_assert(LANES == 64 || LANES == 32, "a wave or half of one");
    static_assert(MH_QP == HY_MAX_RF && MH_QP % 4 == 0, "the register rows hold every chain");
    constexpr int TILES = (HY_N + LANES - 1) / LANES;
    extern __shared__ __attribute__((aligned(16))) float mh_smem[];
    const int nt = a.nt, ns = a.ns, nu = a.n_users, M = nu * ns, Q = a.n_rf, rp = a.rp;
    const int groups = (Q + 3) >> 2;
    const int lane = threadIdx.x;
    const size_t p = blockIdx.x / TILES;
    const int k = (int)(blockIdx.x % TILES) * LANES + lane;
    float* F = mh_smem;                                       // Frf [2 (j MH_QP + q) + z], zero past n_rf, shared by the lanes
    float* G = mh_smem + (size_t)2 * nt * MH_QP + lane;       // G, then X = A^-1 G  [2 (m Q + q) + z][lanes]
    float* T = G + (size_t)2 * M * Q * LANES;                 // lower triangle [2 (i (i + 1) / 2 + c) + z][lanes]
#define MH_G(m, q, z) G[(size_t)(2 * ((m) * Q + (q)) + (z)) * LANES]
#define MH_T(i, c, z) T[(size_t)(2 * ((i) * ((i) + 1) / 2 + (c)) + (z)) * LANES]
    const int32_t* idx = a.idx + p * (size_t)Q;
    for (int e = lane; e < nt * MH_QP; e += LANES) {
        const int j = e / MH_QP, q = e - j * MH_QP;
        float fr = 0.f, fi = 0.f;
        if (q < Q) {
            const int r = idx[q];
            fr = a.at_re[(size_t)j * rp + r];
            fi = a.at_im[(size_t)j * rp + r];
        }
        F[2 * e] = fr;
        F[2 * e + 1] = fi;
    }
    __syncthreads();
    if (k >= HY_N) return;                                    // idle lanes of the last tile: behind the only barrier
    const size_t hoff = p * (size_t)a.nr * nt * HY_N + k;

    // ---- G = B Frf, over j in order; one row of G in registers
    for (int u = 0, m = 0; u < nu; ++u)
        for (int s = 0; s < ns; ++s, ++m) {
            const float* hr = a.h_re[u] + hoff + (size_t)s * nt * HY_N;
            const float* hi = a.h_im[u] + hoff + (size_t)s * nt * HY_N;
            float gr[MH_QP], gi[MH_QP];
#pragma unroll
            for (int q = 0; q < MH_QP; ++q) gr[q] = gi[q] = 0.f;
            for (int j = 0; j < nt; ++j) {
                const float br = hr[(size_t)j * HY_N], bi = hi[(size_t)j * HY_N];
                const float4* f4 = reinterpret_cast<const float4*>(F + 2 * j * MH_QP);
#pragma unroll
                for (int g = 0; g < MH_QP / 4; ++g) {
                    if (g >= groups) break;
                    const float4 fa = f4[2 * g], fb = f4[2 * g + 1];
                    MH_G_ONE(fa.x, fa.y, 4 * g)
                    MH_G_ONE(fa.z, fa.w, 4 * g + 1)
                    MH_G_ONE(fb.x, fb.y, 4 * g + 2)
                    MH_G_ONE(fb.z, fb.w, 4 * g + 3)
                }
            }
#pragma unroll
            for (int q = 0; q < MH_QP; ++q) {
                if (q >= Q) break;
                MH_G(m, q, 0) = gr[q];
                MH_G(m, q, 1) = gi[q];
            }
        }
    // ---- A = G G^H + reg I, lower triangle, over q in order; row i of G in registers
    const float reg = a.reg ? a.reg[p] : 0.f;
    for (int i = 0; i < M; ++i) {
        float xr[MH_QP], xi[MH_QP];
#pragma unroll
        for (int q = 0; q < MH_QP; ++q) {
            xr[q] = q < Q ? MH_G(i, q < Q ? q : 0, 0) : 0.f;
            xi[q] = q < Q ? MH_G(i, q < Q ? q : 0, 1) : 0.f;
        }
        for (int c = 0; c <= i; ++c) {
            float sr = 0.f, si = 0.f;
#pragma unroll
            for (int q = 0; q < MH_QP; ++q) {                  // g_i conj(g_c)
                if (q >= Q) break;
                const float yr = MH_G(c, q, 0), yi = MH_G(c, q, 1);
                sr = fmaf(xr[q], yr, fmaf(xi[q], yi, sr));
                si = fmaf(xi[q], yr, fmaf(-xr[q], yi, si));
            }
            MH_T(i, c, 0) = c == i ? sr + reg : sr;
            MH_T(i, c, 1) = c == i ? 0.f : si;
        }
    }
    // ---- Cholesky A = L L^H in place; the imaginary slot of a diagonal element holds 1 / L_ii  (as mu_precoder_kernel)
    bool ok = true;
    for (int c = 0; c < M; ++c) {
        float d = MH_T(c, c, 0);
        for (int q = 0; q < c; ++q) d -= MH_T(c, q, 0) * MH_T(c, q, 0) + MH_T(c, q, 1) * MH_T(c, q, 1);
        if (!(d > 0.f) || !(d <= 3.0e38f)) ok = false;
        const float l = sqrtf(ok ? d : 1.f);
        const float dinv = 1.f / l;
        MH_T(c, c, 0) = l;
        MH_T(c, c, 1) = dinv;
        for (int i = c + 1; i < M; ++i) {
            float sr = MH_T(i, c, 0), si = MH_T(i, c, 1);
            for (int q = 0; q < c; ++q) {                      // - L[i][q] conj(L[c][q])
                const float ar = MH_T(i, q, 0), ai = MH_T(i, q, 1), br = MH_T(c, q, 0), bi = MH_T(c, q, 1);
                sr -= ar * br + ai * bi;
                si -= ai * br - ar * bi;
            }
            MH_T(i, c, 0) = sr * dinv;
            MH_T(i, c, 1) = si * dinv;
        }
    }
    // ---- per column q of G: A x = g_q by two substitutions, in place.  Vbb[q][m] = conj(x_m)
    for (int q = 0; q < Q; ++q) {
        for (int i = 0; i < M; ++i) {                          // L y = g
            float sr = MH_G(i, q, 0), si = MH_G(i, q, 1);
            for (int c = 0; c < i; ++c) {
                const float ar = MH_T(i, c, 0), ai = MH_T(i, c, 1), yr = MH_G(c, q, 0), yi = MH_G(c, q, 1);
                sr -= ar * yr - ai * yi;
                si -= ar * yi + ai * yr;
            }
            const float dinv = MH_T(i, i, 1);
            MH_G(i, q, 0) = sr * dinv;
            MH_G(i, q, 1) = si * dinv;
        }
        for (int i = M - 1; i >= 0; --i) {                     // L^H x = y
            float sr = MH_G(i, q, 0), si = MH_G(i, q, 1);
            for (int c = i + 1; c < M; ++c) {                  // - conj(L[c][i]) x_c
                const float ar = MH_T(c, i, 0), ai = MH_T(c, i, 1), yr = MH_G(c, q, 0), yi = MH_G(c, q, 1);
                sr -= ar * yr + ai * yi;
                si -= ar * yi - ai * yr;
            }
            const float dinv = MH_T(i, i, 1);
            MH_G(i, q, 0) = sr * dinv;
            MH_G(i, q, 1) = si * dinv;
        }
    }
    // ---- per stream m, x_m in registers: V[j][m] = sum_q Frf[j][q] conj(x_m[q]) over q in order; the norm over j in order, c_m, then
    //      W[:, m] = c_m V[:, m] (V formed again) and Fbb[:, m] = c_m Vbb[:, m]
    float* wre = a.w_re + p * (size_t)M * nt * HY_N + k;
    float* wim = a.w_im + p * (size_t)M * nt * HY_N + k;
    for (int m = 0; m < M; ++m) {
        float xr[MH_QP], xi[MH_QP];
#pragma unroll
        for (int q = 0; q < MH_QP; ++q) {
            xr[q] = q < Q ? MH_G(m, q < Q ? q : 0, 0) : 0.f;
            xi[q] = q < Q ? MH_G(m, q < Q ? q : 0, 1) : 0.f;
        }
        float n2 = 0.f;
        for (int j = 0; j < nt; ++j) {
            float vr = 0.f, vi = 0.f;
            MH_V_ROW(F + 2 * j * MH_QP, vr, vi)
            n2 = fmaf(vr, vr, fmaf(vi, vi, n2));
        }
        const float sc = (ok && n2 > 0.f && n2 <= 3.0e38f) ? sqrtf((float)nt / ((float)M * n2)) : 0.f;
        for (int j = 0; j < nt; ++j) {
            float vr = 0.f, vi = 0.f;
            MH_V_ROW(F + 2 * j * MH_QP, vr, vi)
            const size_t o = ((size_t)m * nt + j) * HY_N;
            wre[o] = sc > 0.f ? vr * sc : 0.f;
            wim[o] = sc > 0.f ? vi * sc : 0.f;
        }
        if (a.fbb_re) {
            float* fre = a.fbb_re + (p * (size_t)HY_N + k) * (size_t)Q * M + m;
            float* fim = a.fbb_im + (p * (size_t)HY_N + k) * (size_t)Q * M + m;
#pragma unroll
            for (int q = 0; q < MH_QP; ++q) {
                if (q >= Q) break;
                fre[(size_t)q * M] = sc > 0.f ? xr[q] * sc : 0.f;
                fim[(size_t)q * M] = sc > 0.f ? -xi[q] * sc : 0.f;
            }
        }
    }
#undef MH_G
#undef MH_T
}
#undef MH_V_ROW
#undef MH_G_ONE

}  // namespace csi
