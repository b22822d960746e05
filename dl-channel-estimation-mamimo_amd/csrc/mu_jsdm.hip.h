// mu_jsdm.hip.h - multi-user JSDM precoding: the analog matrix of a packet from the eigenvectors of the users' transmit
// covariances after a block diagonalisation that nulls the other groups, and a zero-forcing baseband precoder per subcarrier behind it.
//
// Reference call site: BER_test_maMIMO_LTF.m:355-389 (helperJSDMTransmitWeights, a toolbox helper outside the reference tree).  The
// algorithm is stated here on its own, from the JSDM definition.
//   shapes    those of mu_link.hip.h: U users with planes [p][Nr][Nt][234], ns streams per user, M = U ns <= 16, stream m = u ns + s,
//             B_k[m][j] = hest_u[p][s][j][k];  group[u] in 0 .. G-1 (every group non-empty), r_star >= 0 directions of a group that the
//             others null, b >= 1 RF chains per group, n_rf = G b <= 16, ns |group g| <= b, (G-1) r_star <= Nt - b, Nt <= 64
//   cov       R_u[j][j'] = (1 / (Nr 234)) sum_{i < Nr} sum_k conj(h_u[i][j][k]) h_u[i][j'][k]   (Hermitian; a beam w has mean gain
//             w^H R w);  R_g = the mean of R_u over the users of group g in ascending user order    mu_cov_kernel (fp32 MFMA)
//   eig       R_g = U_g L_g U_g^H, eigenvalues descending; in each eigenvector the entry of largest modulus is real and positive (the
//             lowest j on a tie);  r_g = the number of i < r_star with l_i > rank_tol l_0 (l_0 <= 0 or not finite: 0);  U*_g = the first
//             r_g columns                                                                          mu_jsdm_eig_kernel, stage 1
//   null      Xi_g = [U*_g' : g' != g, ascending];  Q_g = modified Gram-Schmidt of Xi_g in column order, two passes over the columns
//             kept so far, a column whose residual is <= 1e-3 of its norm is dropped, q_g columns kept;  P = I - Q_g Q_g^H;
//             Rt_g = P R_g P - l_0(R_g) Q_g Q_g^H, symmetrised: span(Q_g) goes to the bottom of the spectrum, so the leading
//             eigenvectors lie in the null space even where P R_g P has rank below b
//   beams     F_g = the first b eigenvectors of Rt_g, same convention; with flag bit 1 every entry becomes exp(i arg) / sqrt(Nt)
//             (arg of an exact 0 is 0);  Frf[p] = [F_0 ... F_{G-1}], Nt x n_rf, flat over the carriers  mu_jsdm_eig_kernel, stage 2
//   baseband  per (p, k), the stage of mu_hybrid.hip.h with the packet's own Frf: Gm = B_k Frf, with flag bit 0 (per-group processing)
//             the entries whose chain's group differs from the stream's group are set to 0;  A = Gm Gm^H + reg[p] I, Cholesky (a pivot
//             <= 0 or not finite: W = 0 and Fbb = 0 for the item), Vbb = Gm^H A^-1, V = Frf Vbb, c_m = sqrt(Nt / M) / |V[:, m]|_2,
//             W[:, m] = c_m V[:, m], Fbb[:, m] = c_m Vbb[:, m]: W = Frf Fbb, |W|_F^2 = Nt, and with bit 0 Fbb is block diagonal with
//             exact zeros elsewhere                                                                mu_jsdm_baseband_kernel
//
// Plan:
//   * mu_cov_kernel<NTILE>: one workgroup of 4 waves per (packet, user); a Hermitian rank-(Nr 234) update as one real product with the
//     complex structure embedded: per 32 x 32 block of (j, j') two accumulators (re, im) fed by four v_mfma_f32_32x32x2_f32 per two
//     carriers.  The contraction runs along the contiguous carrier axis: per receive antenna four slabs of 64 carriers go through LDS
//     (read along the carriers one slab ahead into registers, stored carrier-major with an odd row stride), the 22 carriers past 233 and the antennas past Nt enter as
//     zeros.  Wave w takes carriers 16 w .. 16 w + 15 of every slab; the four partial sums are added in wave order through LDS.
//     NTILE = 1 serves Nt <= 32, NTILE = 2 Nt <= 64 with the three lower blocks.  Only j >= j' is taken from the accumulators; the rest
//     is mirrored, the diagonal's imaginary part is 0: the planes are Hermitian to the bit.
//   * mu_jsdm_eig_kernel: one workgroup per (packet, group), a Hermitian Jacobi solver in LDS (matrix and vectors, 16 Nt^2 bytes, plus
//     4 KiB of tables).  Parallel round-robin ordering over n' = Nt rounded up to even: n' - 1 steps per sweep, n' / 2 disjoint
//     rotations per step (with an odd Nt the index paired with n' - 1 sits out).  A step computes its rotations, then every 2 x 2 block
//     (pair i, pair j), i <= j, is transformed by one thread as J_i^H B J_j and mirrored, so the matrix stays Hermitian to the bit.
//     Stop rule: with s = max_j |A[j][j]| of the input, a rotation is applied where |A[p][q]| > 2^-23 s; the first sweep that applies
//     none ends the iteration, MJ_MAX_SWEEPS = 24 sweeps at the most.  Then the stable descending sort and the phase convention.
//     Stage 2 forms Q_g (wave 0, one lane per antenna, xor butterflies) and Rt_g (one rank-two update per column of Q_g, lower
//     triangle and mirror) in its prologue.
//   * mu_jsdm_baseband_kernel<LANES>: the body of mu_hybrid_precoder_kernel with Frf read from the packet's planes and the mask.
// All arithmetic is fp32 in an order fixed by the shape alone, no atomics: a packet's bits do not depend on the call, the chunk or its
// position in the batch.  The kernels are compiled without packed fp32 and are templates, so they are emitted behind the earlier ones.
#pragma once
#include "mu_hybrid.hip.h"

namespace csi {

constexpr int MJ_MAX_NT = 64;
constexpr int MJ_COV_WAVES = 4;
constexpr int MJ_COV_THREADS = 64 * MJ_COV_WAVES;
constexpr int MJ_COV_SLAB = 64;            // carriers of a slab in LDS: 16 per wave
constexpr int MJ_COV_SLABS = 4;            // 256 carriers, 22 of them zeros
constexpr int MJ_EIG_THREADS = 256;
constexpr int MJ_MAX_SWEEPS = 24;
constexpr int MJ_EIG_TABLE = 1024;         // floats behind the matrix and the vectors
constexpr int MJ_FLAG_PGP = 1, MJ_FLAG_UNIT = 2;

struct MuJsdmArgs {
    const float* h_re[MU_MAX_USERS];   // estimated planes of user u [pkts][nr][nt][234], at the chunk's first packet
    const float* h_im[MU_MAX_USERS];
    float* cov_re;                     // [pkts][U][nt][nt]
    float* cov_im;
    float* eig;                        // [pkts][G][nt]
    float* us_re;                      // [pkts][G][nt][r_star]
    float* us_im;
    int32_t* rank;                     // [pkts][G][2]
    float* frf_re;                     // [pkts][nt][n_rf]
    float* frf_im;
    const float* reg;                  // [pkts] or null (0)
    float* w_re;                       // [pkts][M][nt][234]
    float* w_im;
    float* fbb_re;                     // [pkts][234][n_rf][M] or null
    float* fbb_im;
    float rank_tol;
    int nt, nr, ns, n_users, n_groups, r_star, b, flags, stage;
    signed char group[MU_MAX_USERS];
};

__host__ __device__ inline int mu_cov_stride(int ntile) { return ntile == 1 ? 33 : 97; }     // = 33 mod 64: stores and reads spread over the banks
__host__ __device__ inline size_t mu_cov_lds_bytes(int ntile) { return sizeof(float) * (size_t)2 * MJ_COV_SLAB * mu_cov_stride(ntile); }
__host__ __device__ inline size_t mu_jsdm_eig_lds_bytes(int nt) { return sizeof(float) * ((size_t)4 * nt * nt + MJ_EIG_TABLE); }

// ------------------------------------------------------------------------------------------------ covariance
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
template <int NTILE>
HY_KERNEL __launch_bounds__(MJ_COV_THREADS) void mu_cov_kernel(const MuJsdmArgs a) {
    static_assert(NTILE == 1 || NTILE == 2, "Nt <= 32 or Nt <= 64");
    constexpr int NTP = NTILE == 1 ? 33 : 97;
    constexpr int NBLK = NTILE * (NTILE + 1) / 2;                            // lower blocks (0,0) | (1,0) (1,1)
    constexpr int ROWS = 32 * NTILE;
    constexpr int B10 = NTILE == 2 ? 1 : 0, B11 = NTILE == 2 ? 2 : 0;    // accumulators of the blocks (1,0) and (1,1)
    static_assert(2 * MJ_COV_SLAB * NTP >= NBLK * 2 * 1024, "the partial sums of a wave fit the slab area");
    extern __shared__ __attribute__((aligned(16))) float mj_slab[];          // [2][64 carriers][NTP]; then the partial sums of one wave
    float* s_re = mj_slab;
    float* s_im = mj_slab + MJ_COV_SLAB * NTP;
    const int nt = a.nt, nr = a.nr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, h = lane >> 5;
    const size_t p = blockIdx.x / a.n_users;
    const int u = (int)(blockIdx.x % a.n_users);
    const float* hr = a.h_re[u] + p * (size_t)nr * nt * HY_N;
    const float* hi = a.h_im[u] + p * (size_t)nr * nt * HY_N;
    hy_f32x16 are[NBLK], aim[NBLK];
    for (int t = 0; t < NBLK; ++t)
        for (int v = 0; v < 16; ++v) { are[t][v] = 0.0f; aim[t][v] = 0.0f; }
    // slab `it` = (receive antenna it / 4, carriers 64 (it % 4) ..): PER values per thread and plane, fetched one slab ahead into registers
    constexpr int PER = ROWS * MJ_COV_SLAB / MJ_COV_THREADS;
    float vr[PER], vi[PER];
    const int slabs = nr * MJ_COV_SLABS;
#define MJ_FETCH(it)                                                                                    \
    _Pragma("unroll") for (int x = 0; x < PER; ++x) {                                                   \
        const int e = (int)threadIdx.x + x * MJ_COV_THREADS;                                            \
        const int j = e >> 6, k = ((it) % MJ_COV_SLABS) * MJ_COV_SLAB + (e & 63);                       \
        const bool in = j < nt && k < HY_N;                                                             \
        const size_t o = ((size_t)((it) / MJ_COV_SLABS) * nt + (in ? j : 0)) * HY_N + (in ? k : 0);     \
        vr[x] = in ? hr[o] : 0.0f;                                                                      \
        vi[x] = in ? hi[o] : 0.0f;                                                                      \
    }
    MJ_FETCH(0)
    for (int it = 0; it < slabs; ++it) {
            __syncthreads();                                                 // the waves are through with the slab before
#pragma unroll
            for (int x = 0; x < PER; ++x) {
                const int e = (int)threadIdx.x + x * MJ_COV_THREADS;
                s_re[(e & 63) * NTP + (e >> 6)] = vr[x];
                s_im[(e & 63) * NTP + (e >> 6)] = vi[x];
            }
            __syncthreads();
            if (it + 1 < slabs) { MJ_FETCH(it + 1) }                         // in flight behind the MFMAs of this slab
            for (int s = 0; s < 8; ++s) {
                const int kk = 16 * wave + 2 * s + h;
                const float xr0 = s_re[kk * NTP + col], xi0 = s_im[kk * NTP + col];
                // conj(x_j) x_j':  re = xr_j xr_j' + xi_j xi_j',  im = xr_j xi_j' - xi_j xr_j'   (first operand: row j, second: column j')
                are[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(xr0, xr0, are[0], 0, 0, 0);
                aim[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(xr0, xi0, aim[0], 0, 0, 0);
                are[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(xi0, xi0, are[0], 0, 0, 0);
                aim[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(-xi0, xr0, aim[0], 0, 0, 0);
                if (NTILE == 2) {
                    const float xr1 = s_re[kk * NTP + 32 + col], xi1 = s_im[kk * NTP + 32 + col];
                    are[B10] = __builtin_amdgcn_mfma_f32_32x32x2f32(xr1, xr0, are[B10], 0, 0, 0);
                    aim[B10] = __builtin_amdgcn_mfma_f32_32x32x2f32(xr1, xi0, aim[B10], 0, 0, 0);
                    are[B10] = __builtin_amdgcn_mfma_f32_32x32x2f32(xi1, xi0, are[B10], 0, 0, 0);
                    aim[B10] = __builtin_amdgcn_mfma_f32_32x32x2f32(-xi1, xr0, aim[B10], 0, 0, 0);
                    are[B11] = __builtin_amdgcn_mfma_f32_32x32x2f32(xr1, xr1, are[B11], 0, 0, 0);
                    aim[B11] = __builtin_amdgcn_mfma_f32_32x32x2f32(xr1, xi1, aim[B11], 0, 0, 0);
                    are[B11] = __builtin_amdgcn_mfma_f32_32x32x2f32(xi1, xi1, are[B11], 0, 0, 0);
                    aim[B11] = __builtin_amdgcn_mfma_f32_32x32x2f32(-xi1, xr1, aim[B11], 0, 0, 0);
                }
            }
        }
#undef MJ_FETCH
    // wave 0 + wave 1 + wave 2 + wave 3, in that order, through the slab area: [block][re | im][register v][lane]
    for (int w = 1; w < MJ_COV_WAVES; ++w) {
        __syncthreads();
        if (wave == w)
            for (int t = 0; t < NBLK; ++t)
                for (int v = 0; v < 16; ++v) {
                    mj_slab[((t * 2 + 0) * 16 + v) * 64 + lane] = are[t][v];
                    mj_slab[((t * 2 + 1) * 16 + v) * 64 + lane] = aim[t][v];
                }
        __syncthreads();
        if (wave == 0)
            for (int t = 0; t < NBLK; ++t)
                for (int v = 0; v < 16; ++v) {
                    are[t][v] += mj_slab[((t * 2 + 0) * 16 + v) * 64 + lane];
                    aim[t][v] += mj_slab[((t * 2 + 1) * 16 + v) * 64 + lane];
                }
    }
    if (wave != 0) return;
    // accumulator register v of this lane: row 8 (v / 4) + 4 h + v % 4, column col of the block
    const float scale = 1.0f / ((float)nr * (float)HY_N);
    float* o_re = a.cov_re + (size_t)blockIdx.x * nt * nt;
    float* o_im = a.cov_im + (size_t)blockIdx.x * nt * nt;
    for (int t = 0; t < NBLK; ++t) {
        const int ta = t == 0 ? 0 : 1, tb = t == 2 ? 1 : 0;
        for (int v = 0; v < 16; ++v) {
            const int j = 32 * ta + 8 * (v >> 2) + 4 * h + (v & 3), jp = 32 * tb + col;
            if (j >= nt || jp >= nt || j < jp) continue;
            const float re = are[t][v] * scale, im = j == jp ? 0.0f : aim[t][v] * scale;
            o_re[(size_t)j * nt + jp] = re;
            o_im[(size_t)j * nt + jp] = im;
            if (j != jp) {
                o_re[(size_t)jp * nt + j] = re;
                o_im[(size_t)jp * nt + j] = -im;
            }
        }
    }
}
#endif

// ------------------------------------------------------------------------------------------------ eigenvectors, nulling, beams
// sum over the 64 lanes of a wave, the same bits in every lane
HY_NO_PK __device__ inline float mj_wave_sum(float x) {
    for (int w = 1; w < 64; w <<= 1) x += __shfl_xor(x, w);
    return x;
}

template <int THREADS>
HY_KERNEL __launch_bounds__(THREADS) void mu_jsdm_eig_kernel(const MuJsdmArgs a) {
    static_assert(THREADS == MJ_EIG_THREADS && THREADS >= 2 * MJ_MAX_NT, "a thread per antenna, wave 0 for the Gram-Schmidt");
    extern __shared__ __attribute__((aligned(16))) float mj_eig[];
    const int nt = a.nt, G = a.n_groups, nn = nt * nt;
    const int tid = threadIdx.x;
    float* Ar = mj_eig;                    // [nt][nt]
    float* Ai = Ar + nn;
    float* Vr = Ai + nn;                   // vectors [nt][nt]; in the prologue of stage 2: Q, column c at [c nt + j]
    float* Vi = Vr + nn;
    float* tab = Vi + nn;                  // MJ_EIG_TABLE floats
    float* rc = tab;                       // [32] rotation of pair i: c, s, e^{i phi} = (er, ei), t |a_pq|
    float* rs = tab + 32;
    float* rer = tab + 64;
    float* rei = tab + 96;
    float* rtb = tab + 128;
    int* rp = reinterpret_cast<int*>(tab + 160);   // [32] the pair (p < q); q >= nt: p sits out
    int* rq = reinterpret_cast<int*>(tab + 192);
    int* ron = reinterpret_cast<int*>(tab + 224);  // [32] 1: pair i rotates in this step
    float* lam = tab + 256;                // [64]
    int* perm = reinterpret_cast<int*>(tab + 320);  // [64] perm[rank] = index
    float* fr = tab + 384;                 // [64] phase factor of column j
    float* fi = tab + 448;
    int* jmx = reinterpret_cast<int*>(tab + 512);   // [64] row of the largest entry of column j
    float* yr = tab + 576;                 // [64]
    float* yi = tab + 640;
    int* misc = reinterpret_cast<int*>(tab + 704);  // [0] rotations of the sweep, [1] r_g, [2] q_g
    const size_t p = blockIdx.x / G;
    const int g = (int)(blockIdx.x % G);
    const size_t item = p * (size_t)G + g;

    // ---- R_g: the mean over the group's users in ascending order; (X + X^H) / 2 leaves a Hermitian input as it is
    int cnt = 0;
    for (int u = 0; u < a.n_users; ++u) cnt += a.group[u] == g ? 1 : 0;
    for (int e = tid; e < nn; e += THREADS) {
        const int r = e / nt, c = e - r * nt, et = c * nt + r;
        float sr = 0.f, si = 0.f, tr = 0.f, ti = 0.f;
        for (int u = 0; u < a.n_users; ++u)
            if (a.group[u] == g) {
                const size_t o = (p * (size_t)a.n_users + u) * (size_t)nn;
                sr += a.cov_re[o + e]; si += a.cov_im[o + e];
                tr += a.cov_re[o + et]; ti += a.cov_im[o + et];
            }
        Ar[e] = 0.5f * (sr + tr) / (float)cnt;
        Ai[e] = r == c ? 0.f : 0.5f * (si - ti) / (float)cnt;
    }
    if (tid == 0) { misc[0] = 0; misc[1] = 0; misc[2] = 0; }
    __syncthreads();

    if (a.stage == 2) {
        // ---- Q_g by modified Gram-Schmidt, wave 0, lane = antenna
        if (tid < 64) {
            const int j = tid;
            int qn = 0;
            for (int g2 = 0; g2 < G; ++g2) {
                if (g2 == g) continue;
                const size_t it2 = p * (size_t)G + g2;
                int r2 = a.rank[it2 * 2];
                r2 = r2 < 0 ? 0 : (r2 > a.r_star ? a.r_star : r2);
                for (int i = 0; i < r2; ++i) {
                    float vr = 0.f, vi = 0.f;
                    if (j < nt) {
                        vr = a.us_re[(it2 * nt + j) * (size_t)a.r_star + i];
                        vi = a.us_im[(it2 * nt + j) * (size_t)a.r_star + i];
                    }
                    const float n0 = sqrtf(mj_wave_sum(fmaf(vr, vr, vi * vi)));
                    for (int pass = 0; pass < 2; ++pass)
                        for (int c = 0; c < qn; ++c) {
                            const float qr = j < nt ? Vr[c * nt + j] : 0.f, qi = j < nt ? Vi[c * nt + j] : 0.f;
                            const float dr = mj_wave_sum(fmaf(qr, vr, qi * vi));          // q^H v
                            const float di = mj_wave_sum(fmaf(qr, vi, -qi * vr));
                            vr -= qr * dr - qi * di;
                            vi -= qr * di + qi * dr;
                        }
                    const float res = sqrtf(mj_wave_sum(fmaf(vr, vr, vi * vi)));
                    if (res > 1e-3f * n0 && res <= 3.0e38f && qn < nt) {
                        if (j < nt) { Vr[qn * nt + j] = vr / res; Vi[qn * nt + j] = vi / res; }
                        ++qn;
                    }
                }
            }
            if (tid == 0) misc[2] = qn;
        }
        __syncthreads();
        const int qn = misc[2];
        const float lam0 = a.eig[item * nt];
        // ---- Rt = P R P - lam0 Q Q^H, one column q of Q at a time: R <- R - q y^H - y q^H + (q^H y - lam0) q q^H with y = R q
        for (int c = 0; c < qn; ++c) {
            const float* qr = Vr + c * nt;
            const float* qi = Vi + c * nt;
            if (tid < nt) {
                float sr = 0.f, si = 0.f;
                for (int k = 0; k < nt; ++k) {
                    const float xr = Ar[tid * nt + k], xi = Ai[tid * nt + k];
                    sr = fmaf(xr, qr[k], fmaf(-xi, qi[k], sr));
                    si = fmaf(xr, qi[k], fmaf(xi, qr[k], si));
                }
                yr[tid] = sr; yi[tid] = si;
            }
            __syncthreads();
            float al = 0.f;
            for (int k = 0; k < nt; ++k) al = fmaf(qr[k], yr[k], fmaf(qi[k], yi[k], al));
            al -= lam0;
            for (int e = tid; e < nn; e += THREADS) {                         // lower triangle; an element depends on itself, q and y only
                const int r = e / nt, cc = e - r * nt;
                if (r < cc) continue;
                // q_r conj(y_c) + y_r conj(q_c) - al q_r conj(q_c)
                const float t1r = qr[r] * yr[cc] + qi[r] * yi[cc], t1i = qi[r] * yr[cc] - qr[r] * yi[cc];
                const float t2r = yr[r] * qr[cc] + yi[r] * qi[cc], t2i = yi[r] * qr[cc] - yr[r] * qi[cc];
                const float t3r = qr[r] * qr[cc] + qi[r] * qi[cc], t3i = qi[r] * qr[cc] - qr[r] * qi[cc];
                const float xr = Ar[e] - t1r - t2r + al * t3r;
                const float xi = r == cc ? 0.f : Ai[e] - t1i - t2i + al * t3i;
                Ar[e] = xr; Ai[e] = xi;
                Ar[cc * nt + r] = xr; Ai[cc * nt + r] = -xi;
            }
            __syncthreads();
        }
    }

    // ---- V = I, the scale of the stop rule
    for (int e = tid; e < nn; e += THREADS) {
        const int r = e / nt, c = e - r * nt;
        Vr[e] = r == c ? 1.f : 0.f;
        Vi[e] = 0.f;
    }
    float smax = 0.f;
    for (int j = 0; j < nt; ++j) smax = fmaxf(smax, fabsf(Ar[j * nt + j]));
    const float thr = smax * 1.1920929e-7f;
    const int n2 = (nt + 1) & ~1, m = n2 >> 1, steps = n2 - 1;
    __syncthreads();

    for (int sweep = 0; sweep < MJ_MAX_SWEEPS; ++sweep) {
        for (int t = 0; t < steps; ++t) {
            if (tid < m) {
                // circle method: n2 - 1 stays, the others turn
                int x = tid == 0 ? n2 - 1 : (t + tid) % steps;
                int y = tid == 0 ? t : (t - tid + steps) % steps;
                const int pp = x < y ? x : y, qq = x < y ? y : x;
                float c = 1.f, s = 0.f, er = 1.f, ei = 0.f, tb = 0.f;
                int on = 0;
                if (qq < nt) {
                    const float br = Ar[pp * nt + qq], bi = Ai[pp * nt + qq];
                    const float bm = sqrtf(fmaf(br, br, bi * bi));
                    if (bm > thr && bm <= 3.0e38f) {
                        const float tau = (Ar[qq * nt + qq] - Ar[pp * nt + pp]) / (2.f * bm);
                        const float tt = (tau >= 0.f ? 1.f : -1.f) / (fabsf(tau) + sqrtf(fmaf(tau, tau, 1.f)));
                        c = 1.f / sqrtf(fmaf(tt, tt, 1.f));
                        s = tt * c;
                        er = br / bm; ei = bi / bm;
                        tb = tt * bm;
                        on = 1;
                        misc[0] = 1;                                         // every writer stores the same value; read behind the step's barriers
                    }
                }
                rc[tid] = c; rs[tid] = s; rer[tid] = er; rei[tid] = ei; rtb[tid] = tb; rp[tid] = pp; rq[tid] = qq; ron[tid] = on;
            }
            __syncthreads();
            // J = [[c, s], [-s e^{-i phi}, c e^{-i phi}]]:  rows by J_i^H, columns by J_j
            for (int e = tid; e < m * m; e += THREADS) {
                const int i = e / m, j = e - i * m;
                if (i > j) continue;
                const int pi = rp[i], qi_ = rq[i], pj = rp[j], qj = rq[j];
                const bool hi_ = qi_ < nt, hj = qj < nt;
                if (i == j) {
                    if (ron[i]) {
                        Ar[pi * nt + pi] -= rtb[i];
                        Ar[qi_ * nt + qi_] += rtb[i];
                        Ar[pi * nt + qi_] = 0.f; Ai[pi * nt + qi_] = 0.f;
                        Ar[qi_ * nt + pi] = 0.f; Ai[qi_ * nt + pi] = 0.f;
                    }
                    continue;
                }
                if (!ron[i] && !ron[j]) continue;
                float b00r = Ar[pi * nt + pj], b00i = Ai[pi * nt + pj];
                float b01r = hj ? Ar[pi * nt + qj] : 0.f, b01i = hj ? Ai[pi * nt + qj] : 0.f;
                float b10r = hi_ ? Ar[qi_ * nt + pj] : 0.f, b10i = hi_ ? Ai[qi_ * nt + pj] : 0.f;
                float b11r = hi_ && hj ? Ar[qi_ * nt + qj] : 0.f, b11i = hi_ && hj ? Ai[qi_ * nt + qj] : 0.f;
                {   // rows: p' = c p - s e^{i phi} q,  q' = s p + c e^{i phi} q
                    const float c = rc[i], s = rs[i], er = rer[i], ei = rei[i];
                    const float z0r = er * b10r - ei * b10i, z0i = er * b10i + ei * b10r;     // e^{i phi} row q
                    const float z1r = er * b11r - ei * b11i, z1i = er * b11i + ei * b11r;
                    const float n00r = c * b00r - s * z0r, n00i = c * b00i - s * z0i;
                    const float n01r = c * b01r - s * z1r, n01i = c * b01i - s * z1i;
                    b10r = s * b00r + c * z0r; b10i = s * b00i + c * z0i;
                    b11r = s * b01r + c * z1r; b11i = s * b01i + c * z1i;
                    b00r = n00r; b00i = n00i; b01r = n01r; b01i = n01i;
                }
                {   // columns: p' = c p - s e^{-i phi} q,  q' = s p + c e^{-i phi} q
                    const float c = rc[j], s = rs[j], er = rer[j], ei = rei[j];
                    const float z0r = er * b01r + ei * b01i, z0i = er * b01i - ei * b01r;     // e^{-i phi} column q
                    const float z1r = er * b11r + ei * b11i, z1i = er * b11i - ei * b11r;
                    const float n00r = c * b00r - s * z0r, n00i = c * b00i - s * z0i;
                    const float n10r = c * b10r - s * z1r, n10i = c * b10i - s * z1i;
                    b01r = s * b00r + c * z0r; b01i = s * b00i + c * z0i;
                    b11r = s * b10r + c * z1r; b11i = s * b10i + c * z1i;
                    b00r = n00r; b00i = n00i; b10r = n10r; b10i = n10i;
                }
                Ar[pi * nt + pj] = b00r; Ai[pi * nt + pj] = b00i; Ar[pj * nt + pi] = b00r; Ai[pj * nt + pi] = -b00i;
                if (hj) { Ar[pi * nt + qj] = b01r; Ai[pi * nt + qj] = b01i; Ar[qj * nt + pi] = b01r; Ai[qj * nt + pi] = -b01i; }
                if (hi_) { Ar[qi_ * nt + pj] = b10r; Ai[qi_ * nt + pj] = b10i; Ar[pj * nt + qi_] = b10r; Ai[pj * nt + qi_] = -b10i; }
                if (hi_ && hj) { Ar[qi_ * nt + qj] = b11r; Ai[qi_ * nt + qj] = b11i; Ar[qj * nt + qi_] = b11r; Ai[qj * nt + qi_] = -b11i; }
            }
            for (int e = tid; e < nt * m; e += THREADS) {                     // V <- V J_j, row r
                const int r = e / m, j = e - r * m;
                if (!ron[j]) continue;
                const int pj = rp[j], qj = rq[j];
                const float c = rc[j], s = rs[j], er = rer[j], ei = rei[j];
                const float v0r = Vr[r * nt + pj], v0i = Vi[r * nt + pj], v1r = Vr[r * nt + qj], v1i = Vi[r * nt + qj];
                const float zr = er * v1r + ei * v1i, zi = er * v1i - ei * v1r;
                Vr[r * nt + pj] = c * v0r - s * zr; Vi[r * nt + pj] = c * v0i - s * zi;
                Vr[r * nt + qj] = s * v0r + c * zr; Vi[r * nt + qj] = s * v0i + c * zi;
            }
            __syncthreads();
        }
        const bool done = misc[0] == 0;
        __syncthreads();
        if (done) break;
        if (tid == 0) misc[0] = 0;
        __syncthreads();
    }

    // ---- descending, stable; a value that is not finite sorts as -inf
    if (tid < nt) {
        const float x = Ar[tid * nt + tid];
        lam[tid] = fabsf(x) <= 3.4028235e38f ? x : -__builtin_inff();
    }
    __syncthreads();
    if (tid < nt) {
        const float x = lam[tid];
        int rk = 0;
        for (int i = 0; i < nt; ++i) rk += (lam[i] > x || (lam[i] == x && i < tid)) ? 1 : 0;
        perm[rk] = tid;
        // phase: the entry of largest modulus of column tid becomes real and positive
        float best = -1.f;
        int jb = 0;
        for (int j = 0; j < nt; ++j) {
            const float q2 = fmaf(Vr[j * nt + tid], Vr[j * nt + tid], Vi[j * nt + tid] * Vi[j * nt + tid]);
            if (q2 > best) { best = q2; jb = j; }
        }
        const float md = sqrtf(best);
        const bool ok = md > 0.f && md <= 3.0e38f;
        fr[tid] = ok ? Vr[jb * nt + tid] / md : 1.f;                          // multiply by conj(v_jb) / |v_jb|
        fi[tid] = ok ? -Vi[jb * nt + tid] / md : 0.f;
        jmx[tid] = ok ? jb : -1;
    }
    __syncthreads();
    if (a.stage == 1) {
        if (tid == 0) {
            const float l0 = lam[perm[0]];
            int rg = 0;
            if (l0 > 0.f)
                for (int i = 0; i < a.r_star; ++i) rg += lam[perm[i]] > a.rank_tol * l0 ? 1 : 0;
            misc[1] = rg;
            a.rank[item * 2] = rg;
        }
        if (tid < nt) a.eig[item * nt + tid] = Ar[perm[tid] * nt + perm[tid]];
        __syncthreads();
        const int rg = misc[1];
        for (int e = tid; e < nt * a.r_star; e += THREADS) {
            const int j = e / a.r_star, i = e - j * a.r_star;
            float vr = 0.f, vi = 0.f;
            if (i < rg) {
                const int c = perm[i];
                const float xr = Vr[j * nt + c], xi = Vi[j * nt + c];
                vr = jmx[c] == j ? sqrtf(fmaf(xr, xr, xi * xi)) : xr * fr[c] - xi * fi[c];
                vi = jmx[c] == j ? 0.f : xr * fi[c] + xi * fr[c];
            }
            a.us_re[item * nt * a.r_star + e] = vr;
            a.us_im[item * nt * a.r_star + e] = vi;
        }
    } else {
        const int b = a.b, n_rf = G * b;
        if (tid == 0) a.rank[item * 2 + 1] = misc[2];
        const float inv = 1.f / sqrtf((float)nt);
        for (int e = tid; e < nt * b; e += THREADS) {
            const int j = e / b, i = e - j * b, c = perm[i];
            const float xr = Vr[j * nt + c], xi = Vi[j * nt + c];
            float vr = jmx[c] == j ? sqrtf(fmaf(xr, xr, xi * xi)) : xr * fr[c] - xi * fi[c];
            float vi = jmx[c] == j ? 0.f : xr * fi[c] + xi * fr[c];
            if (a.flags & MJ_FLAG_UNIT) {
                const float md = sqrtf(fmaf(vr, vr, vi * vi));
                const bool ok = md > 0.f && md <= 3.0e38f;
                vr = ok ? vr / md * inv : inv;
                vi = ok ? vi / md * inv : 0.f;
            }
            a.frf_re[(p * (size_t)nt + j) * n_rf + g * b + i] = vr;
            a.frf_im[(p * (size_t)nt + j) * n_rf + g * b + i] = vi;
        }
    }
}

// ------------------------------------------------------------------------------------------------ baseband stage
// the loops of mu_hybrid_precoder_kernel (mu_hybrid.hip.h), a copy: that kernel's instances stay the machine code they were
#define MJ_V_ROW(Fj, vr, vi)                                                                            \
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
#define MJ_G_ONE(f_re, f_im, q)                                                                         \
    gr[q] = fmaf(br, f_re, fmaf(-bi, f_im, gr[q]));                                                     \
    gi[q] = fmaf(br, f_im, fmaf(bi, f_re, gi[q]));

template <int LANES>
HY_KERNEL __launch_bounds__(LANES) void mu_jsdm_baseband_kernel(const MuJsdmArgs a) {
    static_assert(LANES == 64 || LANES == 32, "a wave or half of one");
    static_assert(MH_QP == HY_MAX_RF && MH_QP % 4 == 0, "the register rows hold every chain");
    constexpr int TILES = (HY_N + LANES - 1) / LANES;
    extern __shared__ __attribute__((aligned(16))) float mj_smem[];
    const int nt = a.nt, ns = a.ns, nu = a.n_users, M = nu * ns, Q = a.n_groups * a.b;
    const int groups = (Q + 3) >> 2;
    const int lane = threadIdx.x;
    const size_t p = blockIdx.x / TILES;
    const int k = (int)(blockIdx.x % TILES) * LANES + lane;
    float* F = mj_smem;                                       // Frf [2 (j MH_QP + q) + z], zero past n_rf, shared by the lanes
    float* G = mj_smem + (size_t)2 * nt * MH_QP + lane;       // Gm, then X = A^-1 Gm  [2 (m Q + q) + z][lanes]
    float* T = G + (size_t)2 * M * Q * LANES;                 // lower triangle [2 (i (i + 1) / 2 + c) + z][lanes]
#define MJ_G(m, q, z) G[(size_t)(2 * ((m) * Q + (q)) + (z)) * LANES]
#define MJ_T(i, c, z) T[(size_t)(2 * ((i) * ((i) + 1) / 2 + (c)) + (z)) * LANES]
    for (int e = lane; e < nt * MH_QP; e += LANES) {
        const int j = e / MH_QP, q = e - j * MH_QP;
        float fr = 0.f, fi = 0.f;
        if (q < Q) {
            fr = a.frf_re[(p * (size_t)nt + j) * Q + q];
            fi = a.frf_im[(p * (size_t)nt + j) * Q + q];
        }
        F[2 * e] = fr;
        F[2 * e + 1] = fi;
    }
    __syncthreads();
    if (k >= HY_N) return;                                    // idle lanes of the last tile: behind the only barrier
    const size_t hoff = p * (size_t)a.nr * nt * HY_N + k;
    const bool pgp = (a.flags & MJ_FLAG_PGP) != 0;

    // ---- Gm = B Frf, over j in order; one row in registers; per-group processing keeps the chains of the stream's own group
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
                    MJ_G_ONE(fa.x, fa.y, 4 * g)
                    MJ_G_ONE(fa.z, fa.w, 4 * g + 1)
                    MJ_G_ONE(fb.x, fb.y, 4 * g + 2)
                    MJ_G_ONE(fb.z, fb.w, 4 * g + 3)
                }
            }
            const int q_lo = (int)a.group[u] * a.b, q_hi = q_lo + a.b;
#pragma unroll
            for (int q = 0; q < MH_QP; ++q) {
                if (q >= Q) break;
                const bool keep = !pgp || (q >= q_lo && q < q_hi);
                MJ_G(m, q, 0) = keep ? gr[q] : 0.f;
                MJ_G(m, q, 1) = keep ? gi[q] : 0.f;
            }
        }
    // ---- A = Gm Gm^H + reg I, lower triangle, over q in order; row i in registers
    const float reg = a.reg ? a.reg[p] : 0.f;
    for (int i = 0; i < M; ++i) {
        float xr[MH_QP], xi[MH_QP];
#pragma unroll
        for (int q = 0; q < MH_QP; ++q) {
            xr[q] = q < Q ? MJ_G(i, q < Q ? q : 0, 0) : 0.f;
            xi[q] = q < Q ? MJ_G(i, q < Q ? q : 0, 1) : 0.f;
        }
        for (int c = 0; c <= i; ++c) {
            float sr = 0.f, si = 0.f;
#pragma unroll
            for (int q = 0; q < MH_QP; ++q) {                  // g_i conj(g_c)
                if (q >= Q) break;
                const float yr = MJ_G(c, q, 0), yi = MJ_G(c, q, 1);
                sr = fmaf(xr[q], yr, fmaf(xi[q], yi, sr));
                si = fmaf(xi[q], yr, fmaf(-xr[q], yi, si));
            }
            MJ_T(i, c, 0) = c == i ? sr + reg : sr;
            MJ_T(i, c, 1) = c == i ? 0.f : si;
        }
    }
    // ---- Cholesky A = L L^H in place; the imaginary slot of a diagonal element holds 1 / L_ii
    bool ok = true;
    for (int c = 0; c < M; ++c) {
        float d = MJ_T(c, c, 0);
        for (int q = 0; q < c; ++q) d -= MJ_T(c, q, 0) * MJ_T(c, q, 0) + MJ_T(c, q, 1) * MJ_T(c, q, 1);
        if (!(d > 0.f) || !(d <= 3.0e38f)) ok = false;
        const float l = sqrtf(ok ? d : 1.f);
        const float dinv = 1.f / l;
        MJ_T(c, c, 0) = l;
        MJ_T(c, c, 1) = dinv;
        for (int i = c + 1; i < M; ++i) {
            float sr = MJ_T(i, c, 0), si = MJ_T(i, c, 1);
            for (int q = 0; q < c; ++q) {                      // - L[i][q] conj(L[c][q])
                const float ar = MJ_T(i, q, 0), ai = MJ_T(i, q, 1), br = MJ_T(c, q, 0), bi = MJ_T(c, q, 1);
                sr -= ar * br + ai * bi;
                si -= ai * br - ar * bi;
            }
            MJ_T(i, c, 0) = sr * dinv;
            MJ_T(i, c, 1) = si * dinv;
        }
    }
    // ---- per column q of Gm: A x = g_q by two substitutions, in place.  Vbb[q][m] = conj(x_m)
    for (int q = 0; q < Q; ++q) {
        for (int i = 0; i < M; ++i) {                          // L y = g
            float sr = MJ_G(i, q, 0), si = MJ_G(i, q, 1);
            for (int c = 0; c < i; ++c) {
                const float ar = MJ_T(i, c, 0), ai = MJ_T(i, c, 1), yr = MJ_G(c, q, 0), yi = MJ_G(c, q, 1);
                sr -= ar * yr - ai * yi;
                si -= ar * yi + ai * yr;
            }
            const float dinv = MJ_T(i, i, 1);
            MJ_G(i, q, 0) = sr * dinv;
            MJ_G(i, q, 1) = si * dinv;
        }
        for (int i = M - 1; i >= 0; --i) {                     // L^H x = y
            float sr = MJ_G(i, q, 0), si = MJ_G(i, q, 1);
            for (int c = i + 1; c < M; ++c) {                  // - conj(L[c][i]) x_c
                const float ar = MJ_T(c, i, 0), ai = MJ_T(c, i, 1), yr = MJ_G(c, q, 0), yi = MJ_G(c, q, 1);
                sr -= ar * yr + ai * yi;
                si -= ar * yi - ai * yr;
            }
            const float dinv = MJ_T(i, i, 1);
            MJ_G(i, q, 0) = sr * dinv;
            MJ_G(i, q, 1) = si * dinv;
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
            xr[q] = q < Q ? MJ_G(m, q < Q ? q : 0, 0) : 0.f;
            xi[q] = q < Q ? MJ_G(m, q < Q ? q : 0, 1) : 0.f;
        }
        float n2 = 0.f;
        for (int j = 0; j < nt; ++j) {
            float vr = 0.f, vi = 0.f;
            MJ_V_ROW(F + 2 * j * MH_QP, vr, vi)
            n2 = fmaf(vr, vr, fmaf(vi, vi, n2));
        }
        const float sc = (ok && n2 > 0.f && n2 <= 3.0e38f) ? sqrtf((float)nt / ((float)M * n2)) : 0.f;
        for (int j = 0; j < nt; ++j) {
            float vr = 0.f, vi = 0.f;
            MJ_V_ROW(F + 2 * j * MH_QP, vr, vi)
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
#undef MJ_G
#undef MJ_T
}
#undef MJ_V_ROW
#undef MJ_G_ONE

}  // namespace csi
