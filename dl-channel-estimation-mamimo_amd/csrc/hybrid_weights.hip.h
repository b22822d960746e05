// hybrid_weights.hip.h - hybrid beamforming weights (SVD + orthogonal matching pursuit) from a CSI tensor.
//
// Reference call sites: BER_test_maMIMO_LTF.m:347-376, generate_maMIMO_LTF.m:414-425 (omphybweights / ompdecomp of the
// toolbox).  One item = one (packet, subcarrier); H[i][j] = csi[p][i][j][k] is Nr x Nt.  Per item:
//   Fopt = right singular vectors of H for the Ns largest singular values              hyb_svd_kernel
//   for m = 0 .. NtRF-1:
//       k_m = argmax_k sum_s |At[:,k]^H Res[:,s]|^2  (lowest k on a tie)                hyb_corr_kernel   (fp32 MFMA)
//       C = (A^H A)^-1 A^H Fopt,  T = Fopt - A C,  e = |T|_F,  Res = T / e              hyb_solve_kernel
//   Fbb = sqrt(Ns) C / |A C|_F;  gain = |H_eval A Fbb|_F^2;  mean of At[:,k_m] over a packet's subcarriers
//                                                                                       hyb_gain_kernel, hyb_frf_mean_kernel
// Plan:
//   * hyb_svd_kernel: one lane per item, so the [p][i][j][k] planes are read coalesced along k.  The Nr x Nr Hermitian
//     H H^H is formed and diagonalised by cyclic Jacobi in fp64 (squaring H costs (sigma_1 / sigma_s)^2 of the fp32 budget,
//     the fp64 vector rate of gfx950 makes the wider type free here, as for the LMMSE solve); the matrix and its
//     eigenvectors live in LDS, [element][lane], so the run-time indexed accesses never leave the CU.
//     Fopt = H^H u / sigma is written in fp32, [s][j][item]: unit stride over items for every later reader.
//   * hyb_corr_kernel: Psi = At^H Res of all items of a chunk as one real product with the complex structure embedded:
//     per 32 rays x 32 items two accumulators (re, im) fed by four v_mfma_f32_32x32x2_f32 per two antennas.  The epilogue
//     squares, adds re, im and the Ns streams and keeps a running (max, lowest index) per item across the ray tiles,
//     so Psi is never written.  The dictionary goes through LDS in tiles of 32 rays; no atomics, fixed order.
//   * hyb_solve_kernel: one lane per item.  The Cholesky factor of A^H A grows by one row per step (its entries are
//     Nt-long products of dictionary columns, gathered from L2), y = L^-1 A^H Fopt grows by one row, C = L^-H y is
//     back-substituted, then T, e and the normalised residual.  Per-item state lives in the workspace, [element][item].
// re and im stay in separate registers and planes everywhere (no complex types: DESIGN.md 4.12).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace csi {

constexpr int HY_N = 234;
constexpr int HY_MAX_RF = 16;              // RF chains (OMP steps) per item
constexpr int HY_MAX_NR = 16;              // rx antennas the singular-vector kernel takes (4 nr^2 doubles per lane in LDS)
constexpr int HY_MAX_RAYS = 4096;
constexpr int HY_RAY_TILE = 32;
constexpr int HY_SWEEPS = 12;              // cyclic Jacobi sweeps (fp64; 16 x 16 converges in 7 - 9)
constexpr int HY_CORR_THREADS = 256;       // 4 waves x 32 items
constexpr int HY_CORR_ITEMS = 128;
constexpr int HY_ITEM_THREADS = 64;
constexpr float HY_DEFAULT_STOP_TOL = 1e-5f;

typedef float hy_f32x16 __attribute__((ext_vector_type(16)));

struct HybArgs {
    const float* h_re;      // CSI planes of the chunk [pkts][nr][nt][234]
    const float* h_im;
    const float* e_re;      // evaluation channel of the gain (the same planes when the caller gave none)
    const float* e_im;
    const float* at_re;     // dictionary [nt][rp], rp = rays rounded up to 32, zero padded
    const float* at_im;
    float* fopt_re;         // workspace [ns][nt][n]
    float* fopt_im;
    float* res_re;          // workspace [ns][nt][n]: the residual; after an item's last step the full-band weights A Fbb
    float* res_im;
    float* chol;            // workspace [ntrf (ntrf + 1)][n]: packed lower triangle, (re, im) per entry
    float* yv;              // workspace [ntrf][ns][2][n]
    float* cv;              // workspace [ntrf][ns][2][n]
    int* cand;              // workspace [n]: the correlation kernel's choice of this step
    int* state;             // workspace [2][n]: atoms so far, finished flag
    float* fbb_re;          // [n][ns][ntrf]
    float* fbb_im;
    int* idx;               // [n][ntrf]
    int* n_atoms;           // [n] or null
    float* gain;            // [n] or null
    int nt, nr, ns, ntrf, rays, rp;
    int n;                  // items of the chunk (packets x 234)
    int step;
    float stop_tol;
};

// These kernels are written re / im planar, and the compiler's pairing of the two halves of a complex product produces exactly the packed-fp32
// form with a cross-half second source that is wrong on gfx950 beside MFMA waves - and the correlation kernel puts MFMA
// waves on every CU.  The kernels of this file are therefore compiled without the packed-fp32 instructions.
#if defined(__HIP_DEVICE_COMPILE__)
#define HY_NO_PK __attribute__((target("no-packed-fp32-ops")))
#else
#define HY_NO_PK
#endif
#define HY_KERNEL __global__ HY_NO_PK
#define HY_HD __host__ __device__ inline HY_NO_PK

// ------------------------------------------------------------------------------------------------ singular vectors
// g / v: this lane's n x n complex matrices, element (r, c) re at [(2 (r n + c)) ld], im at [(2 (r n + c) + 1) ld]
HY_HD void hyb_svd_item(const HybArgs& a, int t, double* g, double* v, int ld) {
    const int nr = a.nr, nt = a.nt, ns = a.ns;
    const size_t n = (size_t)a.n;
    const int p = t / HY_N, k = t - p * HY_N;
    const size_t base = (size_t)p * nr * nt * HY_N + k;
#define HY_G(r, c, z) g[(size_t)(2 * ((r) * nr + (c)) + (z)) * ld]
#define HY_V(r, c, z) v[(size_t)(2 * ((r) * nr + (c)) + (z)) * ld]
    // G = H H^H (lower triangle computed, mirrored), V = I
    for (int r = 0; r < nr; ++r)
        for (int c = 0; c <= r; ++c) {
            const float* xr = a.h_re + base + (size_t)r * nt * HY_N;
            const float* xi = a.h_im + base + (size_t)r * nt * HY_N;
            const float* yr = a.h_re + base + (size_t)c * nt * HY_N;
            const float* yi = a.h_im + base + (size_t)c * nt * HY_N;
            double sr = 0.0, si = 0.0;
            for (int j = 0; j < nt; ++j) {
                const double ar = xr[(size_t)j * HY_N], ai = xi[(size_t)j * HY_N];
                const double br = yr[(size_t)j * HY_N], bi = yi[(size_t)j * HY_N];
                sr += ar * br + ai * bi;          // x conj(y)
                si += ai * br - ar * bi;
            }
            if (r == c) si = 0.0;
            HY_G(r, c, 0) = sr; HY_G(r, c, 1) = si;
            HY_G(c, r, 0) = sr; HY_G(c, r, 1) = -si;
            HY_V(r, c, 0) = r == c ? 1.0 : 0.0; HY_V(r, c, 1) = 0.0;
            HY_V(c, r, 0) = r == c ? 1.0 : 0.0; HY_V(c, r, 1) = 0.0;
        }
    for (int sweep = 0; sweep < HY_SWEEPS; ++sweep)
        for (int p0 = 0; p0 < nr - 1; ++p0)
            for (int q0 = p0 + 1; q0 < nr; ++q0) {
                const double gr = HY_G(p0, q0, 0), gi = HY_G(p0, q0, 1);
                const double r2 = gr * gr + gi * gi;
                const double al = HY_G(p0, p0, 0), be = HY_G(q0, q0, 0);
                if (!(r2 > 1e-36 * fabs(al * be)) || r2 < 1e-300) continue;
                const double r = sqrt(r2);
                const double wr = gr / r, wi = -gi / r;          // w = exp(-i arg g)
                const double th = (be - al) / (2.0 * r);
                const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
                // columns p0, q0 of G and of V:  x' = c x - s (y w),  y' = s x + c (y w)
                for (int i = 0; i < nr; ++i) {
                    double xr_ = HY_G(i, p0, 0), xi_ = HY_G(i, p0, 1), yr_ = HY_G(i, q0, 0), yi_ = HY_G(i, q0, 1);
                    double zr = yr_ * wr - yi_ * wi, zi = yr_ * wi + yi_ * wr;
                    HY_G(i, p0, 0) = cs * xr_ - sn * zr; HY_G(i, p0, 1) = cs * xi_ - sn * zi;
                    HY_G(i, q0, 0) = sn * xr_ + cs * zr; HY_G(i, q0, 1) = sn * xi_ + cs * zi;
                    xr_ = HY_V(i, p0, 0); xi_ = HY_V(i, p0, 1); yr_ = HY_V(i, q0, 0); yi_ = HY_V(i, q0, 1);
                    zr = yr_ * wr - yi_ * wi; zi = yr_ * wi + yi_ * wr;
                    HY_V(i, p0, 0) = cs * xr_ - sn * zr; HY_V(i, p0, 1) = cs * xi_ - sn * zi;
                    HY_V(i, q0, 0) = sn * xr_ + cs * zr; HY_V(i, q0, 1) = sn * xi_ + cs * zi;
                }
                // rows p0, q0 of G:  x' = c x - s (y conj w),  y' = s x + c (y conj w)
                for (int j = 0; j < nr; ++j) {
                    const double xr_ = HY_G(p0, j, 0), xi_ = HY_G(p0, j, 1), yr_ = HY_G(q0, j, 0), yi_ = HY_G(q0, j, 1);
                    const double zr = yr_ * wr + yi_ * wi, zi = yi_ * wr - yr_ * wi;
                    HY_G(p0, j, 0) = cs * xr_ - sn * zr; HY_G(p0, j, 1) = cs * xi_ - sn * zi;
                    HY_G(q0, j, 0) = sn * xr_ + cs * zr; HY_G(q0, j, 1) = sn * xi_ + cs * zi;
                }
                HY_G(p0, q0, 0) = 0.0; HY_G(p0, q0, 1) = 0.0;
                HY_G(q0, p0, 0) = 0.0; HY_G(q0, p0, 1) = 0.0;
                HY_G(p0, p0, 1) = 0.0; HY_G(q0, q0, 1) = 0.0;
            }
    // the ns largest eigenvalues, largest first, lowest index on a tie; Fopt[:, s] = H^H v_s / sigma_s
    unsigned used = 0;
    for (int s = 0; s < ns; ++s) {
        int sel = -1;
        double best = 0.0;
        for (int i = 0; i < nr; ++i) {
            if (used & (1u << i)) continue;
            const double lam = HY_G(i, i, 0);
            if (sel < 0 || lam > best) { sel = i; best = lam; }
        }
        used |= 1u << sel;
        const double inv = best > 0.0 ? 1.0 / sqrt(best) : 0.0;
        for (int j = 0; j < nt; ++j) {
            double sr = 0.0, si = 0.0;
            for (int i = 0; i < nr; ++i) {
                const size_t o = base + ((size_t)i * nt + j) * HY_N;
                const double hr = a.h_re[o], hi = a.h_im[o];
                const double ur = HY_V(i, sel, 0), ui = HY_V(i, sel, 1);
                sr += hr * ur + hi * ui;          // conj(h) u
                si += hr * ui - hi * ur;
            }
            const size_t o = ((size_t)s * nt + j) * n + t;
            const float fr = (float)(sr * inv), fi = (float)(si * inv);
            a.fopt_re[o] = fr; a.fopt_im[o] = fi;
            a.res_re[o] = fr; a.res_im[o] = fi;
        }
    }
#undef HY_G
#undef HY_V
    a.state[t] = 0;
    a.state[n + t] = 0;
}

HY_KERNEL void __launch_bounds__(HY_ITEM_THREADS) hyb_svd_kernel(HybArgs a, int tpb) {
    extern __shared__ double hy_lds[];
    const int t = blockIdx.x * tpb + threadIdx.x;
    if ((int)threadIdx.x >= tpb || t >= a.n) return;
    double* g = hy_lds + threadIdx.x;
    double* v = g + (size_t)2 * a.nr * a.nr * tpb;
    hyb_svd_item(a, t, g, v, tpb);
}

// ------------------------------------------------------------------------------------------------ correlation + argmax
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
HY_KERNEL void __launch_bounds__(HY_CORR_THREADS) hyb_corr_kernel(HybArgs a) {
    extern __shared__ float hy_tile[];          // [2][nt][32]
    const int nt = a.nt, ns = a.ns, rp = a.rp;
    const size_t n = (size_t)a.n;
    float* t_re = hy_tile;
    float* t_im = hy_tile + (size_t)nt * HY_RAY_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, h = lane >> 5;
    const int item = blockIdx.x * HY_CORR_ITEMS + wave * 32 + col;
    const bool valid = item < a.n;
    const size_t it = (size_t)(valid ? item : a.n - 1);          // lanes past the end repeat the last item and store nothing
    float best = -1.0f;
    int bidx = 0;
    for (int r0 = 0; r0 < rp; r0 += HY_RAY_TILE) {
        __syncthreads();
        for (int e = threadIdx.x; e < nt * HY_RAY_TILE; e += HY_CORR_THREADS) {
            const int j = e >> 5, r = e & 31;
            t_re[e] = a.at_re[(size_t)j * rp + r0 + r];
            t_im[e] = a.at_im[(size_t)j * rp + r0 + r];
        }
        __syncthreads();
        hy_f32x16 met;
        for (int v = 0; v < 16; ++v) met[v] = 0.0f;
        for (int s = 0; s < ns; ++s) {
            hy_f32x16 are, aim;
            for (int v = 0; v < 16; ++v) { are[v] = 0.0f; aim[v] = 0.0f; }
            const float* br = a.res_re + (size_t)s * nt * n + it;
            const float* bi = a.res_im + (size_t)s * nt * n + it;
            for (int j = 0; j < nt; j += 2) {
                const int jj = j + h;
                const bool in = jj < nt;
                const int jc = in ? jj : nt - 1;
                float ar = t_re[jc * HY_RAY_TILE + col], ai = t_im[jc * HY_RAY_TILE + col];
                float xr = br[(size_t)jc * n], xi = bi[(size_t)jc * n];
                if (!in) { ar = 0.0f; ai = 0.0f; xr = 0.0f; xi = 0.0f; }
                // psi = conj(at) res:  re = ar xr + ai xi,  im = ar xi - ai xr
                are = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, xr, are, 0, 0, 0);
                aim = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, xi, aim, 0, 0, 0);
                are = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, xi, are, 0, 0, 0);
                aim = __builtin_amdgcn_mfma_f32_32x32x2f32(-ai, xr, aim, 0, 0, 0);
            }
            for (int v = 0; v < 16; ++v) met[v] += are[v] * are[v] + aim[v] * aim[v];
        }
        // accumulator register v of this lane: ray r0 + 8 (v / 4) + 4 h + v % 4 (ascending in v), item = col
        for (int v = 0; v < 16; ++v) {
            const int ray = r0 + 8 * (v >> 2) + 4 * h + (v & 3);
            if (ray < a.rays && met[v] > best) { best = met[v]; bidx = ray; }
        }
    }
    const float ob = __shfl_xor(best, 32);
    const int oi = __shfl_xor(bidx, 32);
    if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    if (valid && h == 0) a.cand[item] = bidx;
}
#endif

// ------------------------------------------------------------------------------------------------ solve + residual
HY_HD void hyb_solve_item(const HybArgs& a, int t) {
    const int nt = a.nt, ns = a.ns, ntrf = a.ntrf, rp = a.rp, m = a.step;
    const size_t n = (size_t)a.n;
    int* idx = a.idx + (size_t)t * ntrf;
    if (a.state[n + t]) return;                  // finished at an earlier step: its outputs are complete
#define HY_L(r, c, z) a.chol[(size_t)(2 * ((r) * ((r) + 1) / 2 + (c)) + (z)) * n + t]
#define HY_Y(i, s, z) a.yv[(size_t)(2 * ((i) * ns + (s)) + (z)) * n + t]
#define HY_C(i, s, z) a.cv[(size_t)(2 * ((i) * ns + (s)) + (z)) * n + t]
    const int kn = a.cand[t];
    const float* nr_ = a.at_re + kn;
    const float* ni_ = a.at_im + kn;
    bool stop = false;
    int atoms = m + 1;
    // new row of the Cholesky factor of A^H A
    float dsum = 0.0f;
    for (int i = 0; i < m; ++i) {
        const int ki = idx[i];
        float gr = 0.0f, gi = 0.0f;              // a_m^H a_i
        for (int j = 0; j < nt; ++j) {
            const float xr = nr_[(size_t)j * rp], xi = ni_[(size_t)j * rp];
            const float yr = a.at_re[(size_t)j * rp + ki], yi = a.at_im[(size_t)j * rp + ki];
            gr += xr * yr + xi * yi;
            gi += xr * yi - xi * yr;
        }
        for (int q = 0; q < i; ++q) {            // - L_mq conj(L_iq)
            const float lr = HY_L(m, q, 0), li = HY_L(m, q, 1), kr = HY_L(i, q, 0), kq = HY_L(i, q, 1);
            gr -= lr * kr + li * kq;
            gi -= li * kr - lr * kq;
        }
        const float d = 1.0f / HY_L(i, i, 0);
        gr *= d; gi *= d;
        HY_L(m, i, 0) = gr; HY_L(m, i, 1) = gi;
        dsum += gr * gr + gi * gi;
    }
    float gmm = 0.0f;
    for (int j = 0; j < nt; ++j) {
        const float xr = nr_[(size_t)j * rp], xi = ni_[(size_t)j * rp];
        gmm += xr * xr + xi * xi;
    }
    const float piv = gmm - dsum;
    if (!(piv > 1e-6f * gmm)) {
        // the chosen column lies in the span of the earlier ones (or is zero): nothing left that the dictionary can add
        stop = true;
        atoms = m;
    } else {
        const float lmm = sqrtf(piv), dm = 1.0f / lmm;
        HY_L(m, m, 0) = lmm; HY_L(m, m, 1) = 0.0f;
        idx[m] = kn;
        // new row of y = L^-1 A^H Fopt
        for (int s = 0; s < ns; ++s) {
            float br = 0.0f, bi = 0.0f;          // a_m^H Fopt[:, s]
            for (int j = 0; j < nt; ++j) {
                const float xr = nr_[(size_t)j * rp], xi = ni_[(size_t)j * rp];
                const size_t o = ((size_t)s * nt + j) * n + t;
                const float fr = a.fopt_re[o], fi = a.fopt_im[o];
                br += xr * fr + xi * fi;
                bi += xr * fi - xi * fr;
            }
            for (int q = 0; q < m; ++q) {
                const float lr = HY_L(m, q, 0), li = HY_L(m, q, 1), yr = HY_Y(q, s, 0), yi = HY_Y(q, s, 1);
                br -= lr * yr - li * yi;
                bi -= lr * yi + li * yr;
            }
            HY_Y(m, s, 0) = br * dm; HY_Y(m, s, 1) = bi * dm;
        }
        // C = L^-H y
        for (int s = 0; s < ns; ++s)
            for (int i = m; i >= 0; --i) {
                float cr = HY_Y(i, s, 0), ci = HY_Y(i, s, 1);
                for (int q = i + 1; q <= m; ++q) {          // - conj(L_qi) C_q
                    const float lr = HY_L(q, i, 0), li = HY_L(q, i, 1), xr = HY_C(q, s, 0), xi = HY_C(q, s, 1);
                    cr -= lr * xr + li * xi;
                    ci -= lr * xi - li * xr;
                }
                const float d = 1.0f / HY_L(i, i, 0);
                HY_C(i, s, 0) = cr * d; HY_C(i, s, 1) = ci * d;
            }
    }
    // T = Fopt - A C (kept in the residual planes), e = |T|_F, |A C|_F
    float e2 = 0.0f, ac2 = 0.0f;
    for (int s = 0; s < ns; ++s)
        for (int j = 0; j < nt; ++j) {
            float pr = 0.0f, pi = 0.0f;
            for (int i = 0; i < atoms; ++i) {
                const int ki = idx[i];
                const float xr = a.at_re[(size_t)j * rp + ki], xi = a.at_im[(size_t)j * rp + ki];
                const float cr = HY_C(i, s, 0), ci = HY_C(i, s, 1);
                pr += xr * cr - xi * ci;
                pi += xr * ci + xi * cr;
            }
            const size_t o = ((size_t)s * nt + j) * n + t;
            const float tr = a.fopt_re[o] - pr, ti = a.fopt_im[o] - pi;
            a.res_re[o] = tr; a.res_im[o] = ti;
            e2 += tr * tr + ti * ti;
            ac2 += pr * pr + pi * pi;
        }
    const float e = sqrtf(e2);
    if (e <= a.stop_tol || m == ntrf - 1) stop = true;
    if (!stop) {
        const float inv = 1.0f / e;
        for (int s = 0; s < ns; ++s)
            for (int j = 0; j < nt; ++j) {
                const size_t o = ((size_t)s * nt + j) * n + t;
                a.res_re[o] *= inv; a.res_im[o] *= inv;
            }
        a.state[t] = atoms;
        return;
    }
    // last step of this item: Fbb = sqrt(ns) C / |A C|_F; the residual planes receive the full-band weights A Fbb
    const float scale = ac2 > 0.0f ? sqrtf((float)ns / ac2) : 0.0f;
    for (int s = 0; s < ns; ++s) {
        for (int j = 0; j < nt; ++j) {
            const size_t o = ((size_t)s * nt + j) * n + t;
            a.res_re[o] = (a.fopt_re[o] - a.res_re[o]) * scale;
            a.res_im[o] = (a.fopt_im[o] - a.res_im[o]) * scale;
        }
        for (int i = 0; i < ntrf; ++i) {
            const size_t o = ((size_t)t * ns + s) * ntrf + i;
            a.fbb_re[o] = i < atoms ? HY_C(i, s, 0) * scale : 0.0f;
            a.fbb_im[o] = i < atoms ? HY_C(i, s, 1) * scale : 0.0f;
        }
    }
    for (int i = atoms; i < ntrf; ++i) idx[i] = -1;
    if (a.n_atoms) a.n_atoms[t] = atoms;
    a.state[t] = atoms;
    a.state[n + t] = 1;
#undef HY_L
#undef HY_Y
#undef HY_C
}

HY_KERNEL void __launch_bounds__(HY_ITEM_THREADS) hyb_solve_kernel(HybArgs a) {
    const int t = blockIdx.x * HY_ITEM_THREADS + threadIdx.x;
    if (t < a.n) hyb_solve_item(a, t);
}

// gain = |H_eval W|_F^2 with W = A Fbb from the residual planes
HY_HD void hyb_gain_item(const HybArgs& a, int t) {
    const int nt = a.nt, nr = a.nr, ns = a.ns;
    const size_t n = (size_t)a.n;
    const int p = t / HY_N, k = t - p * HY_N;
    const size_t base = (size_t)p * nr * nt * HY_N + k;
    float g = 0.0f;
    for (int i = 0; i < nr; ++i)
        for (int s = 0; s < ns; ++s) {
            float sr = 0.0f, si = 0.0f;
            for (int j = 0; j < nt; ++j) {
                const size_t oh = base + ((size_t)i * nt + j) * HY_N, ow = ((size_t)s * nt + j) * n + t;
                const float hr = a.e_re[oh], hi = a.e_im[oh], wr = a.res_re[ow], wi = a.res_im[ow];
                sr += hr * wr - hi * wi;
                si += hr * wi + hi * wr;
            }
            g += sr * sr + si * si;
        }
    a.gain[t] = g;
}

HY_KERNEL void __launch_bounds__(HY_ITEM_THREADS) hyb_gain_kernel(HybArgs a) {
    const int t = blockIdx.x * HY_ITEM_THREADS + threadIdx.x;
    if (t < a.n) hyb_gain_item(a, t);
}

// frf_mean[p][m][j] = mean over the 234 subcarriers of At[j][idx[p][k][m]] (a slot that an early stop left empty adds nothing);
// one thread per output, fixed order, fp64 sum
HY_HD void hyb_frf_mean_item(const HybArgs& a, int64_t o, float* out_re, float* out_im) {
    const int nt = a.nt, ntrf = a.ntrf;
    const int j = (int)(o % nt);
    const int m = (int)((o / nt) % ntrf);
    const int64_t p = o / ((int64_t)nt * ntrf);
    double sr = 0.0, si = 0.0;
    for (int k = 0; k < HY_N; ++k) {
        const int ki = a.idx[((size_t)p * HY_N + k) * ntrf + m];
        if (ki < 0) continue;
        sr += a.at_re[(size_t)j * a.rp + ki];
        si += a.at_im[(size_t)j * a.rp + ki];
    }
    out_re[o] = (float)(sr / HY_N);
    out_im[o] = (float)(si / HY_N);
}

HY_KERNEL void __launch_bounds__(256) hyb_frf_mean_kernel(HybArgs a, int64_t total, float* out_re, float* out_im) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o < total) hyb_frf_mean_item(a, o, out_re, out_im);
}

}  // namespace csi
