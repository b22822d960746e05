// rx_combine.hip.h - receive combining: the U^H combiner of a user's CSI estimate and its application to CSI planes.
//
// One item = one (packet, carrier); H[i][j] = h[p][i][j][k] is Nr x Nt.  Per item:
//   C [ns][Nr]   row s = exp(i t_s) u_s^H, u_s the left singular vector of the s-th largest singular value (largest first, the lowest
//                index on a tie: the selection rule of hyb_svd_item, hybrid_weights.hip.h); t_s makes (C H)[s][Nt-1] real and >= 0 (no
//                rotation when that element is 0) - the column phase of the feedback report (feedback.hip.h), so that
//                conj((C H)[s][:]) / sigma_s is its d_v and C H what CSI_FB_LAYOUT_CSI expands to at continuous angles
//   rank rule    a row whose eigenvalue lambda_s of H H^H is not > 0, not finite or not > 2^-40 lambda_1 (sigma_s not > 2^-20 sigma_1) is
//                all zero and its sigma is 0.  The floor: Jacobi leaves the zero eigenvalues of a rank-deficient matrix as rounding
//                noise of either sign (about Nr 2^-50 lambda_1); "> 0" alone would pass the positive half of them as rows.
//   E = C H      rows s < ns: E[s][j] = sum_i C[s][i] H[i][j], i ascending, fmaf chains; rows >= ns exact zeros (the CSI layout)
// The rows of C are orthonormal, so C w of white noise w is white with the same variance: the data phase (mu_link.hip.h) handed E_u = C_u H_u
// as the user's channel draws exactly the noise a combining receiver sees.  A combiner with other rows would colour it: not modelled.
// Plan:
//   * rx_combiner_kernel: one lane per item, lane = carrier, so the [p][i][j][k] planes are read and C is stored along k.  The Nr x Nr
//     Gram matrix and its eigenvectors live in LDS as [element][lane] in fp64 (cyclic Jacobi, HY_SWEEPS sweeps: the decomposition of
//     hyb_svd_item stated again, operation by operation, because that function also writes Fopt = H^H u / sigma into a workspace this
//     kernel has no use for - so there is no workspace, no chunking against it and nothing to grow under a capture).  The phase factor
//     and the rows are formed in fp64 and rounded once.
//   * rx_apply_kernel<NS, REG>: streaming, one launch, one workgroup of 64 lanes per (packet, 64 carriers).  C of the item sits in
//     registers when ns Nr <= 16 (REG; the loops over Nr are unrolled to the capacity 16 / NS with a uniform bound), else in LDS as
//     [element][lane].  Every access runs along k with unit stride.  (A row of 234 floats is 936 bytes = 8 mod 16: every second row of a
//     plane starts off a 16-byte boundary, so the planes move as 4-byte words per lane, 256 bytes per wave and access.)
// re and im stay in separate registers and planes; no packed fp32 (HY_NO_PK), no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "hybrid_weights.hip.h"

namespace csi {

constexpr int RXC_MAX_NS = 4;
constexpr int RXC_THREADS = 64;            // lanes per workgroup at the most
constexpr int RXC_REG_ELEMS = 16;          // ns Nr up to which the apply kernel keeps C in registers
constexpr size_t RXC_MAX_LDS = 160 * 1024;
constexpr double RXC_RANK_FLOOR = 9.094947017729282e-13;      // 2^-40: lambda_s / lambda_1 at or below which a row is rank noise

struct RxCombinerArgs {
    const float* h_re;      // CSI planes of the launch [pkts][nr][nt][234]
    const float* h_im;
    float* c_re;            // [pkts][ns][nr][234]
    float* c_im;
    float* sigma;           // [pkts][ns][234] or null
    int nt, nr, ns;
    int n;                  // items of the launch (packets x 234)
};

struct RxApplyArgs {
    const float* c_re;      // [npkt][ns][nr][234]
    const float* c_im;
    const float* h_re;      // [npkt][nr][nt][234]
    const float* h_im;
    float* e_re;            // [npkt][nr][nt][234]
    float* e_im;
    int nt, nr, ns;
    int tiles;              // workgroups per packet
};

// one item: t = (packet, carrier) of the launch; g, v: this lane's LDS columns, element (r, c) re at [(2 (r nr + c)) ld], im one plane behind
HY_HD void rx_combiner_item(const RxCombinerArgs& a, int t, double* g, double* v, int ld) {
    const int nr = a.nr, nt = a.nt, ns = a.ns;
    const int p = t / HY_N, k = t - p * HY_N;
    const size_t base = (size_t)p * nr * nt * HY_N + k;
#define RXC_G(r, c, z) g[(size_t)(2 * ((r) * nr + (c)) + (z)) * ld]
#define RXC_V(r, c, z) v[(size_t)(2 * ((r) * nr + (c)) + (z)) * ld]
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
            RXC_G(r, c, 0) = sr; RXC_G(r, c, 1) = si;
            RXC_G(c, r, 0) = sr; RXC_G(c, r, 1) = -si;
            RXC_V(r, c, 0) = r == c ? 1.0 : 0.0; RXC_V(r, c, 1) = 0.0;
            RXC_V(c, r, 0) = r == c ? 1.0 : 0.0; RXC_V(c, r, 1) = 0.0;
        }
    // cyclic Jacobi on G, the rotations gathered in V: G = V diag(lambda) V^H
    for (int sweep = 0; sweep < HY_SWEEPS; ++sweep)
        for (int p0 = 0; p0 < nr - 1; ++p0)
            for (int q0 = p0 + 1; q0 < nr; ++q0) {
                const double gr = RXC_G(p0, q0, 0), gi = RXC_G(p0, q0, 1);
                const double r2 = gr * gr + gi * gi;
                const double al = RXC_G(p0, p0, 0), be = RXC_G(q0, q0, 0);
                if (!(r2 > 1e-36 * fabs(al * be)) || r2 < 1e-300) continue;
                const double r = sqrt(r2);
                const double wr = gr / r, wi = -gi / r;          // w = exp(-i arg g)
                const double th = (be - al) / (2.0 * r);
                const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
                // columns p0, q0 of G and of V:  x' = c x - s (y w),  y' = s x + c (y w)
                for (int i = 0; i < nr; ++i) {
                    double xr_ = RXC_G(i, p0, 0), xi_ = RXC_G(i, p0, 1), yr_ = RXC_G(i, q0, 0), yi_ = RXC_G(i, q0, 1);
                    double zr = yr_ * wr - yi_ * wi, zi = yr_ * wi + yi_ * wr;
                    RXC_G(i, p0, 0) = cs * xr_ - sn * zr; RXC_G(i, p0, 1) = cs * xi_ - sn * zi;
                    RXC_G(i, q0, 0) = sn * xr_ + cs * zr; RXC_G(i, q0, 1) = sn * xi_ + cs * zi;
                    xr_ = RXC_V(i, p0, 0); xi_ = RXC_V(i, p0, 1); yr_ = RXC_V(i, q0, 0); yi_ = RXC_V(i, q0, 1);
                    zr = yr_ * wr - yi_ * wi; zi = yr_ * wi + yi_ * wr;
                    RXC_V(i, p0, 0) = cs * xr_ - sn * zr; RXC_V(i, p0, 1) = cs * xi_ - sn * zi;
                    RXC_V(i, q0, 0) = sn * xr_ + cs * zr; RXC_V(i, q0, 1) = sn * xi_ + cs * zi;
                }
                // rows p0, q0 of G:  x' = c x - s (y conj w),  y' = s x + c (y conj w)
                for (int j = 0; j < nr; ++j) {
                    const double xr_ = RXC_G(p0, j, 0), xi_ = RXC_G(p0, j, 1), yr_ = RXC_G(q0, j, 0), yi_ = RXC_G(q0, j, 1);
                    const double zr = yr_ * wr + yi_ * wi, zi = yi_ * wr - yr_ * wi;
                    RXC_G(p0, j, 0) = cs * xr_ - sn * zr; RXC_G(p0, j, 1) = cs * xi_ - sn * zi;
                    RXC_G(q0, j, 0) = sn * xr_ + cs * zr; RXC_G(q0, j, 1) = sn * xi_ + cs * zi;
                }
                RXC_G(p0, q0, 0) = 0.0; RXC_G(p0, q0, 1) = 0.0;
                RXC_G(q0, p0, 0) = 0.0; RXC_G(q0, p0, 1) = 0.0;
                RXC_G(p0, p0, 1) = 0.0; RXC_G(q0, q0, 1) = 0.0;
            }
    // the ns largest eigenvalues, largest first, lowest index on a tie; row s = exp(i t_s) u_s^H
    unsigned used = 0;
    double first = 0.0;
    for (int s = 0; s < ns; ++s) {
        int sel = -1;
        double best = 0.0;
        for (int i = 0; i < nr; ++i) {
            if (used & (1u << i)) continue;
            const double lam = RXC_G(i, i, 0);
            if (sel < 0 || lam > best) { sel = i; best = lam; }
        }
        used |= 1u << sel;
        if (s == 0) first = best;
        // (a comparison with NaN is false, and an infinite lambda_1 lets no row through: both give the zero row)
        const bool live = best > 0.0 && best > RXC_RANK_FLOOR * first && first < (double)INFINITY;
        // z = (u_s^H H)[Nt-1]; the row is conj(z) / |z| times u_s^H
        double zr = 0.0, zi = 0.0;
        for (int i = 0; i < nr; ++i) {
            const size_t o = base + ((size_t)i * nt + (nt - 1)) * HY_N;
            const double hr = a.h_re[o], hi = a.h_im[o];
            const double ur = RXC_V(i, sel, 0), ui = RXC_V(i, sel, 1);
            zr += ur * hr + ui * hi;          // conj(u) h
            zi += ur * hi - ui * hr;
        }
        const double m = sqrt(zr * zr + zi * zi);
        const bool turn = m > 0.0 && m < (double)INFINITY;
        const double fr = turn ? zr / m : 1.0, fi = turn ? -zi / m : 0.0;
        for (int i = 0; i < nr; ++i) {
            const double ur = RXC_V(i, sel, 0), ui = RXC_V(i, sel, 1);
            const size_t o = (((size_t)p * ns + s) * nr + i) * HY_N + k;
            a.c_re[o] = live ? (float)(fr * ur + fi * ui) : 0.0f;          // f conj(u)
            a.c_im[o] = live ? (float)(fi * ur - fr * ui) : 0.0f;
        }
        if (a.sigma) a.sigma[((size_t)p * ns + s) * HY_N + k] = live ? (float)sqrt(best) : 0.0f;
    }
#undef RXC_G
#undef RXC_V
}

// (templates, like the kernels of feedback.hip.h: instantiated behind every earlier kernel of the library, whose code then keeps its place)
template <int THREADS>
HY_KERNEL void __launch_bounds__(THREADS) rx_combiner_kernel(RxCombinerArgs a, int tpb) {
    extern __shared__ double rxc_lds[];
    const int t = blockIdx.x * tpb + threadIdx.x;
    if ((int)threadIdx.x >= tpb || t >= a.n) return;
    // per lane 4 nr^2 doubles: g, then v
    double* g = rxc_lds + threadIdx.x;
    double* v = g + (size_t)2 * a.nr * a.nr * tpb;
    rx_combiner_item(a, t, g, v, tpb);
}

// REG: C of the item in registers, NS x CAP with CAP = 16 / NS >= nr; otherwise in LDS, element (s, i) re at [(s nr + i) 64 + lane], im
// ns nr planes behind.  Both run the same fmaf chains: the same bits.
template <int NS, bool REG>
HY_KERNEL void __launch_bounds__(RXC_THREADS) rx_apply_kernel(RxApplyArgs a) {
    extern __shared__ float rxa_lds[];
    constexpr int CAP = REG ? RXC_REG_ELEMS / NS : 1;
    const int nt = a.nt, nr = a.nr;
    const int p = blockIdx.x / a.tiles, tile = blockIdx.x - p * a.tiles;
    const int k = tile * RXC_THREADS + threadIdx.x;
    if (k >= HY_N) return;
    const float* c_re = a.c_re + (size_t)p * NS * nr * HY_N + k;
    const float* c_im = a.c_im + (size_t)p * NS * nr * HY_N + k;
    const size_t base = (size_t)p * nr * nt * HY_N + k;
    float cr[NS][CAP], ci[NS][CAP];
    float* l_re = rxa_lds + threadIdx.x;
    float* l_im = l_re + (size_t)NS * nr * RXC_THREADS;
    if (REG) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int i = 0; i < CAP; ++i) {
                cr[s][i] = i < nr ? c_re[(size_t)(s * nr + i) * HY_N] : 0.0f;
                ci[s][i] = i < nr ? c_im[(size_t)(s * nr + i) * HY_N] : 0.0f;
            }
    } else {
        // a lane reads back only what it wrote itself: no barrier
        for (int e = 0; e < NS * nr; ++e) {
            l_re[(size_t)e * RXC_THREADS] = c_re[(size_t)e * HY_N];
            l_im[(size_t)e * RXC_THREADS] = c_im[(size_t)e * HY_N];
        }
    }
    for (int j = 0; j < nt; ++j) {
        float er[NS], ei[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) { er[s] = 0.0f; ei[s] = 0.0f; }
        if (REG) {
#pragma unroll
            for (int i = 0; i < CAP; ++i)
                if (i < nr) {
                    const size_t o = base + ((size_t)i * nt + j) * HY_N;
                    const float hr = a.h_re[o], hi = a.h_im[o];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        er[s] = fmaf(cr[s][i], hr, er[s]); er[s] = fmaf(-ci[s][i], hi, er[s]);
                        ei[s] = fmaf(cr[s][i], hi, ei[s]); ei[s] = fmaf(ci[s][i], hr, ei[s]);
                    }
                }
        } else {
            for (int i = 0; i < nr; ++i) {
                const size_t o = base + ((size_t)i * nt + j) * HY_N;
                const float hr = a.h_re[o], hi = a.h_im[o];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const float xr = l_re[(size_t)(s * nr + i) * RXC_THREADS], xi = l_im[(size_t)(s * nr + i) * RXC_THREADS];
                    er[s] = fmaf(xr, hr, er[s]); er[s] = fmaf(-xi, hi, er[s]);
                    ei[s] = fmaf(xr, hi, ei[s]); ei[s] = fmaf(xi, hr, ei[s]);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const size_t o = base + ((size_t)s * nt + j) * HY_N;
            a.e_re[o] = er[s]; a.e_im[o] = ei[s];
        }
        for (int s = NS; s < nr; ++s) {
            const size_t o = base + ((size_t)s * nt + j) * HY_N;
            a.e_re[o] = 0.0f; a.e_im[o] = 0.0f;
        }
    }
}

}  // namespace csi
