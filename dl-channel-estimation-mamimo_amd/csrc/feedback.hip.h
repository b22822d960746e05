// feedback.hip.h - quantised CSI feedback: the Givens-angle report of a CSI tensor and its expansion.
//
// The definition is IEEE 802.11-2016 19.3.12.3.6 (the compressed beamforming report) with Nt rows.  One report = one (packet, reported
// carrier); reported carriers are k_r = r ng, r < n_rep = ceil(234 / ng), and carrier k is served by report k / ng.  Per report:
//   V [Nt][nc]  = the nc dominant right singular vectors of H, exactly the Fopt of hyb_svd_item (hybrid_weights.hip.h)
//   column s   *= exp(-j arg V[Nt-1][s])                                  the last row real and >= 0
//   for i < min(nc, Nt-1):  phi[l][i] = arg V[l][i], l = i .. Nt-2, row l *= exp(-j phi[l][i])
//                           psi[l][i] = atan2(Re V[l][i], Re V[i][i]), l = i+1 .. Nt-1, rows (i, l) <- (c x_i + s x_l, -s x_i + c x_l)
//   codes: k_phi = floor(phi 2^(b_phi-1) / pi) mod 2^b_phi,  k_psi = min(floor(psi 2^(b_psi+1) / pi), 2^b_psi - 1)
// The expansion runs the steps backwards on the first nc columns of the identity with the cos / sin of the bin centres.
// Plan:
//   * fb_compress_kernel: one lane per report, so the [p][i][j][k] planes are read along k.  hyb_svd_item runs unchanged on a HybArgs
//     whose residual planes alias the Fopt planes; its pointers are shifted per lane so that the item number it derives (p 234 + k_r)
//     lands on this lane's slot of the [s][j][report] workspace.  Its fp64 matrices live in LDS, [element][lane]; the singular values
//     are read off the diagonal it leaves there by its own selection rule.  The Nt x nc matrix is then taken into the SAME LDS slots
//     (a lane's 8-byte slot holds re and im of one element, so no lane ever touches another lane's bytes and no barrier is needed) and
//     decomposed there: a row operation acts on every column on its own, so stage i only visits the columns s >= i - the others can no
//     longer reach an angle.  Phases and rotations use c, s from hypotf; atan2f appears only where an angle is reported.
//   * fb_expand_kernel: one lane per carrier, one workgroup per (packet, tile of carriers).  The cos / sin tables of the bin centres
//     (computed on the host in double) are staged in LDS, the matrix lives in LDS as [element][lane] planes, and both output layouts
//     are written with unit stride over the carriers.  With continuous angles the tables are replaced by sincosf.
// re and im stay in separate registers and planes; no packed fp32 (HY_NO_PK), no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "hybrid_weights.hip.h"

namespace csi {

constexpr int FB_MAX_NC = 4;
constexpr int FB_THREADS = 64;             // lanes per workgroup at the most
constexpr int FB_MIN_BPHI = 2, FB_MAX_BPHI = 10;
constexpr int FB_MIN_BPSI = 1, FB_MAX_BPSI = 8;
constexpr int FB_LAYOUT_W = 0, FB_LAYOUT_CSI = 1;
constexpr size_t FB_MAX_LDS = 160 * 1024;
constexpr float FB_TWO_PI = 6.28318530717958647692f;
constexpr float FB_HALF_PI = 1.57079632679489661923f;

struct FbCompressArgs {
    const float* h_re;      // CSI planes of the chunk [pkts][nr][nt][234]
    const float* h_im;
    float* ws_re;           // workspace [nc][nt][n]: the singular vectors as hyb_svd_item leaves them
    float* ws_im;
    int* ws_state;          // workspace [2][n]: hyb_svd_item's per-item state words
    uint16_t* phi_code;     // [pkts][n_ang][n_rep] or null
    uint16_t* psi_code;
    float* phi;             // [pkts][n_ang][n_rep] or null
    float* psi;
    float* sigma;           // [pkts][nc][n_rep] or null
    float* v_re;            // [pkts][nc][nt][n_rep] or null
    float* v_im;
    int nt, nr, nc, ng, n_rep, n_ang;
    int n;                  // reports of the chunk (packets x n_rep)
    int b_phi, b_psi;       // 0, 0: continuous angles only
    float phi_scale;        // 2^(b_phi-1) / pi
    float psi_scale;        // 2^(b_psi+1) / pi
};

struct FbExpandArgs {
    const uint16_t* phi_code;   // [pkts][n_ang][n_rep], or null with the continuous pair
    const uint16_t* psi_code;
    const float* phi;
    const float* psi;
    const float* sigma;     // [pkts][nc][n_rep] or null
    const float* tab;       // device tables: cos phi [2^b_phi], sin phi, cos psi [2^b_psi], sin psi
    float* out_re;
    float* out_im;
    int nt, nr, nc, ng, n_rep, n_ang;
    int b_phi, b_psi;
    int layout;
    int tiles;              // workgroups per packet
    float scale;            // sqrt(Nt / nc)
};

typedef float __attribute__((may_alias)) fb_f32_lds;      // floats laid over the LDS slots the fp64 step used

// the number of angles of each kind
__host__ __device__ inline int fb_n_angles(int nt, int nc) {
    const int m = nc < nt - 1 ? nc : nt - 1;
    return m * (nt - 1) - m * (m - 1) / 2;
}

HY_HD void fb_unit(float re, float im, float* m, float* cr, float* ci) {
    const float h = hypotf(re, im);
    *m = h;
    if (h > 0.0f) { *cr = re / h; *ci = im / h; }
    else { *cr = 1.0f; *ci = 0.0f; }
}

// one report: t = (packet, reported carrier) of the chunk; g, v: this lane's LDS columns of hyb_svd_item (stride ld doubles)
HY_HD void fb_compress_item(const FbCompressArgs& a, int t, double* g, double* v, int ld) {
    const int nt = a.nt, nr = a.nr, nc = a.nc, n_rep = a.n_rep;
    const size_t n = (size_t)a.n;
    const int p = t / n_rep, r = t - p * n_rep;
    const int item = p * HY_N + r * a.ng;                      // what hyb_svd_item takes for (packet, carrier)
    const ptrdiff_t shift = (ptrdiff_t)t - (ptrdiff_t)item;    // its slot [.. n + item] is this lane's slot [.. n + t]
    HybArgs ha{};
    ha.h_re = a.h_re; ha.h_im = a.h_im;
    ha.fopt_re = a.ws_re + shift; ha.fopt_im = a.ws_im + shift;
    ha.res_re = ha.fopt_re; ha.res_im = ha.fopt_im;
    ha.state = a.ws_state + shift;
    ha.nt = nt; ha.nr = nr; ha.ns = nc; ha.n = a.n;
    hyb_svd_item(ha, item, g, v, ld);
    // the singular values, by the selection rule of hyb_svd_item on the diagonal it left
    if (a.sigma) {
        unsigned used = 0;
        for (int s = 0; s < nc; ++s) {
            int sel = -1;
            double best = 0.0;
            for (int i = 0; i < nr; ++i) {
                if (used & (1u << i)) continue;
                const double lam = g[(size_t)(2 * (i * nr + i)) * ld];
                if (sel < 0 || lam > best) { sel = i; best = lam; }
            }
            used |= 1u << sel;
            a.sigma[((size_t)p * nc + s) * n_rep + r] = best > 0.0 ? (float)sqrt(best) : 0.0f;
        }
    }
    // the matrix into this lane's 8-byte slots: element (j, s) re at m[2 ((s nt + j) ld)], im one float behind
    fb_f32_lds* m = reinterpret_cast<fb_f32_lds*>(g);
#define FB_M(j, s, z) m[(size_t)((s) * nt + (j)) * ld * 2 + (z)]
    for (int s = 0; s < nc; ++s) {
        // column phase: the last row real and >= 0
        const size_t ol = ((size_t)s * nt + (nt - 1)) * n + t;
        float hm, cr, ci;
        fb_unit(a.ws_re[ol], a.ws_im[ol], &hm, &cr, &ci);
        for (int j = 0; j < nt; ++j) {
            const size_t o = ((size_t)s * nt + j) * n + t;
            const float xr = a.ws_re[o], xi = a.ws_im[o];
            float yr = xr * cr + xi * ci, yi = xi * cr - xr * ci;          // x conj(u)
            if (j == nt - 1) { yr = hm; yi = 0.0f; }
            FB_M(j, s, 0) = yr; FB_M(j, s, 1) = yi;
            if (a.v_re) {
                const size_t ov = (((size_t)p * nc + s) * nt + j) * n_rep + r;
                a.v_re[ov] = yr; a.v_im[ov] = yi;
            }
        }
    }
    const int stages = nc < nt - 1 ? nc : nt - 1;
    const int qphi_mask = (1 << a.b_phi) - 1, qpsi_max = (1 << a.b_psi) - 1;
    const size_t ang0 = (size_t)p * a.n_ang * n_rep + r;
    int off = 0;
    for (int i = 0; i < stages; ++i) {
        for (int l = i; l < nt - 1; ++l) {
            const float xr = FB_M(l, i, 0), xi = FB_M(l, i, 1);
            float hm, cr, ci;
            fb_unit(xr, xi, &hm, &cr, &ci);
            float ph = hm > 0.0f ? atan2f(xi, xr) : 0.0f;
            if (ph < 0.0f) ph += FB_TWO_PI;
            if (!(ph < FB_TWO_PI)) ph = 0.0f;
            const size_t oa = ang0 + (size_t)(off + l - i) * n_rep;
            if (a.phi) a.phi[oa] = ph;
            if (a.b_phi) a.phi_code[oa] = (uint16_t)((int)floorf(ph * a.phi_scale) & qphi_mask);
            FB_M(l, i, 0) = hm; FB_M(l, i, 1) = 0.0f;
            for (int s = i + 1; s < nc; ++s) {
                const float yr = FB_M(l, s, 0), yi = FB_M(l, s, 1);
                FB_M(l, s, 0) = yr * cr + yi * ci;
                FB_M(l, s, 1) = yi * cr - yr * ci;
            }
        }
        for (int l = i + 1; l < nt; ++l) {
            const float ar = FB_M(i, i, 0), br = FB_M(l, i, 0);
            const float h = hypotf(ar, br);
            const float cs = h > 0.0f ? ar / h : 1.0f, sn = h > 0.0f ? br / h : 0.0f;
            float ps = atan2f(br, ar);
            ps = ps < 0.0f ? 0.0f : (ps > FB_HALF_PI ? FB_HALF_PI : ps);
            const size_t oa = ang0 + (size_t)(off + l - i - 1) * n_rep;
            if (a.psi) a.psi[oa] = ps;
            if (a.b_psi) {
                const int q = (int)floorf(ps * a.psi_scale);
                a.psi_code[oa] = (uint16_t)(q < qpsi_max ? q : qpsi_max);
            }
            for (int s = i; s < nc; ++s)
                for (int z = 0; z < 2; ++z) {
                    const float xi_ = FB_M(i, s, z), xl = FB_M(l, s, z);
                    FB_M(i, s, z) = cs * xi_ + sn * xl;
                    FB_M(l, s, z) = cs * xl - sn * xi_;
                }
        }
        off += nt - 1 - i;
    }
#undef FB_M
}

// (templates, like the kernels of mu_jsdm.hip.h: instantiated behind every earlier kernel of the library, whose code then keeps its place)
template <int THREADS>
HY_KERNEL void __launch_bounds__(THREADS) fb_compress_kernel(FbCompressArgs a, int tpb) {
    extern __shared__ double fb_lds[];
    const int t = blockIdx.x * tpb + threadIdx.x;
    if ((int)threadIdx.x >= tpb || t >= a.n) return;
    // per lane max(4 nr^2, nt nc) doubles: g and v of the singular-vector step, then the matrix
    double* g = fb_lds + threadIdx.x;
    double* v = g + (size_t)2 * a.nr * a.nr * tpb;
    fb_compress_item(a, t, g, v, tpb);
}

// one carrier: (p, k) of the call; m_re / m_im: this lane's LDS columns, element (j, s) at [(s nt + j) ld]; the tables in LDS
HY_HD void fb_expand_item(const FbExpandArgs& a, int p, int k, float* m_re, float* m_im, int ld, const float* tab) {
    const int nt = a.nt, nc = a.nc, n_rep = a.n_rep;
    const int r = k / a.ng;
#define FB_R(j, s) m_re[(size_t)((s) * nt + (j)) * ld]
#define FB_I(j, s) m_im[(size_t)((s) * nt + (j)) * ld]
    for (int s = 0; s < nc; ++s)
        for (int j = 0; j < nt; ++j) { FB_R(j, s) = j == s ? 1.0f : 0.0f; FB_I(j, s) = 0.0f; }
    const int stages = nc < nt - 1 ? nc : nt - 1;
    const float* cphi = tab;
    const float* sphi = cphi + ((size_t)1 << a.b_phi);
    const float* cpsi = sphi + ((size_t)1 << a.b_phi);
    const float* spsi = cpsi + ((size_t)1 << a.b_psi);
    const size_t ang0 = (size_t)p * a.n_ang * n_rep + r;
    int off = a.n_ang;
    for (int i = stages - 1; i >= 0; --i) {
        off -= nt - 1 - i;
        for (int l = nt - 1; l > i; --l) {
            const size_t oa = ang0 + (size_t)(off + l - i - 1) * n_rep;
            float cs, sn;
            if (a.psi_code) { const int q = a.psi_code[oa]; cs = cpsi[q]; sn = spsi[q]; }
            else sincosf(a.psi[oa], &sn, &cs);
            for (int s = i; s < nc; ++s) {
                const float xr = FB_R(i, s), xl = FB_R(l, s), yr = FB_I(i, s), yl = FB_I(l, s);
                FB_R(i, s) = cs * xr - sn * xl; FB_R(l, s) = sn * xr + cs * xl;
                FB_I(i, s) = cs * yr - sn * yl; FB_I(l, s) = sn * yr + cs * yl;
            }
        }
        for (int l = i; l < nt - 1; ++l) {
            const size_t oa = ang0 + (size_t)(off + l - i) * n_rep;
            float cs, sn;
            if (a.phi_code) { const int q = a.phi_code[oa]; cs = cphi[q]; sn = sphi[q]; }
            else sincosf(a.phi[oa], &sn, &cs);
            for (int s = i; s < nc; ++s) {
                const float xr = FB_R(l, s), xi = FB_I(l, s);
                FB_R(l, s) = xr * cs - xi * sn;
                FB_I(l, s) = xr * sn + xi * cs;
            }
        }
    }
    if (a.layout == FB_LAYOUT_W) {
        for (int s = 0; s < nc; ++s)
            for (int j = 0; j < nt; ++j) {
                const size_t o = (((size_t)p * nc + s) * nt + j) * HY_N + k;
                a.out_re[o] = a.scale * FB_R(j, s);
                a.out_im[o] = a.scale * FB_I(j, s);
            }
    } else {
        for (int s = 0; s < a.nr; ++s) {
            const float sg = s < nc ? (a.sigma ? a.sigma[((size_t)p * nc + s) * n_rep + r] : 1.0f) : 0.0f;
            for (int j = 0; j < nt; ++j) {
                const size_t o = (((size_t)p * a.nr + s) * nt + j) * HY_N + k;
                a.out_re[o] = s < nc ? sg * FB_R(j, s) : 0.0f;
                a.out_im[o] = s < nc ? -(sg * FB_I(j, s)) : 0.0f;
            }
        }
    }
#undef FB_R
#undef FB_I
}

template <int THREADS>
HY_KERNEL void __launch_bounds__(THREADS) fb_expand_kernel(FbExpandArgs a, int tpb, int n_tab) {
    extern __shared__ float fb_lds_f[];
    float* tab = fb_lds_f;                                  // n_tab floats (0 with continuous angles)
    for (int e = threadIdx.x; e < n_tab; e += blockDim.x) tab[e] = a.tab[e];
    __syncthreads();
    const int p = blockIdx.x / a.tiles, tile = blockIdx.x - p * a.tiles;
    const int k = tile * tpb + threadIdx.x;
    if ((int)threadIdx.x >= tpb || k >= HY_N) return;
    float* m_re = tab + n_tab + threadIdx.x;
    float* m_im = m_re + (size_t)a.nt * a.nc * tpb;
    fb_expand_item(a, p, k, m_re, m_im, tpb, tab);
}

}  // namespace csi
