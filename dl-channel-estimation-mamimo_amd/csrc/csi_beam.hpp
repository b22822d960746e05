// csi_beam.hpp - host side of the beam-space smoother (kernels: beam_smooth.hip.h): the basis and its two device images,
// the argument checks, the launches of csi_beam_power_device / csi_beam_smooth_device / csi_beam_wiener_device and the two host entry
// points as one staged call.  The orthonormality check of the basis and the overlap rule of the planes are csi_stage.hpp's, shared
// with csi_subspace.hpp.
#pragma once
#include "csi_context.hpp"
#include "csi_stage.hpp"
#include "beam_smooth.hip.h"

namespace {

constexpr double BM_ORTHO_TOL = 1e-4;          // largest |A^H A - I| entry a basis may have
constexpr size_t BM_IMAGE_FLOATS = (size_t)4 * BM_MAX_NT * BM_MAX_NT;      // a1 re | a1 im | a2 re | a2 im at the largest size

inline int bm_pad(int n) { return (n + 31) / 32 * 32; }

int beam_set_basis(csi_ctx* c, const float* a_re, const float* a_im, int nb) {
    static const char* who = "csi_beam_set_basis";
    const csi_config& cf = c->cfg;
    if (cf.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no beam-space smoother");
    if (cf.nt > BM_MAX_NT) return fail(c, CSI_ERR_INVALID_ARG, "%s: nt %d exceeds %d antennas", who, cf.nt, BM_MAX_NT);
    if (nb < 1 || nb > cf.nt) return fail(c, CSI_ERR_INVALID_ARG, "%s: nb %d outside 1 .. nt = %d", who, nb, cf.nt);
    if (!a_re || !a_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null basis planes", who);
    if (c->user_capture) return fail(c, CSI_ERR_INVALID_ARG, "%s: the basis cannot be replaced while a capture is open", who);
    const int nt = cf.nt;
    if (int rc = basis_orthonormal(c, who, a_re, a_im, nt, nb, BM_ORTHO_TOL, 'A')) return rc;
    const int ntp = bm_pad(nt), nbp = bm_pad(nb);
    const size_t plane = (size_t)ntp * nbp;
    std::vector<float> img(4 * plane, 0.0f);
    float* a1_re = img.data();
    float* a1_im = a1_re + plane;
    float* a2_re = a1_im + plane;
    float* a2_im = a2_re + plane;
    for (int j = 0; j < nt; ++j)
        for (int b = 0; b < nb; ++b) {
            const float vr = a_re[(size_t)j * nb + b], vi = a_im[(size_t)j * nb + b];
            a1_re[(size_t)j * nbp + b] = vr; a1_im[(size_t)j * nbp + b] = vi;
            a2_re[(size_t)b * ntp + j] = vr; a2_im[(size_t)b * ntp + j] = vi;
        }
    HIP_TRY(c, hipSetDevice(cf.device));
    if (!c->beam_a && hipMalloc((void**)&c->beam_a, BM_IMAGE_FLOATS * sizeof(float)) != hipSuccess) {
        c->beam_a = nullptr;
        return fail(c, CSI_ERR_NOMEM, "%s: device allocation of %zu bytes failed", who, BM_IMAGE_FLOATS * sizeof(float));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));                 // calls in flight still read the old images
    c->beam_nb = 0;
    HIP_TRY(c, hipMemcpy(c->beam_a, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
    c->beam_nb = nb;
    c->beam_ntp = ntp;
    c->beam_nbp = nbp;
    return CSI_OK;
}

// what every entry refuses except the alignment of the planes (the caller's: planes_aligned).  `rest`: the other required pointers are
// all there
int beam_check(csi_ctx* c, const char* who, const float* h_re, const float* h_im, int64_t npkt, bool rest, const char* names) {
    const csi_config& cf = c->cfg;
    if (cf.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no beam-space smoother");
    if (npkt < 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld must not be negative", who, (long long)npkt);
    if (!h_re || !h_im || !rest) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (%s)", who, names);
    if (c->beam_nb == 0) return fail(c, CSI_ERR_NOT_READY, "%s: no basis set (csi_beam_set_basis)", who);
    return CSI_OK;
}

// the overlap rule of the in / out planes (csi_stage.hpp: inout_planes_disjoint) over npkt packets
int beam_planes_disjoint(csi_ctx* c, const char* who, const float* h_re, const float* h_im, const float* out_re, const float* out_im, int64_t npkt) {
    return inout_planes_disjoint(c, who, h_re, h_im, out_re, out_im, (size_t)npkt * c->cfg.nr * c->cfg.nt * BM_N * sizeof(float));
}

BeamArgs beam_args(const csi_ctx* c, const float* d_h_re, const float* d_h_im, int64_t npkt) {
    const size_t plane = (size_t)c->beam_ntp * c->beam_nbp;
    BeamArgs a{};
    a.x_re = d_h_re; a.x_im = d_h_im;
    a.a1_re = c->beam_a;
    a.a1_im = a.a1_re + plane;
    a.a2_re = a.a1_im + plane;
    a.a2_im = a.a2_re + plane;
    a.planes = npkt * c->cfg.nr;
    a.nt = c->cfg.nt; a.nb = c->beam_nb; a.ntp = c->beam_ntp; a.nbp = c->beam_nbp;
    return a;
}

// one launch per 2^30 planes (whole packets)
inline int64_t beam_max_packets(const csi_ctx* c) { return std::max<int64_t>(1, ((int64_t)1 << 30) / c->cfg.nr); }

int beam_power_launch(csi_ctx* c, const float* d_h_re, const float* d_h_im, int64_t npkt, float* d_power) {
    const csi_config& cf = c->cfg;
    const int nb = c->beam_nb;
    const int tiles = std::max(c->beam_ntp, c->beam_nbp) / 32;
    const size_t pkt_f = (size_t)cf.nr * cf.nt * BM_N;
    for (int64_t p0 = 0; p0 < npkt; p0 += beam_max_packets(c)) {
        const int64_t np = std::min(beam_max_packets(c), npkt - p0);
        BeamArgs a = beam_args(c, d_h_re + p0 * pkt_f, d_h_im + p0 * pkt_f, np);
        a.power = d_power + (size_t)p0 * cf.nr * nb;
        // one complex product [nb][nt] per carrier, 8 flop per complex multiply-add, and |t|^2; x in, E out, one image of A
        ProfScope ps(c, K_BEAM_POWER, (double)a.planes * BM_N * nb * (8.0 * cf.nt + 3.0),
                     (double)a.planes * cf.nt * BM_N * 8.0 + (double)a.planes * nb * 4.0 + 8.0 * cf.nt * nb);
        const dim3 grid((unsigned)a.planes), block(BM_POWER_THREADS);
        if (tiles == 1) hipLaunchKernelGGL(beam_power_kernel<1>, grid, block, 0, c->stream, a);
        else if (tiles == 2) hipLaunchKernelGGL(beam_power_kernel<2>, grid, block, 0, c->stream, a);
        else hipLaunchKernelGGL(beam_power_kernel<4>, grid, block, 0, c->stream, a);
        HIP_TRY(c, hipGetLastError());
        ++c->beam_launches;
    }
    return CSI_OK;
}

int beam_smooth_launch(csi_ctx* c, const float* d_h_re, const float* d_h_im, int64_t npkt, const float* d_w, float* d_out_re, float* d_out_im) {
    const csi_config& cf = c->cfg;
    const int nb = c->beam_nb;
    const int tiles = std::max(c->beam_ntp, c->beam_nbp) / 32;
    const size_t pkt_f = (size_t)cf.nr * cf.nt * BM_N;
    for (int64_t p0 = 0; p0 < npkt; p0 += beam_max_packets(c)) {
        const int64_t np = std::min(beam_max_packets(c), npkt - p0);
        BeamArgs a = beam_args(c, d_h_re + p0 * pkt_f, d_h_im + p0 * pkt_f, np);
        a.y_re = d_out_re + p0 * pkt_f; a.y_im = d_out_im + p0 * pkt_f;
        a.w = d_w ? d_w + (size_t)p0 * cf.nr * nb : nullptr;
        // two complex products of [nt][nb] per carrier, 8 flop per complex multiply-add; x in, y out, w and the two images of A once
        ProfScope ps(c, K_BEAM_SMOOTH, 16.0 * (double)a.planes * BM_N * cf.nt * nb,
                     (double)a.planes * cf.nt * BM_N * 16.0 + (d_w ? (double)a.planes * nb * 4.0 : 0.0) + 16.0 * cf.nt * nb);
        const dim3 grid((unsigned)((a.planes * BM_KT + BM_THREADS / 64 - 1) / (BM_THREADS / 64))), block(BM_THREADS);
        if (tiles == 1) hipLaunchKernelGGL(beam_smooth_kernel<1>, grid, block, 0, c->stream, a);
        else if (tiles == 2) hipLaunchKernelGGL(beam_smooth_kernel<2>, grid, block, 0, c->stream, a);
        else hipLaunchKernelGGL(beam_smooth_kernel<4>, grid, block, 0, c->stream, a);
        HIP_TRY(c, hipGetLastError());
        ++c->beam_launches;
    }
    return CSI_OK;
}

int beam_weights_launch(csi_ctx* c, const float* d_power, const float* d_err_var, float* d_w, int64_t npkt) {
    const int nb = c->beam_nb;
    const long long per = (long long)beam_max_packets(c) * c->cfg.nr;      // planes per launch
    const long long planes = (long long)npkt * c->cfg.nr;
    for (long long q0 = 0; q0 < planes; q0 += per) {
        const long long n = std::min(per, planes - q0) * nb;
        hipLaunchKernelGGL(beam_wiener_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_power + (size_t)q0 * nb,
                           d_err_var + q0, d_w + (size_t)q0 * nb, n, nb);
        HIP_TRY(c, hipGetLastError());
        ++c->beam_launches;
    }
    return CSI_OK;
}

// the power pass, the weight pass, the smoothing pass.  E, and w when the caller keeps none, live in the context ([planes][nb] each;
// sized by eager calls: inside a capture the workspace must already hold the call)
int beam_wiener_device(csi_ctx* c, const char* who, const float* d_h_re, const float* d_h_im, int64_t npkt, const float* d_err_var,
                       float* d_out_re, float* d_out_im, float* d_w_out) {
    const csi_config& cf = c->cfg;
    HIP_TRY(c, hipSetDevice(cf.device));
    const size_t nw = (size_t)npkt * cf.nr * c->beam_nb;
    const size_t need = 2 * nw * sizeof(float);
    if (c->user_capture && c->beam_ws_bytes < need)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: the workspace of %lld packets is sized by an eager call of the same shape in front of the capture", who,
                    (long long)npkt);
    if (int rc = ensure_bytes(c, &c->beam_ws, &c->beam_ws_bytes, need)) return rc;
    float* d_power = reinterpret_cast<float*>(c->beam_ws);
    float* d_w = d_w_out ? d_w_out : d_power + nw;
    if (int rc = beam_power_launch(c, d_h_re, d_h_im, npkt, d_power)) return rc;
    if (int rc = beam_weights_launch(c, d_power, d_err_var, d_w, npkt)) return rc;
    return beam_smooth_launch(c, d_h_re, d_h_im, npkt, d_w, d_out_re, d_out_im);
}

// both host forms, as one staged call (csi_stage.hpp) whose chunk is sized by the four CSI planes.  wiener: v (err_var, [npkt][Nr]) makes
// the weights, which go back to w_out when that is given; otherwise w ([npkt][Nr][nb] or null) is the smoother's input
int beam_host(csi_ctx* c, const char* who, bool wiener, const float* h_re, const float* h_im, int64_t npkt, const float* w, const float* v,
              float* out_re, float* out_im, float* w_out) {
    if (int rc = beam_check(c, who, h_re, h_im, npkt, out_re && out_im && (!wiener || v), wiener ? "h, err_var, out" : "h, out")) return rc;
    if (npkt == 0) return CSI_OK;
    const csi_config& cf = c->cfg;
    HIP_TRY(c, hipSetDevice(cf.device));
    const size_t pkt = (size_t)cf.nr * cf.nt * BM_N * sizeof(float);      // bytes per packet and plane: a multiple of 16 (nt % 4 == 0)
    StagePlane p[] = {{pkt, h_re, nullptr}, {pkt, h_im, nullptr}, {pkt, nullptr, out_re}, {pkt, nullptr, out_im},
                      {(w || v) ? (size_t)cf.nr * c->beam_nb * sizeof(float) : 0, w, w_out}, {v ? (size_t)cf.nr * sizeof(float) : 0, v, nullptr}};
    return staged_call(c, npkt, stage_budget(c), 4 * pkt, 0, true, p, [&](int64_t, int64_t np) {
        if (v) return beam_wiener_device(c, who, p[0].as<float>(), p[1].as<float>(), np, p[5].as<float>(), p[2].as<float>(), p[3].as<float>(), p[4].as<float>());
        return beam_smooth_launch(c, p[0].as<float>(), p[1].as<float>(), np, w ? p[4].as<float>() : nullptr, p[2].as<float>(), p[3].as<float>());
    });
}

}  // namespace
