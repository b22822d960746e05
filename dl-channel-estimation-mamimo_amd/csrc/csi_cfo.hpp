// csi_cfo.hpp - host side of the carrier-frequency-offset stage (kernels: cfo.hip.h): the argument checks, the launches
// of csi_cfo_estimate_device / csi_cfo_rotate_device, their sequence csi_cfo_correct_device (eps, when the caller keeps none, lives in
// the context; sized by eager calls) and the host entry csi_cfo_correct as one staged call that rotates the staged planes in place.
// Nothing is uploaded, so every device entry can be captured.
#pragma once
#include "csi_context.hpp"
#include "csi_stage.hpp"
#include "cfo.hip.h"

namespace {

// [p, p + pb) and [q, q + qb) share a byte (null passes)
inline bool cfo_hit(const void* p, size_t pb, const void* q, size_t qb) {
    if (!p || !q) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + qb && b < a + pb;
}

// what every entry refuses about the context and the packet count; the planes come behind it
int cfo_check_shape(csi_ctx* c, const char* who, int64_t npkt) {
    const csi_config& cf = c->cfg;
    if (cf.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no sounding symbols");
    if (npkt < 1) return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld must be at least 1", who, (long long)npkt);
    if (cf.len_ltf != CFO_SYM * cf.nt)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: len_ltf %d is not %d sounding symbols of 320 samples", who, cf.len_ltf, cf.nt);
    const int64_t wg = ((int64_t)cf.nr * (CFO_SYM / 4) * cf.nt + CFO_THREADS - 1) / CFO_THREADS;
    if (npkt > 0x7fffffff / wg)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets exceed one launch (2^31 - 1 workgroups of %d 16-byte words)", who, (long long)npkt, CFO_THREADS);
    return CSI_OK;
}

int cfo_check_skip(csi_ctx* c, const char* who, int cp_skip) {
    if (cp_skip < 0 || cp_skip >= CFO_CP) return fail(c, CSI_ERR_INVALID_ARG, "%s: cp_skip %d outside 0 .. %d", who, cp_skip, CFO_CP - 1);
    return CSI_OK;
}

// the two planes of a preamble argument: present and on a 16-byte boundary
int cfo_check_planes(csi_ctx* c, const char* who, const char* name, const float* re, const float* im) {
    if (!re || !im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (%s_re, %s_im)", who, name, name);
    if ((reinterpret_cast<uintptr_t>(re) | reinterpret_cast<uintptr_t>(im)) & 15)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: %s_re / %s_im must start on a 16-byte boundary (got %p, %p)", who, name, name, (const void*)re, (const void*)im);
    return CSI_OK;
}

// eps (8-byte words) and quality (4-byte words): aligned, and no byte shared with a plane or with each other
int cfo_check_scalars(csi_ctx* c, const char* who, const double* d_eps, const float* d_quality, int64_t npkt, const float* const* planes, int n_planes,
                      size_t plane_bytes) {
    if ((reinterpret_cast<uintptr_t>(d_eps) & 7) || (reinterpret_cast<uintptr_t>(d_quality) & 3))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: d_eps must be aligned for 8-byte words and d_quality for 4-byte words (got %p, %p)", who, (const void*)d_eps,
                    (const void*)d_quality);
    const size_t eb = (size_t)npkt * sizeof(double), qb = (size_t)npkt * sizeof(float);
    bool hit = cfo_hit(d_eps, eb, d_quality, qb);
    for (int i = 0; i < n_planes; ++i) hit = hit || cfo_hit(d_eps, eb, planes[i], plane_bytes) || cfo_hit(d_quality, qb, planes[i], plane_bytes);
    if (hit) return fail(c, CSI_ERR_INVALID_ARG, "%s: d_eps / d_quality overlap a plane or each other", who);
    return CSI_OK;
}

// ---- launches (arguments checked by the callers)
int cfo_corr_launch(csi_ctx* c, const float* d_re, const float* d_im, int64_t npkt, int cp_skip, double* d_eps, float* d_quality) {
    const csi_config& cf = c->cfg;
    CfoCorrArgs a{};
    a.x_re = d_re; a.x_im = d_im; a.eps = d_eps; a.quality = d_quality;
    a.nt = cf.nt; a.nr = cf.nr; a.cp_skip = cp_skip;
    const double pairs = (double)npkt * cf.nr * cf.nt * (CFO_CP - cp_skip);
    // per pair of samples: two fp32 products of 3 flop, two energies of 3 flop, four fp64 adds; both samples of both planes in
    ProfScope ps(c, K_CFO_CORR, pairs * 16.0, pairs * 16.0 + (double)npkt * 12.0);
    hipLaunchKernelGGL(cfo_corr_kernel<0>, dim3((unsigned)npkt), dim3(CFO_THREADS), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    ++c->cfo_launches;
    return CSI_OK;
}

int cfo_rotate_launch(csi_ctx* c, const float* d_in_re, const float* d_in_im, int64_t npkt, const double* d_eps, double scale, float* d_out_re, float* d_out_im) {
    const csi_config& cf = c->cfg;
    CfoRotateArgs a{};
    a.x_re = d_in_re; a.x_im = d_in_im; a.y_re = d_out_re; a.y_im = d_out_im; a.eps = d_eps; a.scale = scale;
    a.row = (long long)CFO_SYM * cf.nt;
    a.groups = (long long)cf.nr * (CFO_SYM / 4) * cf.nt;
    a.wg_per_pkt = (int)((a.groups + CFO_THREADS - 1) / CFO_THREADS);
    const double samples = (double)npkt * cf.nr * cf.len_ltf;
    // 6 flop of the complex product per sample (the phase apart); both planes in and out
    ProfScope ps(c, K_CFO_ROTATE, samples * 6.0, samples * 16.0 + (double)npkt * 8.0);
    hipLaunchKernelGGL(cfo_rotate_kernel<0>, dim3((unsigned)(npkt * a.wg_per_pkt)), dim3(CFO_THREADS), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    ++c->cfo_launches;
    return CSI_OK;
}

// ---- entry points
int cfo_estimate_device(csi_ctx* c, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt, int cp_skip, double* d_eps, float* d_quality) {
    static const char* who = "csi_cfo_estimate_device";
    if (int rc = cfo_check_shape(c, who, npkt)) return rc;
    if (int rc = cfo_check_skip(c, who, cp_skip)) return rc;
    if (int rc = cfo_check_planes(c, who, "d_ltf", d_ltf_re, d_ltf_im)) return rc;
    if (!d_eps) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (d_eps)", who);
    const float* planes[] = {d_ltf_re, d_ltf_im};
    if (int rc = cfo_check_scalars(c, who, d_eps, d_quality, npkt, planes, 2, (size_t)npkt * c->cfg.nr * c->cfg.len_ltf * sizeof(float))) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return cfo_corr_launch(c, d_ltf_re, d_ltf_im, npkt, cp_skip, d_eps, d_quality);
}

int cfo_rotate_device(csi_ctx* c, const float* d_in_re, const float* d_in_im, int64_t npkt, const double* d_eps, double scale, float* d_out_re, float* d_out_im) {
    static const char* who = "csi_cfo_rotate_device";
    if (int rc = cfo_check_shape(c, who, npkt)) return rc;
    if (int rc = cfo_check_planes(c, who, "d_in", d_in_re, d_in_im)) return rc;
    if (int rc = cfo_check_planes(c, who, "d_out", d_out_re, d_out_im)) return rc;
    if (!d_eps) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (d_eps)", who);
    if (!std::isfinite(scale)) return fail(c, CSI_ERR_INVALID_ARG, "%s: scale %g must be finite", who, scale);
    const size_t bytes = (size_t)npkt * c->cfg.nr * c->cfg.len_ltf * sizeof(float);
    if (int rc = inout_planes_disjoint(c, who, d_in_re, d_in_im, d_out_re, d_out_im, bytes)) return rc;
    const float* outs[] = {d_out_re, d_out_im};
    if (int rc = cfo_check_scalars(c, who, d_eps, nullptr, npkt, outs, 2, bytes)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return cfo_rotate_launch(c, d_in_re, d_in_im, npkt, d_eps, scale, d_out_re, d_out_im);
}

// estimate, then rotate by -eps_hat: two launches.  eps [npkt], when the caller keeps none, lives in the context (sized by eager calls:
// inside a capture the workspace must already hold the call)
int cfo_correct_device(csi_ctx* c, const char* who, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt, int cp_skip, float* d_out_re, float* d_out_im,
                       double* d_eps, float* d_quality) {
    if (int rc = cfo_check_shape(c, who, npkt)) return rc;
    if (int rc = cfo_check_skip(c, who, cp_skip)) return rc;
    if (int rc = cfo_check_planes(c, who, "d_ltf", d_ltf_re, d_ltf_im)) return rc;
    if (int rc = cfo_check_planes(c, who, "d_out", d_out_re, d_out_im)) return rc;
    const size_t bytes = (size_t)npkt * c->cfg.nr * c->cfg.len_ltf * sizeof(float);
    if (int rc = inout_planes_disjoint(c, who, d_ltf_re, d_ltf_im, d_out_re, d_out_im, bytes)) return rc;
    const float* planes[] = {d_ltf_re, d_ltf_im, d_out_re, d_out_im};
    if (int rc = cfo_check_scalars(c, who, d_eps, d_quality, npkt, planes, 4, bytes)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    double* eps = d_eps;
    if (!eps) {
        const size_t need = (size_t)npkt * sizeof(double);
        if (c->user_capture && c->cfo_ws_bytes < need)
            return fail(c, CSI_ERR_INVALID_ARG, "%s: the workspace of %lld packets is sized by an eager call of the same shape in front of the capture", who,
                        (long long)npkt);
        if (int rc = ensure_bytes(c, &c->cfo_ws, &c->cfo_ws_bytes, need)) return rc;
        eps = reinterpret_cast<double*>(c->cfo_ws);
    }
    if (int rc = cfo_corr_launch(c, d_ltf_re, d_ltf_im, npkt, cp_skip, eps, d_quality)) return rc;
    return cfo_rotate_launch(c, d_ltf_re, d_ltf_im, npkt, eps, -1.0, d_out_re, d_out_im);
}

// host buffers: the two preamble planes go up, are corrected where they lie and come down into out; the chunk is sized by them
int cfo_correct_host(csi_ctx* c, const float* ltf_re, const float* ltf_im, int64_t npkt, int cp_skip, float* out_re, float* out_im, double* eps, float* quality) {
    static const char* who = "csi_cfo_correct";
    if (int rc = cfo_check_shape(c, who, npkt)) return rc;
    if (int rc = cfo_check_skip(c, who, cp_skip)) return rc;
    if (!ltf_re || !ltf_im || !out_re || !out_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (ltf_re, ltf_im, out_re, out_im)", who);
    const csi_config& cf = c->cfg;
    const size_t pkt = (size_t)cf.nr * cf.len_ltf * sizeof(float);      // bytes per packet and plane: a multiple of 16
    // a chunk's results go down before the next chunk's preambles go up: the host arrays obey the overlap rule of the device entry
    if (int rc = inout_planes_disjoint(c, who, ltf_re, ltf_im, out_re, out_im, (size_t)npkt * pkt)) return rc;
    HIP_TRY(c, hipSetDevice(cf.device));
    StagePlane p[] = {{pkt, ltf_re, out_re}, {pkt, ltf_im, out_im}, {sizeof(double), nullptr, eps}, {sizeof(float), nullptr, quality}};
    return staged_call(c, npkt, stage_budget(c), 2 * pkt, 0, true, p, [&](int64_t, int64_t np) {
        return cfo_correct_device(c, who, p[0].as<float>(), p[1].as<float>(), np, cp_skip, p[0].as<float>(), p[1].as<float>(), p[2].as<double>(), p[3].as<float>());
    });
}

}  // namespace
