// csi_sync.hpp - host side of the symbol-timing stage (kernels: sync.hip.h): the argument checks, the launches of
// csi_sync_embed_device / csi_sync_estimate_device / csi_sync_extract_device, their sequence csi_sync_correct_device (theta and eps, when
// the caller keeps none, live in the context; sized by eager calls) and the host entry csi_sync_correct as one staged call.
// Nothing is uploaded, so every device entry can be captured.
#pragma once
#include "csi_context.hpp"
#include "csi_stage.hpp"
#include "csi_cfo.hpp"               // cfo_hit, cfo_check_planes
#include "sync.hip.h"

namespace {

constexpr uint32_t SYNC_FLAG_REMOVE_CFO = 1u;      // csi_sync_correct[_device]: the cut-out also removes eps_hat

// one array of a call, for the overlap rule: an output shares no byte with any other array
struct SyncSpan {
    const char* name;
    const void* p;
    size_t bytes;
    bool out;
};

// what every entry refuses about the context, the packet count and the span; the arrays come behind it
int sync_check_shape(csi_ctx* c, const char* who, int64_t npkt, int span) {
    const csi_config& cf = c->cfg;
    if (cf.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no sounding symbols");
    if (npkt < 1) return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld must be at least 1", who, (long long)npkt);
    if (cf.len_ltf != CFO_SYM * cf.nt)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: len_ltf %d is not %d sounding symbols of 320 samples", who, cf.len_ltf, cf.nt);
    if (span < 4 || span > SYNC_SPAN_MAX || (span & 3))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: span %d must be a multiple of 4 in 4 .. %d", who, span, SYNC_SPAN_MAX);
    const int64_t wg = ((int64_t)cf.nr * ((CFO_SYM * cf.nt + span) / 4) + SYNC_THREADS - 1) / SYNC_THREADS;
    if (npkt > 0x7fffffff / wg)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets exceed one launch (2^31 - 1 workgroups of %d 16-byte words)", who, (long long)npkt, SYNC_THREADS);
    return CSI_OK;
}

int sync_check_rho(csi_ctx* c, const char* who, double rho) {
    if (!std::isfinite(rho) || rho < 0.0 || rho > 1.0) return fail(c, CSI_ERR_INVALID_ARG, "%s: rho %g must be finite and in [0, 1]", who, rho);
    return CSI_OK;
}

int sync_check_flags(csi_ctx* c, const char* who, uint32_t flags) {
    if (flags & ~SYNC_FLAG_REMOVE_CFO) return fail(c, CSI_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (bit 0: also remove eps_hat)", who, flags & ~SYNC_FLAG_REMOVE_CFO);
    return CSI_OK;
}

// a per-packet array on its word size (null passes)
int sync_check_words(csi_ctx* c, const char* who, const char* name, const void* p, size_t word) {
    if (reinterpret_cast<uintptr_t>(p) & (word - 1))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: %s must be aligned for %zu-byte words (got %p)", who, name, word, p);
    return CSI_OK;
}

template <size_t N>
int sync_check_overlap(csi_ctx* c, const char* who, const SyncSpan (&s)[N]) {
    for (size_t i = 0; i < N; ++i)
        for (size_t j = i + 1; j < N; ++j)
            if ((s[i].out || s[j].out) && cfo_hit(s[i].p, s[i].bytes, s[j].p, s[j].bytes))
                return fail(c, CSI_ERR_INVALID_ARG, "%s: %s shares a byte with %s: an output overlaps no other array of the call", who, s[j].name, s[i].name);
    return CSI_OK;
}

inline size_t sync_cap_bytes(const csi_config& cf, int64_t npkt, int span) { return (size_t)npkt * cf.nr * ((size_t)cf.len_ltf + span) * sizeof(float); }
inline size_t sync_pkt_bytes(const csi_config& cf, int64_t npkt) { return (size_t)npkt * cf.nr * (size_t)cf.len_ltf * sizeof(float); }

// ---- launches (arguments checked by the callers)
int sync_metric_launch(csi_ctx* c, const float* d_cap_re, const float* d_cap_im, int64_t npkt, int span, double rho, int32_t* d_theta, double* d_eps,
                       float* d_quality, double* d_metric) {
    const csi_config& cf = c->cfg;
    SyncMetricArgs a{};
    a.c_re = d_cap_re; a.c_im = d_cap_im; a.theta = d_theta; a.eps = d_eps; a.quality = d_quality; a.metric = d_metric;
    a.rho = rho; a.nt = cf.nt; a.nr = cf.nr; a.span = span;
    const double pairs = (double)npkt * cf.nr * cf.nt * (span + CFO_CP);
    // per folded pair of samples: the 16 flop and 16 bytes of cfo_corr; the window sums and the optional metric are small beside them
    ProfScope ps(c, K_SYNC_METRIC, pairs * 16.0, pairs * 16.0 + (double)npkt * (16.0 + (d_metric ? 8.0 * (span + 1) : 0.0)));
    hipLaunchKernelGGL(sync_metric_kernel<0>, dim3((unsigned)npkt), dim3(SYNC_THREADS), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    ++c->sync_launches;
    return CSI_OK;
}

int sync_extract_launch(csi_ctx* c, const float* d_cap_re, const float* d_cap_im, int64_t npkt, int span, const int32_t* d_theta, const double* d_eps,
                        float* d_out_re, float* d_out_im) {
    const csi_config& cf = c->cfg;
    SyncExtractArgs a{};
    a.c_re = d_cap_re; a.c_im = d_cap_im; a.y_re = d_out_re; a.y_im = d_out_im; a.theta = d_theta; a.eps = d_eps;
    a.row = (long long)CFO_SYM * cf.nt;
    a.groups = (long long)cf.nr * (CFO_SYM / 4) * cf.nt;
    a.nr = cf.nr; a.span = span;
    a.wg_per_pkt = (int)((a.groups + SYNC_THREADS - 1) / SYNC_THREADS);
    const double samples = (double)npkt * cf.nr * cf.len_ltf;
    // 6 flop of the complex product per sample when eps is given; both planes in and out
    ProfScope ps(c, K_SYNC_EXTRACT, d_eps ? samples * 6.0 : 0.0, samples * 16.0 + (double)npkt * (d_eps ? 12.0 : 4.0));
    hipLaunchKernelGGL(sync_extract_kernel<0>, dim3((unsigned)(npkt * a.wg_per_pkt)), dim3(SYNC_THREADS), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    ++c->sync_launches;
    return CSI_OK;
}

int sync_embed_launch(csi_ctx* c, uint64_t seed, int64_t first_pkt, int64_t npkt, int span, const int32_t* d_theta, const float* d_margin_std,
                      const float* d_x_re, const float* d_x_im, float* d_cap_re, float* d_cap_im) {
    const csi_config& cf = c->cfg;
    SyncEmbedArgs a{};
    a.x_re = d_x_re; a.x_im = d_x_im; a.c_re = d_cap_re; a.c_im = d_cap_im; a.theta = d_theta; a.std = d_margin_std;
    a.seed = seed; a.first_pkt = first_pkt;
    a.row = (long long)CFO_SYM * cf.nt;
    a.cap_row = a.row + span;
    a.groups = (long long)cf.nr * (a.cap_row / 4);
    a.nr = cf.nr; a.span = span;
    a.wg_per_pkt = (int)((a.groups + SYNC_THREADS - 1) / SYNC_THREADS);
    const double in = (double)npkt * cf.nr * cf.len_ltf, out = (double)npkt * cf.nr * (double)a.cap_row;
    // the packet's samples in, the capture's out, both planes; the margin draws are not counted as flop
    ProfScope ps(c, K_SYNC_EMBED, 0.0, (in + out) * 8.0 + (double)npkt * 8.0);
    hipLaunchKernelGGL(sync_embed_kernel<0>, dim3((unsigned)(npkt * a.wg_per_pkt)), dim3(SYNC_THREADS), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    ++c->sync_launches;
    return CSI_OK;
}

// ---- entry points
int sync_embed_device(csi_ctx* c, uint64_t seed, int64_t first_pkt, int64_t npkt, int span, const int32_t* d_theta, const float* d_margin_std,
                      const float* d_x_re, const float* d_x_im, float* d_cap_re, float* d_cap_im) {
    static const char* who = "csi_sync_embed_device";
    if (int rc = sync_check_shape(c, who, npkt, span)) return rc;
    if (first_pkt < 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: first_pkt %lld must not be negative", who, (long long)first_pkt);
    if (int rc = cfo_check_planes(c, who, "d_x", d_x_re, d_x_im)) return rc;
    if (int rc = cfo_check_planes(c, who, "d_cap", d_cap_re, d_cap_im)) return rc;
    if (!d_theta) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (d_theta)", who);
    if (int rc = sync_check_words(c, who, "d_theta", d_theta, 4)) return rc;
    if (int rc = sync_check_words(c, who, "d_margin_std", d_margin_std, 4)) return rc;
    const size_t xb = sync_pkt_bytes(c->cfg, npkt), cb = sync_cap_bytes(c->cfg, npkt, span);
    const SyncSpan s[] = {{"d_x_re", d_x_re, xb, false}, {"d_x_im", d_x_im, xb, false}, {"d_theta", d_theta, (size_t)npkt * 4, false},
                          {"d_margin_std", d_margin_std, (size_t)npkt * 4, false}, {"d_cap_re", d_cap_re, cb, true}, {"d_cap_im", d_cap_im, cb, true}};
    if (int rc = sync_check_overlap(c, who, s)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return sync_embed_launch(c, seed, first_pkt, npkt, span, d_theta, d_margin_std, d_x_re, d_x_im, d_cap_re, d_cap_im);
}

int sync_estimate_device(csi_ctx* c, const float* d_cap_re, const float* d_cap_im, int64_t npkt, int span, double rho, int32_t* d_theta, double* d_eps,
                         float* d_quality, double* d_metric) {
    static const char* who = "csi_sync_estimate_device";
    if (int rc = sync_check_shape(c, who, npkt, span)) return rc;
    if (int rc = sync_check_rho(c, who, rho)) return rc;
    if (int rc = cfo_check_planes(c, who, "d_cap", d_cap_re, d_cap_im)) return rc;
    if (!d_theta) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (d_theta)", who);
    if (int rc = sync_check_words(c, who, "d_theta", d_theta, 4)) return rc;
    if (int rc = sync_check_words(c, who, "d_eps", d_eps, 8)) return rc;
    if (int rc = sync_check_words(c, who, "d_quality", d_quality, 4)) return rc;
    if (int rc = sync_check_words(c, who, "d_metric", d_metric, 8)) return rc;
    const size_t cb = sync_cap_bytes(c->cfg, npkt, span);
    const SyncSpan s[] = {{"d_cap_re", d_cap_re, cb, false}, {"d_cap_im", d_cap_im, cb, false}, {"d_theta", d_theta, (size_t)npkt * 4, true},
                          {"d_eps", d_eps, (size_t)npkt * 8, true}, {"d_quality", d_quality, (size_t)npkt * 4, true},
                          {"d_metric", d_metric, (size_t)npkt * (span + 1) * 8, true}};
    if (int rc = sync_check_overlap(c, who, s)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return sync_metric_launch(c, d_cap_re, d_cap_im, npkt, span, rho, d_theta, d_eps, d_quality, d_metric);
}

int sync_extract_device(csi_ctx* c, const float* d_cap_re, const float* d_cap_im, int64_t npkt, int span, const int32_t* d_theta, const double* d_eps,
                        float* d_out_re, float* d_out_im) {
    static const char* who = "csi_sync_extract_device";
    if (int rc = sync_check_shape(c, who, npkt, span)) return rc;
    if (int rc = cfo_check_planes(c, who, "d_cap", d_cap_re, d_cap_im)) return rc;
    if (int rc = cfo_check_planes(c, who, "d_out", d_out_re, d_out_im)) return rc;
    if (!d_theta) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (d_theta)", who);
    if (int rc = sync_check_words(c, who, "d_theta", d_theta, 4)) return rc;
    if (int rc = sync_check_words(c, who, "d_eps", d_eps, 8)) return rc;
    const size_t cb = sync_cap_bytes(c->cfg, npkt, span), ob = sync_pkt_bytes(c->cfg, npkt);
    const SyncSpan s[] = {{"d_cap_re", d_cap_re, cb, false}, {"d_cap_im", d_cap_im, cb, false}, {"d_theta", d_theta, (size_t)npkt * 4, false},
                          {"d_eps", d_eps, (size_t)npkt * 8, false}, {"d_out_re", d_out_re, ob, true}, {"d_out_im", d_out_im, ob, true}};
    if (int rc = sync_check_overlap(c, who, s)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return sync_extract_launch(c, d_cap_re, d_cap_im, npkt, span, d_theta, d_eps, d_out_re, d_out_im);
}

// estimate, then cut out at theta_hat (with bit 0 of flags, also removing eps_hat): two launches.  theta and eps [npkt], when the caller
// keeps none, live in the context (sized by eager calls: inside a capture the workspace must already hold the call)
int sync_correct_device(csi_ctx* c, const char* who, const float* d_cap_re, const float* d_cap_im, int64_t npkt, int span, double rho, uint32_t flags,
                        float* d_out_re, float* d_out_im, int32_t* d_theta, double* d_eps, float* d_quality) {
    if (int rc = sync_check_shape(c, who, npkt, span)) return rc;
    if (int rc = sync_check_rho(c, who, rho)) return rc;
    if (int rc = sync_check_flags(c, who, flags)) return rc;
    if (int rc = cfo_check_planes(c, who, "d_cap", d_cap_re, d_cap_im)) return rc;
    if (int rc = cfo_check_planes(c, who, "d_out", d_out_re, d_out_im)) return rc;
    if (int rc = sync_check_words(c, who, "d_theta", d_theta, 4)) return rc;
    if (int rc = sync_check_words(c, who, "d_eps", d_eps, 8)) return rc;
    if (int rc = sync_check_words(c, who, "d_quality", d_quality, 4)) return rc;
    const size_t cb = sync_cap_bytes(c->cfg, npkt, span), ob = sync_pkt_bytes(c->cfg, npkt);
    const SyncSpan s[] = {{"d_cap_re", d_cap_re, cb, false}, {"d_cap_im", d_cap_im, cb, false}, {"d_out_re", d_out_re, ob, true}, {"d_out_im", d_out_im, ob, true},
                          {"d_theta", d_theta, (size_t)npkt * 4, true}, {"d_eps", d_eps, (size_t)npkt * 8, true}, {"d_quality", d_quality, (size_t)npkt * 4, true}};
    if (int rc = sync_check_overlap(c, who, s)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int32_t* theta = d_theta;
    double* eps = d_eps;
    const bool remove = (flags & SYNC_FLAG_REMOVE_CFO) != 0;
    if (!theta || (remove && !eps)) {
        const size_t need = (size_t)npkt * (sizeof(double) + sizeof(int32_t));
        if (c->user_capture && c->sync_ws_bytes < need)
            return fail(c, CSI_ERR_INVALID_ARG, "%s: the workspace of %lld packets is sized by an eager call of the same shape in front of the capture", who,
                        (long long)npkt);
        if (int rc = ensure_bytes(c, &c->sync_ws, &c->sync_ws_bytes, need)) return rc;
        if (remove && !eps) eps = reinterpret_cast<double*>(c->sync_ws);
        if (!theta) theta = reinterpret_cast<int32_t*>(c->sync_ws + (size_t)npkt * sizeof(double));
    }
    if (int rc = sync_metric_launch(c, d_cap_re, d_cap_im, npkt, span, rho, theta, eps, d_quality, nullptr)) return rc;
    return sync_extract_launch(c, d_cap_re, d_cap_im, npkt, span, theta, remove ? eps : nullptr, d_out_re, d_out_im);
}

// host buffers: the capture planes go up, the cut-out planes and the per-packet results come down; the chunk is sized by the four planes
int sync_correct_host(csi_ctx* c, const float* cap_re, const float* cap_im, int64_t npkt, int span, double rho, uint32_t flags, float* out_re, float* out_im,
                      int32_t* theta, double* eps, float* quality) {
    static const char* who = "csi_sync_correct";
    if (int rc = sync_check_shape(c, who, npkt, span)) return rc;
    if (int rc = sync_check_rho(c, who, rho)) return rc;
    if (int rc = sync_check_flags(c, who, flags)) return rc;
    if (!cap_re || !cap_im || !out_re || !out_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (cap_re, cap_im, out_re, out_im)", who);
    const csi_config& cf = c->cfg;
    const size_t cap = sync_cap_bytes(cf, 1, span), pkt = sync_pkt_bytes(cf, 1);      // bytes per packet and plane: multiples of 16
    const SyncSpan s[] = {{"cap_re", cap_re, cap * (size_t)npkt, false}, {"cap_im", cap_im, cap * (size_t)npkt, false},
                          {"out_re", out_re, pkt * (size_t)npkt, true}, {"out_im", out_im, pkt * (size_t)npkt, true},
                          {"theta", theta, (size_t)npkt * 4, true}, {"eps", eps, (size_t)npkt * 8, true}, {"quality", quality, (size_t)npkt * 4, true}};
    if (int rc = sync_check_overlap(c, who, s)) return rc;
    HIP_TRY(c, hipSetDevice(cf.device));
    StagePlane p[] = {{cap, cap_re, nullptr}, {cap, cap_im, nullptr}, {pkt, nullptr, out_re}, {pkt, nullptr, out_im},
                      {sizeof(double), nullptr, eps}, {sizeof(int32_t), nullptr, theta}, {sizeof(float), nullptr, quality}};
    return staged_call(c, npkt, stage_budget(c), 2 * (cap + pkt), 0, true, p, [&](int64_t, int64_t np) {
        return sync_correct_device(c, who, p[0].as<float>(), p[1].as<float>(), np, span, rho, flags, p[2].as<float>(), p[3].as<float>(), p[5].as<int32_t>(),
                                   p[4].as<double>(), p[6].as<float>());
    });
}

}  // namespace
