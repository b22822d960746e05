// csi_forecast.hpp - host side of the channel forecast (kernels: forecast.hip.h): the argument checks, the launches of
// csi_forecast_gram_device / csi_forecast_fit_device / csi_forecast_apply_device, their sequence csi_forecast_device (T, and c when the
// caller keeps none, live in the context; sized by eager calls), the host entry csi_forecast as one staged call with one plane per
// sounding and component, and csi_sounding_noise_device.  Nothing is uploaded, so every device entry can be captured.
#pragma once
#include "csi_context.hpp"
#include "csi_stage.hpp"
#include "forecast.hip.h"

namespace {

struct FcPlane { std::string name; const void* p; size_t bytes; };

// what every forecast entry refuses about the context, the soundings and the packet count
int fc_check_shape(csi_ctx* c, const char* who, int n_snd, int64_t npkt) {
    const csi_config& cf = c->cfg;
    if (cf.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no channel forecast");
    if (n_snd < 2 || n_snd > FC_MAX_SND) return fail(c, CSI_ERR_INVALID_ARG, "%s: n_snd %d outside 2 .. %d", who, n_snd, FC_MAX_SND);
    if (npkt < 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld must not be negative", who, (long long)npkt);
    if (npkt * cf.nr > 0x7fffffff)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets x %d rx antennas exceed one launch (2^31 - 1 items)", who, (long long)npkt, cf.nr);
    return CSI_OK;
}

int fc_check_order(csi_ctx* c, const char* who, int n_snd, int order, int steps) {
    if (order < 1 || order > FC_MAX_ORDER) return fail(c, CSI_ERR_INVALID_ARG, "%s: order %d outside 1 .. %d", who, order, FC_MAX_ORDER);
    if (steps < 1) return fail(c, CSI_ERR_INVALID_ARG, "%s: steps %d must be at least 1", who, steps);
    if (order + steps > n_snd)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: order %d + steps %d exceed n_snd %d (no equation is left)", who, order, steps, n_snd);
    return CSI_OK;
}

int fc_check_fit(csi_ctx* c, const char* who, int n_snd, int order, int steps, double ridge, uint32_t flags) {
    if (int rc = fc_check_order(c, who, n_snd, order, steps)) return rc;
    if (!std::isfinite(ridge) || ridge < 0.0) return fail(c, CSI_ERR_INVALID_ARG, "%s: ridge %g must be finite and not negative", who, ridge);
    if (flags & ~1u) return fail(c, CSI_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (bit 0 = one fit per packet, pooled over its rx antennas)", who, flags);
    return CSI_OK;
}

// a host array of n device planes: no null entry, every plane on a 16-byte boundary
int fc_check_planes(csi_ctx* c, const char* who, const char* name, const float* const* planes, int n) {
    if (!planes) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (%s)", who, name);
    for (int i = 0; i < n; ++i) {
        if (!planes[i]) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (%s[%d])", who, name, i);
        if (reinterpret_cast<uintptr_t>(planes[i]) & 15)
            return fail(c, CSI_ERR_INVALID_ARG, "%s: %s[%d] must start on a 16-byte boundary (got %p)", who, name, i, (const void*)planes[i]);
    }
    return CSI_OK;
}

int fc_check_aligned(csi_ctx* c, const char* who, const FcPlane* planes, int n, unsigned mask) {
    for (int i = 0; i < n; ++i)
        if (reinterpret_cast<uintptr_t>(planes[i].p) & mask) {
            if (mask == 15) return fail(c, CSI_ERR_INVALID_ARG, "%s: %s must start on a 16-byte boundary (got %p)", who, planes[i].name.c_str(), planes[i].p);
            return fail(c, CSI_ERR_INVALID_ARG, "%s: %s must be aligned for 4-byte words (got %p)", who, planes[i].name.c_str(), planes[i].p);
        }
    return CSI_OK;
}

// no output shares a byte with an input or with another output (null planes pass)
int fc_check_disjoint(csi_ctx* c, const char* who, const FcPlane* outs, int n_out, const FcPlane* ins, int n_in) {
    auto hit = [](const FcPlane& x, const FcPlane& y) {
        if (!x.p || !y.p || !x.bytes || !y.bytes) return false;
        const uintptr_t a = reinterpret_cast<uintptr_t>(x.p), b = reinterpret_cast<uintptr_t>(y.p);
        return a < b + y.bytes && b < a + x.bytes;
    };
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i)
            if (hit(outs[o], ins[i])) return fail(c, CSI_ERR_INVALID_ARG, "%s: the output %s overlaps the input %s", who, outs[o].name.c_str(), ins[i].name.c_str());
        for (int q = o + 1; q < n_out; ++q)
            if (hit(outs[o], outs[q])) return fail(c, CSI_ERR_INVALID_ARG, "%s: the outputs %s and %s overlap", who, outs[o].name.c_str(), outs[q].name.c_str());
    }
    return CSI_OK;
}

// the n sounding planes of one component as FcPlane records named name[i]
void fc_name_planes(std::vector<FcPlane>& v, const char* name, const float* const* planes, int n, size_t bytes) {
    for (int i = 0; i < n; ++i) v.push_back({std::string(name) + "[" + std::to_string(i) + "]", planes[i], bytes});
}

// ---- launches (arguments checked by the callers)
int forecast_gram_launch(csi_ctx* c, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t blocks, int64_t kf, float* d_t_re, float* d_t_im) {
    ForecastGramArgs a{};
    for (int i = 0; i < n_snd; ++i) { a.x_re[i] = d_x_re[i]; a.x_im[i] = d_x_im[i]; }
    a.t_re = d_t_re; a.t_im = d_t_im;
    a.kf = kf; a.n_snd = n_snd;
    // three real 16 x 16 products per float of K, 2 flop per multiply-add; the 2 P planes in, T out
    ProfScope ps(c, K_FORECAST_GRAM, (double)blocks * kf * 3.0 * 2.0 * 16.0 * 16.0, (double)blocks * (8.0 * n_snd * kf + 8.0 * n_snd * n_snd));
    const dim3 grid((unsigned)blocks), block(FC_THREADS);
    if (n_snd <= 4) hipLaunchKernelGGL(forecast_gram_kernel<4>, grid, block, 0, c->stream, a);
    else if (n_snd <= 8) hipLaunchKernelGGL(forecast_gram_kernel<8>, grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL(forecast_gram_kernel<16>, grid, block, 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    ++c->forecast_launches;
    return CSI_OK;
}

int forecast_fit_launch(csi_ctx* c, const float* d_t_re, const float* d_t_im, int n_snd, int64_t npkt, int order, int steps, double ridge, uint32_t flags,
                        float* d_c_re, float* d_c_im, float* d_fit_err, int32_t* d_info) {
    ForecastFitArgs a{};
    a.t_re = d_t_re; a.t_im = d_t_im; a.c_re = d_c_re; a.c_im = d_c_im; a.fit_err = d_fit_err; a.info = d_info;
    a.ridge = ridge;
    a.pooled = (flags & 1u) ? 1 : 0;
    a.nr = c->cfg.nr; a.n_snd = n_snd; a.order = order; a.steps = steps;
    a.items = a.pooled ? npkt : npkt * c->cfg.nr;
    const double blocks = (double)npkt * c->cfg.nr, eq = n_snd - order - steps + 1;
    // the sums of G and rhs (2 adds per complex entry and equation), Cholesky and the two triangular solves (8 flop per complex multiply-add)
    ProfScope ps(c, K_FORECAST_FIT, blocks * (2.0 * eq * (order * (order + 1) / 2.0 + order + 1) + 8.0 * (order * order * order / 6.0 + order * order)),
                 blocks * (8.0 * n_snd * n_snd + 8.0 * order + 8.0));
    hipLaunchKernelGGL(forecast_fit_kernel<FC_MAX_ORDER>, dim3((unsigned)((a.items + FC_FIT_THREADS - 1) / FC_FIT_THREADS)), dim3(FC_FIT_THREADS), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    ++c->forecast_launches;
    return CSI_OK;
}

int forecast_apply_launch(csi_ctx* c, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t blocks, int64_t kf, int order,
                          const float* d_c_re, const float* d_c_im, float* d_out_re, float* d_out_im) {
    ForecastApplyArgs a{};
    for (int m = 0; m < order; ++m) { a.x_re[m] = d_x_re[n_snd - 1 - m]; a.x_im[m] = d_x_im[n_snd - 1 - m]; }
    a.c_re = d_c_re; a.c_im = d_c_im; a.y_re = d_out_re; a.y_im = d_out_im;
    a.kf = kf; a.order = order;
    // 8 flop per complex multiply-add; M plane pairs in, one out
    ProfScope ps(c, K_FORECAST_APPLY, (double)blocks * kf * 8.0 * order, (double)blocks * (kf * 8.0 * (order + 1) + 8.0 * order));
    hipLaunchKernelGGL(forecast_apply_kernel<FC_MAX_ORDER>, dim3((unsigned)blocks), dim3(FC_THREADS), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    ++c->forecast_launches;
    return CSI_OK;
}

// ---- entry points
// blocks of kf contiguous floats per plane: csi_forecast_gram_device is the case (npkt Nr, Nt 234) of it
int forecast_gram_blocks_device(csi_ctx* c, const char* who, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t blocks, int64_t kf,
                                float* d_t_re, float* d_t_im) {
    if (n_snd < 2 || n_snd > FC_MAX_SND) return fail(c, CSI_ERR_INVALID_ARG, "%s: n_snd %d outside 2 .. %d", who, n_snd, FC_MAX_SND);
    if (blocks < 0 || blocks > 0x7fffffff) return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld blocks outside 0 .. 2^31 - 1 (one launch)", who, (long long)blocks);
    if (kf < 2 || (kf & 1) || kf > ((int64_t)1 << 40))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: block_floats %lld must be even and at least 2 (blocks start on 8-byte boundaries)", who, (long long)kf);
    if (blocks == 0) return CSI_OK;
    if (int rc = fc_check_planes(c, who, "d_x_re", d_x_re, n_snd)) return rc;
    if (int rc = fc_check_planes(c, who, "d_x_im", d_x_im, n_snd)) return rc;
    if (!d_t_re || !d_t_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (d_t_re, d_t_im)", who);
    const size_t xb = (size_t)blocks * kf * sizeof(float), tb = (size_t)blocks * n_snd * n_snd * sizeof(float);
    const FcPlane outs[] = {{"d_t_re", d_t_re, tb}, {"d_t_im", d_t_im, tb}};
    if (int rc = fc_check_aligned(c, who, outs, 2, 15)) return rc;
    std::vector<FcPlane> ins;
    fc_name_planes(ins, "d_x_re", d_x_re, n_snd, xb);
    fc_name_planes(ins, "d_x_im", d_x_im, n_snd, xb);
    if (int rc = fc_check_disjoint(c, who, outs, 2, ins.data(), (int)ins.size())) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return forecast_gram_launch(c, d_x_re, d_x_im, n_snd, blocks, kf, d_t_re, d_t_im);
}

int forecast_gram_device(csi_ctx* c, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t npkt, float* d_t_re, float* d_t_im) {
    static const char* who = "csi_forecast_gram_device";
    if (int rc = fc_check_shape(c, who, n_snd, npkt)) return rc;
    return forecast_gram_blocks_device(c, who, d_x_re, d_x_im, n_snd, npkt * c->cfg.nr, (int64_t)c->cfg.nt * FC_N, d_t_re, d_t_im);
}

int forecast_fit_device(csi_ctx* c, const float* d_t_re, const float* d_t_im, int n_snd, int64_t npkt, int order, int steps, double ridge, uint32_t flags,
                        float* d_c_re, float* d_c_im, float* d_fit_err, int32_t* d_info) {
    static const char* who = "csi_forecast_fit_device";
    if (int rc = fc_check_shape(c, who, n_snd, npkt)) return rc;
    if (int rc = fc_check_fit(c, who, n_snd, order, steps, ridge, flags)) return rc;
    if (npkt == 0) return CSI_OK;
    if (!d_t_re || !d_t_im || !d_c_re || !d_c_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (d_t_re, d_t_im, d_c_re, d_c_im)", who);
    const size_t blocks = (size_t)npkt * c->cfg.nr, tb = blocks * n_snd * n_snd * sizeof(float), cb = blocks * order * sizeof(float);
    const FcPlane ins[] = {{"d_t_re", d_t_re, tb}, {"d_t_im", d_t_im, tb}};
    const FcPlane outs[] = {{"d_c_re", d_c_re, cb}, {"d_c_im", d_c_im, cb}, {"d_fit_err", d_fit_err, blocks * 4}, {"d_info", d_info, blocks * 4}};
    if (int rc = fc_check_aligned(c, who, ins, 2, 15)) return rc;
    if (int rc = fc_check_aligned(c, who, outs, 4, 3)) return rc;
    if (int rc = fc_check_disjoint(c, who, outs, 4, ins, 2)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return forecast_fit_launch(c, d_t_re, d_t_im, n_snd, npkt, order, steps, ridge, flags, d_c_re, d_c_im, d_fit_err, d_info);
}

// the checks csi_forecast_apply_device and csi_forecast_device share about the soundings and the forecast planes
int fc_check_inout(csi_ctx* c, const char* who, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t npkt, const float* d_c_re,
                   const float* d_c_im, int order, const FcPlane* more_out, int n_more, float* d_out_re, float* d_out_im) {
    if (int rc = fc_check_planes(c, who, "d_x_re", d_x_re, n_snd)) return rc;
    if (int rc = fc_check_planes(c, who, "d_x_im", d_x_im, n_snd)) return rc;
    if (!d_out_re || !d_out_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (d_out_re, d_out_im)", who);
    const size_t blocks = (size_t)npkt * c->cfg.nr, xb = blocks * c->cfg.nt * FC_N * sizeof(float), cb = blocks * order * sizeof(float);
    std::vector<FcPlane> outs = {{"d_out_re", d_out_re, xb}, {"d_out_im", d_out_im, xb}};
    if (int rc = fc_check_aligned(c, who, outs.data(), 2, 15)) return rc;
    for (int i = 0; i < n_more; ++i) outs.push_back(more_out[i]);
    std::vector<FcPlane> ins;
    fc_name_planes(ins, "d_x_re", d_x_re, n_snd, xb);
    fc_name_planes(ins, "d_x_im", d_x_im, n_snd, xb);
    ins.push_back({"d_c_re", d_c_re, cb});
    ins.push_back({"d_c_im", d_c_im, cb});
    return fc_check_disjoint(c, who, outs.data(), (int)outs.size(), ins.data(), (int)ins.size());
}

int forecast_apply_device(csi_ctx* c, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t npkt, int order, const float* d_c_re,
                          const float* d_c_im, float* d_out_re, float* d_out_im) {
    static const char* who = "csi_forecast_apply_device";
    if (int rc = fc_check_shape(c, who, n_snd, npkt)) return rc;
    if (order < 1 || order > FC_MAX_ORDER || order > n_snd)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: order %d outside 1 .. min(%d, n_snd %d)", who, order, FC_MAX_ORDER, n_snd);
    if (npkt == 0) return CSI_OK;
    if (!d_c_re || !d_c_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (d_c_re, d_c_im)", who);
    const FcPlane cs[] = {{"d_c_re", d_c_re, 0}, {"d_c_im", d_c_im, 0}};
    if (int rc = fc_check_aligned(c, who, cs, 2, 3)) return rc;
    if (int rc = fc_check_inout(c, who, d_x_re, d_x_im, n_snd, npkt, d_c_re, d_c_im, order, nullptr, 0, d_out_re, d_out_im)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return forecast_apply_launch(c, d_x_re, d_x_im, n_snd, npkt * c->cfg.nr, (int64_t)c->cfg.nt * FC_N, order, d_c_re, d_c_im, d_out_re, d_out_im);
}

// gram, fit, apply.  T [blocks][P][P] re | im and, when the caller keeps none, c [blocks][M] re | im live in the context (sized by eager
// calls: inside a capture the workspace must already hold the call)
int forecast_device(csi_ctx* c, const char* who, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t npkt, int order, int steps,
                    double ridge, uint32_t flags, float* d_out_re, float* d_out_im, float* d_c_re, float* d_c_im, float* d_fit_err, int32_t* d_info) {
    if (int rc = fc_check_shape(c, who, n_snd, npkt)) return rc;
    if (int rc = fc_check_fit(c, who, n_snd, order, steps, ridge, flags)) return rc;
    if ((d_c_re == nullptr) != (d_c_im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the c planes come as a pair", who);
    if (npkt == 0) return CSI_OK;
    const size_t blocks = (size_t)npkt * c->cfg.nr, cb = blocks * order * sizeof(float);
    const FcPlane more[] = {{"d_c_re", d_c_re, cb}, {"d_c_im", d_c_im, cb}, {"d_fit_err", d_fit_err, blocks * 4}, {"d_info", d_info, blocks * 4}};
    if (int rc = fc_check_aligned(c, who, more, 4, 3)) return rc;
    if (int rc = fc_check_inout(c, who, d_x_re, d_x_im, n_snd, npkt, nullptr, nullptr, order, more, 4, d_out_re, d_out_im)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t tf = (blocks * n_snd * n_snd + 3) / 4 * 4, cfl = (blocks * order + 3) / 4 * 4;      // floats per plane, 16-byte planes
    const size_t need = (2 * tf + 2 * cfl) * sizeof(float);
    if (c->user_capture && c->forecast_ws_bytes < need)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: the workspace of %lld packets is sized by an eager call of the same shape in front of the capture", who,
                    (long long)npkt);
    if (int rc = ensure_bytes(c, &c->forecast_ws, &c->forecast_ws_bytes, need)) return rc;
    float* t_re = reinterpret_cast<float*>(c->forecast_ws);
    float* t_im = t_re + tf;
    float* c_re = d_c_re ? d_c_re : t_im + tf;
    float* c_im = d_c_im ? d_c_im : t_im + tf + cfl;
    const int64_t kf = (int64_t)c->cfg.nt * FC_N;
    if (int rc = forecast_gram_launch(c, d_x_re, d_x_im, n_snd, (int64_t)blocks, kf, t_re, t_im)) return rc;
    if (int rc = forecast_fit_launch(c, t_re, t_im, n_snd, npkt, order, steps, ridge, flags, c_re, c_im, d_fit_err, d_info)) return rc;
    return forecast_apply_launch(c, d_x_re, d_x_im, n_snd, (int64_t)blocks, kf, order, c_re, c_im, d_out_re, d_out_im);
}

// host buffers: one staged plane per sounding and component, the chunk sized by the 2 P + 2 CSI planes of a packet
int forecast_host(csi_ctx* c, const float* const* x_re, const float* const* x_im, int n_snd, int64_t npkt, int order, int steps, double ridge, uint32_t flags,
                  float* out_re, float* out_im, float* c_re, float* c_im, float* fit_err, int32_t* info) {
    static const char* who = "csi_forecast";
    if (int rc = fc_check_shape(c, who, n_snd, npkt)) return rc;
    if (int rc = fc_check_fit(c, who, n_snd, order, steps, ridge, flags)) return rc;
    if ((c_re == nullptr) != (c_im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the c planes come as a pair", who);
    if (npkt == 0) return CSI_OK;
    if (!x_re || !x_im || !out_re || !out_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (x_re, x_im, out_re, out_im)", who);
    for (int i = 0; i < n_snd; ++i)
        if (!x_re[i] || !x_im[i]) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (x_re[%d] / x_im[%d])", who, i, i);
    const csi_config& cf = c->cfg;
    const size_t pkt = (size_t)cf.nr * cf.nt * FC_N * sizeof(float);      // bytes per packet and plane: a multiple of 16 (nt % 4 == 0)
    {      // the host arrays obey the overlap rule of the device entries: a chunk's results go down before the next chunk's soundings go up
        const size_t xb = (size_t)npkt * pkt, cb = (size_t)npkt * cf.nr * order * sizeof(float), sb = (size_t)npkt * cf.nr * 4;
        const FcPlane outs[] = {{"out_re", out_re, xb}, {"out_im", out_im, xb}, {"c_re", c_re, cb}, {"c_im", c_im, cb}, {"fit_err", fit_err, sb}, {"info", info, sb}};
        std::vector<FcPlane> ins;
        fc_name_planes(ins, "x_re", x_re, n_snd, xb);
        fc_name_planes(ins, "x_im", x_im, n_snd, xb);
        if (int rc = fc_check_disjoint(c, who, outs, 6, ins.data(), (int)ins.size())) return rc;
    }
    HIP_TRY(c, hipSetDevice(cf.device));
    constexpr int OUT = 2 * FC_MAX_SND;
    StagePlane p[OUT + 6];
    for (int i = 0; i < FC_MAX_SND; ++i) {
        p[i] = {i < n_snd ? pkt : 0, i < n_snd ? x_re[i] : nullptr, nullptr};
        p[FC_MAX_SND + i] = {i < n_snd ? pkt : 0, i < n_snd ? x_im[i] : nullptr, nullptr};
    }
    p[OUT] = {pkt, nullptr, out_re};
    p[OUT + 1] = {pkt, nullptr, out_im};
    p[OUT + 2] = {(size_t)cf.nr * order * sizeof(float), nullptr, c_re};
    p[OUT + 3] = {(size_t)cf.nr * order * sizeof(float), nullptr, c_im};
    p[OUT + 4] = {(size_t)cf.nr * sizeof(float), nullptr, fit_err};
    p[OUT + 5] = {(size_t)cf.nr * sizeof(int32_t), nullptr, info};
    return staged_call(c, npkt, stage_budget(c), (size_t)(2 * n_snd + 2) * pkt, 0, true, p, [&](int64_t, int64_t np) {
        const float* d_re[FC_MAX_SND];
        const float* d_im[FC_MAX_SND];
        for (int i = 0; i < n_snd; ++i) { d_re[i] = p[i].as<float>(); d_im[i] = p[FC_MAX_SND + i].as<float>(); }
        return forecast_device(c, who, d_re, d_im, n_snd, np, order, steps, ridge, flags, p[OUT].as<float>(), p[OUT + 1].as<float>(), p[OUT + 2].as<float>(),
                               p[OUT + 3].as<float>(), p[OUT + 4].as<float>(), p[OUT + 5].as<int32_t>());
    });
}

int sounding_noise_device(csi_ctx* c, uint64_t seed, int64_t first_pkt, int64_t npkt, const float* d_err_var, const float* d_x_re, const float* d_x_im,
                          float* d_out_re, float* d_out_im) {
    static const char* who = "csi_sounding_noise_device";
    const csi_config& cf = c->cfg;
    if (cf.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no channel forecast");
    if (npkt < 0 || first_pkt < 0)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld / first_pkt %lld must not be negative", who, (long long)npkt, (long long)first_pkt);
    if (npkt * cf.nr > 0x7fffffff)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets x %d rx antennas exceed one launch (2^31 - 1 items)", who, (long long)npkt, cf.nr);
    if (npkt == 0) return CSI_OK;
    if (!d_err_var || !d_x_re || !d_x_im || !d_out_re || !d_out_im)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (d_err_var, d_x_re, d_x_im, d_out_re, d_out_im)", who);
    const size_t blocks = (size_t)npkt * cf.nr, xb = blocks * cf.nt * FC_N * sizeof(float);
    const FcPlane planes[] = {{"d_x_re", d_x_re, xb}, {"d_x_im", d_x_im, xb}, {"d_out_re", d_out_re, xb}, {"d_out_im", d_out_im, xb}};
    if (int rc = fc_check_aligned(c, who, planes, 4, 15)) return rc;
    const FcPlane v[] = {{"d_err_var", d_err_var, blocks * 4}};
    if (int rc = fc_check_aligned(c, who, v, 1, 3)) return rc;
    if (int rc = inout_planes_disjoint(c, who, d_x_re, d_x_im, d_out_re, d_out_im, xb)) return rc;
    if (int rc = fc_check_disjoint(c, who, planes + 2, 2, v, 1)) return rc;
    HIP_TRY(c, hipSetDevice(cf.device));
    SoundingNoiseArgs a{};
    a.x_re = d_x_re; a.x_im = d_x_im; a.y_re = d_out_re; a.y_im = d_out_im; a.v = d_err_var;
    a.seed = seed; a.first_pkt = first_pkt; a.kf = (int64_t)cf.nt * FC_N; a.nr = cf.nr;
    // one fused multiply-add per component; x in, out out
    ProfScope ps(c, K_SOUNDING_NOISE, (double)blocks * a.kf * 4.0, (double)blocks * (a.kf * 16.0 + 4.0));
    hipLaunchKernelGGL(sounding_noise_kernel<0>, dim3((unsigned)blocks), dim3(FC_THREADS), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    ++c->forecast_launches;
    return CSI_OK;
}

}  // namespace
