// csi_mu_hybrid.hpp - host side of the multi-user hybrid precoder (kernels: mu_hybrid.hip.h): the argument checks and the
// chunked launch sequence of csi_mu_hybrid_precoder_device - per packet chunk one score launch over (packet, stream), one selection launch
// over the packets and one baseband launch over (packet, subcarrier tile).
#pragma once
#include "csi_context.hpp"
#include "csi_mu.hpp"
#include "mu_hybrid.hip.h"

namespace {

// lanes of the baseband kernel's workgroup: the tile that keeps more subcarriers resident on a CU's 160 KiB - a whole wave for small
// images, half of one where a second or third workgroup then fits (M = 8, n_rf = 16: 3 x 32 lanes against 1 x 64) and at the caps,
// where 64 lanes do not fit at all.  The arithmetic of a lane does not depend on the choice
int mu_hybrid_lanes(int nt, int m, int n_rf) {
    const size_t l64 = mu_hybrid_lds_bytes(nt, m, n_rf, 64), l32 = mu_hybrid_lds_bytes(nt, m, n_rf, 32);
    if (l64 > MH_MAX_LDS) return 32;
    return (MH_MAX_LDS / l32) * 32 > (MH_MAX_LDS / l64) * 64 ? 32 : 64;
}

int mu_hybrid_precoder_device(csi_ctx* c, int n_users, const float* const* d_hest_re, const float* const* d_hest_im, int64_t npkt, int ns,
                              int n_rf, const float* d_reg, float* d_w_re, float* d_w_im, int32_t* d_idx, float* d_fbb_re, float* d_fbb_im,
                              float* d_score) {
    static const char* who = "csi_mu_hybrid_precoder_device";
    if (int rc = mu_check_shape(c, who, n_users, ns)) return rc;
    const csi_config& cf = c->cfg;
    const int nt = cf.nt, m = n_users * ns;
    if (!c->hyb_at_re) return fail(c, CSI_ERR_NOT_READY, "%s: no dictionary set (csi_hybrid_set_dictionary)", who);
    const int rays = c->hyb_rays, rp = c->hyb_rp;
    const int rf_max = std::min(std::min(HY_MAX_RF, nt), rays);
    if (n_rf < m || n_rf > rf_max)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: n_rf %d outside M %d .. min(%d, Nt %d, rays %d)", who, n_rf, m, HY_MAX_RF, nt, rays);
    if (npkt < 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld must not be negative", who, (long long)npkt);
    if (npkt > 0x7fffffff / std::max(m, 8)) return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets exceed one launch (%d)", who, (long long)npkt, 0x7fffffff / std::max(m, 8));
    if ((d_fbb_re == nullptr) != (d_fbb_im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the fbb planes come as a pair", who);
    const int lanes = mu_hybrid_lanes(nt, m, n_rf);
    const size_t lds_s = mu_score_lds_bytes(nt), lds_b = mu_hybrid_lds_bytes(nt, m, n_rf, lanes);
    if (lds_s > MH_MAX_LDS) return fail(c, CSI_ERR_INVALID_ARG, "%s: Nt %d needs %zu bytes of LDS for a dictionary tile (160 KiB per workgroup)", who, nt, lds_s);
    if (lds_b > MH_MAX_LDS)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: Nt %d, M %d, n_rf %d need %zu bytes of LDS (160 KiB per workgroup)", who, nt, m, n_rf, lds_b);
    if (npkt == 0) return CSI_OK;
    if (int rc = mu_check_planes(c, who, "d_hest_re", d_hest_re, n_users)) return rc;
    if (int rc = mu_check_planes(c, who, "d_hest_im", d_hest_im, n_users)) return rc;
    if (!d_w_re || !d_w_im || !d_idx) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (w_re, w_im, idx)", who);
    const struct { const char* name; const void* p; } planes[] = {{"d_w_re", d_w_re}, {"d_w_im", d_w_im}, {"d_fbb_re", d_fbb_re}, {"d_fbb_im", d_fbb_im},
                                                                    {"d_score", d_score}};
    for (const auto& pl : planes)
        if (int rc = mu_check_aligned(c, who, pl.name, pl.p)) return rc;
    if ((reinterpret_cast<uintptr_t>(d_reg) & 3) || (reinterpret_cast<uintptr_t>(d_idx) & 3))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: d_reg / d_idx must be aligned for 4-byte words (got %p / %p)", who, (const void*)d_reg, (void*)d_idx);
    // packet chunks against the workspace limit: the score planes of a chunk live there when the caller keeps none
    const size_t pkt_bytes = (size_t)m * rays * sizeof(float);
    int64_t chunk = npkt;
    if (!d_score) {
        const size_t budget = cf.workspace_bytes > 0 ? (size_t)cf.workspace_bytes : ((size_t)1 << 30);
        chunk = std::max<int64_t>(1, (int64_t)(budget / pkt_bytes));
        const int64_t nchunks = (npkt + chunk - 1) / chunk;
        chunk = (npkt + nchunks - 1) / nchunks;
        const size_t need = pkt_bytes * (size_t)chunk + 256;
        if (c->user_capture && c->muh_ws_bytes < need)
            return fail(c, CSI_ERR_INVALID_ARG, "%s: the workspace of %lld packets is sized by an eager call of the same shape in front of the capture", who,
                        (long long)npkt);
    }
    HIP_TRY(c, hipSetDevice(cf.device));
    if (!d_score)
        if (int rc = ensure_bytes(c, &c->muh_ws, &c->muh_ws_bytes, pkt_bytes * (size_t)chunk + 256)) return rc;
    const void* fn_b = lanes == 64 ? (const void*)mu_hybrid_precoder_kernel<64> : (const void*)mu_hybrid_precoder_kernel<32>;
    // the dynamic-LDS limits are raised once per context and kernel (never inside a capture that follows an eager call of the shape)
    if (lds_s > 64 * 1024 && c->muh_lds_attr[0] < lds_s) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)mu_beam_score_kernel<MH_SCORE_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_s));
        c->muh_lds_attr[0] = lds_s;
    }
    if (lds_b > 64 * 1024 && c->muh_lds_attr[lanes == 64 ? 1 : 2] < lds_b) {
        HIP_TRY(c, hipFuncSetAttribute(fn_b, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
        c->muh_lds_attr[lanes == 64 ? 1 : 2] = lds_b;
    }
    const size_t pkt_h = (size_t)cf.nr * nt * HY_N;
    const int tiles = (HY_N + lanes - 1) / lanes;
    for (int64_t p0 = 0; p0 < npkt; p0 += chunk) {
        const int64_t np = std::min(chunk, npkt - p0);
        MuHybridArgs a{};
        for (int u = 0; u < n_users; ++u) { a.h_re[u] = d_hest_re[u] + p0 * pkt_h; a.h_im[u] = d_hest_im[u] + p0 * pkt_h; }
        a.at_re = c->hyb_at_re; a.at_im = c->hyb_at_im;
        a.reg = d_reg ? d_reg + p0 : nullptr;
        a.score = d_score ? d_score + (size_t)p0 * m * rays : reinterpret_cast<float*>(c->muh_ws);
        a.idx = d_idx + (size_t)p0 * n_rf;
        a.w_re = d_w_re + (size_t)p0 * m * nt * HY_N; a.w_im = d_w_im + (size_t)p0 * m * nt * HY_N;
        a.fbb_re = d_fbb_re ? d_fbb_re + (size_t)p0 * HY_N * n_rf * m : nullptr;
        a.fbb_im = d_fbb_im ? d_fbb_im + (size_t)p0 * HY_N * n_rf * m : nullptr;
        a.nt = nt; a.nr = cf.nr; a.ns = ns; a.n_users = n_users; a.n_rf = n_rf; a.rays = rays; a.rp = rp;
        const double items = (double)np * HY_N;
        {
            // the definition's flops: 8 per complex product-sum term, 3 per squared magnitude added; the rows of B once per ray tile
            ProfScope ps(c, K_MU_BEAM_SCORE, items * m * rays * (8.0 * nt + 3.0),
                         items * m * nt * 8.0 * (rp / HY_RAY_TILE) + (double)np * m * (rays * 4.0 + (double)nt * rp * 8.0));
            hipLaunchKernelGGL(mu_beam_score_kernel<MH_SCORE_THREADS>, dim3((unsigned)(np * m)), dim3(MH_SCORE_THREADS), lds_s, c->stream, a);
            HIP_TRY(c, hipGetLastError());
            ++c->mu_launches;
        }
        {
            // one comparison per (slot, ray); the stream's score row once per slot
            ProfScope ps(c, K_MU_BEAM_SELECT, (double)np * n_rf * rays, (double)np * n_rf * (rays * 4.0 + 4.0));
            hipLaunchKernelGGL(mu_beam_select_kernel<MH_SELECT_THREADS>, dim3((unsigned)np), dim3(MH_SELECT_THREADS), 0, c->stream, a);
            HIP_TRY(c, hipGetLastError());
            ++c->mu_launches;
        }
        {
            // G, the Gram matrix, the factor, two substitutions per column, V twice; B read once, W (and Fbb) written once
            ProfScope ps(c, K_MU_HYBRID_PRECODER,
                         items * 8.0 * ((double)nt * m * n_rf + (double)n_rf * m * (m + 1) / 2 + (double)m * m * m / 6 + (double)n_rf * m * m + 2.0 * nt * m * n_rf),
                         items * 8.0 * ((double)2 * m * nt + (d_fbb_re ? (double)n_rf * m : 0.0)) + (double)np * tiles * nt * n_rf * 8.0);
            void* kargs[] = {&a};
            HIP_TRY(c, hipLaunchKernel(fn_b, dim3((unsigned)(np * tiles)), dim3((unsigned)lanes), kargs, lds_b, c->stream));
            ++c->mu_launches;
        }
    }
    return CSI_OK;
}

}  // namespace
