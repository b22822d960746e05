// csi_mu_jsdm.hpp - host side of the multi-user JSDM precoder (kernels: mu_jsdm.hip.h): the argument checks, the one
// launch of csi_mu_covariance_device and the chunked launch sequence of csi_mu_jsdm_precoder_device - per packet chunk one covariance
// launch over (packet, user) (none when the caller hands the covariances in), two eigen launches over (packet, group) and one baseband
// launch over (packet, subcarrier tile).  The covariance, eigenvalue, U*, rank and Frf planes of a chunk live in the context's workspace
// unless the caller keeps them.
#pragma once
#include "csi_context.hpp"
#include "csi_mu.hpp"
#include "csi_mu_hybrid.hpp"
#include "mu_jsdm.hip.h"

namespace {

int mu_jsdm_check_nt(csi_ctx* c, const char* who) {
    if (c->cfg.nt > MJ_MAX_NT)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: Nt %d exceeds %d (the eigen kernel holds the matrix and the vectors in LDS)", who, c->cfg.nt, MJ_MAX_NT);
    return CSI_OK;
}

void mu_cov_launch(csi_ctx* c, const MuJsdmArgs& a, int64_t np) {
    const int nt = a.nt;
    const double items = (double)np * a.n_users;
    // the definition's flops: 8 per complex product-sum term; the planes read once, the covariance written once
    ProfScope ps(c, K_MU_COV, items * 8.0 * nt * nt * a.nr * HY_N, items * ((double)a.nr * nt * HY_N * 8.0 + (double)nt * nt * 8.0));
    if (nt <= 32)
        hipLaunchKernelGGL(mu_cov_kernel<1>, dim3((unsigned)(np * a.n_users)), dim3(MJ_COV_THREADS), mu_cov_lds_bytes(1), c->stream, a);
    else
        hipLaunchKernelGGL(mu_cov_kernel<2>, dim3((unsigned)(np * a.n_users)), dim3(MJ_COV_THREADS), mu_cov_lds_bytes(2), c->stream, a);
    ++c->mu_launches;
}

int mu_covariance_device(csi_ctx* c, int n_users, const float* const* d_hest_re, const float* const* d_hest_im, int64_t npkt, float* d_cov_re,
                         float* d_cov_im) {
    static const char* who = "csi_mu_covariance_device";
    const csi_config& cf = c->cfg;
    if (cf.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no multi-user downlink");
    if (n_users < 1 || n_users > MU_MAX_USERS) return fail(c, CSI_ERR_INVALID_ARG, "%s: n_users %d outside 1 .. %d", who, n_users, MU_MAX_USERS);
    if (int rc = mu_jsdm_check_nt(c, who)) return rc;
    if (npkt < 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld must not be negative", who, (long long)npkt);
    if (npkt > 0x7fffffff / MU_MAX_USERS) return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets exceed one launch (%d)", who, (long long)npkt, 0x7fffffff / MU_MAX_USERS);
    if (npkt == 0) return CSI_OK;
    if (int rc = mu_check_planes(c, who, "d_hest_re", d_hest_re, n_users)) return rc;
    if (int rc = mu_check_planes(c, who, "d_hest_im", d_hest_im, n_users)) return rc;
    if (!d_cov_re || !d_cov_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (cov_re, cov_im)", who);
    if (int rc = mu_check_aligned(c, who, "d_cov_re", d_cov_re)) return rc;
    if (int rc = mu_check_aligned(c, who, "d_cov_im", d_cov_im)) return rc;
    HIP_TRY(c, hipSetDevice(cf.device));
    MuJsdmArgs a{};
    for (int u = 0; u < n_users; ++u) { a.h_re[u] = d_hest_re[u]; a.h_im[u] = d_hest_im[u]; }
    a.cov_re = d_cov_re; a.cov_im = d_cov_im;
    a.nt = cf.nt; a.nr = cf.nr; a.n_users = n_users;
    mu_cov_launch(c, a, npkt);
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

int mu_jsdm_precoder_device(csi_ctx* c, int n_users, const float* const* d_hest_re, const float* const* d_hest_im, int64_t npkt, int ns,
                            const int32_t* group, int r_star, int n_beams, float rank_tol, int flags, const float* d_reg, const float* d_cov_re,
                            const float* d_cov_im, float* d_w_re, float* d_w_im, float* d_frf_re, float* d_frf_im, float* d_fbb_re, float* d_fbb_im,
                            float* d_eig, float* d_ustar_re, float* d_ustar_im, int32_t* d_rank) {
    static const char* who = "csi_mu_jsdm_precoder_device";
    if (int rc = mu_check_shape(c, who, n_users, ns)) return rc;
    const csi_config& cf = c->cfg;
    const int nt = cf.nt, m = n_users * ns;
    if (int rc = mu_jsdm_check_nt(c, who)) return rc;
    // the groups: values 0 .. G-1, every group non-empty
    int n_groups = n_users, members[MU_MAX_USERS] = {};
    signed char grp[MU_MAX_USERS] = {};
    if (group) {
        n_groups = 0;
        for (int u = 0; u < n_users; ++u) {
            if (group[u] < 0 || group[u] >= n_users)
                return fail(c, CSI_ERR_INVALID_ARG, "%s: group[%d] = %d outside 0 .. G-1 (at most %d groups)", who, u, (int)group[u], n_users);
            n_groups = std::max(n_groups, (int)group[u] + 1);
            grp[u] = (signed char)group[u];
            ++members[group[u]];
        }
        for (int g = 0; g < n_groups; ++g)
            if (!members[g]) return fail(c, CSI_ERR_INVALID_ARG, "%s: group %d of 0 .. %d has no user", who, g, n_groups - 1);
    } else {
        for (int u = 0; u < n_users; ++u) { grp[u] = (signed char)u; members[u] = 1; }
    }
    if (n_beams < 1) return fail(c, CSI_ERR_INVALID_ARG, "%s: n_beams %d must be at least 1", who, n_beams);
    const int64_t n_rf64 = (int64_t)n_groups * n_beams;
    if (n_rf64 > HY_MAX_RF) return fail(c, CSI_ERR_INVALID_ARG, "%s: n_rf = G %d x n_beams %d = %lld RF chains exceed %d", who, n_groups, n_beams, (long long)n_rf64, HY_MAX_RF);
    const int n_rf = (int)n_rf64;
    for (int g = 0; g < n_groups; ++g)
        if (ns * members[g] > n_beams)
            return fail(c, CSI_ERR_INVALID_ARG, "%s: group %d has ns %d x %d users = %d streams for n_beams %d chains", who, g, ns, members[g], ns * members[g], n_beams);
    if (r_star < 0 || r_star > nt) return fail(c, CSI_ERR_INVALID_ARG, "%s: r_star %d outside 0 .. Nt %d", who, r_star, nt);
    if ((n_groups - 1) * r_star > nt - n_beams)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: (G - 1) r_star = %d directions to null leave fewer than n_beams %d of Nt %d", who, (n_groups - 1) * r_star, n_beams, nt);
    if (!(rank_tol >= 0.f) || !(rank_tol <= 3.0e38f)) return fail(c, CSI_ERR_INVALID_ARG, "%s: rank_tol %g must be finite and not negative", who, (double)rank_tol);
    if (flags & ~(MJ_FLAG_PGP | MJ_FLAG_UNIT)) return fail(c, CSI_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (bit 0: per-group processing, bit 1: unit modulus)", who, flags);
    if (npkt < 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld must not be negative", who, (long long)npkt);
    if (npkt > 0x7fffffff / std::max(m, 8)) return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets exceed one launch (%d)", who, (long long)npkt, 0x7fffffff / std::max(m, 8));
    const struct { const char* name; const void* re; const void* im; } pairs[] = {{"cov", d_cov_re, d_cov_im}, {"frf", d_frf_re, d_frf_im}, {"fbb", d_fbb_re, d_fbb_im},
                                                                                  {"ustar", d_ustar_re, d_ustar_im}};
    for (const auto& pr : pairs)
        if ((pr.re == nullptr) != (pr.im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the %s planes come as a pair", who, pr.name);
    const int lanes = mu_hybrid_lanes(nt, m, n_rf);
    const size_t lds_e = mu_jsdm_eig_lds_bytes(nt), lds_b = mu_hybrid_lds_bytes(nt, m, n_rf, lanes);
    // a guard only: with Nt <= 64 and M, n_rf <= 16 the 32-lane image is 106 KiB at the most, so no shape that passed the checks above gets here
    if (lds_b > MH_MAX_LDS)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: Nt %d, M %d, n_rf %d need %zu bytes of LDS (160 KiB per workgroup)", who, nt, m, n_rf, lds_b);
    if (npkt == 0) return CSI_OK;
    if (int rc = mu_check_planes(c, who, "d_hest_re", d_hest_re, n_users)) return rc;
    if (int rc = mu_check_planes(c, who, "d_hest_im", d_hest_im, n_users)) return rc;
    if (!d_w_re || !d_w_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (w_re, w_im)", who);
    const struct { const char* name; const void* p; } planes[] = {{"d_cov_re", d_cov_re}, {"d_cov_im", d_cov_im}, {"d_w_re", d_w_re}, {"d_w_im", d_w_im},
                                                                    {"d_frf_re", d_frf_re}, {"d_frf_im", d_frf_im}, {"d_fbb_re", d_fbb_re}, {"d_fbb_im", d_fbb_im},
                                                                    {"d_eig", d_eig}, {"d_ustar_re", d_ustar_re}, {"d_ustar_im", d_ustar_im}};
    for (const auto& pl : planes)
        if (int rc = mu_check_aligned(c, who, pl.name, pl.p)) return rc;
    if ((reinterpret_cast<uintptr_t>(d_reg) & 3) || (reinterpret_cast<uintptr_t>(d_rank) & 3))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: d_reg / d_rank must be aligned for 4-byte words (got %p / %p)", who, (const void*)d_reg, (void*)d_rank);
    // packet chunks against the workspace limit: per packet the covariances, the eigenvalues, U*, the ranks and Frf (each part of a chunk
    // starts on a 256-byte boundary); the size does not depend on which of them the caller keeps
    const size_t b_cov = (size_t)n_users * nt * nt * sizeof(float), b_eig = (size_t)n_groups * nt * sizeof(float),
                 b_us = (size_t)n_groups * nt * r_star * sizeof(float), b_rank = (size_t)n_groups * 2 * sizeof(int32_t),
                 b_frf = (size_t)nt * n_rf * sizeof(float);
    const size_t pkt_bytes = 2 * b_cov + b_eig + 2 * b_us + b_rank + 2 * b_frf;
    const size_t budget = cf.workspace_bytes > 0 ? (size_t)cf.workspace_bytes : ((size_t)1 << 30);
    int64_t chunk = std::max<int64_t>(1, (int64_t)(budget / pkt_bytes));
    const int64_t nchunks = (npkt + chunk - 1) / chunk;
    chunk = (npkt + nchunks - 1) / nchunks;
    const size_t need = pkt_bytes * (size_t)chunk + 8 * 256;
    if (c->user_capture && c->muj_ws_bytes < need)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: the workspace of %lld packets is sized by an eager call of the same shape in front of the capture", who,
                    (long long)npkt);
    HIP_TRY(c, hipSetDevice(cf.device));
    if (int rc = ensure_bytes(c, &c->muj_ws, &c->muj_ws_bytes, need)) return rc;
    const void* fn_b = lanes == 64 ? (const void*)mu_jsdm_baseband_kernel<64> : (const void*)mu_jsdm_baseband_kernel<32>;
    // the dynamic-LDS limits are raised once per context and kernel (never inside a capture that follows an eager call of the shape)
    if (lds_e > 64 * 1024 && c->muj_lds_attr[0] < lds_e) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)mu_jsdm_eig_kernel<MJ_EIG_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_e));
        c->muj_lds_attr[0] = lds_e;
    }
    if (lds_b > 64 * 1024 && c->muj_lds_attr[lanes == 64 ? 1 : 2] < lds_b) {
        HIP_TRY(c, hipFuncSetAttribute(fn_b, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
        c->muj_lds_attr[lanes == 64 ? 1 : 2] = lds_b;
    }
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    char* ws = c->muj_ws;
    float* ws_cov_re = reinterpret_cast<float*>(ws); ws += up(b_cov * (size_t)chunk);
    float* ws_cov_im = reinterpret_cast<float*>(ws); ws += up(b_cov * (size_t)chunk);
    float* ws_eig = reinterpret_cast<float*>(ws); ws += up(b_eig * (size_t)chunk);
    float* ws_us_re = reinterpret_cast<float*>(ws); ws += up(b_us * (size_t)chunk);
    float* ws_us_im = reinterpret_cast<float*>(ws); ws += up(b_us * (size_t)chunk);
    int32_t* ws_rank = reinterpret_cast<int32_t*>(ws); ws += up(b_rank * (size_t)chunk);
    float* ws_frf_re = reinterpret_cast<float*>(ws); ws += up(b_frf * (size_t)chunk);
    float* ws_frf_im = reinterpret_cast<float*>(ws);
    const size_t pkt_h = (size_t)cf.nr * nt * HY_N;
    const int tiles = (HY_N + lanes - 1) / lanes;
    for (int64_t p0 = 0; p0 < npkt; p0 += chunk) {
        const int64_t np = std::min(chunk, npkt - p0);
        MuJsdmArgs a{};
        for (int u = 0; u < n_users; ++u) { a.h_re[u] = d_hest_re[u] + p0 * pkt_h; a.h_im[u] = d_hest_im[u] + p0 * pkt_h; a.group[u] = grp[u]; }
        // the kernels of the later launches only read the covariance planes
        a.cov_re = d_cov_re ? const_cast<float*>(d_cov_re) + (size_t)p0 * n_users * nt * nt : ws_cov_re;
        a.cov_im = d_cov_im ? const_cast<float*>(d_cov_im) + (size_t)p0 * n_users * nt * nt : ws_cov_im;
        a.eig = d_eig ? d_eig + (size_t)p0 * n_groups * nt : ws_eig;
        a.us_re = d_ustar_re ? d_ustar_re + (size_t)p0 * n_groups * nt * r_star : ws_us_re;
        a.us_im = d_ustar_im ? d_ustar_im + (size_t)p0 * n_groups * nt * r_star : ws_us_im;
        a.rank = d_rank ? d_rank + (size_t)p0 * n_groups * 2 : ws_rank;
        a.frf_re = d_frf_re ? d_frf_re + (size_t)p0 * nt * n_rf : ws_frf_re;
        a.frf_im = d_frf_im ? d_frf_im + (size_t)p0 * nt * n_rf : ws_frf_im;
        a.reg = d_reg ? d_reg + p0 : nullptr;
        a.w_re = d_w_re + (size_t)p0 * m * nt * HY_N; a.w_im = d_w_im + (size_t)p0 * m * nt * HY_N;
        a.fbb_re = d_fbb_re ? d_fbb_re + (size_t)p0 * HY_N * n_rf * m : nullptr;
        a.fbb_im = d_fbb_im ? d_fbb_im + (size_t)p0 * HY_N * n_rf * m : nullptr;
        a.rank_tol = rank_tol;
        a.nt = nt; a.nr = cf.nr; a.ns = ns; a.n_users = n_users; a.n_groups = n_groups; a.r_star = r_star; a.b = n_beams; a.flags = flags;
        if (!d_cov_re) {
            mu_cov_launch(c, a, np);
            HIP_TRY(c, hipGetLastError());
        }
        for (int stage = 1; stage <= 2; ++stage) {
            a.stage = stage;
            // the sweeps a matrix takes are the kernel's own business (its stop rule), so no flop count is claimed: the entry carries time
            // and bytes - the covariances read, the planes written
            const double mats = (double)np * n_groups;
            ProfScope ps(c, K_MU_JSDM_EIG, 0.0,
                         mats * ((double)nt * nt * 8.0 * (double)n_users / n_groups + (double)nt * 4.0 + (double)nt * (stage == 1 ? r_star : n_beams) * 8.0));
            hipLaunchKernelGGL(mu_jsdm_eig_kernel<MJ_EIG_THREADS>, dim3((unsigned)(np * n_groups)), dim3(MJ_EIG_THREADS), lds_e, c->stream, a);
            HIP_TRY(c, hipGetLastError());
            ++c->mu_launches;
        }
        {
            // Gm, the Gram matrix, the factor, two substitutions per column, V twice; B read once, W (and Fbb) written once
            const double items = (double)np * HY_N;
            ProfScope ps(c, K_MU_JSDM_BASEBAND,
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
