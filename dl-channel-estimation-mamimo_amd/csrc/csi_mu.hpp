// csi_mu.hpp - host side of the multi-user downlink (kernels: mu_link.hip.h): the argument checks, the one launch of
// csi_mu_precoder_device and the chunked launch sequence of csi_mu_link_sim_device (per chunk: one encoder launch per user, one
// transmit / receive launch over (packet, user), one decoder launch per user - the decoder regenerates the information bits of ONE
// stream per launch).
#pragma once
#include "csi_context.hpp"
#include "csi_link.hpp"
#include "mu_link.hip.h"

namespace {

uint64_t mu_splitmix64(uint64_t x) {      // rng.hip.h, on the host
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// seed_0 = seed: user 0 is the user of csi_link_sim_device
uint64_t mu_user_seed(uint64_t seed, int u) { return u == 0 ? seed : mu_splitmix64(seed ^ mu_splitmix64((uint64_t)u)); }

// the shape checks both entry points share, in the same words
int mu_check_shape(csi_ctx* c, const char* who, int n_users, int ns) {
    const int nt = c->cfg.nt, nr = c->cfg.nr;
    if (nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no multi-user downlink");
    if (n_users < 1 || n_users > MU_MAX_USERS) return fail(c, CSI_ERR_INVALID_ARG, "%s: n_users %d outside 1 .. %d", who, n_users, MU_MAX_USERS);
    if (ns < 1 || ns > std::min(LK_MAX_NS, nr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: ns %d outside 1 .. min(%d, Nr %d)", who, ns, LK_MAX_NS, nr);
    const int m = n_users * ns;
    if (m > MU_MAX_STREAMS || m > nt)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: M = n_users %d x ns %d = %d streams exceed min(%d, Nt %d)", who, n_users, ns, m, MU_MAX_STREAMS, nt);
    return CSI_OK;
}

// a host array of n_users device planes: no null entry, every plane on a 16-byte boundary
int mu_check_planes(csi_ctx* c, const char* who, const char* name, const float* const* planes, int n_users) {
    if (!planes) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (%s)", who, name);
    for (int u = 0; u < n_users; ++u) {
        if (!planes[u]) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (%s[%d])", who, name, u);
        if (reinterpret_cast<uintptr_t>(planes[u]) & 15)
            return fail(c, CSI_ERR_INVALID_ARG, "%s: %s[%d] must start on a 16-byte boundary (got %p)", who, name, u, (const void*)planes[u]);
    }
    return CSI_OK;
}

int mu_check_aligned(csi_ctx* c, const char* who, const char* name, const void* p) {
    if (reinterpret_cast<uintptr_t>(p) & 15) return fail(c, CSI_ERR_INVALID_ARG, "%s: %s must start on a 16-byte boundary (got %p)", who, name, p);
    return CSI_OK;
}

int mu_precoder_device(csi_ctx* c, int n_users, const float* const* d_hest_re, const float* const* d_hest_im, int64_t npkt, int ns,
                       const float* d_reg, float* d_w_re, float* d_w_im) {
    static const char* who = "csi_mu_precoder_device";
    if (int rc = mu_check_shape(c, who, n_users, ns)) return rc;
    const csi_config& cf = c->cfg;
    const int nt = cf.nt, m = n_users * ns;
    if (npkt < 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld must not be negative", who, (long long)npkt);
    if (npkt > 0x7fffffff / MU_PRE_TILES) return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets exceed one launch (%d)", who, (long long)npkt, 0x7fffffff / MU_PRE_TILES);
    const size_t lds = mu_precoder_lds_bytes(m);
    if (lds > LK_MAX_LDS) return fail(c, CSI_ERR_INVALID_ARG, "%s: M %d needs %zu bytes of LDS (160 KiB per workgroup)", who, m, lds);
    if (npkt == 0) return CSI_OK;
    if (int rc = mu_check_planes(c, who, "d_hest_re", d_hest_re, n_users)) return rc;
    if (int rc = mu_check_planes(c, who, "d_hest_im", d_hest_im, n_users)) return rc;
    if (!d_w_re || !d_w_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (w_re, w_im)", who);
    if (int rc = mu_check_aligned(c, who, "d_w_re", d_w_re)) return rc;
    if (int rc = mu_check_aligned(c, who, "d_w_im", d_w_im)) return rc;
    if (reinterpret_cast<uintptr_t>(d_reg) & 3) return fail(c, CSI_ERR_INVALID_ARG, "%s: d_reg must be aligned for floats (got %p)", who, (const void*)d_reg);
    HIP_TRY(c, hipSetDevice(cf.device));
    if (lds > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void*)mu_precoder_kernel<MU_PRE_LANES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    MuPrecoderArgs a{};
    for (int u = 0; u < n_users; ++u) { a.h_re[u] = d_hest_re[u]; a.h_im[u] = d_hest_im[u]; }
    a.reg = d_reg; a.w_re = d_w_re; a.w_im = d_w_im;
    a.nt = nt; a.nr = cf.nr; a.ns = ns; a.n_users = n_users;
    const double items = (double)npkt * LK_N;
    ProfScope ps(c, K_MU_PRECODER, items * 8.0 * ((double)nt * m * (m + 1) / 2 + (double)m * m * m / 6 + (double)nt * m * m),
                 items * 8.0 * ((double)2 * m * nt + (double)3 * m * nt));
    hipLaunchKernelGGL(mu_precoder_kernel<MU_PRE_LANES>, dim3((unsigned)(npkt * MU_PRE_TILES)), dim3(MU_PRE_LANES), lds, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    ++c->mu_launches;
    return CSI_OK;
}

template <int NS>
const void* mu_txrx_fn(int bps) { return bps == 2 ? (const void*)mu_txrx_kernel<NS, 1> : (const void*)mu_txrx_kernel<NS, 2>; }

int mu_link_sim_device(csi_ctx* c, int n_users, const float* const* d_h_re, const float* const* d_h_im, const float* d_w_re, const float* d_w_im,
                       const float* d_noise_var, uint64_t seed, int64_t first_pkt, int64_t npkt, int ns, int n_sym, int bps,
                       int32_t* d_bit_errors, float* d_evm_rms, float* d_sinr_db, float* d_g_re, float* d_g_im, float* d_xeq_re, float* d_xeq_im,
                       float* d_csi, float* d_llr, uint8_t* d_bits) {
    static const char* who = "csi_mu_link_sim_device";
    if (int rc = mu_check_shape(c, who, n_users, ns)) return rc;
    const csi_config& cf = c->cfg;
    const int nt = cf.nt, nr = cf.nr, m = n_users * ns;
    if (npkt < 0 || first_pkt < 0)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld / first_pkt %lld must not be negative", who, (long long)npkt, (long long)first_pkt);
    if (bps != 2 && bps != 4) return fail(c, CSI_ERR_INVALID_ARG, "%s: bps %d is not 2 (QPSK) or 4 (16-QAM)", who, bps);
    if (n_sym < 1) return fail(c, CSI_ERR_INVALID_ARG, "%s: n_sym %d must be at least 1", who, n_sym);
    int64_t n_info = 0, n_coded = 0;
    link_frame(ns, n_sym, bps, &n_info, &n_coded);
    const int64_t n_steps = n_coded / 3;
    if (n_steps > LK_MAX_STEPS)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: n_steps %lld = ns %d x n_sym %d x 234 x bps %d / 3 exceeds %d (one codeword per packet and user, 8 bytes of LDS per step)",
                    who, (long long)n_steps, ns, n_sym, bps, LK_MAX_STEPS);
    if ((d_g_re == nullptr) != (d_g_im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the g planes come as a pair", who);
    if ((d_xeq_re == nullptr) != (d_xeq_im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the xeq planes come as a pair", who);
    if (npkt > 0x7fffffff) return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets exceed one launch (2^31 - 1)", who, (long long)npkt);
    const size_t lds = mu_txrx_lds_bytes(ns, m);
    if (lds > LK_MAX_LDS) return fail(c, CSI_ERR_INVALID_ARG, "%s: ns %d, M %d need %zu bytes of LDS (160 KiB per workgroup)", who, ns, m, lds);
    if (npkt == 0) return CSI_OK;
    if (int rc = mu_check_planes(c, who, "d_h_re", d_h_re, n_users)) return rc;
    if (int rc = mu_check_planes(c, who, "d_h_im", d_h_im, n_users)) return rc;
    if (!d_w_re || !d_w_im || !d_noise_var || !d_bit_errors || !d_evm_rms || !d_sinr_db)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (w, noise_var, bit_errors, evm_rms, sinr_db)", who);
    const struct { const char* name; const void* p; } planes[] = {{"d_w_re", d_w_re}, {"d_w_im", d_w_im}, {"d_g_re", d_g_re}, {"d_g_im", d_g_im},
                                                                    {"d_xeq_re", d_xeq_re}, {"d_xeq_im", d_xeq_im}};
    for (const auto& pl : planes)
        if (int rc = mu_check_aligned(c, who, pl.name, pl.p)) return rc;
    HIP_TRY(c, hipSetDevice(cf.device));
    const void* fn = ns == 1 ? mu_txrx_fn<1>(bps) : ns == 2 ? mu_txrx_fn<2>(bps) : ns == 3 ? mu_txrx_fn<3>(bps) : mu_txrx_fn<4>(bps);
    if (lds > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // packet chunks against the workspace limit: per packet the U codewords' coded bits and, when the caller keeps none, their soft bits.
    // (W is the caller's array in this interface: it has no share of the workspace.)
    const size_t coded_b = ((size_t)n_coded + 15) / 16 * 16;
    const size_t llr_b = d_llr ? 0 : (size_t)n_coded * sizeof(float);
    const size_t pkt_bytes = (size_t)n_users * (coded_b + llr_b);
    const size_t budget = cf.workspace_bytes > 0 ? (size_t)cf.workspace_bytes : ((size_t)1 << 30);
    int64_t chunk = std::max<int64_t>(1, (int64_t)(budget / pkt_bytes));
    const int64_t nchunks = (npkt + chunk - 1) / chunk;
    chunk = (npkt + nchunks - 1) / nchunks;
    int rc = ensure_bytes(c, &c->link_ws, &c->link_ws_bytes, pkt_bytes * (size_t)chunk + 256);
    if (rc) return rc;
    const size_t pkt_h = (size_t)nr * nt * LK_N;
    for (int64_t p0 = 0; p0 < npkt; p0 += chunk) {
        const int64_t np = std::min(chunk, npkt - p0);
        uint8_t* coded = reinterpret_cast<uint8_t*>(c->link_ws);
        float* ws_llr = reinterpret_cast<float*>(c->link_ws + coded_b * (size_t)chunk * n_users);
        MuLinkArgs a{};
        for (int u = 0; u < n_users; ++u) {
            a.h_re[u] = d_h_re[u] + p0 * pkt_h; a.h_im[u] = d_h_im[u] + p0 * pkt_h;
            a.seed[u] = mu_user_seed(seed, u);
        }
        a.w_re = d_w_re + (size_t)p0 * m * nt * LK_N; a.w_im = d_w_im + (size_t)p0 * m * nt * LK_N;
        a.noise_var = d_noise_var + p0;
        a.coded = coded;
        a.llr = d_llr ? d_llr + (size_t)p0 * n_coded : ws_llr;
        a.llr_pkts = d_llr ? npkt : chunk;
        a.g_re = d_g_re ? d_g_re + (size_t)p0 * ns * m * LK_N : nullptr;
        a.g_im = d_g_im ? d_g_im + (size_t)p0 * ns * m * LK_N : nullptr;
        a.xeq_re = d_xeq_re ? d_xeq_re + (size_t)p0 * ns * n_sym * LK_N : nullptr;
        a.xeq_im = d_xeq_im ? d_xeq_im + (size_t)p0 * ns * n_sym * LK_N : nullptr;
        a.csi = d_csi ? d_csi + (size_t)p0 * ns * LK_N : nullptr;
        a.evm_rms = d_evm_rms + p0; a.sinr_db = d_sinr_db + p0;
        a.first_pkt = first_pkt + p0;
        a.out_pkts = npkt; a.ws_pkts = chunk; a.coded_stride = (size_t)n_coded;      // link_encode_kernel packs the codewords
        a.nt = nt; a.nr = nr; a.n_users = n_users; a.n_sym = n_sym;
        {
            const double items = (double)np * LK_N * n_users;
            ProfScope ps(c, K_MU_TXRX, items * (8.0 * nt * ns * m + (double)n_sym * 8.0 * ns * (m + ns)),
                         items * (ns + m) * nt * 8.0 + (double)np * n_users * n_coded * (4.0 + n_users));
            const int64_t steps = np * n_steps;
            for (int u = 0; u < n_users; ++u) {
                hipLaunchKernelGGL(link_encode_kernel, dim3((unsigned)((steps + 255) / 256)), dim3(256), 0, c->stream,
                                   coded + (size_t)u * chunk * n_coded, a.seed[u], a.first_pkt, np, (int)n_steps);
                HIP_TRY(c, hipGetLastError());
            }
            void* kargs[] = {&a};
            HIP_TRY(c, hipLaunchKernel(fn, dim3((unsigned)np, (unsigned)n_users), dim3(LK_THREADS), kargs, lds, c->stream));
            c->mu_launches += n_users + 1;
        }
        for (int u = 0; u < n_users; ++u) {
            ViterbiArgs v{};
            v.llr = a.llr + (size_t)u * a.llr_pkts * n_coded;
            v.bits = d_bits ? d_bits + ((size_t)u * npkt + p0) * n_info : nullptr;
            v.bit_errors = d_bit_errors + (size_t)u * npkt + p0;
            v.seed = a.seed[u]; v.first_pkt = a.first_pkt; v.n_steps = (int)n_steps;
            ProfScope ps(c, K_LINK_VITERBI, (double)np * n_steps * 64.0 * 5.0, (double)np * n_steps * 13.0);
            hipLaunchKernelGGL(link_viterbi_kernel, dim3((unsigned)np), dim3(64), (size_t)n_steps * sizeof(unsigned long long), c->stream, v);
            HIP_TRY(c, hipGetLastError());
            ++c->mu_launches;
        }
    }
    return CSI_OK;
}

}  // namespace
