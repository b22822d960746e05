// csi_rx_combine.hpp - host side of receive combining (kernels: rx_combine.hip.h): the argument checks and the launches of
// csi_rx_combiner_device and csi_rx_apply_combiner_device.  Neither uses workspace: a launch depends on its own arguments only.
#pragma once
#include "csi_context.hpp"
#include "csi_mu.hpp"
#include "csi_feedback.hpp"
#include "rx_combine.hip.h"

namespace {

// the checks both entry points share, in the same words
int rxc_check_shape(csi_ctx* c, const char* who, int64_t npkt, int ns) {
    const int nt = c->cfg.nt, nr = c->cfg.nr;
    if (nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no receive combining");
    if (ns < 1 || ns > std::min(RXC_MAX_NS, nr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: ns %d outside 1 .. min(%d, Nr %d)", who, ns, RXC_MAX_NS, nr);
    if (nr > HY_MAX_NR) return fail(c, CSI_ERR_INVALID_ARG, "%s: Nr %d > %d is not supported by the singular-vector routine", who, nr, HY_MAX_NR);
    if (npkt < 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld must not be negative", who, (long long)npkt);
    return CSI_OK;
}

int rx_combiner_device(csi_ctx* c, const float* d_hest_re, const float* d_hest_im, int64_t npkt, int ns, float* d_c_re, float* d_c_im,
                       float* d_sigma) {
    static const char* who = "csi_rx_combiner_device";
    if (int rc = rxc_check_shape(c, who, npkt, ns)) return rc;
    const csi_config& cf = c->cfg;
    const int nt = cf.nt, nr = cf.nr;
    // per lane the fp64 Gram matrix and its eigenvectors: 4 nr^2 doubles
    size_t lds = 0;
    const int tpb = fb_lanes(0, sizeof(double) * (size_t)4 * nr * nr, &lds);
    if (lds > RXC_MAX_LDS) return fail(c, CSI_ERR_INVALID_ARG, "%s: Nr %d needs %zu bytes of LDS (160 KiB per workgroup)", who, nr, lds);
    if (npkt == 0) return CSI_OK;
    if (!d_hest_re || !d_hest_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (hest_re, hest_im)", who);
    if ((d_c_re == nullptr) != (d_c_im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the c planes come as a pair", who);
    if (!d_c_re) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (c_re, c_im)", who);
    const struct { const char* name; const void* p; } planes[] = {{"d_hest_re", d_hest_re}, {"d_hest_im", d_hest_im}, {"d_c_re", d_c_re}, {"d_c_im", d_c_im}};
    for (const auto& pl : planes)
        if (int rc = mu_check_aligned(c, who, pl.name, pl.p)) return rc;
    if (int rc = fb_check_word(c, who, "d_sigma", d_sigma, 4)) return rc;
    HIP_TRY(c, hipSetDevice(cf.device));
    if (lds > 64 * 1024 && c->rxc_lds_attr < lds) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)rx_combiner_kernel<RXC_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        c->rxc_lds_attr = lds;
    }
    // item numbers fit an int: launches of at most this many packets (an item's result depends on its own planes only)
    const int64_t chunk = (int64_t)0x7fffffff / (2 * HY_N);
    const size_t pkt_h = (size_t)nr * nt * HY_N, pkt_c = (size_t)ns * nr * HY_N;
    for (int64_t p0 = 0; p0 < npkt; p0 += chunk) {
        const int64_t np = std::min(chunk, npkt - p0);
        const size_t n = (size_t)np * HY_N;
        RxCombinerArgs a{};
        a.h_re = d_hest_re + p0 * pkt_h; a.h_im = d_hest_im + p0 * pkt_h;
        a.c_re = d_c_re + p0 * pkt_c; a.c_im = d_c_im + p0 * pkt_c;
        a.sigma = d_sigma ? d_sigma + (size_t)p0 * ns * HY_N : nullptr;
        a.nt = nt; a.nr = nr; a.ns = ns; a.n = (int)n;
        // the Gram matrix and the Jacobi sweeps as csi_hybrid_weights_device counts them, then the phase and the rows; H read once
        const double items = (double)n;
        ProfScope ps(c, K_RX_COMBINER, items * (4.0 * nr * (nr + 1) * nt + HY_SWEEPS * 12.0 * nr * nr * nr + 16.0 * ns * nr),
                     (double)np * pkt_h * 8.0 + items * (8.0 * ns * nr + (d_sigma ? 4.0 * ns : 0.0)));
        hipLaunchKernelGGL(rx_combiner_kernel<RXC_THREADS>, dim3((unsigned)((n + tpb - 1) / tpb)), dim3(tpb), lds, c->stream, a, tpb);
        HIP_TRY(c, hipGetLastError());
        ++c->combine_launches;
    }
    return CSI_OK;
}

template <int NS>
void rx_apply_launch(csi_ctx* c, const RxApplyArgs& a, bool reg, unsigned blocks, size_t lds) {
    if (reg) hipLaunchKernelGGL((rx_apply_kernel<NS, true>), dim3(blocks), dim3(RXC_THREADS), 0, c->stream, a);
    else hipLaunchKernelGGL((rx_apply_kernel<NS, false>), dim3(blocks), dim3(RXC_THREADS), lds, c->stream, a);
}

int rx_apply_combiner_device(csi_ctx* c, const float* d_c_re, const float* d_c_im, const float* d_h_re, const float* d_h_im, int64_t npkt, int ns,
                             float* d_e_re, float* d_e_im) {
    static const char* who = "csi_rx_apply_combiner_device";
    if (int rc = rxc_check_shape(c, who, npkt, ns)) return rc;
    const csi_config& cf = c->cfg;
    const int nt = cf.nt, nr = cf.nr;
    const bool reg = ns * nr <= RXC_REG_ELEMS;
    const size_t lds = reg ? 0 : (size_t)2 * ns * nr * RXC_THREADS * sizeof(float);
    if (lds > RXC_MAX_LDS) return fail(c, CSI_ERR_INVALID_ARG, "%s: Nr %d, ns %d need %zu bytes of LDS (160 KiB per workgroup)", who, nr, ns, lds);
    const int tiles = (HY_N + RXC_THREADS - 1) / RXC_THREADS;
    if (npkt > 0x7fffffff / tiles) return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets exceed one launch (%d)", who, (long long)npkt, 0x7fffffff / tiles);
    if (npkt == 0) return CSI_OK;
    if ((d_c_re == nullptr) != (d_c_im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the c planes come as a pair", who);
    if ((d_h_re == nullptr) != (d_h_im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the h planes come as a pair", who);
    if ((d_e_re == nullptr) != (d_e_im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the e planes come as a pair", who);
    if (!d_c_re) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (c_re, c_im)", who);
    if (!d_h_re) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (h_re, h_im)", who);
    if (!d_e_re) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (e_re, e_im)", who);
    const struct { const char* name; const void* p; } planes[] = {{"d_c_re", d_c_re}, {"d_c_im", d_c_im}, {"d_h_re", d_h_re}, {"d_h_im", d_h_im},
                                                                  {"d_e_re", d_e_re}, {"d_e_im", d_e_im}};
    for (const auto& pl : planes)
        if (int rc = mu_check_aligned(c, who, pl.name, pl.p)) return rc;
    HIP_TRY(c, hipSetDevice(cf.device));
    RxApplyArgs a{};
    a.c_re = d_c_re; a.c_im = d_c_im; a.h_re = d_h_re; a.h_im = d_h_im; a.e_re = d_e_re; a.e_im = d_e_im;
    a.nt = nt; a.nr = nr; a.ns = ns; a.tiles = tiles;
    // memory-bound: H read once and E, of the same size, written once, C read once; 8 flops per complex product
    const double items = (double)npkt * HY_N;
    ProfScope ps(c, K_RX_COMBINE, items * 8.0 * ns * nr * nt, items * (2.0 * 8.0 * nr * nt + 8.0 * ns * nr));
    const unsigned blocks = (unsigned)(npkt * tiles);
    if (ns == 1) rx_apply_launch<1>(c, a, reg, blocks, lds);
    else if (ns == 2) rx_apply_launch<2>(c, a, reg, blocks, lds);
    else if (ns == 3) rx_apply_launch<3>(c, a, reg, blocks, lds);
    else rx_apply_launch<4>(c, a, reg, blocks, lds);
    HIP_TRY(c, hipGetLastError());
    ++c->combine_launches;
    return CSI_OK;
}

}  // namespace
