// csi_feedback.hpp - host side of the quantised CSI feedback (kernels: feedback.hip.h): the argument checks, the chunked
// launch of csi_feedback_compress_device, the bin-centre tables on the context and the one launch of csi_feedback_expand_device.
#pragma once
#include "csi_context.hpp"
#include "csi_mu.hpp"
#include "feedback.hip.h"

namespace {

// the checks both entry points share, in the same words
int fb_check_shape(csi_ctx* c, const char* who, int64_t npkt, int nc, int b_phi, int b_psi, int ng) {
    const int nt = c->cfg.nt, nr = c->cfg.nr;
    if (nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no CSI feedback");
    if (nc < 1 || nc > std::min(FB_MAX_NC, std::min(nr, nt)))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: nc %d outside 1 .. min(%d, Nr %d, Nt %d)", who, nc, FB_MAX_NC, nr, nt);
    if (nr > HY_MAX_NR) return fail(c, CSI_ERR_INVALID_ARG, "%s: Nr %d > %d is not supported by the singular-vector routine", who, nr, HY_MAX_NR);
    if (ng != 1 && ng != 2 && ng != 4) return fail(c, CSI_ERR_INVALID_ARG, "%s: ng %d is not 1, 2 or 4", who, ng);
    if ((b_phi == 0) != (b_psi == 0))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: b_phi %d and b_psi %d: only one of them is 0 (0, 0 asks for continuous angles)", who, b_phi, b_psi);
    if (b_phi != 0 && (b_phi < FB_MIN_BPHI || b_phi > FB_MAX_BPHI))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: b_phi %d outside %d .. %d", who, b_phi, FB_MIN_BPHI, FB_MAX_BPHI);
    if (b_psi != 0 && (b_psi < FB_MIN_BPSI || b_psi > FB_MAX_BPSI))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: b_psi %d outside %d .. %d", who, b_psi, FB_MIN_BPSI, FB_MAX_BPSI);
    if (npkt < 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld must not be negative", who, (long long)npkt);
    return CSI_OK;
}

// lanes per workgroup: the most of 64, 32, 16, 8 whose LDS image fits 64 KiB; 8 lanes with a larger image where none does
int fb_lanes(size_t fixed_bytes, size_t lane_bytes, size_t* image) {
    int lanes = 64;
    while (lanes > 8 && fixed_bytes + lane_bytes * lanes > 64 * 1024) lanes /= 2;
    *image = fixed_bytes + lane_bytes * lanes;
    return lanes;
}

int fb_check_word(csi_ctx* c, const char* who, const char* name, const void* p, int bytes) {
    if (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: %s must be aligned for %d-byte words (got %p)", who, name, bytes, p);
    return CSI_OK;
}

int feedback_compress_device(csi_ctx* c, const float* d_h_re, const float* d_h_im, int64_t npkt, int nc, int b_phi, int b_psi, int ng,
                             uint16_t* d_phi_code, uint16_t* d_psi_code, float* d_phi, float* d_psi, float* d_sigma, float* d_v_re,
                             float* d_v_im) {
    static const char* who = "csi_feedback_compress_device";
    if (int rc = fb_check_shape(c, who, npkt, nc, b_phi, b_psi, ng)) return rc;
    const csi_config& cf = c->cfg;
    const int nt = cf.nt, nr = cf.nr;
    const int n_rep = (HY_N + ng - 1) / ng, n_ang = fb_n_angles(nt, nc);
    // per lane: the fp64 matrices of the singular-vector step (4 nr^2 doubles), then the Nt x nc matrix in the same slots
    const size_t lane_bytes = sizeof(double) * std::max((size_t)4 * nr * nr, (size_t)nt * nc);
    size_t lds = 0;
    const int tpb = fb_lanes(0, lane_bytes, &lds);
    if (lds > FB_MAX_LDS)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: Nt %d, Nr %d, nc %d need %zu bytes of LDS (160 KiB per workgroup)", who, nt, nr, nc, lds);
    if (npkt == 0) return CSI_OK;
    if (!d_h_re || !d_h_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (h_re, h_im)", who);
    if ((d_phi_code == nullptr) != (d_psi_code == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the code arrays d_phi_code / d_psi_code come as a pair", who);
    if ((d_phi == nullptr) != (d_psi == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the angle arrays d_phi / d_psi come as a pair", who);
    if ((d_v_re == nullptr) != (d_v_im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the v planes come as a pair", who);
    if (b_phi != 0 && !d_phi_code) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (d_phi_code, d_psi_code)", who);
    if (b_phi == 0 && !d_phi) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (d_phi, d_psi: b_phi = b_psi = 0 asks for them)", who);
    const struct { const char* name; const void* p; } planes[] = {{"d_h_re", d_h_re}, {"d_h_im", d_h_im}, {"d_v_re", d_v_re}, {"d_v_im", d_v_im}};
    for (const auto& pl : planes)
        if (int rc = mu_check_aligned(c, who, pl.name, pl.p)) return rc;
    if (int rc = fb_check_word(c, who, "d_phi_code", d_phi_code, 2)) return rc;
    if (int rc = fb_check_word(c, who, "d_psi_code", d_psi_code, 2)) return rc;
    if (int rc = fb_check_word(c, who, "d_phi", d_phi, 4)) return rc;
    if (int rc = fb_check_word(c, who, "d_psi", d_psi, 4)) return rc;
    if (int rc = fb_check_word(c, who, "d_sigma", d_sigma, 4)) return rc;
    // packet chunks against the workspace limit: per report the singular vectors (two planes) and the two state words of hyb_svd_item
    const size_t pkt_bytes = ((size_t)2 * nc * nt * sizeof(float) + 2 * sizeof(int)) * n_rep;
    const size_t budget = cf.workspace_bytes > 0 ? (size_t)cf.workspace_bytes : ((size_t)1 << 30);
    int64_t chunk = std::max<int64_t>(1, (int64_t)(budget / pkt_bytes));
    chunk = std::min(chunk, (int64_t)0x7fffffff / (2 * HY_N));          // item numbers fit an int
    const int64_t nchunks = (npkt + chunk - 1) / chunk;
    chunk = (npkt + nchunks - 1) / nchunks;
    const size_t need = pkt_bytes * (size_t)chunk + 256;
    if (c->user_capture && c->fb_ws_bytes < need)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: the workspace of %lld packets is sized by an eager call of the same shape in front of the capture", who,
                    (long long)npkt);
    HIP_TRY(c, hipSetDevice(cf.device));
    if (int rc = ensure_bytes(c, &c->fb_ws, &c->fb_ws_bytes, need)) return rc;
    if (lds > 64 * 1024 && c->fb_lds_attr[0] < lds) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)fb_compress_kernel<FB_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        c->fb_lds_attr[0] = lds;
    }
    const size_t pkt_h = (size_t)nr * nt * HY_N;
    for (int64_t p0 = 0; p0 < npkt; p0 += chunk) {
        const int64_t np = std::min(chunk, npkt - p0);
        const size_t n = (size_t)np * n_rep;
        FbCompressArgs a{};
        a.h_re = d_h_re + p0 * pkt_h; a.h_im = d_h_im + p0 * pkt_h;
        float* w = reinterpret_cast<float*>(c->fb_ws);
        a.ws_re = w; w += (size_t)nc * nt * n;
        a.ws_im = w; w += (size_t)nc * nt * n;
        a.ws_state = reinterpret_cast<int*>(w);
        const size_t ang0 = (size_t)p0 * n_ang * n_rep;
        a.phi_code = d_phi_code ? d_phi_code + ang0 : nullptr; a.psi_code = d_psi_code ? d_psi_code + ang0 : nullptr;
        a.phi = d_phi ? d_phi + ang0 : nullptr; a.psi = d_psi ? d_psi + ang0 : nullptr;
        a.sigma = d_sigma ? d_sigma + (size_t)p0 * nc * n_rep : nullptr;
        a.v_re = d_v_re ? d_v_re + (size_t)p0 * nc * nt * n_rep : nullptr;
        a.v_im = d_v_im ? d_v_im + (size_t)p0 * nc * nt * n_rep : nullptr;
        a.nt = nt; a.nr = nr; a.nc = nc; a.ng = ng; a.n_rep = n_rep; a.n_ang = n_ang; a.n = (int)n;
        a.b_phi = b_phi; a.b_psi = b_psi;
        a.phi_scale = b_phi ? (float)(std::ldexp(1.0, b_phi - 1) / M_PI) : 0.0f;
        a.psi_scale = b_psi ? (float)(std::ldexp(1.0, b_psi + 1) / M_PI) : 0.0f;
        // the singular-vector step as csi_hybrid_weights_device counts it, then 6 nc flops per rotation and phase; H read once
        const double items = (double)n;
        ProfScope ps(c, K_FB_COMPRESS, items * (4.0 * nr * (nr + 1) * nt + 8.0 * nc * nr * nt + HY_SWEEPS * 12.0 * nr * nr * nr + 12.0 * nc * n_ang),
                     (double)np * pkt_h * 8.0 + items * ((d_v_re ? 8.0 * nc * nt : 0.0) + (b_phi ? 4.0 : 0.0) * n_ang + (d_phi ? 8.0 : 0.0) * n_ang));
        hipLaunchKernelGGL(fb_compress_kernel<FB_THREADS>, dim3((unsigned)((n + tpb - 1) / tpb)), dim3(tpb), lds, c->stream, a, tpb);
        HIP_TRY(c, hipGetLastError());
        ++c->feedback_launches;
    }
    return CSI_OK;
}

// cos / sin of the bin centres, computed in double and rounded to fp32: cos phi [2^b_phi], sin phi, cos psi [2^b_psi], sin psi
void fb_centre_tables(int b_phi, int b_psi, std::vector<float>* tab) {
    const int n_phi = 1 << b_phi, n_psi = 1 << b_psi;
    tab->resize((size_t)2 * (n_phi + n_psi));
    for (int k = 0; k < n_phi; ++k) {
        const double x = M_PI * (std::ldexp(1.0, -b_phi) + (double)k * std::ldexp(1.0, 1 - b_phi));
        (*tab)[k] = (float)std::cos(x);
        (*tab)[n_phi + k] = (float)std::sin(x);
    }
    for (int k = 0; k < n_psi; ++k) {
        const double x = M_PI * (std::ldexp(1.0, -(b_psi + 2)) + (double)k * std::ldexp(1.0, -(b_psi + 1)));
        (*tab)[2 * n_phi + k] = (float)std::cos(x);
        (*tab)[2 * n_phi + n_psi + k] = (float)std::sin(x);
    }
}

int feedback_expand_device(csi_ctx* c, const uint16_t* d_phi_code, const uint16_t* d_psi_code, const float* d_phi, const float* d_psi,
                           const float* d_sigma, int64_t npkt, int nc, int b_phi, int b_psi, int ng, int layout, float* d_out_re,
                           float* d_out_im) {
    static const char* who = "csi_feedback_expand_device";
    if (int rc = fb_check_shape(c, who, npkt, nc, b_phi, b_psi, ng)) return rc;
    if (layout != FB_LAYOUT_W && layout != FB_LAYOUT_CSI)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: layout %d is not CSI_FB_LAYOUT_W (0) or CSI_FB_LAYOUT_CSI (1)", who, layout);
    const csi_config& cf = c->cfg;
    const int nt = cf.nt, nr = cf.nr;
    const int n_rep = (HY_N + ng - 1) / ng, n_ang = fb_n_angles(nt, nc);
    const bool coded = d_phi_code || d_psi_code;
    const int n_tab = coded && b_phi ? 2 * ((1 << b_phi) + (1 << b_psi)) : 0;      // no tables with continuous angles
    size_t lds = 0;
    const int tpb = fb_lanes((size_t)n_tab * sizeof(float), (size_t)2 * nt * nc * sizeof(float), &lds);
    if (lds > FB_MAX_LDS) return fail(c, CSI_ERR_INVALID_ARG, "%s: Nt %d, nc %d need %zu bytes of LDS (160 KiB per workgroup)", who, nt, nc, lds);
    const int tiles = (HY_N + tpb - 1) / tpb;
    if (npkt > 0x7fffffff / tiles) return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets exceed one launch (%d)", who, (long long)npkt, 0x7fffffff / tiles);
    if (npkt == 0) return CSI_OK;
    if ((d_phi_code == nullptr) != (d_psi_code == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the code arrays d_phi_code / d_psi_code come as a pair", who);
    if ((d_phi == nullptr) != (d_psi == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the angle arrays d_phi / d_psi come as a pair", who);
    if (coded == (d_phi != nullptr))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: exactly one of the pairs (d_phi_code, d_psi_code) and (d_phi, d_psi) is given", who);
    if (coded && b_phi == 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: codes need their bit widths (b_phi %d, b_psi %d)", who, b_phi, b_psi);
    if (!d_out_re || !d_out_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (out_re, out_im)", who);
    if (int rc = mu_check_aligned(c, who, "d_out_re", d_out_re)) return rc;
    if (int rc = mu_check_aligned(c, who, "d_out_im", d_out_im)) return rc;
    if (int rc = fb_check_word(c, who, "d_phi_code", d_phi_code, 2)) return rc;
    if (int rc = fb_check_word(c, who, "d_psi_code", d_psi_code, 2)) return rc;
    if (int rc = fb_check_word(c, who, "d_phi", d_phi, 4)) return rc;
    if (int rc = fb_check_word(c, who, "d_psi", d_psi, 4)) return rc;
    if (int rc = fb_check_word(c, who, "d_sigma", d_sigma, 4)) return rc;
    HIP_TRY(c, hipSetDevice(cf.device));
    if (coded && (c->fb_tab_bphi != b_phi || c->fb_tab_bpsi != b_psi)) {
        if (c->user_capture)
            return fail(c, CSI_ERR_INVALID_ARG, "%s: the tables of (b_phi %d, b_psi %d) are uploaded by an eager call in front of the capture", who, b_phi, b_psi);
        std::vector<float> tab;
        fb_centre_tables(b_phi, b_psi, &tab);
        drop_graphs(c);                                   // captured launches were recorded with the old tables
        HIP_TRY(c, hipStreamSynchronize(c->stream));      // earlier launches may still read them
        if (!c->fb_tab) {
            const size_t bytes = (size_t)2 * ((1 << FB_MAX_BPHI) + (1 << FB_MAX_BPSI)) * sizeof(float);
            if (hipMalloc((void**)&c->fb_tab, bytes) != hipSuccess) {
                c->fb_tab = nullptr;
                return fail(c, CSI_ERR_NOMEM, "%s: device allocation of %zu bytes failed", who, bytes);
            }
        }
        c->fb_tab_bphi = c->fb_tab_bpsi = 0;
        HIP_TRY(c, hipMemcpy(c->fb_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
        c->fb_tab_bphi = b_phi; c->fb_tab_bpsi = b_psi;
    }
    if (lds > 64 * 1024 && c->fb_lds_attr[1] < lds) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)fb_expand_kernel<FB_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        c->fb_lds_attr[1] = lds;
    }
    FbExpandArgs a{};
    a.phi_code = d_phi_code; a.psi_code = d_psi_code; a.phi = d_phi; a.psi = d_psi; a.sigma = d_sigma;
    a.tab = coded ? c->fb_tab : nullptr;
    a.out_re = d_out_re; a.out_im = d_out_im;
    a.nt = nt; a.nr = nr; a.nc = nc; a.ng = ng; a.n_rep = n_rep; a.n_ang = n_ang;
    a.b_phi = coded ? b_phi : 0; a.b_psi = coded ? b_psi : 0;
    a.layout = layout; a.tiles = tiles;
    a.scale = (float)std::sqrt((double)nt / nc);
    const double items = (double)npkt * HY_N, rows = layout == FB_LAYOUT_W ? nc : nr;
    ProfScope ps(c, K_FB_EXPAND, items * 12.0 * nc * n_ang, items * (8.0 * rows * nt + (coded ? 4.0 : 8.0) * n_ang / ng));
    hipLaunchKernelGGL(fb_expand_kernel<FB_THREADS>, dim3((unsigned)(npkt * tiles)), dim3(tpb), lds, c->stream, a, tpb, n_tab);
    HIP_TRY(c, hipGetLastError());
    ++c->feedback_launches;
    return CSI_OK;
}

}  // namespace
