// csi_subspace.hpp - host side of the delay-subspace smoother (kernel: subspace_smooth.hip.h): the basis and its two
// device images, the argument checks, the one launch of csi_subspace_smooth_device and the host entry point as a staged call.  The
// orthonormality check of the basis and the overlap rule of the planes are csi_stage.hpp's, shared with csi_beam.hpp.
#pragma once
#include "csi_context.hpp"
#include "csi_stage.hpp"
#include "subspace_smooth.hip.h"

namespace {

constexpr double SB_ORTHO_TOL = 1e-4;          // largest |Q^H Q - I| entry a basis may have
constexpr size_t SB_IMAGE_FLOATS = (size_t)2 * SB_N * SB_MAX_RANK + (size_t)2 * SB_MAX_RANK * SB_NP;

int subspace_set_basis(csi_ctx* c, const float* q_re, const float* q_im, int rank) {
    static const char* who = "csi_subspace_set_basis";
    const csi_config& cf = c->cfg;
    if (cf.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no subspace smoother");
    if (rank < 1 || rank > SB_MAX_RANK) return fail(c, CSI_ERR_INVALID_ARG, "%s: rank %d outside 1 .. %d", who, rank, SB_MAX_RANK);
    if (!q_re || !q_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null basis planes", who);
    if (c->user_capture) return fail(c, CSI_ERR_INVALID_ARG, "%s: the basis cannot be replaced while a capture is open", who);
    if (int rc = basis_orthonormal(c, who, q_re, q_im, SB_N, rank, SB_ORTHO_TOL, 'Q')) return rc;
    const int rp = (rank + 31) / 32 * 32;
    std::vector<float> img((size_t)2 * SB_N * rp + (size_t)2 * rp * SB_NP, 0.0f);
    float* qa_re = img.data();
    float* qa_im = qa_re + (size_t)SB_N * rp;
    float* qb_re = qa_im + (size_t)SB_N * rp;
    float* qb_im = qb_re + (size_t)rp * SB_NP;
    for (int k = 0; k < SB_N; ++k)
        for (int j = 0; j < rank; ++j) {
            const float vr = q_re[(size_t)k * rank + j], vi = q_im[(size_t)k * rank + j];
            qa_re[(size_t)k * rp + j] = vr; qa_im[(size_t)k * rp + j] = vi;
            qb_re[(size_t)j * SB_NP + k] = vr; qb_im[(size_t)j * SB_NP + k] = vi;
        }
    HIP_TRY(c, hipSetDevice(cf.device));
    if (!c->sub_q && hipMalloc((void**)&c->sub_q, SB_IMAGE_FLOATS * sizeof(float)) != hipSuccess) {
        c->sub_q = nullptr;
        return fail(c, CSI_ERR_NOMEM, "%s: device allocation of %zu bytes failed", who, SB_IMAGE_FLOATS * sizeof(float));
    }
    const size_t lds = subspace_lds_bytes(SB_MAX_RANK);          // once, for the largest rank: nothing is set inside a capture later
    if (c->sub_lds_attr < lds) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)subspace_smooth_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        c->sub_lds_attr = lds;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));                 // calls in flight still read the old images
    c->sub_rank = 0;
    HIP_TRY(c, hipMemcpy(c->sub_q, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
    c->sub_rank = rank;
    c->sub_rp = rp;
    return CSI_OK;
}

// everything csi_subspace_smooth_device refuses except the alignment of the planes (the caller's: planes_aligned)
int subspace_check(csi_ctx* c, const char* who, const float* h_re, const float* h_im, int64_t npkt, const float* out_re, const float* out_im) {
    const csi_config& cf = c->cfg;
    if (cf.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no subspace smoother");
    if (npkt < 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld must not be negative", who, (long long)npkt);
    if (!h_re || !h_im || !out_re || !out_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (h, out)", who);
    if (c->sub_rank == 0) return fail(c, CSI_ERR_NOT_READY, "%s: no basis set (csi_subspace_set_basis)", who);
    return CSI_OK;
}

int subspace_smooth_device(csi_ctx* c, const char* who, const float* d_h_re, const float* d_h_im, int64_t npkt, const float* d_w,
                           float* d_out_re, float* d_out_im) {
    const csi_config& cf = c->cfg;
    if (npkt == 0) return CSI_OK;
    const int64_t rows = npkt * cf.nr * cf.nt;
    const size_t bytes = (size_t)rows * SB_N * sizeof(float);
    if (int rc = inout_planes_disjoint(c, who, d_h_re, d_h_im, d_out_re, d_out_im, bytes)) return rc;
    const int64_t tiles = (rows + SB_ROWS - 1) / SB_ROWS;
    if (tiles > 0x7fffffff) return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld rows exceed one launch (2^31 - 1 tiles of %d rows)", who, (long long)rows, SB_ROWS);
    HIP_TRY(c, hipSetDevice(cf.device));
    const int rank = c->sub_rank, rp = c->sub_rp;
    SubspaceArgs a{};
    a.x_re = d_h_re; a.x_im = d_h_im; a.y_re = d_out_re; a.y_im = d_out_im; a.w = d_w;
    a.qa_re = c->sub_q;
    a.qa_im = a.qa_re + (size_t)SB_N * rp;
    a.qb_re = a.qa_im + (size_t)SB_N * rp;
    a.qb_im = a.qb_re + (size_t)rp * SB_NP;
    a.rows = rows; a.nt = cf.nt; a.rank = rank; a.rp = rp;
    // two complex products of [234][r] per row, 8 flop per complex multiply-add; x in, y out, w and the two images of Q once
    ProfScope ps(c, K_SUBSPACE_SMOOTH, 16.0 * (double)rows * SB_N * rank,
                 (double)rows * SB_N * 16.0 + (d_w ? (double)npkt * cf.nr * rank * 4.0 : 0.0) + 16.0 * SB_N * rank);
    hipLaunchKernelGGL(subspace_smooth_kernel, dim3((unsigned)tiles), dim3(SB_THREADS), subspace_lds_bytes(rp), c->stream, a);
    HIP_TRY(c, hipGetLastError());
    ++c->subspace_launches;
    return CSI_OK;
}

int subspace_smooth_host(csi_ctx* c, const float* h_re, const float* h_im, int64_t npkt, const float* w, float* out_re, float* out_im) {
    static const char* who = "csi_subspace_smooth";
    if (int rc = subspace_check(c, who, h_re, h_im, npkt, out_re, out_im)) return rc;
    if (npkt == 0) return CSI_OK;
    const csi_config& cf = c->cfg;
    HIP_TRY(c, hipSetDevice(cf.device));
    const size_t pkt = (size_t)cf.nr * cf.nt * SB_N * sizeof(float);      // bytes per packet and plane: a multiple of 16 (nt % 4 == 0)
    // a staged call (csi_stage.hpp): the chunk is sized by the four CSI planes, the weights ride behind them
    StagePlane p[] = {{pkt, h_re, nullptr}, {pkt, h_im, nullptr}, {pkt, nullptr, out_re}, {pkt, nullptr, out_im},
                      {w ? (size_t)cf.nr * c->sub_rank * sizeof(float) : 0, w, nullptr}};
    return staged_call(c, npkt, stage_budget(c), 4 * pkt, 0, true, p, [&](int64_t, int64_t np) {
        return subspace_smooth_device(c, who, p[0].as<float>(), p[1].as<float>(), np, w ? p[4].as<float>() : nullptr, p[2].as<float>(), p[3].as<float>());
    });
}

}  // namespace
