// csi_lmmse.hpp - host side of the LMMSE smoothers (kernels: lmmse.hip.h): the argument checks and launches of
// csi_lmmse_estimate_device (statistics handed in), csi_lmmse_blind_device (statistics from the packet itself) and csi_null_noise_device
// (the null-carrier statistic on its own), and the two staged host entry points.  The alignment refusals of the device forms stay with
// their extern "C" wrappers (csi_mamimo.hip: planes_aligned).
#pragma once
#include "csi_context.hpp"
#include "csi_stage.hpp"

namespace {

// ---------------------------------------------------------------- statistics handed in: h_vec and SNR per packet
int lmmse_estimate_check(csi_ctx* c, const float* d_h_re, const float* d_h_im, int64_t npkt, const float* d_hvec, int L, const float* d_snr_db,
                         const float* d_out_re, const float* d_out_im) {
    if (c->cfg.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no LMMSE estimate");
    if (npkt < 0 || L < 1 || (npkt > 0 && (!d_h_re || !d_h_im || !d_hvec || !d_snr_db || !d_out_re || !d_out_im)))
        return fail(c, CSI_ERR_INVALID_ARG, "csi_lmmse_estimate_device: bad argument");
    return CSI_OK;
}

int lmmse_estimate_launch(csi_ctx* c, const float* d_h_re, const float* d_h_im, int64_t npkt, const float* d_hvec, int L, const float* d_snr_db,
                          float* d_out_re, float* d_out_im) {
    const csi_config& cf = c->cfg;
    HIP_TRY(c, hipSetDevice(cf.device));
    const int n_jc = (cf.nt + LM_RHS - 1) / LM_RHS;
    const int64_t nblk = npkt * cf.nr;
    const int64_t max_items = ((int64_t)1 << 30) / n_jc / cf.nr * cf.nr;      // whole packets per launch
    for (int64_t b0 = 0; b0 < nblk; b0 += max_items) {
        const int64_t nb = std::min(max_items, nblk - b0);
        LmmseArgs a{};
        a.h_re = d_h_re + (size_t)b0 * cf.nt * LM_N;
        a.h_im = d_h_im + (size_t)b0 * cf.nt * LM_N;
        a.hvec = d_hvec + (size_t)(b0 / cf.nr) * L;
        a.snr_db = d_snr_db + b0;
        a.o_re = d_out_re + (size_t)b0 * cf.nt * LM_N;
        a.o_im = d_out_im + (size_t)b0 * cf.nt * LM_N;
        a.nt = cf.nt; a.nr = cf.nr; a.L = L;
        // per right-hand side: 2 * n^2 complex multiply-adds = 16 n^2 flop (fp64)
        ProfScope ps(c, K_LMMSE, (double)nb * (cf.nt + n_jc) * 16.0 * LM_N * LM_N, (double)nb * cf.nt * LM_N * 16.0);
        hipLaunchKernelGGL(lmmse_levinson_kernel, dim3((unsigned)(nb * n_jc)), dim3(LM_THREADS), 0, c->stream, a, n_jc);
        HIP_TRY(c, hipGetLastError());
    }
    return CSI_OK;
}

// the chunk is sized by the four CSI planes; hvec and snr_db ride behind them
int lmmse_estimate_host(csi_ctx* c, const float* h_re, const float* h_im, int64_t npkt, const float* hvec, int L, const float* snr_db,
                        float* out_re, float* out_im) {
    if (npkt < 0 || L < 1 || (npkt > 0 && (!h_re || !h_im || !hvec || !snr_db || !out_re || !out_im)))
        return fail(c, CSI_ERR_INVALID_ARG, "csi_lmmse_estimate: bad argument");
    if (npkt == 0) return CSI_OK;
    const csi_config& cf = c->cfg;
    HIP_TRY(c, hipSetDevice(cf.device));
    const size_t pkt = (size_t)cf.nr * cf.nt * LM_N * sizeof(float);       // bytes per packet and plane
    StagePlane p[] = {{pkt, h_re, nullptr}, {pkt, h_im, nullptr}, {pkt, nullptr, out_re}, {pkt, nullptr, out_im},
                      {(size_t)L * sizeof(float), hvec, nullptr}, {(size_t)cf.nr * sizeof(float), snr_db, nullptr}};
    return staged_call(c, npkt, STAGE_BUDGET, 4 * pkt, 0, true, p, [&](int64_t, int64_t np) {
        return csi_lmmse_estimate_device(c, p[0].as<float>(), p[1].as<float>(), np, p[4].as<float>(), L, p[5].as<float>(), p[2].as<float>(), p[3].as<float>());
    });
}

// ---------------------------------------------------------------- statistics from the packet itself (lmmse.hip.h, second half)
// the null-carrier noise statistic of the blocks [b0, b0 + nb): one launch
int lmmse_null_noise_launch(csi_ctx* c, const float* d_ltf_re, const float* d_ltf_im, int64_t b0, int64_t nb, double* d_noise_var) {
    const csi_config& cf = c->cfg;
    LmmseNoiseArgs a{};
    a.ltf_re = d_ltf_re + (size_t)b0 * cf.len_ltf; a.ltf_im = d_ltf_im + (size_t)b0 * cf.len_ltf;
    a.tw = c->lmb_tw; a.nv = d_noise_var + b0; a.nt = cf.nt; a.len_ltf = cf.len_ltf;
    // per (symbol, null bin): 256 complex multiply-adds in fp64 pairs = 4 x 11 flop each
    ProfScope ps(c, K_LMMSE_NULL_NOISE, (double)nb * cf.nt * LMB_NULLS * LMB_FFT * 44.0, (double)nb * cf.nt * LMB_FFT * 8.0);
    hipLaunchKernelGGL(lmmse_null_noise_kernel, dim3((unsigned)nb), dim3(LMB_THREADS), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

// what csi_lmmse_blind_device refuses except the alignment of its pointers
int lmmse_blind_check(csi_ctx* c, const char* who, const float* d_ltf_re, const float* d_ltf_im, const float* d_h_re, const float* d_h_im, int64_t npkt,
                      const float* d_out_re, const float* d_out_im) {
    const csi_config& cf = c->cfg;
    if (cf.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no LMMSE estimate");
    if (npkt <= 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld must be positive", who, (long long)npkt);
    if (!d_ltf_re || !d_ltf_im || !d_h_re || !d_h_im || !d_out_re || !d_out_im)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (ltf, h, out)", who);
    if (cf.len_ltf < LMB_SYM * cf.nt || cf.len_ltf % 4 != 0)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: len_ltf %d does not hold %d sounding symbols of 320 samples in 16-byte words", who, cf.len_ltf, cf.nt);
    return CSI_OK;
}

int lmmse_blind_launch(csi_ctx* c, const float* d_ltf_re, const float* d_ltf_im, const float* d_h_re, const float* d_h_im, int64_t npkt,
                       float* d_out_re, float* d_out_im, double* d_noise_var, double* d_corr) {
    const csi_config& cf = c->cfg;
    HIP_TRY(c, hipSetDevice(cf.device));
    const int n_jc = (cf.nt + LM_RHS - 1) / LM_RHS;
    const int64_t nblk = npkt * cf.nr;
    // the statistics the caller does not keep, and the fallback flags, live in the context ([nblk] nv | [nblk][234] c | [nblk] flags)
    const size_t ws_need = (size_t)nblk * (sizeof(double) + LM_N * sizeof(cd) + sizeof(int));
    if (int rc = ensure_bytes(c, &c->lmb_ws, &c->lmb_ws_bytes, ws_need)) return rc;
    double* nv = d_noise_var ? d_noise_var : reinterpret_cast<double*>(c->lmb_ws);
    cd* corr = d_corr ? reinterpret_cast<cd*>(d_corr) : reinterpret_cast<cd*>(c->lmb_ws + (size_t)nblk * sizeof(double));
    int* flags = reinterpret_cast<int*>(c->lmb_ws + (size_t)nblk * (sizeof(double) + LM_N * sizeof(cd)));
    const int64_t max_items = ((int64_t)1 << 30) / n_jc / cf.nr * cf.nr;      // whole packets per launch
    for (int64_t b0 = 0; b0 < nblk; b0 += max_items) {
        const int64_t nb = std::min(max_items, nblk - b0);
        const size_t ho = (size_t)b0 * cf.nt * LM_N;
        if (int rc = lmmse_null_noise_launch(c, d_ltf_re, d_ltf_im, b0, nb, nv)) return rc;
        {
            LmmseCorrArgs a{};
            a.h_re = d_h_re + ho; a.h_im = d_h_im + ho; a.corr = corr + (size_t)b0 * LM_N; a.nt = cf.nt;
            ProfScope ps(c, K_LMMSE_FREQ_CORR, (double)nb * cf.nt * (LM_N * (LM_N + 1) / 2) * 8.0, (double)nb * cf.nt * LM_N * 8.0);
            hipLaunchKernelGGL(lmmse_freq_corr_kernel, dim3((unsigned)nb), dim3(LMB_THREADS), 0, c->stream, a);
            HIP_TRY(c, hipGetLastError());
        }
        {
            LmmseBlindArgs a{};
            a.h_re = d_h_re + ho; a.h_im = d_h_im + ho; a.nv = nv + b0; a.corr = corr + (size_t)b0 * LM_N;
            a.o_re = d_out_re + ho; a.o_im = d_out_im + ho; a.fallback = flags + b0; a.nt = cf.nt; a.nr = cf.nr;
            ProfScope ps(c, K_LMMSE_BLIND, (double)nb * (cf.nt + n_jc) * 16.0 * LM_N * LM_N, (double)nb * cf.nt * LM_N * 16.0);
            hipLaunchKernelGGL(lmmse_blind_kernel, dim3((unsigned)(nb * n_jc)), dim3(LM_THREADS), 0, c->stream, a, n_jc);
            HIP_TRY(c, hipGetLastError());
            hipLaunchKernelGGL(lmmse_blind_count_kernel, dim3(1), dim3(LMB_THREADS), 0, c->stream, flags + b0, (long long)nb, c->lmb_count);
            HIP_TRY(c, hipGetLastError());
        }
    }
    return CSI_OK;
}

// the chunk is sized by the four CSI planes, as in lmmse_estimate_host; the statistics are staged whether the caller keeps them or not.
// The double planes lie behind float planes of whole packets: on a multiple of 8 bytes
int lmmse_blind_host(csi_ctx* c, const float* ltf_re, const float* ltf_im, const float* h_re, const float* h_im, int64_t npkt, float* out_re,
                     float* out_im, double* noise_var, double* corr) {
    if (npkt <= 0) return fail(c, CSI_ERR_INVALID_ARG, "csi_lmmse_blind: npkt %lld must be positive", (long long)npkt);
    if (!ltf_re || !ltf_im || !h_re || !h_im || !out_re || !out_im)
        return fail(c, CSI_ERR_INVALID_ARG, "csi_lmmse_blind: null required pointer (ltf, h, out)");
    const csi_config& cf = c->cfg;
    if (cf.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no LMMSE estimate");
    HIP_TRY(c, hipSetDevice(cf.device));
    const size_t pkt = (size_t)cf.nr * cf.nt * LM_N * sizeof(float);       // bytes per packet and CSI plane
    const size_t ltf = (size_t)cf.nr * cf.len_ltf * sizeof(float);         // bytes per packet and preamble plane
    StagePlane p[] = {{ltf, ltf_re, nullptr}, {ltf, ltf_im, nullptr}, {pkt, h_re, nullptr}, {pkt, h_im, nullptr}, {pkt, nullptr, out_re}, {pkt, nullptr, out_im},
                      {(size_t)cf.nr * sizeof(double), nullptr, noise_var}, {(size_t)cf.nr * 2 * LM_N * sizeof(double), nullptr, corr}};
    return staged_call(c, npkt, STAGE_BUDGET, 4 * pkt, 0, true, p, [&](int64_t, int64_t np) {
        return csi_lmmse_blind_device(c, p[0].as<float>(), p[1].as<float>(), p[2].as<float>(), p[3].as<float>(), np, p[4].as<float>(), p[5].as<float>(),
                                      p[6].as<double>(), p[7].as<double>());
    });
}

// ---------------------------------------------------------------- the null-carrier statistic on its own
int null_noise_check(csi_ctx* c, const char* who, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt, const double* d_noise_var) {
    const csi_config& cf = c->cfg;
    if (cf.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no sounding symbols");
    if (npkt < 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld must not be negative", who, (long long)npkt);
    if (!d_ltf_re || !d_ltf_im || !d_noise_var) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (ltf, noise_var)", who);
    if (cf.len_ltf < LMB_SYM * cf.nt || cf.len_ltf % 4 != 0)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: len_ltf %d does not hold %d sounding symbols of 320 samples in 16-byte words", who, cf.len_ltf, cf.nt);
    return CSI_OK;
}

// lmmse_null_noise_launch as lmmse_blind_launch calls it: the same kernel, the same launch shape, the same bits
int null_noise_launch(csi_ctx* c, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt, double* d_noise_var) {
    const csi_config& cf = c->cfg;
    HIP_TRY(c, hipSetDevice(cf.device));
    const int64_t nblk = npkt * cf.nr;
    const int64_t max_items = ((int64_t)1 << 30) / cf.nr * cf.nr;      // whole packets per launch
    for (int64_t b0 = 0; b0 < nblk; b0 += max_items)
        if (int rc = lmmse_null_noise_launch(c, d_ltf_re, d_ltf_im, b0, std::min(max_items, nblk - b0), d_noise_var)) return rc;
    return CSI_OK;
}

}  // namespace
