// csi_link.hpp - host side of the link simulation (kernels: link_sim.hip.h): frame sizes, the argument checks and
// the chunked launch sequence of csi_link_sim_device and csi_link_sim_rx_device (one sequence, two transmit / receive kernels), and the
// decoder alone (csi_viterbi_decode_device).
#pragma once
#include "csi_context.hpp"
#include "link_sim.hip.h"

namespace {

// n_coded = ns n_sym 234 bps coded bits, n_steps = n_coded / 3 trellis steps, n_info = n_steps - 6; false when an argument is out of range
bool link_frame(int ns, int n_sym, int bps, int64_t* n_info, int64_t* n_coded) {
    if (ns < 1 || ns > LK_MAX_NS || n_sym < 1 || (bps != 2 && bps != 4)) return false;
    const int64_t nc = (int64_t)ns * n_sym * LK_N * bps;
    if (n_info) *n_info = nc / 3 - LK_TAIL;
    if (n_coded) *n_coded = nc;
    return true;
}

int viterbi_launch(csi_ctx* c, const float* d_llr, int64_t ncw, int n_steps, uint8_t* d_bits, int32_t* d_errors, uint64_t seed, int64_t first_pkt) {
    ViterbiArgs v{};
    v.llr = d_llr; v.bits = d_bits; v.bit_errors = d_errors; v.seed = seed; v.first_pkt = first_pkt; v.n_steps = n_steps;
    ProfScope ps(c, K_LINK_VITERBI, (double)ncw * n_steps * 64.0 * 5.0, (double)ncw * n_steps * 13.0);
    hipLaunchKernelGGL(link_viterbi_kernel, dim3((unsigned)ncw), dim3(64), (size_t)n_steps * sizeof(unsigned long long), c->stream, v);
    HIP_TRY(c, hipGetLastError());
    ++c->link_launches;
    return CSI_OK;
}

int viterbi_decode_device(csi_ctx* c, const float* d_llr, int64_t ncw, int64_t n_steps, uint8_t* d_bits) {
    static const char* who = "csi_viterbi_decode_device";
    if (ncw < 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: ncw %lld is negative", who, (long long)ncw);
    if (n_steps <= LK_TAIL || n_steps > LK_MAX_STEPS)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: n_steps %lld outside %d .. %d (six tail steps; 8 bytes of LDS per step)", who, (long long)n_steps,
                    LK_TAIL + 1, LK_MAX_STEPS);
    if (ncw > 0x7fffffff) return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld codewords exceed one launch (2^31 - 1)", who, (long long)ncw);
    if (ncw > 0 && (!d_llr || !d_bits)) return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (llr, bits)", who);
    if (ncw == 0) return CSI_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return viterbi_launch(c, d_llr, ncw, (int)n_steps, d_bits, nullptr, 0, 0);
}

template <int NS>
const void* link_txrx_fn(int bps) { return bps == 2 ? (const void*)link_txrx_kernel<NS, 1> : (const void*)link_txrx_kernel<NS, 2>; }

template <int NS>
const void* link_txrx_rx_fn(int bps) { return bps == 2 ? (const void*)link_txrx_rx_kernel<NS, 1> : (const void*)link_txrx_rx_kernel<NS, 2>; }

// rx = false: csi_link_sim_device (the three last pointers are not read).  rx = true: csi_link_sim_rx_device, the receiver that estimates
// the effective channel from a precoded preamble - the same checks in the same words, the same chunks, the same three launches per chunk.
int link_sim_run(csi_ctx* c, bool rx, const float* d_h_re, const float* d_h_im, const float* d_fbb_re, const float* d_fbb_im, const float* d_frf_re,
                 const float* d_frf_im, const float* d_noise_var, uint64_t seed, int64_t first_pkt, int64_t npkt, int ns, int ntrf, int n_sym,
                 int bps, int32_t* d_bit_errors, float* d_evm_rms, float* d_dt_snr_db, float* d_xeq_re, float* d_xeq_im, float* d_csi,
                 float* d_llr, uint8_t* d_bits, float* d_g_nmse, float* d_gest_re, float* d_gest_im) {
    const char* who = rx ? "csi_link_sim_rx_device" : "csi_link_sim_device";
    const csi_config& cf = c->cfg;
    const int nt = cf.nt, nr = cf.nr;
    if (nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no link simulation");
    if (npkt < 0 || first_pkt < 0)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld / first_pkt %lld must not be negative", who, (long long)npkt, (long long)first_pkt);
    if (bps != 2 && bps != 4) return fail(c, CSI_ERR_INVALID_ARG, "%s: bps %d is not 2 (QPSK) or 4 (16-QAM)", who, bps);
    if (ntrf < 1) return fail(c, CSI_ERR_INVALID_ARG, "%s: ntrf %d must be at least 1", who, ntrf);
    if (ns < 1 || ns > std::min(std::min(LK_MAX_NS, nr), ntrf))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: ns %d outside 1 .. min(%d, Nr %d, ntrf %d)", who, ns, LK_MAX_NS, nr, ntrf);
    if (n_sym < 1) return fail(c, CSI_ERR_INVALID_ARG, "%s: n_sym %d must be at least 1", who, n_sym);
    int64_t n_info = 0, n_coded = 0;
    link_frame(ns, n_sym, bps, &n_info, &n_coded);
    const int64_t n_steps = n_coded / 3;
    if (n_steps > LK_MAX_STEPS)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: n_steps %lld = ns %d x n_sym %d x 234 x bps %d / 3 exceeds %d (one codeword per packet, 8 bytes of LDS per step)",
                    who, (long long)n_steps, ns, n_sym, bps, LK_MAX_STEPS);
    if ((d_xeq_re == nullptr) != (d_xeq_im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the xeq planes come as a pair", who);
    if (rx && (d_gest_re == nullptr) != (d_gest_im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the gest planes come as a pair", who);
    if (npkt > 0 && (!d_h_re || !d_h_im || !d_fbb_re || !d_fbb_im || !d_frf_re || !d_frf_im || !d_noise_var || !d_bit_errors || !d_evm_rms || !d_dt_snr_db ||
                     (rx && !d_g_nmse)))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (h, fbb, frf_mean, noise_var, bit_errors, evm_rms, dt_snr_db%s)", who,
                    rx ? ", g_nmse" : "");
    if (npkt > 0x7fffffff) return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets exceed one launch (2^31 - 1)", who, (long long)npkt);
    const size_t lds = rx ? link_txrx_rx_lds_bytes(nr, ns, ntrf) : link_txrx_lds_bytes(nr, ns, ntrf);
    if (lds > LK_MAX_LDS)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: Nr %d, ns %d, ntrf %d need %zu bytes of LDS (160 KiB per workgroup)", who, nr, ns, ntrf, lds);
    if (npkt == 0) return CSI_OK;
    HIP_TRY(c, hipSetDevice(cf.device));
    // the kernels of csi_link_sim_device are named first: instantiated in this order, they keep their place in the code object
    const void* fn = !rx ? (ns == 1 ? link_txrx_fn<1>(bps) : ns == 2 ? link_txrx_fn<2>(bps) : ns == 3 ? link_txrx_fn<3>(bps) : link_txrx_fn<4>(bps))
                         : (ns == 1 ? link_txrx_rx_fn<1>(bps) : ns == 2 ? link_txrx_rx_fn<2>(bps) : ns == 3 ? link_txrx_rx_fn<3>(bps) : link_txrx_rx_fn<4>(bps));
    const int n_ltf = rx ? link_preamble_symbols(ns) : 0;
    if (lds > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // packet chunks against the workspace limit: the coded bits, and the soft bits when the caller keeps none
    const size_t coded_b = ((size_t)n_coded + 15) / 16 * 16;
    const size_t pkt_bytes = coded_b + (d_llr ? 0 : (size_t)n_coded * sizeof(float));
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
        float* llr = d_llr ? d_llr + (size_t)p0 * n_coded : reinterpret_cast<float*>(c->link_ws + coded_b * (size_t)chunk);
        LinkRxArgs b{};
        LinkArgs& a = b.a;
        a.h_re = d_h_re + p0 * pkt_h; a.h_im = d_h_im + p0 * pkt_h;
        a.fbb_re = d_fbb_re + (size_t)p0 * LK_N * ns * ntrf; a.fbb_im = d_fbb_im + (size_t)p0 * LK_N * ns * ntrf;
        a.frf_re = d_frf_re + (size_t)p0 * ntrf * nt; a.frf_im = d_frf_im + (size_t)p0 * ntrf * nt;
        a.noise_var = d_noise_var + p0;
        a.coded = coded; a.llr = llr;
        a.xeq_re = d_xeq_re ? d_xeq_re + (size_t)p0 * ns * n_sym * LK_N : nullptr;
        a.xeq_im = d_xeq_im ? d_xeq_im + (size_t)p0 * ns * n_sym * LK_N : nullptr;
        a.csi = d_csi ? d_csi + (size_t)p0 * ns * LK_N : nullptr;
        a.evm_rms = d_evm_rms + p0; a.dt_snr_db = d_dt_snr_db + p0;
        a.seed = seed; a.first_pkt = first_pkt + p0;
        a.nt = nt; a.nr = nr; a.ns = ns; a.ntrf = ntrf; a.n_sym = n_sym; a.bps = bps;
        a.fstride = (ns * ntrf) | 1;
        if (rx) {
            b.g_nmse = d_g_nmse + p0;
            b.gest_re = d_gest_re ? d_gest_re + (size_t)p0 * LK_N * nr * ns : nullptr;
            b.gest_im = d_gest_im ? d_gest_im + (size_t)p0 * LK_N * nr * ns : nullptr;
        }
        {
            const double items = (double)np * LK_N;
            ProfScope ps(c, K_LINK_TXRX, items * (8.0 * nt * ns * (ntrf + nr) + (double)(n_sym + n_ltf) * 16.0 * nr * ns),
                         items * nr * nt * 8.0 + (double)np * n_coded * 5.0);
            const int64_t steps = np * n_steps;
            hipLaunchKernelGGL(link_encode_kernel, dim3((unsigned)((steps + 255) / 256)), dim3(256), 0, c->stream, coded, seed, a.first_pkt, np, (int)n_steps);
            HIP_TRY(c, hipGetLastError());
            void* kargs[] = {&b};      // LinkArgs is the head of LinkRxArgs: link_txrx_kernel reads its own part
            HIP_TRY(c, hipLaunchKernel(fn, dim3((unsigned)np), dim3(LK_THREADS), kargs, lds, c->stream));
            c->link_launches += 2;
        }
        rc = viterbi_launch(c, llr, np, (int)n_steps, d_bits ? d_bits + (size_t)p0 * n_info : nullptr, d_bit_errors + p0, seed, a.first_pkt);
        if (rc) return rc;
    }
    return CSI_OK;
}

int link_sim_device(csi_ctx* c, const float* d_h_re, const float* d_h_im, const float* d_fbb_re, const float* d_fbb_im, const float* d_frf_re,
                    const float* d_frf_im, const float* d_noise_var, uint64_t seed, int64_t first_pkt, int64_t npkt, int ns, int ntrf, int n_sym,
                    int bps, int32_t* d_bit_errors, float* d_evm_rms, float* d_dt_snr_db, float* d_xeq_re, float* d_xeq_im, float* d_csi,
                    float* d_llr, uint8_t* d_bits) {
    return link_sim_run(c, false, d_h_re, d_h_im, d_fbb_re, d_fbb_im, d_frf_re, d_frf_im, d_noise_var, seed, first_pkt, npkt, ns, ntrf, n_sym, bps,
                        d_bit_errors, d_evm_rms, d_dt_snr_db, d_xeq_re, d_xeq_im, d_csi, d_llr, d_bits, nullptr, nullptr, nullptr);
}

}  // namespace
