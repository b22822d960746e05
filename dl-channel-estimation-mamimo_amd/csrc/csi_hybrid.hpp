// csi_hybrid.hpp - host side of the hybrid beamforming weights (kernels: hybrid_weights.hip.h): the dictionary on
// the context, the chunked launch sequence of csi_hybrid_weights_device, the host-pointer form (a staged call, csi_stage.hpp), and the caller-driven graph
// capture that puts several device-pointer calls (csi_estimate_device + csi_hybrid_weights_device) into one hipGraph.
#pragma once
#include "csi_context.hpp"
#include "csi_stage.hpp"

namespace {

int hybrid_set_dictionary(csi_ctx* c, const float* at_re, const float* at_im, int n_rays) {
    const int nt = c->cfg.nt;
    if (nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no hybrid weights");
    if (!at_re || !at_im) return fail(c, CSI_ERR_INVALID_ARG, "csi_hybrid_set_dictionary: null dictionary planes");
    if (n_rays < 1 || n_rays > HY_MAX_RAYS)
        return fail(c, CSI_ERR_INVALID_ARG, "csi_hybrid_set_dictionary: n_rays %d outside 1 .. %d", n_rays, HY_MAX_RAYS);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int rp = (n_rays + HY_RAY_TILE - 1) / HY_RAY_TILE * HY_RAY_TILE;
    std::vector<float> pad((size_t)2 * nt * rp, 0.0f);
    for (int j = 0; j < nt; ++j)
        for (int k = 0; k < n_rays; ++k) {
            pad[(size_t)j * rp + k] = at_re[(size_t)j * n_rays + k];
            pad[(size_t)(nt + j) * rp + k] = at_im[(size_t)j * n_rays + k];
        }
    drop_graphs(c);                                   // captured launches hold the old planes
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->hyb_at_re) { HIP_TRY(c, hipFree(c->hyb_at_re)); c->hyb_at_re = c->hyb_at_im = nullptr; c->hyb_rays = c->hyb_rp = 0; }
    float* d = nullptr;
    if (hipMalloc((void**)&d, pad.size() * sizeof(float)) != hipSuccess)
        return fail(c, CSI_ERR_NOMEM, "csi_hybrid_set_dictionary: device allocation of %zu bytes failed", pad.size() * sizeof(float));
    if (hipMemcpy(d, pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(d);
        return fail(c, CSI_ERR_HIP, "csi_hybrid_set_dictionary: upload failed");
    }
    c->hyb_at_re = d;
    c->hyb_at_im = d + (size_t)nt * rp;
    c->hyb_rays = n_rays;
    c->hyb_rp = rp;
    return CSI_OK;
}

// the argument checks the device and the host form share
int hybrid_check(csi_ctx* c, const char* who, int64_t npkt, int ns, int ntrf) {
    const csi_config& cf = c->cfg;
    if (cf.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): no hybrid weights");
    if (cf.dtype == CSI_DTYPE_BF16) return fail(c, CSI_ERR_INVALID_ARG, "%s: fp32 contexts only (this one is bf16)", who);
    if (!c->hyb_at_re) return fail(c, CSI_ERR_INVALID_ARG, "%s: no dictionary set (csi_hybrid_set_dictionary)", who);
    if (cf.nr > cf.nt) return fail(c, CSI_ERR_INVALID_ARG, "%s: Nr %d > Nt %d is not supported (the singular vectors come from H H^H)", who, cf.nr, cf.nt);
    if (cf.nr > HY_MAX_NR) return fail(c, CSI_ERR_INVALID_ARG, "%s: Nr %d > %d is not supported by the singular-vector kernel", who, cf.nr, HY_MAX_NR);
    if (cf.nt > 256) return fail(c, CSI_ERR_INVALID_ARG, "%s: Nt %d > 256 is not supported by the correlation kernel", who, cf.nt);
    if (npkt < 0) return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld is negative", who, (long long)npkt);
    if (ntrf < 1 || ntrf > std::min(std::min(cf.nt, c->hyb_rays), HY_MAX_RF))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: ntrf %d outside 1 .. min(Nt %d, rays %d, %d)", who, ntrf, cf.nt, c->hyb_rays, HY_MAX_RF);
    if (ns < 1 || ns > std::min(cf.nr, ntrf))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: ns %d outside 1 .. min(Nr %d, ntrf %d)", who, ns, cf.nr, ntrf);
    if (npkt * HY_N > (int64_t)0x7fffffff / std::max(ns * ntrf, ntrf * cf.nt))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets: output offsets would pass 32 bits", who, (long long)npkt);
    return CSI_OK;
}

size_t hybrid_item_bytes(int nt, int ns, int ntrf) {
    return sizeof(float) * ((size_t)4 * ns * nt + (size_t)ntrf * (ntrf + 1) + (size_t)4 * ntrf * ns + 3);
}

int hybrid_weights_device(csi_ctx* c, const float* d_h_re, const float* d_h_im, const float* d_eval_re, const float* d_eval_im,
                          int64_t npkt, int ns, int ntrf, float stop_tol, float* d_fbb_re, float* d_fbb_im, int32_t* d_idx,
                          int32_t* d_n_atoms, float* d_gain, float* d_frf_mean_re, float* d_frf_mean_im) {
    static const char* who = "csi_hybrid_weights_device";
    int rc = hybrid_check(c, who, npkt, ns, ntrf);
    if (rc) return rc;
    if (npkt > 0 && (!d_h_re || !d_h_im || !d_fbb_re || !d_fbb_im || !d_idx))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (h, fbb, idx)", who);
    if ((d_eval_re == nullptr) != (d_eval_im == nullptr) || (d_frf_mean_re == nullptr) != (d_frf_mean_im == nullptr))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: eval / frf_mean planes come in pairs", who);
    if (npkt == 0) return CSI_OK;
    const csi_config& cf = c->cfg;
    const int nt = cf.nt, nr = cf.nr;
    HIP_TRY(c, hipSetDevice(cf.device));
    // packet chunks against the workspace limit (the DNN path's rule: as few as fit, all nearly the same size)
    const size_t budget = cf.workspace_bytes > 0 ? (size_t)cf.workspace_bytes : ((size_t)1 << 30);
    const size_t pkt_bytes = hybrid_item_bytes(nt, ns, ntrf) * HY_N;
    int64_t chunk = std::max<int64_t>(1, (int64_t)(budget / pkt_bytes));
    chunk = std::min(chunk, (int64_t)0x7fffffff / ((int64_t)HY_N * 4 * ns * nt));          // workspace element offsets of a plane fit an int
    if (chunk < 1) return fail(c, CSI_ERR_INVALID_ARG, "%s: one packet's workspace offsets would pass 32 bits", who);
    const int64_t nchunks = (npkt + chunk - 1) / chunk;
    chunk = (npkt + nchunks - 1) / nchunks;
    rc = ensure_bytes(c, &c->hyb_ws, &c->hyb_ws_bytes, pkt_bytes * (size_t)chunk + 256);
    if (rc) return rc;
    const size_t pkt_f = (size_t)nr * nt * HY_N;
    for (int64_t p0 = 0; p0 < npkt; p0 += chunk) {
        const int64_t np = std::min(chunk, npkt - p0);
        const size_t n = (size_t)np * HY_N, i0 = (size_t)p0 * HY_N;
        HybArgs a{};
        a.h_re = d_h_re + p0 * pkt_f; a.h_im = d_h_im + p0 * pkt_f;
        a.e_re = d_eval_re ? d_eval_re + p0 * pkt_f : a.h_re;
        a.e_im = d_eval_im ? d_eval_im + p0 * pkt_f : a.h_im;
        a.at_re = c->hyb_at_re; a.at_im = c->hyb_at_im;
        float* w = reinterpret_cast<float*>(c->hyb_ws);
        const size_t plane = (size_t)ns * nt * n;
        a.fopt_re = w; w += plane;
        a.fopt_im = w; w += plane;
        a.res_re = w; w += plane;
        a.res_im = w; w += plane;
        a.chol = w; w += (size_t)ntrf * (ntrf + 1) * n;
        a.yv = w; w += (size_t)2 * ntrf * ns * n;
        a.cv = w; w += (size_t)2 * ntrf * ns * n;
        a.cand = reinterpret_cast<int*>(w); w += n;
        a.state = reinterpret_cast<int*>(w);
        a.fbb_re = d_fbb_re + i0 * ns * ntrf; a.fbb_im = d_fbb_im + i0 * ns * ntrf;
        a.idx = d_idx + i0 * ntrf;
        a.n_atoms = d_n_atoms ? d_n_atoms + i0 : nullptr;
        a.gain = d_gain ? d_gain + i0 : nullptr;
        a.nt = nt; a.nr = nr; a.ns = ns; a.ntrf = ntrf; a.rays = c->hyb_rays; a.rp = c->hyb_rp;
        a.n = (int)n;
        a.stop_tol = stop_tol > 0.0f ? stop_tol : HY_DEFAULT_STOP_TOL;
        const double items = (double)n, h_bytes = items * nr * nt * 8.0;
        {
            const int tpb = std::max(1, std::min(HY_ITEM_THREADS, 65536 / (32 * nr * nr)));
            ProfScope ps(c, K_HYB_SVD, items * (4.0 * nr * (nr + 1) * nt + 8.0 * ns * nr * nt + HY_SWEEPS * 12.0 * nr * nr * nr),
                         h_bytes * (1 + ns) + items * ns * nt * 16.0);
            hipLaunchKernelGGL(hyb_svd_kernel, dim3((unsigned)((n + tpb - 1) / tpb)), dim3(tpb), (size_t)32 * nr * nr * tpb, c->stream, a, tpb);
            HIP_TRY(c, hipGetLastError());
            ++c->hybrid_launches;
        }
        for (int m = 0; m < ntrf; ++m) {
            a.step = m;
            {
                ProfScope ps(c, K_HYB_CORR, items * 8.0 * c->hyb_rays * nt * ns,       // the definition's flops (the zero-padded rays of the last tile are not counted)
                             items * ns * nt * 8.0 * (c->hyb_rp / HY_RAY_TILE));
                hipLaunchKernelGGL(hyb_corr_kernel, dim3((unsigned)((n + HY_CORR_ITEMS - 1) / HY_CORR_ITEMS)), dim3(HY_CORR_THREADS),
                                   (size_t)2 * nt * HY_RAY_TILE * sizeof(float), c->stream, a);
                HIP_TRY(c, hipGetLastError());
                ++c->hybrid_launches;
            }
            {
                ProfScope ps(c, K_HYB_SOLVE, items * 8.0 * nt * ((m + 1) + ns * (m + 2)), items * ns * nt * 32.0);
                hipLaunchKernelGGL(hyb_solve_kernel, dim3((unsigned)((n + HY_ITEM_THREADS - 1) / HY_ITEM_THREADS)), dim3(HY_ITEM_THREADS), 0, c->stream, a);
                HIP_TRY(c, hipGetLastError());
                ++c->hybrid_launches;
            }
        }
        if (d_gain) {
            ProfScope ps(c, K_HYB_FINISH, items * 8.0 * nr * nt * ns, h_bytes * ns + items * ns * nt * 8.0 * nr);
            hipLaunchKernelGGL(hyb_gain_kernel, dim3((unsigned)((n + HY_ITEM_THREADS - 1) / HY_ITEM_THREADS)), dim3(HY_ITEM_THREADS), 0, c->stream, a);
            HIP_TRY(c, hipGetLastError());
            ++c->hybrid_launches;
        }
        if (d_frf_mean_re) {
            const int64_t total = np * ntrf * nt;
            ProfScope ps(c, K_HYB_FINISH, (double)total * HY_N * 2.0, (double)total * HY_N * 12.0);
            hipLaunchKernelGGL(hyb_frf_mean_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, a, total,
                               d_frf_mean_re + (size_t)p0 * ntrf * nt, d_frf_mean_im + (size_t)p0 * ntrf * nt);
            HIP_TRY(c, hipGetLastError());
            ++c->hybrid_launches;
        }
    }
    return CSI_OK;
}

// host pointers: a staged call (csi_stage.hpp) whose chunk is sized by everything it stages.  The optional planes keep their room when the
// caller leaves them out; the device form then gets a null pointer in their place
int hybrid_weights_host(csi_ctx* c, const float* h_re, const float* h_im, const float* eval_re, const float* eval_im, int64_t npkt,
                        int ns, int ntrf, float stop_tol, float* fbb_re, float* fbb_im, int32_t* idx, int32_t* n_atoms, float* gain,
                        float* frf_mean_re, float* frf_mean_im) {
    static const char* who = "csi_hybrid_weights";
    int rc = hybrid_check(c, who, npkt, ns, ntrf);
    if (rc) return rc;
    if (npkt > 0 && (!h_re || !h_im || !fbb_re || !fbb_im || !idx))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: null required pointer (h, fbb, idx)", who);
    if ((eval_re == nullptr) != (eval_im == nullptr) || (frf_mean_re == nullptr) != (frf_mean_im == nullptr))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: eval / frf_mean planes come in pairs", who);
    if (npkt == 0) return CSI_OK;
    const csi_config& cf = c->cfg;
    HIP_TRY(c, hipSetDevice(cf.device));
    const size_t pkt = (size_t)cf.nr * cf.nt * HY_N * sizeof(float);      // bytes per packet and CSI plane
    const size_t item = (size_t)HY_N * 4;                                 // ... and per 4-byte word of a carrier's result
    const size_t mean = (size_t)ntrf * cf.nt * sizeof(float);
    StagePlane p[] = {{pkt, h_re, nullptr}, {pkt, h_im, nullptr}, {pkt, eval_re, nullptr}, {pkt, eval_im, nullptr},
                      {item * ns * ntrf, nullptr, fbb_re}, {item * ns * ntrf, nullptr, fbb_im}, {item * ntrf, nullptr, idx},
                      {item, nullptr, n_atoms}, {item, nullptr, gain}, {mean, nullptr, frf_mean_re}, {mean, nullptr, frf_mean_im}};
    size_t per_pkt = 0;
    for (const StagePlane& q : p) per_pkt += q.bytes;
    return staged_call(c, npkt, STAGE_BUDGET, per_pkt, 0, true, p, [&](int64_t, int64_t np) {
        return hybrid_weights_device(c, p[0].as<float>(), p[1].as<float>(), eval_re ? p[2].as<float>() : nullptr, eval_re ? p[3].as<float>() : nullptr, np,
                                     ns, ntrf, stop_tol, p[4].as<float>(), p[5].as<float>(), p[6].as<int32_t>(), n_atoms ? p[7].as<int32_t>() : nullptr,
                                     gain ? p[8].as<float>() : nullptr, frf_mean_re ? p[9].as<float>() : nullptr, frf_mean_re ? p[10].as<float>() : nullptr);
    });
}

// ---------------------------------------------------------------- caller-driven capture of several device-pointer calls
struct csi_user_graph {
    hipGraphExec_t exec = nullptr;
    int64_t hs_launches = 0;      // split-engine GEMMs inside (a replay owes them to the range-guard bookkeeping)
    uint64_t epoch = 0;           // the context's buffer / option epoch at capture: a later reallocation makes the graph stale
};

int capture_begin(csi_ctx* c) {
    if (c->user_capture) return fail(c, CSI_ERR_INVALID_ARG, "csi_capture_begin: a capture is already open");
    if (c->prof_on) return fail(c, CSI_ERR_INVALID_ARG, "csi_capture_begin: per-kernel profiling records events the capture cannot hold");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    c->user_capture = true;
    c->user_capture_use_graph = c->use_graph;
    c->use_graph = false;                      // the calls that follow are the graph's content, not graphs of their own
    c->in_graph_call = true;
    c->user_capture_hs0 = c->hs_launches;
    return CSI_OK;
}

int capture_end(csi_ctx* c, void** out) {
    if (!c->user_capture) return fail(c, CSI_ERR_INVALID_ARG, "csi_capture_end: no capture is open");
    c->user_capture = false;
    c->use_graph = c->user_capture_use_graph;
    c->in_graph_call = false;
    hipGraph_t graph = nullptr;
    const hipError_t e_end = hipStreamEndCapture(c->stream, &graph);
    if (e_end != hipSuccess || !graph) return fail(c, CSI_ERR_HIP, "csi_capture_end: hipStreamEndCapture failed: %s", hipGetErrorString(e_end));
    if (!out) { hipGraphDestroy(graph); return fail(c, CSI_ERR_INVALID_ARG, "csi_capture_end: null result pointer"); }
    hipGraphExec_t exec = nullptr;
    const hipError_t e_inst = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e_inst != hipSuccess) return fail(c, CSI_ERR_HIP, "csi_capture_end: hipGraphInstantiate failed: %s", hipGetErrorString(e_inst));
    csi_user_graph* g = new csi_user_graph;
    g->exec = exec;
    g->hs_launches = c->hs_launches - c->user_capture_hs0;
    g->epoch = c->graph_epoch;
    *out = g;
    return CSI_OK;
}

int capture_launch(csi_ctx* c, void* graph) {
    csi_user_graph* g = static_cast<csi_user_graph*>(graph);
    if (!g || !g->exec) return fail(c, CSI_ERR_INVALID_ARG, "csi_capture_launch: null graph");
    if (c->user_capture) return fail(c, CSI_ERR_INVALID_ARG, "csi_capture_launch: a capture is open");
    if (g->epoch != c->graph_epoch)
        return fail(c, CSI_ERR_INVALID_ARG, "csi_capture_launch: the graph is stale (a buffer, the weights, the pilot, the dictionary or an option changed since its capture)");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    ++c->graph_replays;
    c->hs_launches += g->hs_launches;
    HIP_TRY(c, hipGraphLaunch(g->exec, c->stream));
    return CSI_OK;
}

}  // namespace
