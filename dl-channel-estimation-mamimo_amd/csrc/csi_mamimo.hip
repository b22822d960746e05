// csi_mamimo.hip - C-ABI (include/csi_mamimo.h) and host-side orchestration of the MI355X
// channel-estimation hot path.  gfx950 only; built with
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC csi_mamimo.hip -o libcsi_mamimo.so
// (host code for the baseline x86-64 ISA; the AVX2 staging loops of csi_hostpipe.hpp carry their own target attribute), after
// band_kernel_gen.py -> clang -x assembler -mcpu=gfx950 -> ld.lld -> band8_hsaco.inc (_lib.build_library does all of it)
//
// What runs where (reference call sites in include/csi_mamimo.h):
//   csi_predict*        layer 0 once per (packet, rx)  -> gemm_f32_kernel<EPI_RAW> (optional split-K)
//                       (+ splitk_reduce_kernel)          then per pair (packet, rx, tx):
//                       hidden 1.. and regressor       -> pair_gemm_f32_kernel / gemm_f32_kernel
//   csi_predict_samples literal un-shared network      -> gemm_f32_kernel
//   csi_ls_estimate*    FFT + despread                 -> ls_estimate_kernel
#include "csi_context.hpp"
#include "csi_weights.hpp"
#include "csi_dnn_hs.hpp"
#include "csi_dnn_f32.hpp"
#include "csi_ls.hpp"
#include "csi_lmmse.hpp"
#include "csi_dnn_small.hpp"
#include "csi_dnn_bf16.hpp"
#include "csi_train.hpp"
#include "csi_hostpipe.hpp"
#include "csi_comm.hpp"
#include "csi_hybrid.hpp"
#include "csi_link.hpp"
#include "csi_scatter.hpp"
#include "csi_subspace.hpp"
#include "csi_beam.hpp"
#include "csi_mu.hpp"
#include "csi_mu_hybrid.hpp"
#include "csi_mu_jsdm.hpp"
#include "csi_feedback.hpp"
#include "csi_rx_combine.hpp"
#include "csi_scatter_aged.hpp"      // last: its kernels are emitted behind every other kernel, whose pc-relative addresses stay what they were
#include "csi_forecast.hpp"          // ... and these behind them, for the same reason
#include "csi_cfo.hpp"               // ... and these
#include "csi_sync.hpp"              // ... and these
#include <initializer_list>

namespace {

// The pointer contract of the device-pointer entry points (include/csi_mamimo.h, "Device pointers"): every re / im plane starts on a
// 16-byte boundary - the LS and layer-0 kernels load and store the caller's rows as 16-byte words and through LDS-DMA.  Checked on the
// host before anything is launched or counted; a null pointer (an optional plane) passes.
struct PlaneArg { const char* name; const void* p; };
int planes_aligned(csi_ctx* c, const char* who, std::initializer_list<PlaneArg> planes) {
    for (const PlaneArg& a : planes)
        if (reinterpret_cast<uintptr_t>(a.p) & 15)
            return fail(c, CSI_ERR_INVALID_ARG, "%s: %s must start on a 16-byte boundary (got %p)", who, a.name, a.p);
    return CSI_OK;
}

int check_ready(csi_ctx* c, bool need_models, int model = -1) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (c->cfg.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "single-input context (nt=0): only csi_predict_samples is available");
    if (!c->pilot_ok) return fail(c, CSI_ERR_NOT_READY, "csi_set_pilot has not been called");
    if (need_models) {
        for (int d = 0; d < 2; ++d) {
            if (model >= 0 && d != model) continue;
            if (!c->model[d].loaded)
                return fail(c, CSI_ERR_NOT_READY, "weights of the %s model are not loaded", d ? "imag" : "real");
            if (!c->model[d].table_ok) {
                int rc = build_pilot_table(c, c->model[d]);
                if (rc) return rc;
            }
        }
    }
    return CSI_OK;
}

// hipGraph replay of a device-pointer call ("use_graph"): the 1st call with a key runs eagerly (it sizes every
// buffer), the 2nd is captured - the whole launch sequence of the call: range-guard memsets, magnitude sample,
// layer 0 (+ slab sum), per-pair layers, regressor, for both component models and every packet chunk, and the LS
// kernel for csi_estimate_device - later calls replay it.  Any reallocation / weight / pilot / option change
// drops the cache.  Calls that fork a second stream (small_call_overlap) or profile per kernel run eagerly.
template <typename Run>
int graph_or_run(csi_ctx* c, const GraphEntry& key, Run&& run) {
    if (!c->use_graph || c->prof_on) return run();
    auto same = [&](const GraphEntry& g) {
        return g.in_re == key.in_re && g.in_im == key.in_im && g.out_re == key.out_re && g.out_im == key.out_im && g.h_re == key.h_re &&
               g.h_im == key.h_im && g.npkt == key.npkt;
    };
    GraphEntry* ge = nullptr;
    for (auto& g : c->graphs)
        if (same(g)) ge = &g;
    if (!ge) {
        if (c->graphs.size() >= 16) drop_graphs(c);
        c->graphs.push_back(key);
        ge = &c->graphs.back();
    }
    if (ge->exec) {
        ++c->graph_replays;
        c->hs_launches += ge->hs_launches;         // the replayed kernels feed the range guard like eager ones
        HIP_TRY(c, hipGraphLaunch(ge->exec, c->stream));
        return CSI_OK;
    }
    if (ge->seen++ == 0) return run();
    const int64_t launches = c->hs_launches;
    HIP_TRY(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    int rc = run();
    hipGraph_t graph = nullptr;
    const hipError_t e_end = hipStreamEndCapture(c->stream, &graph);
    if (rc) { if (graph) hipGraphDestroy(graph); return rc; }
    if (e_end != hipSuccess) return fail(c, CSI_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e_end));
    hipGraphExec_t exec = nullptr;
    const hipError_t e_inst = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e_inst != hipSuccess) return fail(c, CSI_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e_inst));
    for (auto& g : c->graphs)
        if (same(g)) { g.exec = exec; g.hs_launches = c->hs_launches - launches; }
    HIP_TRY(c, hipGraphLaunch(exec, c->stream));
    return CSI_OK;
}

}  // namespace

// =====================================================================================
extern "C" {

int csi_abi_version(void) { return CSI_ABI_VERSION; }

const char* csi_last_error(const csi_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int csi_set_input_pool(csi_ctx* c, int mode) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (mode < POOL_NONE || mode > POOL_AVG)
        return fail(c, CSI_ERR_INVALID_ARG, "csi_set_input_pool: mode %d is none (0), max (1) or avg (2)", mode);
    if (mode != POOL_NONE && c->cfg.nt == 0)
        return fail(c, CSI_ERR_INVALID_ARG, "csi_set_input_pool: pooling needs the pilot input (nt > 0); the single-input model has none");
    for (int d = 0; d < 2; ++d) {
        if (c->model[d].loaded)
            return fail(c, CSI_ERR_INVALID_ARG, "csi_set_input_pool: the %s model holds weights; the pooling mode is set before csi_load_weights", d ? "imag" : "real");
        if (c->trainer[d])
            return fail(c, CSI_ERR_INVALID_ARG, "csi_set_input_pool: a trainer of the %s model exists; the pooling mode is set before csi_train_begin", d ? "imag" : "real");
    }
    if (mode != POOL_NONE && c->model_type == CSI_MODEL_CONV1D)
        return fail(c, CSI_ERR_INVALID_ARG, "csi_set_input_pool: a CONV1D model has no input pooling (the reference decimates only in its FC branch); csi_set_model_type(FC) first");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    drop_graphs(c);
    c->input_pool = mode;
    set_layer0_width(c);
    return CSI_OK;
}

int csi_set_model_type(csi_ctx* c, int type) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (type != CSI_MODEL_FC && type != CSI_MODEL_CONV1D)
        return fail(c, CSI_ERR_INVALID_ARG, "csi_set_model_type: type %d is FC (0) or CONV1D (1)", type);
    if (type != CSI_MODEL_FC && c->cfg.nt == 0)
        return fail(c, CSI_ERR_INVALID_ARG, "csi_set_model_type: CONV1D needs the pilot input (nt > 0); the single-input model has none");
    for (int d = 0; d < 2; ++d) {
        if (c->model[d].loaded)
            return fail(c, CSI_ERR_INVALID_ARG, "csi_set_model_type: the %s model holds weights; the model type is set before csi_load_weights", d ? "imag" : "real");
        if (c->trainer[d])
            return fail(c, CSI_ERR_INVALID_ARG, "csi_set_model_type: a trainer of the %s model exists; the model type is set before csi_train_begin", d ? "imag" : "real");
    }
    if (type == CSI_MODEL_CONV1D) {
        if (c->input_pool != POOL_NONE)
            return fail(c, CSI_ERR_INVALID_ARG, "csi_set_model_type: CONV1D and input pooling (%s) exclude each other (the reference decimates only in its FC branch); "
                        "csi_set_input_pool(none) first", input_pool_name(c->input_pool));
        if (c->cfg.len_ltf % 2 != 0 || c->cfg.len_ltf < 2)
            return fail(c, CSI_ERR_INVALID_ARG, "csi_set_model_type: CONV1D needs an even len_ltf (AveragePooling1D pairs the samples), got %d", c->cfg.len_ltf);
        // K0 = 64 len_ltf features per preamble: the layer-0 GEMMs address a 256-row tile of their operands with 32-bit byte offsets
        // (buffer loads of gemm_hs.hip.h / gemm_bf16.hip.h, 2 halves per split-f16 weight): 256 x 2 x 64 len_ltf x 2 bytes stays below 2^31
        if (c->cfg.len_ltf > 20480)
            return fail(c, CSI_ERR_INVALID_ARG, "csi_set_model_type: CONV1D supports len_ltf <= 20480 (nt <= 64 at 320 samples per antenna), got %d: "
                        "its %lld layer-0 features per preamble would overflow the 32-bit offsets of the layer-0 kernels", c->cfg.len_ltf, 64LL * c->cfg.len_ltf);
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    drop_graphs(c);
    c->model_type = type;
    set_layer0_width(c);
    return CSI_OK;
}

int csi_create(const csi_config* cfg, csi_ctx** out) {
    if (!cfg || !out) return fail(nullptr, CSI_ERR_INVALID_ARG, "csi_create: null argument");
    *out = nullptr;
    if (cfg->nt < 0 || cfg->nr < 1 || cfg->n_out < 1 || cfg->n_hidden < 1 || cfg->n_hidden > CSI_MAX_HIDDEN)
        return fail(nullptr, CSI_ERR_INVALID_ARG, "csi_create: bad shape nt=%d nr=%d n_hidden=%d n_out=%d",
                    cfg->nt, cfg->nr, cfg->n_hidden, cfg->n_out);
    // nt == 0: single-input model without pilot input (DNN.py:180,234); csi_predict_samples only
    if (cfg->nt > 0 && cfg->len_ltf != LS_SYM * cfg->nt)
        return fail(nullptr, CSI_ERR_INVALID_ARG, "csi_create: len_ltf (%d) must be 320*nt (%d)", cfg->len_ltf,
                    LS_SYM * cfg->nt);
    if (cfg->nt == 0 && (cfg->len_ltf < 4 || cfg->len_ltf % 4))
        return fail(nullptr, CSI_ERR_INVALID_ARG, "csi_create: single-input width %d must be a positive multiple of 4", cfg->len_ltf);
    if (cfg->nt % 4)
        return fail(nullptr, CSI_ERR_INVALID_ARG, "csi_create: nt must be a multiple of 4 (16-byte rows), got %d", cfg->nt);
    for (int i = 0; i < cfg->n_hidden; ++i)
        if (cfg->hidden[i] < 4 || cfg->hidden[i] % 4)
            return fail(nullptr, CSI_ERR_INVALID_ARG, "csi_create: hidden[%d]=%d must be a positive multiple of 4", i,
                        cfg->hidden[i]);
    if (cfg->dtype != CSI_DTYPE_F32 && cfg->dtype != CSI_DTYPE_BF16)
        return fail(nullptr, CSI_ERR_INVALID_ARG, "csi_create: unknown dtype %d", cfg->dtype);
    if (cfg->dtype == CSI_DTYPE_BF16) {
        for (int i = 0; i < cfg->n_hidden; ++i)
            if (cfg->hidden[i] % 8)
                return fail(nullptr, CSI_ERR_INVALID_ARG, "csi_create: bf16 needs hidden widths that are multiples of 8 (hidden[%d]=%d)", i, cfg->hidden[i]);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, CSI_ERR_NO_DEVICE, "csi_create: no HIP device visible");
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, CSI_ERR_INVALID_ARG, "csi_create: device %d out of range (%d visible)", cfg->device, ndev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess)
        return fail(nullptr, CSI_ERR_HIP, "csi_create: hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, CSI_ERR_NO_DEVICE, "csi_create: device %d is %s; this library is built for gfx950 only",
                    cfg->device, prop.gcnArchName);

    csi_ctx* c = new csi_ctx();
    if (const char* h = std::getenv("CSI_DEBUG_HOOKS")) if (h[0] == '1') if (const char* d = std::getenv("CSI_SMALL_TILE16")) c->debug_small_tile16 = d[0] == '1';   // (once: not in the call path)
    c->cfg = *cfg;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (c->cfg.bn_eps <= 0.f) c->cfg.bn_eps = 1e-3f;
    set_layer0_width(c);
    if (const char* e = std::getenv("CSI_FORCE_PAIR_TILE")) c->force_pair_tile = std::atoi(e);
    if (const char* e = std::getenv("CSI_LS_FFT_FIRST_MAX")) c->ls_fft_first_max = std::min(64, std::max(0, std::atoi(e)));
    if (const char* e = std::getenv("CSI_LS_DEBUG")) c->ls_debug = std::atoi(e);
    if (const char* e = std::getenv("CSI_LS_KERNEL")) c->ls_kernel = std::min(7, std::max(0, std::atoi(e)));
    if (const char* e = std::getenv("CSI_LS_V2")) c->ls_v2 = std::atoi(e);
    if (const char* e = std::getenv("CSI_HS_VM")) c->hs_vm_cast = c->hs_vm_pair = std::min(3, std::max(0, std::atoi(e)));
    auto bail = [&](int code) {
        g_create_error = c->err;
        csi_destroy(c);
        return code;
    };
    if (hipSetDevice(cfg->device) != hipSuccess) { c->err = "hipSetDevice failed"; return bail(CSI_ERR_HIP); }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        c->err = "hipStreamCreate failed";
        return bail(CSI_ERR_HIP);
    }
    {
        int widest = 1;
        for (int i = 0; i < cfg->n_hidden; ++i) widest = std::max(widest, cfg->hidden[i]);
        const size_t zb = ((size_t)widest + 64) * sizeof(float);
        if (hipMalloc((void**)&c->hs_zero, zb) != hipSuccess || hipMemset(c->hs_zero, 0, zb) != hipSuccess) {
            c->err = "device allocation failed";
            return bail(CSI_ERR_NOMEM);
        }
    }
    if (hipMalloc((void**)&c->hs_peak, 256) != hipSuccess || hipMemset(c->hs_peak, 0, 256) != hipSuccess) {
        c->err = "device allocation failed";
        return bail(CSI_ERR_NOMEM);
    }
    // LS constants.  Twiddles in double on the host so the table is correctly rounded.
    std::vector<float> tw(2 * LS_FFT);
    for (int u = 0; u < LS_FFT; ++u) {
        const double ang = -2.0 * M_PI * u / LS_FFT;
        tw[u] = (float)std::cos(ang);
        tw[LS_FFT + u] = (float)std::sin(ang);
    }
    // VHT-LTF literal of helperMIMOChannelEstimate.m:16-23 and the data-bin list of
    // generate_maMIMO_LTF.m:98-102, in fftshift-ed (1-based MATLAB) bin order.
    static const int ltfL[26] = {1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1};
    static const int ltfR[26] = {1, -1, -1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1, -1, 1, -1, 1, 1, 1, 1};
    static const int midA[11] = {-1, -1, -1, 1, 1, -1, 1, -1, 1, 1, -1};
    static const int midB[9] = {1, -1, 1, -1, 0, 1, -1, -1, 1};
    std::vector<int> ltf;
    auto push = [&](const int* v, int n) { ltf.insert(ltf.end(), v, v + n); };
    auto seg = [&]() { push(ltfL, 26); ltf.push_back(1); push(ltfR, 26); };
    ltf.assign(7, 0);
    seg(); push(midA, 11); seg(); push(midB, 9); seg(); push(midA, 11); seg();
    ltf.insert(ltf.end(), 6, 0);
    if ((int)ltf.size() != LS_FFT) { c->err = "internal: LTF literal length"; return bail(CSI_ERR_INVALID_ARG); }
    static const int pilots[8] = {26, 54, 90, 118, 140, 168, 204, 232};
    std::vector<int> bin_pos;
    std::vector<float> denom;
    for (int k1 = 1; k1 <= LS_FFT; ++k1) {
        bool skip = (k1 <= 7) || (k1 == 129) || (k1 >= 251);
        for (int pk : pilots) skip = skip || (k1 == pk);
        if (skip) continue;
        bin_pos.push_back((k1 - 1 + LS_FFT / 2) % LS_FFT);      // undo fftshift: shifted index -> FFT bin
        denom.push_back((float)cfg->nt * (float)ltf[k1 - 1]);
    }
    if ((int)bin_pos.size() != LS_NDATA) { c->err = "internal: data-bin count"; return bail(CSI_ERR_INVALID_ARG); }
    if (upload(c, &c->tw, tw.data(), tw.size())) return bail(CSI_ERR_HIP);
    if (upload(c, &c->denom, denom.data(), denom.size())) return bail(CSI_ERR_HIP);
    {
        std::vector<float> ltf_nat(LS_FFT);      // the generator needs all 242 non-null bins, in FFT bin order
        for (int k = 0; k < LS_FFT; ++k) ltf_nat[(k + LS_FFT / 2) % LS_FFT] = (float)ltf[k];
        if (upload(c, &c->ltf_nat, ltf_nat.data(), ltf_nat.size())) return bail(CSI_ERR_HIP);
    }
    if (hipMalloc((void**)&c->bin_pos, LS_NDATA * sizeof(int)) != hipSuccess ||
        hipMemcpy(c->bin_pos, bin_pos.data(), LS_NDATA * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        c->err = "bin table upload failed";
        return bail(CSI_ERR_HIP);
    }
    {
        // the blind LMMSE smoother's null-carrier sums run in fp64 pairs: their own twiddle table (the fp32 one above is the LS kernels'),
        // from the quarter wave by symmetry: u = 64 q + r, phi = 2 pi r / 256, cos phi = C[r], sin phi = C[64 - r]
        std::vector<LmbTwiddle> tw64(LMB_FFT);
        for (int u = 0; u < LMB_FFT; ++u) {
            const int q = u >> 6, r = u & 63;
            const double* cs = kLmbQuarterCos[r];
            const double* sn = kLmbQuarterCos[64 - r];
            const double* co = (q & 1) ? sn : cs;                    // |cos theta|, |sin theta|
            const double* si = (q & 1) ? cs : sn;
            const double sc = (q == 1 || q == 2) ? -1.0 : 1.0, ss = q >= 2 ? -1.0 : 1.0;      // signs of cos theta, sin theta
            tw64[u] = LmbTwiddle{sc * co[0], sc * co[1], -ss * si[0], -ss * si[1]};             // exp(-i theta)
        }
        if (hipMalloc((void**)&c->lmb_tw, LMB_FFT * sizeof(LmbTwiddle)) != hipSuccess ||
            hipMemcpy(c->lmb_tw, tw64.data(), LMB_FFT * sizeof(LmbTwiddle), hipMemcpyHostToDevice) != hipSuccess ||
            hipMalloc((void**)&c->lmb_count, 256) != hipSuccess || hipMemset(c->lmb_count, 0, 256) != hipSuccess) {
            c->err = "blind LMMSE constants: device allocation failed";
            return bail(CSI_ERR_NOMEM);
        }
    }
    if (ls_prepare(c) != CSI_OK) return bail(CSI_ERR_HIP);
    *out = c;
    return CSI_OK;
}

void csi_destroy(csi_ctx* c) {
    if (!c) return;
    hipSetDevice(c->cfg.device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (auto& sp : c->spans) { hipEventDestroy(sp.beg); hipEventDestroy(sp.end); }
    for (auto e : c->ev_pool) hipEventDestroy(e);
    drop_graphs(c);
    free_model(c->model[0]);
    free_model(c->model[1]);
    for (int d = 0; d < 2; ++d) tr_free(c->trainer[d]);
    delete c->hostpipe;
    comm_free(c);
    if (c->band_mod) hipModuleUnload(c->band_mod);
    if (c->P) hipFree(c->P);
    if (c->hyb_at_re) hipFree(c->hyb_at_re);
    if (c->hyb_ws) hipFree(c->hyb_ws);
    if (c->link_ws) hipFree(c->link_ws);
    if (c->muh_ws) hipFree(c->muh_ws);
    if (c->muj_ws) hipFree(c->muj_ws);
    if (c->fb_ws) hipFree(c->fb_ws);
    if (c->fb_tab) hipFree(c->fb_tab);
    if (c->lmb_tw) hipFree(c->lmb_tw);
    if (c->lmb_ws) hipFree(c->lmb_ws);
    if (c->lmb_count) hipFree(c->lmb_count);
    if (c->sub_q) hipFree(c->sub_q);
    if (c->beam_a) hipFree(c->beam_a);
    if (c->beam_ws) hipFree(c->beam_ws);
    if (c->forecast_ws) hipFree(c->forecast_ws);
    if (c->cfo_ws) hipFree(c->cfo_ws);
    if (c->sync_ws) hipFree(c->sync_ws);
    if (c->hs_peak) hipFree(c->hs_peak);
    if (c->hs_zero) hipFree(c->hs_zero);
    if (c->fuse_ws) hipFree(c->fuse_ws);
    if (c->small_ws) hipFree(c->small_ws);
    if (c->Ppad) hipFree(c->Ppad);
    if (c->Pbf) hipFree(c->Pbf);
    if (c->p_tables) hipFree(c->p_tables);
    if (c->tw) hipFree(c->tw);
    if (c->bin_pos) hipFree(c->bin_pos);
    if (c->denom) hipFree(c->denom);
    if (c->ltf_nat) hipFree(c->ltf_nat);
    if (c->synth_ws) hipFree(c->synth_ws);
    if (c->ws) hipFree(c->ws);
    if (c->stage) hipFree(c->stage);
    if (c->aux_ws) hipFree(c->aux_ws);
    if (c->aux_l0skinny) hipFree(c->aux_l0skinny);
    if (c->aux_skbuf) hipFree(c->aux_skbuf);
    if (c->aux_fuse_ws) hipFree(c->aux_fuse_ws);
    if (c->aux_fork) hipEventDestroy(c->aux_fork);
    if (c->aux_join) hipEventDestroy(c->aux_join);
    if (c->aux_stream) hipStreamDestroy(c->aux_stream);
    if (c->skbuf) hipFree(c->skbuf);
    if (c->l0skinny) hipFree(c->l0skinny);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

int csi_load_weights(csi_ctx* c, int model, const csi_tensor* tensors, int n) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (model < 0 || model > 1 || !tensors || n <= 0) return fail(c, CSI_ERR_INVALID_ARG, "csi_load_weights: bad argument");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    Model& m = c->model[model];
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    drop_graphs(c);
    free_model(m);                          // before the tensors are looked at: a refused load leaves the model unloaded
    const WeightFacts facts{c->cfg, c->d_in, c->l0_k, c->model_type, c->input_pool}; PreparedModel pm;
    // upload by the table (csi_context.hpp; T, T_hs, T_sw, Wt1, Wt2, l0_rowmax are derived on the device and not in it): payload + slack allocated and zeroed, the payload copied
    auto put = [&](void** dst, const HostBuf& b, size_t payload, size_t slack, const char* name) {
        if (!b.data) return (int)CSI_OK;
        if (b.bytes != payload) return fail(c, CSI_ERR_INVALID_ARG, "csi_load_weights: internal - %s prepared as %zu bytes, %zu in the buffer table", name, b.bytes, payload);
        if (hipMalloc(dst, payload + slack) != hipSuccess) { *dst = nullptr; return fail(c, CSI_ERR_NOMEM, "device allocation of %zu bytes failed", payload + slack); }
        HIP_TRY(c, hipMemset(*dst, 0, payload + slack));
        HIP_TRY(c, hipMemcpy(*dst, b.data, payload, hipMemcpyHostToDevice));
        return (int)CSI_OK;
    };
    m.layers.resize(c->cfg.n_hidden + 1);
    for (int li = 0; li <= c->cfg.n_hidden; ++li) {
        const int bad = prepare_layer(facts, tensors, n, li, pm);
        m.hs_repr_err = pm.hs_repr_err;         // as measured so far, also when this layer is refused ("hs_weight_err_e12")
        if (bad) return fail(c, bad, "%s", pm.err.c_str());
        Layer& L = m.layers[li] = pm.layer;
        for (int k = 0; k < LAYER_BUFS; ++k)
            if (int rc = put(kLayerBufs[k].slot(L), pm.lbuf[k], kLayerBufs[k].payload(L), kLayerBufs[k].slack, kLayerBufs[k].name)) return rc;
    }
    for (int k = 0; k < MODEL_BUFS; ++k)
        if (int rc = put(kModelBufs[k].slot(m), pm.mbuf[k], kModelBufs[k].payload(m, c->cfg.nt, c->l0_k), kModelBufs[k].slack, kModelBufs[k].name)) return rc;
    m.loaded = true, m.table_ok = false;
    if (c->cfg.dtype == CSI_DTYPE_F32) {
        m.hs_repr_ok = m.hs_repr_err <= 0x1p-20;
        // not an error: the fp32 MFMA kernels serve such a model.  It is reported through the counters "hs_weight_pins" / "hs_weight_err_e12"
        // (include/csi_mamimo.h), never through csi_last_error: a successful call leaves no error text behind
        if (!m.hs_repr_ok) ++c->hs_weight_pins;
    }
    return build_pilot_table(c, m);
}

// host-only: CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) - the per-tensor checksum of TensorFlow's TensorBundle files
// (keras_files.py); continuing value in, value out (both un-inverted outside: crc = 0 starts a new checksum)
__attribute__((target("sse4.2"))) static uint32_t crc32c_sse42(const unsigned char* p, size_t n, uint32_t c) {
    while (n && (reinterpret_cast<uintptr_t>(p) & 7)) { c = __builtin_ia32_crc32qi(c, *p++); --n; }
    uint64_t c64 = c;
    for (; n >= 8; n -= 8, p += 8) { uint64_t v; std::memcpy(&v, p, 8); c64 = __builtin_ia32_crc32di(c64, v); }
    c = (uint32_t)c64;
    while (n--) c = __builtin_ia32_crc32qi(c, *p++);
    return c;
}
uint32_t csi_crc32c(const void* data, int64_t bytes, uint32_t crc) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    uint32_t c = crc ^ 0xFFFFFFFFu;
    if (!p || bytes <= 0) return crc;
    if (__builtin_cpu_supports("sse4.2")) return crc32c_sse42(p, (size_t)bytes, c) ^ 0xFFFFFFFFu;
    for (int64_t i = 0; i < bytes; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
    }
    return c ^ 0xFFFFFFFFu;
}

// host-only: which LS despread a pilot matrix gets (no context, no device)
int csi_pilot_classify(const float* P, int nt, int32_t* sym_src, int32_t* out_row) {
    if (!P || nt <= 0) return CSI_ERR_INVALID_ARG;
    int perm[2][CSI_WIRE_MAX_NT];
    bool ident = true;
    if (!pilot_decompose(P, nt, perm, &ident)) return 0;
    for (int u = 0; u < nt; ++u) {
        if (sym_src) sym_src[u] = perm[0][u];
        if (out_row) out_row[u] = perm[1][u];
    }
    return ident ? 1 : 2;
}

int csi_set_pilot(csi_ctx* c, const float* P) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (!P || c->cfg.nt == 0) return fail(c, CSI_ERR_INVALID_ARG, "csi_set_pilot: null P or single-input context");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    drop_graphs(c);
    const int nt = c->cfg.nt;
    int rc = upload(c, &c->P, P, (size_t)nt * nt);
    if (rc) return rc;
    // what the plan reads (csi_ls.hpp): Sylvester order, a signed permutation of it (-> the tables of the PERM kernel), bf16 pieces
    c->p_sylvester = pilot_is_sylvester(P, nt);
    c->p_fast_identity = true;
    c->p_fast_ok = pilot_decompose(P, nt, c->p_perm, &c->p_fast_identity);
    if ((rc = pilot_fast_tables(c))) return rc;
    c->p_pieces = pilot_pieces(P, nt);
    const std::vector<float> packed = pilot_packed(P, nt), padded = pilot_padded(P, nt);
    if ((rc = upload(c, &c->Pbf, packed.data(), packed.size()))) return rc;
    if ((rc = upload(c, &c->Ppad, padded.data(), padded.size()))) return rc;
    rc = ls_prepare(c);
    if (rc) return rc;
    c->pilot_ok = true;
    for (int d = 0; d < 2; ++d) {
        c->model[d].table_ok = false;
        rc = build_pilot_table(c, c->model[d]);
        if (rc) return rc;
    }
    return CSI_OK;
}

namespace {
// does csi_predict_device run the two component models of this call on two streams?
bool two_stream_call(csi_ctx* c, int64_t npkt) {
    const bool bf16 = c->cfg.dtype == CSI_DTYPE_BF16;
    return c->small_call_overlap && !c->prof_on && !c->use_graph && !c->in_graph_call && !c->in_host_pipeline &&
           (npkt * c->cfg.nr * std::max(c->cfg.nt, 1) <= (bf16 ? 262144 : 327680) || c->small_call_overlap == 2);
    // (fp32 contexts, round 6: 131 072 -> 327 680 pair rows.  With the register-blocked band kernels two streams win up to 2560 packets of the shipped shape -
    // 1025 packets 2396 -> 2239 us per call, 1408: 2997 -> 2893, 2048: 4117 -> 4047, 2560: 5293 -> 5252 - and lose from 3000 on (+1.8 %, 4000: +3 %);
    // bf16 contexts: even at 1280 packets, worse beyond.  tools/regime_probe.py small_call_overlap=1 small_call_overlap=2, profiles/r06_band_probe.txt (H))
}
int aux_stream_ensure(csi_ctx* c) {
    if (!c->aux_stream) {
        HIP_TRY(c, hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
        HIP_TRY(c, hipEventCreateWithFlags(&c->aux_fork, hipEventDisableTiming));
        HIP_TRY(c, hipEventCreateWithFlags(&c->aux_join, hipEventDisableTiming));
    }
    return CSI_OK;
}
}  // namespace

int csi_predict_device(csi_ctx* c, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt, float* d_out_re,
                       float* d_out_im) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (npkt < 0 || (npkt > 0 && (!d_ltf_re || !d_ltf_im || !d_out_re || !d_out_im)))
        return fail(c, CSI_ERR_INVALID_ARG, "csi_predict_device: bad argument");
    if (npkt == 0) return CSI_OK;
    if ((rc = planes_aligned(c, "csi_predict_device", {{"d_ltf_re", d_ltf_re}, {"d_ltf_im", d_ltf_im}, {"d_out_re", d_out_re}, {"d_out_im", d_out_im}}))) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    auto run = [&]() -> int {
        const bool bf16 = c->cfg.dtype == CSI_DTYPE_BF16;
        auto plane = [&](Model& m, const float* in, float* out) { return bf16 ? predict_plane_bf16(c, m, in, npkt, out) : predict_plane(c, m, in, npkt, out); };
        // the one-packet regime: both models in 1 + n_hidden launches on this stream (csi_dnn_small.hpp)
        if (small_call_ok(c, npkt)) return predict_small(c, d_ltf_re, d_ltf_im, npkt, d_out_re, d_out_im);
        // small call: the two component models are independent and each is a chain of short,
        // launch-latency-bound kernels - run the imag model on a second stream with its own scratch
        // Round 5: up to 98 304 pair rows (768 bands of the fused kernel per model - three rounds of the chip), not 64 preambles: a
        // component model's kernels of a mid-size call fill a fraction of the 256 CUs (64 packets = 64 bands), and the other model's
        // fill the rest - 24 ... 128 packets 1.25-1.55x, 384 packets +16 %, 500 packets +1.4 % (profiles/r05_regime_probe.txt).  Beyond
        // that the gain is below 1 % and not worth the second workspace; 2 = any size (A/B runs).  (With the fork in front of the LS kernel:
        // 131 072 rows - 1000 packets +2.8 %, 2000 equal, 4000 packets 2.5 % slower.)  bf16 contexts (sequential until the
        // end of round 5): up to 262 144 pair rows - Nt = 64: one packet 129 -> 95 us, 64 packets 271 -> 198, 500: 1478 -> 1196, 1000: 2380 -> 2096,
        // 2000 packets equal (profiles/r05_band_split_probe.txt).
        const bool overlap = two_stream_call(c, npkt);
        if (!overlap) {
            int r = plane(c->model[0], d_ltf_re, d_out_re);
            if (r) return r;
            return plane(c->model[1], d_ltf_im, d_out_im);
        }
        if (int ra = aux_stream_ensure(c)) return ra;
        if (!c->aux_preforked) {           // (csi_estimate_device forks in front of its LS kernel)
            HIP_TRY(c, hipEventRecord(c->aux_fork, c->stream));
            HIP_TRY(c, hipStreamWaitEvent(c->aux_stream, c->aux_fork, 0));
        }
        c->aux_preforked = false;
        auto swap_scratch = [&]() {
            std::swap(c->stream, c->aux_stream);
            std::swap(c->ws, c->aux_ws); std::swap(c->ws_bytes, c->aux_ws_bytes);
            std::swap(c->l0skinny, c->aux_l0skinny); std::swap(c->l0skinny_bytes, c->aux_l0skinny_bytes);
            std::swap(c->skbuf, c->aux_skbuf); std::swap(c->skbuf_bytes, c->aux_skbuf_bytes);
            std::swap(c->fuse_ws, c->aux_fuse_ws); std::swap(c->fuse_ws_bytes, c->aux_fuse_ws_bytes);
        };
        swap_scratch();                                   // imag model: aux stream, aux scratch
        c->models_in_flight = 2;
        int r = plane(c->model[1], d_ltf_im, d_out_im);
        hipError_t e = r ? hipSuccess : hipEventRecord(c->aux_join, c->stream);
        swap_scratch();
        if (r) { c->models_in_flight = 1; return r; }
        if (e == hipSuccess) r = plane(c->model[0], d_ltf_re, d_out_re);
        c->models_in_flight = 1;
        HIP_TRY(c, e);
        if (r) return r;
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->aux_join, 0));
        return CSI_OK;
    };
    return graph_or_run(c, GraphEntry{d_ltf_re, d_ltf_im, d_out_re, d_out_im, nullptr, nullptr, npkt, 0, nullptr}, run);
}

int csi_estimate_device(csi_ctx* c, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt, float* d_out_re, float* d_out_im,
                        float* d_h_re, float* d_h_im) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (npkt < 0 || (npkt > 0 && (!d_ltf_re || !d_ltf_im || !d_out_re || !d_out_im || !d_h_re || !d_h_im)))
        return fail(c, CSI_ERR_INVALID_ARG, "csi_estimate_device: bad argument");
    if (npkt == 0) return CSI_OK;
    if ((rc = planes_aligned(c, "csi_estimate_device", {{"d_ltf_re", d_ltf_re}, {"d_ltf_im", d_ltf_im}, {"d_out_re", d_out_re}, {"d_out_im", d_out_im},
                                                        {"d_h_re", d_h_re}, {"d_h_im", d_h_im}}))) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    auto run = [&]() -> int {
        const bool g = c->use_graph;
        c->use_graph = false;                      // the two calls below are the graph's content, not graphs of their own
        c->in_graph_call = g || c->user_capture;
        int r = CSI_OK;
        // (one-packet calls, round 5: the LS kernel on a second stream beside the three DNN launches was built and measured -
        // 72.5 us per call against 64.2 in this order; the fork / join events cost more than the 8.7 us kernel hides, and it
        // runs 16.8 us beside the weight stream.  profiles/r05_small_call_trace.txt)
        // The second stream of a two-stream call is forked HERE, in front of the LS kernel: the imag model's chain needs the
        // preambles, not the LS result, and the cross-queue wait (6-7 us before its first kernel starts) passes under the LS kernel
        // (Round 6, first: bf16 contexts forked BEHIND the LS kernel, because 19 of 20 calls of 500 ... 1000 packets at Nt = 64 came back with wrong LS items when
        // the imag model's layer 0 - gemm_bf16_kernel, 64 KiB of LDS: its MFMA waves fit on an LS workgroup's CU - ran beside the LS kernel.  Root cause found
        // later in the round (tools/pk_opsel_probe.hip, profiles/r06_pk_opsel_probe.txt): a packed-fp32 instruction whose SECOND source takes its
        // low half from the high register (the transform's +-i rotations were v_pk_add_f32 op_sel:[0,1] op_sel_hi:[1,0]) loses that operand in lanes 48-63 while
        // another wave of the SIMD issues MFMAs.  The rotations are single adds now (ls_estimate.hip.h) and every context forks here again.)
        if (c->aux_fork_early && !small_call_ok(c, npkt) && two_stream_call(c, npkt) && aux_stream_ensure(c) == CSI_OK) {
            hipError_t e = hipEventRecord(c->aux_fork, c->stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(c->aux_stream, c->aux_fork, 0);
            if (e != hipSuccess) r = fail(c, CSI_ERR_HIP, "csi_estimate_device: forking the second stream failed: %s", hipGetErrorString(e));
            else c->aux_preforked = true;
        }
        // one-packet calls (round 6): the LS estimate rides in the layer-0 launch of the DNN (small_l0_ls_kernel); predict_small takes it from
        // the context - a call that does not reach that kernel after all runs the LS kernel behind the DNN
        const bool ls_inside = !r && small_ls_fusable(c, npkt);
        if (ls_inside) { c->small_ls_h_re = d_h_re; c->small_ls_h_im = d_h_im; }
        else if (!r) r = csi_ls_estimate_device(c, d_ltf_re, d_ltf_im, npkt, d_h_re, d_h_im);
        if (!r) r = csi_predict_device(c, d_ltf_re, d_ltf_im, npkt, d_out_re, d_out_im);
        if (ls_inside && c->small_ls_h_re) {
            c->small_ls_h_re = c->small_ls_h_im = nullptr;
            if (!r) r = csi_ls_estimate_device(c, d_ltf_re, d_ltf_im, npkt, d_h_re, d_h_im);
        }
        c->aux_preforked = false;
        c->use_graph = g;
        c->in_graph_call = c->user_capture;
        return r;
    };
    return graph_or_run(c, GraphEntry{d_ltf_re, d_ltf_im, d_out_re, d_out_im, d_h_re, d_h_im, npkt, 0, nullptr}, run);
}

int csi_ls_estimate_device(csi_ctx* c, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt, float* d_h_re,
                           float* d_h_im) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (npkt < 0 || (npkt > 0 && (!d_ltf_re || !d_ltf_im || !d_h_re || !d_h_im)))
        return fail(c, CSI_ERR_INVALID_ARG, "csi_ls_estimate_device: bad argument");
    if (npkt == 0) return CSI_OK;
    if ((rc = planes_aligned(c, "csi_ls_estimate_device", {{"d_ltf_re", d_ltf_re}, {"d_ltf_im", d_ltf_im}, {"d_h_re", d_h_re}, {"d_h_im", d_h_im}}))) return rc;
    return ls_run(c, d_ltf_re, d_ltf_im, npkt, d_h_re, d_h_im);
}

// ---------------------------------------------------------------- LMMSE smoothers (csi_lmmse.hpp, lmmse.hip.h)
int csi_lmmse_estimate_device(csi_ctx* c, const float* d_h_re, const float* d_h_im, int64_t npkt, const float* d_hvec, int L,
                              const float* d_snr_db, float* d_out_re, float* d_out_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (int rc = lmmse_estimate_check(c, d_h_re, d_h_im, npkt, d_hvec, L, d_snr_db, d_out_re, d_out_im)) return rc;
    if (npkt == 0) return CSI_OK;
    if (int rc = planes_aligned(c, "csi_lmmse_estimate_device", {{"d_h_re", d_h_re}, {"d_h_im", d_h_im}, {"d_out_re", d_out_re}, {"d_out_im", d_out_im}})) return rc;
    return lmmse_estimate_launch(c, d_h_re, d_h_im, npkt, d_hvec, L, d_snr_db, d_out_re, d_out_im);
}

int csi_lmmse_estimate(csi_ctx* c, const float* h_re, const float* h_im, int64_t npkt, const float* hvec, int L,
                       const float* snr_db, float* out_re, float* out_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return lmmse_estimate_host(c, h_re, h_im, npkt, hvec, L, snr_db, out_re, out_im);
}

int csi_lmmse_blind_device(csi_ctx* c, const float* d_ltf_re, const float* d_ltf_im, const float* d_h_re, const float* d_h_im, int64_t npkt,
                           float* d_out_re, float* d_out_im, double* d_noise_var, double* d_corr) {
    if (!c) return CSI_ERR_INVALID_ARG;
    static const char* who = "csi_lmmse_blind_device";
    if (int rc = lmmse_blind_check(c, who, d_ltf_re, d_ltf_im, d_h_re, d_h_im, npkt, d_out_re, d_out_im)) return rc;
    if (int rc = planes_aligned(c, who, {{"d_ltf_re", d_ltf_re}, {"d_ltf_im", d_ltf_im}, {"d_h_re", d_h_re}, {"d_h_im", d_h_im},
                                         {"d_out_re", d_out_re}, {"d_out_im", d_out_im}})) return rc;
    if ((reinterpret_cast<uintptr_t>(d_noise_var) | reinterpret_cast<uintptr_t>(d_corr)) & 7)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: d_noise_var / d_corr must be aligned for doubles (got %p / %p)", who, (void*)d_noise_var, (void*)d_corr);
    return lmmse_blind_launch(c, d_ltf_re, d_ltf_im, d_h_re, d_h_im, npkt, d_out_re, d_out_im, d_noise_var, d_corr);
}

int csi_lmmse_blind(csi_ctx* c, const float* ltf_re, const float* ltf_im, const float* h_re, const float* h_im, int64_t npkt,
                    float* out_re, float* out_im, double* noise_var, double* corr) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return lmmse_blind_host(c, ltf_re, ltf_im, h_re, h_im, npkt, out_re, out_im, noise_var, corr);
}

int csi_null_noise_device(csi_ctx* c, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt, double* d_noise_var) {
    if (!c) return CSI_ERR_INVALID_ARG;
    static const char* who = "csi_null_noise_device";
    if (int rc = null_noise_check(c, who, d_ltf_re, d_ltf_im, npkt, d_noise_var)) return rc;
    if (int rc = planes_aligned(c, who, {{"d_ltf_re", d_ltf_re}, {"d_ltf_im", d_ltf_im}})) return rc;
    if (reinterpret_cast<uintptr_t>(d_noise_var) & 7)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: d_noise_var must be aligned for doubles (got %p)", who, (void*)d_noise_var);
    if (npkt == 0) return CSI_OK;
    return null_noise_launch(c, d_ltf_re, d_ltf_im, npkt, d_noise_var);
}

// ---------------------------------------------------------------- delay-subspace smoother (csi_subspace.hpp, subspace_smooth.hip.h)
int csi_subspace_set_basis(csi_ctx* c, const float* q_re, const float* q_im, int rank) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return subspace_set_basis(c, q_re, q_im, rank);
}

int csi_subspace_smooth_device(csi_ctx* c, const float* d_h_re, const float* d_h_im, int64_t npkt, const float* d_w, float* d_out_re, float* d_out_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    static const char* who = "csi_subspace_smooth_device";
    if (int rc = subspace_check(c, who, d_h_re, d_h_im, npkt, d_out_re, d_out_im)) return rc;
    if (int rc = planes_aligned(c, who, {{"d_h_re", d_h_re}, {"d_h_im", d_h_im}, {"d_out_re", d_out_re}, {"d_out_im", d_out_im}})) return rc;
    if (reinterpret_cast<uintptr_t>(d_w) & 3) return fail(c, CSI_ERR_INVALID_ARG, "%s: d_w must be aligned for floats (got %p)", who, (const void*)d_w);
    return subspace_smooth_device(c, who, d_h_re, d_h_im, npkt, d_w, d_out_re, d_out_im);
}

int csi_subspace_smooth(csi_ctx* c, const float* h_re, const float* h_im, int64_t npkt, const float* w, float* out_re, float* out_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return subspace_smooth_host(c, h_re, h_im, npkt, w, out_re, out_im);
}

// ---------------------------------------------------------------- beam-space smoother across the Tx antennas (csi_beam.hpp, beam_smooth.hip.h)
int csi_beam_set_basis(csi_ctx* c, const float* a_re, const float* a_im, int nb) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return beam_set_basis(c, a_re, a_im, nb);
}

int csi_beam_power_device(csi_ctx* c, const float* d_h_re, const float* d_h_im, int64_t npkt, float* d_power) {
    if (!c) return CSI_ERR_INVALID_ARG;
    static const char* who = "csi_beam_power_device";
    if (int rc = beam_check(c, who, d_h_re, d_h_im, npkt, d_power != nullptr, "h, power")) return rc;
    if (int rc = planes_aligned(c, who, {{"d_h_re", d_h_re}, {"d_h_im", d_h_im}})) return rc;
    if (reinterpret_cast<uintptr_t>(d_power) & 3) return fail(c, CSI_ERR_INVALID_ARG, "%s: d_power must be aligned for floats (got %p)", who, (const void*)d_power);
    if (npkt == 0) return CSI_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return beam_power_launch(c, d_h_re, d_h_im, npkt, d_power);
}

int csi_beam_smooth_device(csi_ctx* c, const float* d_h_re, const float* d_h_im, int64_t npkt, const float* d_w, float* d_out_re, float* d_out_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    static const char* who = "csi_beam_smooth_device";
    if (int rc = beam_check(c, who, d_h_re, d_h_im, npkt, d_out_re && d_out_im, "h, out")) return rc;
    if (int rc = planes_aligned(c, who, {{"d_h_re", d_h_re}, {"d_h_im", d_h_im}, {"d_out_re", d_out_re}, {"d_out_im", d_out_im}})) return rc;
    if (reinterpret_cast<uintptr_t>(d_w) & 3) return fail(c, CSI_ERR_INVALID_ARG, "%s: d_w must be aligned for floats (got %p)", who, (const void*)d_w);
    if (npkt == 0) return CSI_OK;
    if (int rc = beam_planes_disjoint(c, who, d_h_re, d_h_im, d_out_re, d_out_im, npkt)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return beam_smooth_launch(c, d_h_re, d_h_im, npkt, d_w, d_out_re, d_out_im);
}

int csi_beam_smooth(csi_ctx* c, const float* h_re, const float* h_im, int64_t npkt, const float* w, float* out_re, float* out_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return beam_host(c, "csi_beam_smooth", false, h_re, h_im, npkt, w, nullptr, out_re, out_im, nullptr);
}

int csi_beam_wiener_device(csi_ctx* c, const float* d_h_re, const float* d_h_im, int64_t npkt, const float* d_err_var, float* d_out_re, float* d_out_im,
                           float* d_w_out) {
    if (!c) return CSI_ERR_INVALID_ARG;
    static const char* who = "csi_beam_wiener_device";
    if (int rc = beam_check(c, who, d_h_re, d_h_im, npkt, d_err_var && d_out_re && d_out_im, "h, err_var, out")) return rc;
    if (int rc = planes_aligned(c, who, {{"d_h_re", d_h_re}, {"d_h_im", d_h_im}, {"d_out_re", d_out_re}, {"d_out_im", d_out_im}})) return rc;
    if ((reinterpret_cast<uintptr_t>(d_err_var) | reinterpret_cast<uintptr_t>(d_w_out)) & 3)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: d_err_var / d_w_out must be aligned for floats (got %p / %p)", who, (const void*)d_err_var, (void*)d_w_out);
    if (npkt == 0) return CSI_OK;
    if (int rc = beam_planes_disjoint(c, who, d_h_re, d_h_im, d_out_re, d_out_im, npkt)) return rc;
    return beam_wiener_device(c, who, d_h_re, d_h_im, npkt, d_err_var, d_out_re, d_out_im, d_w_out);
}

int csi_beam_wiener(csi_ctx* c, const float* h_re, const float* h_im, int64_t npkt, const float* err_var, float* out_re, float* out_im, float* w_out) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return beam_host(c, "csi_beam_wiener", true, h_re, h_im, npkt, nullptr, err_var, out_re, out_im, w_out);
}

// ---------------------------------------------------------------- hybrid beamforming weights (csi_hybrid.hpp, hybrid_weights.hip.h)
int csi_hybrid_set_dictionary(csi_ctx* c, const float* at_re, const float* at_im, int n_rays) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return hybrid_set_dictionary(c, at_re, at_im, n_rays);
}

int csi_hybrid_weights_device(csi_ctx* c, const float* d_h_re, const float* d_h_im, const float* d_eval_re, const float* d_eval_im, int64_t npkt,
                              int ns, int ntrf, float stop_tol, float* d_fbb_re, float* d_fbb_im, int32_t* d_idx, int32_t* d_n_atoms,
                              float* d_gain, float* d_frf_mean_re, float* d_frf_mean_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (npkt > 0)
        if (int rc = planes_aligned(c, "csi_hybrid_weights_device", {{"d_h_re", d_h_re}, {"d_h_im", d_h_im}, {"d_eval_re", d_eval_re}, {"d_eval_im", d_eval_im},
                                                                  {"d_fbb_re", d_fbb_re}, {"d_fbb_im", d_fbb_im}, {"d_frf_mean_re", d_frf_mean_re},
                                                                  {"d_frf_mean_im", d_frf_mean_im}})) return rc;
    return hybrid_weights_device(c, d_h_re, d_h_im, d_eval_re, d_eval_im, npkt, ns, ntrf, stop_tol, d_fbb_re, d_fbb_im, d_idx, d_n_atoms, d_gain,
                                 d_frf_mean_re, d_frf_mean_im);
}

int csi_hybrid_weights(csi_ctx* c, const float* h_re, const float* h_im, const float* eval_re, const float* eval_im, int64_t npkt, int ns, int ntrf,
                       float stop_tol, float* fbb_re, float* fbb_im, int32_t* idx, int32_t* n_atoms, float* gain, float* frf_mean_re,
                       float* frf_mean_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return hybrid_weights_host(c, h_re, h_im, eval_re, eval_im, npkt, ns, ntrf, stop_tol, fbb_re, fbb_im, idx, n_atoms, gain, frf_mean_re, frf_mean_im);
}

int csi_capture_begin(csi_ctx* c) { return c ? capture_begin(c) : CSI_ERR_INVALID_ARG; }

int csi_capture_end(csi_ctx* c, void** graph) { return c ? capture_end(c, graph) : CSI_ERR_INVALID_ARG; }

int csi_capture_launch(csi_ctx* c, void* graph) { return c ? capture_launch(c, graph) : CSI_ERR_INVALID_ARG; }

void csi_capture_free(csi_ctx* c, void* graph) {
    csi_user_graph* g = static_cast<csi_user_graph*>(graph);
    if (!g) return;
    if (c) { hipSetDevice(c->cfg.device); hipStreamSynchronize(c->stream); }
    if (g->exec) hipGraphExecDestroy(g->exec);
    delete g;
}

// ---------------------------------------------------------------- link simulation (csi_link.hpp, link_sim.hip.h)
int csi_link_frame_bits(int ns, int n_sym, int bps, int64_t* n_info, int64_t* n_coded) {
    return link_frame(ns, n_sym, bps, n_info, n_coded) ? CSI_OK : CSI_ERR_INVALID_ARG;
}

int csi_viterbi_decode_device(csi_ctx* c, const float* d_llr, int64_t ncw, int64_t n_steps, uint8_t* d_bits) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return viterbi_decode_device(c, d_llr, ncw, n_steps, d_bits);
}

int csi_link_sim_device(csi_ctx* c, const float* d_h_re, const float* d_h_im, const float* d_fbb_re, const float* d_fbb_im, const float* d_frf_re,
                        const float* d_frf_im, const float* d_noise_var, uint64_t seed, int64_t first_pkt, int64_t npkt, int ns, int ntrf, int n_sym,
                        int bps, int32_t* d_bit_errors, float* d_evm_rms, float* d_dt_snr_db, float* d_xeq_re, float* d_xeq_im, float* d_csi,
                        float* d_llr, uint8_t* d_bits) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (npkt > 0)
        if (int rc = planes_aligned(c, "csi_link_sim_device", {{"d_h_re", d_h_re}, {"d_h_im", d_h_im}, {"d_fbb_re", d_fbb_re}, {"d_fbb_im", d_fbb_im},
                                                            {"d_frf_re", d_frf_re}, {"d_frf_im", d_frf_im}, {"d_xeq_re", d_xeq_re}, {"d_xeq_im", d_xeq_im}})) return rc;
    return link_sim_device(c, d_h_re, d_h_im, d_fbb_re, d_fbb_im, d_frf_re, d_frf_im, d_noise_var, seed, first_pkt, npkt, ns, ntrf, n_sym, bps,
                           d_bit_errors, d_evm_rms, d_dt_snr_db, d_xeq_re, d_xeq_im, d_csi, d_llr, d_bits);
}

int csi_link_preamble_symbols(int ns) { return link_preamble_symbols(ns); }

int csi_link_sim_rx_device(csi_ctx* c, const float* d_h_re, const float* d_h_im, const float* d_fbb_re, const float* d_fbb_im, const float* d_frf_re,
                           const float* d_frf_im, const float* d_noise_var, uint64_t seed, int64_t first_pkt, int64_t npkt, int ns, int ntrf, int n_sym,
                           int bps, int32_t* d_bit_errors, float* d_evm_rms, float* d_dt_snr_db, float* d_xeq_re, float* d_xeq_im, float* d_csi,
                           float* d_llr, uint8_t* d_bits, float* d_g_nmse, float* d_gest_re, float* d_gest_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (npkt > 0)
        if (int rc = planes_aligned(c, "csi_link_sim_rx_device", {{"d_h_re", d_h_re}, {"d_h_im", d_h_im}, {"d_fbb_re", d_fbb_re}, {"d_fbb_im", d_fbb_im},
                                                               {"d_frf_re", d_frf_re}, {"d_frf_im", d_frf_im}, {"d_xeq_re", d_xeq_re}, {"d_xeq_im", d_xeq_im},
                                                               {"d_gest_re", d_gest_re}, {"d_gest_im", d_gest_im}})) return rc;
    return link_sim_run(c, true, d_h_re, d_h_im, d_fbb_re, d_fbb_im, d_frf_re, d_frf_im, d_noise_var, seed, first_pkt, npkt, ns, ntrf, n_sym, bps,
                        d_bit_errors, d_evm_rms, d_dt_snr_db, d_xeq_re, d_xeq_im, d_csi, d_llr, d_bits, d_g_nmse, d_gest_re, d_gest_im);
}

// ---------------------------------------------------------------- multi-user downlink (csi_mu.hpp, mu_link.hip.h)
int csi_mu_precoder_device(csi_ctx* c, int n_users, const float* const* d_hest_re, const float* const* d_hest_im, int64_t npkt, int ns,
                           const float* d_reg, float* d_w_re, float* d_w_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return mu_precoder_device(c, n_users, d_hest_re, d_hest_im, npkt, ns, d_reg, d_w_re, d_w_im);
}

int csi_mu_link_sim_device(csi_ctx* c, int n_users, const float* const* d_h_re, const float* const* d_h_im, const float* d_w_re, const float* d_w_im,
                           const float* d_noise_var, uint64_t seed, int64_t first_pkt, int64_t npkt, int ns, int n_sym, int bps,
                           int32_t* d_bit_errors, float* d_evm_rms, float* d_sinr_db, float* d_g_re, float* d_g_im, float* d_xeq_re,
                           float* d_xeq_im, float* d_csi, float* d_llr, uint8_t* d_bits) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return mu_link_sim_device(c, n_users, d_h_re, d_h_im, d_w_re, d_w_im, d_noise_var, seed, first_pkt, npkt, ns, n_sym, bps, d_bit_errors,
                              d_evm_rms, d_sinr_db, d_g_re, d_g_im, d_xeq_re, d_xeq_im, d_csi, d_llr, d_bits);
}

// ---------------------------------------------------------------- multi-user hybrid precoder (csi_mu_hybrid.hpp, mu_hybrid.hip.h)
int csi_mu_hybrid_precoder_device(csi_ctx* c, int n_users, const float* const* d_hest_re, const float* const* d_hest_im, int64_t npkt, int ns,
                                  int n_rf, const float* d_reg, float* d_w_re, float* d_w_im, int32_t* d_idx, float* d_fbb_re, float* d_fbb_im,
                                  float* d_score) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return mu_hybrid_precoder_device(c, n_users, d_hest_re, d_hest_im, npkt, ns, n_rf, d_reg, d_w_re, d_w_im, d_idx, d_fbb_re, d_fbb_im, d_score);
}

// ---------------------------------------------------------------- multi-user JSDM precoder (csi_mu_jsdm.hpp, mu_jsdm.hip.h)
int csi_mu_covariance_device(csi_ctx* c, int n_users, const float* const* d_hest_re, const float* const* d_hest_im, int64_t npkt,
                             float* d_cov_re, float* d_cov_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return mu_covariance_device(c, n_users, d_hest_re, d_hest_im, npkt, d_cov_re, d_cov_im);
}

int csi_mu_jsdm_precoder_device(csi_ctx* c, int n_users, const float* const* d_hest_re, const float* const* d_hest_im, int64_t npkt, int ns,
                                const int32_t* group, int r_star, int n_beams, float rank_tol, int flags, const float* d_reg,
                                const float* d_cov_re, const float* d_cov_im, float* d_w_re, float* d_w_im, float* d_frf_re, float* d_frf_im,
                                float* d_fbb_re, float* d_fbb_im, float* d_eig, float* d_ustar_re, float* d_ustar_im, int32_t* d_rank) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return mu_jsdm_precoder_device(c, n_users, d_hest_re, d_hest_im, npkt, ns, group, r_star, n_beams, rank_tol, flags, d_reg, d_cov_re, d_cov_im,
                                   d_w_re, d_w_im, d_frf_re, d_frf_im, d_fbb_re, d_fbb_im, d_eig, d_ustar_re, d_ustar_im, d_rank);
}

// ---------------------------------------------------------------- quantised CSI feedback (csi_feedback.hpp, feedback.hip.h)
int csi_feedback_compress_device(csi_ctx* c, const float* d_h_re, const float* d_h_im, int64_t npkt, int nc, int b_phi, int b_psi, int ng,
                                 uint16_t* d_phi_code, uint16_t* d_psi_code, float* d_phi, float* d_psi, float* d_sigma, float* d_v_re,
                                 float* d_v_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return feedback_compress_device(c, d_h_re, d_h_im, npkt, nc, b_phi, b_psi, ng, d_phi_code, d_psi_code, d_phi, d_psi, d_sigma, d_v_re, d_v_im);
}

int csi_feedback_expand_device(csi_ctx* c, const uint16_t* d_phi_code, const uint16_t* d_psi_code, const float* d_phi, const float* d_psi,
                               const float* d_sigma, int64_t npkt, int nc, int b_phi, int b_psi, int ng, int layout, float* d_out_re,
                               float* d_out_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return feedback_expand_device(c, d_phi_code, d_psi_code, d_phi, d_psi, d_sigma, npkt, nc, b_phi, b_psi, ng, layout, d_out_re, d_out_im);
}

// ---------------------------------------------------------------- receive combining (csi_rx_combine.hpp, rx_combine.hip.h)
int csi_rx_combiner_device(csi_ctx* c, const float* d_hest_re, const float* d_hest_im, int64_t npkt, int ns, float* d_c_re, float* d_c_im,
                           float* d_sigma) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return rx_combiner_device(c, d_hest_re, d_hest_im, npkt, ns, d_c_re, d_c_im, d_sigma);
}

int csi_rx_apply_combiner_device(csi_ctx* c, const float* d_c_re, const float* d_c_im, const float* d_h_re, const float* d_h_im, int64_t npkt,
                                 int ns, float* d_e_re, float* d_e_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return rx_apply_combiner_device(c, d_c_re, d_c_im, d_h_re, d_h_im, npkt, ns, d_e_re, d_e_im);
}

// ---------------------------------------------------------------- accuracy metric
int csi_nmse_device(csi_ctx* c, const float* d_ref_re, const float* d_ref_im, const float* d_est_re, const float* d_est_im,
                    int64_t nlinks, int n_bins, float* d_per_link, double* mean_out) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (nlinks <= 0 || n_bins <= 0 || !d_ref_re || !d_ref_im || !d_est_re || !d_est_im || !mean_out)
        return fail(c, CSI_ERR_INVALID_ARG, "csi_nmse_device: bad argument");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // scratch: the per-link ratios (unless the caller wants them) followed by the fp64 sum
    const size_t need = (d_per_link ? 0 : (size_t)nlinks * sizeof(float)) + 64;
    int rc = ensure_bytes(c, &c->skbuf, &c->skbuf_bytes, need + 64);
    if (rc) return rc;
    float* ratio = d_per_link ? d_per_link : reinterpret_cast<float*>(c->skbuf);
    double* d_sum = reinterpret_cast<double*>(c->skbuf + ((need - 64 + 63) / 64) * 64);
    HIP_TRY(c, hipMemsetAsync(d_sum, 0, sizeof(double), c->stream));
    {
        ProfScope ps(c, K_NMSE, 8.0 * (double)nlinks * n_bins, 16.0 * (double)nlinks * n_bins);
        const unsigned blocks = (unsigned)std::min<int64_t>((nlinks + 3) / 4, 8192);
        hipLaunchKernelGGL(nmse_links_kernel, dim3(blocks), dim3(256), 0, c->stream, d_ref_re, d_ref_im, d_est_re, d_est_im, nlinks, n_bins, ratio);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(nmse_sum_kernel, dim3(1), dim3(1024), 0, c->stream, ratio, nlinks, d_sum);
        HIP_TRY(c, hipGetLastError());
    }
    double sum = 0.0;
    HIP_TRY(c, hipMemcpyAsync(&sum, d_sum, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *mean_out = sum / (double)nlinks;
    return CSI_OK;
}

int csi_nmse(csi_ctx* c, const float* ref_re, const float* ref_im, const float* est_re, const float* est_im, int64_t nlinks,
             int n_bins, double* mean_out) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (nlinks <= 0 || n_bins <= 0 || !ref_re || !ref_im || !est_re || !est_im || !mean_out)
        return fail(c, CSI_ERR_INVALID_ARG, "csi_nmse: bad argument");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // four planes of whole links and 256 bytes of room behind them; csi_nmse_device synchronizes, and every chunk's mean is weighed with its links
    const size_t row = (size_t)n_bins * sizeof(float);
    StagePlane p[] = {{row, ref_re, nullptr}, {row, ref_im, nullptr}, {row, est_re, nullptr}, {row, est_im, nullptr}};
    double total = 0.0;
    int rc = staged_call(c, nlinks, STAGE_BUDGET, 4 * row, 256, false, p, [&](int64_t, int64_t nl) {
        double mean = 0.0;
        const int r = csi_nmse_device(c, p[0].as<float>(), p[1].as<float>(), p[2].as<float>(), p[3].as<float>(), nl, n_bins, nullptr, &mean);
        total += mean * (double)nl;
        return r;
    });
    if (rc) return rc;
    *mean_out = total / (double)nlinks;
    return CSI_OK;
}

int csi_get_option(csi_ctx* c, const char* name, int64_t* value) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (!name || !value) return fail(c, CSI_ERR_INVALID_ARG, "csi_get_option: null argument");
    const std::string n(name);
    if (n == "use_graph") *value = c->use_graph;
    else if (n == "force_tile") *value = c->force_pair_tile;
    else if (n == "xcd_order") *value = c->xcd_order;
    else if (n == "ls_fft_first_max") *value = c->ls_fft_first_max;
    else if (n == "small_call_overlap") *value = c->small_call_overlap;
    else if (n == "small_fused") *value = c->small_fused;
    else if (n == "small_ls_fused") *value = c->small_ls_fused;
    else if (n == "small_ls_launches") *value = c->small_ls_launches;
    else if (n == "small_calls") *value = c->small_calls;
    else if (n == "input_pool") *value = c->input_pool;
    else if (n == "model_type") *value = c->model_type;
    else if (n == "conv_launches") *value = c->conv_launches;
    else if (n == "hybrid_launches") *value = c->hybrid_launches;
    else if (n == "link_launches") *value = c->link_launches;
    else if (n == "subspace_launches") *value = c->subspace_launches;
    else if (n == "beam_launches") *value = c->beam_launches;
    else if (n == "mu_launches") *value = c->mu_launches;
    else if (n == "feedback_launches") *value = c->feedback_launches;
    else if (n == "combine_launches") *value = c->combine_launches;
    else if (n == "lmmse_blind_fallbacks") {
        // counted on the device behind every launch (lmmse_blind_count_kernel): reading it waits for the stream
        if (c->user_capture) return fail(c, CSI_ERR_INVALID_ARG, "csi_get_option: lmmse_blind_fallbacks cannot be read while a capture is open");
        long long v = 0;
        HIP_TRY(c, hipSetDevice(c->cfg.device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipMemcpy(&v, c->lmb_count, sizeof v, hipMemcpyDeviceToHost));
        *value = v;
    }
    else if (n == "scatter_launches") *value = c->scatter_launches;
    else if (n == "scatter_aged_launches") *value = c->scatter_aged_launches;
    else if (n == "forecast_launches") *value = c->forecast_launches;
    else if (n == "cfo_launches") *value = c->cfo_launches;
    else if (n == "sync_launches") *value = c->sync_launches;
    else if (n == "small_rows") *value = c->small_rows;
    else if (n == "small_rows_band") *value = c->small_rows_band;
    else if (n == "f32_engine") *value = c->f32_engine;
    else if (n == "hs_band") *value = c->hs_band;
    else if (n == "band4") *value = c->band4;
    else if (n == "band4_available") *value = c->band_kernel[c->cfg.dtype == CSI_DTYPE_BF16][BAND_FOUR].fn != nullptr;
    else if (n == "band_launches") *value = c->band_launches;
    else if (n == "band4_launches") *value = c->band4_launches;              // read-only: launches of a csi_band4* function (band_run)
    else if (n == "band_split") *value = c->band_split;
    else if (n == "aux_fork_early") *value = c->aux_fork_early;
    else if (n == "l0_stream") *value = c->l0_stream;
    else if (n == "l0_stream_ks") *value = c->l0_stream_ks;
    else if (n == "l0_stream_prepass_rows") *value = c->l0_stream_prepass_rows;
    else if (n == "l0_stream_max_rows") *value = c->l0_stream_max_rows;
    else if (n == "l0_stream_launches") *value = c->l0_stream_launches;
    else if (n == "band_split_launches") *value = c->band_split_launches;
    else if (n == "comm_bytes") *value = c->comm ? c->comm->bytes_broadcast : 0;
    else if (n == "comm_blobs") *value = c->comm ? c->comm->blobs_broadcast : 0;
    else if (n == "comm_world") *value = c->comm ? c->comm->world : 0;
    else if (n == "comm_rank") *value = c->comm ? c->comm->rank : -1;
    else if (n == "hs_act_shift") *value = c->hs_act_shift;
    else if (n == "hs_min_blocks") *value = c->hs_min_blocks;
    else if (n == "hs_fuse_regressor") *value = c->hs_fuse_regressor;
    else if (n == "hs_blocked") *value = c->hs_blocked;
    else if (n == "hs_in_shift") *value = c->hs_in_shift;
    else if (n == "bf16_fused_h1") *value = c->bf16_fused_h1;
    else if (n == "band_tail_split") *value = c->band_tail_split;
    else if (n == "band_tail_launches") *value = c->band_tail_launches;
    else if (n == "bf16_l0_fused_split") *value = c->bf16_l0_fused_split;
    else if (n == "bf16_l0_fused_split_launches") *value = c->bf16_l0_fused_split_launches;
    else if (n == "host_threads") *value = c->host_threads;
    else if (n == "ls_kernel") *value = c->ls_kernel;
    else if (n == "ls_v2") *value = c->ls_v2;
    else if (n == "ls_ringb_min") *value = c->ls_ringb_min;
    else if (n == "ls_pilot_pieces") *value = c->p_pieces;
    else if (n == "ls_mode") *value = ls_plan(c).mode;
    else if (n == "ls_per_cu") *value = ls_plan(c).per_cu;                    // read-only: resident workgroups per CU of the kernel the next LS call runs
    else if (n == "hp_stage_us") *value = c->hostpipe ? (int64_t)c->hostpipe->us_stage : 0;           // read-only: where the last csi_estimate_c128 spent its time
    else if (n == "hp_wait_stage_us") *value = c->hostpipe ? c->hostpipe->us_wait_stage : 0;
    else if (n == "hp_wait_out_us") *value = c->hostpipe ? c->hostpipe->us_wait_out : 0;
    else if (n == "hp_weave_us") *value = c->hostpipe ? c->hostpipe->us_weave : 0;
    else if (n == "hp_total_us") *value = c->hostpipe ? c->hostpipe->us_total : 0;
    else if (n == "hp_chunk_packets") *value = c->hp_chunk_packets;
    else if (n == "train_rank") *value = c->train_rank;
    else if (n == "hp_side_threads") *value = c->hp_side_threads;
    else if (n == "hp_device_weave") *value = c->hp_device_weave;
    else if (n == "hp_direct_out_calls") *value = c->hp_direct_out_calls;
    else if (n == "ls_fast_perm") *value = c->ls_fast_perm;
    else if (n == "ls_overlap_cus") *value = 0;            // see csi_set_option
    else if (n == "ls_pilot_fast") *value = !c->p_fast_ok ? 0 : (c->p_fast_identity ? 1 : 2);     // read-only: 0 generic P, 1 Sylvester Hadamard, 2 a signed permutation of it
    else if (n == "hs_vm_cast") *value = c->hs_vm_cast;
    else if (n == "hs_vm_pair") *value = c->hs_vm_pair;
    else if (n == "hs_l0_mfma") *value = c->hs_l0_mfma;
    else if (n == "hs_l0_mfma16_launches") *value = c->hs_l0_mfma16_launches;    // read-only: layer-0 launches of the 16x16x32 form
    else if (n == "graph_replays") *value = c->graph_replays;                // read-only counters
    else if (n == "hs_launches") *value = c->hs_launches;
    else if (n == "hs_range_fallbacks") *value = c->hs_range_fallbacks;
    else if (n == "hs_weight_pins") *value = c->hs_weight_pins;                  // models pinned to the fp32 MFMA kernels by the load-time check of their split copies
    else if (n == "hs_weight_err_e12") *value = (int64_t)(1e12 * std::max(c->model[0].hs_repr_err, c->model[1].hs_repr_err));    // worst relative representation error x 1e12
    else if (n == "band_available") *value = band_load(c);                      // 1: the fused band kernel's code object is embedded in this build and loads
    else return fail(c, CSI_ERR_INVALID_ARG, "csi_get_option: unknown option '%s'", name);
    return CSI_OK;
}

int csi_set_option(csi_ctx* c, const char* name, int64_t value) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (!name) return fail(c, CSI_ERR_INVALID_ARG, "csi_set_option: null name");
    const std::string n(name);
    if (n == "use_graph") {
        if (!value) drop_graphs(c);
        c->use_graph = value != 0;
    } else if (n == "force_tile") {
        if (value != 0 && value != 128 && value != 256) return fail(c, CSI_ERR_INVALID_ARG, "force_tile must be 0, 128 or 256");
        drop_graphs(c);
        c->force_pair_tile = (int)value;
    } else if (n == "xcd_order") {
        if (value < -1 || value > 1) return fail(c, CSI_ERR_INVALID_ARG, "xcd_order must be -1 (auto), 0 or 1");
        drop_graphs(c);
        c->xcd_order = (int)value;
    } else if (n == "ls_fft_first_max") {
        if (value < 0 || value > 64) return fail(c, CSI_ERR_INVALID_ARG, "ls_fft_first_max must be 0..64");
        c->ls_fft_first_max = (int)value;
        return ls_prepare(c);
    } else if (n == "ls_ringb_min") {
        if (value < 0 || value > 1024) return fail(c, CSI_ERR_INVALID_ARG, "ls_ringb_min must be 0..1024");
        c->ls_ringb_min = (int)value;
        return ls_prepare(c);
    } else if (n == "small_call_overlap") {
        c->small_call_overlap = value == 2 ? 2 : (value != 0);
    } else if (n == "small_ls_fused") {
        drop_graphs(c);
        c->small_ls_fused = value != 0;
    } else if (n == "small_fused") {
        drop_graphs(c);
        c->small_fused = value != 0;
    } else if (n == "small_rows") {
        if (value < 0 || value > 65536) return fail(c, CSI_ERR_INVALID_ARG, "small_rows must be 0..65536");
        drop_graphs(c);
        c->small_rows = (int)value;
    } else if (n == "small_rows_band") {
        if (value < 0 || value > 65536) return fail(c, CSI_ERR_INVALID_ARG, "small_rows_band must be 0..65536");
        drop_graphs(c);
        c->small_rows_band = (int)value;
    } else if (n == "f32_engine") {
        if (value < -1 || value > 1) return fail(c, CSI_ERR_INVALID_ARG, "f32_engine must be -1 (automatic), 0 (fp32 MFMA) or 1 (split f16)");
        drop_graphs(c);
        c->f32_engine = (int)value;
    } else if (n == "hs_blocked") {
        drop_graphs(c);
        c->hs_blocked = value != 0;
    } else if (n == "hs_fuse_regressor") {
        drop_graphs(c);
        c->hs_fuse_regressor = value != 0;
    } else if (n == "hs_band") {
        if (value < 0 || value > 3)
            return fail(c, CSI_ERR_INVALID_ARG, "hs_band must be 0 (separate kernels), 1 (band kernel where its LDS-staged form applies, every fp32 shape it serves), "
                                                "2 (bf16 contexts: also the form with per-lane loads, any nt) or 3 (fp32 contexts: only that form; A/B runs)");
        drop_graphs(c);
        c->hs_band = (int)value;
    } else if (n == "band4") {
        drop_graphs(c);
        c->band4 = value != 0;
    } else if (n == "l0_stream") {
        drop_graphs(c);
        c->l0_stream = value != 0;
    } else if (n == "l0_stream_max_rows") {
        if (value < 8 || value > 4096) return fail(c, CSI_ERR_INVALID_ARG, "l0_stream_max_rows must be 8..4096");
        drop_graphs(c);
        c->l0_stream_max_rows = (int)value;
    } else if (n == "l0_stream_prepass_rows") {
        if (value < 0 || value > 256) return fail(c, CSI_ERR_INVALID_ARG, "l0_stream_prepass_rows must be 0..256");
        drop_graphs(c);
        c->l0_stream_prepass_rows = (int)value;
    } else if (n == "l0_stream_ks") {
        if (value < 0 || value > 256) return fail(c, CSI_ERR_INVALID_ARG, "l0_stream_ks must be 0 (automatic) .. 256");
        drop_graphs(c);
        c->l0_stream_ks = (int)value;
    } else if (n == "aux_fork_early") {
        drop_graphs(c);
        c->aux_fork_early = value != 0;
    } else if (n == "band_split") {
        if (value != -1 && value != 0 && value != 1 && value != 2 && value != 4)
            return fail(c, CSI_ERR_INVALID_ARG, "band_split must be -1 (automatic), 0 / 1 (never) or 2 / 4 (column splits of every band)");
        drop_graphs(c);
        c->band_split = (int)value;
    } else if (n == "hs_min_blocks") {
        if (value < 1 || value > 65536) return fail(c, CSI_ERR_INVALID_ARG, "hs_min_blocks must be 1..65536");
        drop_graphs(c);
        c->hs_min_blocks = (int)value;
    } else if (n == "hs_act_shift" || n == "hs_in_shift") {
        if (value != HS_SHIFT_AUTO && (value < -8 || value > 14)) return fail(c, CSI_ERR_INVALID_ARG, "%s must be -8..14 or 99 (automatic)", name);
        drop_graphs(c);
        (n == "hs_act_shift" ? c->hs_act_shift : c->hs_in_shift) = (int)value;
    } else if (n == "band_tail_split") {
        drop_graphs(c);
        c->band_tail_split = value != 0;
    } else if (n == "bf16_l0_fused_split") {
        drop_graphs(c);
        c->bf16_l0_fused_split = value != 0;
    } else if (n == "bf16_fused_h1") {
        drop_graphs(c);
        c->bf16_fused_h1 = value != 0;
    } else if (n == "host_threads") {
        if (value < 0 || value > 256) return fail(c, CSI_ERR_INVALID_ARG, "host_threads must be 0 (automatic) .. 256");
        if (c->hostpipe) { delete c->hostpipe; c->hostpipe = nullptr; }
        c->host_threads = (int)value;
    } else if (n == "hs_vm_cast" || n == "hs_vm_pair") {
        if (value < 0 || value > 3) return fail(c, CSI_ERR_INVALID_ARG, "%s must be 0 ... 3", name);
        drop_graphs(c);
        (n == "hs_vm_cast" ? c->hs_vm_cast : c->hs_vm_pair) = (int)value;
    } else if (n == "hs_l0_mfma") {
        if (value != 32 && value != 16) return fail(c, CSI_ERR_INVALID_ARG, "hs_l0_mfma must be 32 or 16");
        drop_graphs(c);
        c->hs_l0_mfma = (int)value;
    } else if (n == "ls_overlap_cus") {
        // the LS kernel on a CU-masked side stream beside the matrix kernels: measured slower than the serial order, and it put LS
        // workgroups beside other kernels' MFMA waves.  The path was removed; the name stays so that callers that ask for 0 keep working.
        if (value != 0)
            return fail(c, CSI_ERR_INVALID_ARG, "ls_overlap_cus must be 0: the LS kernel on a side stream beside the matrix kernels was an experiment that "
                                                "measured slower than the serial order and is not part of the product build");
    } else if (n == "hp_side_threads") {
        if (c->hostpipe) { delete c->hostpipe; c->hostpipe = nullptr; }
        c->hp_side_threads = value != 0;
    } else if (n == "hp_device_weave") {
        c->hp_device_weave = value != 0;
    } else if (n == "hp_chunk_packets") {
        if (value < 0 || value > (1 << 20)) return fail(c, CSI_ERR_INVALID_ARG, "hp_chunk_packets must be 0 (automatic) .. 2^20");
        c->hp_chunk_packets = (int)value;
    } else if (n == "train_rank") {
        if (value < 0 || value >= (1 << 20)) return fail(c, CSI_ERR_INVALID_ARG, "train_rank must be 0 .. 2^20 - 1");
        c->train_rank = (int)value;
    } else if (n == "ls_fast_perm") {
        c->ls_fast_perm = value != 0;
        drop_graphs(c);
        return ls_prepare(c);
    } else if (n == "ls_v2") {
        c->ls_v2 = (int)value;
        return ls_prepare(c);
    } else if (n == "ls_debug") {
        // timing experiments: the LS kernels get it as LsArgs::dbg and skip or instrument a phase per bit (1 transforms, 2 despread, 4 stores, ...: ls_estimate.hip.h) - results are wrong when
        // non-zero.  It selects no kernel; a non-zero value keeps the LS estimate of a one-packet call out of the layer-0 launch (ls_default_fwht2).
        c->ls_debug = (int)value;
        return ls_prepare(c);
    } else if (n == "ls_kernel") {
        if (value < 0 || value > 7)
            return fail(c, CSI_ERR_INVALID_ARG, "ls_kernel must be 0 (auto), 1 (FFT first), 2 (chunked), 3 (despread first), 4 (Walsh-Hadamard), "
                                                "5 (Walsh-Hadamard, LDS-DMA fed), 6 (generic P, LDS-DMA fed, fp32 despread) or 7 (generic P, bf16-split despread)");
        c->ls_kernel = (int)value;
        return ls_prepare(c);
    } else {
        return fail(c, CSI_ERR_INVALID_ARG, "csi_set_option: unknown option '%s'", name);
    }
    return CSI_OK;
}


// ---------------------------------------------------------------- on-box fine-tuning
static int trainer_of(csi_ctx* c, int model, const char* fn, csi_trainer** t) {
    if (model < 0 || model > 1) return fail(c, CSI_ERR_INVALID_ARG, "%s: model must be 0 or 1", fn);
    if (!c->trainer[model]) return fail(c, CSI_ERR_NOT_READY, "%s: csi_train_begin was not called for model %d", fn, model);
    *t = c->trainer[model];
    return CSI_OK;
}

int csi_train_begin(csi_ctx* c, int model, const csi_train_config* tc, const csi_tensor* tensors, int n) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (model < 0 || model > 1 || !tc || n < 0 || (n > 0 && !tensors)) return fail(c, CSI_ERR_INVALID_ARG, "csi_train_begin: bad argument");
    if (c->model_type == CSI_MODEL_CONV1D)
        return fail(c, CSI_ERR_INVALID_ARG, "csi_train_begin: training a CONV1D model is not supported (it needs the conv backward pass and BatchNormalization "
                    "batch statistics over B x len_ltf positions); train the FC models, or train CONV1D models elsewhere and load them");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int rc = tr_begin(c, model, tc, tensors, n);
    if (rc && c->trainer[model]) { tr_free(c->trainer[model]); c->trainer[model] = nullptr; }
    return rc;
}

int csi_train_step(csi_ctx* c, int model, const float* x, const float* y, int64_t B, float noise_std, float* loss) {
    if (!c) return CSI_ERR_INVALID_ARG;
    csi_trainer* t = nullptr;
    if (int rc0 = trainer_of(c, model, "csi_train_step", &t)) return rc0;
    if (!x || !y || B < 2 || B > (1 << 20) || noise_std < 0.f) return fail(c, CSI_ERR_INVALID_ARG, "csi_train_step: bad argument (2 <= B <= 2^20)");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int rc = tr_backward(c, t, x, y, nullptr, (int)B, noise_std, nullptr);
    if (rc) return rc;
    const int rc2 = tr_apply(c, t);
    if (rc2) return rc2;
    if (loss) {
        HIP_TRY(c, hipMemcpyAsync(loss, t->loss, sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return CSI_OK;
}

int csi_train_backward(csi_ctx* c, int model, const float* x, const float* y, int64_t B, float noise_std, float* loss) {
    if (!c) return CSI_ERR_INVALID_ARG;
    csi_trainer* t = nullptr;
    if (int rc0 = trainer_of(c, model, "csi_train_backward", &t)) return rc0;
    if (!x || !y || B < 2 || B > (1 << 20) || noise_std < 0.f) return fail(c, CSI_ERR_INVALID_ARG, "csi_train_backward: bad argument (2 <= B <= 2^20)");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return tr_backward(c, t, x, y, nullptr, (int)B, noise_std, loss);
}

int csi_train_grads(csi_ctx* c, int model, float** d_grads, int64_t* count) {
    if (!c) return CSI_ERR_INVALID_ARG;
    csi_trainer* t = nullptr;
    if (int rc0 = trainer_of(c, model, "csi_train_grads", &t)) return rc0;
    if (!d_grads || !count) return fail(c, CSI_ERR_INVALID_ARG, "csi_train_grads: bad argument");
    *d_grads = t->gflat;
    *count = t->gcount;
    return CSI_OK;
}

int csi_train_apply(csi_ctx* c, int model) {
    if (!c) return CSI_ERR_INVALID_ARG;
    csi_trainer* t = nullptr;
    if (int rc0 = trainer_of(c, model, "csi_train_apply", &t)) return rc0;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return tr_apply(c, t);
}

int csi_train_eval(csi_ctx* c, int model, const float* x, const float* y, int64_t B, float* loss) {
    if (!c) return CSI_ERR_INVALID_ARG;
    csi_trainer* t = nullptr;
    if (int rc0 = trainer_of(c, model, "csi_train_eval", &t)) return rc0;
    if (!x || !y || !loss || B < 1 || B > (1 << 20)) return fail(c, CSI_ERR_INVALID_ARG, "csi_train_eval: bad argument");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return tr_eval(c, t, x, y, nullptr, (int)B, loss);
}

int csi_train_set_dataset(csi_ctx* c, int model, const float* ltf_table, int64_t n_rows, const int32_t* ltf_row, const int32_t* itx,
                          const float* y, int64_t N) {
    if (!c) return CSI_ERR_INVALID_ARG;
    csi_trainer* t = nullptr;
    if (int rc0 = trainer_of(c, model, "csi_train_set_dataset", &t)) return rc0;
    if (!ltf_table || !ltf_row || !y || n_rows <= 0 || N <= 0 || N > 0x7fffffff || (c->cfg.nt > 0 && !itx))
        return fail(c, CSI_ERR_INVALID_ARG, "csi_train_set_dataset: bad argument");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return tr_set_dataset(c, t, ltf_table, n_rows, ltf_row, itx, y, N);
}

// mode 0: step (backward + Adam), 1: backward only, 2: inference-mode loss
int csi_train_indexed(csi_ctx* c, int model, int mode, const int32_t* ids, int64_t B, float noise_std, float* loss) {
    if (!c) return CSI_ERR_INVALID_ARG;
    csi_trainer* t = nullptr;
    if (int rc0 = trainer_of(c, model, "csi_train_indexed", &t)) return rc0;
    if (!ids || mode < 0 || mode > 2 || B < (mode == 2 ? 1 : 2) || B > (1 << 20) || noise_std < 0.f || (mode == 2 && !loss))
        return fail(c, CSI_ERR_INVALID_ARG, "csi_train_indexed: bad argument");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (mode == 2) return tr_eval(c, t, nullptr, nullptr, ids, (int)B, loss);
    int rc = tr_backward(c, t, nullptr, nullptr, ids, (int)B, noise_std, mode == 1 ? loss : nullptr);
    if (rc || mode == 1) return rc;
    rc = tr_apply(c, t);
    if (rc) return rc;
    if (loss) {
        HIP_TRY(c, hipMemcpyAsync(loss, t->loss, sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return CSI_OK;
}

int csi_train_set_lr(csi_ctx* c, int model, float lr) {
    if (!c) return CSI_ERR_INVALID_ARG;
    csi_trainer* t = nullptr;
    if (int rc0 = trainer_of(c, model, "csi_train_set_lr", &t)) return rc0;
    if (!(lr > 0.f)) return fail(c, CSI_ERR_INVALID_ARG, "csi_train_set_lr: lr must be positive");
    t->tc.lr = lr;
    return CSI_OK;
}

int csi_train_get(csi_ctx* c, int model, const char* name, float* out, int64_t count) {
    if (!c) return CSI_ERR_INVALID_ARG;
    csi_trainer* t = nullptr;
    if (int rc0 = trainer_of(c, model, "csi_train_get", &t)) return rc0;
    if (!name || !out || count <= 0) return fail(c, CSI_ERR_INVALID_ARG, "csi_train_get: bad argument");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return tr_get(c, t, name, out, count);
}

int csi_train_end(csi_ctx* c, int model, int commit) {
    if (!c) return CSI_ERR_INVALID_ARG;
    csi_trainer* t = nullptr;
    if (int rc0 = trainer_of(c, model, "csi_train_end", &t)) return rc0;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = CSI_OK;
    if (commit) {
        // hand the trained tensors to the inference model exactly as a caller of csi_load_weights would
        const csi_config& cf = c->cfg;
        std::vector<std::string> names;
        std::vector<std::vector<float>> data;
        std::vector<std::pair<int64_t, int64_t>> shape;
        auto add = [&](const std::string& nm, int64_t r, int64_t q) {
            names.push_back(nm);
            shape.push_back({r, q});
            data.emplace_back((size_t)(r * q));
        };
        for (int li = 0; li <= cf.n_hidden; ++li) {
            const auto& l = t->layers[li];
            const std::string base = layer_tensor_base(cf, li);
            add(base + ".kernel", l.in, l.out);
            add(base + ".bias", 1, l.out);
            if (li < cf.n_hidden && cf.use_bn)
                for (const char* sfx : {".gamma", ".beta", ".moving_mean", ".moving_variance"}) add("bn" + std::to_string(li) + sfx, 1, l.out);
        }
        std::vector<csi_tensor> ts(names.size());
        for (size_t i = 0; i < names.size() && !rc; ++i) {
            rc = tr_get(c, t, names[i].c_str(), data[i].data(), (int64_t)data[i].size());
            ts[i] = csi_tensor{names[i].c_str(), data[i].data(), shape[i].first, shape[i].second};
        }
        if (!rc) rc = csi_load_weights(c, model, ts.data(), (int)ts.size());
    }
    hipStreamSynchronize(c->stream);
    tr_free(t);
    c->trainer[model] = nullptr;
    return rc;
}

// ---- multi-GPU: RCCL weight broadcast inside the C-ABI (csi_comm.hpp)
int csi_get_unique_id(char id[CSI_UNIQUE_ID_BYTES]) {
    if (!id) return fail(nullptr, CSI_ERR_INVALID_ARG, "csi_get_unique_id: null buffer");
    RcclApi& r = rccl();
    if (!r.lib) return fail(nullptr, CSI_ERR_HIP, "%s", r.why.c_str());
    nccl_uid u;
    NCCL_TRY(nullptr, r.GetUniqueId(&u));
    std::memcpy(id, u.internal, CSI_UNIQUE_ID_BYTES);
    return CSI_OK;
}

int csi_comm_init(csi_ctx* c, int rank, int world, const char id[CSI_UNIQUE_ID_BYTES]) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (!id || world < 1 || rank < 0 || rank >= world) return fail(c, CSI_ERR_INVALID_ARG, "csi_comm_init: bad rank %d / world %d", rank, world);
    RcclApi& r = rccl();
    if (!r.lib) return fail(c, CSI_ERR_HIP, "%s", r.why.c_str());
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    comm_free(c);
    c->comm = new csi_comm;
    c->comm->rank = rank;
    c->comm->world = world;
    nccl_uid u;
    std::memcpy(u.internal, id, CSI_UNIQUE_ID_BYTES);
    NCCL_TRY(c, r.CommInitRank(&c->comm->comm, world, u, rank));
    HIP_TRY(c, hipMalloc(&c->comm->wire, WIRE_STATUS_OFF + 64));
    return CSI_OK;
}

int csi_comm_destroy(csi_ctx* c) {
    if (!c) return CSI_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    if (c->stream) hipStreamSynchronize(c->stream);
    comm_free(c);
    return CSI_OK;
}

int csi_broadcast_weights(csi_ctx* c, int root) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (!c->comm || !c->comm->comm) return fail(c, CSI_ERR_NOT_READY, "csi_broadcast_weights: csi_comm_init has not been called");
    csi_comm& cm = *c->comm;
    if (root < 0 || root >= cm.world) return fail(c, CSI_ERR_INVALID_ARG, "csi_broadcast_weights: root %d of %d ranks", root, cm.world);
    RcclApi& r = rccl();
    const csi_config& cf = c->cfg;
    HIP_TRY(c, hipSetDevice(cf.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    drop_graphs(c);
    const bool is_root = cm.rank == root;
    // 1. the host-side scalars that belong to the device blobs: root -> everybody
    WireMeta w;
    std::memset(&w, 0, sizeof w);
    if (is_root) {
        wire_fill(c, w);
        HIP_TRY(c, hipMemcpyAsync(cm.wire, &w, sizeof w, hipMemcpyHostToDevice, c->stream));
    }
    NCCL_TRY(c, r.Broadcast(cm.wire, cm.wire, sizeof w, NCCL_CHAR, root, cm.comm, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&w, cm.wire, sizeof w, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // 2. receivers: the record against the own csi_config, the old model out, buffers of the root's sizes
    std::vector<WBlob> blobs;
    int rc_local = CSI_OK;
    if (is_root) wire_blobs(c, w, blobs);
    else rc_local = wire_receive(c, w, blobs, "csi_broadcast_weights");
    // 3. every rank learns whether EVERY rank can take the blobs (one min all-reduce of a status word): a refusing rank - other
    //    csi_config, allocation failure - must not leave the others inside the grouped broadcast, and it must not enter it itself
    int32_t* d_status = reinterpret_cast<int32_t*>(static_cast<char*>(cm.wire) + WIRE_STATUS_OFF);
    int32_t ok = rc_local == CSI_OK ? 1 : 0;
    const std::string why_local = c->err;
    HIP_TRY(c, hipMemcpyAsync(d_status, &ok, sizeof ok, hipMemcpyHostToDevice, c->stream));
    NCCL_TRY(c, r.AllReduce(d_status, d_status, 1, NCCL_INT32, NCCL_MIN, cm.comm, c->stream));
    int32_t all_ok = 0;
    HIP_TRY(c, hipMemcpyAsync(&all_ok, d_status, sizeof all_ok, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    cm.bytes_broadcast = 0;
    cm.blobs_broadcast = 0;
    if (rc_local != CSI_OK) { c->err = why_local; return rc_local; }
    if (!all_ok) {
        if (!is_root) wire_drop_receiver(c);
        return fail(c, CSI_ERR_INVALID_ARG, "csi_broadcast_weights: another rank refused the root's record (its csi_config differs or its allocation failed; "
                                             "see csi_last_error there) - nothing was broadcast");
    }
    // 4. the blobs themselves, device to device, one group.  The group is always closed, also on an error inside it
    cm.blobs_broadcast = (int64_t)blobs.size();
    int rc_g = r.GroupStart();
    if (rc_g == 0) {
        int rc_b = 0;
        for (WBlob& b : blobs) {
            rc_b = r.Broadcast(*b.p, *b.p, b.bytes, NCCL_CHAR, root, cm.comm, c->stream);
            if (rc_b) break;
            cm.bytes_broadcast += (int64_t)b.bytes;
        }
        const int rc_e = r.GroupEnd();
        rc_g = rc_b ? rc_b : rc_e;
    }
    if (rc_g) {
        if (!is_root) wire_drop_receiver(c);
        return fail(c, CSI_ERR_HIP, "csi_broadcast_weights: ncclBroadcast group failed: %s", r.GetErrorString ? r.GetErrorString(rc_g) : "?");
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // 5. what is derived locally
    if (!is_root) {
        const int rc = wire_finish(c, w);
        if (rc) { const std::string why = c->err; wire_drop_receiver(c); c->err = why; return rc; }
    }
    return CSI_OK;
}

// The same protocol inside one process: dst takes what src holds, device to device.  Runs every line of the receiver side of
// csi_broadcast_weights (wire_receive / wire_blobs / wire_finish) - which a single-GPU box cannot reach through RCCL, two ranks
// on one GPU being refused - and is useful by itself: a second context (another stream, another packet range, another GPU of the
// same process) without a second pass through csi_load_weights and the host copies of the tensors.
int csi_clone_weights(csi_ctx* dst, const csi_ctx* src_c) {
    if (!dst) return CSI_ERR_INVALID_ARG;
    csi_ctx* src = const_cast<csi_ctx*>(src_c);        // only pointer VALUES are read from it
    if (!src || src == dst) return fail(dst, CSI_ERR_INVALID_ARG, "csi_clone_weights: source context is null or the destination itself");
    HIP_TRY(dst, hipSetDevice(src->cfg.device));
    HIP_TRY(dst, hipStreamSynchronize(src->stream));   // whatever still writes the source's buffers (csi_train_end, a pilot table build)
    HIP_TRY(dst, hipSetDevice(dst->cfg.device));
    HIP_TRY(dst, hipStreamSynchronize(dst->stream));
    drop_graphs(dst);
    WireMeta w;
    wire_fill(src, w);
    std::vector<WBlob> to, from;
    int rc = wire_receive(dst, w, to, "csi_clone_weights");
    if (rc) return rc;
    wire_blobs(src, w, from);
    if (to.size() != from.size()) { wire_drop_receiver(dst); return fail(dst, CSI_ERR_INVALID_ARG, "csi_clone_weights: internal - %zu buffers here, %zu on the source", to.size(), from.size()); }
    for (size_t i = 0; i < to.size(); ++i) {
        if (to[i].bytes != from[i].bytes || !*from[i].p) { wire_drop_receiver(dst); return fail(dst, CSI_ERR_INVALID_ARG, "csi_clone_weights: internal - buffer %zu differs", i); }
        const hipError_t e = src->cfg.device == dst->cfg.device
                                 ? hipMemcpyAsync(*to[i].p, *from[i].p, to[i].bytes, hipMemcpyDeviceToDevice, dst->stream)
                                 : hipMemcpyPeerAsync(*to[i].p, dst->cfg.device, *from[i].p, src->cfg.device, to[i].bytes, dst->stream);
        if (e != hipSuccess) { wire_drop_receiver(dst); return fail(dst, CSI_ERR_HIP, "csi_clone_weights: device copy failed: %s", hipGetErrorString(e)); }
    }
    HIP_TRY(dst, hipStreamSynchronize(dst->stream));
    rc = wire_finish(dst, w);
    if (rc) { const std::string why = dst->err; wire_drop_receiver(dst); dst->err = why; return rc; }
    return CSI_OK;
}

int csi_synchronize(csi_ctx* c) {
    if (!c) return CSI_ERR_INVALID_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float hit = 0.f;
    bool low = false;
    int rc = hs_range_check(c, &hit, &low);
    if (rc) return rc;
    if (hit > 0.f)
        return fail(c, CSI_ERR_RANGE, "split-f16 engine: an operand reached %.4g after scaling (f16 limit 65504) in a device-pointer call since the "
                    "last check - the outputs of those calls are not valid; lower hs_in_shift / hs_act_shift or set f32_engine to 0 and run them again", (double)hit);
    if (low)
        return fail(c, CSI_ERR_RANGE, "split-f16 engine: a row of operands stayed below %.3g after scaling in a device-pointer call since the last check - "
                    "its results may miss the 1e-5 contract; raise hs_in_shift / hs_act_shift or set f32_engine to 0 and run those calls again", (double)HS_LOW_REPORT);
    return CSI_OK;
}

// Range guard of the split-f16 engine behind a host-buffer entry point (the stream is synchronised, the caller's buffers
// are still here): if an operand left the f16 range, or a row sat in its denormals, run `again` on the fp32 MFMA kernels.
// The retry must not replay a hipGraph captured with the split-engine kernels (the host pipeline calls the device
// entry points with recurring buffers and chunk sizes, i.e. recurring graph keys): graphs are dropped and graph use is
// off for its duration; and the guard is read once more behind it - nothing of the split engine may have run.
static int range_guard_retry(csi_ctx* c, const std::function<int()>& again) {
    float hit = 0.f;
    bool low = false;
    int rc = hs_range_check(c, &hit, &low);
    if (rc || (hit == 0.f && !low)) return rc;
    ++c->hs_range_fallbacks;
    const int engine = c->f32_engine;
    const bool graph = c->use_graph;
    drop_graphs(c);
    c->f32_engine = 0;
    c->use_graph = false;
    const int64_t launches = c->hs_launches;
    rc = again();
    c->f32_engine = engine;
    c->use_graph = graph;
    drop_graphs(c);
    if (rc) return rc;
    if (c->hs_launches != launches)
        return fail(c, CSI_ERR_RANGE, "range-guard retry: the split-f16 engine ran again although f32_engine was 0");
    return CSI_OK;
}

// ---- host-buffer entry points: two-slot pipeline of csi_hostpipe.hpp
static int host_packets(csi_ctx* c, const float* re, const float* im, int64_t npkt, float* o_re, float* o_im,
                        int n_out, bool ls) {
    return hp_packets(c, re, im, npkt, o_re, o_im, n_out,
                      [c, ls](const float* d_re, const float* d_im, int64_t np, float* d_ore, float* d_oim) {
                          return ls ? csi_ls_estimate_device(c, d_re, d_im, np, d_ore, d_oim) : csi_predict_device(c, d_re, d_im, np, d_ore, d_oim);
                      });
}

int csi_predict(csi_ctx* c, const float* ltf_re, const float* ltf_im, int64_t npkt, float* out_re, float* out_im) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (npkt < 0 || (npkt > 0 && (!ltf_re || !ltf_im || !out_re || !out_im)))
        return fail(c, CSI_ERR_INVALID_ARG, "csi_predict: bad argument");
    if (npkt == 0) return CSI_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    rc = host_packets(c, ltf_re, ltf_im, npkt, out_re, out_im, c->cfg.n_out, false);
    if (rc) return rc;
    // range guard of the split-f16 engine: an operand beyond the f16 range, or a row of operands deep in
    // its denormal range -> the same call again on the
    // fp32 MFMA kernels (the caller's buffers are still here), so that this entry point never returns inf
    return range_guard_retry(c, [&] { return host_packets(c, ltf_re, ltf_im, npkt, out_re, out_im, c->cfg.n_out, false); });
}

int csi_estimate_c128(csi_ctx* c, const double* ltf_c128, int64_t npkt, float* dnn_c64, float* ls_c64) {
    int rc = check_ready(c, dnn_c64 != nullptr);
    if (rc) return rc;
    if (npkt < 0 || (npkt > 0 && (!ltf_c128 || (!dnn_c64 && !ls_c64))))
        return fail(c, CSI_ERR_INVALID_ARG, "csi_estimate_c128: bad argument");
    if (npkt == 0) return CSI_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    rc = hp_estimate_c128(c, ltf_c128, false, npkt, dnn_c64, ls_c64);
    if (rc || !dnn_c64) return rc;
    // range guard of the split-f16 engine, as in csi_predict: repeat the DNN on the fp32 MFMA kernels
    return range_guard_retry(c, [&] { return hp_estimate_c128(c, ltf_c128, false, npkt, dnn_c64, nullptr); });
}

int csi_estimate_c64(csi_ctx* c, const float* ltf_c64, int64_t npkt, float* dnn_c64, float* ls_c64) {
    int rc = check_ready(c, dnn_c64 != nullptr);
    if (rc) return rc;
    if (npkt < 0 || (npkt > 0 && (!ltf_c64 || (!dnn_c64 && !ls_c64))))
        return fail(c, CSI_ERR_INVALID_ARG, "csi_estimate_c64: bad argument");
    if (npkt == 0) return CSI_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    rc = hp_estimate_c128(c, ltf_c64, true, npkt, dnn_c64, ls_c64);
    if (rc || !dnn_c64) return rc;
    return range_guard_retry(c, [&] { return hp_estimate_c128(c, ltf_c64, true, npkt, dnn_c64, nullptr); });
}

int csi_ls_estimate(csi_ctx* c, const float* ltf_re, const float* ltf_im, int64_t npkt, float* h_re, float* h_im) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (npkt < 0 || (npkt > 0 && (!ltf_re || !ltf_im || !h_re || !h_im)))
        return fail(c, CSI_ERR_INVALID_ARG, "csi_ls_estimate: bad argument");
    if (npkt == 0) return CSI_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return host_packets(c, ltf_re, ltf_im, npkt, h_re, h_im, LS_NDATA, true);
}

int csi_predict_samples(csi_ctx* c, int model, const float* x, int64_t B, float* y) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (model < 0 || model > 1) return fail(c, CSI_ERR_INVALID_ARG, "csi_predict_samples: model must be 0 or 1");
    Model& m = c->model[model];
    if (!m.loaded) return fail(c, CSI_ERR_NOT_READY, "weights of the %s model are not loaded", model ? "imag" : "real");
    if (B < 0 || (B > 0 && (!x || !y))) return fail(c, CSI_ERR_INVALID_ARG, "csi_predict_samples: bad argument");
    if (B == 0) return CSI_OK;
    const csi_config& cf = c->cfg;
    HIP_TRY(c, hipSetDevice(cf.device));
    int maxh = 0;
    for (int i = 0; i < cf.n_hidden; ++i) maxh = std::max(maxh, cf.hidden[i]);
    // rows arrive raw, [B][len_ltf + nt], as keras' predict receives them; a decimated-input model pools them on the device into the
    // [B][len_ltf / 2 + nt] rows its layer 0 reads (input_pool_rows_kernel)
    // (a CONV1D model: its front end turns them into [B][64 len_ltf + nt] rows, the pilot columns copied - conv_frontend.hip.h)
    const bool pooled = l0_features(c);
    const int raw_in = pooled ? cf.len_ltf + cf.nt : c->d_in;
    auto upload_rows = [&](float* d_raw, float* d_rows, int64_t r0, int64_t nb) -> int {
        HIP_TRY(c, hipMemcpyAsync(pooled ? d_raw : d_rows, x + (size_t)r0 * raw_in, (size_t)nb * raw_in * sizeof(float), hipMemcpyHostToDevice, c->stream));
        if (!pooled) return CSI_OK;
        if (c->model_type == CSI_MODEL_CONV1D) return launch_conv_frontend(c, &m, nullptr, d_raw, nullptr, d_rows, nullptr, nb, raw_in, c->d_in, cf.nt, false);
        ProfScope ps(c, K_INPUT_POOL, 0.0, 4.0 * (double)nb * (raw_in + c->d_in));
        const unsigned blocks = (unsigned)std::min<size_t>(((size_t)nb * c->d_in + 255) / 256, 8192);
        if (c->input_pool == POOL_MAX)
            hipLaunchKernelGGL(input_pool_rows_kernel<POOL_MAX>, dim3(blocks), dim3(256), 0, c->stream, d_raw, raw_in, d_rows, c->d_in, (int)nb, c->l0_k, cf.nt);
        else
            hipLaunchKernelGGL(input_pool_rows_kernel<POOL_AVG>, dim3(blocks), dim3(256), 0, c->stream, d_raw, raw_in, d_rows, c->d_in, (int)nb, c->l0_k, cf.nt);
        HIP_TRY(c, hipGetLastError());
        return CSI_OK;
    };
    if (cf.dtype == CSI_DTYPE_BF16) {
        const int ldx = (c->d_in + B_BK - 1) / B_BK * B_BK;
        const size_t per_row_b = (size_t)c->d_in * 4 + (size_t)ldx * 2 + 2 * (size_t)maxh * 2 + (size_t)cf.n_out * 4 + (pooled ? (size_t)raw_in * 4 : 0);
        int64_t chunk_b = std::min<int64_t>(B, std::max<int64_t>(1, ((int64_t)512 << 20) / (int64_t)per_row_b));
        int rcb = ensure_bytes(c, &c->stage, &c->stage_bytes, per_row_b * (size_t)chunk_b + 1024);
        if (rcb) return rcb;
        char* base = c->stage;
        float* d_xf = reinterpret_cast<float*>(base);      base += (size_t)chunk_b * c->d_in * 4;
        float* d_yf = reinterpret_cast<float*>(base);      base += (size_t)chunk_b * cf.n_out * 4;
        bf16_t* d_xb = reinterpret_cast<bf16_t*>(base);    base += (size_t)chunk_b * ldx * 2;
        bf16_t* hb0 = reinterpret_cast<bf16_t*>(base);     base += (size_t)chunk_b * maxh * 2;
        bf16_t* hb1 = reinterpret_cast<bf16_t*>(base);     base += (size_t)chunk_b * maxh * 2;
        float* d_raw = reinterpret_cast<float*>(base);     // [chunk_b][raw_in] (pooled models)
        for (int64_t r0 = 0; r0 < B; r0 += chunk_b) {
            const int nb = (int)std::min(chunk_b, B - r0);
            rcb = upload_rows(d_raw, d_xf, r0, nb);
            if (rcb) return rcb;
            {
                ProfScope ps(c, K_CAST_BF16, 0.0, 6.0 * nb * c->d_in);
                const unsigned blocks = (unsigned)std::min<size_t>(((size_t)nb * ldx + 255) / 256, 8192);
                hipLaunchKernelGGL(f32_to_bf16_rows_kernel, dim3(blocks), dim3(256), 0, c->stream, d_xf, d_xb, nb, c->d_in, ldx);
                HIP_TRY(c, hipGetLastError());
            }
            const Layer& l0 = m.layers[0];
            GemmBf16Args q{};
            q.A = d_xb; q.lda = ldx;
            q.Bt = l0.Wb; q.ldb = l0.ldwb;
            q.C = hb0; q.ldc = l0.out;
            q.M = nb; q.N = l0.out; q.K = c->d_in;
            q.bias = l0.bias; q.scale = l0.scale; q.shift = l0.shift;
            q.k_per_split = l0.ldwb;
            rcb = launch_gemm_bf16<EPI_BIAS_RELU_AFFINE, true>(c, K_NAIVE_DENSE0, q, 1);
            if (rcb) return rcb;
            // hidden layers 1.. ping-pong starting from hb1, so layer 1 never overwrites its input
            rcb = bf16_tail(c, m, hb0, nb, hb1, hb0, d_yf, 1);
            if (rcb) return rcb;
            HIP_TRY(c, hipMemcpyAsync(y + (size_t)r0 * cf.n_out, d_yf, (size_t)nb * cf.n_out * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        return CSI_OK;
    }
    const size_t per_row = ((size_t)c->d_in + 2 * (size_t)maxh + cf.n_out + (pooled ? (size_t)raw_in : 0)) * sizeof(float);
    int64_t chunk = std::max<int64_t>(1, ((int64_t)512 << 20) / (int64_t)per_row);
    chunk = std::min(chunk, B);
    int rc = ensure_bytes(c, &c->stage, &c->stage_bytes, per_row * (size_t)chunk + G_SLACK_FLOATS * sizeof(float));
    if (rc) return rc;
    float* d_x = reinterpret_cast<float*>(c->stage);
    float* hb[2];
    // the staging buffer is shared with csi_nmse / csi_lmmse_estimate (raw caller data): keep G_SLACK_FLOATS of zeros
    // behind the input rows, the K tail of the last row (d_in is rarely a multiple of the k-tile) reads into them
    hb[0] = d_x + (size_t)chunk * c->d_in + G_SLACK_FLOATS;
    hb[1] = hb[0] + (size_t)chunk * maxh;
    float* d_y = hb[1] + (size_t)chunk * maxh;
    float* d_raw = d_y + (size_t)chunk * cf.n_out;       // [chunk][raw_in] (pooled models)
    for (int64_t r0 = 0; r0 < B; r0 += chunk) {
        const int64_t nb = std::min(chunk, B - r0);
        rc = upload_rows(d_raw, d_x, r0, nb);
        if (rc) return rc;
        HIP_TRY(c, hipMemsetAsync(d_x + (size_t)nb * c->d_in, 0, G_SLACK_FLOATS * sizeof(float), c->stream));
        const float* cur = d_x;
        int cur_ld = c->d_in, w = 0;
        for (int li = 0; li <= cf.n_hidden; ++li) {
            const Layer& l = m.layers[li];
            GemmArgs q{};
            q.A = cur; q.lda = cur_ld;
            q.Bt = l.Wt; q.ldb = l.ldw;
            q.M = (int)nb; q.N = l.out; q.K = l.in;
            q.bias = l.bias; q.scale = l.scale; q.shift = l.shift;
            q.k_per_split = ((l.in + G_BK - 1) / G_BK) * G_BK;
            if (li == cf.n_hidden) {
                q.C = d_y; q.ldc = cf.n_out;
                rc = launch_gemm<EPI_BIAS>(c, K_REGRESSOR, q, 1);
            } else {
                q.C = hb[w]; q.ldc = l.out;
                rc = launch_gemm<EPI_BIAS_RELU_AFFINE>(c, li == 0 ? K_NAIVE_DENSE0 : K_DENSE_HIDDEN, q, 1);
                cur = hb[w];
                cur_ld = l.out;
                w ^= 1;
            }
            if (rc) return rc;
        }
        HIP_TRY(c, hipMemcpyAsync(y + (size_t)r0 * cf.n_out, d_y, (size_t)nb * cf.n_out * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return CSI_OK;
}

// ---- device memory plumbing
int csi_device_malloc(csi_ctx* c, void** dptr, int64_t bytes) {
    if (!c || !dptr || bytes < 0) return c ? fail(c, CSI_ERR_INVALID_ARG, "csi_device_malloc: bad argument") : CSI_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    *dptr = nullptr;
    if (bytes == 0) return CSI_OK;
    if (hipMalloc(dptr, (size_t)bytes) != hipSuccess) {
        *dptr = nullptr;
        return fail(c, CSI_ERR_NOMEM, "csi_device_malloc: %lld bytes failed", (long long)bytes);
    }
    return CSI_OK;
}

int csi_device_free(csi_ctx* c, void* dptr) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (!dptr) return CSI_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipFree(dptr));
    return CSI_OK;
}

int csi_host_malloc(csi_ctx* c, void** ptr, int64_t bytes) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (!ptr || bytes <= 0) return fail(c, CSI_ERR_INVALID_ARG, "csi_host_malloc: bad argument");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (hipHostMalloc(ptr, (size_t)bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, CSI_ERR_NOMEM, "csi_host_malloc: %lld bytes of pinned host memory are not available", (long long)bytes);
    }
    return CSI_OK;
}

int csi_host_free(csi_ctx* c, void* ptr) {
    if (!c) {          // a buffer may outlive the context that allocated it (python finalizers run in any order)
        if (ptr && hipHostFree(ptr) != hipSuccess) { (void)hipGetLastError(); return CSI_ERR_HIP; }
        return CSI_OK;
    }
    if (ptr) HIP_TRY(c, hipHostFree(ptr));
    return CSI_OK;
}

int csi_memcpy_h2d(csi_ctx* c, void* dst_dev, const void* src_host, int64_t bytes) {
    if (!c || bytes < 0 || (bytes > 0 && (!dst_dev || !src_host))) return c ? fail(c, CSI_ERR_INVALID_ARG, "csi_memcpy_h2d: bad argument") : CSI_ERR_INVALID_ARG;
    HIP_TRY(c, hipMemcpyAsync(dst_dev, src_host, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CSI_OK;
}

int csi_memcpy_d2h(csi_ctx* c, void* dst_host, const void* src_dev, int64_t bytes) {
    if (!c || bytes < 0 || (bytes > 0 && (!dst_host || !src_dev))) return c ? fail(c, CSI_ERR_INVALID_ARG, "csi_memcpy_d2h: bad argument") : CSI_ERR_INVALID_ARG;
    HIP_TRY(c, hipMemcpyAsync(dst_host, src_dev, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CSI_OK;
}

int csi_synth_white(csi_ctx* c, uint64_t seed, int64_t first_pkt, int64_t npkt, float* d_re, float* d_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (npkt < 0 || first_pkt < 0 || (npkt > 0 && (!d_re || !d_im))) return fail(c, CSI_ERR_INVALID_ARG, "csi_synth_white: bad argument");
    if (npkt == 0) return CSI_OK;
    if (int rc = planes_aligned(c, "csi_synth_white", {{"d_re", d_re}, {"d_im", d_im}})) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t per_pkt = (size_t)c->cfg.nr * c->cfg.len_ltf;
    const size_t n = per_pkt * (size_t)npkt;
    ProfScope ps(c, K_SYNTH_WHITE, 0.0, 8.0 * n);
    hipLaunchKernelGGL(synth_white_kernel, dim3(2048), dim3(256), 0, c->stream, seed, (uint64_t)first_pkt * per_pkt, n, d_re, d_im);
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

int csi_synth_structured(csi_ctx* c, uint64_t seed, int64_t first_pkt, int64_t npkt, const float* snr_db, int n_taps, uint32_t flags,
                         float* d_ltf_re, float* d_ltf_im, float* d_h_re, float* d_h_im, float* d_noise_std) {
    if (!c) return CSI_ERR_INVALID_ARG;
    const csi_config& cf = c->cfg;
    if (cf.nt < 4 || cf.nt % 4 != 0 || cf.len_ltf != LS_SYM * cf.nt)
        return fail(c, CSI_ERR_INVALID_ARG, "csi_synth_structured: needs a context of nt >= 1 antennas and len_ltf = 320 nt (nt %d, len_ltf %d)", cf.nt, cf.len_ltf);
    if (npkt < 0 || first_pkt < 0) return fail(c, CSI_ERR_INVALID_ARG, "csi_synth_structured: npkt %lld / first_pkt %lld must not be negative", (long long)npkt, (long long)first_pkt);
    if (n_taps == 0) n_taps = 8;
    if (n_taps < 1 || n_taps > SS_MAX_TAPS) return fail(c, CSI_ERR_INVALID_ARG, "csi_synth_structured: n_taps %d outside 1 .. %d", n_taps, SS_MAX_TAPS);
    if (flags & ~1u) return fail(c, CSI_ERR_INVALID_ARG, "csi_synth_structured: unknown flag bits 0x%x (bit 0 = amplitude scale)", flags);
    if (npkt == 0) return CSI_OK;
    if (!d_ltf_re || !d_ltf_im) return fail(c, CSI_ERR_INVALID_ARG, "csi_synth_structured: null ltf planes for %lld packets", (long long)npkt);
    if ((d_h_re == nullptr) != (d_h_im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "csi_synth_structured: the channel planes come as a pair (one of h_re / h_im is null)");
    if (!c->pilot_ok) return fail(c, CSI_ERR_NOT_READY, "csi_synth_structured: no pilot matrix set (csi_set_pilot)");
    if (c->user_capture && snr_db) return fail(c, CSI_ERR_INVALID_ARG, "csi_synth_structured: a call with an SNR array uploads it and cannot be captured");
    if (((reinterpret_cast<uintptr_t>(d_ltf_re) | reinterpret_cast<uintptr_t>(d_ltf_im) | reinterpret_cast<uintptr_t>(d_h_re) | reinterpret_cast<uintptr_t>(d_h_im)) & 15) != 0)
        return fail(c, CSI_ERR_INVALID_ARG, "csi_synth_structured: output planes must start on 16-byte boundaries");
    const int64_t nblk = npkt * cf.nr;
    if (nblk > 0x7fffffff) return fail(c, CSI_ERR_INVALID_ARG, "csi_synth_structured: %lld packets x %d rx antennas exceed one launch (2^31 - 1 items)", (long long)npkt, cf.nr);
    HIP_TRY(c, hipSetDevice(cf.device));
    // tap profile and per-packet noise factors in double on the host, one upload; the item powers follow them in the same buffer
    const size_t n_host = SS_MAX_TAPS + (snr_db ? (size_t)npkt : 0);
    int rc = ensure_bytes(c, &c->synth_ws, &c->synth_ws_bytes, (n_host + (snr_db ? (size_t)nblk : 0)) * sizeof(float));
    if (rc) return rc;
    c->synth_host.resize(n_host);
    for (int t = 0; t < SS_MAX_TAPS; ++t) c->synth_host[t] = (float)(std::exp(-0.5 * t) / std::sqrt(2.0));
    for (int64_t p = 0; snr_db && p < npkt; ++p) c->synth_host[SS_MAX_TAPS + p] = (float)(0.5 * std::pow(10.0, -0.1 * (double)snr_db[p]));
    float* ws = reinterpret_cast<float*>(c->synth_ws);
    HIP_TRY(c, hipMemcpyAsync(ws, c->synth_host.data(), n_host * sizeof(float), hipMemcpyHostToDevice, c->stream));
    SynthArgs a{};
    a.P = c->P; a.tw = c->tw; a.ltf_nat = c->ltf_nat; a.bin_pos = c->bin_pos;
    a.decay = ws;
    a.fac = snr_db ? ws + SS_MAX_TAPS : nullptr;
    a.part = snr_db ? ws + n_host : nullptr;
    a.ltf_re = d_ltf_re; a.ltf_im = d_ltf_im; a.h_re = d_h_re; a.h_im = d_h_im; a.noise_std = d_noise_std;
    a.seed = seed; a.first_pkt = first_pkt;
    a.nt = cf.nt; a.nr = cf.nr; a.len_ltf = cf.len_ltf; a.n_taps = n_taps;
    a.amp = (flags & 1u) ? (float)(std::sqrt((double)(LS_FFT - 14)) / LS_FFT) : 1.0f;
    const size_t lds = synth_lds_floats(cf.nt, n_taps) * sizeof(float);
    if (lds > 160 * 1024) return fail(c, CSI_ERR_INVALID_ARG, "csi_synth_structured: nt %d with %d taps needs %zu bytes of LDS (160 KiB per workgroup)", cf.nt, n_taps, lds);
    if (lds > 48 * 1024 && lds > c->synth_lds_attr) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)synth_structured_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIP_TRY(c, hipFuncSetAttribute((const void*)synth_structured_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        c->synth_lds_attr = lds;
    }
    const double bytes = (double)nblk * (8.0 * cf.len_ltf + (d_h_re ? 8.0 * cf.nt * LS_NDATA : 0.0));
    ProfScope ps(c, K_SYNTH_STRUCTURED, 0.0, bytes);
    if (snr_db) hipLaunchKernelGGL(synth_structured_kernel<true>, dim3((unsigned)nblk), dim3(SS_THREADS), lds, c->stream, a);
    hipLaunchKernelGGL(synth_structured_kernel<false>, dim3((unsigned)nblk), dim3(SS_THREADS), lds, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

int csi_synth_scattering(csi_ctx* c, uint64_t seed, int64_t first_pkt, int64_t npkt, const float* snr_db, const csi_scatter_config* cfg,
                         float* d_ltf_re, float* d_ltf_im, float* d_h_re, float* d_h_im, float* d_noise_std, float* d_tau) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return synth_scattering(c, seed, first_pkt, npkt, snr_db, cfg, d_ltf_re, d_ltf_im, d_h_re, d_h_im, d_noise_std, d_tau);
}

int csi_scatter_channel_at_device(csi_ctx* c, uint64_t seed, int64_t first_pkt, int64_t npkt, const csi_scatter_config* cfg,
                                  const csi_motion_config* motion, const double* t_s, int n_times, float* d_h_re, float* d_h_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return scatter_channel_at(c, seed, first_pkt, npkt, cfg, motion, t_s, n_times, d_h_re, d_h_im);
}

// ---- channel forecast (csi_forecast.hpp, forecast.hip.h)
int csi_forecast_gram_device(csi_ctx* c, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t npkt, float* d_t_re, float* d_t_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return forecast_gram_device(c, d_x_re, d_x_im, n_snd, npkt, d_t_re, d_t_im);
}

int csi_forecast_gram_blocks_device(csi_ctx* c, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t n_blocks, int64_t block_floats,
                                    float* d_t_re, float* d_t_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return forecast_gram_blocks_device(c, "csi_forecast_gram_blocks_device", d_x_re, d_x_im, n_snd, n_blocks, block_floats, d_t_re, d_t_im);
}

int csi_forecast_fit_device(csi_ctx* c, const float* d_t_re, const float* d_t_im, int n_snd, int64_t npkt, int order, int steps, double ridge,
                            uint32_t flags, float* d_c_re, float* d_c_im, float* d_fit_err, int32_t* d_info) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return forecast_fit_device(c, d_t_re, d_t_im, n_snd, npkt, order, steps, ridge, flags, d_c_re, d_c_im, d_fit_err, d_info);
}

int csi_forecast_apply_device(csi_ctx* c, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t npkt, int order,
                              const float* d_c_re, const float* d_c_im, float* d_out_re, float* d_out_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return forecast_apply_device(c, d_x_re, d_x_im, n_snd, npkt, order, d_c_re, d_c_im, d_out_re, d_out_im);
}

int csi_forecast_device(csi_ctx* c, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t npkt, int order, int steps, double ridge,
                        uint32_t flags, float* d_out_re, float* d_out_im, float* d_c_re, float* d_c_im, float* d_fit_err, int32_t* d_info) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return forecast_device(c, "csi_forecast_device", d_x_re, d_x_im, n_snd, npkt, order, steps, ridge, flags, d_out_re, d_out_im, d_c_re, d_c_im,
                           d_fit_err, d_info);
}

int csi_forecast(csi_ctx* c, const float* const* x_re, const float* const* x_im, int n_snd, int64_t npkt, int order, int steps, double ridge, uint32_t flags,
                 float* out_re, float* out_im, float* c_re, float* c_im, float* fit_err, int32_t* info) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return forecast_host(c, x_re, x_im, n_snd, npkt, order, steps, ridge, flags, out_re, out_im, c_re, c_im, fit_err, info);
}

int csi_sounding_noise_device(csi_ctx* c, uint64_t seed, int64_t first_pkt, int64_t npkt, const float* d_err_var, const float* d_x_re, const float* d_x_im,
                              float* d_out_re, float* d_out_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return sounding_noise_device(c, seed, first_pkt, npkt, d_err_var, d_x_re, d_x_im, d_out_re, d_out_im);
}

// ---- carrier frequency offset (csi_cfo.hpp, cfo.hip.h)
int csi_cfo_estimate_device(csi_ctx* c, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt, int cp_skip, double* d_eps, float* d_quality) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return cfo_estimate_device(c, d_ltf_re, d_ltf_im, npkt, cp_skip, d_eps, d_quality);
}

int csi_cfo_rotate_device(csi_ctx* c, const float* d_in_re, const float* d_in_im, int64_t npkt, const double* d_eps, double scale, float* d_out_re,
                          float* d_out_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return cfo_rotate_device(c, d_in_re, d_in_im, npkt, d_eps, scale, d_out_re, d_out_im);
}

int csi_cfo_correct_device(csi_ctx* c, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt, int cp_skip, float* d_out_re, float* d_out_im,
                           double* d_eps, float* d_quality) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return cfo_correct_device(c, "csi_cfo_correct_device", d_ltf_re, d_ltf_im, npkt, cp_skip, d_out_re, d_out_im, d_eps, d_quality);
}

int csi_cfo_correct(csi_ctx* c, const float* ltf_re, const float* ltf_im, int64_t npkt, int cp_skip, float* out_re, float* out_im, double* eps,
                    float* quality) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return cfo_correct_host(c, ltf_re, ltf_im, npkt, cp_skip, out_re, out_im, eps, quality);
}

// ---- symbol timing (csi_sync.hpp, sync.hip.h)
int csi_sync_embed_device(csi_ctx* c, uint64_t seed, int64_t first_pkt, int64_t npkt, int span, const int32_t* d_theta, const float* d_margin_std,
                          const float* d_x_re, const float* d_x_im, float* d_cap_re, float* d_cap_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return sync_embed_device(c, seed, first_pkt, npkt, span, d_theta, d_margin_std, d_x_re, d_x_im, d_cap_re, d_cap_im);
}

int csi_sync_estimate_device(csi_ctx* c, const float* d_cap_re, const float* d_cap_im, int64_t npkt, int span, double rho, int32_t* d_theta, double* d_eps,
                             float* d_quality, double* d_metric) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return sync_estimate_device(c, d_cap_re, d_cap_im, npkt, span, rho, d_theta, d_eps, d_quality, d_metric);
}

int csi_sync_extract_device(csi_ctx* c, const float* d_cap_re, const float* d_cap_im, int64_t npkt, int span, const int32_t* d_theta, const double* d_eps,
                            float* d_out_re, float* d_out_im) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return sync_extract_device(c, d_cap_re, d_cap_im, npkt, span, d_theta, d_eps, d_out_re, d_out_im);
}

int csi_sync_correct_device(csi_ctx* c, const float* d_cap_re, const float* d_cap_im, int64_t npkt, int span, double rho, uint32_t flags, float* d_out_re,
                            float* d_out_im, int32_t* d_theta, double* d_eps, float* d_quality) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return sync_correct_device(c, "csi_sync_correct_device", d_cap_re, d_cap_im, npkt, span, rho, flags, d_out_re, d_out_im, d_theta, d_eps, d_quality);
}

int csi_sync_correct(csi_ctx* c, const float* cap_re, const float* cap_im, int64_t npkt, int span, double rho, uint32_t flags, float* out_re, float* out_im,
                     int32_t* theta, double* eps, float* quality) {
    if (!c) return CSI_ERR_INVALID_ARG;
    return sync_correct_host(c, cap_re, cap_im, npkt, span, rho, flags, out_re, out_im, theta, eps, quality);
}

// ---- profiling
int csi_profile_enable(csi_ctx* c, int on) {
    if (!c) return CSI_ERR_INVALID_ARG;
    int rc = prof_collect(c);
    c->prof_on = on != 0;
    return rc;
}

int csi_profile_reset(csi_ctx* c) {
    if (!c) return CSI_ERR_INVALID_ARG;
    int rc = prof_collect(c);
    for (int i = 0; i < K_COUNT; ++i) {
        c->prof_ms[i] = 0;
        c->prof_launches[i] = 0;
        c->prof_flops[i] = 0;
        c->prof_bytes[i] = 0;
    }
    return rc;
}

int csi_profile_band_skeleton(csi_ctx* c, int64_t rows, int iters, double* ms_per_launch, double* executed_flops) {
    if (!c) return CSI_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return band_skeleton_time(c, rows, iters, ms_per_launch, executed_flops);
}

int csi_profile_pcie(csi_ctx* c, int64_t h2d_bytes, int64_t d2h_bytes, double* ms_h2d, double* ms_d2h, double* ms_both) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (h2d_bytes < 0 || d2h_bytes < 0 || (h2d_bytes == 0 && d2h_bytes == 0)) return fail(c, CSI_ERR_INVALID_ARG, "csi_profile_pcie: bad byte counts");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return hp_pcie_probe(c, h2d_bytes, d2h_bytes, ms_h2d, ms_d2h, ms_both);
}

int csi_profile_num_kernels(void) { return K_COUNT; }

const char* csi_profile_kernel_name(int id) { return (id >= 0 && id < K_COUNT) ? kKernelNames[id] : ""; }

int csi_profile_query(csi_ctx* c, int id, double* total_ms, int64_t* launches, double* flops, double* bytes) {
    if (!c) return CSI_ERR_INVALID_ARG;
    if (id < 0 || id >= K_COUNT) return fail(c, CSI_ERR_INVALID_ARG, "csi_profile_query: kernel id %d out of range", id);
    int rc = prof_collect(c);
    if (rc) return rc;
    if (total_ms) *total_ms = c->prof_ms[id];
    if (launches) *launches = c->prof_launches[id];
    if (flops) *flops = c->prof_flops[id];
    if (bytes) *bytes = c->prof_bytes[id];
    return CSI_OK;
}

}  // extern "C"
