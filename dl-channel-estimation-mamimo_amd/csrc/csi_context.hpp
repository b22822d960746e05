// csi_context.hpp - the csi_ctx object behind include/csi_mamimo.h and the host-side plumbing every
// entry point shares: error reporting, per-kernel HIP-event profiling, device buffers, weight storage.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/csi_mamimo.h"
#include "gemm_f32.hip.h"
#include "gemm_bf16.hip.h"
#include "gemm_hs.hip.h"
#include "gemm_hs_band.hip.h"
#include "l0_hs_stream.hip.h"
#include "ls_estimate.hip.h"
#include "lmmse.hip.h"
#include "hybrid_weights.hip.h"
#include "metrics.hip.h"
#include "input_pool.hip.h"
#include "conv_frontend.hip.h"
#include "synth_structured.hip.h"
#include "synth_scattering.hip.h"
#include "link_sim.hip.h"
#include "subspace_smooth.hip.h"
#include "beam_smooth.hip.h"
#include "mu_link.hip.h"
#include "mu_hybrid.hip.h"
#include "mu_jsdm.hip.h"
#include "feedback.hip.h"
#include "rx_combine.hip.h"

using namespace csi;

namespace {

enum KernelId {
    K_LAYER0_LTF = 0,    // layer 0, LTF part, once per (packet, rx)
    K_SPLITK_REDUCE,     // deterministic split-K combine of layer 0
    K_PAIR_DENSE,        // first per-pair layer, h1 generated in the prologue  (dominant)
    K_DENSE_HIDDEN,      // further hidden layers
    K_REGRESSOR,         // fc_regressor
    K_LS_ESTIMATE,       // FFT + despread
    K_NAIVE_DENSE0,      // un-shared layer 0 of csi_predict_samples
    K_SYNTH_WHITE,
    K_PILOT_TABLE,
    K_CAST_BF16,         // fp32 -> bf16 of the preambles (bf16 mode)
    K_PAIR_H1_BF16,      // materialise h1 in bf16 (bf16 mode)
    K_LMMSE,             // Levinson solve of the LMMSE smoother
    K_TRAIN_GEMM,        // forward / dgrad / wgrad products of csi_train_step
    K_TRAIN_ELEMWISE,    // BatchNormalization, dropout, loss, Adam of csi_train_step
    K_NMSE,              // per-link NMSE metric
    K_PAIR_DENSE_TAIL,   // the last, partly filled round of band workgroups launched in column splits ("band_tail_split", round 6)
    K_INPUT_POOL,        // MaxPooling1D / AveragePooling1D of the preambles of a decimated-input model (csi_set_input_pool)
    K_CONV_FRONTEND,     // Conv1D + BN + AveragePooling1D front end of a CONV1D model (csi_set_model_type, conv_frontend.hip.h)
    K_HYB_SVD,           // hybrid weights: dominant right singular vectors per (packet, subcarrier) (hybrid_weights.hip.h)
    K_HYB_CORR,          // hybrid weights: dictionary correlation + argmax of one matching-pursuit step (fp32 MFMA)
    K_HYB_SOLVE,         // hybrid weights: Cholesky row, coefficients and residual of one matching-pursuit step
    K_HYB_FINISH,        // hybrid weights: gain and per-packet mean of the analog part
    K_SYNTH_STRUCTURED,  // known-channel sounding packets (synth_structured.hip.h): the power pass and the packet pass of csi_synth_structured
    K_LINK_TXRX,         // link simulation: encoder, precoder, true channel, zero forcing and soft bits per (packet, subcarrier) (link_sim.hip.h)
    K_LINK_VITERBI,      // link simulation: one-wavefront Viterbi decoder per codeword, traceback and bit errors
    K_SUBSPACE_SMOOTH,   // delay-subspace smoother y = Q diag(w) Q^H x of a CSI tensor (csi_subspace_smooth, subspace_smooth.hip.h).  In front of the
                         // ids below, not behind them: tests/test_blind_lmmse_host.py pins the last four names of the table, and every reader
                         // of the table looks an id up by its name (csi_profile_kernel_name)
    K_MU_PRECODER,       // multi-user downlink: (regularised) zero-forcing precoder per (packet, subcarrier) (mu_link.hip.h); placed like K_SUBSPACE_SMOOTH
    K_MU_TXRX,           // multi-user downlink: encoders + transmit / receive pass per (packet, user)
    K_MU_BEAM_SCORE,     // multi-user hybrid precoder (mu_hybrid.hip.h): wideband beam score per (packet, stream, ray) (fp32 MFMA); placed like K_SUBSPACE_SMOOTH
    K_MU_BEAM_SELECT,    // multi-user hybrid precoder: greedy choice of the n_rf beams of a packet
    K_MU_HYBRID_PRECODER,// multi-user hybrid precoder: zero forcing on the effective channel B Frf per (packet, subcarrier)
    K_MU_COV,            // multi-user JSDM precoder (mu_jsdm.hip.h): transmit covariance per (packet, user) (fp32 MFMA); placed like K_SUBSPACE_SMOOTH
    K_MU_JSDM_EIG,       // multi-user JSDM precoder: Jacobi eigenvectors per (packet, group), both stages (covariance; nulled covariance -> beams)
    K_MU_JSDM_BASEBAND,  // multi-user JSDM precoder: zero forcing on the effective channel B Frf per (packet, subcarrier), per group or jointly
    K_FB_COMPRESS,       // quantised CSI feedback (feedback.hip.h): singular vectors, Givens angles and codes per (packet, reported carrier)
    K_FB_EXPAND,         // quantised CSI feedback: the report expanded into precoder or CSI planes per (packet, carrier)
    K_RX_COMBINER,       // receive combining (rx_combine.hip.h): the U^H combiner of a CSI estimate per (packet, carrier); placed like K_SUBSPACE_SMOOTH
    K_RX_COMBINE,        // receive combining: E = C H on CSI planes, streaming
    K_BEAM_POWER,        // beam-space smoother (csi_beam_*, beam_smooth.hip.h): beam power E per (packet, rx, beam); placed like K_SUBSPACE_SMOOTH
    K_BEAM_SMOOTH,       // beam-space smoother: y = A diag(w) A^H x across the Tx antennas
    K_SCATTER_AGED,      // the scattering channel of a moving user at later times (scatter_aged.hip.h): the one kernel of csi_scatter_channel_at_device; placed like K_SUBSPACE_SMOOTH
    K_FORECAST_GRAM,     // channel forecast (csi_forecast_*, forecast.hip.h): Gram matrix of the soundings per (packet, rx) (fp32 MFMA); placed like K_SUBSPACE_SMOOTH
    K_FORECAST_FIT,      // channel forecast: normal equations, ridge and fp64 Cholesky per (packet, rx) or per packet
    K_FORECAST_APPLY,    // channel forecast: y = sum_m c_m x_{P-1-m}, streaming
    K_SYNC_METRIC,       // symbol timing (csi_sync_*, sync.hip.h): cyclic-prefix timing metric, theta_hat / eps_hat / quality per packet; placed like K_SUBSPACE_SMOOTH
    K_SYNC_EXTRACT,      // symbol timing: y[n] = c[theta + n] exp(-2 pi i eps n / 256), streaming
    K_SYNC_EMBED,        // symbol timing: the packet at theta inside a capture with noise margins, streaming
    K_SOUNDING_NOISE,    // white estimation error on a CSI plane pair (csi_sounding_noise_device)
    K_CFO_CORR,          // carrier frequency offset (csi_cfo_*, cfo.hip.h): cyclic-prefix correlation, eps_hat and quality per packet; placed like K_SUBSPACE_SMOOTH
    K_CFO_ROTATE,        // carrier frequency offset: y = x exp(2 pi i scale eps n / 256), streaming
    K_SYNTH_SCATTERING,  // known-channel sounding packets of the scattering channel (synth_scattering.hip.h): the power pass and the packet pass of csi_synth_scattering
    K_LMMSE_NULL_NOISE,  // blind LMMSE smoother (csi_lmmse_blind, lmmse.hip.h): noise variance from the null carriers of the sounding symbols
    K_LMMSE_FREQ_CORR,   // blind LMMSE smoother: sample frequency correlation of the LS rows
    K_LMMSE_BLIND,       // blind LMMSE smoother: Levinson solve on the measured first column (+ the fallback count)
    K_COUNT
};
const char* const kKernelNames[K_COUNT] = {
    "layer0_ltf_gemm", "splitk_reduce", "pair_dense_gemm", "dense_hidden_gemm", "regressor_gemm",
    "ls_estimate", "naive_dense0_gemm", "synth_white", "pilot_table", "cast_bf16", "pair_h1_bf16", "lmmse_levinson",
    "train_gemm", "train_elementwise", "nmse_links", "pair_dense_tail", "input_pool", "conv_frontend",
    "hybrid_svd", "hybrid_corr_argmax", "hybrid_solve", "hybrid_finish", "synth_structured", "link_txrx", "link_viterbi",
    "subspace_smooth", "mu_precoder", "mu_txrx", "mu_beam_score", "mu_beam_select", "mu_hybrid_precoder", "mu_cov", "mu_jsdm_eig", "mu_jsdm_baseband", "fb_compress", "fb_expand", "rx_combiner", "rx_combine", "beam_power", "beam_smooth", "scatter_aged", "forecast_gram", "forecast_fit", "forecast_apply", "sync_metric", "sync_extract", "sync_embed", "sounding_noise", "cfo_corr", "cfo_rotate", "synth_scattering", "lmmse_null_noise", "lmmse_freq_corr", "lmmse_blind"};

thread_local std::string g_create_error;

constexpr int CSI_WIRE_MAX_NT = 128;      // Hadamard-equivalent pilots are recognised up to this many antennas (the Walsh-Hadamard LS kernels' range)
constexpr int HS_SHIFT_AUTO = 99;         // "hs_in_shift" / "hs_act_shift" options: scale chosen from the data / from the model

struct Layer {
    float* Wt = nullptr;      // [out][ldw] (K-major, ldw = in rounded up to 32, zero padded)   fp32 mode
    int ldw = 0;
    bf16_t* Wb = nullptr;     // [out][ldwb] bf16 (K-major, ldwb = in rounded up to 64)          bf16 mode
    int ldwb = 0;
    bf16_t* Wb_p = nullptr;   // regressor behind one per-pair layer, bf16 mode: 256 rows, k permuted inside every group of 16 (band kernel)
    uint16_t* Wh_f = nullptr; // regressor behind ONE per-pair layer: Wh with that layer's BN scale folded into its rows (fused kernel)
    int wshift_f = 0;
    uint16_t* Wh_p = nullptr; // the same folded regressor weights, 256 rows (rows >= out zero), k permuted inside every group of 16
                              // (hs_band_kperm): the fused band kernel (gemm_hs_band.hip.h / band_kernel_gen.py)
    int ashift_pre = 4;       // like ashift for this layer's relu output BEFORE BatchNormalization (its scale lives in the next weights)
    uint16_t* Wh = nullptr;   // [out][ldwh] split-f16 ("hs", gemm_hs.hip.h) copy of Wt * 2^wshift; layer 0: LTF columns only
    int ldwh = 0;             // halves per row = 2 * (in rounded up to 16)
    int wshift = 0;
    int ashift = 4;           // split engine: this layer's OUTPUT activations are carried times 2^ashift (from its BN vectors at load);
                              // layer 0: its relu output BEFORE BatchNormalization (the scale lives in layer 1's split weights)
    float* bias = nullptr;    // [out]
    float* bias_hs = nullptr; // [out]  split engine (layers >= 1): bias + (BN shift of the previous layer) . W
    float* scale = nullptr;   // [out]  BN: gamma * rsqrt(var + eps)   (1 without BN)
    float* shift = nullptr;   // [out]  BN: beta - mean * scale        (0 without BN)
    int in = 0, out = 0;
};

struct Model {
    std::vector<Layer> layers;   // n_hidden dense layers + regressor (last)
    float* W0p = nullptr;        // [nt][H1] pilot rows of fc_dense0.kernel, row-major
    float* W0rm = nullptr;       // [lenLTF][H1] LTF rows of fc_dense0.kernel as stored (skinny layer-0 kernel)
    float* T = nullptr;          // [nt][H1] pilot table incl. bias
    float* T_hs = nullptr;       // [nt][H1] 2^T_hs_shift * T: what the split-f16 pair kernel adds (gemm_hs.hip.h)
    int T_hs_shift = HS_SHIFT_AUTO;   // HS_SHIFT_AUTO = not built
    float* T_sw = nullptr;       // T (bf16 contexts) / T_hs (split engine) in the slab order of the staged band kernels (band_tsw_kernel); rebuilt with the table
    bool T_sw_ok = false;
    uint16_t* Wt1 = nullptr;     // bf16 contexts: the pair layer's and the regressor's weights pre-tiled for the register-blocked band kernel
    uint16_t* Wt2 = nullptr;     // (band4_tile_kernel, built on first use from layers[1].Wb / layers[2].Wb_p)
    bool tiled_ok = false;
    float* conv = nullptr;       // CONV1D models: [CONV_PRM_FLOATS] taps, bias, BN scale, BN shift of the front end (conv_frontend.hip.h)
    float* l0_rowmax = nullptr;  // [4096] row maxima of a mid-size call's preambles (l0_row_max_kernel -> l0_hs_stream_kernel)
    bool loaded = false;
    bool table_ok = false;
    // csi_load_weights measures how well the split-f16 copies represent the fp32 matrices: the weight scale comes from max |w| of a
    // whole matrix, so a matrix whose bulk sits ~2^20 below its largest entry would lose its lo halves to the f16 denormals -
    // silently (the range guard watches activations).  Worst OUTPUT ROW ||w_o s - (hi + lo)_o|| / ||w_o s|| over the split matrices of
    // this model (per row: a whole-matrix norm is carried by the outlier itself); above 2^-20 the model is pinned to the fp32 MFMA
    // kernels (hs_static_ok) and "hs_weight_pins" counts it.
    double hs_repr_err = 0.0;
    bool hs_repr_ok = true;
};

// The ONE table of the device buffers csi_load_weights fills (prepared on the host by csi_weights.hpp): per row the pointer, the payload bytes as a function of
// the scalars above, and the zeroed slack allocated behind the payload (256 bytes: bf16 copies, 4096: split-f16 copies, UPLOAD_SLACK: every fp32 array - the K
// tail of a GEMM's last tile over-reads into finite memory).  The upload, free_layer / free_model, and the blobs and has[] flags of the weight broadcast
// (csi_comm.hpp) walk it IN THIS ORDER, the order on the wire; a new weight layout is one row here plus the function in csi_weights.hpp that prepares it.
constexpr size_t UPLOAD_SLACK = G_SLACK_FLOATS * sizeof(float);
struct LayerBuf { const char* name; void** (*slot)(const Layer&); size_t (*payload)(const Layer&); size_t slack; };
struct ModelBuf { const char* name; void** (*slot)(const Model&); size_t (*payload)(const Model&, int nt, int l0_k); size_t slack; };
#define CSI_LAYER_BUF(f, bytes, slack) {#f, [](const Layer& l) { return (void**)&const_cast<Layer&>(l).f; }, [](const Layer& l) { return (size_t)(bytes); }, slack}
#define CSI_MODEL_BUF(f, bytes) {#f, [](const Model& m) { return (void**)&const_cast<Model&>(m).f; }, \
                                 [](const Model& m, int nt, int l0_k) { (void)m; (void)nt; (void)l0_k; return (size_t)(bytes); }, UPLOAD_SLACK}
enum { LB_Wt, LB_Wb, LB_Wb_p, LB_Wh, LB_Wh_f, LB_Wh_p, LB_bias, LB_bias_hs, LB_scale, LB_shift, LAYER_BUFS };
enum { MB_W0p, MB_W0rm, MB_conv, MODEL_BUFS };
const LayerBuf kLayerBufs[LAYER_BUFS] = {
    CSI_LAYER_BUF(Wt, (size_t)l.out * l.ldw * 4, UPLOAD_SLACK),   CSI_LAYER_BUF(Wb, (size_t)l.out * l.ldwb * 2, 256),   CSI_LAYER_BUF(Wb_p, (size_t)256 * l.ldwb * 2, 256),
    CSI_LAYER_BUF(Wh, (size_t)l.out * l.ldwh * 2, 4096),          CSI_LAYER_BUF(Wh_f, (size_t)l.out * l.ldwh * 2, 4096), CSI_LAYER_BUF(Wh_p, (size_t)256 * l.ldwh * 2, 4096),
    CSI_LAYER_BUF(bias, (size_t)l.out * 4, UPLOAD_SLACK),         CSI_LAYER_BUF(bias_hs, (size_t)l.out * 4, UPLOAD_SLACK),
    CSI_LAYER_BUF(scale, (size_t)l.out * 4, UPLOAD_SLACK),        CSI_LAYER_BUF(shift, (size_t)l.out * 4, UPLOAD_SLACK)};
#define CSI_H1(m) ((m).layers.empty() ? (size_t)0 : (size_t)(m).layers[0].out)
const ModelBuf kModelBufs[MODEL_BUFS] = {CSI_MODEL_BUF(W0p, (size_t)nt * CSI_H1(m) * 4), CSI_MODEL_BUF(W0rm, (size_t)l0_k * CSI_H1(m) * 4),
                                         CSI_MODEL_BUF(conv, (size_t)CONV_PRM_FLOATS * 4)};

struct GraphEntry {           // one captured csi_predict_device / csi_estimate_device call
    const void* in_re; const void* in_im; void* out_re; void* out_im;
    void* h_re; void* h_im;   // LS outputs (csi_estimate_device), null for csi_predict_device
    int64_t npkt;
    int seen;                 // eager runs with this key so far (capture happens on the 2nd call)
    hipGraphExec_t exec;
    int64_t hs_launches = 0;  // split-engine GEMMs inside the graph (a replay owes them to the range-guard bookkeeping)
};

struct ProfSpan {
    int id;
    hipEvent_t beg, end;
};

}  // namespace

struct csi_trainer;          // csi_train.hpp
struct csi_hostpipe;         // csi_hostpipe.hpp
struct csi_comm;             // csi_comm.hpp

// The forms of the fused band kernel (gemm_hs_band.hip.h) a context can launch, per arithmetic mode: the 8-wave kernel of band_kernel_gen.py with the
// L0 / T streams staged through LDS, with per-lane global loads of them (nt outside the staged range), in its column-split launch (grid (bands, splits),
// split y computes N1 / splits of the hidden features), and the register-blocked kernel of band4_kernel_gen.py (staged only) unsplit / column-split.
enum BandForm { BAND_EIGHT, BAND_EIGHT_NOSTAGE, BAND_EIGHT_CS, BAND_FOUR, BAND_FOUR_CS, BAND_FORMS };
struct BandKernel {
    hipFunction_t fn;         // null: the code object does not hold this form
    unsigned threads;         // its workgroup size
};

struct csi_ctx {
    csi_config cfg;
    int d_in = 0;                // layer-0 input width: l0_k + nt
    int input_pool = 0;          // csi_set_input_pool: POOL_NONE / POOL_MAX / POOL_AVG (input_pool.hip.h)
    int l0_k = 0;                // LTF inputs of layer 0: len_ltf, len_ltf / 2 with pooling, 64 len_ltf for CONV1D (the preamble row stride stays len_ltf)
    int model_type = 0;          // csi_set_model_type: CSI_MODEL_FC / CSI_MODEL_CONV1D
    hipStream_t stream = nullptr;
    std::string err;
    Model model[2];
    csi_trainer* trainer[2] = {nullptr, nullptr};   // on-box fine-tuning state per component model
    int train_rank = 0;                             // "train_rank": rank of this process in a data-parallel fit; keys the trainers' noise / dropout streams (csi_train.hpp tr_stream)
    csi_hostpipe* hostpipe = nullptr;               // streams / pinned slots / host threads of the host-buffer entry points
    csi_comm* comm = nullptr;                       // RCCL communicator of csi_comm_init (weight broadcast)
    int host_threads = 0;                           // "host_threads" option: threads of the user <-> pinned copies (0 = automatic)
    int hp_side_threads = 1;                        // "hp_side_threads": 1 = input staging and result staging on their own threads beside the caller's enqueue loop, 0 = inline, in turn
    int hp_chunk_packets = 0;                       // "hp_chunk_packets": packets per pipeline slot of the host-buffer entry points (0 = automatic)
    int hp_device_weave = 1;                        // "hp_device_weave": csi_estimate_c128 with PINNED result arrays assembles the complex64 values on the device and downloads into the arrays themselves (0 = host threads weave, as for pageable arrays)
    int64_t hp_direct_out_calls = 0;                // "hp_direct_out_calls": calls that took that path
    float* P = nullptr;          // device [nt][nt]
    float* Pbf = nullptr;        // device: bf16 pieces of P in MFMA operand order (ls_pilot layout of ls_estimate_ringb_kernel), 2 per float
    float* Ppad = nullptr;       // device [ceil32(nt)][ceil32(nt)], zero padded (chunked LS kernel)
    bool pilot_ok = false;
    // LS constants
    float* tw = nullptr;         // [2][256]
    int* bin_pos = nullptr;      // [234]
    float* denom = nullptr;      // [234]
    // csi_synth_structured (synth_structured.hip.h)
    float* ltf_nat = nullptr;    // [256] LTF sequence in FFT bin order, 0 on the null bins
    char* synth_ws = nullptr;    // [64] tap profile | [npkt] 0.5 * 10^(-snr/10) | [npkt * nr] item powers
    size_t synth_ws_bytes = 0;
    std::vector<float> synth_host;   // host image of the first two parts (stays alive behind the asynchronous upload)
    size_t synth_lds_attr = 0;   // dynamic-LDS limit already raised for its kernels
    size_t scatter_lds_attr = 0; // the same for the kernels of csi_synth_scattering (csi_scatter.hpp), which shares synth_ws / synth_host
    int64_t scatter_launches = 0;   // "scatter_launches": kernels launched by csi_synth_scattering
    size_t scatter_aged_lds_attr = 0;      // csi_scatter_channel_at_device (csi_scatter_aged.hpp): dynamic-LDS limit already raised for its kernel
    int64_t scatter_aged_launches = 0;     // "scatter_aged_launches": kernels launched by csi_scatter_channel_at_device
    char* forecast_ws = nullptr;           // channel forecast (csi_forecast.hpp): T and, when the caller keeps none, c of a csi_forecast_device call (sized by eager calls)
    size_t forecast_ws_bytes = 0;
    char* cfo_ws = nullptr;                // carrier frequency offset (csi_cfo.hpp): eps of a csi_cfo_correct_device call whose caller keeps none (sized by eager calls)
    size_t cfo_ws_bytes = 0;
    int64_t cfo_launches = 0;              // "cfo_launches": kernels launched by the csi_cfo_* entry points
    char* sync_ws = nullptr;               // symbol timing (csi_sync.hpp): eps and theta of a csi_sync_correct_device call whose caller keeps none (sized by eager calls)
    size_t sync_ws_bytes = 0;
    int64_t sync_launches = 0;             // "sync_launches": kernels launched by the csi_sync_* entry points
    int64_t forecast_launches = 0;         // "forecast_launches": kernels launched by the csi_forecast_* entry points and csi_sounding_noise_device
    // activation workspace
    char* ws = nullptr;
    size_t ws_bytes = 0;
    // layer-0 slabs + sum of the one-packet (skinny) path
    char* l0skinny = nullptr;
    size_t l0skinny_bytes = 0;
    // split-K slabs of the small-batch path
    char* skbuf = nullptr;
    size_t skbuf_bytes = 0;
    // second stream + scratch set so that the real and the imag model of a SMALL call run side by side
    // (a one-packet call is launch-latency bound: 12 short kernels in a row; see csi_predict_device)
    hipStream_t aux_stream = nullptr;
    hipEvent_t aux_fork = nullptr, aux_join = nullptr;
    char *aux_ws = nullptr, *aux_l0skinny = nullptr, *aux_skbuf = nullptr, *aux_fuse_ws = nullptr;
    size_t aux_ws_bytes = 0, aux_l0skinny_bytes = 0, aux_skbuf_bytes = 0, aux_fuse_ws_bytes = 0;
    int small_call_overlap = 1;  // "small_call_overlap" option
    // the one-packet regime (csi_dnn_small.hpp): both models of a call of <= 8 rx preambles in 1 + n_hidden launches
    int small_ls_fused = 1;      // "small_ls_fused": a one-packet csi_estimate_device call runs its LS estimate inside the layer-0 launch (small_l0_ls_kernel)
    float* small_ls_h_re = nullptr;   // set by csi_estimate_device around its predict call, consumed by predict_small
    float* small_ls_h_im = nullptr;
    int64_t small_ls_launches = 0;
    // hybrid beamforming weights (csi_hybrid.hpp): the dictionary [nt][hyb_rp] (rays padded to 32 with zero columns) and the per-item workspace
    float* hyb_at_re = nullptr;
    float* hyb_at_im = nullptr;
    int hyb_rays = 0, hyb_rp = 0;
    char* hyb_ws = nullptr;
    size_t hyb_ws_bytes = 0;
    char* link_ws = nullptr;     // link simulation (csi_link.hpp): coded bits and, when the caller keeps none, the soft bits of a packet chunk
    size_t link_ws_bytes = 0;
    // blind LMMSE smoother (csi_lmmse_blind[_device]): fp64-pair twiddles exp(-2 pi i u / 256), the statistics of a call the caller keeps
    // none of ([nblk] nv | [nblk][234] c | [nblk] fallback flags; sized by eager calls) and the device word behind "lmmse_blind_fallbacks"
    LmbTwiddle* lmb_tw = nullptr;
    char* lmb_ws = nullptr;
    size_t lmb_ws_bytes = 0;
    long long* lmb_count = nullptr;
    // delay-subspace smoother (csi_subspace.hpp): the basis as the kernel's two images, qa re | qa im [234][rp] then qb re | qb im [rp][256],
    // in one allocation of the largest size (rank 128) that a second csi_subspace_set_basis overwrites; rank 0 = none set
    float* sub_q = nullptr;
    int sub_rank = 0, sub_rp = 0;
    size_t sub_lds_attr = 0;
    int64_t subspace_launches = 0;   // "subspace_launches": kernels launched by csi_subspace_smooth_device
    // beam-space smoother (csi_beam.hpp): the basis as the kernels' two images, a1 re | a1 im [ntp][nbp] then a2 re | a2 im [nbp][ntp], in one
    // allocation of the largest size (128 x 128) that a second csi_beam_set_basis overwrites; nb 0 = none set.  beam_ws: E and, when the
    // caller keeps none, w of a csi_beam_wiener_device call ([npkt][nr][nb] each; sized by eager calls)
    float* beam_a = nullptr;
    int beam_nb = 0, beam_ntp = 0, beam_nbp = 0;
    char* beam_ws = nullptr;
    size_t beam_ws_bytes = 0;
    int64_t beam_launches = 0;   // "beam_launches": kernels launched by the csi_beam_* entry points
    int64_t mu_launches = 0;     // "mu_launches": kernels launched by csi_mu_precoder_device / csi_mu_link_sim_device / csi_mu_hybrid_precoder_device / csi_mu_covariance_device / csi_mu_jsdm_precoder_device
    char* muh_ws = nullptr;      // multi-user hybrid precoder (csi_mu_hybrid.hpp): the score planes of a packet chunk when the caller keeps none (sized by eager calls)
    size_t muh_ws_bytes = 0;
    size_t muh_lds_attr[3] = {}; // dynamic-LDS limit already raised for its score kernel / baseband kernel of 64 lanes / of 32 lanes
    char* muj_ws = nullptr;      // multi-user JSDM precoder (csi_mu_jsdm.hpp): covariance, eigenvalue, U*, rank and Frf planes of a packet chunk (sized by eager calls)
    size_t muj_ws_bytes = 0;
    size_t muj_lds_attr[3] = {}; // dynamic-LDS limit already raised for its eigen kernel / baseband kernel of 64 lanes / of 32 lanes
    char* fb_ws = nullptr;       // quantised CSI feedback (csi_feedback.hpp): the singular vectors of a packet chunk (sized by eager calls)
    size_t fb_ws_bytes = 0;
    float* fb_tab = nullptr;     // ... and the cos / sin tables of the bin centres of (fb_tab_bphi, fb_tab_bpsi)
    int fb_tab_bphi = 0, fb_tab_bpsi = 0;
    size_t fb_lds_attr[2] = {};  // dynamic-LDS limit already raised for its compress / expand kernel
    int64_t feedback_launches = 0;   // "feedback_launches": kernels launched by csi_feedback_compress_device / csi_feedback_expand_device
    size_t rxc_lds_attr = 0;     // receive combining (csi_rx_combine.hpp): dynamic-LDS limit already raised for its combiner kernel
    int64_t combine_launches = 0;    // "combine_launches": kernels launched by csi_rx_combiner_device / csi_rx_apply_combiner_device
    int64_t link_launches = 0;   // "link_launches": kernels launched by csi_link_sim_device / csi_viterbi_decode_device
    bool user_capture = false;   // between csi_capture_begin and csi_capture_end (csi_hybrid.hpp): device-pointer calls are recorded, not run
    bool user_capture_use_graph = false;
    int64_t user_capture_hs0 = 0;
    uint64_t graph_epoch = 0;    // bumped by drop_graphs: graphs a caller captured before are stale
    int64_t hybrid_launches = 0; // "hybrid_launches": kernels launched by csi_hybrid_weights[_device]
    int64_t conv_launches = 0;   // "conv_launches": CONV1D front-end passes launched (conv_frontend.hip.h)
    int debug_small_tile16 = 0;  // CSI_DEBUG_HOOKS=1 CSI_SMALL_TILE16=1, read once at csi_create (A/B runs)
    int small_fused = 1;         // "small_fused" option: 0 = the general kernels (six launches per model on two streams)
    int small_rows = 1024;       // "small_rows": pair rows up to which a call takes it (and at most 64 preambles).  Measured (profiles/r05_regime_probe.txt):
                                 // 4 packets 117 us against 143 on the general kernels, 8 packets 162 / 170, 12 packets 251 / 246, 16 packets 283 / 252
    int l0_stream = 1;           // "l0_stream": layer 0 of a call of 9 ... 256 rx preambles on the weight-streaming split-f16 kernel (l0_hs_stream.hip.h)
    int l0_stream_ks = 0;        // "l0_stream_ks": its k ranges (0 = automatic: ~256 workgroups per component model up to 64 preambles, ~128 beyond)
    int64_t l0_stream_launches = 0;
    int l0_stream_max_rows = 1280;     // "l0_stream_max_rows": the largest call (rx preambles) the kernel takes (<= 4096), beyond 256 in row blocks (gridDim.z).
                                       // Measured (profiles/r05_band_split_probe.txt): 128 packets 400 -> 323 us, 256: 693 -> 595, 320: 862 -> 790; 500 packets 1108 -> 1134 (not taken)
    int l0_stream_prepass_rows = 64;   // "l0_stream_prepass_rows": beyond this many preambles the row scales come from l0_row_max_kernel
    int small_rows_band = 256;   // "small_rows_band": the same limit where the column-split band kernel serves the model (csi_band.hpp): the general
                                 // path with it and the weight-streaming layer 0 takes 102 us at 3 ... 5 packets against 117-121 here (2 packets: 111 / 61)
    bool in_host_pipeline = false;   // a chunk of a host-buffer entry point is being enqueued: no second-stream fork inside (measured: the
                                 // two-stream arrangement costs the PCIe-bound pipeline 6 % - profiles/r05_regime_probe.txt)
    int64_t small_calls = 0;     // "small_calls": calls that took it
    char* small_ws = nullptr;    // its scratch: L0 of both models + ping-pong activations
    size_t small_ws_bytes = 0;
    // staging for host-buffer entry points
    char* stage = nullptr;
    size_t stage_bytes = 0;
    int xcd_order = -1;          // option "xcd_order": -1 auto, 0 linear tile order, 1 XCD super-tile order
    bool use_graph = false;
    bool in_graph_call = false;  // csi_estimate_device is running the content of a (future) graph: no second-stream fork inside
    int64_t graph_replays = 0;   // hipGraphLaunch count ("graph_replays", read-only)
    std::vector<GraphEntry> graphs;
    int f32_engine = -1;         // "f32_engine" option: fp32 contexts, 0 = native fp32 MFMA kernels, 1 = split-f16 kernels (gemm_hs.hip.h)
                                 // wherever the shapes allow, -1 = split-f16 once a GEMM fills the chip (default)
    int hs_act_shift = HS_SHIFT_AUTO;        // split-f16: hidden activations are carried times 2^hs_act_shift (|h| < 65504 / 2^shift)
    float* hs_zero = nullptr;    // zeros, widest hidden layer: the BN shift the split-engine kernels see (it lives in the next layer's bias)
    unsigned* hs_peak = nullptr; // device word: range guard of the split engine (gemm_hs.hip.h), 0 = no operand came near the f16 limit
    size_t hs_lds_attr[21] = {};   // dynamic-LDS limit already raised on this context's device: layer 0 / pair (hs out) / pair (fp32 out) / pair + fused regressor
    int64_t hs_launches = 0;     // split-engine GEMMs launched so far / at the last range check
    int64_t hs_checked = 0;
    int64_t hs_range_fallbacks = 0;
    int64_t hs_weight_pins = 0;  // models csi_load_weights pinned to the fp32 MFMA kernels: their split-f16 weight copies were not fp32-grade (read-only option)
    int hs_blocked = 1;          // "hs_blocked": hs activation buffers between split-engine layers in the blocked layout (gemm_hs.hip.h)
    int hs_fuse_regressor = 0;   // "hs_fuse_regressor": two hidden layers -> the regressor runs inside the pair kernel (h2 stays on the CU).
                                 // Off by default: measured SLOWER (2.45 vs 1.88 ms per 262144 rows, profiles/r02_hs_probe.txt) - the
                                 // partial sums the four column tiles exchange cost what the h2 round trip cost
    char* fuse_ws = nullptr;     // its partial-sum slabs + row-tile flags
    size_t fuse_ws_bytes = 0;
    int hs_band = 1;             // "hs_band": two hidden layers -> first per-pair layer + regressor as ONE kernel, the assembly "band8"
                                 // kernel of band_kernel_gen.py (h2 stays in registers; measured -4 .. -7 % against the two kernels,
                                 // profiles/r03_band_probe.txt); 0 = the separate pair and regressor kernels
    hipModule_t band_mod = nullptr;          // its code object (embedded in the library, loaded on first use)
    BandKernel band_kernel[2][BAND_FORMS] = {};   // its kernels by [bf16 context][form] (csi_band.hpp: band_load fills the table, band_plan chooses from it)
    int n_cu = 256;                          // compute units of the device (csi_create)
    int band4 = 1;                           // "band4": staged shapes with at most 2 column splits take the register-blocked forms csi_band4* (band4_kernel_gen.py:
                                             // 4 waves x 512 registers) in fp32 and bf16 contexts alike; 0 = the 8-wave forms csi_band8* everywhere (A/B)
    bool band_failed = false;                // the code object could not be loaded: separate kernels from then on
    int64_t band_launches = 0;
    int64_t band4_launches = 0;              // "band4_launches" (read-only): those of band_launches that launched a register-blocked csi_band4* function
    int band_split = -1;         // "band_split": calls with fewer bands than CUs split every band's hidden features over 2 / 4 workgroups (the
                                 // regressor sums of the splits are added in split order by band_split_sum_kernel); -1 = automatic (as many
                                 // splits as keep the workgroups of the models in flight within the 256 CUs), 0 / 1 = never, 2 / 4 = always
    int64_t band_split_launches = 0;
    int aux_fork_early = 1;      // "aux_fork_early": csi_estimate_device forks the second stream of a two-stream call in front of its LS kernel
    bool aux_preforked = false;
    int models_in_flight = 1;    // 2 while csi_predict_device runs the component models on two streams
    int hs_min_blocks = 48;      // automatic mode: the per-pair layers go to the split engine from this many 256x256 workgroups on
                                 // ("hs_min_blocks"; measured crossover at Nt=32, 1024x1024 with the two component models on two
                                 // streams: 24 packets - profiles/r05_regime_probe.txt; 80 = 40 packets before round 5); layer 0 from max(this, 128)
    int hs_in_shift = HS_SHIFT_AUTO;         // split-f16: the preamble samples times 2^hs_in_shift
    long long bf16_l0_fused_split_launches = 0;   // layer-0 products that took the fused kernel with K ranges because of "bf16_l0_fused_split" (get only)
    int band_tail_split = 1;     // "band_tail_split": a call of more bands than CUs whose last round of band workgroups would leave >= half of the CUs idle launches
                                 // that round in 2 or 4 column splits (one-stream calls; round 6); 0 = one launch
    long long band_tail_launches = 0;
    int bf16_l0_fused_split = 1; // "bf16_l0_fused_split": bf16 layer 0 of calls between the streaming kernel's range and 256 tiles on the fused kernel with K ranges (round 6); 0 = cast pass + 128 x 128 kernel
    int bf16_fused_h1 = 1;       // "bf16_fused_h1" option: 0 = materialise h1 (pair_h1_bf16_kernel) instead of generating it in the GEMM
    int p_pieces = 3;            // bf16 pieces (8 significand bits each) the entries of P need: 1 for +-1 pilots, 3 for arbitrary floats
    int ls_ringb_min = 33;       // "ls_ringb_min": from this Nt on a non-Hadamard pilot takes the bf16-split despread (ls_estimate_ringb_kernel).
                                 // Round 4: 33, not 16 - the one-antenna-tile form of that kernel (Nt <= 32, TWO workgroups per CU) produced, on
                                 // ONE box of the pool, 1-3 wrong items in ~1 % of the first launches of a fresh context (always the first item of
                                 // a CU's second workgroup, lane groups of an FFT stage; 7 events in 570 cycles there, none in 1170 on two other
                                 // boxes, none ever in the other LS kernels).  Not understood, so not selected: Nt <= 32 takes
                                 // the fp32 ring kernel (3-5 % slower); "ls_kernel" 7 still forces it (one workgroup per CU since round 5; cause found
                                 // in round 6)
    bool p_sylvester = false;    // csi_set_pilot saw the Sylvester Hadamard matrix (Walsh-Hadamard LS despread applies)
    // csi_set_pilot saw P = D1 Pi1 H Pi2 D2 (H Sylvester, Pi permutations, D signs; e.g. the 802.11 VHT 4x4 base doubled up): the
    // Walsh-Hadamard kernel applies with permuted / signed symbol loads and output rows.  p_perm[0][u] = source symbol of transform
    // input u (| 256 when it enters negated), p_perm[1][r] = output antenna of transform row r (| 256 when negated)
    bool p_fast_ok = false;
    bool p_fast_identity = true; // ... and both are the identity without signs (the Sylvester matrix itself): the kernel without tables
    int p_perm[2][CSI_WIRE_MAX_NT] = {};
    int* p_tables = nullptr;     // device: [4][nt] source symbol, its sign (float bits), output row, its sign
    int ls_fast_perm = 1;        // "ls_fast_perm": 0 = only the exact Sylvester matrix takes the Walsh-Hadamard kernel (A/B runs)
    int ls_debug = 0;            // CSI_LS_DEBUG / "ls_debug": skip phases of the chunked LS kernel (timing experiments only)
    int ls_kernel = 0;           // "ls_kernel" option / CSI_LS_KERNEL: 0 auto, 1 FFT-first, 2 chunked, 3 despread-first, 4 / 5 Walsh-Hadamard (register prefetch / LDS-DMA ring), 6 generic P on the ring (fp32 despread), 7 generic P, bf16-split despread (tests, A/B runs)
    int hs_vm_cast = 2, hs_vm_pair = 3;   // "hs_vm_cast" / "hs_vm_pair": vector-memory schedule of the layer-0 / pair kernel (gemm_hs.hip.h): 0 builtin LDS-DMA + one drain per sub-tile, 1 hand-counted, 2 + one more sub-tile of look-ahead, 3 + one load and one 24-MFMA segment per sub-tile
    int hs_l0_mfma = 16;         // "hs_l0_mfma": MFMA shape of the split-f16 layer-0 kernel's main loop (gemm_hs.hip.h): 32 = v_mfma_f32_32x32x16_f16, 16 (default: -8.7 % on the kernel, profiles/l0_mfma16_ab.txt) = the 16x16x32 form
                                 // on pairs of sub-tiles (taken with "hs_vm_cast" = 2 when every k range holds an even number of sub-tiles)
    int64_t hs_l0_mfma16_launches = 0;
    int ls_v2 = 0;               // CSI_LS_V2: shape variant of the LDS-DMA fed Walsh-Hadamard kernel (experiments)
    int ls_fft_first_max = 15;   // FFT-first LS kernel (all Nt spectra in LDS) up to this Nt; from 16 on the ring kernel is faster (Nt = 16: 0.47 vs 0.72 ms); debug knob CSI_LS_FFT_FIRST_MAX
    int force_pair_tile = 0;     // debug knob CSI_FORCE_PAIR_TILE=128|256: forces the row-tile height of every GEMM (tests)
    // profiling
    bool prof_on = false;
    std::vector<ProfSpan> spans;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[K_COUNT] = {0};
    int64_t prof_launches[K_COUNT] = {0};
    double prof_flops[K_COUNT] = {0};
    double prof_bytes[K_COUNT] = {0};
};

namespace {

int fail(csi_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_create_error = buf;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(ctx, CSI_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                    \
    } while (0)

struct ProfScope {
    csi_ctx* c;
    bool on;
    ProfSpan sp;
    ProfScope(csi_ctx* ctx, int id, double flops, double bytes) : c(ctx), on(ctx->prof_on) {
        if (!on) return;
        sp.id = id;
        sp.beg = take();
        sp.end = take();
        c->prof_launches[id] += 1;
        c->prof_flops[id] += flops;
        c->prof_bytes[id] += bytes;
        hipEventRecord(sp.beg, c->stream);
    }
    ~ProfScope() {
        if (!on) return;
        hipEventRecord(sp.end, c->stream);
        c->spans.push_back(sp);
    }
    hipEvent_t take() {
        if (!c->ev_pool.empty()) {
            hipEvent_t e = c->ev_pool.back();
            c->ev_pool.pop_back();
            return e;
        }
        hipEvent_t e;
        hipEventCreate(&e);
        return e;
    }
};

const char* input_pool_name(int mode) { return mode == POOL_MAX ? "max" : (mode == POOL_AVG ? "avg" : "none"); }

// pooled preambles of a decimated-input model: planes x[p] [rows][len_ltf] -> y[p] [rows][len_ltf / 2], fp32 or bf16 (input_pool.hip.h)
int launch_input_pool(csi_ctx* c, const float* x0, const float* x1, void* y0, void* y1, int64_t rows, bool to_bf16) {
    const int planes = x1 ? 2 : 1;
    PoolArgs a{};
    a.x[0] = x0; a.x[1] = x1 ? x1 : x0;
    a.y[0] = y0; a.y[1] = y1 ? y1 : y0;
    a.nq = (size_t)rows * (size_t)c->cfg.len_ltf / 8;
    // 8 workgroups of 256 lanes per CU (32 waves), 8 loads of 16 bytes in flight per lane: 256 KiB requested per CU at a time
    const size_t per_trip = (size_t)IPOOL_THREADS * IPOOL_UNR;
    const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((a.nq + per_trip - 1) / per_trip, (size_t)c->n_cu * 8 / planes));
    ProfScope ps(c, K_INPUT_POOL, 0.0, (double)planes * rows * c->cfg.len_ltf * (4.0 + (to_bf16 ? 1.0 : 2.0)));
    const bool mx = c->input_pool == POOL_MAX;
    if (to_bf16) {
        if (mx) hipLaunchKernelGGL(input_pool_bf16_kernel<POOL_MAX>, dim3(blocks, planes), dim3(IPOOL_THREADS), 0, c->stream, a);
        else hipLaunchKernelGGL(input_pool_bf16_kernel<POOL_AVG>, dim3(blocks, planes), dim3(IPOOL_THREADS), 0, c->stream, a);
    } else {
        if (mx) hipLaunchKernelGGL(input_pool_kernel<POOL_MAX>, dim3(blocks, planes), dim3(IPOOL_THREADS), 0, c->stream, a);
        else hipLaunchKernelGGL(input_pool_kernel<POOL_AVG>, dim3(blocks, planes), dim3(IPOOL_THREADS), 0, c->stream, a);
    }
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

// K ranges a CONV1D context's layer 0 may be cut into (K0 = 64 len_ltf: a chunk of ~800 preambles at nn0 = 256 has only a handful of
// output tiles; FC routes stop at 8 ... 40 ranges, tuned at K ~ 10k)
constexpr int L0_CONV_MAX_SPLITS = 256;

const char* model_type_name(int t) { return t == CSI_MODEL_CONV1D ? "CONV1D" : "FC"; }

// the layer-0 LTF width from BOTH context settings (csi_set_model_type, csi_set_input_pool - either may be called, with any value, after
// the other): 64 len_ltf features of the CONV1D front end, len_ltf / 2 pooled samples, or the len_ltf samples themselves
void set_layer0_width(csi_ctx* c) {
    const int L = c->cfg.len_ltf;
    c->l0_k = c->model_type == CSI_MODEL_CONV1D ? 64 * L : (c->input_pool != POOL_NONE ? L / 2 : L);
    c->d_in = c->l0_k + c->cfg.nt;
}

// layer 0 of this context reads a feature slab written by a pass in front of it (pooling or the CONV1D front end), not the preambles
bool l0_features(const csi_ctx* c) { return c->input_pool != POOL_NONE || c->model_type == CSI_MODEL_CONV1D; }

// CONV1D front end: planes x[p] [rows][ldx] raw preambles -> y[p] [rows][ldy] features (K0 = 64 len_ltf of them, then `tail` copied
// columns), fp32 or bf16; the constants of model md[p] (conv_frontend.hip.h)
int launch_conv_frontend(csi_ctx* c, const Model* md0, const Model* md1, const float* x0, const float* x1, void* y0, void* y1, int64_t rows,
                         int ldx, int ldy, int tail, bool to_bf16) {
    const int planes = x1 ? 2 : 1;
    ConvArgs a{};
    a.x[0] = x0; a.x[1] = x1 ? x1 : x0;
    a.y[0] = y0; a.y[1] = y1 ? y1 : y0;
    a.prm[0] = md0->conv; a.prm[1] = md1 ? md1->conv : md0->conv;
    a.rows = rows; a.L = c->cfg.len_ltf; a.ldx = ldx; a.ldy = ldy; a.tail = tail;
    if (!a.prm[0] || !a.prm[1]) return fail(c, CSI_ERR_NOT_READY, "CONV1D front end: the model holds no cnn1d_1 weights");
    if (c->model_type != CSI_MODEL_CONV1D || c->l0_k != 64 * c->cfg.len_ltf || (int64_t)ldy < (int64_t)c->l0_k + tail || ldx < c->cfg.len_ltf + tail)
        return fail(c, CSI_ERR_INVALID_ARG, "CONV1D front end: row pitches %d / %d do not hold %d samples / %d features + %d columns (context layer-0 width %d)",
                    ldx, ldy, c->cfg.len_ltf, 64 * c->cfg.len_ltf, tail, c->l0_k);
    const int64_t tiles = rows * ((c->cfg.len_ltf / 2 + CF_TILE - 1) / CF_TILE);
    // 8 workgroups of 256 lanes per CU (32 waves, 8 KB of tile per workgroup in flight as stores)
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, (int64_t)c->n_cu * 8 / planes));
    const double outs = (double)planes * rows * ((double)c->l0_k + tail);
    ProfScope ps(c, K_CONV_FRONTEND, outs * 20.0, (double)planes * rows * ldx * 4.0 + outs * (to_bf16 ? 2.0 : 4.0));
    // every lane stores 16 bytes: the callers' slabs start on 16-byte boundaries and ldy is K0 (a multiple of 64) or K0 + nt (nt % 4 == 0)
    if ((ldy % (to_bf16 ? 8 : 4)) != 0 || (reinterpret_cast<uintptr_t>(a.y[0]) & 15) != 0 || (reinterpret_cast<uintptr_t>(a.y[1]) & 15) != 0)
        return fail(c, CSI_ERR_INVALID_ARG, "CONV1D front end: feature rows of pitch %d at %p / %p are not 16-byte aligned", ldy, a.y[0], a.y[1]);
    const dim3 grid(blocks, planes);
    if (to_bf16) hipLaunchKernelGGL((conv_frontend_kernel<8, true>), grid, dim3(CF_THREADS), 0, c->stream, a);
    else hipLaunchKernelGGL((conv_frontend_kernel<4, false>), grid, dim3(CF_THREADS), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    ++c->conv_launches;
    return CSI_OK;
}

// the pass in front of layer 0 of a feature-slab context: pooling (planes 0 and 1 of one call share the pooling mode) or the CONV1D
// front end (md0 / md1: the models whose constants each plane takes).  rows of len_ltf raw samples -> rows of K0 features
int launch_l0_features(csi_ctx* c, const Model* md0, const Model* md1, const float* x0, const float* x1, void* y0, void* y1, int64_t rows, bool to_bf16) {
    if (c->model_type == CSI_MODEL_CONV1D)
        return launch_conv_frontend(c, md0, md1, x0, x1, y0, y1, rows, c->cfg.len_ltf, c->l0_k, 0, to_bf16);
    return launch_input_pool(c, x0, x1, y0, y1, rows, to_bf16);
}

int prof_collect(csi_ctx* c) {
    if (c->spans.empty()) return CSI_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (auto& sp : c->spans) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, sp.beg, sp.end) == hipSuccess) c->prof_ms[sp.id] += ms;
        c->ev_pool.push_back(sp.beg);
        c->ev_pool.push_back(sp.end);
    }
    c->spans.clear();
    return CSI_OK;
}

void drop_graphs(csi_ctx* c) {
    for (auto& g : c->graphs)
        if (g.exec) hipGraphExecDestroy(g.exec);
    c->graphs.clear();
    ++c->graph_epoch;
}

int ensure_bytes(csi_ctx* c, char** buf, size_t* have, size_t need) {
    if (*have >= need) return CSI_OK;
    drop_graphs(c);           // captured launches point into the old buffer
    if (*buf) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipFree(*buf));
        *buf = nullptr;
        *have = 0;
    }
    const size_t bytes = need + G_SLACK_FLOATS * sizeof(float);
    if (hipMalloc((void**)buf, bytes) != hipSuccess) {
        *buf = nullptr;
        return fail(c, CSI_ERR_NOMEM, "device allocation of %zu bytes failed", bytes);
    }
    HIP_TRY(c, hipMemsetAsync(*buf, 0, bytes, c->stream));     // never-written parts must be finite
    *have = need;
    return CSI_OK;
}

// Every device array a GEMM may read as its A side (or as a per-column vector) is followed by
// G_SLACK_FLOATS zeroed floats: the K tail of the last tile over-reads into finite memory.
int upload(csi_ctx* c, float** dst, const float* src, size_t n) {
    if (*dst) { hipFree(*dst); *dst = nullptr; }
    const size_t bytes = (n + G_SLACK_FLOATS) * sizeof(float);
    if (hipMalloc((void**)dst, bytes) != hipSuccess)
        return fail(c, CSI_ERR_NOMEM, "device allocation of %zu bytes failed", bytes);
    HIP_TRY(c, hipMemset(*dst, 0, bytes));
    HIP_TRY(c, hipMemcpy(*dst, src, n * sizeof(float), hipMemcpyHostToDevice));
    return CSI_OK;
}

void free_layer(Layer& l) {
    for (const LayerBuf& b : kLayerBufs)
        if (*b.slot(l)) hipFree(*b.slot(l));
    l = Layer();
}

void free_model(Model& m) {
    for (auto& l : m.layers) free_layer(l);
    m.layers.clear();
    for (const ModelBuf& b : kModelBufs)
        if (*b.slot(m)) { hipFree(*b.slot(m)); *b.slot(m) = nullptr; }
    for (void* p : {(void*)m.T, (void*)m.T_hs, (void*)m.T_sw, (void*)m.Wt1, (void*)m.Wt2, (void*)m.l0_rowmax})
        if (p) hipFree(p);
    m.Wt1 = m.Wt2 = nullptr;
    m.T = m.T_hs = m.T_sw = m.l0_rowmax = nullptr;
    m.T_hs_shift = HS_SHIFT_AUTO;
    m.loaded = m.table_ok = m.tiled_ok = m.T_sw_ok = false;
    m.hs_repr_err = 0.0;
    m.hs_repr_ok = true;
}

const csi_tensor* find_tensor(const csi_tensor* t, int n, const std::string& name) {
    for (int i = 0; i < n; ++i)
        if (t[i].name && name == t[i].name) return &t[i];
    return nullptr;
}

}  // namespace
