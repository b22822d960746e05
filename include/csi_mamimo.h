/* csi_mamimo.h - C-ABI of the MI355X (gfx950) massive-MIMO channel-estimation hot path.
 *
 * The reference (mauro-belgiovine/DL-channel-estimation-MaMIMO) has no FFI: the path sits
 * behind two Python call surfaces, which the entry points below replace one for one.
 * Citations are file:line in the reference repository.
 *
 *   reference interface                                             replaced by
 *   --------------------------------------------------------------  ---------------------------
 *   model construction, massiveMIMO_CSI_prediction_DNN.py:176-234   csi_create
 *   Model.load_weights(<d>_weights-improvement.hdf5)   DNN.py:334   csi_load_weights
 *   keras.models.load_model(<d>_keras_model)     inference.py:15-16  csi_load_weights
 *   dataset['P'] fed as seq_p     massiveMIMO_dataGenerator.py:311  csi_set_pilot
 *   Model.predict(generator) over packets, batch = nTX*nRX
 *        DNN.py:339-346 + sample assembly dataGenerator.py:299-316  csi_predict[_device]
 *   CSIPredictor.inference: X.real / X.imag -> predict x2 ->
 *        real + 1j*imag on complex128 batches    inference.py:24-32  csi_estimate_c128 (complex64 batches: csi_estimate_c64)
 *   Model.predict(x, batch_size=bs)              inference.py:29-30
 *        / DNN.py:434,470  (arbitrary rows [B, lenLTF+Nt])          csi_predict_samples
 *   ofdmdemod + helperMIMOChannelEstimate
 *        generate_maMIMO_LTF.m:336-342, helperMIMOChannelEstimate.m:24-36
 *                                                                   csi_ls_estimate[_device]
 *   LMMSE_ce per link   helperMIMOChannelEstimate.m:37-39, LMMSE_ce.m  csi_lmmse_estimate[_device]
 *   the same call site, helperMIMOChannelEstimate.m:37-39, for a receiver that has
 *        neither the impulse response nor the SNR                   csi_lmmse_blind[_device]
 *   (an addition, no reference counterpart: the delay-subspace
 *        smoother of an LS estimate, same place in the chain)       csi_subspace_set_basis, csi_subspace_smooth[_device]
 *   (an addition, no reference counterpart: the beam-space Wiener
 *        smoother of an LS estimate across the Tx antennas, same
 *        place in the chain, and the null-carrier noise level)       csi_beam_set_basis, csi_beam_power_device, csi_beam_smooth[_device], csi_beam_wiener[_device], csi_null_noise_device
 *   NMSE_subk           BER_test_maMIMO_LTF.m:675-686                csi_nmse[_device]
 *   known-channel sounding packets  generate_maMIMO_LTF.m:197-342   csi_synth_structured
 *   phased.ScatteringMIMOChannel    helperApplyMUChannel.m:44-143   csi_synth_scattering
 *   (an addition, no reference counterpart - the reference sets
 *        'MaximumDopplerShift',0: that channel at later times for
 *        a user that moves)                                          csi_scatter_channel_at_device
 *   (an addition: a linear predictor over several soundings of
 *        that channel, fitted on the soundings themselves)          csi_forecast[_device], csi_forecast_gram/fit/apply_device, csi_sounding_noise_device
 *   (an addition: the synchronisation stage in front of the
 *        estimators - carrier frequency offset of the preamble
 *        from its cyclic prefixes, and the rotation that removes it) csi_cfo_estimate_device, csi_cfo_rotate_device, csi_cfo_correct[_device]
 *   (an addition, the stage in front of that one: where the packet
 *        starts inside a capture, from the same cyclic prefixes,
 *        the cut-out that applies it and the embedding that tests it) csi_sync_embed_device, csi_sync_estimate_device, csi_sync_extract_device, csi_sync_correct[_device]
 *   omphybweights       BER_test_maMIMO_LTF.m:347-376                csi_hybrid_weights[_device]
 *   --execTime profiler loop                       DNN.py:441-475   csi_profile_*
 *   Model.fit step (noise, BN, dropout, Adam)       DNN.py:272-316   csi_train_*
 *
 * Conventions: every function returns 0 on success or a negative csi_status; it never calls
 * exit().  All buffers are caller-owned, row-major, contiguous float32.  A context is bound
 * to one GPU and one HIP stream and is not thread-safe; use one context per GPU.  Host-buffer
 * entry points are synchronous; internally they pipeline upload, kernels and download over packet
 * chunks (pinned staging slots, a few host threads) and DMA directly from / to buffers the caller
 * has pinned (hipHostMalloc / hipHostRegister).  *_device entry points take device pointers, enqueue on the
 * context's stream and return without waiting; call csi_synchronize before reading results.
 *
 * Device pointers (csi_predict_device, csi_ls_estimate_device, csi_estimate_device, csi_lmmse_estimate_device, csi_lmmse_blind_device, csi_subspace_smooth_device, csi_beam_power_device, csi_beam_smooth_device, csi_beam_wiener_device, csi_null_noise_device, csi_nmse_device,
 * csi_hybrid_weights_device, csi_link_sim_device, csi_link_sim_rx_device, csi_mu_precoder_device, csi_mu_link_sim_device, csi_mu_hybrid_precoder_device, csi_mu_covariance_device, csi_mu_jsdm_precoder_device, csi_feedback_compress_device, csi_feedback_expand_device, csi_rx_combiner_device, csi_rx_apply_combiner_device, csi_viterbi_decode_device, csi_synth_*, csi_scatter_channel_at_device, csi_forecast_*_device, csi_sounding_noise_device, csi_cfo_*_device, csi_sync_*_device).  An array of exactly the documented
 * size suffices: it may be a slice of a larger allocation whose neighbours hold live data of any value (NaN and 1e38 included).
 * Nothing outside the arrays is written, nothing outside them reaches a result, and input arrays are not modified.  Every re / im
 * PLANE (the preambles [npkt][Nr][len_ltf], the CSI planes [npkt][Nr][Nt][234 or n_out], fbb, frf_mean, xeq, gest, the precoder planes W, g) starts on a 16-byte
 * boundary: the LS and layer-0 kernels move the caller's rows as 16-byte words and by LDS-DMA; hipMalloc, csi_device_malloc and
 * whole torch tensors satisfy that, and so does every packet range of a preamble or CSI plane (Nt is a multiple of 4).  A
 * misaligned plane is refused with CSI_ERR_INVALID_ARG and a text that names the argument, before anything is launched or counted.
 * The remaining arrays - hvec, snr_db, the weights w of csi_subspace_smooth_device, power, w and err_var of the csi_beam_* entry points, noise_var, noise_std, tau, the per-packet and per-link results, idx, n_atoms, gain, csi,
 * llr, bits - and the four planes of csi_nmse_device ([nlinks][n_bins] for ANY n_bins) are read and written element by element and
 * need the alignment of their element type only.
 *
 * Sample / output order everywhere: s = p*Nr*Nt + iRx*Nt + iTx
 * (create_massiveMIMO_CSIest_dnn_dataset.py:62), i.e. outputs are [Npkt][Nr][Nt][n_out],
 * which is MATLAB CSI(:, iTx, iRx) of packet p (BER_test_maMIMO_LTF.m:191-195).
 */
#ifndef CSI_MAMIMO_H
#define CSI_MAMIMO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSI_MAX_HIDDEN 8
#define CSI_ABI_VERSION 1

typedef enum {
    CSI_OK = 0,
    CSI_ERR_INVALID_ARG = -1,   /* null pointer, bad shape, unsupported size              */
    CSI_ERR_NOT_READY = -2,     /* predict before weights / pilot were loaded             */
    CSI_ERR_HIP = -3,           /* a HIP runtime call failed; text in csi_last_error       */
    CSI_ERR_NO_DEVICE = -4,     /* no gfx950 device visible                                */
    CSI_ERR_NOMEM = -5,         /* device allocation failed                                */
    CSI_ERR_RANGE = -6          /* split-f16 engine: an operand left the f16 range (csi_synchronize) */
} csi_status;

typedef enum {
    CSI_DTYPE_F32 = 0,          /* fp32 in / accumulate / out.  GEMMs that fill the chip run on the split-f16 engine (every fp32
                                 * operand as hi + lo f16 halves, 3 x v_mfma_f32_32x32x16_f16 per product, fp32 accumulation; same
                                 * 1e-5 contract, both f16 range ends guarded with an automatic repeat); smaller calls and
                                 * "f32_engine" = 0 run v_mfma_f32_32x32x2_f32 (exact fp32 products)                    */
    CSI_DTYPE_BF16 = 1          /* bf16 operands, fp32 accumulate MFMA, fp32 out            */
} csi_dtype;

/* Model + problem shape.  n_out = 234 and hidden = {1024, 1024} in the shipped pipeline
 * (full_pipeline_maMIMO_DNNEst.sh:40,47). */
typedef struct {
    int32_t nt;                      /* tx antennas = LTF symbols = pilot-row length        */
    int32_t nr;                      /* rx antennas per packet                              */
    int32_t len_ltf;                 /* samples per rx preamble, 320*nt                     */
    int32_t n_hidden;                /* number of Dense+relu(+BN) layers, 1..CSI_MAX_HIDDEN */
    int32_t hidden[CSI_MAX_HIDDEN];  /* their widths (--nn)                                 */
    int32_t n_out;                   /* fc_regressor width (nSubCarr)                       */
    int32_t use_bn;                  /* --useBN                                             */
    float   bn_eps;                  /* keras BatchNormalization epsilon, 1e-3              */
    int32_t dtype;                   /* csi_dtype                                           */
    int32_t device;                  /* HIP device ordinal                                  */
    int64_t workspace_bytes;         /* cap for activation workspace; 0 = default (4 GiB fp32, 8 GiB bf16) */
} csi_config;

/* One named weight tensor on the host.  Names are the keras ones:
 *   fc_dense<i>.kernel [in,out]   fc_dense<i>.bias [out]
 *   bn<i>.gamma / .beta / .moving_mean / .moving_variance [out]      (iff use_bn)
 *   fc_regressor.kernel [in,n_out]   fc_regressor.bias [n_out]
 * Rows 0..len_ltf-1 of fc_dense0.kernel multiply the LTF samples, rows len_ltf..len_ltf+nt-1
 * the pilot row (Concatenate([flatten, seq_p]), DNN.py:207-208). */
typedef struct {
    const char*  name;
    const float* data;
    int64_t      rows;               /* 1 for vectors                                       */
    int64_t      cols;
} csi_tensor;

typedef struct csi_ctx csi_ctx;

int  csi_abi_version(void);
int  csi_create(const csi_config* cfg, csi_ctx** out);
void csi_destroy(csi_ctx* ctx);
const char* csi_last_error(const csi_ctx* ctx);      /* ctx may be NULL: last create error  */

/* Decimated-input models (--decimate_max / --decimate_avg, massiveMIMO_CSI_prediction_DNN.py:30-31,197-205): the LTF passes a
 * MaxPooling1D() (mode 1) or AveragePooling1D() (mode 2) - pool 2, stride 2, 'valid' - before Flatten + Concatenate, so layer 0 sees
 * len_ltf/2 + nt inputs: fc_dense0.kernel has len_ltf/2 + nt rows.  0 = none (default).  Every entry point still takes the raw
 * [..][len_ltf] preambles / [B][len_ltf+nt] rows and pools inside; LS, LMMSE and NMSE read the raw preambles.  Only for nt > 0,
 * and only while neither component model holds weights and no trainer exists (CSI_ERR_INVALID_ARG with text otherwise).
 * csi_get_option("input_pool") reads the mode; csi_clone_weights / csi_broadcast_weights refuse contexts of different modes. */
int  csi_set_input_pool(csi_ctx* ctx, int mode);

/* CONV1D models (--model CONV1D, massiveMIMO_CSI_prediction_DNN.py:236-270): type 1 puts a front end in front of layer 0.  The
 * LTF row x[len_ltf] goes through Conv1D(128, 7, padding='same') + bias, relu, its BatchNormalization (always present, moving
 * statistics, eps = csi_config.bn_eps), AveragePooling1D() (pool 2, stride 2) and Flatten (channels last), so layer 0 sees
 * K0 = 64 len_ltf features + nt pilot inputs: fc_dense0.kernel has 64 len_ltf + nt rows.  0 = FC (default).  Extra tensors of
 * csi_load_weights: "cnn1d_1.kernel" [7 taps][128 filters], "cnn1d_1.bias" [128], "conv_bn.gamma" / ".beta" / ".moving_mean" /
 * ".moving_variance" [128].  Callers still pass raw preambles / [B][len_ltf+nt] rows; LS, LMMSE and NMSE read the raw preambles.
 * Preconditions and errors as csi_set_input_pool (nt > 0, no weights, no trainer); CONV1D and input pooling exclude each other,
 * len_ltf must be even and at most 20480 (nt <= 64 at 320 samples per antenna: the 32-bit byte offsets of the buffer loads in the
 * layer-0 GEMMs), and 64 len_ltf x hidden[0] must stay below 2^31 elements (csi_load_weights refuses it).  csi_train_begin refuses
 * CONV1D contexts.  csi_get_option("model_type") reads the type, "conv_launches" counts front-end passes; clone / broadcast refuse
 * contexts of different types.
 * Routes (the front end writes the features into the per-chunk workspace; the layer-0 kernels read them with lda = K0):
 *   fp32, <= 8 rx preambles (one-packet path):  1 front-end launch for both models + the weight-streaming gemv + n_hidden launches;
 *                                               the LS estimate of csi_estimate_device does NOT ride in the layer-0 launch
 *   fp32, larger calls, per model and chunk:   1 front-end launch + layer 0 (weight-streaming split-f16 kernel, split-f16 GEMM or
 *                                               fp32 MFMA GEMM, K cut in up to 256 ranges) + its k-range sum + the FC stack as today
 *   bf16, per model and chunk:                 1 front-end launch (bf16 features) + the bf16 MFMA GEMM (K cut in up to 256 ranges) +
 *                                               the FC stack as today (no weight-streaming or fused-cast layer 0) */
#define CSI_MODEL_FC 0
#define CSI_MODEL_CONV1D 1
int  csi_set_model_type(csi_ctx* ctx, int type);

/* model: 0 = real, 1 = imag.  Tensors are copied (and re-laid-out) to the device. */
int  csi_load_weights(csi_ctx* ctx, int model, const csi_tensor* tensors, int n);
/* P [nt][nt], row j = pilot sequence of tx antenna j = MATLAB P(j,:) = dataset['P'][:, j]. */
int  csi_set_pilot(csi_ctx* ctx, const float* P);

/* Which LS despread csi_set_pilot will choose for P (host only; no context or device needed).  Returns 0: generic real P
 * (matrix-core despread), 1: the Sylvester Hadamard matrix, 2: a signed row / column permutation of it - e.g. the 802.11 VHT
 * 4x4 mapping matrix doubled up, what helperGetP (helperMIMOChannelEstimate.m:13, un-vendored toolbox code) yields - both served
 * by the Walsh-Hadamard kernel; negative csi_status on a bad argument.  For 1 / 2 the optional tables receive the decomposition
 * P[j][s] = rs[j] H[sigma(j)][tau(s)] cs[s]:  sym_src[u] = tau^-1(u) | (cs < 0 ? 256 : 0),  out_row[r] = sigma^-1(r) | (rs < 0 ? 256 : 0)
 * (nt entries each, nt <= 128). */
int  csi_pilot_classify(const float* P, int nt, int32_t* sym_src, int32_t* out_row);

/* CRC-32C (Castagnoli) of a host buffer - the per-tensor checksum of the SavedModel variable files the reference writes
 * (DNN.py:411) and keras_files.py verifies; host only (SSE4.2 when the CPU has it).  crc = 0 starts, a returned value continues. */
uint32_t csi_crc32c(const void* data, int64_t bytes, uint32_t crc);

/* DNN estimate of npkt packets.  ltf_re / ltf_im [npkt][nr][len_ltf]; out_re / out_im
 * [npkt][nr][nt][n_out].  Layer 0 is evaluated once per (packet, rx) and shared by the nt
 * pairs (the reference stores each rx preamble once for the same reason, mk.py:50-63). */
int  csi_predict(csi_ctx* ctx, const float* ltf_re, const float* ltf_im, int64_t npkt,
                 float* out_re, float* out_im);
int  csi_predict_device(csi_ctx* ctx, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt,
                        float* d_out_re, float* d_out_im);

/* Literal Model.predict: x [B][len_ltf+nt] -> y [B][n_out] through the un-shared network. */
int  csi_predict_samples(csi_ctx* ctx, int model, const float* x, int64_t B, float* y);

/* LS estimate: h_re / h_im [npkt][nr][nt][234]. */
int  csi_ls_estimate(csi_ctx* ctx, const float* ltf_re, const float* ltf_im, int64_t npkt,
                     float* h_re, float* h_im);
int  csi_ls_estimate_device(csi_ctx* ctx, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt,
                            float* d_h_re, float* d_h_im);
/* LS + DNN of device-resident packets as ONE unit (the per-packet work of generate_maMIMO_LTF.m:336-342 plus
 * DNN.py:346): with "use_graph" the whole launch sequence - LS kernel, range-guard memsets, magnitude sample,
 * layer 0, per-pair layers, regressor, both component models, every packet chunk - is captured into one hipGraph
 * on the 2nd identical call and replayed afterwards. */
int  csi_estimate_device(csi_ctx* ctx, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt,
                         float* d_out_re, float* d_out_im, float* d_h_re, float* d_h_im);

/* Both estimators on the arrays the reference's deployment wrapper handles (inference.py:24-32: a numpy
 * complex128 batch in, ``output_real + 1j*output_imag`` = complex64 out): ltf_c128 [npkt][nr][len_ltf] as
 * interleaved (re, im) doubles; dnn_c64 [npkt][nr][nt][n_out] and ls_c64 [npkt][nr][nt][234] as interleaved
 * (re, im) floats, either may be NULL.  One upload of the preambles serves both; the complex128 -> 2 x float32
 * split and the complex64 interleave run in the staging copies of the host pipeline, chunk by chunk beside the
 * transfers and kernels, instead of as whole-array passes in the caller (X.real / X.imag, inference.py:29-31).
 * Result arrays in pinned host memory (csi_host_malloc) skip the result-side host pass: the complex64 values are
 * assembled on the device and downloaded into the arrays themselves (option "hp_device_weave", default 1; counter
 * "hp_direct_out_calls"); same bits either way. */
int  csi_estimate_c128(csi_ctx* ctx, const double* ltf_c128, int64_t npkt, float* dnn_c64, float* ls_c64);

/* The same call for a batch the caller already holds as complex64 (an addition: inference.py:39-43 insists on complex128, and
 * CSIPredictor.inference keeps that contract; a pipeline that produces its preambles in single precision need not widen them
 * first).  ltf_c64 [npkt][nr][len_ltf] as interleaved (re, im) floats; results as csi_estimate_c128.  Half the bytes to read on
 * the host and no conversion pass there: the interleaved chunk is uploaded as it is - straight from the caller's array when
 * that is pinned host memory (csi_host_malloc) - and split into the two float32 planes on the device (csrc/weave.hip.h).
 * Bit-identical with csi_estimate_c128 on a batch whose values are representable in single precision. */
int  csi_estimate_c64(csi_ctx* ctx, const float* ltf_c64, int64_t npkt, float* dnn_c64, float* ls_c64);

/* LMMSE smoothing of an LS estimate (the 'hDmmse' output of helperMIMOChannelEstimate.m:37-39,
 * LMMSE_ce.m:23-39 with Nfft = Np = 234, Nps = 1).  h_re / h_im: LS estimate [npkt][nr][nt][234];
 * hvec [npkt][L]: the vector the reference passes as LMMSE_ce's 'h' (generate_maMIMO_LTF.m:342
 * hands it the scatterer delays h_tau); snr_db [npkt][nr]: SNR(i) in dB; out like h.
 * An all-zero hvec row is taken as zero delay spread (tau_rms = 0, the result for a one-tap row); the reference formula
 * divides 0 by 0 there (LMMSE_ce.m:28-29) and yields NaN. */
int  csi_lmmse_estimate(csi_ctx* ctx, const float* h_re, const float* h_im, int64_t npkt, const float* hvec, int L,
                        const float* snr_db, float* out_re, float* out_im);
int  csi_lmmse_estimate_device(csi_ctx* ctx, const float* d_h_re, const float* d_h_im, int64_t npkt, const float* d_hvec,
                               int L, const float* d_snr_db, float* d_out_re, float* d_out_im);

/* LMMSE smoothing from the packet's own statistics: the 'hDmmse' output of helperMIMOChannelEstimate.m:37-39 for a receiver that has
 * only the preamble and its LS estimate - no impulse response, no SNR (csrc/lmmse.hip.h).  Per (packet p, rx r), in
 * the contiguous-index convention of csi_lmmse_estimate (Nfft = Np = 234, Nps = 1):
 *   noise        nv = sum_{s < Nt} sum_b |Y[s][b]|^2 / (14 Nt),  Y[s][b] = sum_{n < 256} x[320 s + 64 + n] exp(-2 pi i b n / 256) over the
 *                14 null carriers b (1-based shifted bins [1:7 129 251:256] = FFT bins 0 and 122 ... 134), where the VHT-LTF is zero.
 *                The DC bin IS counted.  nv is the variance per complex bin of one sounding symbol in the units of h (what
 *                synth.link_noise_var models); the error variance of an LS row is nv / Nt.
 *   correlation  c[d] = 1 / (234 Nt) sum_j sum_{k < 234 - d} h_ls[j][k + d] conj(h_ls[j][k]),  d = 0 .. 233: the Nt links of an rx antenna
 *                share one delay profile.  The biased estimate: T = Toeplitz(c) is positive definite for any non-zero input.
 *   smoother     out[j] = h_ls[j] - (nv / Nt) T^-1 h_ls[j]   (T estimates R_h + (nv / Nt) I as it stands).
 *   guards       all-zero LS rows (c[0] == 0): out = h_ls.  A step of the Levinson recursion whose 1 - |ef|^2 is not positive or
 *                not finite: that (packet, rx)'s LS rows go out unchanged and the read-only option "lmmse_blind_fallbacks" counts
 *                it (the count is kept on the device: reading it waits for the context's stream).  Non-finite inputs are not
 *                screened; they end in that fallback.
 * ltf_re / ltf_im [npkt][nr][len_ltf] (len_ltf >= 320 Nt); h_re / h_im: LS estimate [npkt][nr][nt][234]; out like h and may alias h
 * (re with re, im with im); noise_var [npkt][nr] and corr [npkt][nr][234][2] (re, im) doubles, either may be NULL.  All three kernels
 * compute in fp64 with sums in a fixed order: a packet's bits do not depend on the call or chunk that holds it.
 * csi_lmmse_blind_device: planes as for csi_lmmse_estimate_device (16-byte boundaries; the two double arrays 8); asynchronous on the
 * context's stream; usable inside csi_capture_begin / _end after one eager call of the same shape (statistics the caller does not
 * keep live in a context workspace sized by eager calls).  csi_lmmse_blind: host buffers, packet chunks of csi_lmmse_estimate's size.
 * Refused with text: npkt <= 0, null ltf / h / out pointers, misaligned planes, a single-input context.  A null context returns -1.
 * Profile entries "lmmse_null_noise", "lmmse_freq_corr", "lmmse_blind". */
int  csi_lmmse_blind(csi_ctx* ctx, const float* ltf_re, const float* ltf_im, const float* h_re, const float* h_im, int64_t npkt,
                     float* out_re, float* out_im, double* noise_var, double* corr);
int  csi_lmmse_blind_device(csi_ctx* ctx, const float* d_ltf_re, const float* d_ltf_im, const float* d_h_re, const float* d_h_im,
                            int64_t npkt, float* d_out_re, float* d_out_im, double* d_noise_var, double* d_corr);

/* Delay-subspace smoother of a CSI tensor (csrc/subspace_smooth.hip.h, csrc/csi_subspace.hpp).  An addition: the
 * reference has no such estimator.  It stands where LMMSE_ce stands (helperMIMOChannelEstimate.m:37-39) and needs no SNR, no
 * power-delay profile and no training: fit the LS row with a channel of at most L delay taps and evaluate the fit on the data carriers.
 *   carriers   ind = the 234 data carriers in 1-based shifted bins as generate_maMIMO_LTF.m:72-78 has them: 1 .. 256 without the nulls
 *              [1:7 129 251:256] and the pilots [26 54 90 118 140 168 204 232]; f_k = ind_k - 129, in -128 .. 127.
 *   basis      for a window (L, pre), 1 <= L <= 128, 0 <= pre <= L:  F[k][l] = exp(-2 pi i f_k (l - pre) / 256), l < L;  thin SVD
 *              F = U S V^H in fp64;  r = number of s_j > 1e-10 s_0;  Q = U[:, :r];  lam_j = s_j^2 / L  (subspace.delay_basis of the
 *              Python package).  The sign is that of the generators: H[b] = sum_l c_l exp(-2 pi i b l / 256).
 *   smoother   for every row x of 234 values of the [npkt][Nr][Nt][234] planes:
 *                  t_j = sum_k conj(Q[k][j]) x_k,   y_k = sum_j Q[k][j] w[p][rx][j] t_j
 *              w float32 [npkt][Nr][r]; NULL means all ones (the projection onto the window).  With
 *              w_j = lam_j / (lam_j + nu)  (subspace.robust_weights) the map is R (R + nu I)^-1 for R = F F^H / L written in its
 *              eigenbasis Q: the robust LMMSE smoother for a uniform delay profile.
 * csi_subspace_set_basis: host planes q_re / q_im [234][rank], rank 1 .. 128, kept on the context as device copies; a second call
 * replaces them (it waits for the stream; graphs captured with the earlier basis must be captured again).  Refused with text: rank
 * outside 1 .. 128, null planes, a non-finite entry, a Q^H Q further than 1e-4 from the identity in any entry, an open capture.
 * ANY orthonormal Q is accepted; the delay window is what the Python package builds.
 * csi_subspace_smooth_device: d_h_re / d_h_im [npkt][Nr][Nt][234], d_out like d_h, d_w [npkt][Nr][rank] or NULL.  One kernel launch on
 * the context's stream, asynchronous, no workspace, usable inside csi_capture_begin / _end.  Exact fp32 products with fp32
 * accumulation (v_mfma_f32_32x32x2_f32) in a fixed order: a packet's bits do not depend on the call, the chunk or its position in
 * the batch.  out may be the input planes themselves, re with re and im with im; any other overlap of an output plane with an
 * input plane or with the other output plane is refused.
 * csi_subspace_smooth: host buffers, in the packet chunks of csi_lmmse_estimate (256 MiB of staging; the context's workspace_bytes
 * when that is smaller), w [npkt][Nr][rank] or NULL; same bits as the device entry point.
 * Refused with text, before anything is launched or counted: no basis set (CSI_ERR_NOT_READY), npkt < 0, null h / out pointers,
 * planes off a 16-byte boundary, overlapping planes, a single-input context.  npkt == 0 returns 0 and launches nothing.  A null
 * context returns -1.  Read-only option "subspace_launches"; profile entry "subspace_smooth" (16 * rows * 234 * rank flop). */
int  csi_subspace_set_basis(csi_ctx* ctx, const float* q_re, const float* q_im, int rank);
int  csi_subspace_smooth(csi_ctx* ctx, const float* h_re, const float* h_im, int64_t npkt, const float* w, float* out_re, float* out_im);
int  csi_subspace_smooth_device(csi_ctx* ctx, const float* d_h_re, const float* d_h_im, int64_t npkt, const float* d_w,
                                float* d_out_re, float* d_out_im);

/* Beam-space Wiener smoother of a CSI tensor across the Tx antennas (csrc/beam_smooth.hip.h, csrc/csi_beam.hpp).  An
 * addition: the reference has no such estimator.  It stands where LMMSE_ce stands (helperMIMOChannelEstimate.m:37-39) and is the
 * antenna-domain counterpart of the delay-subspace smoother above: the paths that reach a user leave a half-wavelength ULA inside a
 * narrow cone, so across the antennas h[p][rx][:][k] is a sum of a few steering vectors.  It needs no direction, no angular spread, no
 * SNR from a simulator and no training.
 * The planes are [npkt][Nr][Nt][234], re and im separate, as everywhere.  For an orthonormal basis A [Nt][nb] with
 * 1 <= nb <= Nt <= 128, for every (packet p, rx r):
 *     t_b[k]  = sum_j conj(A[j][b]) h[p][r][j][k]              b < nb, k < 234
 *     E[p][r][b] = (1 / 234) sum_k |t_b[k]|^2                  (beam power)
 *     y_j[k]  = sum_b A[j][b] w[p][r][b] t_b[k]
 * w float32 [npkt][Nr][nb]; NULL means all ones (the projection onto the span of A).  The Wiener entry makes its own weights from
 * v float32 [npkt][Nr], the error variance of ONE element of the input planes:  w = 1 - v / E  where E > v,  w = 0  everywhere else
 * (E = 0 falls under this case).  Non-finite inputs are not screened.
 * The Python package builds the DFT beams of the half-wavelength ULA (beamspace.dft_basis):  A[j][b] = exp(-2 pi i y_j u_b) / sqrt(Nt),
 * y_j = (j - (Nt - 1) / 2) / 2,  u_b = 2 (b - Nt / 2) / Nt  - the sign of the transmit factor exp(-2 pi i y_j v_s) of
 * csrc/synth_scattering.hip.h.  The library accepts ANY orthonormal A, as csi_subspace_set_basis does.
 * csi_beam_set_basis: host planes a_re / a_im [Nt][nb], kept on the context as device images padded to whole tiles of 32; a second
 * call replaces them (it waits for the stream; graphs captured with the earlier basis must be captured again).  Refused with text: nb
 * outside 1 .. Nt, null planes, a non-finite entry, an A^H A further than 1e-4 from the identity in any entry (checked in double on
 * the host), an open capture, a single-input context, Nt > 128.
 * csi_beam_power_device: d_power [npkt][Nr][nb] = E.  One launch.
 * csi_beam_smooth_device: d_w [npkt][Nr][nb] or NULL, d_out like d_h.  One launch, no workspace.  out may be the input planes
 * themselves, re with re and im with im; any other overlap of an output plane with an input plane or with the other output plane is
 * refused.
 * csi_beam_wiener_device: d_err_var [npkt][Nr], d_w_out [npkt][Nr][nb] or NULL.  Three launches: the power pass, the weight pass, the
 * smoothing pass (h is read twice).  E, and w when the caller keeps none, live in a context workspace sized by eager calls: inside
 * csi_capture_begin / _end the call is usable after one eager call of the same shape, as csi_lmmse_blind_device is.  The output is
 * bit for bit what csi_beam_smooth_device gives with the w it reports, and E bit for bit what csi_beam_power_device writes.
 * All products are exact fp32 products with fp32 accumulation (v_mfma_f32_32x32x2_f32) and every sum, the 234-carrier sum of E
 * included, runs in an order that depends on Nt, nb and the carrier index only (no atomics): the bits of a (packet, rx) do not depend
 * on the call, the chunk or its position in the batch.  The *_device entries enqueue on the context's stream and do not wait.
 * csi_beam_smooth / csi_beam_wiener: host buffers, in the packet chunks of csi_subspace_smooth (256 MiB of staging; the context's
 * workspace_bytes when that is smaller); same bits as the device entries.  w_out of csi_beam_wiener may be NULL.
 * csi_null_noise_device: d_noise_var double [npkt][Nr] = the null-carrier statistic of csi_lmmse_blind_device on its own, from the
 * preambles d_ltf [npkt][Nr][len_ltf]: same kernel, same definition, same bits as that entry's noise_var output.  The error variance
 * of one element of the LS estimate of these preambles is noise_var / Nt.
 * Every entry returns -1 on a null context, and refuses with text, before anything is launched or counted: npkt < 0, null required
 * pointers, planes off a 16-byte boundary, and (the csi_beam_* entries) no basis set (CSI_ERR_NOT_READY).  npkt == 0 returns 0 and
 * launches nothing.  Read-only option "beam_launches"; profile entries "beam_power" (planes * 234 * nb * (8 Nt + 3) flop,
 * planes * (8 * 234 Nt + 4 nb) + 8 Nt nb bytes) and "beam_smooth" (16 * planes * 234 * Nt * nb flop, planes * (16 * 234 Nt + 4 nb)
 * + 16 Nt nb bytes); planes = npkt * Nr. */
int  csi_beam_set_basis(csi_ctx* ctx, const float* a_re, const float* a_im, int nb);
int  csi_beam_power_device(csi_ctx* ctx, const float* d_h_re, const float* d_h_im, int64_t npkt, float* d_power);
int  csi_beam_smooth(csi_ctx* ctx, const float* h_re, const float* h_im, int64_t npkt, const float* w, float* out_re, float* out_im);
int  csi_beam_smooth_device(csi_ctx* ctx, const float* d_h_re, const float* d_h_im, int64_t npkt, const float* d_w,
                            float* d_out_re, float* d_out_im);
int  csi_beam_wiener(csi_ctx* ctx, const float* h_re, const float* h_im, int64_t npkt, const float* err_var, float* out_re, float* out_im,
                     float* w_out);
int  csi_beam_wiener_device(csi_ctx* ctx, const float* d_h_re, const float* d_h_im, int64_t npkt, const float* d_err_var,
                            float* d_out_re, float* d_out_im, float* d_w_out);
int  csi_null_noise_device(csi_ctx* ctx, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt, double* d_noise_var);

/* Hybrid beamforming weights from a CSI tensor (BER_test_maMIMO_LTF.m:347-376, generate_maMIMO_LTF.m:414-425: the toolbox's
 * SVD + orthogonal-matching-pursuit split of the optimal precoder into an analog and a digital part).  One item = one
 * (packet p, subcarrier k) with H[i][j] = csi[p][i][j][k] (Nr x Nt):
 *   Fopt = right singular vectors of H for its ns largest singular values;
 *   for m = 1 .. ntrf, Res = Fopt at the start: k_m = argmax_k sum_s |At[:,k]^H Res[:,s]|^2 (lowest k on a tie),
 *     C = (A^H A)^-1 A^H Fopt over the chosen columns A, T = Fopt - A C, e = |T|_F, Res = T / e; stop when e <= stop_tol;
 *   Fbb = sqrt(ns) C / |A C|_F.
 * Outputs in the reference's orientation: fbb [npkt][234][ns][ntrf] (re / im planes), idx int32 [npkt][234][ntrf] (the analog part
 * is frf[m][:] = At[:, idx[m]] and is not written out), n_atoms int32 [npkt][234], gain [npkt][234] = |H_eval frf^T fbb^T|_F^2
 * with H_eval = the eval planes (same shape as h) or h itself when they are NULL, frf_mean [npkt][ntrf][Nt] = mean of frf over a
 * packet's subcarriers.  Slots behind an early stop hold index -1 and zero coefficients (and add nothing to frf_mean).
 * An all-zero item has Fopt = 0 and every metric 0: its first step takes column 0 (the lowest index of the tie), fits it with zero
 * coefficients and stops there - n_atoms 1, idx (0, -1, ..), fbb 0, gain 0, every output finite; other items are not affected.
 * stop_tol <= 0 selects 1e-5.  eval, n_atoms, gain and frf_mean may be NULL.
 * csi_hybrid_set_dictionary: host planes [Nt][n_rays], n_rays <= 4096, kept on the context; columns are used as given (no
 * normalisation); a second call replaces the dictionary.
 * csi_hybrid_weights_device: asynchronous on the context's stream, inputs are the planes csi_predict_device /
 * csi_ls_estimate_device / csi_lmmse_estimate_device write; large calls run in packet chunks against the context's
 * workspace_bytes (default 1 GiB for this stage).  Refused with text: no dictionary, Nr > Nt, Nr > 16, ns outside
 * 1 .. min(Nr, ntrf), ntrf outside 1 .. min(Nt, n_rays, 16), bf16 contexts, null required pointers.
 * "hybrid_launches" (csi_get_option) counts the kernels launched. */
int  csi_hybrid_set_dictionary(csi_ctx* ctx, const float* at_re, const float* at_im, int n_rays);
int  csi_hybrid_weights_device(csi_ctx* ctx, const float* d_h_re, const float* d_h_im, const float* d_eval_re, const float* d_eval_im,
                               int64_t npkt, int ns, int ntrf, float stop_tol, float* d_fbb_re, float* d_fbb_im, int32_t* d_idx,
                               int32_t* d_n_atoms, float* d_gain, float* d_frf_mean_re, float* d_frf_mean_im);
int  csi_hybrid_weights(csi_ctx* ctx, const float* h_re, const float* h_im, const float* eval_re, const float* eval_im, int64_t npkt,
                        int ns, int ntrf, float stop_tol, float* fbb_re, float* fbb_im, int32_t* idx, int32_t* n_atoms, float* gain,
                        float* frf_mean_re, float* frf_mean_im);

/* Several device-pointer calls as ONE hipGraph (for instance csi_estimate_device followed by csi_hybrid_weights_device):
 * between csi_capture_begin and csi_capture_end the device-pointer calls on this context are recorded on its stream instead of
 * run.  Run the same calls once eagerly first: a call that has to grow a buffer fails inside a capture.  csi_capture_end hands back
 * the graph (also after a failed call: the capture must be closed); csi_capture_launch replays it on the context's stream and
 * refuses a graph that a later reallocation, weight / pilot / dictionary load or option change made stale. */
int  csi_capture_begin(csi_ctx* ctx);
int  csi_capture_end(csi_ctx* ctx, void** graph);
int  csi_capture_launch(csi_ctx* ctx, void* graph);
void csi_capture_free(csi_ctx* ctx, void* graph);

/* Link-level simulation of a beamformed data phase (BER_test_maMIMO_LTF.m:408-646; model and deviations: DESIGN.md 4.17,
 * csrc/link_sim.hip.h).  Per packet p one terminated codeword of the rate-1/3, K = 7 code (133, 171, 165 octal) over
 * n_info = n_steps - 6 counter-based random bits, n_steps = ns n_sym 234 bps / 3; square Gray QAM (bps 2 or 4), coded bit
 * c = ((s n_sym + n) 234 + k) bps + b; precoder W_k = sqrt(Nt) F_k / |F_k|_F with F_k = frf_mean^T fbb_k^T from the planes
 * csi_hybrid_weights_device writes (fbb [npkt][234][ns][ntrf], frf_mean [npkt][ntrf][Nt]); y = H_k W_k d + w through the TRUE
 * channel planes h [npkt][Nr][Nt][234] of csi_synth_structured with noise of variance noise_var[p] per complex sample (draws of
 * the stream `seed`, absolute packet index first_pkt + p: packets are the same bits whichever call holds them); zero forcing with
 * the exact effective channel, max-log soft bits (positive = 0), Viterbi decoding.
 * Outputs per packet: bit_errors int32 (against the information bits), evm_rms (100 sqrt(mean |x - nearest point|^2)),
 * dt_snr_db (10 log10(sum_k |H_k W_k|_F^2 / sum_k |H_k|_F^2)).  Optional (may be NULL): xeq planes [npkt][ns][n_sym][234] (as a
 * pair), csi [npkt][ns][234] (1 / [(G^H G)^-1]_ss; 0 and x = 0 where G^H G is singular), llr [npkt][n_coded], bits uint8
 * [npkt][n_info] (the decoded bits).
 * csi_link_frame_bits: n_info and n_coded of (ns, n_sym, bps); -1 for ns outside 1 .. 4, n_sym < 1 or bps not in {2, 4}.
 * csi_viterbi_decode_device: the decoder alone, llr [ncw][3 n_steps] -> bits uint8 [ncw][n_steps - 6].  fp32 path metrics; the
 * larger sum survives, on equal sums the predecessor with the lower state number; start and end state 0.
 * Both device calls are asynchronous on the context's stream, usable inside csi_capture_begin / _end (after one eager call of
 * the same shape) and serve fp32 and bf16 contexts alike (every plane is fp32).  csi_link_sim_device runs in packet chunks
 * against the context's workspace_bytes (default 1 GiB for this stage) with the same bits whatever the chunking.
 * Refused with text: null required pointers, bps not in {2, 4}, ns outside 1 .. min(4, Nr, ntrf), ntrf < 1, n_sym < 1,
 * n_steps > 8190 (csi_viterbi_decode_device: outside 7 .. 8190), negative npkt / first_pkt / ncw, one xeq plane without the other,
 * a single-input context, shapes whose per-packet LDS image (Nr ns and ns ntrf) passes 160 KiB.  A null context returns -1.
 * Profile entries "link_txrx" (encoder + transmit / receive pass) and "link_viterbi"; "link_launches" (csi_get_option) counts
 * the kernels launched. */
int  csi_link_frame_bits(int ns, int n_sym, int bps, int64_t* n_info, int64_t* n_coded);
int  csi_viterbi_decode_device(csi_ctx* ctx, const float* d_llr, int64_t ncw, int64_t n_steps, uint8_t* d_bits);
int  csi_link_sim_device(csi_ctx* ctx, const float* d_h_re, const float* d_h_im, const float* d_fbb_re, const float* d_fbb_im,
                         const float* d_frf_re, const float* d_frf_im, const float* d_noise_var, uint64_t seed, int64_t first_pkt,
                         int64_t npkt, int ns, int ntrf, int n_sym, int bps, int32_t* d_bit_errors, float* d_evm_rms,
                         float* d_dt_snr_db, float* d_xeq_re, float* d_xeq_im, float* d_csi, float* d_llr, uint8_t* d_bits);

/* The same data phase with a receiver that does not know the effective channel (BER_test_maMIMO_LTF.m / generate_maMIMO_LTF_SINR.m:
 * 433-435, 528-533: a precoded preamble in front of the data).  n_ltf = csi_link_preamble_symbols(ns) = 1, 2, 4, 4 preamble symbols
 * with the pilot matrix P = P4[0:ns][0:n_ltf] (the 802.11 matrix) pass through the same G_k = H_k W_k:
 * Ypre[m][r] = sum_s G[r][s] P[s][m] + w[m][r]; the receiver forms Ghat[r][s] = (1 / n_ltf) sum_m Ypre[m][r] P[s][m] and equalises
 * the data with Ghat in place of G (A = Ghat^H Ghat, z = Ghat^H y, csi_s = 1 / [A^-1]_ss; the same singular rule).  The preamble noise
 * continues the packet's data noise stream at symbol index n_sym + m, so the data symbols are, draw for draw, those of
 * csi_link_sim_device: the two entries are a paired comparison, and with noise_var = 0 and ns = 1 they agree bit for bit.
 * dt_snr_db is that of the true G.  Arguments, refusals and chunking of csi_link_sim_device, then
 *   d_g_nmse [npkt] (required): sum_{k,r,s} |Ghat - G|^2 / sum_{k,r,s} |G|^2; 0 when both sums are 0, otherwise the IEEE quotient
 *   d_gest_re / d_gest_im [npkt][234][Nr][ns] (optional, as a pair): Ghat.
 * Also refused: one gest plane without the other, a null d_g_nmse; the LDS image holds G twice.  Profile entries and counter as above.
 * csi_link_preamble_symbols: n_ltf of ns; -1 for ns outside 1 .. 4. */
int  csi_link_preamble_symbols(int ns);
int  csi_link_sim_rx_device(csi_ctx* ctx, const float* d_h_re, const float* d_h_im, const float* d_fbb_re, const float* d_fbb_im,
                            const float* d_frf_re, const float* d_frf_im, const float* d_noise_var, uint64_t seed, int64_t first_pkt,
                            int64_t npkt, int ns, int ntrf, int n_sym, int bps, int32_t* d_bit_errors, float* d_evm_rms,
                            float* d_dt_snr_db, float* d_xeq_re, float* d_xeq_im, float* d_csi, float* d_llr, uint8_t* d_bits,
                            float* d_g_nmse, float* d_gest_re, float* d_gest_im);

/* Multi-user downlink (BER_test_maMIMO_LTF.m:110-112, 238-246, 360-385, 417-484, prm.numUsers; model and deviations: DESIGN.md 4.20,
 * csrc/mu_link.hip.h).  An addition: the ABI version stays 1.  U = n_users users (1 .. 8), each with CSI planes [npkt][Nr][Nt][234]; ns
 * streams per user (1 .. min(4, Nr)) addressed to the user's receive antennas 0 .. ns-1; M = U ns <= min(16, Nt); stream m = u ns + s.
 * csi_mu_precoder_device: per (packet p, subcarrier k)  B[m][j] = hest_u[p][s][j][k],  A = B B^H + reg[p] I (d_reg [npkt], NULL = 0:
 * zero forcing; the regularised form uses reg = M noise_var / Nt),  Cholesky A = L L^H (a pivot <= 0 or not finite: W = 0 for the item),
 * V = B^H A^-1,  W[:, m] = sqrt(Nt / M) V[:, m] / |V[:, m]|_2 (a zero or non-finite norm: 0), so that |W|_F^2 = Nt.  d_hest_re / d_hest_im
 * are HOST arrays of U device pointers (read before the call returns); d_w_re / d_w_im [npkt][M][Nt][234].  One kernel launch.
 * csi_mu_link_sim_device: the data phase of csi_link_sim_device for every user through the TRUE planes d_h_re / d_h_im (host arrays of
 * U device pointers) with the precoder planes W.  User seed: seed_0 = seed, seed_u = splitmix64(seed ^ splitmix64(u)); bits, encoder,
 * mapper and frame sizes of csi_link_sim_device for (ns, n_sym, bps) on the stream seed_u; at user u, antenna i < ns,
 * y = sum_m G_u[i][m] d_m + w with G_u = H_u[0:ns] W (ns x M) and noise of variance d_noise_var[u][p] (draws of the stream seed_u with
 * Nr = ns in the index: user 0 with ns = Nr has the bits and the noise of csi_link_sim_device); the single-user equaliser on the user's
 * own ns x ns block G_uu, the same singular rule; soft bits csi_s / noise_var times the max-log difference - the interference of the other
 * users' streams is NOT in the scale, the receiver does not know it; Viterbi decoding.
 * Outputs [U][npkt]: bit_errors int32, evm_rms, sinr_db = 10 log10(sum_k |G_uu|_F^2 / (sum_k |G_u,others|_F^2 + 234 ns noise_var)) (the
 * IEEE quotient; G_u,others = the columns of the other users).  Optional (may be NULL; planes as pairs): g [U][npkt][ns][M][234],
 * xeq [U][npkt][ns][n_sym][234], csi [U][npkt][ns][234], llr [U][npkt][n_coded], bits uint8 [U][npkt][n_info].
 * Both calls are asynchronous on the context's stream and serve fp32 and bf16 contexts alike (every plane is fp32); the data phase runs
 * in packet chunks against the context's workspace_bytes (the U codewords' coded bits and, when the caller keeps none, their soft bits;
 * default 1 GiB) with the same bits whatever the chunking.
 * Refused with text, before anything is launched or counted: n_users outside 1 .. 8, ns outside 1 .. min(4, Nr), M > 16 or M > Nt, bps
 * not in {2, 4}, n_sym < 1, n_steps > 8190, negative npkt / first_pkt, null required pointers or a null entry of a pointer array, one
 * plane of a pair without the other, planes off a 16-byte boundary, a single-input context, an LDS image beyond 160 KiB.  npkt == 0
 * returns 0 and launches nothing; a null context returns -1.  Read-only option "mu_launches"; profile entries "mu_precoder" and
 * "mu_txrx" (encoders + transmit / receive pass); the decoder is counted under "link_viterbi". */
int  csi_mu_precoder_device(csi_ctx* ctx, int n_users, const float* const* d_hest_re, const float* const* d_hest_im, int64_t npkt, int ns,
                            const float* d_reg, float* d_w_re, float* d_w_im);
int  csi_mu_link_sim_device(csi_ctx* ctx, int n_users, const float* const* d_h_re, const float* const* d_h_im, const float* d_w_re,
                            const float* d_w_im, const float* d_noise_var, uint64_t seed, int64_t first_pkt, int64_t npkt, int ns,
                            int n_sym, int bps, int32_t* d_bit_errors, float* d_evm_rms, float* d_sinr_db, float* d_g_re, float* d_g_im,
                            float* d_xeq_re, float* d_xeq_im, float* d_csi, float* d_llr, uint8_t* d_bits);

/* Multi-user hybrid precoder (generate_maMIMO_LTF_SINR.m:357-369, helperJSDMTransmitWeights - a toolbox helper outside the reference tree;
 * model, deviation from JSDM and kernel plans: DESIGN.md 4.22, csrc/mu_hybrid.hip.h).  An addition: the ABI version stays 1.  The shapes of
 * csi_mu_precoder_device (U users, ns streams per user, M = U ns, B_k[m][j] = hest_u[p][s][j][k]), the dictionary At [Nt][R] of
 * csi_hybrid_set_dictionary (columns as given) and n_rf RF chains, M <= n_rf <= min(16, Nt, R):
 *   score     S[p][m][r] = sum_k | sum_j B_k[m][j] At[j][r] |^2  (fp32 MFMA; every sum in an order that depends on Nt, R and the subcarrier
 *             index alone, no atomics)
 *   select    per packet, q = 0 .. n_rf-1: stream m = q mod M; idx[p][q] = argmax over the rays not yet taken in this packet of S[p][m][r],
 *             the lowest r on a tie, a non-finite score compares as -inf;  Frf[:, q] = At[:, idx[p][q]] (Nt x n_rf, flat over the subcarriers)
 *   baseband  per (packet, subcarrier): G = B_k Frf,  A = G G^H + reg[p] I (d_reg [npkt], NULL = 0),  Cholesky A = L L^H (a pivot <= 0 or
 *             not finite: W = 0 and Fbb = 0 for the item),  Vbb = G^H A^-1,  V = Frf Vbb,  c_m = sqrt(Nt / M) / |V[:, m]|_2 (a zero or
 *             non-finite norm: 0),  W[:, m] = c_m V[:, m],  Fbb[:, m] = c_m Vbb[:, m]:  W = Frf Fbb and |W|_F^2 = Nt, the normalisation of
 *             csi_mu_precoder_device.
 * Outputs: d_w_re / d_w_im [npkt][M][Nt][234] (what csi_mu_link_sim_device reads), d_idx int32 [npkt][n_rf]; optional (may be NULL): the pair
 * d_fbb_re / d_fbb_im [npkt][234][n_rf][M], d_score [npkt][M][R].  d_hest_re / d_hest_im are HOST arrays of U device pointers.
 * Asynchronous on the context's stream; serves fp32 and bf16 contexts alike; usable inside csi_capture_begin / _end after one eager call
 * of the same shape.  Runs in packet chunks against the context's workspace_bytes when d_score is NULL (the score planes of a chunk live
 * in the workspace; default 1 GiB), three kernel launches per chunk, with the same bits whatever the chunking, the call or the packet's
 * position in it.
 * Refused with text, before anything is launched or counted: everything csi_mu_precoder_device refuses, no dictionary set
 * (CSI_ERR_NOT_READY), n_rf outside M .. min(16, Nt, R), one fbb plane without the other, planes off a 16-byte boundary, an LDS image beyond
 * 160 KiB (the score kernel stages four dictionary tiles, 1 KiB per antenna: Nt > 160), an open capture that would have to grow the workspace.  npkt == 0 returns 0 and launches nothing; a null context returns -1.
 * The launches count under "mu_launches"; profile entries "mu_beam_score", "mu_beam_select" and "mu_hybrid_precoder". */
int  csi_mu_hybrid_precoder_device(csi_ctx* ctx, int n_users, const float* const* d_hest_re, const float* const* d_hest_im, int64_t npkt,
                                   int ns, int n_rf, const float* d_reg, float* d_w_re, float* d_w_im, int32_t* d_idx, float* d_fbb_re,
                                   float* d_fbb_im, float* d_score);

/* Multi-user JSDM precoder (BER_test_maMIMO_LTF.m:355-389: joint spatial division multiplexing - the users grouped by their transmit
 * covariance, an analog matrix from the covariance eigenvectors after a block diagonalisation that nulls the other groups, a precoder per
 * group behind it; model, deviation from the toolbox helper and kernel plans: DESIGN.md 4.23, csrc/mu_jsdm.hip.h).  An addition: the ABI
 * version stays 1.  The shapes of csi_mu_precoder_device (U users, ns streams per user, M = U ns <= 16, B_k[m][j] = hest_u[p][s][j][k]) and
 *   group[u]   a HOST array of U ints with values 0 .. G-1, every group non-empty; NULL: every user is its own group
 *   r_star     >= 0, directions of a group that the others null;  n_beams = b >= 1 RF chains per group, n_rf = G b <= 16;  rank_tol >= 0
 *   flags      bit 0: per-group processing (PGP, the reference's block-diagonal form), otherwise joint processing (JGP); bit 1: analog
 *              weights of unit modulus
 *   conditions ns |group g| <= b for every group, (G-1) r_star <= Nt - b, Nt <= 64
 *   cov        per (packet, user): R_u[j][j'] = (1 / (Nr 234)) sum_{i < Nr} sum_k conj(h_u[i][j][k]) h_u[i][j'][k]  (all Nr receive
 *              antennas; Nt x Nt Hermitian, to the bit; a beam w has mean gain w^H R w; fp32 MFMA, every sum in an order fixed by the shape,
 *              no atomics).  R_g = the mean over the users of group g in ascending user order
 *   eig        R_g = U_g L_g U_g^H, eigenvalues descending; in each eigenvector the entry of largest modulus is real and positive, the
 *              lowest j on a tie.  r_g = the number of i < r_star with l_i > rank_tol l_0 (l_0 <= 0 or not finite: 0); U*_g = the first r_g
 *              columns.  (Hermitian Jacobi in fp32, parallel round-robin ordering; with s = max_j |R[j][j]| a rotation is applied where
 *              |R[p][q]| > 2^-23 s, the first sweep without one ends the iteration, 24 sweeps at the most)
 *   null       Xi_g = [U*_g' : g' != g, ascending]; Q_g = modified Gram-Schmidt of Xi_g in column order, two passes, a column whose
 *              residual is <= 1e-3 of its norm is dropped, q_g columns kept; Rt_g = P R_g P - l_0(R_g) Q_g Q_g^H with P = I - Q_g Q_g^H,
 *              symmetrised: span(Q_g) goes to the bottom of the spectrum, so the leading eigenvectors of Rt_g lie in the null space even
 *              where P R_g P has rank below b
 *   beams      F_g = the first b eigenvectors of Rt_g, same convention; with bit 1 F_g[j][q] = exp(i arg F_g[j][q]) / sqrt(Nt) (arg of an
 *              exact 0 is 0).  Frf[p] = [F_0 ... F_{G-1}], Nt x n_rf, flat over the subcarriers
 *   baseband   per (packet, subcarrier), the stage of csi_mu_hybrid_precoder_device with the packet's own Frf: Gm = B_k Frf, with PGP the
 *              entries whose chain's group differs from the stream's group set to 0; A = Gm Gm^H + reg[p] I; Cholesky (a pivot <= 0 or not
 *              finite: W = 0 and Fbb = 0 for the item); Vbb = Gm^H A^-1; V = Frf Vbb; c_m = sqrt(Nt / M) / |V[:, m]|_2; W[:, m] = c_m V[:, m],
 *              Fbb[:, m] = c_m Vbb[:, m]: W = Frf Fbb, |W|_F^2 = Nt, and with PGP Fbb is block diagonal with exact zeros elsewhere.
 * csi_mu_covariance_device writes the covariances alone, d_cov_re / d_cov_im [npkt][U][Nt][Nt] (one launch).  csi_mu_jsdm_precoder_device:
 * the optional pair d_cov_re / d_cov_im IN replaces the covariance step (a caller's long-term covariance); outputs d_w_re / d_w_im
 * [npkt][M][Nt][234] (what csi_mu_link_sim_device reads); optional (may be NULL): the pairs d_frf_re / d_frf_im [npkt][Nt][n_rf],
 * d_fbb_re / d_fbb_im [npkt][234][n_rf][M], d_eig [npkt][G][Nt] (descending), the pair d_ustar_re / d_ustar_im [npkt][G][Nt][r_star] (zero
 * past r_g), d_rank int32 [npkt][G][2] = (r_g, q_g).  d_hest_re / d_hest_im are HOST arrays of U device pointers.
 * Both are asynchronous on the context's stream, serve fp32 and bf16 contexts alike and are usable inside csi_capture_begin / _end after
 * one eager call of the same shape.  The precoder runs in packet chunks against the context's workspace_bytes (the covariance, eigenvalue,
 * U*, rank and Frf planes of a chunk live in the workspace; default 1 GiB), four kernel launches per chunk (three with the covariances
 * handed in), with the same bits whatever the chunking, the call or the packet's position in it.
 * Refused with text, before anything is launched or counted: everything csi_mu_precoder_device refuses, a group entry outside 0 .. G-1 or
 * an empty group, n_rf > 16, ns |group g| > b, r_star < 0 or > Nt, (G-1) r_star > Nt - b, rank_tol negative or not finite, unknown flag
 * bits, Nt > 64 (the eigen kernel holds the matrix and the vectors in LDS), one plane of a pair without the other, planes off a 16-byte
 * boundary, an open capture that would have to grow the workspace.  npkt == 0 returns 0 and launches nothing; a null context returns -1.
 * The launches count under "mu_launches"; profile entries "mu_cov", "mu_jsdm_eig" and "mu_jsdm_baseband". */
int  csi_mu_covariance_device(csi_ctx* ctx, int n_users, const float* const* d_hest_re, const float* const* d_hest_im, int64_t npkt,
                              float* d_cov_re, float* d_cov_im);
int  csi_mu_jsdm_precoder_device(csi_ctx* ctx, int n_users, const float* const* d_hest_re, const float* const* d_hest_im, int64_t npkt,
                                 int ns, const int32_t* group, int r_star, int n_beams, float rank_tol, int flags, const float* d_reg,
                                 const float* d_cov_re, const float* d_cov_im, float* d_w_re, float* d_w_im, float* d_frf_re,
                                 float* d_frf_im, float* d_fbb_re, float* d_fbb_im, float* d_eig, float* d_ustar_re, float* d_ustar_im,
                                 int32_t* d_rank);

/* Quantised CSI feedback: the compressed beamforming report of IEEE 802.11-2016 19.3.12.3.6 with Nt rows, and its expansion at the
 * base station (model, plan and what is not modelled: DESIGN.md 4.24, csrc/feedback.hip.h).  An addition: the ABI version stays 1.
 *   reports    carriers k_r = r ng, r < n_rep = ceil(234 / ng), ng in {1, 2, 4}; carrier k is served by report k / ng (hold, no interpolation)
 *   V          per (packet, reported carrier) the nc <= min(4, Nr, Nt) dominant right singular vectors of H[i][j] = h[p][i][j][k_r], exactly
 *              the Fopt of csi_hybrid_weights_device (fp64 Jacobi on H H^H, largest first, lowest index on a tie, a zero column where
 *              sigma_s = 0); sigma[s] the singular value in fp32.  Column s is multiplied by exp(-j arg V[Nt-1][s]): the last row real and >= 0
 *   angles     for i = 0 .. min(nc, Nt-1) - 1:  phi[l][i] = arg V[l][i] in [0, 2 pi), l = i .. Nt-2, row l multiplied by exp(-j phi[l][i]);
 *              then for l = i+1 .. Nt-1 in this order psi[l][i] = atan2(Re V[l][i], Re V[i][i]) in [0, pi/2], rows (i, l) <- (c x_i + s x_l,
 *              -s x_i + c x_l) with c, s from the unquantised values (hypot 0: c = 1, s = 0).  n_ang = sum_i (Nt-1-i) angles of each kind,
 *              stored in this loop order
 *   codes      k_phi = floor(phi 2^(b_phi-1) / pi) mod 2^b_phi, k_psi = min(floor(psi 2^(b_psi+1) / pi), 2^b_psi - 1); the expansion uses
 *              the bin centres phi = pi (2^-b_phi + k 2^(1-b_phi)), psi = pi (2^-(b_psi+2) + k 2^-(b_psi+1)), their cos / sin computed on the
 *              host in double and rounded to fp32.  b_phi 2 .. 10, b_psi 1 .. 8 (the standard's pairs: SU (4,2) / (6,4), MU (7,5) / (9,7))
 *   expansion  the steps backwards on the first nc columns of the identity: Vhat has orthonormal columns whatever the codes
 * csi_feedback_compress_device: d_h_re / d_h_im [npkt][Nr][Nt][234] IN; d_phi_code / d_psi_code uint16 [npkt][n_ang][n_rep]; optional (may
 * be NULL): the continuous angles d_phi / d_psi fp32 [npkt][n_ang][n_rep], d_sigma [npkt][nc][n_rep], the pair d_v_re / d_v_im
 * [npkt][nc][Nt][n_rep] (the vectors after the column phases: what was decomposed).  b_phi = b_psi = 0 asks for the continuous angles only;
 * the code pointers may then be NULL.
 * csi_feedback_expand_device: exactly one of the pairs (d_phi_code, d_psi_code) and (d_phi, d_psi) is non-NULL; d_sigma [npkt][nc][n_rep]
 * or NULL; layout CSI_FB_LAYOUT_W: d_out_re / d_out_im [npkt][nc][Nt][234], the columns scaled by sqrt(Nt / nc), so |W|_F^2 = Nt - what
 * csi_mu_link_sim_device reads with n_users = 1, ns = nc; CSI_FB_LAYOUT_CSI: [npkt][Nr][Nt][234], row s < nc = sigma_s conj(Vhat[:, s])
 * (conj(Vhat[:, s]) when d_sigma is NULL), rows >= nc zero: the base station's rebuilt S V^H in the layout csi_mu_precoder_device and
 * every other estimate consumer reads.  sigma travels UNQUANTISED: the report's per-stream SNR fields are not modelled.
 * Both are asynchronous on the context's stream and serve fp32 and bf16 contexts alike (all planes are fp32).  The compression runs in
 * packet chunks against the context's workspace_bytes (the singular vectors of a chunk live in the workspace; default 1 GiB), one launch
 * per chunk; the expansion is one launch; the same bits whatever the chunking, the call or the packet's position in it.
 * Refused with text, before anything is launched or counted: nc outside 1 .. min(4, Nr, Nt), Nr > 16, ng not 1, 2 or 4, b_phi outside
 * 2 .. 10 or b_psi outside 1 .. 8 or only one of them 0, an unknown layout, null required pointers, one array of a pair without the other,
 * both or neither of the expansion's input pairs, re / im planes off a 16-byte boundary, a single-input context, a per-workgroup LDS image
 * beyond 160 KiB (Nt nc beyond 2560), negative npkt, an open capture that would have to grow the workspace or change the tables.
 * npkt == 0 returns 0 and launches nothing; a null context returns -1.  The launches count under "feedback_launches"; profile entries
 * "fb_compress" and "fb_expand". */
#define CSI_FB_LAYOUT_W 0
#define CSI_FB_LAYOUT_CSI 1
int  csi_feedback_compress_device(csi_ctx* ctx, const float* d_h_re, const float* d_h_im, int64_t npkt, int nc, int b_phi, int b_psi,
                                  int ng, uint16_t* d_phi_code, uint16_t* d_psi_code, float* d_phi, float* d_psi, float* d_sigma,
                                  float* d_v_re, float* d_v_im);
int  csi_feedback_expand_device(csi_ctx* ctx, const uint16_t* d_phi_code, const uint16_t* d_psi_code, const float* d_phi,
                                const float* d_psi, const float* d_sigma, int64_t npkt, int nc, int b_phi, int b_psi, int ng, int layout,
                                float* d_out_re, float* d_out_im);

/* Receive combining: the U^H combiner of a user's CSI estimate and its application to CSI planes (model, plan and traps: DESIGN.md 4.25,
 * csrc/rx_combine.hip.h).  An addition: the ABI version stays 1.
 *   combiner   per (packet, carrier), H[i][j] = hest[p][i][j][k] (Nr x Nt): row s < ns of C is exp(i t_s) u_s^H, u_s the left singular
 *              vector of the s-th largest singular value (fp64 Jacobi on H H^H as csi_hybrid_weights_device runs it: largest first, the
 *              lowest index on a tie); t_s makes (C H)[s][Nt-1] real and >= 0 (that element 0: no rotation) - the column phase of the
 *              feedback report, so conj((C H)[s][:]) / sigma_s is the d_v of csi_feedback_compress_device on the same planes and C H is
 *              what CSI_FB_LAYOUT_CSI expands to at continuous angles.  sigma[s] the singular value in fp32
 *   rank rule  a row whose eigenvalue is not > 0, not finite or not above 2^-40 of the largest (sigma_s <= 2^-20 sigma_1: the rounding of
 *              the Jacobi sweeps on a rank-deficient matrix) is all zero and its sigma is 0; the data phase's own singular rule then gives
 *              x = 0, csi = 0 for the item
 *   apply      E[s][j] = sum_{i < Nr} C[s][i] H[i][j] for s < ns (i ascending, fmaf chains), rows ns .. Nr-1 exact zeros: the CSI layout
 *              every estimate consumer reads.  H = the true planes gives the channel csi_mu_link_sim_device sees behind the combiner (its
 *              rows s < ns are the ns combined streams); H = the estimate gives the unquantised report S V^H
 *   noise      the rows of C are orthonormal, so C w of white noise w is white with the same variance: the data phase on E draws exactly
 *              the noise a combining receiver sees.  A combiner whose rows are not orthonormal would colour the noise: not modelled
 * csi_rx_combiner_device: d_hest_re / d_hest_im [npkt][Nr][Nt][234] IN; d_c_re / d_c_im [npkt][ns][Nr][234] OUT; d_sigma [npkt][ns][234]
 * OUT, optional (may be NULL).
 * csi_rx_apply_combiner_device: d_c_re / d_c_im [npkt][ns][Nr][234] IN, d_h_re / d_h_im [npkt][Nr][Nt][234] IN, d_e_re / d_e_im
 * [npkt][Nr][Nt][234] OUT (no overlap with the inputs).
 * Both are asynchronous on the context's stream, serve fp32 and bf16 contexts alike (all planes are fp32) and use no workspace: the same
 * bits whatever the call or the packet's position in it, and nothing to size in front of a capture.  The apply step is one launch.
 * Refused with text, before anything is launched or counted: ns outside 1 .. min(4, Nr), Nr > 16, a single-input context, null required
 * pointers, one plane of a pair without the other, re / im planes off a 16-byte boundary, negative npkt, a per-workgroup LDS image beyond
 * 160 KiB.  npkt == 0 returns 0 and launches nothing; a null context returns -1.  The launches count under "combine_launches"; profile
 * entries "rx_combiner" and "rx_combine". */
int  csi_rx_combiner_device(csi_ctx* ctx, const float* d_hest_re, const float* d_hest_im, int64_t npkt, int ns, float* d_c_re,
                            float* d_c_im, float* d_sigma);
int  csi_rx_apply_combiner_device(csi_ctx* ctx, const float* d_c_re, const float* d_c_im, const float* d_h_re, const float* d_h_im,
                                  int64_t npkt, int ns, float* d_e_re, float* d_e_im);

/* Accuracy metric of the reference's evaluation, NMSE_subk (BER_test_maMIMO_LTF.m:675-686): per link
 * ||ref - est||^2 / ||ref||^2 over the n_bins bins, mean over the nlinks links ([link][n_bins] planes, e.g.
 * the [npkt][nr][nt][234] outputs of csi_predict / csi_ls_estimate with nlinks = npkt*nr*nt).  Synchronous;
 * d_per_link (may be NULL) receives the per-link ratios, e.g. for per-packet averages
 * (snr_loop_testing.m:44,51,58). */
int  csi_nmse(csi_ctx* ctx, const float* ref_re, const float* ref_im, const float* est_re, const float* est_im,
              int64_t nlinks, int n_bins, double* mean_out);
int  csi_nmse_device(csi_ctx* ctx, const float* d_ref_re, const float* d_ref_im, const float* d_est_re, const float* d_est_im,
                     int64_t nlinks, int n_bins, float* d_per_link, double* mean_out);

/* ---- On-box fine-tuning: one optimiser step of the reference's fit(),
 * massiveMIMO_CSI_prediction_DNN.py:272-316, for one component model (fp32 contexts only).
 *   GaussianNoise on the LTF columns of x only (DNN.py:191-193; stddev per batch from the caller,
 *   changeNoisePower DNN.py:92-100) -> Dense(relu) -> BatchNormalization(batch statistics) ->
 *   Dropout after every hidden layer but the last (DNN.py:211-226) -> Dense(linear), loss 'mse',
 *   Adam (DNN.py:272-273).  Keras defaults: beta1 0.9, beta2 0.999, eps 1e-7, BN momentum 0.99. */
typedef struct {
    float    lr;            /* --lr (1e-4)                                                  */
    float    beta1, beta2, eps;
    float    bn_momentum;
    float    dropout;       /* --dropout (0.15)                                             */
    uint64_t seed;          /* noise / dropout / initialisation streams                     */
} csi_train_config;

/* Creates the trainer of model 0 (real) / 1 (imag) from the named tensors of csi_load_weights
 * (n > 0), or with Glorot-uniform kernels, zero biases and identity BatchNormalization (n == 0,
 * DNN.py:213,227).  The inference model of the context is untouched until csi_train_end(commit). */
int  csi_train_begin(csi_ctx* ctx, int model, const csi_train_config* cfg, const csi_tensor* tensors, int n);
/* x [B][len_ltf+nt] rows as Model.fit receives them (dataGenerator.py:299-316), y [B][n_out];
 * host buffers, synchronous when loss != NULL.  noise_std = 0 disables the AWGN layer. */
int  csi_train_step(csi_ctx* ctx, int model, const float* x, const float* y, int64_t B, float noise_std, float* loss);
/* Data-parallel form of a step: csi_train_backward computes the loss and every gradient of the
 * rank's batch without touching the parameters; csi_train_grads exposes all gradients as ONE
 * flat device buffer (regressor first, layer 0 last) for a single sum all-reduce (RCCL) that the
 * caller scales by 1/world; csi_train_apply runs Adam on whatever the buffer then holds.
 * csi_train_step == backward + apply.  BatchNormalization statistics stay per rank (keras
 * MirroredStrategy default). */
int  csi_train_backward(csi_ctx* ctx, int model, const float* x, const float* y, int64_t B, float noise_std, float* loss);
int  csi_train_grads(csi_ctx* ctx, int model, float** d_grads, int64_t* count);
int  csi_train_apply(csi_ctx* ctx, int model);
/* Resident training set (288 GB of HBM: the data stays on the device for the whole fit).  The
 * dataset is handed over once in the reference's own de-duplicated form
 * (create_massiveMIMO_CSIest_dnn_dataset.py:50-63): ltf_table [n_rows][len_ltf] = every rx preamble
 * of this component once, and per sample s its table row ltf_row[s], its tx index itx[s] (the
 * pilot columns are row itx[s] of csi_set_pilot's P) and its labels y[s][n_out].  A batch is then
 * B sample indices: csi_train_indexed(mode 0 = step, 1 = backward only, 2 = inference-mode loss)
 * gathers the rows on the device (AWGN applied on the fly) - no per-step host assembly or upload. */
int  csi_train_set_dataset(csi_ctx* ctx, int model, const float* ltf_table, int64_t n_rows, const int32_t* ltf_row,
                           const int32_t* itx, const float* y, int64_t N);
int  csi_train_indexed(csi_ctx* ctx, int model, int mode, const int32_t* ids, int64_t B, float noise_std, float* loss);
/* mse of the current parameters in inference mode (running statistics, no noise, no dropout):
 * the val_loss that EarlyStopping / ReduceLROnPlateau monitor (DNN.py:285-286). */
int  csi_train_eval(csi_ctx* ctx, int model, const float* x, const float* y, int64_t B, float* loss);
int  csi_train_set_lr(csi_ctx* ctx, int model, float lr);
/* Reads one tensor by its keras name (kernels as [in][out]); "grad:<name>" reads the gradient of
 * the last step (tests). */
int  csi_train_get(csi_ctx* ctx, int model, const char* name, float* out, int64_t count);
/* commit != 0: loads the trained tensors into the inference model (as csi_load_weights would,
 * pilot table included); then releases the trainer. */
int  csi_train_end(csi_ctx* ctx, int model, int commit);

int  csi_synchronize(csi_ctx* ctx);

/* Tuning / debug knobs (no reference counterpart).  name:
 *   "use_graph"        1: csi_predict_device replays a captured hipGraph when it is called again
 *                         with the same pointers and packet count (the reference's per-packet loop,
 *                         DNN.py:346, repeats one launch sequence); 0 (default): eager launches
 *   "force_tile"       128 | 256: row-tile height of every GEMM (0 = chosen by grid size)
 *   "xcd_order"        1 | 0: force the XCD super-tile / the linear tile order of the plain GEMMs
 *                         (-1 = automatic)
 *   "ls_fft_first_max" largest Nt served by the FFT-first LS kernel (default 15, max 64)
 *   "small_call_overlap" 1 (default): calls of at most 327 680 pair rows (2560 packets at Nt = 32, Nr = 4; 131 072 until round 6) run the real and the imag
 *                         model on two streams side by side - a mid-size call's kernels fill a fraction of the chip (24 ... 128 packets:
 *                         1.25-1.55x, 500 packets +1.4 %; device-pointer calls only: inside the host-buffer entry points' pipeline the
 *                         chunks stay on one stream, where the fork measured 6 % slower); 0: one after the other; 2: any size (A/B runs).
 *                         bf16 contexts: up to 262 144 pair rows.  "aux_fork_early" (default 1): csi_estimate_device forks the second
 *                         stream in front of its LS kernel - the imag model's chain needs the preambles, not the LS result (3 ... 32
 *                         packets 6 % faster); 0: behind it (A/B runs)
 *   "small_fused"      1 (default): a call of at most "small_rows" pair rows (default 1024 = 8 packets at Nt = 32, Nr = 4; and at most 64
 *                         rx preambles) - the reference's literal one-packet predict, DNN.py:339-346, and its small multiples - runs BOTH
 *                         component models in 1 + n_hidden launches: layer 0 as one weight-streaming kernel (up to 8 preambles) or on
 *                         fp32-MFMA tiles, every layer behind it as 16 x 16 / 32 x 32 fp32-MFMA tiles over the whole K, no split-K slabs
 *                         (csrc/small_call.hip.h); 0: the general kernels (A/B runs).  Read-only: "small_calls" (calls that took it).
 *                         "small_rows_band" (default 256 = 2 packets of that shape; calls of at most 8 preambles are not subject to it): the limit where the column-split band kernel serves
 *                         the model ("band_split": two hidden layers, 16 <= Nt <= 128, hidden[1] a multiple of 512) - from there
 *                         on the general path (weight-streaming layer 0 + that kernel) is the faster one
 *   "small_ls_fused"   1 (default): a csi_estimate_device call of at most 8 rx preambles runs its LS estimate INSIDE the layer-0 launch of the
 *                         one-packet path (csrc/small_call.hip.h: small_l0_ls_kernel - LS workgroups beside the weight-streaming ones;
 *                         Sylvester-ordered pilot, Nt = 16 / 32 / 64): one launch and 8 us less per call, same bits; 0: the LS kernel
 *                         in front (A/B runs).  Read-only: "small_ls_launches".
 *   "l0_stream"        1 (default): layer 0 of a call of 9 ... "l0_stream_max_rows" (default 1280) rx preambles runs on the weight-streaming split-f16 kernel
 *                         (csrc/l0_hs_stream.hip.h: every preamble row scaled by its own power of two, no range guard needed);
 *                         0: the general kernels.  "l0_stream_ks": its k ranges (0 = automatic); "l0_stream_prepass_rows": beyond
 *                         this many preambles (default 64) the row maxima come from their own small kernel.
 *                         Read-only: "l0_stream_launches"
 *   "f32_engine"       fp32 contexts: -1 (default) large GEMMs - at least half a round of 256x256 tiles - run on
 *                         the f16 matrix cores with split operands (x = hi + lo halves, three MFMA per
 *                         product, fp32 accumulation: the same 1e-5 contract at ~2.6x the fp32 MFMA rate,
 *                         gemm_hs.hip.h), small ones on the fp32 MFMA kernels - except that calls of 9 ... 1280 rx preambles run
 *                         layer 0 on the engine's weight-streaming kernel ("l0_stream") and models the column-split band kernel
 *                         serves ("band_split") run their per-pair layers on it at every size; 0: fp32 MFMA kernels only;
 *                         1: split engine wherever the layer shapes allow (hidden widths multiples of 16)
 *   "hs_blocked"       split engine: 1 (default) keeps the hidden activations between its layers in a blocked layout
 *                         ([16 rows][k-group of 16] = the 1 KiB one LDS-DMA piece of the next GEMM fetches, contiguous),
 *                         0 row-major (A-B)
 *   "hs_fuse_regressor" split engine, two hidden layers, n_out <= 256: 1 runs the regressor inside the first per-pair
 *                         layer's kernel (its 256 x 256 tile of activations becomes the A operand of a second product
 *                         on the CU; only partial sums reach memory).  0 (default): measured slower than two kernels
 *   "hs_min_blocks"    automatic mode: the per-pair layers take the split engine from this many 256x256 workgroups
 *                         on (default 48 = 24 packets of the shipped shape; 80 before the two-stream arrangement of round 5),
 *                         layer 0 from max(this, 128).  (Models the column-split band kernel serves take the split engine's
 *                         per-pair layers at every size - "band_split" - and are not subject to this threshold.)
 *   "hs_in_shift"      split engine: the preamble samples are carried times 2^shift.  99 (default): chosen per
 *                         launch on the device from a sampled maximum of the data, so that it lands at
 *                         2^13..2^14 (any input scaling is served); -8..14: fixed
 *   "hs_act_shift"     split engine: hidden activations are carried times 2^shift.  99 (default): per layer from
 *                         its BatchNormalization vectors at load (|beta| + 6 |gamma| lands at 2^10..2^11; 2^4
 *                         without BN); -8..14: fixed.  Operands that leave the f16 range at either end are
 *                         detected on the device: csi_predict repeats the call on the fp32 MFMA kernels by
 *                         itself, after device-pointer calls csi_synchronize returns CSI_ERR_RANGE
 *   "band_tail_split"  fp32 contexts, 1 (default, round 6): a one-stream call of more bands (128 pair rows) than compute units whose LAST round of band workgroups would
 *                      fill at most half (a quarter) of them launches that round in 2 (4) column splits; 0 = one launch.  "band_tail_launches" (get only)
 *                      counts the calls that did.
 *   "bf16_l0_fused_split" bf16 mode: 1 (default, round 6) runs layer 0 of calls between the weight-streaming kernel's range and 256 tiles
 *                      of the fused 256 x 256 kernel (321 ... 4095 packets at Nt = 64, Nr = 4) on that kernel with its K cut into ranges;
 *                      0 = a cast pass plus the 128 x 128 kernel, as before.
 *                      "bf16_l0_fused_split_launches" (get only) counts the layer-0 products that took that form.
 *   "bf16_fused_h1"    bf16 mode: 1 (default) generates the first per-pair activations inside the GEMM,
 *                         0 materialises them in HBM first (tests / A-B)
 *   "host_threads"     threads that copy between the caller's (pageable) buffers and the pinned
 *                         slots of the host-buffer entry points (0 = automatic: cores / 8, between 2 and 24)
 *   "ls_kernel"        0: automatic, 1: FFT-first (all Nt spectra in LDS, Nt <= 64), 2: chunked
 *                         FFT-first (16 <= Nt <= 128), 3: despread-first (any Nt), 4: Walsh-Hadamard
 *                         despread (Nt = 16 / 32 / 64 / 128 and P the Sylvester Hadamard matrix), 5: the same
 *                         fed by an LDS-DMA ring (chosen automatically for that P), 6: generic P on
 *                         the LDS-DMA ring, fp32 matrix-core despread, 7: generic P, despread on the bf16 matrix
 *                         cores with every fp32 value cut exactly into three bf16 pieces (one of the two is chosen
 *                         automatically for any other P, 16 <= Nt <= 128); a choice the kernel cannot serve falls back
 *   "ls_ringb_min"     the smallest Nt at which a non-Hadamard P takes kernel 7 (default 33; below, kernel 6 serves - DESIGN.md 4.2).
 *                         Kernel 7 runs ONE workgroup per CU at every Nt: a two-workgroups-per-CU form at Nt <= 32 is not built
 *                          and no option selects one
 *   get only: "ls_mode" (the kernel the next LS call runs), "ls_per_cu" (its resident workgroups per CU),
 *                         "ls_pilot_pieces" (bf16 pieces the entries of P need: 1 - 3)
 *   "ls_v2"            1: the runner-up shape (chunk length / ring depth) of kernels 5 and 6, for A/B runs
 *   "hs_band"          1 (default): two hidden layers -> first per-pair layer + regressor as ONE kernel, h2 in registers (generated
 *                         gfx950 assembly, csrc/band_kernel_gen.py): the split engine of fp32 contexts (the form that streams the
 *                         L0 / pilot-table values through LDS at 16 <= nt <= 128, per-lane loads elsewhere) and bf16 contexts at
 *                         32 <= nt <= 64 (streamed form); 0: the separate kernels (A/B runs); 2: bf16 contexts take the per-lane form
 *                         at any other nt as well (measured slower than the separate kernels); 3: only the per-lane forms (A/B runs).
 *                         Read-only: "band_launches".
 *   "band4"            1 (default): fp32 and bf16 contexts take the REGISTER-BLOCKED form of that kernel where its streamed form applies
 *                         (fp32: 16 <= nt <= 128, bf16: 32 <= nt <= 64) and the call runs unsplit or in 2 column splits
 *                         (csrc/band4_kernel_gen.py "csi_band4" / "csi_band4_bf16" and their "_cs" launches: 4 waves x 512 registers,
 *                         every weight fragment against two row groups, weights pre-tiled at first use); 4 column splits stay on the
 *                         8-wave form; 0: the 8-wave forms "csi_band8*" everywhere (A/B runs; same operand roundings, fp32 sums in
 *                         another order).  Read-only: "band4_available"; "band4_launches" counts the launches of a "csi_band4*" function
 *                         (a subset of "band_launches": which form served a call).
 *                         Routing of fp32 contexts: the split engine's band kernel takes the register-blocked form at 16 <= nt <= 128
 *                         when the call runs in ONE launch ("csi_band4") or in at most TWO column splits ("csi_band4_cs", also the tail
 *                         launch of "band_tail_split" when that is 2 splits); 4 splits and nt outside that range take "csi_band8*".
 *   "band_split"       -1 (default): a call with fewer bands of 128 pair rows than the part has CUs (24 ... 64 packets of the shipped
 *                         shape) splits every band's hidden features over 2 or 4 workgroups ("csi_band8_cs") and adds their regressor
 *                         sums in split order - same arithmetic, the final fp32 sums associate differently (1 ulp class);
 *                         0 / 1: never; 2 / 4: always (A/B runs, tests).  Read-only: "band_split_launches".
 *   "hs_vm_cast", "hs_vm_pair"  vector-memory schedule of the split-f16 layer-0 / first per-pair kernel: 0 builtin LDS-DMA
 *                         with one drain per sub-tile, 1 hand-counted waits, 2 + one more sub-tile of look-ahead (default for
 *                         layer 0), 3 + one load and one 24-MFMA segment per sub-tile (default for the pair layer); same
 *                         results bit for bit, for A/B runs (tools/vm_ab.sh)
 *   "hs_l0_mfma"       MFMA shape of the split-f16 layer-0 kernel's main loop: 32 = v_mfma_f32_32x32x16_f16, three products per
 *                         sub-tile of 16 k-columns; 16 (default) = v_mfma_f32_16x16x32_f16 on pairs of sub-tiles (same terms and matrix-pipe
 *                         cycles, the part holds a higher clock on it: profiles/mfma_shape_probe.txt, profiles/l0_mfma16_ab.txt).
 *                         16 is taken with "hs_vm_cast" = 2 when every k range of the launch holds an even number of sub-tiles
 *                         (every FC model), anything else runs the 32 form.  Same terms, the fp32 sums associate differently
 *                         (parts in 1e-7).  Read-only: "hs_l0_mfma16_launches" counts the launches of the 16 form.
 *   "ls_fast_perm"     1 (default): a pilot matrix that is a signed row / column permutation of the Sylvester Hadamard matrix
 *                         takes the Walsh-Hadamard LS kernel through permutation tables; 0: the generic kernels (A/B runs)
 *   "ls_overlap_cus"   always 0.  It ran the LS kernel of csi_estimate_device on a side stream masked to this many CUs beside the DNN
 *                         kernels: an experiment that measured slower than the serial order and was removed.
 *                         Setting 0 succeeds, anything else is refused (CSI_ERR_INVALID_ARG with text)
 *   "hp_side_threads"  host-buffer entry points: 1 (default) input staging and result staging on their own threads beside the
 *                         caller's enqueue loop; 0: inline on the calling thread, in turn (A/B runs)
 *   "hp_chunk_packets" packets per pipeline slot of csi_estimate_c128 (0 = automatic)
 *   "hp_device_weave"  1 (default): csi_estimate_c128 with pinned result arrays assembles the complex64 values on the device
 *   "train_rank"       0 (default) .. 2^20 - 1: rank of this process in a data-parallel fit.  The trainers fold it into the noise and
 *                         dropout streams (not into the Glorot initialisation), so every rank draws its own noise and masks for its
 *                         shard of the global batch; rank 0 has the streams of a single process.  Takes effect at the next step.
 *   "ls_debug"         development switches of the LS kernels (skip phases for timing: tools/ls_probe.py); write-only, 0 in production */
int  csi_set_option(csi_ctx* ctx, const char* name, int64_t value);
/* Current value of an option, or of the read-only values: "hs_launches" (split-engine GEMMs launched), "hs_range_fallbacks"
 * (csi_predict calls repeated on the fp32 MFMA kernels), "hs_weight_pins" / "hs_weight_err_e12" (layers pinned to the fp32 kernels
 * at load because their split copies were not fp32-grade; worst relative error x 1e12), "band_available" (the assembly band kernel
 * is embedded in this build), "graph_replays", "subspace_launches" (kernels launched by csi_subspace_smooth[_device]), "beam_launches" (kernels launched by the csi_beam_* entry points), "mu_launches" (kernels launched by csi_mu_precoder_device / csi_mu_link_sim_device / csi_mu_hybrid_precoder_device / csi_mu_covariance_device / csi_mu_jsdm_precoder_device), "feedback_launches" (kernels launched by csi_feedback_compress_device / csi_feedback_expand_device), "lmmse_blind_fallbacks" ((packet, rx) pairs csi_lmmse_blind[_device] handed back unsmoothed), "ls_pilot_fast" (0 generic / 1 Sylvester / 2 permuted pilot), "comm_world",
 * "comm_rank", "comm_blobs", "comm_bytes" (communicator and last broadcast), "hp_direct_out_calls", and where the last pipelined
 * host-buffer call spent its time in microseconds: "hp_total_us", "hp_stage_us", "hp_wait_stage_us", "hp_wait_out_us", "hp_weave_us". */
int  csi_get_option(csi_ctx* ctx, const char* name, int64_t* value);

/* Device-memory plumbing so that a host program needs no other GPU runtime. */
int  csi_device_malloc(csi_ctx* ctx, void** dptr, int64_t bytes);
int  csi_device_free(csi_ctx* ctx, void* dptr);
/* Pinned (page-locked) host memory: buffers from here are DMA'd directly by the host-buffer entry
 * points instead of being staged through the library's own pinned slots. */
int  csi_host_malloc(csi_ctx* ctx, void** ptr, int64_t bytes);
int  csi_host_free(csi_ctx* ctx, void* ptr);          /* ctx may be NULL (a buffer that outlived its context) */
int  csi_memcpy_h2d(csi_ctx* ctx, void* dst_dev, const void* src_host, int64_t bytes);
int  csi_memcpy_d2h(csi_ctx* ctx, void* dst_host, const void* src_dev, int64_t bytes);
/* i.i.d. CN(0,1) preambles generated on the device by a counter-based RNG (element index
 * -> value), for workloads too large to stage through the host (SURVEY.md 8d 'white'). */
int  csi_synth_white(csi_ctx* ctx, uint64_t seed, int64_t first_pkt, int64_t npkt,
                     float* d_ltf_re, float* d_ltf_im);
/* Sounding packets with a KNOWN channel, generated on the device (the synthetic twin of generate_maMIMO_LTF.m:197-342 and the inverse
 * of the LS estimate; csrc/synth_structured.hip.h).  Per (packet, rx): every tx link draws an n_taps complex Gaussian impulse response
 * with the decay exp(-0.5 t) / sqrt(2); H is its 256-point DFT; the frequency-domain LTF symbols are X[s][k] = ltf[k] sum_j H[j][k] P[j][s]
 * on all 242 non-null bins, with P the matrix of csi_set_pilot (any real Nt x Nt matrix); then the 256-point inverse FFT, the 64-sample
 * cyclic prefix and complex AWGN.
 *   snr_db       HOST array [npkt], dB, relative to the packet's OWN power = the mean of |x|^2 over its nr * len_ltf complex samples
 *                (generate_maMIMO_LTF.m:283-295); NULL = noise-free.  It is read before the call returns.
 *   n_taps       1 .. 64; 0 selects 8
 *   flags        bit 0: the sqrt(242) / 256 amplitude scale of :303-304 on signal and noise; other bits must be 0
 *   d_ltf_re/im  [npkt][nr][len_ltf], what csi_estimate_device / csi_ls_estimate_device read
 *   d_h_re/im    optional (both or neither): the true channel [npkt][nr][nt][234] in the layout and bin order of the LS output, DEFINED as
 *                what csi_ls_estimate_device returns for the noise-free packet whenever P P^T = Nt I (so it carries the amplitude scale)
 *   d_noise_std  optional [npkt]: sqrt(power / 10^(snr/10) / 2), the noise deviation per real component BEFORE the amplitude scale
 *                (0 for a noise-free call)
 * Draws are counter-based, keyed by (seed, absolute packet index first_pkt + i, position inside the packet): packets [first, first + n)
 * are the same bits whichever call produces them and whatever the call size, noise never moves the channel draws, and the packet power
 * is summed in a fixed order, so a call repeats bit for bit.  All arithmetic is fp32; serves fp32 and bf16 contexts alike (the planes are
 * fp32 either way).  Asynchronous on the context's stream.  Output planes must start on 16-byte boundaries (csi_device_malloc does).
 * Refused with text: no pilot set, negative npkt / first_pkt, n_taps outside 1 .. 64, unknown flag bits, null ltf planes with
 * npkt > 0, one channel plane without the other, misaligned planes, a context without antennas (nt = 0), a call with an SNR array
 * inside csi_capture_begin / _end.  Profile entry "synth_structured". */
int  csi_synth_structured(csi_ctx* ctx, uint64_t seed, int64_t first_pkt, int64_t npkt, const float* snr_db, int n_taps, uint32_t flags,
                          float* d_ltf_re, float* d_ltf_im, float* d_h_re, float* d_h_im, float* d_noise_std);

/* The same packets from a geometric single-bounce scattering channel: what phased.ScatteringMIMOChannel models in the reference
 * (helperApplyMUChannel.m:44-143; csrc/synth_scattering.hip.h).  The toolbox object is not part of the reference tree, so
 * its random stream and sign conventions cannot be pinned; the model is restated from the physics.  A zero in a field of the
 * configuration selects its default (an azimuth of exactly 0 is written 360). */
typedef struct {
    int32_t  n_scat;           /* scatterers S, 1 .. 256; default 100 (N_chan_taps, generate_maMIMO_LTF.m:9) */
    uint32_t flags;            /* bit 0: the sqrt(242) / 256 amplitude scale, as in csi_synth_structured; bit 1: the user position is drawn
                                  per packet; other bits must be 0 */
    float    range_m;          /* distance R transmitter - receiver, default 100 (with bit 1: the upper end of the draw) */
    float    az_deg, el_deg;   /* direction of the user seen from the transmitter, default 30 and 0; |el| <= 90 */
    float    box_frac;         /* half edge of the scatterer box around the receiver in units of R, default 0.1 (helperApplyMUChannel.m:90) */
    float    sample_rate_hz;   /* default 100e6 (:89) */
} csi_scatter_config;
/* Per packet p = first_pkt + i (absolute index) the channel stream kc = key(seed, p, 0) of csi_synth_structured is read as follows
 * (tr_uniform / tr_normal of csrc/rng.hip.h; no tap is drawn in this mode):
 *   user        flag bit 1: u0..u2 = uniform(kc, 0..2), R = 1 + (range_m - 1) u0, az = 180 (2 u1 - 1), el = 90 (2 u2 - 1) degrees
 *               (generate_maMIMO_LTF.m:48-51); otherwise R, az, el as configured.  e = (cos el cos az, cos el sin az, sin el)
 *   scatterer s base index b = 8 (s + 1): offset from the receiver o_s[i] = box_frac R (2 uniform(kc, b + i) - 1), i = 0, 1, 2;
 *               reflection coefficient g_s = (normal(kc, b + 3) + i normal(kc, b + 4)) / sqrt(2).  The carrier phase 2 pi fc tau is
 *               absorbed in g_s (uniform for positions random at the scale of metres), so fc does not enter.
 *   geometry    q_s = R e + o_s;  excess path x_s = (2 R (e . o_s) + |o_s|^2) / (|q_s| + R) + |o_s| (= |q_s| - R + |o_s|, without the
 *               cancellation);  excess delay tau_s = (x_s - min_s' x_s') fs / c samples, c = 299792458: the first path sits at delay 0
 *               (the reference removes floor(min tau) samples);  direction cosines along the array axis y: v_s = q_s,y / |q_s| at the
 *               transmitter, w_s = o_s,y / |o_s| at the receiver (0 for a zero offset)
 *   arrays      ULAs along y at half a wavelength: y_j = (j - (Nt - 1) / 2) / 2, z_r = (r - (Nr - 1) / 2) / 2 (URAs are out of scope)
 *   response    H[r][j][f] = S^(-1/2) sum_s g_s exp(2 pi i z_r w_s) exp(-2 pi i y_j v_s) exp(-2 pi i f tau_s / 256),  f the SIGNED bin
 *               index -128 .. 127 (FFT bins 128 .. 255 are f - 256; the delays are fractional).  The transmit factor is the conjugate
 *               of synth.steering_ula: the dominant right singular vector of a one-scatterer H is steering_ula at its direction.
 *               E|H|^2 = 1.
 * Everything behind H is csi_synth_structured's: the LTF symbols on the 242 non-null bins mapped by P, the inverse transform, the
 * prefix, the amplitude scale, noise relative to the packet's own power from key(p, 1) at the same indices, h = amp H on the 234 data
 * bins DEFINED as what csi_ls_estimate_device returns for the noise-free packet when P P^T = Nt I.  Packets [first, first + n) are the
 * same bits whichever call holds them, a noisy call leaves the channel bits of the noise-free call unchanged, and a call repeats bit
 * for bit.  The configuration is fp32, the per-scatterer geometry is evaluated in fp64 and rounded once, all per-bin arithmetic is fp32.
 *   snr_db, d_ltf_re/im, d_h_re/im, d_noise_std   as in csi_synth_structured
 *   cfg          NULL = all defaults
 *   d_tau        optional [npkt][S]: (R + x_s) fs / c, the absolute path delays in samples - the TAU the reference hands LMMSE_ce
 *                (generate_maMIMO_LTF.m:342)
 * Asynchronous on the context's stream; serves fp32 and bf16 contexts alike.  Refused with text: everything csi_synth_structured
 * refuses, S outside 1 .. 256, a non-finite or non-positive range, box fraction or sample rate, a non-finite azimuth, |el| > 90, unknown
 * flag bits, a call with an SNR array inside csi_capture_begin / _end.  A null context returns -1.  Profile entry "synth_scattering";
 * "scatter_launches" (csi_get_option) counts the kernels launched. */
int  csi_synth_scattering(csi_ctx* ctx, uint64_t seed, int64_t first_pkt, int64_t npkt, const float* snr_db, const csi_scatter_config* cfg,
                          float* d_ltf_re, float* d_ltf_im, float* d_h_re, float* d_h_im, float* d_noise_std, float* d_tau);

/* Channel aging: the true channel of csi_synth_scattering's packets at other times, for a user that moves
 * (csrc/scatter_aged.hip.h).  No reference counterpart: the reference's channel sets 'MaximumDopplerShift',0. */
typedef struct {
    float    speed_mps;                      /* >= 0; 0: a static user, every time returns the planes of csi_synth_scattering */
    float    heading_az_deg, heading_el_deg; /* literal values, no default substitution; |el| <= 90 */
    float    carrier_hz;                     /* 0 selects 28e9 (prm.fc) */
    uint32_t flags;                          /* bit 0: heading azimuth drawn per packet; other bits must be 0 */
} csi_motion_config;
/* Packet p = first_pkt + i of stream `seed` has the scatterers, coefficients g_s, delays tau_s and direction cosines v_s, w_s of
 * csi_synth_scattering: the same draws of kc = key(seed, p, 0), nothing moved.  The transmitter and the scatterers stand still; the user
 * moves with speed_mps along the unit vector m = (cos el cos az, cos el sin az, sin el) of heading_az_deg / heading_el_deg in the
 * transmitter's frame, the frame of az_deg / el_deg.  Only the last leg of path s changes: with o_s the scatterer's offset from the
 * receiver it shortens at speed_mps (m . o_s) / |o_s| metres per second, so
 *   nu_s = speed_mps carrier_hz / c  (m . o_s) / |o_s|      Hz; 0 for a zero offset; c = 299792458
 *   H_t[r][j][f] = S^(-1/2) sum_s g_s exp(+2 pi i nu_s t) exp(2 pi i z_r w_s) exp(-2 pi i y_j v_s) exp(-2 pi i f tau_s / 256)
 *   h_t = amp H_t on the 234 data bins in the LS layout, as in csi_synth_scattering; h_0 IS what that call returns, bit for bit, and
 *   so is every h_t of a static user.
 * The model is FIRST ORDER: delays and direction cosines are frozen at their t = 0 values.  That is good while speed_mps |t| is small
 * against the scatterer box box_frac R - millimetres against metres for walking speed and milliseconds; nothing is refused on it.
 * Random heading (flag bit 0): the azimuth of m is drawn per packet as 180 (2 uniform(kc, 3) - 1) degrees - index 3 of the channel
 * stream is otherwise unused (the user takes 0 .. 2, scatterer s starts at 8 (s + 1)), so no existing draw moves - and the elevation
 * stays as configured.
 * Precision: nu_s and the product nu_s t are evaluated in fp64 by scatterer s's lane, next to the fp64 geometry; the turn count is
 * reduced in fp64 (x - rint(x)) and rounded once to fp32 for sincospif; c_s is multiplied by that phasor in fp32; everything behind
 * it is csi_synth_scattering's fp32 arithmetic in its order.  At t = 0 or speed 0 the phasor is exactly (1, 0).
 *   cfg          as in csi_synth_scattering, defaults included (sample_rate_hz, n_scat, flag bits 0 and 1 act as there); NULL = all defaults
 *   motion       NULL = a static user
 *   t_s          HOST array of n_times seconds, 1 <= n_times <= 16, any sign and any order; it is read before the call returns and
 *                travels to the kernel as kernel arguments, not as an upload
 *   d_h_re/im    [n_times][npkt][nr][nt][234], 16-byte aligned: slice t is a plane pair that every consumer of CSI planes takes as it is
 * No pilot matrix is needed: no LTF is made.  One launch per call, asynchronous on the context's stream; it may be captured between
 * csi_capture_begin and csi_capture_end.  Serves fp32 and bf16 contexts alike.  Refused with text: everything csi_synth_scattering
 * refuses about the context, cfg, npkt, first_pkt, alignment and LDS size; n_times outside 1 .. 16, a null t_s, a non-finite time, a
 * negative or non-finite speed, a non-finite heading azimuth, |heading_el_deg| > 90, a negative or non-finite carrier, unknown motion
 * flag bits, null planes with npkt > 0, npkt * nr beyond one launch.  npkt == 0 writes nothing.  A null context returns -1.  Profile
 * entry "scatter_aged"; "scatter_aged_launches" (csi_get_option) counts its kernels ("scatter_launches" does not move). */
int  csi_scatter_channel_at_device(csi_ctx* ctx, uint64_t seed, int64_t first_pkt, int64_t npkt, const csi_scatter_config* cfg,
                                   const csi_motion_config* motion, const double* t_s, int n_times, float* d_h_re, float* d_h_im);

/* Channel forecasting: a linear predictor over several soundings (csrc/forecast.hip.h).  No reference counterpart (the
 * reference's channel does not move); it is what a transmitter does about the ageing csi_scatter_channel_at_device shows.
 * The soundings x_0 .. x_{n_snd-1} run oldest to newest and are equally spaced; each is a CSI plane pair [npkt][nr][nt][234].  They
 * arrive as HOST arrays of n_snd device pointers (the convention of csi_mu_precoder_device).  With P = n_snd, order M, horizon
 * d = steps (in sounding intervals), 2 <= P <= 16, 1 <= M <= 8, d >= 1, M + d <= P, per (packet, rx):
 *   T[i][q]  = sum_j sum_k conj(x_i[j][k]) x_q[j][k]                 P x P, Hermitian to the bit       csi_forecast_gram_device
 *   G[a][b]  = sum_{p = M+d-1}^{P-1} T[p-d-a][p-d-b]                 M x M
 *   rhs[a]   = sum_{p = M+d-1}^{P-1} T[p-d-a][p]
 *   (G + ridge trace(G) / M I) c = rhs                               fp64 Cholesky, c rounded to fp32  csi_forecast_fit_device
 *   y[j][k]  = sum_{m < M} c_m x_{P-1-m}[j][k]                       the forecast of x at index P-1+d  csi_forecast_apply_device
 * flags bit 0 (pooling): G, rhs and the target energy of a packet's receive antennas are added in ascending rx order before the solve;
 * every rx of the packet gets the same c, fit_err and info.  Other bits must be 0.
 * Fallback: a pivot <= 0 or not finite (all-zero planes included) gives c = (1, 0, .., 0) - the newest sounding is held - and info 1
 * (0 otherwise).  fit_err = max(0, 1 - Re(c^H rhs) / sum_{p = M+d-1}^{P-1} T[p][p]) with the fp64 c, the in-sample relative residual
 * (0 where that energy is not positive).  ridge is taken literally (0 is 0; the Python default is 1e-5): without it the noise-free
 * system of a smooth channel has a condition number near 1e7.
 * Arithmetic: T on the fp32 matrix cores (three v_mfma_f32_16x16x4_f32 products per four floats, re = RR + II, im = RI - RI^T), the
 * order of every sum fixed by (nt, P) alone, no atomics: a (packet, rx) has the same bits whatever the call size or its position.
 * The fit in fp64 from the fp32 T.  The apply pass in fp32, complex FMAs in the order m = 0 .. M-1.
 *   d_t_re/im    [npkt][nr][P][P], 16-byte aligned
 *   d_c_re/im    [npkt][nr][M]
 *   d_fit_err    float [npkt][nr] or NULL;  d_info  int32 [npkt][nr] or NULL
 *   d_out_re/im  a plane pair like a sounding, 16-byte aligned
 * csi_forecast_gram_blocks_device is the Gram kernel on its own terms: n_blocks blocks of block_floats contiguous floats per plane
 * (even, >= 2: a block starts on an 8-byte boundary; the kernel assumes nothing wider), T [n_blocks][P][P]; csi_forecast_gram_device
 * is the case (npkt nr, 234 nt) of it.
 * csi_forecast_device runs the three in sequence - the same bits as the three calls made by hand; T and, when d_c_re / d_c_im are
 * NULL, c live in a context workspace sized by eager calls: inside a capture (csi_capture_begin) the workspace must already hold the
 * call, so an eager call of the same shape goes first.  csi_forecast: the same on host buffers (x_re / x_im: host arrays of n_snd host
 * pointers), in packet chunks of 256 MiB of staging (the context's workspace_bytes when that is smaller); same bits as the device entry; its host arrays obey the overlap rule of
 * the device entries (no output array may share a byte with a sounding or with another output).
 * csi_sounding_noise_device gives a simulated history its estimation error: out = x + s (n_re + i n_im), s = sqrtf(0.5f v[p][r]),
 * n_re / n_im = normal(kn, 2 e) / normal(kn, 2 e + 1), kn the noise key of packet first_pkt + p of stream `seed` (kind 1 of
 * csi_synth_structured), e = (r nt + j) 234 + k; one fused multiply-add per component.  d_err_var float [npkt][nr].  out may be x
 * itself (re with re, im with im); a zero v returns the input bits.
 * Every entry is asynchronous on the context's stream and may be captured.  Refused with text, before any launch: n_snd, order, steps
 * outside the ranges above, a negative npkt (or first_pkt), npkt * nr beyond one launch, a non-finite or negative ridge, unknown flag
 * bits, null required pointers, planes off a 16-byte boundary, an output that overlaps an input or another output (the noise entry's
 * in-place case excepted), a single-input context.  npkt == 0 launches nothing.  A null context returns -1.  Profile entries
 * "forecast_gram" (1536 flop per float of a block; 8 P K + 8 P^2 bytes per block, K = 234 nt), "forecast_fit", "forecast_apply"
 * (8 M flop and 8 (M + 1) bytes per float) and "sounding_noise"; read-only option "forecast_launches" counts their kernels. */
int  csi_forecast_gram_device(csi_ctx* ctx, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t npkt, float* d_t_re, float* d_t_im);
int  csi_forecast_gram_blocks_device(csi_ctx* ctx, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t n_blocks,
                                     int64_t block_floats, float* d_t_re, float* d_t_im);
int  csi_forecast_fit_device(csi_ctx* ctx, const float* d_t_re, const float* d_t_im, int n_snd, int64_t npkt, int order, int steps, double ridge,
                             uint32_t flags, float* d_c_re, float* d_c_im, float* d_fit_err, int32_t* d_info);
int  csi_forecast_apply_device(csi_ctx* ctx, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t npkt, int order,
                               const float* d_c_re, const float* d_c_im, float* d_out_re, float* d_out_im);
int  csi_forecast_device(csi_ctx* ctx, const float* const* d_x_re, const float* const* d_x_im, int n_snd, int64_t npkt, int order, int steps,
                         double ridge, uint32_t flags, float* d_out_re, float* d_out_im, float* d_c_re, float* d_c_im, float* d_fit_err, int32_t* d_info);
int  csi_forecast(csi_ctx* ctx, const float* const* x_re, const float* const* x_im, int n_snd, int64_t npkt, int order, int steps, double ridge,
                  uint32_t flags, float* out_re, float* out_im, float* c_re, float* c_im, float* fit_err, int32_t* info);
int  csi_sounding_noise_device(csi_ctx* ctx, uint64_t seed, int64_t first_pkt, int64_t npkt, const float* d_err_var, const float* d_x_re,
                               const float* d_x_im, float* d_out_re, float* d_out_im);

/* Carrier frequency offset of the sounding preamble: cyclic-prefix estimator and corrector (csrc/cfo.hip.h).  No
 * reference counterpart (the reference's receiver sits exactly on the transmitter's carrier); it is the synchronisation stage in front of
 * csi_ls_estimate_device / csi_estimate_device / csi_lmmse_blind_device, and the impairment that tests it.
 * x[p][r][n] are the preamble planes [npkt][Nr][320 Nt], n = 320 s + m (64 samples of cyclic prefix, 256 of body per symbol); eps is in
 * subcarrier spacings (cycles per 256 samples), one per packet, shared by its Nr antennas.
 *   y[p][r][n] = x[p][r][n] exp(2 pi i scale eps[p] n / 256)              scale +1 impairs, -1 corrects    csi_cfo_rotate_device
 *   gamma[p]   = sum_r sum_s sum_{m = cp_skip}^{63} conj(x[p][r][320 s + m]) x[p][r][320 s + m + 256]
 *   E[p]       = 1/2 sum (|x[.. m]|^2 + |x[.. m + 256]|^2) over the same samples
 *   eps_hat[p] = atan2(Im gamma, Re gamma) / 2 pi,  quality[p] = |gamma| / E  (about snr / (1 + snr));
 *   E == 0 gives eps_hat = 0 and quality = 0                                                               csi_cfo_estimate_device
 * cp_skip (0 .. 63) leaves out the head of every prefix, which a real capture loses to the previous symbol's echo.  The phase counts
 * from sample 0 of the packet: a corrected packet carries no residual common phase.  The estimate is unambiguous for |eps| < 0.5.
 * Arithmetic: the estimator reads only [cp_skip, 64) and [256 + cp_skip, 320) of every symbol; products in fp32, every sum in fp64 in an
 * order fixed by (Nt, Nr, cp_skip) alone, no atomics, one fp64 atan2 per packet: a packet has the same bits whatever the call size or
 * its position.  The rotation forms the turn count scale eps n / 256 in fp64, reduces it to [-1/2, 1/2] in fp64 and only then takes an
 * fp32 sine and cosine; scale eps[p] == 0 returns the input bits.  out may be in itself (re with re, im with im).
 *   d_eps      double [npkt], 8-byte aligned;  d_quality  float [npkt] or NULL
 * csi_cfo_correct_device is the estimate followed by the rotation with scale -1, two launches, the bits of the two calls made by hand;
 * d_eps may be NULL, then eps lives in a context workspace sized by eager calls (inside a capture an eager call of the same shape goes
 * first).  csi_cfo_correct: the same on host buffers in packet chunks of 256 MiB of staging (the context's workspace_bytes when that is
 * smaller), eps and quality optional; same bits as the device entry.
 * Every device entry is asynchronous on the context's stream and may be captured.  Refused with text, before any launch: null planes,
 * npkt < 1, cp_skip outside 0 .. 63, planes off a 16-byte boundary, planes that overlap partially (an output plane that is not its own
 * input plane but shares a byte with a plane), d_eps / d_quality that share a byte with a plane, a non-finite scale, a single-input
 * context.  A null context returns -1.  Profile entries "cfo_corr" (16 bytes per correlated pair of samples) and "cfo_rotate" (16 bytes
 * per sample); read-only option "cfo_launches" counts their kernels. */
int  csi_cfo_estimate_device(csi_ctx* ctx, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt, int cp_skip, double* d_eps, float* d_quality);
int  csi_cfo_rotate_device(csi_ctx* ctx, const float* d_in_re, const float* d_in_im, int64_t npkt, const double* d_eps, double scale,
                           float* d_out_re, float* d_out_im);
int  csi_cfo_correct_device(csi_ctx* ctx, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt, int cp_skip, float* d_out_re, float* d_out_im,
                            double* d_eps, float* d_quality);
int  csi_cfo_correct(csi_ctx* ctx, const float* ltf_re, const float* ltf_im, int64_t npkt, int cp_skip, float* out_re, float* out_im, double* eps,
                     float* quality);

/* Symbol timing of the sounding preamble: cyclic-prefix timing estimator, joint with the carrier frequency offset (csrc/sync.hip.h,
 * DESIGN.md 4.29).  No reference counterpart (the reference's receiver is handed the packet from its first sample); it is the stage in
 * front of csi_cfo_* and of every estimator, and the impairment that tests it.
 * c[p][r][n] are CAPTURE planes [npkt][Nr][L], L = 320 Nt + span; span is a multiple of 4 in 4 .. 256, so every row starts on a 16-byte
 * boundary.  The packet of len = 320 Nt samples starts at theta[p] in 0 .. span, one per packet, shared by its Nr antennas.  A span of
 * 320 would be ambiguous by a whole symbol; the metric takes no cp_skip, which would make every start in [theta - cp_skip, theta] an
 * exact tie (a caller who wants one runs csi_cfo_estimate_device on the cut-out planes).  For theta = 0 .. span:
 *   gamma(theta)  = sum_r sum_s sum_{m<64} conj(c[p][r][theta + 320 s + m]) c[p][r][theta + 320 s + m + 256]
 *   Phi(theta)    = 1/2 sum (|c[.. m]|^2 + |c[.. m + 256]|^2) over the same samples
 *   Lambda(theta) = |gamma(theta)| - rho Phi(theta)        rho in [0, 1]; 1 is the high-SNR form (van de Beek's rho = snr / (1 + snr))
 *   theta_hat = the lowest theta of the largest Lambda,  eps_hat = atan2(Im, Re of gamma(theta_hat)) / 2 pi,
 *   quality = |gamma(theta_hat)| / Phi(theta_hat);  Phi == 0 there gives eps_hat = 0 and quality = 0; an all-zero capture (0, 0, 0)
 *                                                                                                          csi_sync_estimate_device
 *   y[p][r][n] = c[p][r][theta[p] + n] exp(-2 pi i eps[p] n / 256), n < len; without d_eps, or with eps[p] == 0, a copy of the bits;
 *   the phase counts from the packet's own sample 0 and the bits are those of a plain cut-out followed by
 *   csi_cfo_rotate_device(scale = -1)                                                                      csi_sync_extract_device
 *   c[p][r][theta[p] + n] = x[p][r][n] (the packet's bits); every other sample is the margin
 *   std[p] (normal(km, 2 e) + i normal(km, 2 e + 1)), e = r L + n, km = splitmix64(kn ^ 0x53594E43), kn the noise key of packet
 *   first_pkt + p of csi_synth_structured's streams; d_margin_std NULL or std[p] == 0 gives zero margins.  std is the deviation per
 *   real component as applied (csi_synth_*'s noise_std times the amplitude scale where flag bit 0 was set)   csi_sync_embed_device
 * A theta outside 0 .. span in a device array cannot be refused before the launch: embed and extract clamp it into the range, so
 * nothing outside the arrays is ever touched.
 * Arithmetic of the estimator: products in fp32 as in csi_cfo_estimate_device, every sum in fp64 in an order fixed by (Nt, Nr, span)
 * alone, no atomics: a packet has the same bits whatever the call size or its position.
 *   d_theta    int32 [npkt];  d_eps  double [npkt], 8-byte aligned;  d_quality  float [npkt];  d_metric  double [npkt][span + 1], the
 *   values of Lambda the argmax compared.  d_eps, d_quality and d_metric of the estimate are optional (NULL).
 * csi_sync_correct_device is the estimate followed by the cut-out at theta_hat - with bit 0 of flags also removing eps_hat - two
 * launches, the bits of the two calls made by hand; d_theta / d_eps / d_quality are optional, theta and eps then live in a context
 * workspace sized by eager calls (inside a capture an eager call of the same shape goes first).  csi_sync_correct: the same on host
 * buffers in packet chunks of 256 MiB of staging (the context's workspace_bytes when that is smaller), theta, eps and quality optional;
 * same bits as the device entry.
 * Every device entry is asynchronous on the context's stream and may be captured.  Refused with text, before any launch: null planes,
 * npkt < 1, a span that is no multiple of 4 in 4 .. 256, rho non-finite or outside [0, 1], unknown flag bits, planes off a 16-byte
 * boundary, an output that shares a byte with an input or with another output (the cut-out is never in place), per-packet arrays off
 * their word size, a single-input context.  A null context returns -1.  Profile entries "sync_metric" (16 bytes per folded pair of
 * samples), "sync_extract" (16 bytes per sample of the packet) and "sync_embed" (8 bytes per sample in and out); read-only option
 * "sync_launches" counts their kernels. */
int  csi_sync_embed_device(csi_ctx* ctx, uint64_t seed, int64_t first_pkt, int64_t npkt, int span, const int32_t* d_theta, const float* d_margin_std,
                           const float* d_x_re, const float* d_x_im, float* d_cap_re, float* d_cap_im);
int  csi_sync_estimate_device(csi_ctx* ctx, const float* d_cap_re, const float* d_cap_im, int64_t npkt, int span, double rho, int32_t* d_theta,
                              double* d_eps, float* d_quality, double* d_metric);
int  csi_sync_extract_device(csi_ctx* ctx, const float* d_cap_re, const float* d_cap_im, int64_t npkt, int span, const int32_t* d_theta,
                             const double* d_eps, float* d_out_re, float* d_out_im);
int  csi_sync_correct_device(csi_ctx* ctx, const float* d_cap_re, const float* d_cap_im, int64_t npkt, int span, double rho, uint32_t flags,
                             float* d_out_re, float* d_out_im, int32_t* d_theta, double* d_eps, float* d_quality);
int  csi_sync_correct(csi_ctx* ctx, const float* cap_re, const float* cap_im, int64_t npkt, int span, double rho, uint32_t flags, float* out_re,
                      float* out_im, int32_t* theta, double* eps, float* quality);

/* ---- multi-GPU: packets shard over the GPUs of a node (one process and one context per GPU), the weights are shared and
 * read-only, outputs stay sharded.  The single collective of the path is the load-time broadcast of the
 * weights, here inside the library on RCCL (ncclBroadcast over xGMI), device to device on the context's stream.  The
 * reference has no multi-device code; this replaces what `Model.load_weights` (DNN.py:334) would otherwise do once per GPU.
 * RCCL (librccl.so.1) is dlopen'ed by csi_comm_init; nothing else in the library needs it.
 *
 *   rank 0:      csi_get_unique_id(id);  -> hand the 128 bytes to the other ranks (file, environment, socket, MPI ...)
 *   every rank:  csi_create(...);  csi_comm_init(ctx, rank, world, id);
 *   rank root:   csi_load_weights(ctx, 0, ...);  csi_load_weights(ctx, 1, ...);  csi_set_pilot(ctx, P);
 *   every rank:  csi_broadcast_weights(ctx, root);      -> every context is loaded; no host copy of the weights elsewhere
 *   every rank:  csi_predict[_device] / csi_ls_estimate[_device] on its own packet range  */
#define CSI_UNIQUE_ID_BYTES 128
int  csi_get_unique_id(char id[CSI_UNIQUE_ID_BYTES]);            /* ncclGetUniqueId; errors: csi_last_error(NULL) */
int  csi_comm_init(csi_ctx* ctx, int rank, int world, const char id[CSI_UNIQUE_ID_BYTES]);   /* ncclCommInitRank on the context's device (collective) */
int  csi_comm_destroy(csi_ctx* ctx);
/* Both component models and the pilot matrix as csi_load_weights / csi_set_pilot left them on `root`: the re-laid-out fp32
 * matrices, their split-f16 / bf16 forms, bias and BatchNormalization vectors, P - ncclBroadcast of the device buffers
 * themselves, then the pilot tables are rebuilt locally.  Collective; synchronous at return.  Contexts must share one csi_config
 * (shape and dtype): every rank checks the root's record against its own, the ranks agree on the outcome (one ncclAllReduce of a
 * status word) BEFORE the buffers move, and if any rank refuses, every rank returns an error (the refusing one with the reason)
 * instead of waiting inside the broadcast; a receiver that failed holds no model and no pilot afterwards.
 * "comm_bytes" / "comm_blobs" (csi_get_option) report what the last call moved. */
int  csi_broadcast_weights(csi_ctx* ctx, int root);
/* The same transfer inside ONE process: `dst` takes both component models and the pilot matrix as they sit in `src` (device to
 * device on dst's stream, hipMemcpyPeer when the contexts live on different GPUs), then rebuilds its pilot tables - a second
 * context (another stream, packet range or GPU of the process) without a second csi_load_weights.  It walks exactly the receiver
 * side of csi_broadcast_weights (same record, same buffer list, same rebuild), which is how a one-GPU box tests that code.
 * The contexts must agree in nt, len_ltf, hidden widths, n_out, use_bn, dtype and input pooling (nr, device and workspace may differ); a
 * mismatch is refused with text and leaves `dst` empty (nothing loaded, no pilot).  Synchronous at return. */
int  csi_clone_weights(csi_ctx* dst, const csi_ctx* src);

/* Per-kernel HIP-event timing on the context's stream (the reference's --execTime). */
int  csi_profile_enable(csi_ctx* ctx, int on);
int  csi_profile_reset(csi_ctx* ctx);
/* The practical ceiling of the dominant kernel, measured: the fused per-pair kernel's MFMA + barrier skeleton (no operand
 * conversion, no operand streams, no LDS traffic; operand registers filled once with the loaded model's own split weights) over
 * `rows` pair rows, `iters` launches timed with HIP events.  executed_flops = f16 flop per launch (3 MFMA products per multiply,
 * padded regressor tile included).  The part clocks to its power budget (~1.4 kW, 1.8-2.0 GHz under these
 * kernels), so the table peak of 2.5 PFLOP/s at 2.4 GHz is not reachable on real data; this is what is.  fp32 contexts with the
 * two-hidden-layer model loaded; the outputs it writes are garbage and go to the context's workspace. */
int  csi_profile_band_skeleton(csi_ctx* ctx, int64_t rows, int iters, double* ms_per_launch, double* executed_flops);
/* The host link, measured in this process: h2d_bytes up and d2h_bytes down between pinned host memory and device memory on the
 * host pipeline's two copy streams - each direction alone and both at once (ms).  ms_both is the floor of a host-buffer call that
 * moves these byte counts; bench.py reports the host-buffer entry points as a fraction of it. */
int  csi_profile_pcie(csi_ctx* ctx, int64_t h2d_bytes, int64_t d2h_bytes, double* ms_h2d, double* ms_d2h, double* ms_both);
int  csi_profile_num_kernels(void);
const char* csi_profile_kernel_name(int kernel_id);
/* total_ms / launches / flops / bytes accumulated since the last reset. */
int  csi_profile_query(csi_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches,
                       double* flops, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* CSI_MAMIMO_H */
