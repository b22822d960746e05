// csi_dnn_hs.hpp - host side of the split-f16 engine of fp32 contexts (gemm_hs.hip.h): which GEMMs
// of a packet chunk run on it and how they are launched.  The engine serves the throughput regime
// (256x256 tiles, one workgroup per CU); small calls stay on the native fp32 MFMA kernels, and since
// the layer-0 product L0 is plain fp32 either way the two engines mix freely per layer.
#pragma once
#include "csi_context.hpp"
#include "csi_band.hpp"

namespace {

constexpr int HS_L0_MAX_SPLITS = 8;

// shapes the kernels can serve: every hidden width a multiple of 16 (hs groups), split weights present
bool hs_static_ok(const csi_ctx* c, const Model& m) {
    const csi_config& cf = c->cfg;
    if (c->f32_engine == 0 || cf.dtype != CSI_DTYPE_F32 || cf.nt <= 0 || (c->l0_k % HS_G) != 0) return false;
    if (!m.hs_repr_ok) return false;          // split copies of this model's weights are not fp32-grade (csi_load_weights): fp32 MFMA kernels
    for (int i = 0; i < cf.n_hidden; ++i)
        if (cf.hidden[i] % HS_G) return false;
    for (size_t i = 0; i < m.layers.size(); ++i)
        if (!m.layers[i].Wh || (i >= 1 && !m.layers[i].bias_hs)) return false;
    return true;
}

long hs_tiles(int M, int N) { return (long)((M + PP_BM - 1) / PP_BM) * ((N + PP_BN - 1) / PP_BN); }

// per-pair layers of a chunk of M2 rows on the split engine?  ("force_tile" = 128 / 256 keeps addressing the
// fp32 MFMA kernels of that tile height for small shapes - tests - and 128 excludes this engine)
bool hs_tail_wanted(const csi_ctx* c, int M2, int n1) {
    if (c->force_pair_tile == 128) return false;
    return c->f32_engine == 1 || hs_tiles(M2, n1) >= c->hs_min_blocks;
}

// Split-K of the layer-0 product on the split engine: the count (<= 8, >= 512 k-columns each) whose
// last round of 256 workgroups is fullest; 0 = leave layer 0 to the native kernels.
int hs_layer0_splits(const csi_ctx* c, int M1, int h1, int K, int* k_per_split) {
    if (M1 <= 8 || c->force_pair_tile == 128) return 0;
    const long tiles = (long)((M1 + PP_BM - 1) / PP_BM + 7) / 8 * 8 * ((h1 + PP_BN - 1) / PP_BN);       // as launched (pp_grid)
    int best = 1;
    double best_eff = 0.0;
    // CONV1D contexts (K0 = 64 len_ltf): up to L0_CONV_MAX_SPLITS ranges, so that a chunk's few output tiles fill the chip
    const int max_s = c->model_type == CSI_MODEL_CONV1D ? L0_CONV_MAX_SPLITS : HS_L0_MAX_SPLITS;
    for (int s = 1; s <= max_s; ++s) {
        if (s > 1 && K / s < 512) break;
        const long blocks = tiles * s;
        const double eff = (double)blocks / (double)((blocks + 255) / 256 * 256) - 0.01 * (s - 1);
        if (eff > best_eff) { best_eff = eff; best = s; }
    }
    const int kps = ((K + best - 1) / best + 63) / 64 * 64;
    const int real = (K + kps - 1) / kps;
    if (kps / HS_G < 3) return 0;
    if (c->f32_engine != 1 && hs_tiles(M1, h1) * real < std::max(c->hs_min_blocks, 128)) return 0;
    *k_per_split = kps;
    return real;
}

// Range guard: has any split-engine GEMM since the last check converted an operand near / beyond the
// f16 limit (*hit = the magnitude seen), or a row whose scaled magnitudes all sat in the f16 denormal
// range (*low)?  The caller has synchronised the stream.
int hs_range_check(csi_ctx* c, float* hit, bool* low) {
    *hit = 0.f;
    *low = false;
    if (!c->hs_peak || c->hs_launches == c->hs_checked) return CSI_OK;
    c->hs_checked = c->hs_launches;
    unsigned bits[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpy(bits, c->hs_peak, sizeof(bits), hipMemcpyDeviceToHost));
    if (bits[0] || bits[1] || bits[2]) {
        std::memcpy(hit, &bits[0], 4);
        *low = bits[1] != 0;
        HIP_TRY(c, hipMemset(c->hs_peak, 0, sizeof(bits)));
    }
    if (bits[2])
        return fail(c, CSI_ERR_HIP, "fused regressor: a workgroup waited 2 s for the partial sums of its row tile - results of the calls since the "
                    "last check are not valid (set hs_fuse_regressor to 0 and report this)");
    return CSI_OK;
}

template <typename Kern>
int hs_dynamic_lds(csi_ctx* c, Kern kern, size_t bytes, size_t* have) {
    if (*have < bytes) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        *have = bytes;
    }
    return CSI_OK;
}

// Layer 0 of a mid-size call on the weight-streaming kernel (l0_hs_stream.hip.h): the number of k ranges, 0 = the call is not its
// (at most 8 preambles: layer0_skinny_kernel / the one-packet path; more than 256: the 256 x 256 kernels have enough row tiles)
int l0_stream_splits(const csi_ctx* c, const Model& m, int M1, int h1, int K, int* k_per_split) {
    if (c->hs_in_shift != HS_SHIFT_AUTO) return 0;        // a fixed input scale ("hs_in_shift") addresses the kernels that take one scale per launch
    if (!c->l0_stream || M1 <= 8 || M1 > c->l0_stream_max_rows || (K % L0S_KC) != 0 || K < 2 * L0S_KC || c->force_pair_tile || !m.layers[0].Wh) return 0;
    const int groups = (h1 + L0S_COLS - 1) / L0S_COLS;
    const int blocks = (M1 + 255) / 256;                              // row blocks (gridDim.z)
    int ks = c->l0_stream_ks > 0 ? c->l0_stream_ks : std::max(1, (M1 <= 128 ? 256 : 128) / (groups * blocks));
    ks = std::max(1, std::min(ks, K / (2 * L0S_KC)));                 // at least two chunks per range
    const int kps = ((K + ks - 1) / ks + L0S_KC - 1) / L0S_KC * L0S_KC;
    *k_per_split = kps;
    return (K + kps - 1) / kps;
}

int l0_stream_launch(csi_ctx* c, Model& m, const float* x, int ldx, int M1, int h1, int K, int kps, int splits, float* slabs) {
    const Layer& l0 = m.layers[0];
    L0StreamArgs a{};
    a.x = x; a.Wh = l0.Wh; a.slabs = slabs;
    a.M = M1; a.N = h1; a.K = K; a.lda = ldx; a.ldwh = l0.ldwh; a.kps = kps; a.wshift = l0.wshift;
    const int blocks = (M1 + 255) / 256;
    const int rt = ((M1 + 31) / 32 + blocks - 1) / blocks;           // row tiles per workgroup: the row blocks are (nearly) equal
    const int rt_inst = rt <= 4 ? rt : (rt <= 6 ? 6 : 8);
    const dim3 grid((unsigned)((h1 + L0S_COLS - 1) / L0S_COLS), (unsigned)splits, (unsigned)((M1 + 32 * rt_inst - 1) / (32 * rt_inst)));
    ++c->l0_stream_launches;
    if (M1 > c->l0_stream_prepass_rows) {
        // row maxima over the whole K by their own small kernel (beyond 64 preambles cheaper than the first pass of every workgroup)
        if (!m.l0_rowmax && hipMalloc((void**)&m.l0_rowmax, 4096 * sizeof(float)) != hipSuccess)
            return fail(c, CSI_ERR_NOMEM, "device allocation of the row maxima failed");
        hipLaunchKernelGGL(l0_row_max_kernel, dim3((unsigned)M1), dim3(256), 0, c->stream, x, ldx, K, m.l0_rowmax);
        HIP_TRY(c, hipGetLastError());
        a.row_max = m.l0_rowmax;
    }
    ProfScope ps(c, K_LAYER0_LTF, 2.0 * (double)M1 * h1 * K, 4.0 * ((double)M1 * K + (double)h1 * K + (double)M1 * h1 * splits));
    auto go = [&](auto kern, int rtt, size_t* attr) {
        const size_t lds = l0s_lds_bytes(rtt);
        int rc = hs_dynamic_lds(c, kern, lds, attr);
        if (rc) return rc;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, c->stream, a);
        HIP_TRY(c, hipGetLastError());
        return (int)CSI_OK;
    };
    if (rt <= 1) return go(l0_hs_stream_kernel<1>, 1, &c->hs_lds_attr[14]);
    if (rt <= 2) return go(l0_hs_stream_kernel<2>, 2, &c->hs_lds_attr[15]);
    if (rt <= 3) return go(l0_hs_stream_kernel<3>, 3, &c->hs_lds_attr[16]);
    if (rt <= 4) return go(l0_hs_stream_kernel<4>, 4, &c->hs_lds_attr[17]);
    if (rt <= 6) return go(l0_hs_stream_kernel<6>, 6, &c->hs_lds_attr[18]);
    return go(l0_hs_stream_kernel<8>, 8, &c->hs_lds_attr[19]);
}

// layer 0: slabs[z][M1][h1] = (X[M1][K] * W0[0:K, :]) over k range z, X converted inside the kernel
int hs_launch_layer0(csi_ctx* c, const Model& m, const float* x, int ldx, int M1, int h1, int K, int kps, int splits, float* slabs) {
    const Layer& l0 = m.layers[0];
    GemmHsArgs g{};
    g.Bt = l0.Wh; g.ldb = l0.ldwh;
    g.C = slabs; g.ldc = h1;
    g.M = M1; g.N = h1; g.K = K;
    g.k_per_split = kps;
    g.tiles_n = (h1 + PP_BN - 1) / PP_BN;
    const bool auto_scale = c->hs_in_shift == HS_SHIFT_AUTO;
    const int in_shift = auto_scale ? 0 : c->hs_in_shift;
    g.acc_scale = std::ldexp(1.f, -(in_shift + l0.wshift));
    g.peak = c->hs_peak;
    g.wshift = l0.wshift;
    ++c->hs_launches;
    if (auto_scale) {
        // magnitude estimate of these rows (1-KiB blocks, at most ~4 MiB of them), stream-ordered in front of the GEMM
        unsigned* dyn = c->hs_peak + 8 + (&m == &c->model[1] ? 1 : 0);      // one word per component model (small calls run them on two streams)
        HIP_TRY(c, hipMemsetAsync(dyn, 0, sizeof(unsigned), c->stream));
        const size_t n4 = (size_t)M1 * ldx / 4;
        const size_t nblk = (n4 + 63) / 64;                                   // 1-KiB blocks
        const size_t step = std::max<size_t>(1, nblk / 4096);                 // at most ~4 MiB (a million samples) are read
        const unsigned blocks = (unsigned)std::min<size_t>((nblk / step + 3) / 4, 1024);
        hipLaunchKernelGGL(hs_absmax_sample_kernel, dim3(std::max(blocks, 1u)), dim3(256), 0, c->stream, x, n4, step, dyn);
        HIP_TRY(c, hipGetLastError());
        g.dyn_max = dyn;
    }
    const double flops = 2.0 * (double)M1 * h1 * K;
    const double bytes = 4.0 * ((double)M1 * K + (double)h1 * K + (double)M1 * h1 * splits);
    ProfScope ps(c, K_LAYER0_LTF, flops, bytes);
    const size_t lds = (size_t)PPP_RING_FLOATS * sizeof(float);
    PairSrc src{x, nullptr, ldx, 1};
    const int tiles_m = (M1 + PP_BM - 1) / PP_BM;
    auto go = [&](auto kern, size_t* attr) {
        int rc = hs_dynamic_lds(c, kern, lds, attr);
        if (rc) return rc;
        hipLaunchKernelGGL(kern, dim3(pp_grid(tiles_m, g.tiles_n), 1, (unsigned)splits), dim3(PP_THREADS), lds, c->stream, g, src,
                           std::ldexp(1.f, in_shift), PairRegArgs{});
        HIP_TRY(c, hipGetLastError());
        return (int)CSI_OK;
    };
    // "hs_vm": hand-counted vector-memory operations (gemm_hs.hip.h) - 2 = with the extra sub-tile of look-ahead for the fp32 rows
    if (c->hs_vm_cast == 3) {
        const size_t lds5 = (size_t)5 * PP_SUBF * sizeof(float);
        auto kern = gemm_hs_pp_pair_kernel<EPI_RAW, false, true, 0, false, 3>;
        int rc = hs_dynamic_lds(c, kern, lds5, &c->hs_lds_attr[11]);
        if (rc) return rc;
        hipLaunchKernelGGL(kern, dim3(pp_grid(tiles_m, g.tiles_n), 1, (unsigned)splits), dim3(PP_THREADS), lds5, c->stream, g, src,
                           std::ldexp(1.f, in_shift), PairRegArgs{});
        HIP_TRY(c, hipGetLastError());
        return CSI_OK;
    }
    if (c->hs_vm_cast == 2) {
        // "hs_l0_mfma" = 16: the 16x16x32 main loop walks PAIRS of sub-tiles - every k range must hold an even number of them
        bool even = c->hs_l0_mfma == 16 && kps % (2 * HS_G) == 0;
        if (even) {
            const int klast = K - (splits - 1) * kps;
            even = klast > 0 && ((klast + HS_G - 1) / HS_G) % 2 == 0;
        }
        if (even) {
            ++c->hs_l0_mfma16_launches;
            return go(gemm_hs_pp_pair_kernel<EPI_RAW, false, true, 0, false, 2, 16>, &c->hs_lds_attr[20]);
        }
        return go(gemm_hs_pp_pair_kernel<EPI_RAW, false, true, 0, false, 2>, &c->hs_lds_attr[5]);
    }
    if (c->hs_vm_cast == 1) return go(gemm_hs_pp_pair_kernel<EPI_RAW, false, true, 0, false, 1>, &c->hs_lds_attr[6]);
    return go(gemm_hs_pp_pair_kernel<EPI_RAW, false, true>, &c->hs_lds_attr[0]);
}

// first per-pair layer: A generated from (L0, T, bn0); hs output (a hidden layer follows) or fp32
// output with bias only (the regressor follows layer 0 directly)
// shift of the OUTPUT activations of hidden layer li
// (pre: the consumer reads this layer's bare relu output - its BatchNormalization scale sits in the consumer's weights)
int hs_act_shift_of(const csi_ctx* c, const Model& m, int li, bool pre = false) {
    return c->hs_act_shift == HS_SHIFT_AUTO ? (pre ? m.layers[li].ashift_pre : m.layers[li].ashift) : c->hs_act_shift;
}

template <int EPI, bool OUT_HS>
int hs_launch_pair(csi_ctx* c, int kid, GemmHsArgs g, const PairSrc& src, int in_shift) {
    g.tiles_n = (g.N + PP_BN - 1) / PP_BN;
    g.peak = c->hs_peak;
    g.xcd_cols = 1;            // a column tile per XCD: its 1 MiB of weights stays in that L2 (the A side is 32 KB per row tile); -2.5 %
    ++c->hs_launches;
    const double flops = 2.0 * (double)g.M * g.N * g.K;
    const double bytes = 4.0 * ((double)g.M / src.nt * g.K + (double)src.nt * g.K + (double)g.N * g.K + (double)g.M * g.N);
    ProfScope ps(c, kid, flops, bytes);
    const size_t lds = (size_t)PPP_RING_FLOATS * sizeof(float);
    const int tiles_m = (g.M + PP_BM - 1) / PP_BM;
    auto go = [&](auto kern, size_t* attr) {
        int rc = hs_dynamic_lds(c, kern, lds, attr);
        if (rc) return rc;
        hipLaunchKernelGGL(kern, dim3(pp_grid(tiles_m, g.tiles_n)), dim3(PP_THREADS), lds, c->stream, g, src, std::ldexp(1.f, in_shift), PairRegArgs{});
        HIP_TRY(c, hipGetLastError());
        return (int)CSI_OK;
    };
    if (c->hs_vm_pair == 3) {
        const size_t lds5 = (size_t)5 * PP_SUBF * sizeof(float);
        auto kern = gemm_hs_pp_pair_kernel<EPI, OUT_HS, false, 0, false, 3>;
        int rc = hs_dynamic_lds(c, kern, lds5, &c->hs_lds_attr[OUT_HS ? 12 : 13]);
        if (rc) return rc;
        hipLaunchKernelGGL(kern, dim3(pp_grid(tiles_m, g.tiles_n)), dim3(PP_THREADS), lds5, c->stream, g, src, std::ldexp(1.f, in_shift), PairRegArgs{});
        HIP_TRY(c, hipGetLastError());
        return CSI_OK;
    }
    if (c->hs_vm_pair == 2) return go(gemm_hs_pp_pair_kernel<EPI, OUT_HS, false, 0, false, 2>, &c->hs_lds_attr[OUT_HS ? 7 : 8]);
    if (c->hs_vm_pair == 1) return go(gemm_hs_pp_pair_kernel<EPI, OUT_HS, false, 0, false, 1>, &c->hs_lds_attr[OUT_HS ? 9 : 10]);
    return go(gemm_hs_pp_pair_kernel<EPI, OUT_HS, false>, &c->hs_lds_attr[OUT_HS ? 1 : 2]);
}

template <int EPI, bool OUT_HS>
int hs_launch_gemm(csi_ctx* c, int kid, GemmHsArgs g) {
    g.tiles_n = (g.N + PP_BN - 1) / PP_BN;
    g.peak = c->hs_peak;
    ++c->hs_launches;
    g.k_per_split = (g.K + HS_G - 1) / HS_G * HS_G;
    const double flops = 2.0 * (double)g.M * g.N * g.K;
    const double bytes = 4.0 * ((double)g.M * g.K + (double)g.N * g.K + (double)g.M * g.N);
    ProfScope ps(c, kid, flops, bytes);
    const int tiles_m = (g.M + PP_BM - 1) / PP_BM;
    hipLaunchKernelGGL((gemm_hs_pp_kernel<EPI, OUT_HS>), dim3(pp_grid(tiles_m, g.tiles_n)), dim3(PP_THREADS), 0, c->stream, g);
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

// csi_profile_band_skeleton: the band kernel's MFMA + barrier skeleton (band_kernel_gen.py 'skeleton_rnd': no operand conversion, no
// L0 / T streams, no LDS-DMA, no fragment reads; its 48 operand registers filled once from the model's own split weights, relu-like
// zeros in the activation fragments) on `rows` pair rows of the loaded real model.  What it measures is the rate the matrix pipe of
// THIS part sustains on THIS data inside the power budget with everything else of the kernel removed - the practical ceiling the
// bench divides by next to the table peak (its output is garbage and goes to the workspace).
int band_skeleton_time(csi_ctx* c, int64_t rows, int iters, double* ms_per_launch, double* executed_flops) {
#ifdef CSI_HAVE_BAND8
    const csi_config& cf = c->cfg;
    Model& m = c->model[0];
    if (cf.dtype != CSI_DTYPE_F32 || cf.n_hidden != 2 || !m.loaded || !m.layers[2].Wh_p || rows <= 0 || rows > (1 << 30) || iters < 1)
        return fail(c, CSI_ERR_INVALID_ARG, "csi_profile_band_skeleton: needs an fp32 context with the two-hidden-layer model loaded, rows > 0");
    hipFunction_t sk = nullptr;
    if (!band_load(c) || hipModuleGetFunction(&sk, c->band_mod, "csi_band8_skeleton_rnd") != hipSuccess || !sk) {
        (void)hipGetLastError();
        return fail(c, CSI_ERR_NOT_READY, "csi_profile_band_skeleton: the band kernel's code object holds no skeleton variant");
    }
    const Layer &l1 = m.layers[1], &lr = m.layers[2];
    const int h1 = cf.hidden[0], M2 = (int)rows;
    int rc = ensure_bytes(c, &c->ws, &c->ws_bytes, (size_t)M2 * cf.n_out * sizeof(float) + ((size_t)M2 / std::max(cf.nt, 1) + 256) * h1 * sizeof(float));
    if (rc) return rc;
    BandArgs ba{};
    ba.out = reinterpret_cast<float*>(c->ws); ba.ldo = cf.n_out;
    ba.L0 = ba.out + (size_t)M2 * cf.n_out; ba.Ts = m.T_hs ? m.T_hs : m.T; ba.ldl = h1; ba.nt = cf.nt; ba.in_scale = 1.f;
    ba.W1 = l1.Wh; ba.ldb1 = l1.ldwh; ba.bias1 = l1.bias_hs; ba.M = M2; ba.K1 = h1; ba.N1 = l1.out;
    ba.acc_scale1 = 1.f; ba.out_scale = 1.f;
    ba.W2p = lr.Wh_p; ba.ldb2 = lr.ldwh; ba.bias2 = lr.bias_hs; ba.n2 = cf.n_out; ba.acc_scale2 = 1.f;
    ba.peak = nullptr;
    if (!band8_serves(ba)) return fail(c, CSI_ERR_INVALID_ARG, "csi_profile_band_skeleton: the band kernel does not serve this shape");
    Band8Args a8 = band8_args(ba);
    size_t sz = sizeof(a8);
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a8, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
    const unsigned grid = (unsigned)((M2 + BAND_ROWS - 1) / BAND_ROWS);
    struct Events {                                    // destroyed on every return path (an early HIP_TRY return leaked them)
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
    } ev;
    HIP_TRY(c, hipEventCreate(&ev.a));
    HIP_TRY(c, hipEventCreate(&ev.b));
    const hipEvent_t e0 = ev.a, e1 = ev.b;
    for (int i = 0; i < 2; ++i) HIP_TRY(c, hipModuleLaunchKernel(sk, grid, 1, 1, BAND8_THREADS, 1, 1, 0, c->stream, nullptr, extra));
    HIP_TRY(c, hipEventRecord(e0, c->stream));
    for (int i = 0; i < iters; ++i) HIP_TRY(c, hipModuleLaunchKernel(sk, grid, 1, 1, BAND8_THREADS, 1, 1, 0, c->stream, nullptr, extra));
    HIP_TRY(c, hipEventRecord(e1, c->stream));
    HIP_TRY(c, hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
    if (ms_per_launch) *ms_per_launch = (double)ms / iters;
    // executed f16 flop: 3 products, the padded 256-column regressor tile included (what the pipe really does)
    if (executed_flops) *executed_flops = 3.0 * (2.0 * (double)grid * BAND_ROWS * l1.out * h1 + 2.0 * (double)grid * BAND_ROWS * 256.0 * l1.out);
    return CSI_OK;
#else
    return fail(c, CSI_ERR_NOT_READY, "csi_profile_band_skeleton: the library was built without the band kernel");
#endif
}

// the per-pair layers of one chunk: l0sum [M1][h1] fp32 -> out [M2][n_out] fp32; hbuf0 / hbuf1 are the
// ping-pong activation buffers of the fp32 path re-used as hs matrices (same 4 bytes per element)
int hs_tail(csi_ctx* c, Model& m, const float* l0sum, int M2, float* hbuf0, float* hbuf1, float* out) {
    const csi_config& cf = c->cfg;
    const int nh = cf.n_hidden, h1 = cf.hidden[0];
    const Layer& l1 = m.layers[1];
    const int s0 = hs_act_shift_of(c, m, 0, true);
    // bn0 is not applied by the pair kernel: its scale multiplies the rows of layer 1's split weights, its shift
    // (like every later BatchNormalization shift) lives in layer 1's bias (Layer::bias_hs) - A = relu(2^s0 L0 + Ts)
    // with Ts = 2^s0 T, a copy of the pilot table rebuilt when the table or the shift changes
    if (m.T_hs_shift != s0) {
        const size_t bytes = ((size_t)cf.nt * h1 + G_SLACK_FLOATS) * sizeof(float);
        if (!m.T_hs) {
            if (hipMalloc((void**)&m.T_hs, bytes) != hipSuccess) return fail(c, CSI_ERR_NOMEM, "pilot table allocation failed");
            HIP_TRY(c, hipMemsetAsync(m.T_hs, 0, bytes, c->stream));
        }
        ProfScope ps(c, K_PILOT_TABLE, 2.0 * cf.nt * cf.nt * h1, 4.0 * (cf.nt * cf.nt + 2.0 * cf.nt * h1));
        hipLaunchKernelGGL(pilot_table_kernel, dim3((h1 + 255) / 256, cf.nt), dim3(256), 0, c->stream, c->P, m.W0p, m.layers[0].bias, m.T_hs,
                           cf.nt, h1, std::ldexp(1.f, s0));
        HIP_TRY(c, hipGetLastError());
        m.T_hs_shift = s0;
        m.T_sw_ok = false;
    }
    PairSrc src{l0sum, m.T_hs, h1, cf.nt};
    GemmHsArgs p{};
    p.Bt = l1.Wh; p.ldb = l1.ldwh;
    p.M = M2; p.N = l1.out; p.K = h1;
    p.bias = l1.bias_hs; p.scale = l1.scale; p.shift = c->hs_zero;
    p.acc_scale = std::ldexp(1.f, -(s0 + l1.wshift));
    if (nh == 1) {
        p.C = out; p.ldc = cf.n_out;
        return hs_launch_pair<EPI_BIAS, false>(c, K_REGRESSOR, p, src, s0);
    }
    const Layer& lr = m.layers[nh];
    if (nh == 2 && c->hs_band && !c->hs_fuse_regressor && lr.Wh_p) {
        // first per-pair layer + regressor in one kernel, h2 in registers: the assembly band kernels (csi_band.hpp chooses the form)
        const int s1 = hs_act_shift_of(c, m, 1, true);
        BandArgs ba{};
        ba.L0 = l0sum; ba.Ts = m.T_hs; ba.ldl = h1; ba.nt = cf.nt; ba.in_scale = std::ldexp(1.f, s0);
        ba.W1 = l1.Wh; ba.ldb1 = l1.ldwh; ba.bias1 = l1.bias_hs; ba.M = M2; ba.K1 = h1; ba.N1 = l1.out;
        ba.acc_scale1 = std::ldexp(1.f, -(s0 + l1.wshift)); ba.out_scale = std::ldexp(1.f, s1);
        ba.W2p = lr.Wh_p; ba.ldb2 = lr.ldwh; ba.bias2 = lr.bias_hs; ba.n2 = cf.n_out; ba.acc_scale2 = std::ldexp(1.f, -(s1 + lr.wshift_f));
        ba.out = out; ba.ldo = cf.n_out; ba.peak = c->hs_peak;
        const bool staged = band8_staged(ba, false) && c->hs_band != 3;       // "hs_band" = 3: the form with per-lane global loads of L0 / T (A/B runs)
        if (band8_serves(ba) && h1 == l1.in && lr.in == l1.out && band_load(c)) {
            ++c->hs_launches;
            const double flops = 2.0 * (double)M2 * l1.out * h1 + 2.0 * (double)M2 * cf.n_out * l1.out;
            const double bytes = 4.0 * ((double)M2 / cf.nt * h1 + (double)cf.nt * h1 + (double)l1.out * h1 + (double)cf.n_out * l1.out + (double)M2 * cf.n_out);
            // (the band path leaves the activation buffers unused: hbuf0 - M2 x 1024 floats here - holds the partial outputs of column splits)
            return band_run(c, m, ba, false, staged, hbuf0, (size_t)M2 * l1.out, flops, bytes);
        }
    }
    if (nh == 2 && c->hs_fuse_regressor && lr.Wh_f && cf.n_out <= PP_BN && l1.out % PP_BN == 0) {
        // regressor inside the pair kernel: h2 never leaves the CU (hs_fused_regressor)
        const int tiles_m = (M2 + PP_BM - 1) / PP_BM, tiles_n = l1.out / PP_BN;
        const size_t slab_bytes = (size_t)(tiles_n - 1) * M2 * cf.n_out * sizeof(float);
        int rc = ensure_bytes(c, &c->fuse_ws, &c->fuse_ws_bytes, slab_bytes + ((size_t)tiles_m + 64) * sizeof(unsigned));
        if (rc) return rc;
        const int s1 = hs_act_shift_of(c, m, 1, true);
        PairRegArgs rg{};
        rg.B2 = lr.Wh_f; rg.ldb2 = lr.ldwh; rg.n2 = cf.n_out;
        rg.bias2 = lr.bias_hs;
        rg.out = out;
        rg.slabs = reinterpret_cast<float*>(c->fuse_ws);
        rg.flags = reinterpret_cast<unsigned*>(c->fuse_ws + slab_bytes);
        rg.err = c->hs_peak + 2;
        rg.acc_scale2 = std::ldexp(1.f, -(s1 + lr.wshift_f));
        p.out_scale = std::ldexp(1.f, s1);
        p.tiles_n = tiles_n;
        p.peak = c->hs_peak;
        p.xcd_cols = 0;                     // the kernel's flag wait relies on the plain blockIdx -> (row tile, column tile) order: never the XCD remap
        HIP_TRY(c, hipMemsetAsync(rg.flags, 0, (size_t)tiles_m * sizeof(unsigned), c->stream));
        ++c->hs_launches;
        const double flops = 2.0 * (double)M2 * l1.out * h1 + 2.0 * (double)M2 * cf.n_out * l1.out;
        const double bytes = 4.0 * ((double)M2 / cf.nt * h1 + (double)cf.nt * h1 + (double)l1.out * h1 + (double)cf.n_out * l1.out +
                                    (double)M2 * cf.n_out * (2.0 * (tiles_n - 1) + 1.0));
        ProfScope ps(c, K_PAIR_DENSE, flops, bytes);
        auto kern = gemm_hs_pp_pair_kernel<EPI_RAW, false, false, 0, true>;
        rc = hs_dynamic_lds(c, kern, (size_t)PR_LDS_FLOATS * sizeof(float), &c->hs_lds_attr[3]);
        if (rc) return rc;
        hipLaunchKernelGGL(kern, dim3(pp_grid(tiles_m, tiles_n)), dim3(PP_THREADS), (size_t)PR_LDS_FLOATS * sizeof(float), c->stream, p, src,
                           std::ldexp(1.f, s0), rg);
        HIP_TRY(c, hipGetLastError());
        return CSI_OK;
    }
    uint16_t* hb[2] = {reinterpret_cast<uint16_t*>(hbuf0), reinterpret_cast<uint16_t*>(hbuf1)};
    p.C = hb[0]; p.ldc = 2 * l1.out;
    p.c_blk = c->hs_blocked;            // activation matrices between split-engine layers: blocked layout (hs_blk_offset)
    p.out_scale = std::ldexp(1.f, hs_act_shift_of(c, m, 1));
    int rc = hs_launch_pair<EPI_BIAS_RELU_AFFINE, true>(c, K_PAIR_DENSE, p, src, s0);
    if (rc) return rc;
    int cur = 0;
    for (int li = 2; li <= nh; ++li) {
        const Layer& l = m.layers[li];
        GemmHsArgs q{};
        q.A = hb[cur]; q.lda = 2 * l.in;
        q.a_blk = q.c_blk = c->hs_blocked;
        q.Bt = l.Wh; q.ldb = l.ldwh;
        q.M = M2; q.N = l.out; q.K = l.in;
        q.bias = l.bias_hs; q.scale = l.scale; q.shift = c->hs_zero;
        q.acc_scale = std::ldexp(1.f, -(hs_act_shift_of(c, m, li - 1) + l.wshift));
        if (li == nh) {
            q.C = out; q.ldc = cf.n_out;
            rc = hs_launch_gemm<EPI_BIAS, false>(c, K_REGRESSOR, q);
        } else {
            q.out_scale = std::ldexp(1.f, hs_act_shift_of(c, m, li));
            q.C = hb[cur ^ 1]; q.ldc = 2 * l.out;
            rc = hs_launch_gemm<EPI_BIAS_RELU_AFFINE, true>(c, K_DENSE_HIDDEN, q);
            cur ^= 1;
        }
        if (rc) return rc;
    }
    return CSI_OK;
}

}  // namespace
