// csi_weights.hpp - what csi_load_weights uploads, prepared on the host: pure functions from the caller's csi_tensors and the facts of the context
// that shape them (WeightFacts) to a PreparedModel - layer by layer, one HostBuf per row of the buffer table (csi_context.hpp: kLayerBufs /
// kModelBufs) plus the scalars of the Layer.  No HIP call in this file: tests/test_weight_prep_host.py pins every byte of it on a machine without
// a GPU.  A new weight layout is one row of the table plus one function here.
#pragma once
#include "csi_context.hpp"

namespace {

struct WeightFacts { csi_config cfg; int d_in, l0_k, model_type, input_pool; };

// payload of one device buffer: bytes made here or - W0rm, a bias nothing is folded into - the caller's own array, uploaded without a host copy
struct HostBuf {
    std::vector<char> own;
    const void* data = nullptr; size_t bytes = 0;
    template <typename T> T* make(size_t n) { own.assign(n * sizeof(T), 0); data = own.data(); bytes = own.size(); return reinterpret_cast<T*>(own.data()); }
    void view(const float* p, size_t n) { data = p; bytes = n * sizeof(float); }
};

// What prepare_layer leaves: the layer it was called for last (a layer is uploaded before the next one is prepared: the host never holds more than
// one layer's copies), the per-model buffers, and what the next layer needs
struct PreparedModel {
    Layer layer;                                                // the scalars; the pointers stay null until the upload
    HostBuf lbuf[LAYER_BUFS], mbuf[MODEL_BUFS];                 // mbuf: conv from prepare_conv, W0p / W0rm from layer 0
    double hs_repr_err = 0.0;                                   // Model::hs_repr_err: worst row over the split copies of the layers so far
    std::string err;
    std::vector<float> prev_shift;          // BN shift of the previous layer: folded into this layer's bias (bf16) / bias_hs (split engine)
    std::vector<float> prev_scale;          // BN scale of the previous layer: folded into this layer's weights (bf16: always; split engine: where a kernel reads the bare relu)
    std::vector<float> wt_scratch; int fan_in = 0;
    int refuse(const char* fmt, ...) {
        char buf[512];
        va_list ap; va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return CSI_ERR_INVALID_ARG;
    }
};

std::string layer_tensor_base(const csi_config& cf, int li) { return li == cf.n_hidden ? std::string("fc_regressor") : "fc_dense" + std::to_string(li); }

uint16_t rne(float f) {                       // fp32 -> bf16, round to nearest even
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// keras [in][out] -> [out][ldw] (K-major, K zero-padded to a multiple of the k-tile), blocked for cache friendliness; wt arrives zeroed
void transpose_padded(const float* k, int in, int out, int ldw, float* wt) {
    const int TB = 32;
    for (int i0 = 0; i0 < in; i0 += TB)
        for (int o0 = 0; o0 < out; o0 += TB)
            for (int i = i0; i < std::min(in, i0 + TB); ++i)
                for (int o = o0; o < std::min(out, o0 + TB); ++o) wt[(size_t)o * ldw + i] = k[(size_t)i * out + o];
}

// The BatchNormalization SHIFT of the previous layer moves into this layer's bias, in double: (relu(z) sc + sh) W + b  =  (relu(z) sc) W + (b + sh W)
// - split engine (bias_hs): the A operand keeps the exact zeros of the relu (about half of it); the f16 matrix pipe is power-bound and runs ~5 %
// faster on such operands.  bf16 mode (bias): every hidden activation is bf16(relu(z)), see prepare_layer
void fold_bias(const float* b, const float* k, const std::vector<float>& prev_shift, int in, int out, float* dst) {
    for (int o = 0; o < out; ++o) {
        double acc = b[o];
        if (!prev_shift.empty())
            for (int i = 0; i < in; ++i) acc += (double)prev_shift[i] * (double)k[(size_t)i * out + o];
        dst[o] = (float)acc;
    }
}

// Split-f16 copy for gemm_hs.hip.h of the matrix value(o, i), o < out, i < kh: value * 2^wshift (largest magnitude in [2^12, 2^13)) as hi + lo
// halves in groups of 16 k-columns, ldwh halves per row (dst arrives zeroed).  Returns wshift and the representation error of the copy: worst
// OUTPUT ROW, ||x_o - (hi + lo)_o|| / ||x_o|| (a whole-matrix norm would be carried by the very outlier that causes the damage: the scale follows
// max |w|, the rows far below it lose their lo halves); 1.0 for a row that is not finite
struct SplitResult { int wshift; double worst; };
template <typename Value>
SplitResult split_f16_rows(Value value, int out, int kh, int ldwh, uint16_t* dst) {
    float wmax = 0.f;
    for (int o = 0; o < out; ++o)
        for (int i = 0; i < kh; ++i) wmax = std::max(wmax, std::fabs(value(o, i)));
    int e = 0;
    if (wmax > 0.f && std::isfinite(wmax)) std::frexp(wmax, &e);
    SplitResult r{std::max(-40, std::min(40, 13 - e)), 0.0};
    const float ws = std::ldexp(1.f, r.wshift);
    for (int o = 0; o < out; ++o) {
        double e_num = 0.0, e_den = 0.0;
        for (int i = 0; i < kh; ++i) {
            const float x = value(o, i) * ws;
            const _Float16 hi = (_Float16)x;
            const _Float16 lo = (_Float16)(x - (float)hi);
            uint16_t* d = &dst[(size_t)o * ldwh + (i >> 4) * 32 + (i & 15)];
            std::memcpy(d, &hi, 2);
            std::memcpy(d + 16, &lo, 2);
            const double res = (double)x - ((double)(float)hi + (double)(float)lo);
            e_num += res * res;
            e_den += (double)x * (double)x;
        }
        if (e_den > 0.0 && std::isfinite(e_den)) r.worst = std::max(r.worst, std::sqrt(e_num / e_den));
        else if (!std::isfinite(e_den)) r.worst = 1.0;
    }
    return r;
}

// The form the fused band kernels read (gemm_hs_band.hip.h): 256 rows (rows >= out zero: dst arrives zeroed), k permuted inside every group of 16 (hs_band_kperm)
// so that a lane's stage-1 accumulators are its stage-2 operand.  One rule for bf16 rows and for split rows, whose 16 hi and 16 lo halves of a k-group are two such groups
void kperm_rows(const uint16_t* src, int out, int ld, uint16_t* dst) {
    for (int o = 0; o < out; ++o)
        for (int i = 0; i < ld; ++i) dst[(size_t)o * ld + i] = src[(size_t)o * ld + (i & ~15) + hs_band_kperm(i & 15)];
}

// BatchNormalization of layer li as per-column scale / shift, and the split engine's scales of the activations this layer hands on
int bn_vectors(const csi_config& cf, const csi_tensor* tensors, int n, int li, Layer& L, std::vector<float>& sc, std::vector<float>& sh, PreparedModel& pm) {
    const int out = L.out;
    const std::string bn = "bn" + std::to_string(li);
    const csi_tensor *ga = find_tensor(tensors, n, bn + ".gamma"), *be = find_tensor(tensors, n, bn + ".beta");
    const csi_tensor *mu = find_tensor(tensors, n, bn + ".moving_mean"), *va = find_tensor(tensors, n, bn + ".moving_variance");
    if (!ga || !be || !mu || !va) return pm.refuse("csi_load_weights: missing %s.* (use_bn=1)", bn.c_str());
    for (const csi_tensor* t : {ga, be, mu, va})
        if (!t->data || t->rows * t->cols != out) return pm.refuse("csi_load_weights: %s.* must have %d elements", bn.c_str(), out);
    for (int o = 0; o < out; ++o) {
        // keras non-fused inference: inv = rsqrt(var + eps) * gamma; y = x*inv + (beta - mean*inv)
        const float inv = (1.0f / std::sqrt(va->data[o] + cf.bn_eps)) * ga->data[o];
        sc[o] = inv;
        sh[o] = be->data[o] - mu->data[o] * inv;
    }
    // split-f16 engine: scale of the activations this layer hands on.  Where the next kernel reads relu * scale (BatchNormalization output minus its
    // shift; Layer::ashift): beta + gamma * (standardised relu) is bounded by |beta| + 6 |gamma| at six moving standard deviations.  Where it reads the
    // bare relu because the scale sits in the next layer's weights (layer 0 on the shared path, the pair layer in front of the fused regressor;
    // Layer::ashift_pre): moving_mean + 6 moving standard deviations.  The bound is put at 2^10..2^11 - 32x of head room for outliers before the range
    // guard takes over, and values down to 2^-13 of the bound keep a normal lo half
    float amax = 0.f, amax_pre = 0.f;
    for (int o = 0; o < out; ++o) {
        amax = std::max(amax, std::fabs(be->data[o]) + 6.f * std::fabs(ga->data[o]));
        amax_pre = std::max(amax_pre, std::fabs(mu->data[o]) + 6.f * std::sqrt(std::max(va->data[o], 0.f) + cf.bn_eps));
    }
    auto shift_for = [](float bound, int dflt) {
        int ea = 0;
        if (!(bound > 0.f) || !std::isfinite(bound)) return dflt;
        std::frexp(bound, &ea);
        return std::max(-8, std::min(14, 11 - ea));
    };
    L.ashift = shift_for(amax, L.ashift);
    L.ashift_pre = shift_for(amax_pre, L.ashift_pre);
    return CSI_OK;
}

// the front end of a CONV1D model (conv_frontend.hip.h): cnn1d_1 [7 taps][128 filters] + bias, then its BatchNormalization folded to scale / shift in
// double - q = relu(conv) * gamma / sqrt(var + eps) + (beta - mean * gamma / sqrt(var + eps))
int prepare_conv(const WeightFacts& f, const csi_tensor* tensors, int n, PreparedModel& pm) {
    const char* names[6] = {"cnn1d_1.kernel", "cnn1d_1.bias", "conv_bn.gamma", "conv_bn.beta", "conv_bn.moving_mean", "conv_bn.moving_variance"};
    const csi_tensor* t[6];
    for (int i = 0; i < 6; ++i) {
        t[i] = find_tensor(tensors, n, names[i]);
        if (!t[i] || !t[i]->data)
            return pm.refuse("csi_load_weights: CONV1D model: missing %s (the front end needs cnn1d_1.kernel/.bias and conv_bn.gamma/.beta/.moving_mean/.moving_variance)", names[i]);
        if ((i == 0 && (t[i]->rows != CONV_TAPS || t[i]->cols != CONV_FILTERS)) || (i > 0 && t[i]->rows * t[i]->cols != CONV_FILTERS))
            return pm.refuse("csi_load_weights: CONV1D model: %s is [%lld,%lld], expected %s", names[i], (long long)t[i]->rows,
                             (long long)t[i]->cols, i == 0 ? "[7,128] (7 taps x 128 filters)" : "128 values");
    }
    float* prm = pm.mbuf[MB_conv].make<float>(CONV_PRM_FLOATS);
    for (int i = 0; i < CONV_TAPS * CONV_FILTERS; ++i) prm[i] = t[0]->data[i];
    for (int ch = 0; ch < CONV_FILTERS; ++ch) {
        const double sc = (double)t[2]->data[ch] / std::sqrt((double)t[5]->data[ch] + (double)f.cfg.bn_eps);
        prm[CONV_TAPS * CONV_FILTERS + ch] = t[1]->data[ch];
        prm[(CONV_TAPS + 1) * CONV_FILTERS + ch] = (float)sc;
        prm[(CONV_TAPS + 2) * CONV_FILTERS + ch] = (float)((double)t[3]->data[ch] - (double)t[4]->data[ch] * sc);
    }
    const int64_t ldw0 = ((int64_t)f.d_in + G_BK - 1) / G_BK * G_BK;
    if (ldw0 * f.cfg.hidden[0] >= ((int64_t)1 << 31))
        return pm.refuse("csi_load_weights: CONV1D model: fc_dense0 holds %lld x %d weights, at or above 2^31 elements (the layer-0 kernels "
                         "index it with 32-bit element offsets); a narrower hidden[0] or a smaller len_ltf", (long long)ldw0, f.cfg.hidden[0]);
    return CSI_OK;
}

// kernel / bias of layer li, found and checked against the width the context gives the layer
int layer_tensors(const WeightFacts& f, const csi_tensor* tensors, int n, int li, int fan_in, int out, const csi_tensor** k_out, const csi_tensor** b_out, PreparedModel& pm) {
    const csi_config& cf = f.cfg;
    const std::string base = layer_tensor_base(cf, li);
    const csi_tensor* k = *k_out = find_tensor(tensors, n, base + ".kernel");
    const csi_tensor* b = *b_out = find_tensor(tensors, n, base + ".bias");
    if (!k || !b || !k->data || !b->data) return pm.refuse("csi_load_weights: missing %s.kernel/.bias", base.c_str());
    if (li == 0 && cf.nt > 0 && k->rows != fan_in && k->cols == out)
        return pm.refuse("csi_load_weights: %s.kernel is [%lld,%lld], expected [%d,%d] (%s model, input pooling %s: %d LTF rows + %d pilot rows)%s",
                         base.c_str(), (long long)k->rows, (long long)k->cols, fan_in, out, model_type_name(f.model_type), input_pool_name(f.input_pool), f.l0_k, cf.nt,
                         k->rows == (int64_t)64 * cf.len_ltf + cf.nt ? " - a CONV1D model: csi_set_model_type(CONV1D) first" :
                         k->rows == (int64_t)cf.len_ltf / 2 + cf.nt ? " - a decimated model: csi_set_input_pool(max | avg) first" :
                         (k->rows == (int64_t)cf.len_ltf + cf.nt ? (f.model_type == CSI_MODEL_CONV1D ? " - an FC model: csi_set_model_type(FC)" : " - a model without pooling: csi_set_input_pool(none)") : ""));
    if (k->rows != fan_in || k->cols != out || b->rows * b->cols != out)
        return pm.refuse("csi_load_weights: %s.kernel is [%lld,%lld], expected [%d,%d]", base.c_str(), (long long)k->rows, (long long)k->cols, fan_in, out);
    return CSI_OK;
}

// Every buffer and scalar of layer li = 0, 1, ... n_hidden of one component model, in this order on one PreparedModel (layer 0: with the front end of
// a CONV1D model in front); stops at the first tensor that is missing or mis-shaped (pm.err, CSI_ERR_INVALID_ARG)
int prepare_layer(const WeightFacts& f, const csi_tensor* tensors, int n, int li, PreparedModel& pm) {
    const csi_config& cf = f.cfg;
    const bool bf16 = cf.dtype == CSI_DTYPE_BF16;
    if (li == 0) {
        pm.fan_in = f.d_in;
        if (f.model_type == CSI_MODEL_CONV1D)
            if (int rc = prepare_conv(f, tensors, n, pm)) return rc;
    }
    const int fan_in = pm.fan_in;
    std::vector<float>&prev_shift = pm.prev_shift, &prev_scale = pm.prev_scale, &wt_scratch = pm.wt_scratch;
    const bool reg = li == cf.n_hidden;
    const int out = reg ? cf.n_out : cf.hidden[li];
    const csi_tensor *k, *b;
    if (int rc = layer_tensors(f, tensors, n, li, fan_in, out, &k, &b, pm)) return rc;
    Layer& L = pm.layer = Layer();
    HostBuf* const B = pm.lbuf;
    for (int r = 0; r < LAYER_BUFS; ++r) { B[r].data = nullptr; B[r].bytes = 0; }      // (the vectors keep their memory for the next layer)
    L.in = fan_in; L.out = out;
    L.ldw = (fan_in + G_BK - 1) / G_BK * G_BK;
    if (bf16) wt_scratch.assign((size_t)out * L.ldw, 0.f);                 // bf16 mode keeps no fp32 copy on the device
    float* wt = bf16 ? wt_scratch.data() : B[LB_Wt].make<float>((size_t)out * L.ldw);
    transpose_padded(k->data, fan_in, out, L.ldw, wt);
    // the weight times the previous layer's BN scale: (relu(z) sc) W = relu(z) (diag(sc) W)
    auto wv = [&](bool fold) {
        return [&, fold](int o, int i) { const float w = wt[(size_t)o * L.ldw + i]; return fold ? (float)((double)w * (double)prev_scale[i]) : w; };
    };
    if (bf16) {
        // bf16 mode: the BatchNormalization of the previous layer lives in THIS layer's operands,
        //     (relu(z) sc + sh) W + b  =  relu(z) (diag(sc) W) + (b + sh W),
        // scaled rows rounded once, the shift product kept in fp32 in the bias below - so every hidden activation is bf16(relu(z)) and the kernels
        // that build or read it carry no per-column affine (the fused first per-pair layer generated its A operand slower than the matrix cores consumed it)
        L.ldwb = (fan_in + B_BK - 1) / B_BK * B_BK;
        uint16_t* wb = B[LB_Wb].make<uint16_t>((size_t)out * L.ldwb);
        auto scaled = wv(!prev_scale.empty());
        for (int o = 0; o < out; ++o)
            for (int i = 0; i < fan_in; ++i) wb[(size_t)o * L.ldwb + i] = rne(scaled(o, i));
        // the regressor behind ONE per-pair layer: a copy for the fused band kernel
        if (reg && li == 2 && cf.nt > 0 && out <= 256) kperm_rows(wb, out, L.ldwb, B[LB_Wb_p].make<uint16_t>((size_t)256 * L.ldwb));
        if (li == 0) B[LB_bias].view(b->data, out);
        else fold_bias(b->data, k->data, prev_shift, fan_in, out, B[LB_bias].make<float>(out));
    } else {
        // layer 0 keeps its LTF columns only (the pilot rows live in the table T)
        const int kh = (li == 0 && cf.nt > 0) ? f.l0_k : fan_in;
        L.ldwh = 2 * ((kh + HS_G - 1) / HS_G * HS_G);
        // layer 1 (the first per-pair layer; the regressor when there is one hidden layer) on the shared-layer-0 path: the pair kernel generates
        // A = relu(L0 + T) without bn0, so bn0's scale multiplies the rows of this copy and bn0's shift sits in bias_hs
        SplitResult r = split_f16_rows(wv(li == 1 && cf.nt > 0 && !prev_scale.empty()), out, kh, L.ldwh, B[LB_Wh].make<uint16_t>((size_t)out * L.ldwh));
        L.wshift = r.wshift;
        pm.hs_repr_err = std::max(pm.hs_repr_err, r.worst);
        if (reg && li == 2 && cf.nt > 0 && !prev_scale.empty()) {
            // the regressor behind ONE per-pair layer (the shipped 2-hidden-layer network): a second copy with that layer's BN scale folded into
            // the rows, for the kernel that runs the regressor behind the pair layer without h2 leaving the CU (gemm_hs.hip.h:
            // hs_fused_regressor); the unfused path keeps Wh.  And, up to 256 outputs, the form the fused band kernel reads
            uint16_t* whf = B[LB_Wh_f].make<uint16_t>((size_t)out * L.ldwh);
            r = split_f16_rows(wv(true), out, kh, L.ldwh, whf);
            L.wshift_f = r.wshift;
            pm.hs_repr_err = std::max(pm.hs_repr_err, r.worst);
            if (out <= 256) kperm_rows(whf, out, L.ldwh, B[LB_Wh_p].make<uint16_t>((size_t)256 * L.ldwh));
        }
        B[LB_bias].view(b->data, out);
        if (li >= 1) fold_bias(b->data, k->data, prev_shift, fan_in, out, B[LB_bias_hs].make<float>(out));
    }
    std::vector<float> sc(out, 1.f), sh(out, 0.f);
    if (!reg && cf.use_bn)
        if (int rc = bn_vectors(cf, tensors, n, li, L, sc, sh, pm)) return rc;
    if (!reg) {
        // bf16 mode: identity here, the real vectors go into the next layer (above)
        float *scale = B[LB_scale].make<float>(out), *shift = B[LB_shift].make<float>(out);
        for (int o = 0; o < out; ++o) { scale[o] = bf16 ? 1.f : sc[o]; shift[o] = bf16 ? 0.f : sh[o]; }
    }
    if (li == 0 && cf.nt > 0) {
        // pilot rows of fc_dense0.kernel, [nt][h1] row-major as stored (bf16 mode: rounded like every other weight, the table itself is
        // evaluated in fp32); split engine: the LTF rows as stored for the skinny layer-0 kernel
        float* w0p = pm.mbuf[MB_W0p].make<float>((size_t)cf.nt * out);
        std::memcpy(w0p, k->data + (size_t)f.l0_k * out, (size_t)cf.nt * out * sizeof(float));
        if (bf16)
            for (size_t i = 0; i < (size_t)cf.nt * out; ++i) { const uint32_t u = (uint32_t)rne(w0p[i]) << 16; std::memcpy(&w0p[i], &u, 4); }
        else pm.mbuf[MB_W0rm].view(k->data, (size_t)f.l0_k * out);
    }
    prev_shift = sh;
    prev_scale = sc;
    pm.fan_in = out;
    return CSI_OK;
}

}  // namespace
