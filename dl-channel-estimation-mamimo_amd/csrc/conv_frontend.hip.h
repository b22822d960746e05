// conv_frontend.hip.h - the front end of the reference's CONV1D models (massiveMIMO_CSI_prediction_DNN.py:236-250, --model CONV1D): the
// time-domain LTF row x[L] (L = len_ltf) is a [L, 1] sequence that goes through
//     conv[t,c] = b[c] + sum_{j<7} K[j][c] x[t + j - 3]     (Conv1D(128, 7, padding='same'); x = 0 outside [0, L))
//     q[t,c]    = relu(conv[t,c]) * scale[c] + shift[c]    (its BatchNormalization, moving statistics: scale = gamma rsqrt(var + eps),
//                                                           shift = beta - mean scale, folded at csi_load_weights)
//     f[u*128 + c] = (q[2u,c] + q[2u+1,c]) / 2             (AveragePooling1D(): pool 2, stride 2, valid; Flatten, channels last)
// so layer 0 reads K0 = 64 L features per preamble (then the nt pilot inputs, as for the FC models).  Everything in fp32; bf16 contexts
// store the features rounded to bf16 (nearest even, as f32_to_bf16_kernel rounds).
//
//   conv_frontend_kernel<CPL, BF16>        planes x[p] [rows][ldx] -> y[p] [rows][ldy] (ldy >= K0).  `tail` > 0 copies the tail columns
//                                          x[r][L .. L + tail) to y[r][K0 .. K0 + tail): the rows form of csi_predict_samples ([B][L + nt] raw
//                                          rows -> [B][K0 + nt]).
// A workgroup takes tiles of CF_TILE pooled positions of one row: it stages the 2 CF_TILE samples of the tile plus the 3-sample halo on each
// side in LDS once (loaded into registers while the previous tile is computed), then every lane owns CPL consecutive channels (their 7 taps, bias and BN constants in registers) and walks the tile's
// positions.  A wave-instruction stores 64 x CPL contiguous outputs (CPL = 4 fp32 / 8 bf16: 16 bytes per lane): 64 outputs per input
// sample, about 20 (fp32) / 22 (bf16) VALU operations each (profiles/conv1d_model.txt has the counters).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csi {

constexpr int CONV_TAPS = 7;
constexpr int CONV_FILTERS = 128;
// the per-model constants on the device: taps [7][128] (cnn1d_1.kernel as stored), bias [128], BN scale [128], BN shift [128]
constexpr int CONV_PRM_FLOATS = CONV_TAPS * CONV_FILTERS + 3 * CONV_FILTERS;
constexpr int CF_THREADS = 256;
constexpr int CF_TILE = 64;          // pooled positions per tile: 128 samples + halo staged, 64 x 128 outputs written

struct ConvArgs {
    const float* x[2];       // raw planes (blockIdx.y selects one)
    void* y[2];              // feature planes: float or bf16
    const float* prm[2];     // CONV_PRM_FLOATS constants of the plane's model
    int64_t rows;
    int L;                   // samples per row (even)
    int ldx, ldy;            // row pitches in elements
    int tail;                // columns copied behind the features (rows form), else 0
};

__device__ __forceinline__ uint32_t cf_bf16_bits(float f) {      // round to nearest even (f2bf of gemm_bf16.hip.h)
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

// grid (blocks, planes), CF_THREADS lanes.  Every lane's CPL outputs sit on a 16-byte boundary: 16-byte aligned planes, ldy a multiple
// of CPL (K0 = 64 L is; the rows form's ldy = K0 + nt with nt a multiple of 4, csi_create) - launch_conv_frontend checks it
template <int CPL, bool BF16>
__global__ __launch_bounds__(CF_THREADS) void conv_frontend_kernel(ConvArgs a) {
    constexpr int LPU = CONV_FILTERS / CPL;           // lanes per pooled position
    constexpr int UPI = CF_THREADS / LPU;             // pooled positions per workgroup-instruction
    __shared__ float xs[2 * CF_TILE + 12];            // xs[i] = x[2 u0 - 4 + i] (0 outside the row)

    const int p = blockIdx.y;
    const float* __restrict__ x = a.x[p];
    const float* __restrict__ prm = a.prm[p];
    const int tid = threadIdx.x;
    const int c0 = (tid % LPU) * CPL, du0 = tid / LPU;
    float w[CONV_TAPS][CPL], bias[CPL], sc[CPL], sh[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
#pragma unroll
        for (int j = 0; j < CONV_TAPS; ++j) w[j][k] = prm[j * CONV_FILTERS + c0 + k];
        bias[k] = prm[CONV_TAPS * CONV_FILTERS + c0 + k];
        sc[k] = prm[(CONV_TAPS + 1) * CONV_FILTERS + c0 + k];
        sh[k] = prm[(CONV_TAPS + 2) * CONV_FILTERS + c0 + k];
    }
    const int L = a.L, Lh = L / 2;
    const int64_t K0 = (int64_t)Lh * CONV_FILTERS;
    const int tpr = (Lh + CF_TILE - 1) / CF_TILE;     // tiles per row
    const int64_t ntiles = a.rows * tpr;
    // lane tid < CF_XS holds sample tid of the window of its workgroup's NEXT tile in a register: the load is in flight while the
    // current tile is computed, and the window goes to LDS between the two barriers of the next trip
    constexpr int CF_XS = 2 * CF_TILE + 12;
    static_assert(CF_XS <= CF_THREADS, "one staged sample per lane");
    auto window = [&](int64_t t_) -> float {
        const int64_t r_ = t_ / tpr;
        const int t = 2 * (int)(t_ - r_ * tpr) * CF_TILE - 4 + tid;
        return (tid < CF_XS && t_ < ntiles && t >= 0 && t < L) ? x[r_ * a.ldx + t] : 0.f;
    };
    float nxt = window(blockIdx.x);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r = tile / tpr;
        const int u0 = (int)(tile - r * tpr) * CF_TILE;
        const float* xr = x + r * a.ldx;
        __syncthreads();                              // the previous tile's readers are done with xs
        if (tid < CF_XS) xs[tid] = nxt;
        __syncthreads();
        nxt = window(tile + gridDim.x);
        if (a.tail > 0 && u0 == 0) {
            for (int i = tid; i < a.tail; i += CF_THREADS) {
                const float v = xr[L + i];
                if constexpr (BF16) reinterpret_cast<uint16_t*>(a.y[p])[r * a.ldy + K0 + i] = (uint16_t)cf_bf16_bits(v);
                else reinterpret_cast<float*>(a.y[p])[r * a.ldy + K0 + i] = v;
            }
        }
        const int un = min(CF_TILE, Lh - u0);
#pragma unroll 2
        for (int du = du0; du < un; du += UPI) {
            // conv at t = 2u needs x[2u - 3 .. 2u + 3] = xs[2 du + 1 .. 2 du + 7], at t = 2u + 1 xs[2 du + 2 .. 2 du + 8]
            float v[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) v[i] = xs[2 * du + i];
            float out[CPL];
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                float e = bias[k], o = bias[k];
#pragma unroll
                for (int j = 0; j < CONV_TAPS; ++j) {
                    e = __builtin_fmaf(w[j][k], v[1 + j], e);
                    o = __builtin_fmaf(w[j][k], v[2 + j], o);
                }
                const float qe = __builtin_fmaf(fmaxf(e, 0.f), sc[k], sh[k]);
                const float qo = __builtin_fmaf(fmaxf(o, 0.f), sc[k], sh[k]);
                out[k] = 0.5f * (qe + qo);
            }
            const int64_t off = r * a.ldy + (int64_t)(u0 + du) * CONV_FILTERS + c0;
            if constexpr (BF16) {
                static_assert(CPL == 8, "bf16 features: 8 channels = one 16-byte store per lane");
                uint32_t q[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) q[k] = cf_bf16_bits(out[2 * k]) | (cf_bf16_bits(out[2 * k + 1]) << 16);
                *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(a.y[p]) + off) = make_uint4(q[0], q[1], q[2], q[3]);
            } else {
                static_assert(CPL == 4, "fp32 features: 4 channels = one 16-byte store per lane");
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.y[p]) + off) = make_float4(out[0], out[1], out[2], out[3]);
            }
        }
    }
}

}  // namespace csi
