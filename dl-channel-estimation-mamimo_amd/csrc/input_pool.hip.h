// input_pool.hip.h - the decimated-input models of the reference (massiveMIMO_CSI_prediction_DNN.py:30-31, 197-205): with
// --decimate_max / --decimate_avg the time-domain LTF goes through MaxPooling1D() / AveragePooling1D() (pool 2, stride 2, 'valid')
// before Flatten + Concatenate([.., seq_p]).  Layer 0 then sees len_ltf / 2 + nt inputs:
//     xp[k] = op(x[2k], x[2k+1]),  k < len_ltf / 2,  op = fmaxf (max) or 0.5f * (a + b) (avg; the same bits as keras' (a + b) / 2)
// computed in fp32.  The pilot columns are not pooled.
//
//   input_pool_kernel       [rows][len_ltf] fp32 -> [rows][len_ltf / 2] fp32 (the preambles of a call, a contiguous matrix): every lane
//                           reads two f32x4 (8 raw samples, 32 contiguous bytes) and writes one f32x4; UNR of them in flight per lane
//   input_pool_bf16_kernel  the same, pooled in fp32, then rounded to bf16 (nearest even, as f32_to_bf16_kernel rounds): replaces the
//                           cast pass of the bf16 layer-0 route
//   input_pool_rows_kernel  rows with a pilot tail ([B][len_ltf + nt] -> [B][len_ltf / 2 + nt]): csi_predict_samples
// The one-packet path pools inside its layer-0 loads (small_call.hip.h, POOL); training pools after the noise (train.hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csi {

enum { POOL_NONE = 0, POOL_MAX = 1, POOL_AVG = 2 };

typedef float ipool_f32x4 __attribute__((ext_vector_type(4)));

template <int MODE>
__device__ __forceinline__ float pool2(float a, float b) {
    if constexpr (MODE == POOL_MAX) return fmaxf(a, b);
    else return 0.5f * (a + b);
}

// two raw quads (8 consecutive samples) -> one pooled quad
template <int MODE>
__device__ __forceinline__ ipool_f32x4 pool_quads(const ipool_f32x4 a, const ipool_f32x4 b) {
    ipool_f32x4 r;
    r[0] = pool2<MODE>(a[0], a[1]);
    r[1] = pool2<MODE>(a[2], a[3]);
    r[2] = pool2<MODE>(b[0], b[1]);
    r[3] = pool2<MODE>(b[2], b[3]);
    return r;
}

__device__ __forceinline__ uint32_t ipool_bf16_bits(float f) {      // round to nearest even (f2bf of gemm_bf16.hip.h)
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

struct PoolArgs {
    const float* x[2];       // raw planes (blockIdx.y selects one)
    void* y[2];              // pooled planes: float or bf16
    size_t nq;               // pooled quads per plane = rows * len_ltf / 8
};

constexpr int IPOOL_THREADS = 256;
constexpr int IPOOL_UNR = 4;        // pooled quads per lane and trip: 8 loads of 16 bytes in flight per lane

// grid (blocks, planes).  A trip of a workgroup covers IPOOL_THREADS * IPOOL_UNR consecutive pooled quads: lane l of the
// workgroup owns quads base + u * IPOOL_THREADS + l, so every load and store instruction of a wave touches one contiguous run.
template <int MODE>
__global__ __launch_bounds__(IPOOL_THREADS) void input_pool_kernel(PoolArgs a) {
    const ipool_f32x4* __restrict__ x = reinterpret_cast<const ipool_f32x4*>(a.x[blockIdx.y]);
    ipool_f32x4* __restrict__ y = reinterpret_cast<ipool_f32x4*>(a.y[blockIdx.y]);
    const size_t step = (size_t)gridDim.x * IPOOL_THREADS * IPOOL_UNR;
    for (size_t base = (size_t)blockIdx.x * IPOOL_THREADS * IPOOL_UNR + threadIdx.x; base < a.nq; base += step) {
        ipool_f32x4 lo[IPOOL_UNR], hi[IPOOL_UNR];
#pragma unroll
        for (int u = 0; u < IPOOL_UNR; ++u) {
            const size_t q = base + (size_t)u * IPOOL_THREADS;
            if (q < a.nq) { lo[u] = x[2 * q]; hi[u] = x[2 * q + 1]; }
        }
#pragma unroll
        for (int u = 0; u < IPOOL_UNR; ++u) {
            const size_t q = base + (size_t)u * IPOOL_THREADS;
            if (q < a.nq) y[q] = pool_quads<MODE>(lo[u], hi[u]);
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(IPOOL_THREADS) void input_pool_bf16_kernel(PoolArgs a) {
    const ipool_f32x4* __restrict__ x = reinterpret_cast<const ipool_f32x4*>(a.x[blockIdx.y]);
    uint2* __restrict__ y = reinterpret_cast<uint2*>(a.y[blockIdx.y]);
    const size_t step = (size_t)gridDim.x * IPOOL_THREADS * IPOOL_UNR;
    for (size_t base = (size_t)blockIdx.x * IPOOL_THREADS * IPOOL_UNR + threadIdx.x; base < a.nq; base += step) {
        ipool_f32x4 lo[IPOOL_UNR], hi[IPOOL_UNR];
#pragma unroll
        for (int u = 0; u < IPOOL_UNR; ++u) {
            const size_t q = base + (size_t)u * IPOOL_THREADS;
            if (q < a.nq) { lo[u] = x[2 * q]; hi[u] = x[2 * q + 1]; }
        }
#pragma unroll
        for (int u = 0; u < IPOOL_UNR; ++u) {
            const size_t q = base + (size_t)u * IPOOL_THREADS;
            if (q < a.nq) {
                const ipool_f32x4 p = pool_quads<MODE>(lo[u], hi[u]);
                uint2 o;
                o.x = ipool_bf16_bits(p[0]) | (ipool_bf16_bits(p[1]) << 16);
                o.y = ipool_bf16_bits(p[2]) | (ipool_bf16_bits(p[3]) << 16);
                y[q] = o;
            }
        }
    }
}

// y[r][0..kp) = pool(x[r][0..2 kp)), y[r][kp..kp + tail) = x[r][2 kp..2 kp + tail)   (one thread per output element)
template <int MODE>
__global__ __launch_bounds__(256) void input_pool_rows_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy,
                                                              int rows, int kp, int tail) {
    const int w = kp + tail;
    const size_t total = (size_t)rows * w;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int r = (int)(i / w), k = (int)(i - (size_t)r * w);
        const float* xr = x + (size_t)r * ldx;
        y[(size_t)r * ldy + k] = k < kp ? pool2<MODE>(xr[2 * k], xr[2 * k + 1]) : xr[kp + k];
    }
}

}  // namespace csi
