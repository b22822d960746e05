// beam_smooth.hip.h - beam-space smoother of a CSI tensor across the Tx antennas (csi_beam_*):
//   t_b[k] = sum_j conj(A[j][b]) x[j][k],   E[b] = (1 / 234) sum_k |t_b[k]|^2,   y_j[k] = sum_b A[j][b] w[b] t_b[k]
// for every (packet, rx) plane x [Nt][234] of the [npkt][Nr][Nt][234] planes, A [Nt][nb] orthonormal (nb <= Nt <= 128), w
// [npkt][Nr][nb] real (or none = ones).  An addition: the reference has no such estimator.  The antenna-domain counterpart of
// subspace_smooth.hip.h: there the products run along the carriers of a row, here along the antennas of a carrier.
//
// One work item = one wave = (plane, tile of 32 carriers): 8 tiles per plane, the last one holds carriers 224 .. 233 and masks the
// rest.  The item needs every antenna of its 32 carriers and nothing else, so the whole chain stays in the registers of the wave:
//   stage 1  t[b][c] = sum_j conj(A[j][b]) x[j][c] on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation): the A operand
//            is the image a1 [Ntp][nbp] (beam on the rows of the tile: one coalesced 128-byte read per half wave and step), the B
//            operand x[2s + h][c] straight from the caller's plane - the carriers are the contiguous axis, 128 bytes per half wave.
//            Antennas past Nt and carriers past 234 are masked to zero in the load, never read.  Steps s = 0 .. ceil(Nt / 2) - 1 in
//            ascending order, x and A of BM_U steps in flight in front of the instructions that use them.
//   weights  accumulator register v of lane (c, h) holds beam 32 bt + 8 (v / 4) + 4 h + v % 4: multiplied by w of that beam.
//   stage 2  y[i][c] = sum_b A[i][b] t[b][c].  The B operand of an MFMA step wants t of two beams, one in each half wave, in the
//            lane of carrier c: register v holds exactly that, beams 32 bt + 8 (v / 4) + v % 4 (h = 0) and that + 4 (h = 1).  So step
//            (bt, v) takes its B operand from the accumulators of stage 1 as they are - t never leaves the registers - and the A operand
//            from the image a2 [nbp][Ntp] at the row of the lane's own beam.  Steps in ascending (bt, v), those whose beams all lie
//            past nb skipped: the order of every sum depends on Nt and nb alone.
//   store    register v of antenna tile it is antenna 32 it + 8 (v / 4) + 4 h + v % 4, carrier c: 128 bytes per half wave.
// A wave reads its 32 carriers of every antenna before it stores any of them and no other wave touches these carriers, so out may be the
// input planes.  No LDS in the smoother.
//
// beam_power_kernel: one workgroup of 8 waves per plane, wave kt = carrier tile kt through the same stage 1; |t|^2 summed over the 32
// carriers of the tile by a butterfly in a fixed order, the 8 tile sums added in ascending tile order by one lane per beam, divided by
// 234.  Masked carriers contribute exact zeros.  No atomics: the bits of E depend on the plane, Nt and nb alone.
// beam_wiener_weights_kernel: w = 1 - v / E where E > v, 0 elsewhere (E = 0 and NaN fall under "elsewhere").
//
// The template parameter TT is the number of 32-tiles the accumulators are laid out for (1, 2 or 4: max of the antenna and the beam
// tiles); tiles past the actual count are skipped by wave-uniform branches.
// re / im planar everywhere, and compiled without the packed-fp32 instructions like the other MFMA-side kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csi {

constexpr int BM_N = 234;                  // data carriers of a row
constexpr int BM_KT = 8;                   // carrier tiles of 32 per plane (the last one: 10 carriers)
constexpr int BM_MAX_NT = 128;
constexpr int BM_THREADS = 256;            // smoother: 4 independent waves
constexpr int BM_POWER_THREADS = 64 * BM_KT;      // power pass: the 8 carrier tiles of one plane
constexpr int BM_U = 4;                    // stage 1: steps per block of loads in flight

typedef float bm_f32x16 __attribute__((ext_vector_type(16)));

struct BeamArgs {
    const float* x_re;      // [planes][nt][234]
    const float* x_im;
    float* y_re;            // [planes][nt][234]; may be x_re / x_im
    float* y_im;
    const float* w;         // [planes][nb] or null (all ones)
    float* power;           // [planes][nb] (power pass)
    const float* a1_re;     // [ntp][nbp]: A, rows and columns zero padded to whole tiles
    const float* a1_im;
    const float* a2_re;     // [nbp][ntp]: A transposed, padded the same way
    const float* a2_im;
    long long planes;
    int nt, nb, ntp, nbp;
};

#if defined(__HIP_DEVICE_COMPILE__)
#define BM_NO_PK __attribute__((target("no-packed-fp32-ops")))
#else
#define BM_NO_PK
#endif

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// stage 1 of one (plane, carrier tile): tre / tim [bt][v] = t of beam 32 bt + 8 (v / 4) + 4 h + v % 4 at carrier 32 kt + col
template <int TT>
__device__ inline BM_NO_PK void bm_stage1(const BeamArgs& a, const float* xr_p, const float* xi_p, bool cvalid, int col, int h, bm_f32x16 (&tre)[TT],
                                          bm_f32x16 (&tim)[TT]) {
    const int nt = a.nt, nbp = a.nbp, nbt = nbp >> 5;
    const int nsteps = (nt + 1) >> 1;                   // the images have ntp >= 2 nsteps rows
#pragma unroll
    for (int bt = 0; bt < TT; ++bt)
#pragma unroll
        for (int v = 0; v < 16; ++v) { tre[bt][v] = 0.0f; tim[bt][v] = 0.0f; }
    float xr[BM_U], xi[BM_U], ar[BM_U][TT], ai[BM_U][TT];
    float nxr[BM_U], nxi[BM_U], nar[BM_U][TT], nai[BM_U][TT];
    // a block of BM_U steps: addresses past the last step are clamped and their values unused; antennas past nt and carriers past
    // 234 are not read
#define BM_LOAD_BLOCK(S0, XR, XI, AR, AI)                                                                     \
    _Pragma("unroll") for (int u = 0; u < BM_U; ++u) {                                                        \
        const int s_ = (S0) + u < nsteps ? (S0) + u : nsteps - 1;                                             \
        const int j_ = 2 * s_ + h;                                                                            \
        const bool ok_ = cvalid && j_ < nt;                                                                   \
        XR[u] = ok_ ? xr_p[(size_t)j_ * BM_N] : 0.0f;                                                         \
        XI[u] = ok_ ? xi_p[(size_t)j_ * BM_N] : 0.0f;                                                         \
        _Pragma("unroll") for (int bt = 0; bt < TT; ++bt) {                                                   \
            const int bo_ = bt < nbt ? bt * 32 : 0;                                                           \
            AR[u][bt] = a.a1_re[(size_t)j_ * nbp + bo_ + col];                                                \
            AI[u][bt] = a.a1_im[(size_t)j_ * nbp + bo_ + col];                                                \
        }                                                                                                     \
    }
    BM_LOAD_BLOCK(0, xr, xi, ar, ai)
    for (int s = 0; s < nsteps; s += BM_U) {
        BM_LOAD_BLOCK(s + BM_U, nxr, nxi, nar, nai)
#pragma unroll
        for (int u = 0; u < BM_U; ++u) {
            if (s + u < nsteps) {
#pragma unroll
                for (int bt = 0; bt < TT; ++bt) {
                    if (bt < nbt) {
                        // t = conj(a) x:  re = ar xr + ai xi,  im = ar xi - ai xr
                        tre[bt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[u][bt], xr[u], tre[bt], 0, 0, 0);
                        tim[bt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[u][bt], xi[u], tim[bt], 0, 0, 0);
                        tre[bt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ai[u][bt], xi[u], tre[bt], 0, 0, 0);
                        tim[bt] = __builtin_amdgcn_mfma_f32_32x32x2f32(-ai[u][bt], xr[u], tim[bt], 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < BM_U; ++u) {
            xr[u] = nxr[u]; xi[u] = nxi[u];
#pragma unroll
            for (int bt = 0; bt < TT; ++bt) { ar[u][bt] = nar[u][bt]; ai[u][bt] = nai[u][bt]; }
        }
    }
#undef BM_LOAD_BLOCK
}

template <int TT>
__global__ BM_NO_PK void __launch_bounds__(BM_THREADS) beam_smooth_kernel(BeamArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, h = lane >> 5;
    const long long item = (long long)blockIdx.x * (BM_THREADS / 64) + wave;      // (plane, carrier tile)
    const long long plane = item / BM_KT;
    if (plane >= a.planes) return;                      // wave-uniform; the kernel has no barrier
    const int kt = (int)(item % BM_KT);
    const int cidx = kt * 32 + col;
    const bool cvalid = cidx < BM_N;
    const int nt = a.nt, nb = a.nb, ntp = a.ntp;
    const int nbt = a.nbp >> 5, ntt = ntp >> 5;
    const size_t off = (size_t)plane * nt * BM_N + (cvalid ? cidx : 0);

    bm_f32x16 tre[TT], tim[TT];
    bm_stage1<TT>(a, a.x_re + off, a.x_im + off, cvalid, col, h, tre, tim);

    if (a.w) {
        const float* w_p = a.w + (size_t)plane * nb;
#pragma unroll
        for (int bt = 0; bt < TT; ++bt)
            if (bt < nbt) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int b = bt * 32 + 8 * (v >> 2) + 4 * h + (v & 3);
                    const float wv = b < nb ? w_p[b] : 0.0f;      // t of a padded beam is an exact zero already
                    tre[bt][v] *= wv;
                    tim[bt][v] *= wv;
                }
            }
    }

    bm_f32x16 yre[TT], yim[TT];
#pragma unroll
    for (int it = 0; it < TT; ++it)
#pragma unroll
        for (int v = 0; v < 16; ++v) { yre[it][v] = 0.0f; yim[it][v] = 0.0f; }
#pragma unroll
    for (int bt = 0; bt < TT; ++bt) {
        if (bt < nbt) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int b0 = bt * 32 + 8 * (v >> 2) + (v & 3);       // the beam of the h = 0 half; the h = 1 half holds b0 + 4
                if (b0 < nb) {
                    const size_t row = (size_t)(b0 + 4 * h) * ntp + col;       // b0 + 4 < nbp: a padded row of zeros at the worst
                    const float tr = tre[bt][v], ti = tim[bt][v];
#pragma unroll
                    for (int it = 0; it < TT; ++it) {
                        if (it < ntt) {
                            const float qr = a.a2_re[row + it * 32], qi = a.a2_im[row + it * 32];
                            // y = a t:  re = ar tr - ai ti,  im = ar ti + ai tr
                            yre[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(qr, tr, yre[it], 0, 0, 0);
                            yim[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(qr, ti, yim[it], 0, 0, 0);
                            yre[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(-qi, ti, yre[it], 0, 0, 0);
                            yim[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(qi, tr, yim[it], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }

    if (cvalid) {
        float* yr_p = a.y_re + off;
        float* yi_p = a.y_im + off;
#pragma unroll
        for (int it = 0; it < TT; ++it)
            if (it < ntt) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int i = it * 32 + 8 * (v >> 2) + 4 * h + (v & 3);
                    if (i < nt) {
                        yr_p[(size_t)i * BM_N] = yre[it][v];
                        yi_p[(size_t)i * BM_N] = yim[it][v];
                    }
                }
            }
    }
}

template <int TT>
__global__ BM_NO_PK void __launch_bounds__(BM_POWER_THREADS) beam_power_kernel(BeamArgs a) {
    __shared__ float part[BM_KT][BM_MAX_NT];            // per carrier tile: sum of |t|^2 over its carriers
    const int lane = threadIdx.x & 63, kt = threadIdx.x >> 6;
    const int col = lane & 31, h = lane >> 5;
    const long long plane = blockIdx.x;
    const int cidx = kt * 32 + col;
    const bool cvalid = cidx < BM_N;
    const int nt = a.nt, nb = a.nb;
    const int nbt = a.nbp >> 5;
    const size_t off = (size_t)plane * nt * BM_N + (cvalid ? cidx : 0);

    bm_f32x16 tre[TT], tim[TT];
    bm_stage1<TT>(a, a.x_re + off, a.x_im + off, cvalid, col, h, tre, tim);
#pragma unroll
    for (int bt = 0; bt < TT; ++bt)
        if (bt < nbt) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                float p = tre[bt][v] * tre[bt][v] + tim[bt][v] * tim[bt][v];
                // the 32 carriers of the tile: a butterfly inside the half wave, the same order in every call
                for (int m = 1; m < 32; m <<= 1) p += __shfl_xor(p, m, 64);
                if (col == 0) part[kt][bt * 32 + 8 * (v >> 2) + 4 * h + (v & 3)] = p;
            }
        }
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += BM_POWER_THREADS) {
        float s = part[0][b];
        for (int t = 1; t < BM_KT; ++t) s += part[t][b];
        a.power[(size_t)plane * nb + b] = s / (float)BM_N;
    }
}

// w = 1 - v / E where E > v, 0 elsewhere: one element of w per lane, v per plane
__global__ BM_NO_PK void __launch_bounds__(256) beam_wiener_weights_kernel(const float* power, const float* err_var, float* w, long long n, int nb) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float e = power[i], v = err_var[i / nb];
    w[i] = e > v ? 1.0f - v / e : 0.0f;
}
#endif

}  // namespace csi
