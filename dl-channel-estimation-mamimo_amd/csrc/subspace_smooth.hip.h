// subspace_smooth.hip.h - delay-subspace smoother of a CSI tensor (csi_subspace_smooth[_device]):
//   y = Q diag(w) Q^H x   for every row x of 234 carriers of the [npkt][Nr][Nt][234] planes,
// Q [234][r] orthonormal (r <= 128), w [npkt][Nr][r] real (or none = ones).  An addition: the reference has no such estimator.
//
// One launch, one kernel.  A workgroup of 4 waves owns SB_ROWS = 32 whole rows - 32 x 936 bytes, contiguous in both planes and on a
// 16-byte boundary because the tile starts at an even row:
//   load     the x_re / x_im tile into LDS in 16-byte words, rows past the end of the call as zeros.  The row pitch stays 234 floats:
//            234 mod 64 = 42, so the 32 rows of an MFMA operand read fall into 32 different even banks and the second k of the
//            instruction into the odd ones.
//   stage 1  t^T[j][row] = sum_k conj(Q[k][j]) x[row][k] on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation): A = Q
//            (rank index on the rows of the tile), B = x (tile row on the column), two accumulators (re, im), four instructions per
//            two carriers.  K = 234 is 117 whole steps of 2 - nothing is padded or read past a row.  The r columns of Q are padded
//            with zeros to rp = whole tiles of 32; wave w takes rank tile w.  Up to rank 64 the idle waves take a share of the
//            carriers instead (rp = 32: four quarters, rp = 64: two halves) and the partial sums are added in ascending carrier
//            order in LDS - the split depends on the rank alone, so a row's bits depend on nothing but the row, Q and w.
//   weights  the pass that adds the partial sums multiplies by w[row / Nt][j] and leaves t^T in LDS, [j][row].
//   stage 2  y^T[k][row] = sum_j Q[k][j] t^T[j][row]: A = Q^T image [j][256] (carriers padded to 8 tiles of 32 with zeros), B = t^T
//            from LDS; wave w takes carrier tiles w and w + 4 against one read of t.  (r + 1) / 2 steps.
//   store    the accumulators go back into the x tile's LDS (carriers below 234 only) and out in 16-byte words.
// Because the whole tile is in LDS before anything is stored and no other workgroup touches these rows, out may be the input planes.
//
// Q is read from the two device images the context keeps (csi_subspace_set_basis) straight into the A operand: one coalesced
// 128-byte read per half wave and k.  Within a 32-row tile every element of Q is used by exactly one wave, once per stage, so a
// copy of Q in LDS would be written and read once - it would add LDS traffic and save no L2 read; the images are at most 502 KB
// and stay in L2.
// re / im planar everywhere, and compiled without the packed-fp32 instructions like the other MFMA-side kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csi {

constexpr int SB_N = 234;                  // data carriers of a row
constexpr int SB_NP = 256;                 // ... padded to 8 carrier tiles of 32 (stage 2 image)
constexpr int SB_MAX_RANK = 128;
constexpr int SB_ROWS = 32;                // rows per workgroup: the N of the MFMA
constexpr int SB_THREADS = 256;
constexpr int SB_STEPS = SB_N / 2;         // 117 k-steps of stage 1
constexpr int SB_U1 = 4;                    // stage 1: steps per block of Q loads in flight
constexpr int SB_TILE_FLOATS = SB_ROWS * SB_N;

typedef float sb_f32x16 __attribute__((ext_vector_type(16)));

struct SubspaceArgs {
    const float* x_re;      // [rows][234]
    const float* x_im;
    float* y_re;            // [rows][234]; may be x_re / x_im
    float* y_im;
    const float* w;         // [rows / nt][rank] or null (all ones)
    const float* qa_re;     // [234][rp]: Q, columns zero padded to rp
    const float* qa_im;
    const float* qb_re;     // [rp][256]: Q transposed, carriers zero padded to 256
    const float* qb_im;
    long long rows;
    int nt, rank, rp;
};

inline size_t subspace_lds_bytes(int rp) { return ((size_t)2 * SB_TILE_FLOATS + (size_t)2 * rp * SB_ROWS) * sizeof(float); }

#if defined(__HIP_DEVICE_COMPILE__)
#define SB_NO_PK __attribute__((target("no-packed-fp32-ops")))
#else
#define SB_NO_PK
#endif

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// tile <-> global in 16-byte words, n floats.  On the way in every lane has its SB_TILE_LD loads of both planes in flight before the
// first LDS store (one trip to memory per tile, not one per word), and the words past n become zeros.
constexpr int SB_TILE_V4 = SB_TILE_FLOATS / 4;
constexpr int SB_TILE_LD = (SB_TILE_V4 + SB_THREADS - 1) / SB_THREADS;

__device__ inline SB_NO_PK float4 sb_word_in(const float* g, int i, int n) {
    const int n4 = n >> 2;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i < n4) v = reinterpret_cast<const float4*>(g)[i];
    else if (i == n4) {                                 // a row count that is no multiple of 2: the last word is partly filled
        if (4 * i + 0 < n) v.x = g[4 * i + 0];
        if (4 * i + 1 < n) v.y = g[4 * i + 1];
        if (4 * i + 2 < n) v.z = g[4 * i + 2];
    }
    return v;
}
__device__ inline SB_NO_PK void sb_tile_in(float* l_re, float* l_im, const float* g_re, const float* g_im, int n) {
    float4 vr[SB_TILE_LD], vi[SB_TILE_LD];
#pragma unroll
    for (int u = 0; u < SB_TILE_LD; ++u) {
        const int i = threadIdx.x + u * SB_THREADS;
        vr[u] = sb_word_in(g_re, i, n);
        vi[u] = sb_word_in(g_im, i, n);
    }
#pragma unroll
    for (int u = 0; u < SB_TILE_LD; ++u) {
        const int i = threadIdx.x + u * SB_THREADS;
        if (i < SB_TILE_V4) {
            reinterpret_cast<float4*>(l_re)[i] = vr[u];
            reinterpret_cast<float4*>(l_im)[i] = vi[u];
        }
    }
}
__device__ inline SB_NO_PK void sb_tile_out(float* g, const float* lds, int n) {
    const int n4 = n >> 2;
    float4* g4 = reinterpret_cast<float4*>(g);
    const float4* l4 = reinterpret_cast<const float4*>(lds);
    for (int i = threadIdx.x; i < n4; i += SB_THREADS) g4[i] = l4[i];
    for (int i = 4 * n4 + threadIdx.x; i < n; i += SB_THREADS) g[i] = lds[i];
}

__global__ SB_NO_PK void __launch_bounds__(SB_THREADS) subspace_smooth_kernel(SubspaceArgs a) {
    extern __shared__ float sb_lds[];
    float* xs_re = sb_lds;                              // the x tile; then the partial sums of stage 1; then the y tile
    float* xs_im = sb_lds + SB_TILE_FLOATS;
    float* t_re = sb_lds + 2 * SB_TILE_FLOATS;          // t^T [rp][32]
    float* t_im = t_re + a.rp * SB_ROWS;
    const int rp = a.rp, rank = a.rank;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, h = lane >> 5;
    const long long row0 = (long long)blockIdx.x * SB_ROWS;
    const long long left = a.rows - row0;
    const int nrows = left < SB_ROWS ? (int)left : SB_ROWS;
    const int n = nrows * SB_N;
    const size_t off = (size_t)row0 * SB_N;

    sb_tile_in(xs_re, xs_im, a.x_re + off, a.x_im + off, n);
    __syncthreads();

    // ---- stage 1: rank tile jt, carrier steps [s0, s1) of this wave
    const int njt = rp >> 5;
    const int nparts = njt == 1 ? 4 : (njt == 2 ? 2 : 1);
    const int jt = nparts == 4 ? 0 : (nparts == 2 ? (wave & 1) : wave);
    const int part = nparts == 4 ? wave : (nparts == 2 ? (wave >> 1) : 0);
    const bool active = jt < njt;
    sb_f32x16 are, aim;
    for (int v = 0; v < 16; ++v) { are[v] = 0.0f; aim[v] = 0.0f; }
    if (active) {
        const int s0 = part * SB_STEPS / nparts, s1 = (part + 1) * SB_STEPS / nparts;
        const float* qr_p = a.qa_re + jt * 32 + col;
        const float* qi_p = a.qa_im + jt * 32 + col;
        const float* xr_p = xs_re + col * SB_N;
        const float* xi_p = xs_im + col * SB_N;
        // Q one block of SB_U1 steps ahead of the MFMAs that use it (16 instructions = 1024 cycles per block to cover the L2 latency);
        // addresses past the range are clamped and their values unused
        float qr[SB_U1], qi[SB_U1], nr[SB_U1], ni[SB_U1];
        for (int u = 0; u < SB_U1; ++u) {
            const int k = 2 * min(s0 + u, SB_STEPS - 1) + h;
            qr[u] = qr_p[(size_t)k * rp]; qi[u] = qi_p[(size_t)k * rp];
        }
        for (int s = s0; s < s1; s += SB_U1) {
            for (int u = 0; u < SB_U1; ++u) {
                const int k = 2 * min(s + SB_U1 + u, SB_STEPS - 1) + h;
                nr[u] = qr_p[(size_t)k * rp]; ni[u] = qi_p[(size_t)k * rp];
            }
            for (int u = 0; u < SB_U1; ++u) {
                if (s + u < s1) {
                    const int k = 2 * (s + u) + h;
                    const float xr = xr_p[k], xi = xi_p[k];
                    // t = conj(q) x:  re = qr xr + qi xi,  im = qr xi - qi xr
                    are = __builtin_amdgcn_mfma_f32_32x32x2f32(qr[u], xr, are, 0, 0, 0);
                    aim = __builtin_amdgcn_mfma_f32_32x32x2f32(qr[u], xi, aim, 0, 0, 0);
                    are = __builtin_amdgcn_mfma_f32_32x32x2f32(qi[u], xi, are, 0, 0, 0);
                    aim = __builtin_amdgcn_mfma_f32_32x32x2f32(-qi[u], xr, aim, 0, 0, 0);
                }
            }
            for (int u = 0; u < SB_U1; ++u) { qr[u] = nr[u]; qi[u] = ni[u]; }
        }
    }
    __syncthreads();                                    // every wave is done with the x tile
    // partial sums [part][re, im][rp][32] over the x tile.  Accumulator register v of this lane: rank index 32 jt + 8 (v / 4) + 4 h + v % 4
    if (active) {
        float* p_re = sb_lds + (size_t)(2 * part) * rp * SB_ROWS;
        float* p_im = p_re + rp * SB_ROWS;
        for (int v = 0; v < 16; ++v) {
            const int j = jt * 32 + 8 * (v >> 2) + 4 * h + (v & 3);
            p_re[j * SB_ROWS + col] = are[v];
            p_im[j * SB_ROWS + col] = aim[v];
        }
    }
    __syncthreads();
    // ---- partial sums in ascending carrier order, times w
    for (int e = threadIdx.x; e < rp * SB_ROWS; e += SB_THREADS) {
        float sr = sb_lds[e], si = sb_lds[rp * SB_ROWS + e];
        for (int p = 1; p < nparts; ++p) {
            sr += sb_lds[(size_t)(2 * p) * rp * SB_ROWS + e];
            si += sb_lds[(size_t)(2 * p + 1) * rp * SB_ROWS + e];
        }
        if (a.w) {
            const int j = e >> 5, row = e & 31;
            const float wv = (j < rank && row < nrows) ? a.w[(size_t)((row0 + row) / a.nt) * rank + j] : 1.0f;
            sr *= wv;
            si *= wv;
        }
        t_re[e] = sr;
        t_im[e] = si;
    }
    __syncthreads();

    // ---- stage 2: carrier tiles wave and wave + 4
    sb_f32x16 yre[2], yim[2];
    for (int u = 0; u < 2; ++u)
        for (int v = 0; v < 16; ++v) { yre[u][v] = 0.0f; yim[u][v] = 0.0f; }
    {
        const int nsteps = (rank + 1) >> 1;
        const float* qr_p = a.qb_re + wave * 32 + col;
        const float* qi_p = a.qb_im + wave * 32 + col;
        // Q one step (8 instructions = 512 cycles) ahead; the image has rp >= rank + 1 rows or the last step ends on row rank - 1
        float qr[2], qi[2], nr[2], ni[2];
        for (int u = 0; u < 2; ++u) { qr[u] = qr_p[(size_t)h * SB_NP + u * 128]; qi[u] = qi_p[(size_t)h * SB_NP + u * 128]; }
        for (int s = 0; s < nsteps; ++s) {
            const int j = 2 * s + h;
            const int jn = 2 * min(s + 1, nsteps - 1) + h;
            for (int u = 0; u < 2; ++u) { nr[u] = qr_p[(size_t)jn * SB_NP + u * 128]; ni[u] = qi_p[(size_t)jn * SB_NP + u * 128]; }
            const float tr = t_re[j * SB_ROWS + col], ti = t_im[j * SB_ROWS + col];
            for (int u = 0; u < 2; ++u) {
                // y = q t:  re = qr tr - qi ti,  im = qr ti + qi tr
                yre[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(qr[u], tr, yre[u], 0, 0, 0);
                yim[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(qr[u], ti, yim[u], 0, 0, 0);
                yre[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(-qi[u], ti, yre[u], 0, 0, 0);
                yim[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(qi[u], tr, yim[u], 0, 0, 0);
            }
            for (int u = 0; u < 2; ++u) { qr[u] = nr[u]; qi[u] = ni[u]; }
        }
    }
    // the partial sums were consumed in front of the last barrier: the tile space is free for y
    for (int u = 0; u < 2; ++u)
        for (int v = 0; v < 16; ++v) {
            const int k = (wave + 4 * u) * 32 + 8 * (v >> 2) + 4 * h + (v & 3);
            if (k < SB_N) {
                xs_re[col * SB_N + k] = yre[u][v];
                xs_im[col * SB_N + k] = yim[u][v];
            }
        }
    __syncthreads();
    sb_tile_out(a.y_re + off, xs_re, n);
    sb_tile_out(a.y_im + off, xs_im, n);
}
#endif

}  // namespace csi
