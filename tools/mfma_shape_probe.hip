// mfma_shape_probe.hip - does the f16 MFMA SHAPE change the clock the part holds on split (hi, lo) operands?
// Stand-alone (no library code).  Two kernels that differ only in the MFMA shape:
//     32:  v_mfma_f32_32x32x16_f16, the three-phase order of gemm_hs.hip.h (a_hi b_lo, a_hi b_hi, a_lo b_hi per sub-tile)
//     16:  v_mfma_f32_16x16x32_f16 on PAIRS of sub-tiles: fragment X = the hi planes of sub-tiles g and g + 1, Y = their
//          lo planes (one ds_read_b128 per 16-row tile, the lanes address two ring slots); X Y, X X, Y X per tile
// Same output tile per wave, same LDS image (64-byte rows: 16 hi halves, 16 lo halves, XOR swizzle by (row >> 2) & 3),
// same LDS read bytes and the same matrix-pipe cycles per flop; every operand is re-read from LDS with ds_read_b128 at
// every step, the fp32 accumulators stay live and are written out.  No barrier, no global traffic inside the loop.
// Geometries:  a = layer 0's: 8 waves per CU as 2 x 4, 128 rows x 64 columns per wave
//              b = the band kernel's: 4 waves per CU (one per SIMD), 64 rows x 128 features per wave
// Fills:       dense = hi = f16(x), lo = f16(x - hi) of full-range random fp32 x (what layer 0 multiplies)
//              half  = the same with half of the A values exactly zero (relu output: what the band kernel multiplies)
//              zero  = all zeros (control: both shapes must then rank by cycles, ratio ~1.00)
// Per arm: wall time per launch (device events around batches of back-to-back launches, >= 2 s per visit), shader
// cycles and the in-kernel clock (cycle counter over the 100 MHz wall counter, stamped once around the loop by wave 0 of
// every workgroup into a buffer of their own; median over the workgroups of the visit's last launch).  Arms are visited
// interleaved in one process: 32, 16, 32 again (A, B, A': |A - A'| is the spread of the probe itself) for every
// geometry and fill, several rounds; median and minimum over the rounds are reported.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/mfma_shape_probe.hip -o tools/mfma_shape_probe.bin
// Run:   mfma_shape_probe.bin [rounds = 3] [seconds per visit = 2.0]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cmath>
#include <vector>
#include <algorithm>
#include <random>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NSLOT = 4;            // sub-tiles (16 k-columns each) resident in LDS; the loop walks them round and round
constexpr int ROWF = 16;            // floats per image row (64 B)

template <int WR_, int WC_, int RT_, int CT_>
struct Geom {
    static constexpr int WR = WR_, WC = WC_, RT = RT_, CT = CT_;
    static constexpr int ROWS_A = WR * RT, ROWS_B = WC * CT, ROWS = ROWS_A + ROWS_B;
    static constexpr int THREADS = 64 * WR * WC;
    static constexpr int SLOTF = ROWS * ROWF;                     // floats per sub-tile
    static constexpr size_t LDS_BYTES = (size_t)NSLOT * SLOTF * 4;
    static constexpr size_t IMG_CHUNKS = (size_t)NSLOT * ROWS * 4; // 16-byte chunks of the image
    static constexpr size_t C_FLOATS = (size_t)ROWS_A * ROWS_B;   // output tile of a workgroup
};
using GeomA = Geom<2, 4, 128, 64>;
using GeomB = Geom<4, 1, 64, 128>;

__device__ __forceinline__ f16x8 ldsrd(const float* p) { return __builtin_bit_cast(f16x8, *reinterpret_cast<const f32x4*>(p)); }

// issue order inside a scheduling region: its LDS reads (they feed the NEXT region) in front of its MFMAs
#define reads_then_mfmas(nrd, nmf) do { __builtin_amdgcn_sched_group_barrier(0x100, nrd, 0); __builtin_amdgcn_sched_group_barrier(0x008, nmf, 0); } while (0)

// img: the logical image [slot][row][chunk 0..3 = hi k 0-7, hi k 8-15, lo k 0-7, lo k 8-15]; C: [workgroup][ROWS_A][ROWS_B];
// stamps: [workgroup][4] = cycle counter and wall counter before / after the loop; iters: trips of NSLOT sub-tiles
template <int SHAPE, class G>
__global__ __launch_bounds__(G::THREADS, 2) void probe_kernel(const uint4* __restrict__ img, float* __restrict__ C,
                                                              unsigned long long* __restrict__ stamps, int iters) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / G::WC, wc = wave % G::WC;

    for (int i = tid; i < (int)G::IMG_CHUNKS; i += G::THREADS) {
        const int row = (i >> 2) % G::ROWS, c = i & 3;
        reinterpret_cast<uint4*>(lds)[(i & ~3) | (c ^ ((row >> 2) & 3))] = img[i];
    }
    __syncthreads();

    float* cw = C + (size_t)blockIdx.x * G::C_FLOATS;
    unsigned long long t0 = 0, w0 = 0, t1 = 0, w1 = 0;

    if constexpr (SHAPE == 32) {
        constexpr int NA = G::RT / 32, NB = G::CT / 32;
        const int l31 = lane & 31, hi = lane >> 5;
        const int fswz = (l31 >> 2) & 3;
        int xo[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) xo[c] = ((2 * c + hi) ^ fswz) << 2;
        const float* ab = lds + (wr * G::RT + l31) * ROWF;
        const float* bb = lds + (G::ROWS_A + wc * G::CT + l31) * ROWF;
        f32x16 acc[NA][NB];
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        f16x8 a_hi[NA], a_lo[NA], b_hi[NB], b_lo[NB];
#pragma unroll
        for (int i = 0; i < NA; ++i) a_hi[i] = ldsrd(ab + i * 32 * ROWF + xo[0]);
#pragma unroll
        for (int j = 0; j < NB; ++j) b_lo[j] = ldsrd(bb + j * 32 * ROWF + xo[1]);
        t0 = __builtin_amdgcn_s_memtime();
        w0 = __builtin_amdgcn_s_memrealtime();
        __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0) alone: the loop's LDS waits stay counted
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int s = 0; s < NSLOT; ++s) {
                const int ns = (s + 1) % NSLOT;
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < NB; ++j) b_hi[j] = ldsrd(bb + s * G::SLOTF + j * 32 * ROWF + xo[0]);
#pragma unroll
                for (int i = 0; i < NA; ++i)
#pragma unroll
                    for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi[i], b_lo[j], acc[i][j], 0, 0, 0);
                reads_then_mfmas(NB, NA * NB);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < NA; ++i) a_lo[i] = ldsrd(ab + s * G::SLOTF + i * 32 * ROWF + xo[1]);
#pragma unroll
                for (int i = 0; i < NA; ++i)
#pragma unroll
                    for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi[i], b_hi[j], acc[i][j], 0, 0, 0);
                reads_then_mfmas(NA, NA * NB);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < NA; ++i) a_hi[i] = ldsrd(ab + ns * G::SLOTF + i * 32 * ROWF + xo[0]);
#pragma unroll
                for (int j = 0; j < NB; ++j) b_lo[j] = ldsrd(bb + ns * G::SLOTF + j * 32 * ROWF + xo[1]);
#pragma unroll
                for (int i = 0; i < NA; ++i)
#pragma unroll
                    for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo[i], b_hi[j], acc[i][j], 0, 0, 0);
                reads_then_mfmas(NA + NB, NA * NB);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        t1 = __builtin_amdgcn_s_memtime();
        w1 = __builtin_amdgcn_s_memrealtime();
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wr * G::RT + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    const int col = wc * G::CT + j * 32 + l31;
                    cw[(size_t)row * G::ROWS_B + col] = acc[i][j][r];
                }
    } else {
        // held operand: the one with 4 tiles of 16 (X and Y of a pair double-buffered: 64 registers); streamed operand: 8 tiles
        constexpr bool HELD_B = G::CT == 64;
        static_assert((HELD_B ? G::CT : G::RT) == 64 && (HELD_B ? G::RT : G::CT) == 128, "4 held and 8 streamed tiles");
        const int r16 = lane & 15, q = lane >> 4;
        const int swz = (r16 >> 2) & 3;
        int lo16[2];                                 // plane 0 = X (hi), 1 = Y (lo): k-octet q from slot g + (q & 1), chunk q >> 1
#pragma unroll
        for (int p = 0; p < 2; ++p) lo16[p] = (q & 1) * G::SLOTF + r16 * ROWF + (((2 * p + (q >> 1)) ^ swz) << 2);
        const float* ab = lds + (wr * G::RT) * ROWF;
        const float* bb = lds + (G::ROWS_A + wc * G::CT) * ROWF;
        const float* hb = HELD_B ? bb : ab;
        const float* sb = HELD_B ? ab : bb;
        f32x4 acc[8][4];
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int h = 0; h < 4; ++h) acc[s][h] = f32x4{0.f, 0.f, 0.f, 0.f};
        f16x8 HX[2][4], HY[2][4], SX[2], SY[2];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            HX[0][h] = ldsrd(hb + h * 16 * ROWF + lo16[0]);
            HY[0][h] = ldsrd(hb + h * 16 * ROWF + lo16[1]);
        }
        SX[0] = ldsrd(sb + lo16[0]);
        SY[0] = ldsrd(sb + lo16[1]);
        t0 = __builtin_amdgcn_s_memtime();
        w0 = __builtin_amdgcn_s_memrealtime();
        __builtin_amdgcn_s_waitcnt(0xC07F);
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int p = 0; p < NSLOT / 2; ++p) {
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    constexpr int NP = NSLOT / 2;
                    const int cur = s & 1;
                    const int ns = (s + 1) & 7, np = s == 7 ? (p + 1) % NP : p;
                    __builtin_amdgcn_sched_barrier(0);
                    SX[cur ^ 1] = ldsrd(sb + np * 2 * G::SLOTF + ns * 16 * ROWF + lo16[0]);
                    SY[cur ^ 1] = ldsrd(sb + np * 2 * G::SLOTF + ns * 16 * ROWF + lo16[1]);
                    if (s >= 4) {                    // the next pair's held fragments, one tile under each of the last four
                        HX[(p + 1) & 1][s - 4] = ldsrd(hb + ((p + 1) % NP) * 2 * G::SLOTF + (s - 4) * 16 * ROWF + lo16[0]);
                        HY[(p + 1) & 1][s - 4] = ldsrd(hb + ((p + 1) % NP) * 2 * G::SLOTF + (s - 4) * 16 * ROWF + lo16[1]);
                    }
#pragma unroll
                    for (int pr = 0; pr < 3; ++pr)
#pragma unroll
                        for (int h = 0; h < 4; ++h) {
                            const f16x8 sv = pr == 2 ? SY[cur] : SX[cur];
                            const f16x8 hv = pr == 0 ? HY[p & 1][h] : HX[p & 1][h];
                            acc[s][h] = HELD_B ? __builtin_amdgcn_mfma_f32_16x16x32_f16(sv, hv, acc[s][h], 0, 0, 0)
                                               : __builtin_amdgcn_mfma_f32_16x16x32_f16(hv, sv, acc[s][h], 0, 0, 0);
                        }
                    if (s >= 4) reads_then_mfmas(4, 12); else reads_then_mfmas(2, 12);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        t1 = __builtin_amdgcn_s_memtime();
        w1 = __builtin_amdgcn_s_memrealtime();
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int h = 0; h < 4; ++h)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int rt = HELD_B ? s : h, ct = HELD_B ? h : s;
                    const int row = wr * G::RT + rt * 16 + 4 * q + e;
                    const int col = wc * G::CT + ct * 16 + r16;
                    cw[(size_t)row * G::ROWS_B + col] = acc[s][h][e];
                }
    }
    if (tid == 0) {
        unsigned long long* st = stamps + (size_t)blockIdx.x * 4;
        st[0] = t0; st[1] = w0; st[2] = t1; st[3] = w1;
    }
}

// ---------------------------------------------------------------------------------------------------------------
static uint16_t f16_bits(float x) { _Float16 h = (_Float16)x; uint16_t b; __builtin_memcpy(&b, &h, 2); return b; }
static float f16_val(float x) { return (float)(_Float16)x; }

// fill 0 dense, 1 half of the A values zero, 2 all zero.  Scaled as the library scales: maximum in [2^12, 2^13)
template <class G>
static std::vector<uint16_t> make_image(int fill, unsigned seed) {
    std::vector<uint16_t> img(G::IMG_CHUNKS * 8, 0);
    if (fill == 2) return img;
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> ud(-1.f, 1.f);
    std::bernoulli_distribution coin(0.5);
    for (int s = 0; s < NSLOT; ++s)
        for (int r = 0; r < G::ROWS; ++r)
            for (int k = 0; k < 16; ++k) {
                float x = 8191.f * ud(rng);
                if (fill == 1 && r < G::ROWS_A && coin(rng)) x = 0.f;
                const float h = f16_val(x);
                uint16_t* row = img.data() + ((size_t)s * G::ROWS + r) * 32;
                row[k] = f16_bits(x);
                row[16 + k] = f16_bits(x - h);
            }
    return img;
}

static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v.empty() ? 0. : v[v.size() / 2]; }
static double minimum(const std::vector<double>& v) { return v.empty() ? 0. : *std::min_element(v.begin(), v.end()); }

struct Visit { double ms_med, ms_min, cycles, ghz; };

template <int SHAPE, class G>
static Visit visit(const uint4* d_img, float* d_c, unsigned long long* d_st, int nwg, int iters, double seconds) {
    auto kern = probe_kernel<SHAPE, G>;
    static bool once = false;
    if (!once) { CK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES)); once = true; }
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    constexpr int BATCH = 20;
    std::vector<double> per;
    double total = 0;
    while (total < seconds * 1e3) {
        CK(hipEventRecord(a));
        for (int i = 0; i < BATCH; ++i) hipLaunchKernelGGL(kern, dim3(nwg), dim3(G::THREADS), G::LDS_BYTES, 0, d_img, d_c, d_st, iters);
        CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        per.push_back(ms / BATCH); total += ms;
    }
    CK(hipGetLastError());
    std::vector<unsigned long long> st((size_t)nwg * 4);
    CK(hipMemcpy(st.data(), d_st, st.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> cyc, ghz;
    for (int w = 0; w < nwg; ++w) {
        const double dc = (double)(st[w * 4 + 2] - st[w * 4 + 0]), dw = (double)(st[w * 4 + 3] - st[w * 4 + 1]);
        cyc.push_back(dc);
        if (dw > 0) ghz.push_back(dc / dw * 0.1);
    }
    CK(hipEventDestroy(a)); CK(hipEventDestroy(b));
    return {median(per), minimum(per), median(cyc), median(ghz)};
}

template <class G>
static void run_geometry(const char* name, int rounds, double seconds, int nwg, int iters) {
    float* d_c; unsigned long long* d_st; uint4* d_img[3];
    CK(hipMalloc(&d_c, (size_t)nwg * G::C_FLOATS * 4));
    CK(hipMalloc(&d_st, (size_t)nwg * 4 * 8));
    for (int f = 0; f < 3; ++f) {
        const auto img = make_image<G>(f, 11 + f);
        CK(hipMalloc(&d_img[f], img.size() * 2));
        CK(hipMemcpy(d_img[f], img.data(), img.size() * 2, hipMemcpyHostToDevice));
    }
    const char* fills[3] = {"dense", "half", "zero"};
    const double flop = 2.0 * 3 * G::ROWS_A * G::ROWS_B * 16.0 * NSLOT * iters * nwg;      // three products per real k

    // the two shapes compute the same sums in another order: compare their outputs on the dense fill (2 trips)
    {
        std::vector<float> c32(G::C_FLOATS), c16(G::C_FLOATS);
        CK(hipFuncSetAttribute((const void*)probe_kernel<32, G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES));
        CK(hipFuncSetAttribute((const void*)probe_kernel<16, G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES));
        hipLaunchKernelGGL((probe_kernel<32, G>), dim3(nwg), dim3(G::THREADS), G::LDS_BYTES, 0, d_img[0], d_c, d_st, 2);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(c32.data(), d_c, c32.size() * 4, hipMemcpyDeviceToHost));
        hipLaunchKernelGGL((probe_kernel<16, G>), dim3(nwg), dim3(G::THREADS), G::LDS_BYTES, 0, d_img[0], d_c, d_st, 2);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(c16.data(), d_c, c16.size() * 4, hipMemcpyDeviceToHost));
        double e = 0, r = 0;
        for (size_t i = 0; i < c32.size(); ++i) { const double d = (double)c32[i] - c16[i]; e += d * d; r += (double)c32[i] * c32[i]; }
        printf("geometry %s: shapes agree to %.2e (norm-relative, dense fill, %d sub-tiles; 0 < expected ~1e-7)  |C| = %.3e\n", name,
               std::sqrt(e / std::max(r, 1e-300)), 2 * NSLOT, std::sqrt(r));
    }

    std::vector<Visit> res[3][3];        // [fill][arm A, B, A']
    for (int rd = 0; rd < rounds; ++rd)
        for (int f = 0; f < 3; ++f) {
            res[f][0].push_back(visit<32, G>(d_img[f], d_c, d_st, nwg, iters, seconds));
            res[f][1].push_back(visit<16, G>(d_img[f], d_c, d_st, nwg, iters, seconds));
            res[f][2].push_back(visit<32, G>(d_img[f], d_c, d_st, nwg, iters, seconds));
        }
    const char* arms[3] = {"A  32x32x16", "B  16x16x32", "A' 32x32x16"};
    for (int f = 0; f < 3; ++f) {
        double med[3];
        for (int a = 0; a < 3; ++a) {
            std::vector<double> m, mn, cy, gz;
            for (const Visit& v : res[f][a]) { m.push_back(v.ms_med); mn.push_back(v.ms_min); cy.push_back(v.cycles); gz.push_back(v.ghz); }
            med[a] = median(m);
            printf("geometry %s  fill %-5s  %s  ms/launch median %.4f min %.4f  Tflop/s %.1f  cycles %.0f  clock %.3f GHz   rounds:", name, fills[f],
                   arms[a], med[a], minimum(mn), flop / (med[a] * 1e-3) * 1e-12, median(cy), median(gz));
            for (double x : m) printf(" %.4f", x);
            printf("\n");
        }
        printf("geometry %s  fill %-5s  flop/s ratio 16 over 32: %.4f vs A, %.4f vs A'   A'/A spread %.4f\n", name, fills[f], med[0] / med[1],
               med[2] / med[1], med[2] / med[0]);
    }
    for (int f = 0; f < 3; ++f) CK(hipFree(d_img[f]));
    CK(hipFree(d_c)); CK(hipFree(d_st));
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 3;
    const double seconds = argc > 2 ? atof(argv[2]) : 2.0;
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    const int nwg = prop.multiProcessorCount;          // one workgroup per CU (the LDS image admits no second one)
    printf("%s  %d CUs  rounds %d  %.1f s per visit\n", prop.name, nwg, rounds, seconds);
    // trips of NSLOT sub-tiles: ~3 ms per launch (a: 1536, b: 768 matrix-pipe cycles per sub-tile and SIMD)
    run_geometry<GeomA>("a (8 waves, 128x64)", rounds, seconds, nwg, 800);
    run_geometry<GeomB>("b (4 waves, 64x128)", rounds, seconds, nwg, 1600);
    return 0;
}
