// csi_band.hpp - host side of the fused band kernel (gemm_hs_band.hip.h, band_kernel_gen.py, band4_kernel_gen.py) for both arithmetic
// modes: everything between "the caller has a BandArgs" and "the launches are queued" - the kernel table of the context, which form
// serves a call and in how many column splits (band_plan), and the launches themselves (band_run).  A new form gets a BandForm, a name
// in BAND_KERNEL_NAMES and its rule in band_plan.
#pragma once
#include "csi_context.hpp"

namespace {

// the code object embedded at build time
#if __has_include("band8_hsaco.inc")
#include "band8_hsaco.inc"
#define CSI_HAVE_BAND8 1
#else
#warning "band8_hsaco.inc not found: this build has NO fused band kernel (the separate pair + regressor kernels serve every call; option band_available reads 0).  _lib.build_library() generates it: band_kernel_gen.py -> clang -x assembler -mcpu=gfx950 -> ld.lld"
#endif

constexpr const char* BAND_KERNEL_NAMES[2][BAND_FORMS] = {
    {"csi_band8", "csi_band8_nostage", "csi_band8_cs", "csi_band4", "csi_band4_cs"},
    {"csi_band8_bf16", "csi_band8_bf16_nostage", "csi_band8_bf16_cs", "csi_band4_bf16", "csi_band4_bf16_cs"}};
// the register-blocked forms are workgroups of 4 waves (band4_kernel_gen.py) and stream PRE-TILED weights (band4_prepare), the others of 8 on the plain ones
constexpr unsigned BAND4_THREADS = 256;
inline bool band_tiled(const BandKernel& k) { return k.threads == BAND4_THREADS; }

// The kernel table of the context, loaded with the code object on first use.  false: this context has no band kernel (a build without the
// code object, or it did not load - not fatal: the separate kernels serve the call).
bool band_load(csi_ctx* c) {
#ifdef CSI_HAVE_BAND8
    if (c->band_failed) return false;
    if (c->band_mod) return true;
    // timing experiments (tools/): CSI_BAND8_HSACO = a code object built by tools/build_band8.sh (every ablation variant of the generators),
    // CSI_BAND8_NAME / CSI_BAND8_BF16_NAME = the variant that takes the place of the 8-wave staged kernel of its mode; one named csi_band4* is a
    // register-blocked form: 256 threads, tiled weights.
    // Honoured only together with CSI_DEBUG_HOOKS=1: a production process never loads a code object named by its environment.
    const char* hooks = std::getenv("CSI_DEBUG_HOOKS");
    const char* ext = hooks && hooks[0] == '1' ? std::getenv("CSI_BAND8_HSACO") : nullptr;
    const char* hooked[2] = {ext ? std::getenv("CSI_BAND8_NAME") : nullptr, ext ? std::getenv("CSI_BAND8_BF16_NAME") : nullptr};
    bool ok = (ext && *ext ? hipModuleLoad(&c->band_mod, ext) : hipModuleLoadData(&c->band_mod, band8_hsaco)) == hipSuccess;
    for (int bf16 = 0; bf16 < 2 && ok; ++bf16)
        for (int f = 0; f < BAND_FORMS && ok; ++f) {
            const char* name = f == BAND_EIGHT && hooked[bf16] ? hooked[bf16] : BAND_KERNEL_NAMES[bf16][f];
            BandKernel& k = c->band_kernel[bf16][f];
            k.threads = std::strncmp(name, "csi_band4", 9) == 0 ? BAND4_THREADS : (unsigned)BAND8_THREADS;
            if (hipModuleGetFunction(&k.fn, c->band_mod, name) != hipSuccess) {
                (void)hipGetLastError();
                k.fn = nullptr;
                ok = f > BAND_EIGHT_NOSTAGE;       // the two 8-wave unsplit forms are required; an external code object may lack the others
            }
        }
    if (!ok) {
        (void)hipGetLastError();           // not fatal - and not left pending: the separate kernels that serve the call check the thread's last error
        c->band_failed = true;
        for (auto& mode : c->band_kernel)
            for (BandKernel& k : mode) k.fn = nullptr;
    }
    return ok;
#else
    return false;
#endif
}

// Static part of "the column-split band kernel serves this model's per-pair layers" (band8_serves + band8_staged + band8_splits on
// the shapes alone): with it a call of a few hundred pair rows is faster on the split engine than on the fp32 MFMA kernels -
// 5 ... 20 packets of the shipped shape 136-142 us against 155-260 (profiles/r05_band_split_probe.txt)
bool band_split_static_ok(csi_ctx* c, const Model& m) {
    const csi_config& cf = c->cfg;
    if (cf.n_hidden != 2 || !c->hs_band || c->hs_band == 3 || c->hs_fuse_regressor || c->band_split == 0 || c->band_split == 1 ||
        c->force_pair_tile == 128)
        return false;
    if (m.layers.size() < 3 || !m.layers[2].Wh_p) return false;
    const int h1 = cf.hidden[0], n1 = cf.hidden[1];
    if (cf.nt < 16 || cf.nt > 128 || h1 < 128 || (h1 % 64) != 0 || (n1 % 512) != 0 || n1 > BAND8_MAX_N1 || cf.n_out < 1 || cf.n_out > 256) return false;
    return band_load(c) && c->band_kernel[0][BAND_EIGHT_CS].fn != nullptr;
}

// The register-blocked band kernels (band4_kernel_gen.py) stream PRE-TILED weights: built once per model at first use (band4_tile_kernel), then the
// argument record's W1 / W2p point at the tiled copies.  bf16: sub-tiles of 32 k, 8 regressor fragments per column step; split-f16: 16 k, 16 fragments.
int band4_prepare(csi_ctx* c, Model& m, BandArgs& ba, bool bf16) {
    if (!m.tiled_ok) {
        const int ncol = ba.N1 / 256, nsub = ba.K1 / (bf16 ? 32 : 16), nq = bf16 ? 8 : 16;
        const size_t b1 = (size_t)(ncol * nsub + 4) * BAND_SLOT_BYTES, b2 = (size_t)ncol * nq * BAND_SLOT_BYTES;
        if (b1 >= 0x7fffffffull) return fail(c, CSI_ERR_INVALID_ARG, "band weights of %zu bytes: beyond what the tiled copy addresses", b1);
        if ((!m.Wt1 && hipMalloc((void**)&m.Wt1, b1) != hipSuccess) || (!m.Wt2 && hipMalloc((void**)&m.Wt2, b2) != hipSuccess))
            return fail(c, CSI_ERR_NOMEM, "device allocation of the tiled band weights failed");
        hipLaunchKernelGGL(band4_tile_kernel, dim3(512), dim3(256), 0, c->stream, ba.W1, ba.ldb1, ncol, nsub, 0, 4, m.Wt1);
        hipLaunchKernelGGL(band4_tile_kernel, dim3(512), dim3(256), 0, c->stream, ba.W2p, ba.ldb2, ncol, nq, bf16 ? 1 : 2, 0, m.Wt2);
        HIP_TRY(c, hipGetLastError());
        m.tiled_ok = true;
    }
    ba.W1 = m.Wt1;
    ba.W2p = m.Wt2;
    return CSI_OK;
}

// What band_run queues for one call: ONE unsplit launch; the whole call in `splits` column splits; or the full rounds unsplit and the
// rows from tail_row0 on in tail_splits column splits.
struct BandPlan {
    int splits = 1;
    int tail_splits = 0;
    long tail_row0 = 0;
    bool blocked = false;        // the unsplit launch takes the register-blocked form
    bool blocked_cs = false;     // the column-split launch (of the whole call or of the tail) takes it
};

// Column splits of a call of `bands` bands: a band is one workgroup's work for ~200 us, so a call with fewer bands than CUs leaves
// CUs idle for that long - 2 or 4 workgroups per band, each over N1 / splits hidden features, fill them ("band_split";
// profiles/r05_band_split_probe.txt: 24 packets 248 -> 149 us, 64 packets 299 -> 251 us)
int band8_splits(const csi_ctx* c, const BandArgs& ba, bool bf16, size_t part_capacity_floats) {
    if (!c->band_kernel[bf16][BAND_EIGHT_CS].fn || c->band_split == 0 || c->band_split == 1) return 1;
    const long bands = (ba.M + BAND_ROWS - 1) / BAND_ROWS;
    int S = 1;
    if (c->band_split > 1) {
        S = c->band_split;
    } else {
        const long in_flight = bands * std::max(c->models_in_flight, 1);
        while (S < 4 && in_flight * (2 * S) <= 256) S *= 2;
        // a second round of workgroups that is at most a quarter full (129 ... 160 packets of the shipped shape): half-size workgroups
        // fill it better - 144 packets 502 -> 460 us, 160: 511 -> 476; from 192 packets on the split only costs (profiles/r05_band_split_probe.txt)
        if (S == 1 && in_flight > 256 && in_flight <= 320) S = 2;
    }
    while (S > 1 && (ba.N1 % (256 * S)) != 0) S >>= 1;
    // refused: partial outputs beyond the caller's buffer or the kernel's 32-bit offsets, weights beyond its 31-bit ones
    const unsigned long long part = (unsigned long long)(S - 1) * (unsigned long long)ba.M * (unsigned long long)ba.ldo;
    if (S > 1 && (part > part_capacity_floats || part * 4ull >= 0xffffffffull || (unsigned long long)ba.N1 * ba.ldb1 * 2ull >= 0x7fffffffull)) return 1;
    return S;
}

// "band_tail_split" (round 6): one workgroup per CU computes a band for 75-190 us, so a call of `bands` bands runs in ceil(bands / CUs) rounds and a last
// round of a few bands costs a whole one (configs[2]: 10 000 bands = 39 rounds + 16 bands = 2.5 % of the kernel's time for 0.16 % of the work).  When that
// round holds at most half (a quarter) of the CUs' worth of bands it is launched separately in 2 (4) column splits - the rows of the full rounds through
// the unsplit kernel, the rest through the column-split one on shifted operand pointers.  Returns the split count of the tail (0: one launch) and its first row.
int band_tail_splits(const csi_ctx* c, const BandArgs& ba, bool bf16, size_t part_capacity_floats, long* row0) {
    // measured (tools/band_tail_ab.py, profiles/r06_band_probe.txt (G)): fp32 contexts -2.8 ... -3.2 % per call where it applies (2100 / 2600 / 3100 / 4150 packets of the
    // shipped shape); bf16 contexts 0 ... +1 % (bands of 75 us backfill the last round well enough; the 8-wave split kernels and the extra sum eat the rest): fp32 only
    if (bf16) return 0;
    if (!c->band_tail_split || c->models_in_flight > 1 || c->band_split == 0 || c->band_split == 1) return 0;
    if (!c->band_kernel[bf16][BAND_EIGHT_CS].fn || ba.ldo != ba.n2) return 0;
    const long ncu = std::max(c->n_cu, 1), bands = (ba.M + BAND_ROWS - 1) / BAND_ROWS;
    const long full = bands / ncu * ncu, tail = bands - full;
    if (full < ncu || tail == 0) return 0;
    int S = 0;
    for (int s = 4; s >= 2; s >>= 1)
        if (tail * s <= ncu && (ba.N1 % (256 * s)) == 0) { S = s; break; }
    const long r0 = full * BAND_ROWS;
    if (!S || ba.nt < 1 || (r0 % ba.nt) != 0) return 0;
    const unsigned long long part = (unsigned long long)(S - 1) * (unsigned long long)(ba.M - r0) * (unsigned long long)ba.ldo;
    if (part > part_capacity_floats || (unsigned long long)ba.N1 * ba.ldb1 * 2ull >= 0x7fffffffull) return 0;
    *row0 = r0;
    return S;
}

// Which launches serve the call `ba` of a context whose table is loaded; part_capacity_floats = room for the partial outputs of column
// splits.  No HIP call.
BandPlan band_plan(const csi_ctx* c, const BandArgs& ba, bool bf16, bool staged, size_t part_capacity_floats) {
    BandPlan p;
    if (!staged) return p;          // the forms with per-lane global loads of L0 / T: one launch of the 8-wave kernel
    // round 6: the register-blocked forms (band4_kernel_gen.py: 4 waves x 512 registers, every weight fragment against two row groups) serve the
    // staged shapes on the same operands, their weight streams pre-tiled once per model ("band4" = 0: the 8-wave forms; A/B)
    const bool four = c->band4 && c->band_kernel[bf16][BAND_FOUR].fn;
    const bool four_cs = four && c->band_kernel[bf16][BAND_FOUR_CS].fn;
    if (ba.ldo == ba.n2) p.splits = band8_splits(c, ba, bf16, part_capacity_floats);
    if (p.splits > 1) {
        // 4 splits always take the 8-wave form (measured, tools/regime_probe.py band4=1 / 0 alternating: 2 splits - 64 packets - 192 against 195 us, 128 packets
        // unsplit 304 against 315; 4 splits - 24 packets - 120 against 117 us: a quarter band on four waves has less to hide its waits behind)
        p.blocked_cs = four_cs && p.splits == 2;
        return p;
    }
    p.blocked = four;
    p.tail_splits = band_tail_splits(c, ba, bf16, part_capacity_floats, &p.tail_row0);
    p.blocked_cs = four_cs && p.tail_splits == 2;
    return p;
}

int band_launch(csi_ctx* c, const BandKernel& k, const BandArgs& ba, double flops, double bytes) {
    ++c->band_launches;
    c->band4_launches += band_tiled(k);      // a csi_band4* function (band_load: 256 threads <=> that name)
    ProfScope ps(c, K_PAIR_DENSE, flops, bytes);
    Band8Args a8 = band8_args(ba);
    size_t sz = sizeof(a8);
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a8, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
    HIP_TRY(c, hipModuleLaunchKernel(k.fn, (unsigned)((ba.M + BAND_ROWS - 1) / BAND_ROWS), 1, 1, k.threads, 1, 1, 0, c->stream, nullptr, extra));
    return CSI_OK;
}

// the column-split launch: grid (bands, S), split y over N1 / S hidden features (a register-blocked form: ba.W1 / W2p are the tiled copies of
// the WHOLE layer, split y starts at its own column steps); partial outputs of splits 1 .. in `part`, added to split 0's output in split order
int band_launch_split(csi_ctx* c, const BandKernel& k, const BandArgs& ba, int S, float* part, double flops, double bytes, int kid) {
    ++c->band_launches;
    c->band4_launches += band_tiled(k);
    ++c->band_split_launches;
    BandArgs one = ba;
    one.N1 = ba.N1 / S;
    Band8ArgsCs a{};
    a.a = band8_args(one);
    a.part = part;
    size_t sz = sizeof(a);
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
    {
        ProfScope ps(c, kid, flops, bytes);
        HIP_TRY(c, hipModuleLaunchKernel(k.fn, (unsigned)((ba.M + BAND_ROWS - 1) / BAND_ROWS), (unsigned)S, 1, k.threads, 1, 1, 0, c->stream, nullptr, extra));
    }
    const size_t n = (size_t)ba.M * ba.ldo;
    ProfScope ps(c, K_SPLITK_REDUCE, (double)(S - 1) * n, 4.0 * (S + 1) * (double)n);
    hipLaunchKernelGGL(band_split_sum_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, c->stream, ba.out, part, n, n, S - 1);
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

// The staged kernels stream the (pre-scaled) pilot table slab by slab through LDS: its slab-ordered copy m.T_sw, slabs of 16 (bf16: 32)
// k-columns, built from ba.Ts when the model has none that is current.  band_run calls it; a caller with work of its own to queue behind it
// (the layer-0 slab sum of bf16 contexts) calls it first.
int band_pilot_slabs(csi_ctx* c, Model& m, const BandArgs& ba, bool bf16) {
    if (m.T_sw_ok) return CSI_OK;
    // (+ 2 KiB: the last 1-KiB DMA chunk of a slab may reach past it, and the kernel requests one slab past the column step)
    const int SK = bf16 ? 32 : 16;
    const size_t floats = (size_t)(ba.K1 / SK + 1) * ba.nt * SK;
    if (!m.T_sw && hipMalloc((void**)&m.T_sw, (floats + 512) * sizeof(float)) != hipSuccess)
        return fail(c, CSI_ERR_NOMEM, "device allocation of the slab-ordered pilot table failed");
    if (bf16) hipLaunchKernelGGL(band_tsw_kernel<32>, dim3(256), dim3(256), 0, c->stream, ba.Ts, ba.ldl, ba.nt, ba.K1, m.T_sw);
    else hipLaunchKernelGGL(band_tsw_kernel<16>, dim3(256), dim3(256), 0, c->stream, ba.Ts, ba.ldl, ba.nt, ba.K1, m.T_sw);
    HIP_TRY(c, hipGetLastError());
    m.T_sw_ok = true;
    return CSI_OK;
}

// Queues the band kernel for one call of a context whose table is loaded (band_load): `ba` with the plain weights of model m and the pilot
// table in ba.Ts, `part` = part_capacity_floats floats for the partial outputs of column splits, flops / bytes for the profile.
int band_run(csi_ctx* c, Model& m, BandArgs ba, bool bf16, bool staged, float* part, size_t part_capacity_floats, double flops, double bytes) {
    if (staged) {
        const int rc = band_pilot_slabs(c, m, ba, bf16);
        if (rc) return rc;
        ba.Ts = m.T_sw;
    }
    const BandPlan p = band_plan(c, ba, bf16, staged, part_capacity_floats);
    const BandKernel& unsplit = c->band_kernel[bf16][!staged ? BAND_EIGHT_NOSTAGE : (p.blocked ? BAND_FOUR : BAND_EIGHT)];
    const BandKernel& cs = c->band_kernel[bf16][p.blocked_cs ? BAND_FOUR_CS : BAND_EIGHT_CS];
    BandArgs tiled = ba;
    if (band_tiled(p.splits > 1 ? cs : unsplit)) {       // (a tail takes a register-blocked form only behind a register-blocked unsplit launch: band_plan)
        const int rc = band4_prepare(c, m, tiled, bf16);
        if (rc) return rc;
    }
    const auto args = [&](const BandKernel& k) -> const BandArgs& { return band_tiled(k) ? tiled : ba; };
    if (p.splits > 1) return band_launch_split(c, cs, args(cs), p.splits, part, flops, bytes, K_PAIR_DENSE);
    if (!p.tail_splits) return band_launch(c, unsplit, args(unsplit), flops, bytes);
    // the full rounds, then the tail on shifted operand pointers
    const long r0 = p.tail_row0;
    const double f0 = (double)r0 / (double)ba.M;
    BandArgs a0 = args(unsplit);
    a0.M = (int)r0;
    const int rc = band_launch(c, unsplit, a0, flops * f0, bytes * f0);
    if (rc) return rc;
    BandArgs a1 = args(cs);
    a1.M = ba.M - (int)r0;
    a1.L0 = ba.L0 + (size_t)(r0 / ba.nt) * ba.ldl;
    a1.out = ba.out + (size_t)r0 * ba.ldo;
    ++c->band_tail_launches;
    return band_launch_split(c, cs, a1, p.tail_splits, part, flops * (1.0 - f0), bytes * (1.0 - f0), K_PAIR_DENSE_TAIL);
}

}  // namespace
