// csi_ls.hpp - host side of the LS estimator (ls_estimate.hip.h): what csi_set_pilot learns about a pilot matrix and uploads (pilot_*),
// the table of kernel shapes and which of them serves a context (LS_KERNELS, ls_plan), and the launches of one call (ls_run).  A new
// shape gets a row in LS_KERNELS; a new family a row, its LDS formula in ls_lds and its rule in ls_resolve.
// tests/test_ls_routes_host.py pins every route - kernel, grid, workgroup size, LDS request - without a GPU.
#pragma once
#include "csi_context.hpp"

namespace {

// ---- the pilot matrix: pure host functions, no HIP call ----------------------------------------------------------------------
// Sylvester Hadamard?  P[j][s] == (-1)^popcount(j & s) exactly -> the Walsh-Hadamard despread applies
bool pilot_is_sylvester(const float* P, int nt) {
    if (nt < 2 || (nt & (nt - 1))) return false;
    for (int j = 0; j < nt; ++j)
        for (int q = 0; q < nt; ++q)
            if (P[(size_t)j * nt + q] != ((__builtin_popcount(j & q) & 1) ? -1.0f : 1.0f)) return false;
    return true;
}

// Is P a signed row / column permutation of the Sylvester Hadamard matrix H[a][u] = (-1)^popcount(a & u)?  (helperGetP of the
// reference's toolbox is un-vendored, helperMIMOChannelEstimate.m:13; the 802.11 VHT mapping matrix [1 -1 1 1; 1 1 -1 1; 1 1 1 -1;
// -1 1 1 1] doubled up recursively is of this kind without being in the Sylvester order.)  Normalise: cs[s] = P[0][s] makes the first
// row +1, then rs[j] = P[j][0] cs[0] the first column; the normalised matrix N = diag(rs) P diag(cs) of such a P is H with rows and
// columns PERMUTED only: N[j][s] = H[sigma(j)][tau(s)] (rows of H multiply like XOR of their indices).  Label log2(nt) independent
// rows of N with the unit vectors (any basis does: sigma' = A sigma, tau' = A^-T tau leave the inner product alone), read tau(s) off
// their signs in column s and sigma(j) off row j's signs in the columns whose tau is a unit vector, then VERIFY every entry.
// On success perm[0][u] = tau^-1(u) | (cs < 0 ? 256 : 0), perm[1][r] = sigma^-1(r) | (rs < 0 ? 256 : 0).
bool pilot_decompose(const float* P, int nt, int perm[2][CSI_WIRE_MAX_NT], bool* identity) {
    if (nt < 2 || nt > CSI_WIRE_MAX_NT || (nt & (nt - 1))) return false;
    for (size_t i = 0; i < (size_t)nt * nt; ++i)
        if (P[i] != 1.0f && P[i] != -1.0f) return false;
    int n = 0;
    while ((1 << n) < nt) ++n;
    std::vector<int> cs(nt), rs(nt);
    for (int s = 0; s < nt; ++s) cs[s] = P[s] < 0 ? -1 : 1;
    for (int j = 0; j < nt; ++j) rs[j] = (P[(size_t)j * nt] < 0 ? -1 : 1) * cs[0];
    typedef std::pair<uint64_t, uint64_t> bits;              // a row of N as the set of its -1 columns
    std::vector<bits> row(nt);
    for (int j = 0; j < nt; ++j) {
        bits b{0, 0};
        for (int s = 0; s < nt; ++s)
            if (P[(size_t)j * nt + s] * (float)(rs[j] * cs[s]) < 0) (s < 64 ? b.first : b.second) |= (uint64_t)1 << (s & 63);
        row[j] = b;
    }
    // greedy basis: a row outside the group generated so far extends it
    std::vector<bits> span{bits{0, 0}};
    std::vector<int> basis;
    for (int j = 0; j < nt && (int)basis.size() < n; ++j) {
        if (std::find(span.begin(), span.end(), row[j]) != span.end()) continue;
        basis.push_back(j);
        const size_t m = span.size();
        for (size_t k = 0; k < m; ++k) span.push_back(bits{span[k].first ^ row[j].first, span[k].second ^ row[j].second});
    }
    if ((int)basis.size() != n) return false;
    std::vector<int> tau(nt), sigma(nt), tau_inv(nt, -1), sigma_inv(nt, -1);
    for (int s = 0; s < nt; ++s) {
        int t = 0;
        for (int i = 0; i < n; ++i)
            if (((s < 64 ? row[basis[i]].first : row[basis[i]].second) >> (s & 63)) & 1) t |= 1 << i;
        tau[s] = t;
        if (tau_inv[t] >= 0) return false;
        tau_inv[t] = s;
    }
    for (int j = 0; j < nt; ++j) {
        int g = 0;
        for (int i = 0; i < n; ++i) {
            const int col = tau_inv[1 << i];
            if (((col < 64 ? row[j].first : row[j].second) >> (col & 63)) & 1) g |= 1 << i;
        }
        sigma[j] = g;
        if (sigma_inv[g] >= 0) return false;
        sigma_inv[g] = j;
    }
    for (int j = 0; j < nt; ++j)
        for (int s = 0; s < nt; ++s) {
            const float want = (float)(rs[j] * cs[s]) * ((__builtin_popcount(sigma[j] & tau[s]) & 1) ? -1.0f : 1.0f);
            if (P[(size_t)j * nt + s] != want) return false;
        }
    bool ident = true;
    for (int u = 0; u < nt; ++u) {
        perm[0][u] = tau_inv[u] | (cs[tau_inv[u]] < 0 ? 256 : 0);
        perm[1][u] = sigma_inv[u] | (rs[sigma_inv[u]] < 0 ? 256 : 0);
        ident = ident && perm[0][u] == u && perm[1][u] == u;
    }
    *identity = ident;
    return true;
}

// the leading bf16 piece (8 significand bits, truncation) of x
inline float bf16_piece(float x) { uint32_t u; std::memcpy(&u, &x, 4); u &= 0xffff0000u; std::memcpy(&x, &u, 4); return x; }
// how many bf16 pieces the entries of P need: the bf16-split LS despread keeps that many
int pilot_pieces(const float* P, int nt) {
    int pieces = 1;
    for (size_t i = 0; i < (size_t)nt * nt && pieces < 3; ++i) {
        const float r1 = P[i] - bf16_piece(P[i]);
        if (r1 != 0.f) pieces = std::max(pieces, r1 - bf16_piece(r1) != 0.f ? 3 : 2);
    }
    return pieces;
}
// bf16 elements of the packed pieces (csi_ctx::Pbf): blocks of LSB_BLOCK per (chunk of 16 symbols, piece, antenna tile)
inline size_t pilot_packed_elems(int nt) { return (size_t)((nt + 15) / 16) * 3 * ((nt + 31) / 32) * LSB_BLOCK; }
// the three pieces in the operand order of v_mfma_f32_32x32x16_bf16: block (chunk of 16 symbols, piece, antenna tile) =
// [k half][row 32][8 symbols], what lane (row + 32 half) of a wave reads as one 16-byte LDS word.  Two elements per float.
std::vector<float> pilot_packed(const float* P, int nt) {
    const int jt = (nt + 31) / 32;
    std::vector<uint16_t> pb(pilot_packed_elems(nt), 0);
    for (int j = 0; j < nt; ++j)
        for (int s = 0; s < nt; ++s) {
            float x = P[(size_t)j * nt + s];
            for (int k = 0; k < 3; ++k) {
                const float f = bf16_piece(x);
                uint32_t u; std::memcpy(&u, &f, 4);
                pb[(((size_t)(s >> 4) * 3 + k) * jt + (j >> 5)) * LSB_BLOCK + (((s >> 3) & 1) * 32 + (j & 31)) * 8 + (s & 7)] = (uint16_t)(u >> 16);
                x -= f;
            }
        }
    std::vector<float> pbf((pb.size() + 1) / 2);
    std::memcpy(pbf.data(), pb.data(), pb.size() * 2);
    return pbf;
}
// zero-padded copy for the chunked and ring kernels (rows / columns up to the next multiple of 32)
std::vector<float> pilot_padded(const float* P, int nt) {
    const int ldp = (nt + 31) / 32 * 32;
    std::vector<float> pad((size_t)ldp * ldp, 0.f);
    for (int j = 0; j < nt; ++j) std::memcpy(&pad[(size_t)j * ldp], P + (size_t)j * nt, sizeof(float) * nt);
    return pad;
}

// Tables of the PERM Walsh-Hadamard kernel from perm (pilot_decompose; every entry & 255 below nt): t[4][nt] = source symbol, its sign, byte offset of
// the output antenna's row inside an item, its sign
std::vector<int> pilot_perm_tables(const int perm[2][CSI_WIRE_MAX_NT], int nt) {
    std::vector<int> t((size_t)4 * nt);
    const float one = 1.0f, minus = -1.0f;
    for (int k = 0; k < 2; ++k)
        for (int u = 0; u < nt; ++u) {
            const int v = perm[k][u];
            t[(size_t)(2 * k) * nt + u] = k == 0 ? (v & 255) : (v & 255) * LS_NDATA * (int)sizeof(float);
            std::memcpy(&t[(size_t)(2 * k + 1) * nt + u], (v & 256) ? &minus : &one, 4);
        }
    // Row 1 as the Walsh-Hadamard kernels consume it (ls_estimate_fwht2_kernel, PERM): the input signs S of a chunk of CH symbols are
    // multiplied out into butterfly coefficients, so that the kernel spends no instruction on them.  Per chunk: [S_r S_{r+8}, r < 8:
    // the fold of the two-threads-per-bin kernel (Nt = 128, CH = 16)], S_0, then for the levels of stride hh = 1, 2, 4 of the
    // 8-point transform one coefficient S_{i0} S_{i0+hh} per group i0 = 0, 2 hh, ..
    if (nt >= 16) {
        const int CH = nt == 128 ? 16 : 8, CHH = 8, L0 = CH - CHH;
        std::vector<float> sg(nt), cf(nt);
        std::memcpy(sg.data(), &t[(size_t)nt], sizeof(float) * nt);
        for (int ch = 0; ch < nt / CH; ++ch) {
            const float* s = sg.data() + ch * CH;
            float* o = cf.data() + ch * CH;
            float pend[8];
            for (int r = 0; r < CHH; ++r) { pend[r] = s[r]; if (L0) o[r] = s[r] * s[r + CHH]; }
            o[L0] = pend[0];
            int idx = L0 + 1;
            for (int hh = 1; hh < CHH; hh <<= 1) {
                for (int grp = 0; grp < CHH / (2 * hh); ++grp) o[idx + grp] = pend[grp * 2 * hh] * pend[grp * 2 * hh + hh];
                idx += CHH / (2 * hh);
            }
        }
        std::memcpy(&t[(size_t)nt], cf.data(), sizeof(float) * nt);
    }
    return t;
}

// device tables of the PERM Walsh-Hadamard kernel from c->p_perm (csi_set_pilot, and a receiver of csi_bcast_state)
int pilot_fast_tables(csi_ctx* c) {
    const int nt = c->cfg.nt;
    if (c->p_tables) { hipFree(c->p_tables); c->p_tables = nullptr; }
    if (!c->p_fast_ok || nt <= 0 || nt > CSI_WIRE_MAX_NT) return CSI_OK;
    c->p_fast_identity = true;
    for (int k = 0; k < 2; ++k)
        for (int u = 0; u < nt; ++u) {
            if ((c->p_perm[k][u] & 255) >= nt) return fail(c, CSI_ERR_INVALID_ARG, "pilot permutation table entry %d out of range", c->p_perm[k][u]);
            c->p_fast_identity = c->p_fast_identity && c->p_perm[k][u] == u;
        }
    const std::vector<int> t = pilot_perm_tables(c->p_perm, nt);
    if (hipMalloc((void**)&c->p_tables, t.size() * sizeof(int)) != hipSuccess)
        return fail(c, CSI_ERR_NOMEM, "device allocation of %zu bytes failed", t.size() * sizeof(int));
    HIP_TRY(c, hipMemcpy(c->p_tables, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice));
    return CSI_OK;
}

// ---- which LS kernel serves a context ----------------------------------------------------------------------------------------
// With the Sylvester Hadamard pilot matrix, or a signed permutation of it, the Walsh-Hadamard kernel on the LDS-DMA ring.  Any other
// P: FFT-first (all Nt spectra in LDS) up to ls_fft_first_max antennas, the ring kernels with the matrix-core despread up to Nt = 128 -
// bf16-split (ls_estimate_ringb_kernel) except for a pilot matrix of arbitrary floats at Nt <= 32, where the fp32 despread of
// ls_estimate_ring_kernel is as fast (profiles/r03_ls_probe_generic.txt) - the despread-first kernel beyond.  The older chunked kernel
// and the register-prefetch Walsh-Hadamard kernel stay selectable through the "ls_kernel" option, the runner-up shapes of a family
// through "ls_v2" (tests, A/B runs: tools/ls_probe.py, tools/ls_pilot_probe.py, tests/fuzz_ls.py, tests/stress_ls_generic.py).
enum LsMode { LS_AUTO = 0, LS_FFT_FIRST = 1, LS_CHUNKED = 2, LS_DESPREAD_FIRST = 3, LS_FWHT = 4, LS_FWHT2 = 5, LS_RING = 6, LS_RINGB = 7 };
struct LsPlan { int mode; const void* fn; size_t lds; int threads; int per_cu; };      // per_cu: resident workgroups per CU (persistent grids)

// One kernel shape.  ls_kernel_row takes, among the rows of a (family, key, pieces) group, the one whose v2 is the context's "ls_v2" - on a signed
// permutation of the Sylvester matrix the LS_V2_PERM row (table-driven symbol fetch / antenna store, whatever "ls_v2" says) - else the LS_V2_ANY row.
constexpr long LS_V2_ANY = 1L << 40, LS_V2_PERM = LS_V2_ANY + 1;      // (outside the int range of the option)
struct LsKernel {
    int mode, key;        // the family = the LsMode it serves; Nt (Walsh-Hadamard families), antenna tiles ceil(Nt / 32) (every other; FFT first: 2 = beyond Nt 32), 0 = any Nt
    long v2;
    int npp;              // ringb: bf16 pieces of the pilot (1 ... 3); 0 elsewhere
    const void* fn;
    int nw, ch, nstg, nf, cap;      // waves; ring families: symbols per chunk, ring slots, spectra images - the others: rows of spectra in LDS (0 = Nt); workgroups per CU at most
};
// a row from the template arguments of its instantiation, one maker per family
template <int J, int W, int NS, int NPP, bool DB> LsKernel ringb(long v2) { return {LS_RINGB, J, v2, NPP, (const void*)ls_estimate_ringb_kernel<J, W, NS, NPP, 1, DB>, W, 16, NS, DB ? 2 : 1, 1}; }
template <int NT, int SP, int CH, int NS, bool DB, int MINB = (SP == 1 ? 2 : 1), bool PERM = false, bool SST = PERM> LsKernel fwht2(long v2) {
    return {LS_FWHT2, NT, PERM ? LS_V2_PERM : v2, 0, (const void*)ls_estimate_fwht2_kernel<NT, SP, CH, NS, DB, MINB, PERM, SST>, 4 * SP, CH, NS, DB ? 2 : 1, MINB};
}
template <int J, int W, int CH, int NS, int MINB = (W == 4 ? 2 : 1)> LsKernel ring(long v2) { return {LS_RING, J, v2, 0, (const void*)ls_estimate_ring_kernel<J, W, CH, NS, MINB>, W, CH, NS, 1, MINB}; }
template <int NT, int SP = 1> LsKernel fwht(int cap) { return {LS_FWHT, NT, LS_V2_ANY, 0, (const void*)ls_estimate_fwht_kernel<NT, SP>, 4 * SP, 16, 1, 1, cap}; }
template <int SPW> LsKernel fft_first() { return {LS_FFT_FIRST, SPW / 8, LS_V2_ANY, 0, (const void*)ls_estimate_kernel<SPW>, LS_THREADS / 64, 0, 1, 1, 8}; }
template <int J, int W, int CH> LsKernel chunked() { return {LS_CHUNKED, J, LS_V2_ANY, 0, (const void*)ls_estimate_chunked_kernel<J, W, CH>, W, CH, 1, 1, W == 4 ? 2 : 1}; }

const LsKernel LS_KERNELS[] = {
    // bf16-split despread on the ring <tiles, waves, slots, pieces, two spectra images>, shapes as measured (profiles/r03_ls_probe_generic.txt); "ls_v2" = 1: the runner-up.
    // One antenna tile (Nt <= 32): ONE workgroup per CU.  The two-workgroups-per-CU form (4 % faster) is not built: its packed +-i rotations went
    // wrong beside another workgroup's MFMAs; ls_lds pads the request so that the dispatcher cannot co-locate two either.
    ringb<1, 4, 2, 1, false>(1), ringb<1, 4, 2, 2, false>(1), ringb<1, 4, 2, 3, false>(1),
    ringb<1, 4, 1, 1, false>(LS_V2_ANY), ringb<1, 4, 1, 2, false>(LS_V2_ANY), ringb<1, 4, 1, 3, false>(LS_V2_ANY),
    ringb<2, 8, 1, 1, false>(1), ringb<2, 8, 1, 2, false>(1), ringb<2, 8, 1, 3, false>(1),
    ringb<2, 8, 1, 1, true>(LS_V2_ANY), ringb<2, 8, 1, 2, true>(LS_V2_ANY), ringb<2, 8, 1, 3, true>(LS_V2_ANY),
    ringb<3, 8, 2, 1, false>(1), ringb<3, 8, 2, 2, false>(1), ringb<3, 8, 2, 3, false>(1),
    ringb<3, 8, 1, 1, true>(LS_V2_ANY), ringb<3, 8, 1, 2, true>(LS_V2_ANY), ringb<3, 8, 1, 3, true>(LS_V2_ANY),
    ringb<4, 8, 1, 1, false>(1), ringb<4, 8, 1, 2, false>(1), ringb<4, 8, 1, 3, false>(1),
    ringb<4, 8, 1, 1, true>(LS_V2_ANY), ringb<4, 8, 1, 2, true>(LS_V2_ANY), ringb<4, 8, 1, 3, true>(LS_V2_ANY),
    // Walsh-Hadamard despread on the ring <Nt, threads per bin, chunk, slots, two images, workgroups per CU, PERM, scalar-base stores>, shape per Nt as
    // measured (profiles/r02_ls_probe.txt); "ls_v2" = 1: the runner-up, 3: the default shape with vector-address stores (round 3) in place of stores with
    // the row base in scalar registers (round 4: -3 ... -5 % at Nt = 32 / 64, -1 ... -1.9 % at 128, profiles/r04_ls_probe.txt).  Nt = 32: 8-symbol chunks, one
    // slot: 38 KiB of LDS and 122 VGPRs - four workgroups per CU (0.379 ms; two with 16-symbol chunks: 0.402).  Nt = 128: two spectra images: -6 %.
    fwht2<16, 1, 16, 1, false>(1), fwht2<16, 1, 8, 1, false, 4>(3), fwht2<16, 1, 8, 1, false, 4, false, true>(LS_V2_ANY),
    fwht2<32, 1, 16, 1, false>(1), fwht2<32, 1, 8, 1, false, 4>(3), fwht2<32, 1, 8, 1, false, 4, false, true>(LS_V2_ANY),
    fwht2<64, 1, 16, 1, false>(1), fwht2<64, 1, 8, 3, false>(3), fwht2<64, 1, 8, 3, false, 2, false, true>(LS_V2_ANY),
    fwht2<128, 2, 16, 3, false>(1), fwht2<128, 2, 16, 2, true>(3), fwht2<128, 2, 16, 2, true, 1, false, true>(LS_V2_ANY),
    // ... and on a signed permutation of the Sylvester matrix: the default shapes
    fwht2<16, 1, 8, 1, false, 4, true>(0), fwht2<32, 1, 8, 1, false, 4, true>(0), fwht2<64, 1, 8, 3, false, 2, true>(0), fwht2<128, 2, 16, 2, true, 1, true>(0),
    // fp32 despread on the ring <tiles, waves, chunk, slots, workgroups per CU> (profiles/r02_ls_probe.txt).  One antenna tile: 8-symbol chunks and one slot
    // leave room for three workgroups per CU (Nt = 32: 0.438 against 0.470 ms) - "ls_v2" = 0 only; 2: three slots; anything else: 16-symbol chunks.
    // Two tiles: 8-symbol chunks let two workgroups share a CU, "ls_v2" = 1 selects the 8-wave form.
    ring<1, 4, 8, 1, 3>(0), ring<1, 4, 8, 3>(2), ring<1, 4, 16, 1>(LS_V2_ANY),
    ring<2, 4, 8, 2>(LS_V2_ANY), ring<2, 8, 16, 3>(1), ring<3, 8, 16, 2>(LS_V2_ANY), ring<4, 8, 16, 1>(LS_V2_ANY),
    // Walsh-Hadamard despread with the register prefetch (round 1; the Sylvester order only), workgroups per CU as the registers allow
    fwht<16>(3), fwht<32>(2), fwht<64>(2), fwht<128, 2>(1),
    // FFT first: all Nt spectra in LDS, 8 symbols per wave in registers up to Nt = 32, 16 up to 64
    fft_first<8>(), fft_first<16>(),
    // chunked <tiles, waves, chunk>: register-limited, 2 waves per SIMD
    chunked<1, 4, 16>(), chunked<2, 4, 16>(), chunked<3, 8, 32>(), chunked<4, 8, 32>(),
    // despread first: one workgroup per (item, LSD_ROWS antennas) - any Nt (ls_run launches it on its own grid)
    {LS_DESPREAD_FIRST, 0, LS_V2_ANY, 0, (const void*)ls_despread_first_kernel, LS_THREADS / 64, LSD_ROWS, 1, 1, 2},
};
constexpr size_t LS_LDS_CU = 160 * 1024;        // LDS of a CU

// Dynamic LDS bytes of a row's kernel at this Nt.  Ring families: twiddles, nf images of a chunk's padded rows, nstg ring slots of a chunk's symbols; ring: + the
// padded tile rows of P; ringb: + nstg + 1 chunks of P's bf16 blocks.  The others: rows of spectra planes and the twiddles.
size_t ls_lds(const LsKernel& k, int nt) {
    const size_t jt = (size_t)(nt + 31) / 32;
    const size_t ring = (size_t)(2 * LSC_NTW + k.nf * k.ch * 2 * LSC_ROW + k.nstg * k.ch * 2 * LS_FFT) * sizeof(float);
    if (k.mode == LS_FWHT2) return ring;
    if (k.mode == LS_RING) return ring + 32 * jt * (jt * 32 + 1) * sizeof(float);
    if (k.mode != LS_RINGB) return (size_t)((k.ch ? k.ch : nt) * 2 * LS_PLANE + 2 * LS_FFT) * sizeof(float);
    const size_t lds = ring + (size_t)(k.nstg + 1) * k.npp * jt * LSB_BLOCK * 2;
    return jt == 1 ? std::max(lds, (size_t)(81 * 1024)) : lds;      // one antenna tile: one workgroup per CU by construction (see the table)
}

// the row that serves (family, Nt) under this context's "ls_v2" and pilot; nullptr: the family has no kernel for this Nt
const LsKernel* ls_kernel_row(const csi_ctx* c, int mode) {
    const int nt = c->cfg.nt, jt = (nt + 31) / 32;
    const int key = mode == LS_FWHT || mode == LS_FWHT2 ? nt : (mode == LS_DESPREAD_FIRST ? 0 : (mode == LS_FFT_FIRST ? (nt <= 32 ? 1 : 2) : jt));
    const int npp = mode == LS_RINGB ? std::min(3, std::max(1, c->p_pieces)) : 0;
    const long v2 = mode == LS_FWHT2 && c->p_fast_ok && !c->p_fast_identity ? LS_V2_PERM : c->ls_v2;
    const LsKernel* row = nullptr;
    for (const LsKernel& k : LS_KERNELS) {
        if (k.mode != mode || k.key != key || k.npp != npp) continue;
        if (k.v2 == v2) { row = &k; break; }
        if (k.v2 == LS_V2_ANY) row = &k;
    }
    // the bf16-split kernel: Nt = 16 ... 128 (four antenna tiles), and only where its request fits the LDS of a CU
    if (mode == LS_RINGB && (nt < 16 || (row && ls_lds(*row, nt) > LS_LDS_CU))) return nullptr;
    return row;
}

// "ls_kernel" against what the shape and the pilot admit: the family that serves the context, and its row.  Every family it can return has a row for
// this Nt: the Walsh-Hadamard ones are taken at Nt = 16 / 32 / 64 / 128 only, ringb only with its row in hand, FFT first up to Nt = 64 (two keys),
// chunked and ring at Nt = 16 ... 128 (four tiles), despread first at any Nt.
const LsKernel* ls_resolve(const csi_ctx* c, int* family) {
    const int nt = c->cfg.nt;
    int mode = c->ls_kernel;
    // Walsh-Hadamard despread: the Sylvester matrix itself, or (round 4) any signed row / column permutation of it - the kernel
    // then fetches the symbols and stores the antennas through the tables csi_set_pilot derived (PERM form)
    const bool perm = c->p_fast_ok && !c->p_fast_identity;
    const bool fwht_ok = (c->p_sylvester || (c->p_fast_ok && (c->p_fast_identity || c->ls_fast_perm))) && (nt == 16 || nt == 32 || nt == 64 || nt == 128);
    if ((mode == LS_FWHT || mode == LS_FWHT2) && !fwht_ok) mode = LS_AUTO;
    if (mode == LS_FWHT && perm) mode = LS_FWHT2;            // the round-1 kernel knows the Sylvester order only
    const LsKernel* rb = nullptr;
    const auto ringb_ok = [&] { return (rb = ls_kernel_row(c, LS_RINGB)) != nullptr; };
    if (mode == LS_RINGB && !ringb_ok()) mode = LS_AUTO;
    if (mode == LS_AUTO)
        mode = fwht_ok ? LS_FWHT2 : (nt <= c->ls_fft_first_max ? LS_FFT_FIRST : (nt <= 128 ? (nt >= c->ls_ringb_min && (c->p_pieces < 3 || nt > 32) && ringb_ok() ? LS_RINGB : LS_RING) : LS_DESPREAD_FIRST));
    if (mode == LS_FFT_FIRST && nt > 64) mode = LS_CHUNKED;
    if ((mode == LS_CHUNKED || mode == LS_RING) && (nt < 16 || nt > 128)) mode = nt < 16 ? LS_FFT_FIRST : LS_DESPREAD_FIRST;
    *family = mode;
    return mode == LS_RINGB ? rb : ls_kernel_row(c, mode);
}

// The kernel of the next LS call of this context.  A pure function of the context's LIVE state (pilot fields and options change without
// ls_prepare - wire_drop_receiver): never cached.  No HIP call.
LsPlan ls_plan(const csi_ctx* c) {
    int mode = LS_AUTO;
    const LsKernel& k = *ls_resolve(c, &mode);
    const size_t lds = ls_lds(k, c->cfg.nt);
    // as many workgroups per CU as the LDS holds, at most the row's cap (which is what binds for the fixed-LDS kernels: registers limit them first)
    return {mode, k.fn, lds, 64 * k.nw, std::max(1, std::min(k.cap, (int)(LS_LDS_CU / lds)))};
}

// the LS kernel of this context is the Walsh-Hadamard one in its default one-thread-per-bin shape on the Sylvester order itself: its LDS bytes
bool ls_default_fwht2(const csi_ctx* c, size_t* lds_bytes) {
    if (c->ls_v2 != 0 || c->ls_debug != 0 || c->ls_kernel != LS_AUTO || (c->p_fast_ok && !c->p_fast_identity)) return false;
    const LsPlan p = ls_plan(c);
    *lds_bytes = p.lds;
    return p.mode == LS_FWHT2 && p.threads == 256;
}
LsArgs ls_args(const csi_ctx* c, const float* d_ltf_re, const float* d_ltf_im, float* d_h_re, float* d_h_im) {
    const csi_config& cf = c->cfg;
    LsArgs a{};
    a.P = c->P; a.Ppad = c->Ppad; a.Pbf = reinterpret_cast<const uint16_t*>(c->Pbf); a.ldp = (cf.nt + 31) / 32 * 32; a.dbg = c->ls_debug;
    a.tw = c->tw; a.bin_pos = c->bin_pos; a.denom = c->denom; a.nt = cf.nt; a.len_ltf = cf.len_ltf; a.perm = c->p_tables;
    a.ltf_re = d_ltf_re; a.ltf_im = d_ltf_im; a.h_re = d_h_re; a.h_im = d_h_im;
    return a;
}
// the LDS attribute of whatever ls_plan returns now: after every change of the pilot or of an option the plan reads
int ls_prepare(csi_ctx* c) {
    if (c->cfg.nt == 0) return CSI_OK;
    const LsPlan p = ls_plan(c);
    HIP_TRY(c, hipFuncSetAttribute(p.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    return CSI_OK;
}

// Queues the LS estimate of npkt packets (checked by the caller): items = (packet, rx) pairs, at most max_grid of them per launch.
int ls_run(csi_ctx* c, const float* d_ltf_re, const float* d_ltf_im, int64_t npkt, float* d_h_re, float* d_h_im) {
    const csi_config& cf = c->cfg;
    const LsPlan plan = ls_plan(c);
    const int n_jc = (cf.nt + LSD_ROWS - 1) / LSD_ROWS;
    HIP_TRY(c, hipSetDevice(cf.device));
    const int64_t nblk = npkt * cf.nr;
    LsArgs a = ls_args(c, d_ltf_re, d_ltf_im, d_h_re, d_h_im);
    const int64_t max_grid = ((int64_t)1 << 30) / n_jc;      // also keeps nb inside an int
    for (int64_t b0 = 0; b0 < nblk; b0 += max_grid) {
        const int64_t nb = std::min(max_grid, nblk - b0);
        a.ltf_re = d_ltf_re + (size_t)b0 * cf.len_ltf; a.ltf_im = d_ltf_im + (size_t)b0 * cf.len_ltf;
        a.h_re = d_h_re + (size_t)b0 * cf.nt * LS_NDATA; a.h_im = d_h_im + (size_t)b0 * cf.nt * LS_NDATA;
        const double pairs = (double)nb * cf.nt;
        int nb32 = (int)nb;
        ProfScope ps(c, K_LS_ESTIMATE, pairs * (10240.0 + 8.0 * LS_NDATA * cf.nt), pairs * (2560.0 + 1872.0));
        if (plan.mode == LS_DESPREAD_FIRST) {
            hipLaunchKernelGGL(ls_despread_first_kernel, dim3((unsigned)(nb * n_jc)), dim3(LS_THREADS), plan.lds, c->stream, a, n_jc);
        } else {
            // persistent grid: as many workgroups as can reside (x256 CUs)
            const unsigned grid = (unsigned)std::min<int64_t>(nb, (int64_t)256 * plan.per_cu);
            void* kargs[] = {(void*)&a, (void*)&nb32};
            HIP_TRY(c, hipLaunchKernel(plan.fn, dim3(grid), dim3(plan.threads), kargs, plan.lds, c->stream));
        }
        HIP_TRY(c, hipGetLastError());
    }
    return CSI_OK;
}

}  // namespace
