// csi_stage.hpp - the staged host call: what every entry point that takes host pointers and runs a device form over packets (links, for
// csi_nmse) in chunks does with the context's staging buffer, once.  The caller declares its planes; staged_call sizes the chunk, sizes
// c->stage, places the planes in it and moves each chunk up, through the caller's body and down.  Users: csi_lmmse_estimate and
// csi_lmmse_blind (csi_lmmse.hpp), csi_nmse (csi_mamimo.hip), csi_hybrid_weights (csi_hybrid.hpp), csi_subspace_smooth (csi_subspace.hpp),
// csi_beam_smooth / csi_beam_wiener (csi_beam.hpp).  csi_predict_samples keeps its own loops: they interleave scratch tensors and slack
// zeroing with the staged rows.
// Beside it, the two checks the smoothers share: the overlap rule of their in / out planes and the orthonormality of a basis.
#pragma once
#include "csi_context.hpp"

namespace {

constexpr int64_t STAGE_BUDGET = (int64_t)256 << 20;      // bytes of staging a chunk is sized for

// ... or what the context's workspace_bytes allows when that is less (the two smoothers)
inline int64_t stage_budget(const csi_ctx* c) {
    return c->cfg.workspace_bytes > 0 ? std::min<int64_t>(c->cfg.workspace_bytes, STAGE_BUDGET) : STAGE_BUDGET;
}

// One plane of the staging buffer: `bytes` per item (a packet, or a link), `chunk` items long.  src: the host array that goes up in
// front of the body; dst: the host array that takes the plane behind it; a plane with neither still has its room (an optional result
// the caller did not ask for, a scratch plane).  dev is set by staged_call.
struct StagePlane {
    size_t bytes;
    const void* src;
    void* dst;
    char* dev = nullptr;
    template <typename T> T* as() const { return reinterpret_cast<T*>(dev); }
};

// chunk = min(n, max(1, budget / divisor)) items - the divisor is the caller's: most size the chunk by their four CSI planes and leave
// the small side planes out.  c->stage holds the planes in declared order, chunk items each, and `extra` bytes behind them.  Per chunk:
// the uploads in declared order, body(first item, items), the downloads in declared order and, with `sync`, hipStreamSynchronize
// (csi_nmse's body synchronizes by itself).
template <size_t N, typename Body>
int staged_call(csi_ctx* c, int64_t n, int64_t budget, size_t divisor, size_t extra, bool sync, StagePlane (&planes)[N], Body&& body) {
    const int64_t chunk = std::min(n, std::max<int64_t>(1, budget / (int64_t)divisor));
    size_t item = 0;
    for (const StagePlane& p : planes) item += p.bytes;
    if (int rc = ensure_bytes(c, &c->stage, &c->stage_bytes, item * (size_t)chunk + extra)) return rc;
    char* d = c->stage;
    for (StagePlane& p : planes) { p.dev = d; d += p.bytes * (size_t)chunk; }
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t ni = std::min(chunk, n - i0);
        for (const StagePlane& p : planes)
            if (p.src) HIP_TRY(c, hipMemcpyAsync(p.dev, static_cast<const char*>(p.src) + p.bytes * (size_t)i0, p.bytes * (size_t)ni, hipMemcpyHostToDevice, c->stream));
        if (int rc = body(i0, ni)) return rc;
        for (const StagePlane& p : planes)
            if (p.dst) HIP_TRY(c, hipMemcpyAsync(static_cast<char*>(p.dst) + p.bytes * (size_t)i0, p.dev, p.bytes * (size_t)ni, hipMemcpyDeviceToHost, c->stream));
        if (sync) HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return CSI_OK;
}

// [p, p + bytes) and [q, q + bytes) share a byte
inline bool planes_overlap(const void* p, const void* q, size_t bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + bytes && b < a + bytes;
}

// out may be the input planes themselves, re with re and im with im; every other shared byte is refused
int inout_planes_disjoint(csi_ctx* c, const char* who, const float* h_re, const float* h_im, const float* out_re, const float* out_im, size_t bytes) {
    if ((out_re != h_re && planes_overlap(out_re, h_re, bytes)) || (out_im != h_im && planes_overlap(out_im, h_im, bytes)) ||
        planes_overlap(out_re, h_im, bytes) || planes_overlap(out_im, h_re, bytes) || planes_overlap(out_re, out_im, bytes))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: an output plane may be its own input plane (re with re, im with im); any other overlap of the planes is refused", who);
    return CSI_OK;
}

// a basis X [rows][cols] (re / im planes): every entry finite, and X^H X the identity within tol - in double on the host
// (rows cols^2 complex products once per basis).  `letter` names X in the message.
int basis_orthonormal(csi_ctx* c, const char* who, const float* re, const float* im, int rows, int cols, double tol, char letter) {
    const size_t n = (size_t)rows * cols;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(re[i]) || !std::isfinite(im[i]))
            return fail(c, CSI_ERR_INVALID_ARG, "%s: non-finite basis entry at [%zu][%zu]", who, i / cols, i % cols);
    double worst = 0.0;
    int wi = 0, wj = 0;
    for (int i = 0; i < cols; ++i)
        for (int j = i; j < cols; ++j) {
            double sr = 0.0, si = 0.0;
            for (int k = 0; k < rows; ++k) {
                const double ar = re[(size_t)k * cols + i], ai = im[(size_t)k * cols + i];
                const double br = re[(size_t)k * cols + j], bi = im[(size_t)k * cols + j];
                sr += ar * br + ai * bi;          // conj(a) b
                si += ar * bi - ai * br;
            }
            const double d = std::hypot(sr - (i == j ? 1.0 : 0.0), si);
            if (d > worst) { worst = d; wi = i; wj = j; }
        }
    if (!(worst <= tol))
        return fail(c, CSI_ERR_INVALID_ARG, "%s: basis is not orthonormal: |%c^H %c - I| = %.3g at [%d][%d] (at most %g)", who, letter, letter, worst, wi, wj, tol);
    return CSI_OK;
}

}  // namespace
