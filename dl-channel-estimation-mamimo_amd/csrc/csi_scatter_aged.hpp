// csi_scatter_aged.hpp - host side of csi_scatter_channel_at_device (kernel: scatter_aged.hip.h): the motion record's
// checks on top of csi_scatter.hpp's, and the one launch.  Nothing is uploaded - the times are kernel arguments - so the call can be
// captured.
#pragma once
#include "csi_scatter.hpp"
#include "scatter_aged.hip.h"

namespace {

int scatter_channel_at(csi_ctx* c, uint64_t seed, int64_t first_pkt, int64_t npkt, const csi_scatter_config* cfg, const csi_motion_config* motion,
                       const double* t_s, int n_times, float* d_h_re, float* d_h_im) {
    static const char* who = "csi_scatter_channel_at_device";
    const csi_config& cf = c->cfg;
    csi_scatter_config k;
    if (int rc = scatter_config(c, who, first_pkt, npkt, cfg, k)) return rc;
    csi_motion_config m{};
    if (motion) m = *motion;
    if (m.carrier_hz == 0.f) m.carrier_hz = 28e9f;
    if (n_times < 1 || n_times > SA_MAX_TIMES) return fail(c, CSI_ERR_INVALID_ARG, "%s: n_times %d outside 1 .. %d", who, n_times, SA_MAX_TIMES);
    if (!t_s) return fail(c, CSI_ERR_INVALID_ARG, "%s: null t_s for %d times", who, n_times);
    for (int i = 0; i < n_times; ++i)
        if (!std::isfinite(t_s[i])) return fail(c, CSI_ERR_INVALID_ARG, "%s: t_s[%d] = %g must be finite", who, i, t_s[i]);
    if (!std::isfinite(m.speed_mps) || m.speed_mps < 0.f) return fail(c, CSI_ERR_INVALID_ARG, "%s: speed_mps %g must be finite and not negative", who, (double)m.speed_mps);
    if (!std::isfinite(m.heading_az_deg)) return fail(c, CSI_ERR_INVALID_ARG, "%s: heading_az_deg %g must be finite", who, (double)m.heading_az_deg);
    if (!(std::fabs(m.heading_el_deg) <= 90.f)) return fail(c, CSI_ERR_INVALID_ARG, "%s: heading_el_deg %g outside -90 .. 90", who, (double)m.heading_el_deg);
    if (!std::isfinite(m.carrier_hz) || m.carrier_hz < 0.f) return fail(c, CSI_ERR_INVALID_ARG, "%s: carrier_hz %g must be finite and not negative", who, (double)m.carrier_hz);
    if (m.flags & ~1u) return fail(c, CSI_ERR_INVALID_ARG, "%s: unknown motion flag bits 0x%x (bit 0 = random heading)", who, m.flags);
    if (npkt == 0) return CSI_OK;
    if (!d_h_re || !d_h_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null channel planes (d_h_re / d_h_im) for %lld packets", who, (long long)npkt);
    if (((reinterpret_cast<uintptr_t>(d_h_re) | reinterpret_cast<uintptr_t>(d_h_im)) & 15) != 0)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: the channel planes d_h_re / d_h_im must start on 16-byte boundaries", who);
    const int64_t nblk = npkt * cf.nr;
    if (nblk > 0x7fffffff) return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets x %d rx antennas exceed one launch (2^31 - 1 items)", who, (long long)npkt, cf.nr);
    const size_t lds = scatter_aged_lds_floats(k.n_scat) * sizeof(float);
    if (lds > 160 * 1024) return fail(c, CSI_ERR_INVALID_ARG, "%s: %d scatterers need %zu bytes of LDS (160 KiB per workgroup)", who, k.n_scat, lds);
    HIP_TRY(c, hipSetDevice(cf.device));
    ScatterAgedArgs a{};
    scatter_fill(a, cf, k, seed, first_pkt);
    a.bin_pos = c->bin_pos;
    a.h_re = d_h_re; a.h_im = d_h_im;
    a.n_times = n_times;
    for (int i = 0; i < n_times; ++i) a.t[i] = t_s[i];
    a.random_heading = (m.flags & 1u) ? 1 : 0;
    a.dop = (double)m.speed_mps * (double)m.carrier_hz / SC_LIGHT;
    const double deg = 3.14159265358979323846 / 180.0, az = (double)m.heading_az_deg * deg, el = (double)m.heading_el_deg * deg;
    a.mce = std::cos(el);
    a.mx = a.mce * std::cos(az); a.my = a.mce * std::sin(az); a.mz = std::sin(el);
    if (lds > 48 * 1024 && lds > c->scatter_aged_lds_attr) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)scatter_aged_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIP_TRY(c, hipFuncSetAttribute((const void*)scatter_aged_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        c->scatter_aged_lds_attr = lds;
    }
    const double chunks = (double)((cf.nt + SS_CH - 1) / SS_CH);
    const double flops = (double)nblk * LS_FFT * k.n_scat * 64.0 * chunks * n_times;
    const double bytes = (double)nblk * 8.0 * cf.nt * LS_NDATA * n_times;
    ProfScope ps(c, K_SCATTER_AGED, flops, bytes);
    if (a.dop != 0.0) hipLaunchKernelGGL(scatter_aged_kernel<true>, dim3((unsigned)nblk), dim3(SS_THREADS), lds, c->stream, a);
    else hipLaunchKernelGGL(scatter_aged_kernel<false>, dim3((unsigned)nblk), dim3(SS_THREADS), lds, c->stream, a);
    ++c->scatter_aged_launches;
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

}  // namespace
