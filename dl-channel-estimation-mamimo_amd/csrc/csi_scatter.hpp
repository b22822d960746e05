// csi_scatter.hpp - host side of csi_synth_scattering (kernels: synth_scattering.hip.h): defaults, the argument
// checks (shared with csi_scatter_aged.hpp) and the two launches.
#pragma once
#include "csi_context.hpp"
#include "synth_scattering.hip.h"

namespace {

// What both scattering entry points (csi_synth_scattering, csi_scatter_channel_at_device) check first: the context, the packet range and the
// configuration, whose defaults are filled in on the way.  `who` names the entry point in the text of a refusal.
int scatter_config(csi_ctx* c, const char* who, int64_t first_pkt, int64_t npkt, const csi_scatter_config* cfg, csi_scatter_config& k) {
    const csi_config& cf = c->cfg;
    if (cf.nt < 4 || cf.nt % 4 != 0 || cf.len_ltf != LS_SYM * cf.nt)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: needs a context of nt >= 1 antennas and len_ltf = 320 nt (nt %d, len_ltf %d)", who, cf.nt, cf.len_ltf);
    if (npkt < 0 || first_pkt < 0)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: npkt %lld / first_pkt %lld must not be negative", who, (long long)npkt, (long long)first_pkt);
    k = csi_scatter_config{};
    if (cfg) k = *cfg;
    if (k.n_scat == 0) k.n_scat = 100;
    if (k.range_m == 0.f) k.range_m = 100.f;
    if (k.az_deg == 0.f) k.az_deg = 30.f;
    if (k.box_frac == 0.f) k.box_frac = 0.1f;
    if (k.sample_rate_hz == 0.f) k.sample_rate_hz = 100e6f;
    if (k.n_scat < 1 || k.n_scat > SC_MAX_SCAT) return fail(c, CSI_ERR_INVALID_ARG, "%s: n_scat %d outside 1 .. %d", who, k.n_scat, SC_MAX_SCAT);
    if (!std::isfinite(k.range_m) || k.range_m <= 0.f) return fail(c, CSI_ERR_INVALID_ARG, "%s: range_m %g must be finite and positive", who, (double)k.range_m);
    if (!std::isfinite(k.box_frac) || k.box_frac <= 0.f) return fail(c, CSI_ERR_INVALID_ARG, "%s: box_frac %g must be finite and positive", who, (double)k.box_frac);
    if (!std::isfinite(k.sample_rate_hz) || k.sample_rate_hz <= 0.f)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: sample_rate_hz %g must be finite and positive", who, (double)k.sample_rate_hz);
    if (!std::isfinite(k.az_deg)) return fail(c, CSI_ERR_INVALID_ARG, "%s: az_deg %g must be finite", who, (double)k.az_deg);
    if (!(std::fabs(k.el_deg) <= 90.f)) return fail(c, CSI_ERR_INVALID_ARG, "%s: el_deg %g outside -90 .. 90", who, (double)k.el_deg);
    if (k.flags & ~3u) return fail(c, CSI_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (bit 0 = amplitude scale, bit 1 = random users)", who, k.flags);
    return CSI_OK;
}

// The fields that ScatterArgs and ScatterAgedArgs share: the stream, the shape and the geometry of the configuration
template <class Args>
void scatter_fill(Args& a, const csi_config& cf, const csi_scatter_config& k, uint64_t seed, int64_t first_pkt) {
    a.seed = seed; a.first_pkt = first_pkt;
    a.nt = cf.nt; a.nr = cf.nr; a.n_scat = k.n_scat;
    a.random_users = (k.flags & 2u) ? 1 : 0;
    a.amp = (k.flags & 1u) ? (float)(std::sqrt((double)(LS_FFT - 14)) / LS_FFT) : 1.0f;
    a.range_m = k.range_m; a.box_frac = k.box_frac;
    const double deg = 3.14159265358979323846 / 180.0, az = (double)k.az_deg * deg, el = (double)k.el_deg * deg;
    a.ex = (float)(std::cos(el) * std::cos(az)); a.ey = (float)(std::cos(el) * std::sin(az)); a.ez = (float)std::sin(el);
    a.spm = (float)((double)k.sample_rate_hz / SC_LIGHT);
    a.gscale = (float)(1.0 / std::sqrt(2.0 * k.n_scat));
}

int synth_scattering(csi_ctx* c, uint64_t seed, int64_t first_pkt, int64_t npkt, const float* snr_db, const csi_scatter_config* cfg,
                     float* d_ltf_re, float* d_ltf_im, float* d_h_re, float* d_h_im, float* d_noise_std, float* d_tau) {
    static const char* who = "csi_synth_scattering";
    const csi_config& cf = c->cfg;
    csi_scatter_config k;
    if (int rc = scatter_config(c, who, first_pkt, npkt, cfg, k)) return rc;
    if (npkt == 0) return CSI_OK;
    if (!d_ltf_re || !d_ltf_im) return fail(c, CSI_ERR_INVALID_ARG, "%s: null ltf planes for %lld packets", who, (long long)npkt);
    if ((d_h_re == nullptr) != (d_h_im == nullptr)) return fail(c, CSI_ERR_INVALID_ARG, "%s: the channel planes come as a pair (one of h_re / h_im is null)", who);
    if (!c->pilot_ok) return fail(c, CSI_ERR_NOT_READY, "%s: no pilot matrix set (csi_set_pilot)", who);
    if (c->user_capture && snr_db) return fail(c, CSI_ERR_INVALID_ARG, "%s: a call with an SNR array uploads it and cannot be captured", who);
    if (((reinterpret_cast<uintptr_t>(d_ltf_re) | reinterpret_cast<uintptr_t>(d_ltf_im) | reinterpret_cast<uintptr_t>(d_h_re) | reinterpret_cast<uintptr_t>(d_h_im)) & 15) != 0)
        return fail(c, CSI_ERR_INVALID_ARG, "%s: output planes must start on 16-byte boundaries", who);
    const int64_t nblk = npkt * cf.nr;
    if (nblk > 0x7fffffff) return fail(c, CSI_ERR_INVALID_ARG, "%s: %lld packets x %d rx antennas exceed one launch (2^31 - 1 items)", who, (long long)npkt, cf.nr);
    const size_t lds = scatter_lds_floats(cf.nt, k.n_scat) * sizeof(float);
    if (lds > 160 * 1024) return fail(c, CSI_ERR_INVALID_ARG, "%s: nt %d with %d scatterers needs %zu bytes of LDS (160 KiB per workgroup)", who, cf.nt, k.n_scat, lds);
    HIP_TRY(c, hipSetDevice(cf.device));
    ScatterArgs a{};
    if (snr_db) {      // per-packet noise factors in double on the host, one upload; the item powers follow them in the same buffer
        int rc = ensure_bytes(c, &c->synth_ws, &c->synth_ws_bytes, (size_t)(npkt + nblk) * sizeof(float));
        if (rc) return rc;
        c->synth_host.resize((size_t)npkt);
        for (int64_t p = 0; p < npkt; ++p) c->synth_host[p] = (float)(0.5 * std::pow(10.0, -0.1 * (double)snr_db[p]));
        float* ws = reinterpret_cast<float*>(c->synth_ws);
        HIP_TRY(c, hipMemcpyAsync(ws, c->synth_host.data(), (size_t)npkt * sizeof(float), hipMemcpyHostToDevice, c->stream));
        a.fac = ws;
        a.part = ws + npkt;
    }
    a.P = c->P; a.tw = c->tw; a.ltf_nat = c->ltf_nat; a.bin_pos = c->bin_pos;
    a.ltf_re = d_ltf_re; a.ltf_im = d_ltf_im; a.h_re = d_h_re; a.h_im = d_h_im; a.noise_std = d_noise_std; a.tau = d_tau;
    scatter_fill(a, cf, k, seed, first_pkt);
    a.len_ltf = cf.len_ltf;
    if (lds > 48 * 1024 && lds > c->scatter_lds_attr) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)synth_scattering_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIP_TRY(c, hipFuncSetAttribute((const void*)synth_scattering_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        c->scatter_lds_attr = lds;
    }
    const double chunks = (double)((cf.nt + SS_CH - 1) / SS_CH);
    const double flops = (double)nblk * LS_FFT * k.n_scat * 64.0 * chunks * ((snr_db ? 2.0 : 1.0) + (d_h_re ? 1.0 : 0.0));
    const double bytes = (double)nblk * (8.0 * cf.len_ltf + (d_h_re ? 8.0 * cf.nt * LS_NDATA : 0.0));
    ProfScope ps(c, K_SYNTH_SCATTERING, flops, bytes);
    if (snr_db) {
        hipLaunchKernelGGL(synth_scattering_kernel<true>, dim3((unsigned)nblk), dim3(SS_THREADS), lds, c->stream, a);
        ++c->scatter_launches;
    }
    hipLaunchKernelGGL(synth_scattering_kernel<false>, dim3((unsigned)nblk), dim3(SS_THREADS), lds, c->stream, a);
    ++c->scatter_launches;
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

}  // namespace
