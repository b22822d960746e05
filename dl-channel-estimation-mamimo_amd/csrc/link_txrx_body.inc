// link_txrx_body.inc - the body of link_txrx_kernel (link_sim.hip.h), included twice: into link_txrx_kernel with LK_RX 0 - so that the
// kernel of csi_link_sim_device stays, token for token, the function it was before the estimating receiver existed - and into
// link_txrx_rx_kernel with LK_RX 1, where `a` names the LinkArgs part of its LinkRxArgs `b`.  (A device function called by both kernels
// changes the code of the first: cf. ls_fwht2_body.inc.)  The LK_RX parts: the preamble through G and its LS estimate Ghat, kept in a
// second LDS array GH; A, the matched filter and csi from Ghat; the sum |Ghat - G|^2 as a fourth row of the lane sums; g_nmse and gest.
    extern __shared__ __attribute__((aligned(16))) float lk_smem[];
    const int nt = a.nt, nr = a.nr, ntrf = a.ntrf, n_sym = a.n_sym, fs = a.fstride;
    constexpr int BPS = 2 * M;
    float* G = lk_smem;                                       // [2 (r NS + s) + z][LK_THREADS]
#if LK_RX
    constexpr int NL = NS == 1 ? 1 : NS == 2 ? 2 : 4;         // link_preamble_symbols(NS)
    float* GH = G + (size_t)2 * nr * NS * LK_THREADS;         // Ghat, the same layout
    float* fb_re = GH + (size_t)2 * nr * NS * LK_THREADS;     // [234][fs]
#else
    float* fb_re = G + (size_t)2 * nr * NS * LK_THREADS;      // [234][fs]
#endif
    float* fb_im = fb_re + (size_t)LK_N * fs;
    float* red = fb_im + (size_t)LK_N * fs;                   // [3][LK_THREADS]; LK_RX: [4][LK_THREADS]
    const int k = threadIdx.x;
    const bool live = k < LK_N;
    const int kk = live ? k : LK_N - 1;                       // idle lanes repeat the last subcarrier and add nothing
    const size_t p = blockIdx.x;
    const float a_unit = M == 1 ? 0.70710678118654752f : 0.31622776601683794f;

    {   // fbb of the packet -> LDS, pitch fs per subcarrier
        const int per = NS * ntrf;
        const float* gre = a.fbb_re + p * (size_t)LK_N * per;
        const float* gim = a.fbb_im + p * (size_t)LK_N * per;
        for (int i = k; i < LK_N * per; i += LK_THREADS) {
            const int q = i / per, e = i - q * per;
            fb_re[q * fs + e] = gre[i];
            fb_im[q * fs + e] = gim[i];
        }
        for (int i = 0; i < 2 * nr * NS; ++i) G[(size_t)i * LK_THREADS + k] = 0.f;
    }
    __syncthreads();
#define LK_G(r, s, z) G[(size_t)(2 * ((r) * NS + (s)) + (z)) * LK_THREADS + k]

    // ---- G = H F (unscaled), |F|_F^2, |H|_F^2
    const float* hre = a.h_re + p * (size_t)nr * nt * LK_N + kk;
    const float* him = a.h_im + p * (size_t)nr * nt * LK_N + kk;
    const float* qre = a.frf_re + p * (size_t)ntrf * nt;
    const float* qim = a.frf_im + p * (size_t)ntrf * nt;
    const float* mre = fb_re + kk * fs;
    const float* mim = fb_im + kk * fs;
    float f2 = 0.f, h2 = 0.f;
    for (int j = 0; j < nt; ++j) {
        float fr[NS], fi[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) fr[s] = fi[s] = 0.f;
        for (int m = 0; m < ntrf; ++m) {
            const float ur = qre[(size_t)m * nt + j], ui = qim[(size_t)m * nt + j];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float br = mre[s * ntrf + m], bi = mim[s * ntrf + m];
                fr[s] = fmaf(ur, br, fmaf(-ui, bi, fr[s]));
                fi[s] = fmaf(ur, bi, fmaf(ui, br, fi[s]));
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) f2 = fmaf(fr[s], fr[s], fmaf(fi[s], fi[s], f2));
        for (int r = 0; r < nr; ++r) {
            const float xr = hre[((size_t)r * nt + j) * LK_N], xi = him[((size_t)r * nt + j) * LK_N];
            h2 = fmaf(xr, xr, fmaf(xi, xi, h2));
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                LK_G(r, s, 0) = fmaf(xr, fr[s], fmaf(-xi, fi[s], LK_G(r, s, 0)));
                LK_G(r, s, 1) = fmaf(xr, fi[s], fmaf(xi, fr[s], LK_G(r, s, 1)));
            }
        }
    }
    // ---- W = sqrt(Nt) F / |F|_F:  G scaled, A = G^H G (lower triangle), |G|_F^2
    const float wscale = f2 > 0.f ? sqrtf((float)nt / f2) : 0.f;
    float Ar[NS][NS], Ai[NS][NS];
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int c = 0; c < NS; ++c) Ar[i][c] = Ai[i][c] = 0.f;
    float g2 = 0.f;
#if LK_RX
    float e2 = 0.f;                                            // |Ghat - G|_F^2
    const float pstd = sqrtf(0.5f * a.noise_var[p]);
    const uint64_t pkey = ss_key(a.seed, (uint64_t)(a.first_pkt + (int64_t)p), LK_KIND_NOISE);
#endif
    for (int r = 0; r < nr; ++r) {
        float gr[NS], gi[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            gr[s] = LK_G(r, s, 0) * wscale;
            gi[s] = LK_G(r, s, 1) * wscale;
            LK_G(r, s, 0) = gr[s];
            LK_G(r, s, 1) = gi[s];
            g2 = fmaf(gr[s], gr[s], fmaf(gi[s], gi[s], g2));
        }
#if LK_RX
        {   // the preamble through row r of G, despread; from here on the row is Ghat's.  No contraction in this block: fused with the
            // product gr = G wscale above, er - gr would be the product's rounding error where Ghat = G (one stream, no noise)
#pragma clang fp contract(off)
            float er[NS], ei[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) er[s] = ei[s] = 0.f;
#pragma unroll
            for (int m = 0; m < NL; ++m) {
                const uint64_t i = (((uint64_t)((n_sym + m) * LK_N + kk) * nr) + r) * 2;
                float yr = pstd * tr_normal(pkey, i), yi = pstd * tr_normal(pkey, i + 1);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    yr += lk_p4(s, m) * gr[s];
                    yi += lk_p4(s, m) * gi[s];
                }
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    er[s] += lk_p4(s, m) * yr;
                    ei[s] += lk_p4(s, m) * yi;
                }
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                er[s] *= 1.f / NL;
                ei[s] *= 1.f / NL;
                const float dr = er[s] - gr[s], di = ei[s] - gi[s];
                e2 = fmaf(dr, dr, fmaf(di, di, e2));
                GH[(size_t)(2 * (r * NS + s)) * LK_THREADS + k] = gr[s] = er[s];
                GH[(size_t)(2 * (r * NS + s) + 1) * LK_THREADS + k] = gi[s] = ei[s];
            }
        }
#endif
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int c = 0; c <= i; ++c) {                     // A[i][c] += conj(g_i) g_c
                Ar[i][c] = fmaf(gr[i], gr[c], fmaf(gi[i], gi[c], Ar[i][c]));
                Ai[i][c] = fmaf(gr[i], gi[c], fmaf(-gi[i], gr[c], Ai[i][c]));
            }
    }
    // ---- Cholesky A = L L^H in place, then Li = L^-1 (lower); [A^-1]_ss = sum_{i >= s} |Li[i][s]|^2
    bool ok = true;
    float dinv[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        float d = Ar[c][c];
#pragma unroll
        for (int q = 0; q < c; ++q) d -= Ar[c][q] * Ar[c][q] + Ai[c][q] * Ai[c][q];
        if (!(d > 0.f) || !(d <= 3.0e38f)) ok = false;
        const float l = sqrtf(ok ? d : 1.f);
        dinv[c] = 1.f / l;
        Ar[c][c] = l;
        Ai[c][c] = 0.f;
#pragma unroll
        for (int i = c + 1; i < NS; ++i) {
            float sr = Ar[i][c], si = Ai[i][c];
#pragma unroll
            for (int q = 0; q < c; ++q) {                      // - L[i][q] conj(L[c][q])
                sr -= Ar[i][q] * Ar[c][q] + Ai[i][q] * Ai[c][q];
                si -= Ai[i][q] * Ar[c][q] - Ar[i][q] * Ai[c][q];
            }
            Ar[i][c] = sr * dinv[c];
            Ai[i][c] = si * dinv[c];
        }
    }
    float Lr[NS][NS], Lm[NS][NS];                              // Li, lower triangle
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        Lr[c][c] = dinv[c];
        Lm[c][c] = 0.f;
#pragma unroll
        for (int i = c + 1; i < NS; ++i) {                     // Li[i][c] = - (sum_{q = c}^{i - 1} L[i][q] Li[q][c]) / L[i][i]
            float sr = 0.f, si = 0.f;
#pragma unroll
            for (int q = c; q < i; ++q) {
                sr += Ar[i][q] * Lr[q][c] - Ai[i][q] * Lm[q][c];
                si += Ar[i][q] * Lm[q][c] + Ai[i][q] * Lr[q][c];
            }
            Lr[i][c] = -sr * dinv[i];
            Lm[i][c] = -si * dinv[i];
        }
    }
    float csi[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float v = 0.f;
#pragma unroll
        for (int i = s; i < NS; ++i) v += Lr[i][s] * Lr[i][s] + Lm[i][s] * Lm[i][s];
        csi[s] = ok ? 1.f / v : 0.f;
        if (!(csi[s] <= 3.0e38f)) { csi[s] = 0.f; ok = false; }
    }
    if (!ok) {
#pragma unroll
        for (int s = 0; s < NS; ++s) csi[s] = 0.f;
    }
    if (a.csi && live) {
#pragma unroll
        for (int s = 0; s < NS; ++s) a.csi[(p * NS + s) * LK_N + k] = csi[s];
    }
#if LK_RX
    if (b.gest_re) {   // the same for every lane of the packet.  [234][nr][NS]: through LDS, so that the stores run along the plane
        __syncthreads();
        const int per = nr * NS;
        float* ore = b.gest_re + p * (size_t)LK_N * per;
        float* oim = b.gest_im + p * (size_t)LK_N * per;
        for (int i = k; i < LK_N * per; i += LK_THREADS) {
            const int q = i / per, e = i - q * per;
            ore[i] = GH[(size_t)(2 * e) * LK_THREADS + q];
            oim[i] = GH[(size_t)(2 * e + 1) * LK_THREADS + q];
        }
    }
#endif

    // ---- the data symbols
    const float nv = a.noise_var[p];
    const float nstd = sqrtf(0.5f * nv);
    float lscale[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) lscale[s] = nv > 0.f ? csi[s] / nv : csi[s];
    const uint64_t kn = ss_key(a.seed, (uint64_t)(a.first_pkt + (int64_t)p), LK_KIND_NOISE);
    const size_t n_coded = (size_t)NS * n_sym * LK_N * BPS;
    const uint8_t* cb = a.coded + p * n_coded;
    float* lo = a.llr + p * n_coded;
    float evm = 0.f;
    for (int n = 0; n < n_sym; ++n) {
        float dr[NS], di[NS], zr[NS], zi[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const uint8_t* c = cb + ((size_t)(s * n_sym + n) * LK_N + kk) * BPS;
            int b[BPS];
#pragma unroll
            for (int i = 0; i < BPS; ++i) b[i] = c[i];
            dr[s] = a_unit * lk_pam_level<M>(b);
            di[s] = a_unit * lk_pam_level<M>(b + M);
            zr[s] = zi[s] = 0.f;
        }
        const uint64_t base = ((uint64_t)(n * LK_N + kk) * nr) * 2;
        for (int r = 0; r < nr; ++r) {
            float yr = nstd * tr_normal(kn, base + 2 * r), yi = nstd * tr_normal(kn, base + 2 * r + 1);
            float gr[NS], gi[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                gr[s] = LK_G(r, s, 0);
                gi[s] = LK_G(r, s, 1);
                yr = fmaf(gr[s], dr[s], fmaf(-gi[s], di[s], yr));
                yi = fmaf(gr[s], di[s], fmaf(gi[s], dr[s], yi));
            }
#if LK_RX
#pragma unroll
            for (int s = 0; s < NS; ++s) {                     // y came through G; the matched filter is the estimate's
                gr[s] = GH[(size_t)(2 * (r * NS + s)) * LK_THREADS + k];
                gi[s] = GH[(size_t)(2 * (r * NS + s) + 1) * LK_THREADS + k];
            }
#endif
#pragma unroll
            for (int s = 0; s < NS; ++s) {                     // z += conj(g) y
                zr[s] = fmaf(gr[s], yr, fmaf(gi[s], yi, zr[s]));
                zi[s] = fmaf(gr[s], yi, fmaf(-gi[s], yr, zi[s]));
            }
        }
        // x = Li^H (Li z)
        float vr[NS], vi[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            float sr = 0.f, si = 0.f;
#pragma unroll
            for (int c = 0; c <= i; ++c) {
                sr += Lr[i][c] * zr[c] - Lm[i][c] * zi[c];
                si += Lr[i][c] * zi[c] + Lm[i][c] * zr[c];
            }
            vr[i] = sr;
            vi[i] = si;
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float xr = 0.f, xi = 0.f;
#pragma unroll
            for (int i = s; i < NS; ++i) {                     // conj(Li[i][s]) v_i
                xr += Lr[i][s] * vr[i] + Lm[i][s] * vi[i];
                xi += Lr[i][s] * vi[i] - Lm[i][s] * vr[i];
            }
            if (!ok) xr = xi = 0.f;
            float dI[M], dQ[M];
            const float eI = lk_pam_soft<M>(xr, a_unit, dI), eQ = lk_pam_soft<M>(xi, a_unit, dQ);
            if (live) {
                evm += eI + eQ;
                float* l = lo + ((size_t)(s * n_sym + n) * LK_N + k) * BPS;
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    l[i] = lscale[s] * dI[i];
                    l[M + i] = lscale[s] * dQ[i];
                }
                if (a.xeq_re) {
                    const size_t o = ((p * NS + s) * n_sym + n) * LK_N + k;
                    a.xeq_re[o] = xr;
                    a.xeq_im[o] = xi;
                }
            }
        }
    }
#undef LK_G
    // ---- the packet's sums: a fixed tree over the lanes
    red[k] = live ? evm : 0.f;
    red[LK_THREADS + k] = live ? g2 : 0.f;
    red[2 * LK_THREADS + k] = live ? h2 : 0.f;
#if LK_RX
    red[3 * LK_THREADS + k] = live ? e2 : 0.f;
#endif
    __syncthreads();
    for (int w = LK_THREADS / 2; w > 0; w >>= 1) {
        if (k < w) {
            red[k] += red[k + w];
            red[LK_THREADS + k] += red[LK_THREADS + k + w];
            red[2 * LK_THREADS + k] += red[2 * LK_THREADS + k + w];
#if LK_RX
            red[3 * LK_THREADS + k] += red[3 * LK_THREADS + k + w];
#endif
        }
        __syncthreads();
    }
    if (k == 0) {
        a.evm_rms[p] = 100.f * sqrtf(red[0] / ((float)NS * (float)n_sym * (float)LK_N));
        a.dt_snr_db[p] = 10.f * log10f(red[LK_THREADS] / red[2 * LK_THREADS]);
#if LK_RX
        const float num = red[3 * LK_THREADS], den = red[LK_THREADS];
        b.g_nmse[p] = (num == 0.f && den == 0.f) ? 0.f : num / den;
#endif
    }
