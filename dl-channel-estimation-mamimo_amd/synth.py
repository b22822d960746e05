"""Synthetic inputs for benchmarks and smoke runs.  The reference ships neither trained
weights nor datasets (README.md:17-18), so throughput is measured on random-initialised
weights of the shipped architecture and synthetic packets of the shipped shape."""
import numpy as np

SYM_LEN = 320


def hadamard(n):
    """Sylvester-Hadamard pilot mapping matrix; stand-in for the un-vendored helperGetP
    (helperMIMOChannelEstimate.m:13).  In the real pipeline P arrives with the dataset."""
    if n < 1 or n & (n - 1):
        raise ValueError('hadamard(n) needs a power of two')
    h = np.ones((1, 1), dtype=np.float32)
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h.astype(np.float32)


def make_weights(rng, nt, hidden=(1024, 1024), n_out=234, use_bn=True):
    """Random weights with the keras initialisers of the reference model
    (glorot_uniform kernels, DNN.py:213,227) and non-trivial BatchNormalization statistics."""
    w = {}
    fan_in = SYM_LEN * nt + nt
    for i, h in enumerate(hidden):
        lim = np.sqrt(6.0 / (fan_in + h))
        w[f'fc_dense{i}.kernel'] = rng.uniform(-lim, lim, (fan_in, h)).astype(np.float32)
        w[f'fc_dense{i}.bias'] = (0.01 * rng.standard_normal(h)).astype(np.float32)
        if use_bn:
            w[f'bn{i}.gamma'] = rng.uniform(0.5, 1.5, h).astype(np.float32)
            w[f'bn{i}.beta'] = (0.1 * rng.standard_normal(h)).astype(np.float32)
            w[f'bn{i}.moving_mean'] = (0.1 * rng.standard_normal(h)).astype(np.float32)
            w[f'bn{i}.moving_variance'] = rng.uniform(0.5, 1.5, h).astype(np.float32)
        fan_in = h
    lim = np.sqrt(6.0 / (fan_in + n_out))
    w['fc_regressor.kernel'] = rng.uniform(-lim, lim, (fan_in, n_out)).astype(np.float32)
    w['fc_regressor.bias'] = (0.01 * rng.standard_normal(n_out)).astype(np.float32)
    return w


def white_packets(rng, npkt, nr, nt):
    """i.i.d. CN(0,1) preambles, complex64 [npkt, nr, 320*nt] (host twin of csi_synth_white's
    distribution, not of its stream)."""
    shape = (npkt, nr, SYM_LEN * nt)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)).astype(np.complex64)


# ---- structured sounding packets (the synthetic twin of generate_maMIMO_LTF.m:197-342) -----------
FFT_LEN, CP_LEN = 256, 64
SNR_LEVELS_DB = (-25, -20, -15, -10, -5, 0, 5, 10)      # setenv.sh:19-25 (SNRLev), 500 test packets per level
AMP_SCALE = np.sqrt(FFT_LEN - 14) / FFT_LEN             # generate_maMIMO_LTF.m:303-304: sqrt(FFTLength - #nulls) / FFTLength


def vht_ltf_sequence():
    """256-bin VHT-LTF frequency sequence of helperMIMOChannelEstimate.m:16-23, fftshift-ed order
    (index 0 = most negative frequency); 0 on the 7 + 1 + 6 null bins of generate_maMIMO_LTF.m:99."""
    left = [1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1]
    right = [1, -1, -1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1, -1, 1, -1, 1, 1, 1, 1]
    mid_a = [-1, -1, -1, 1, 1, -1, 1, -1, 1, 1, -1]
    mid_b = [1, -1, 1, -1, 0, 1, -1, -1, 1]
    seg = left + [1] + right
    seq = [0] * 7 + seg + mid_a + seg + mid_b + seg + mid_a + seg + [0] * 6
    assert len(seq) == FFT_LEN
    return np.asarray(seq, dtype=np.float32)


def structured_packets(rng, npkt, nr, P, snr_db, n_taps=8):
    """Sounding packets as the reference's simulator hands them to the estimators: every (rx, tx) link
    an n_taps complex Gaussian impulse response, the Nt LTF symbols mapped by P, OFDM-modulated with
    the 64-sample cyclic prefix (generate_maMIMO_LTF.m:202,210), complex AWGN at `snr_db` relative to
    the received preamble power (:283-295; `snr_db` scalar or one value per packet), then the
    sub-carrier power scaling of :303-304 applied to signal AND noise, as there.  The signal level is
    the same at every SNR - only the noise moves - so a batch that mixes levels spans the amplitude
    range the reference's test set spans.  Returns complex64 [npkt, nr, 320*nt]."""
    P = np.asarray(P, dtype=np.float32)
    nt = P.shape[0]
    snr = np.broadcast_to(np.asarray(snr_db, dtype=np.float64), (npkt,))
    decay = (np.exp(-0.5 * np.arange(n_taps)) / np.sqrt(2.0)).astype(np.float32)
    cir = np.zeros((npkt * nr, nt, FFT_LEN), dtype=np.complex64)
    cir.real[..., :n_taps] = rng.standard_normal((npkt * nr, nt, n_taps), dtype=np.float32) * decay
    cir.imag[..., :n_taps] = rng.standard_normal((npkt * nr, nt, n_taps), dtype=np.float32) * decay
    h = np.fft.fft(cir, axis=-1)                                           # [pr, j, bin], un-shifted bin order
    # frequency-domain LTF symbols X[pr, s, k] = ltf[k] * sum_j H[pr, j, k] P[j, s]
    xf = np.matmul(np.ascontiguousarray(P.T).astype(np.complex64), h)      # [pr, s, bin]
    xf *= np.fft.ifftshift(vht_ltf_sequence())[None, None, :]
    xt = np.fft.ifft(xf, axis=-1)                                          # [pr, s, n]
    ltf = np.empty((npkt * nr, nt, SYM_LEN), dtype=np.complex64)
    ltf[..., :CP_LEN] = xt[..., -CP_LEN:]                                  # cyclic prefix
    ltf[..., CP_LEN:] = xt
    ltf = ltf.reshape(npkt, nr, nt * SYM_LEN)
    sig_pow = float(np.mean(ltf.real ** 2 + ltf.imag ** 2))
    nstd = np.sqrt(sig_pow / (10.0 ** (snr / 10.0)) / 2.0).astype(np.float32)       # per packet, per real component
    for part in (ltf.real, ltf.imag):
        part += rng.standard_normal(ltf.shape, dtype=np.float32) * nstd[:, None, None]
    ltf *= np.float32(AMP_SCALE)
    return ltf


# ---- geometric single-bounce scattering channel (csi_synth_scattering) -----------
LIGHT_SPEED = 299792458.0


def scattering_channel(u, g, R, az_deg, el_deg, nr, nt, box_frac=0.1, sample_rate_hz=100e6, details=False):
    """The channel model of csi_synth_scattering in float64 (include/csi_mamimo.h states it; what phased.ScatteringMIMOChannel
    models in helperApplyMUChannel.m:44-143, restated from the physics).  u [S][3]: the uniform draws in (0, 1) that place the
    scatterers in the box of half edge box_frac * R around the receiver; g [S] complex reflection coefficients; the user sits at
    distance R in direction (az_deg, el_deg) of the transmitter; both arrays are half-wavelength ULAs along y.

        e = (cos el cos az, cos el sin az, sin el),  o_s = box_frac R (2 u_s - 1),  q_s = R e + o_s
        x_s = (2 R (e . o_s) + |o_s|^2) / (|q_s| + R) + |o_s|           excess path, = |q_s| - R + |o_s| without the cancellation
        tau_s = (x_s - min x) fs / c                                      excess delay in samples: the first path sits at 0
        v_s = q_s,y / |q_s|,  w_s = o_s,y / |o_s|                         direction cosines along the array axis
        H[r][j][k] = S^(-1/2) sum_s g_s exp(2 pi i z_r w_s) exp(-2 pi i y_j v_s) exp(-2 pi i f_k tau_s / 256)

    with y_j = (j - (nt - 1) / 2) / 2, z_r = (r - (nr - 1) / 2) / 2 and f_k the SIGNED index of FFT bin k (k < 128: k, else k - 256).
    The transmit factor is the conjugate of steering_ula: a single scatterer's H has steering_ula at (v_s) as its dominant right
    singular vector.  Returns (H complex128 [nr][nt][256] in FFT bin order, tau [S] = (R + x_s) fs / c, the absolute path delays in
    samples); details=True adds a dict with x, tau_excess, v, w."""
    u = np.asarray(u, np.float64).reshape(-1, 3)
    g = np.asarray(g, np.complex128).reshape(-1)
    S = g.size
    if u.shape[0] != S or S < 1:
        raise ValueError('u must be [S][3] and g [S] with S >= 1')
    R, az, el = float(R), np.deg2rad(float(az_deg)), np.deg2rad(float(el_deg))
    e = np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    o = box_frac * R * (2.0 * u - 1.0)
    q = R * e + o
    on, qn = np.linalg.norm(o, axis=1), np.linalg.norm(q, axis=1)
    x = (2.0 * R * (o @ e) + on ** 2) / (qn + R) + on
    spm = float(sample_rate_hz) / LIGHT_SPEED
    tau_ex = (x - x.min()) * spm
    v = q[:, 1] / qn
    w = np.divide(o[:, 1], on, out=np.zeros(S), where=on > 0)
    y = (np.arange(nt) - (nt - 1) / 2.0) / 2.0
    z = (np.arange(nr) - (nr - 1) / 2.0) / 2.0
    f = np.fft.fftfreq(FFT_LEN, 1.0 / FFT_LEN)                                # 0 .. 127, -128 .. -1
    rx = g[None, :] * np.exp(2j * np.pi * z[:, None] * w[None, :])             # [r, s]
    tx = np.exp(-2j * np.pi * y[:, None] * v[None, :])                         # [j, s]
    dl = np.exp(-2j * np.pi * f[:, None] * tau_ex[None, :] / FFT_LEN)          # [k, s]
    H = np.einsum('rs,js,ks->rjk', rx, tx, dl) / np.sqrt(S)
    tau = (R + x) * spm
    if details:
        return H, tau, dict(x=x, tau_excess=tau_ex, v=v, w=w)
    return H, tau


def scattering_packets(rng, npkt, nr, P, snr_db, n_scat=100, range_m=100.0, az_deg=30.0, el_deg=0.0, box_frac=0.1, random_users=False,
                       sample_rate_hz=100e6, return_channel=False):
    """Host twin of csi_synth_scattering's distribution (not of its stream), as structured_packets is of the tap model's: per
    packet n_scat scatterers uniform in the box, CN(0, 1) reflection coefficients, the user fixed or - random_users - drawn as
    generate_maMIMO_LTF.m:48-51 draws it (range 1 .. range_m, azimuth +-180, elevation +-90 degrees); the LTF symbols mapped by P,
    OFDM-modulated with the cyclic prefix, AWGN at `snr_db` (scalar or per packet; None = noise-free) relative to each packet's own
    power, then the sub-carrier power scaling.  Returns complex64 [npkt, nr, 320 nt]; return_channel=True returns
    (ltf, H complex128 [npkt, nr, nt, 256] before the scaling, tau [npkt, n_scat])."""
    P = np.asarray(P, dtype=np.float64)
    nt = P.shape[0]
    ltf_seq = np.fft.ifftshift(vht_ltf_sequence()).astype(np.float64)
    out = np.empty((npkt, nr, nt * SYM_LEN), np.complex64)
    Hs, taus = np.empty((npkt, nr, nt, FFT_LEN), np.complex128), np.empty((npkt, n_scat))
    snr = None if snr_db is None else np.broadcast_to(np.asarray(snr_db, dtype=np.float64), (npkt,))
    for p in range(npkt):
        R, az, el = float(range_m), float(az_deg), float(el_deg)
        if random_users:
            R, az, el = 1.0 + (range_m - 1.0) * rng.random(), rng.uniform(-180.0, 180.0), rng.uniform(-90.0, 90.0)
        g = (rng.standard_normal(n_scat) + 1j * rng.standard_normal(n_scat)) / np.sqrt(2.0)
        H, tau = scattering_channel(rng.random((n_scat, 3)), g, R, az, el, nr, nt, box_frac, sample_rate_hz)
        x = np.fft.ifft(np.einsum('rjk,js->rsk', H, P) * ltf_seq, axis=-1)
        ltf = np.concatenate([x[..., -CP_LEN:], x], axis=-1).reshape(nr, nt * SYM_LEN)
        if snr is not None:
            nstd = np.sqrt(np.mean(np.abs(ltf) ** 2) / 10.0 ** (snr[p] / 10.0) / 2.0)
            ltf = ltf + nstd * (rng.standard_normal(ltf.shape) + 1j * rng.standard_normal(ltf.shape))
        out[p] = ltf * AMP_SCALE
        Hs[p], taus[p] = H, tau
    return (out, Hs, taus) if return_channel else out


def cfo_offsets(seed, first_pkt, npkt, max_eps):
    """Carrier frequency offsets of packets first_pkt .. first_pkt + npkt - 1 in subcarrier spacings (the eps of
    CsiEngine.cfo_rotate_device): float64 [npkt], uniform in [-max_eps, max_eps].  Packet i's draw is a hash of (seed, i) alone
    (two rounds of the splitmix64 finaliser, the top 53 bits as the uniform), so the SNR levels of a sweep, its chunks and any
    sub-range of a longer call see the same offset for the same packet."""
    def mix(z):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))
    with np.errstate(over='ignore'):
        i = np.arange(int(first_pkt), int(first_pkt) + int(npkt), dtype=np.uint64)
        z = mix(mix(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + np.uint64(0x9E3779B97F4A7C15)) + (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))
    u = (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53          # [0, 1)
    return float(max_eps) * (2.0 * u - 1.0)


def timing_offsets(seed, first_pkt, npkt, span):
    """Packet starts of packets first_pkt .. first_pkt + npkt - 1 inside captures of len_ltf + span samples (the theta of
    CsiEngine.sync_embed_device): int32 [npkt], uniform in 0 .. span.  Packet i's draw is a hash of (seed, i) alone, the hash of
    cfo_offsets under its own tag, so the levels of a sweep, its chunks and any sub-range of a longer call see the same start for the
    same packet, and a packet's start is independent of its frequency offset."""
    def mix(z):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))
    with np.errstate(over='ignore'):
        i = np.arange(int(first_pkt), int(first_pkt) + int(npkt), dtype=np.uint64)
        z = mix(mix((np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ np.uint64(0x53594E43)) + np.uint64(0x9E3779B97F4A7C15)) + (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))
    u = (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53          # [0, 1)
    return np.minimum(np.floor(u * (int(span) + 1)), int(span)).astype(np.int32)


def link_noise_var(noise_std, amp_scale=True):
    """Noise variance per complex frequency-domain sample, in the units of the channel planes h, that goes with a sounding packet
    of csi_synth_structured: the time samples carry amp * noise_std per real component (2 amp^2 noise_std^2 per complex sample), and
    the 256-point transform the LS kernel takes sums 256 of them: 512 amp^2 noise_std^2 (csrc/synth_structured.hip.h:6-11).  The LS
    estimate of a link averages Nt such bins (P P^T = Nt I), so its error variance is this value / Nt.  `noise_std` is the array
    synth_structured returns (before the amplitude scale); a data symbol of the link simulation sees the same level."""
    amp = float(np.float32(AMP_SCALE)) if amp_scale else 1.0
    return (2.0 * FFT_LEN * amp * amp) * np.asarray(noise_std, dtype=np.float64) ** 2


def mixed_snr_jobs(seed, per_level=500, levels=SNR_LEVELS_DB, block=250):
    """BASELINE config 2's defining input: `per_level` test packets at EACH of the pipeline's SNR levels
    (setenv.sh:19-25, full_pipeline_maMIMO_DNNEst.sh:44-48), level after level (lowest SNR first), so
    that ONE launch sees the whole 35 dB spread.  The batch is cut into blocks of <= `block` packets with
    one independent random stream each (SeedSequence children of `seed`), so that blocks can be produced
    in any order / in parallel and any block can be regenerated alone (the parity checks do that).
    Returns [(first_packet, n_packets, snr_db, SeedSequence)]."""
    jobs, first = [], 0
    for lv in levels:
        left = per_level
        while left > 0:
            n = min(block, left)
            jobs.append([first, n, float(lv)])
            first += n
            left -= n
    for job, ss in zip(jobs, np.random.SeedSequence(seed).spawn(len(jobs))):
        job.append(ss)
    return [tuple(j) for j in jobs]


def mixed_snr_block(job, nr, P):
    """The packets of one job of mixed_snr_jobs: complex64 [n, nr, 320*nt]."""
    first, n, snr_db, ss = job
    return structured_packets(np.random.default_rng(ss), n, nr, P, snr_db)


def mixed_snr_batch(seed, nr, P, per_level=500, levels=SNR_LEVELS_DB, block=250, threads=2):
    """Generator over the blocks of the mixed-SNR batch, produced by a small thread pool (numpy's FFT and
    normal generator release the GIL): yields (first_packet, snr_db, complex64 [n, nr, 320*nt]) in order."""
    from concurrent.futures import ThreadPoolExecutor
    jobs = mixed_snr_jobs(seed, per_level, levels, block)
    with ThreadPoolExecutor(max_workers=max(1, threads)) as pool:
        pending = []
        it = iter(jobs)
        for job in it:
            pending.append((job, pool.submit(mixed_snr_block, job, nr, P)))
            if len(pending) >= max(1, threads):
                j, f = pending.pop(0)
                yield j[0], j[2], f.result()
        for j, f in pending:
            yield j[0], j[2], f.result()


def steering_ula(nt, az_deg, el_deg=0.0, spacing=0.5):
    """Array responses of a uniform linear array of nt elements along the y axis, spacing in wavelengths:
    a_n = exp(2 pi i y_n cos(el) sin(az)), y_n = (n - (nt - 1) / 2) * spacing.  az_deg / el_deg broadcast against each
    other; returns complex128 [nt][rays], the dictionary layout of CsiEngine.set_dictionary.  The sign and the axis
    convention of the toolbox's steervec (which the reference calls) cannot be pinned without MATLAB and may differ
    from this one by a conjugation or a mirror of the azimuth; nothing in the library depends on it, since the
    dictionary is an input."""
    az, el = np.broadcast_arrays(np.deg2rad(np.asarray(az_deg, np.float64)), np.deg2rad(np.asarray(el_deg, np.float64)))
    y = (np.arange(nt, dtype=np.float64) - (nt - 1) / 2.0) * spacing
    u = (np.cos(el) * np.sin(az)).reshape(-1)
    return np.exp(2j * np.pi * y[:, None] * u[None, :])


def random_rays(rng, n):
    """n ray directions as BER_test_maMIMO_LTF.m:364 draws them: azimuth uniform in +-180 degrees, elevation uniform
    in +-90 degrees.  Returns (az_deg [n], el_deg [n])."""
    az = rng.uniform(-180.0, 180.0, n)
    el = rng.uniform(-90.0, 90.0, n)
    return az, el
