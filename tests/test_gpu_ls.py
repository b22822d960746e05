"""GPU tests (-m gpu; every call through the C-ABI of libcsi_mamimo.so, checked against the numpy oracle on identical seeded inputs at the
1e-5 norm-relative contract of BASELINE.json unless a test states its own): LS pilot estimate (helperMIMOChannelEstimate.m:24-36 / generate_maMIMO_LTF.m:336-342) and the LMMSE smoother (LMMSE_ce.m:23-39): every LS kernel against the oracle, known channels, the reference-produced OFDM fixture."""
import sys

import os

import numpy as np
import pytest

from conftest import rel_rows

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


TOL = 1e-5


def _pilot(rng, nt, orthogonal=True):
    from oracle import csi_oracle as o
    if orthogonal:
        P = o.hadamard(nt)
        return (P[rng.permutation(nt)] * rng.choice([-1.0, 1.0], nt)[:, None]).astype(np.float64)
    return rng.integers(-3, 4, (nt, nt)).astype(np.float64)


P_VHT4 = np.array([[1, -1, 1, 1], [1, 1, -1, 1], [1, 1, 1, -1], [-1, 1, 1, 1]], np.float64)


def vht_pilot(oracle, nt):
    """kron(H_{nt/4}, P_VHT4): Hadamard, NOT in the Sylvester order."""
    return np.kron(oracle.hadamard(nt // 4), P_VHT4)


def signed_perm_pilot(oracle, rng, nt):
    """D1 Pi1 H Pi2 D2 with random permutations and signs."""
    H = oracle.hadamard(nt)
    return (rng.choice([-1.0, 1.0], nt)[:, None] * H[rng.permutation(nt)][:, rng.permutation(nt)]) * rng.choice([-1.0, 1.0], nt)[None, :]


FAST_PILOT_CASES = [(16, 4, 40), (32, 4, 30), (64, 2, 12), (128, 2, 5)]


def _weights(oracle, seed, nt, hidden, use_bn=True, n_out=234):
    rng = np.random.default_rng(seed)
    d_in = 320 * nt + nt
    return (oracle.make_weights(rng, d_in, list(hidden), n_out, use_bn=use_bn),
            oracle.make_weights(rng, d_in, list(hidden), n_out, use_bn=use_bn))


# ------------------------------------------------------------------------------------ LS
@pytest.mark.parametrize('nt,nr,npkt', [(4, 2, 3), (8, 1, 5), (16, 3, 2), (32, 4, 4), (64, 4, 2), (128, 2, 2)])
def test_ls_matches_oracle_and_known_channel(pkg, oracle, nt, nr, npkt):
    rng = np.random.default_rng(100 + nt)
    P = _pilot(rng, nt)
    ltf, H = oracle.make_structured_packets(rng, npkt, nr, P, snr_db=None)
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(P)
    h = e.ls_estimate(ltf)
    assert h.shape == (npkt, nr, nt, 234) and h.dtype == np.complex64
    ref = oracle.ls_estimate(ltf, P)
    assert rel_rows(np.concatenate([h.real, h.imag], -1), np.concatenate([ref.real, ref.imag], -1)) < TOL
    # known-answer: noiseless structured packet -> LS == H
    assert rel_rows(np.concatenate([h.real, h.imag], -1), np.concatenate([H.real, H.imag], -1)) < TOL


def test_ls_kernel_on_reference_ofdm_fixture(pkg, oracle, golden_dir):
    """The LS kernels against spectra the REFERENCE computed: tests/golden/ref_ofdm_reshape_nt4.npz holds the
    per-symbol FFTs recorded from massiveMIMO_dataGenerator.py:425-453 (method 'reshape') on the Nt=4 fixture
    preambles.  Despreading those spectra (helperMIMOChannelEstimate.m:24-36, non-symmetric P) must give what
    the HIP kernels compute from the time-domain preambles - symbol split, CP window, FFT and bin order of
    the kernels are thereby checked against reference-executed output, for every LS kernel that serves Nt=4."""
    g = np.load(os.path.join(golden_dir, 'ref_ofdm_reshape_nt4.npz'))
    nt, nr, npkt = int(g['nt']), int(g['nr']), int(g['npkt'])
    spec = g['real_fft_pre_shift'] + 1j * g['imag_fft_pre_shift']                       # [pr, 256, nt], FFT bin order
    rx = np.fft.fftshift(spec, axes=1)[:, oracle.data_carrier_indices() - 1, :]
    want = np.swapaxes(oracle.ls_from_rxsym(rx, g['P_matlab']), -1, -2).reshape(npkt, nr, nt, 234)
    want2 = np.concatenate([want.real, want.imag], -1)
    ltf = (g['ds_ltf_real'] + 1j * g['ds_ltf_imag']).reshape(npkt, nr, 320 * nt)
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(g['P_matlab'])
    for kernel in (0, 1, 3):                                                            # automatic, FFT-first, despread-first
        e.set_option('ls_kernel', kernel)
        h = e.ls_estimate(ltf)
        assert rel_rows(np.concatenate([h.real, h.imag], -1), want2) < TOL, kernel


def test_ls_noisy_generic_pilot_and_linearity(pkg, oracle):
    rng = np.random.default_rng(7)
    nt, nr, npkt = 8, 2, 6
    P = _pilot(rng, nt, orthogonal=False)            # generic real P: no Hadamard assumption
    a = oracle.make_structured_packets(rng, npkt, nr, oracle.hadamard(nt), snr_db=0.0)[0]
    b = (rng.standard_normal(a.shape) + 1j * rng.standard_normal(a.shape))
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(P)
    ha, hb = e.ls_estimate(a), e.ls_estimate(b)
    ref = oracle.ls_estimate(a, P)
    assert rel_rows(np.concatenate([ha.real, ha.imag], -1), np.concatenate([ref.real, ref.imag], -1)) < TOL
    hab = e.ls_estimate(2.0 * a - 0.5 * b)
    lin = 2.0 * ha.astype(np.complex128) - 0.5 * hb.astype(np.complex128)
    assert rel_rows(np.concatenate([hab.real, hab.imag], -1), np.concatenate([lin.real, lin.imag], -1)) < 5e-6


@pytest.mark.parametrize('nt', [12, 72, 96])
def test_ls_non_power_of_two_nt_generic_pilot(pkg, oracle, nt):
    """Nt that is not a power of two (partial 32-row MFMA tiles, and for Nt > 64 the
    despread-first kernel with a partial last chunk), generic real P."""
    rng = np.random.default_rng(nt)
    P = rng.integers(-2, 3, (nt, nt)).astype(np.float64)
    ltf = rng.standard_normal((2, 2, 320 * nt)) + 1j * rng.standard_normal((2, 2, 320 * nt))
    e = pkg.CsiEngine(nt, 2, hidden=(8,))
    e.set_pilot(P)
    h = e.ls_estimate(ltf)
    ref = oracle.ls_estimate(ltf.astype(np.complex64), P)
    assert rel_rows(np.concatenate([h.real, h.imag], -1), np.concatenate([ref.real, ref.imag], -1)) < TOL


@pytest.mark.parametrize('kernel', [1, 2, 3, 6])
def test_ls_all_kernels_agree(pkg, oracle, kernel):
    """The generic LS kernels (1 FFT-first, 2 chunked FFT-first, 3 despread-first, 6 LDS-DMA ring) against the oracle on
    every Nt each of them serves, incl. partial MFMA tiles and partial symbol chunks (Nt = 40, 72, 100)
    and many more items than resident workgroups (persistent loops)."""
    rng = np.random.default_rng(kernel + 3)
    cases = {1: ((8, 2, 3), (32, 3, 3), (64, 2, 3), (40, 1, 2)),
             2: ((40, 2, 3), (64, 2, 3), (72, 1, 2), (96, 2, 2), (100, 1, 2), (128, 2, 2), (64, 4, 300)),
             3: ((8, 2, 3), (64, 2, 3), (72, 1, 2), (128, 2, 2), (160, 1, 1)),
             # 6 = the chunked kernel's successor on the LDS-DMA ring (generic P): every antenna-tile count, partial last chunks
             6: ((16, 2, 5), (24, 2, 3), (32, 3, 300), (40, 2, 3), (64, 2, 3), (72, 1, 2), (96, 2, 2), (100, 1, 2), (128, 2, 2),
                 (64, 4, 300), (128, 3, 100))}[kernel]
    for nt, nr, npkt in cases:
        P = _pilot(rng, nt) if nt & (nt - 1) == 0 else rng.integers(-2, 3, (nt, nt)).astype(np.float64)
        if npkt > 10:
            ltf = pkg.synth.white_packets(rng, npkt, nr, nt)
        else:
            ltf = rng.standard_normal((npkt, nr, 320 * nt)) + 1j * rng.standard_normal((npkt, nr, 320 * nt))
        e = pkg.CsiEngine(nt, nr, hidden=(8,))
        e.set_option('ls_kernel', kernel)
        e.set_pilot(P)
        h = e.ls_estimate(ltf)
        sel = slice(None) if npkt <= 10 else np.r_[0:2, npkt - 2:npkt]
        ref = oracle.ls_estimate(np.asarray(ltf)[sel].astype(np.complex64), P)
        assert rel_rows(np.concatenate([h[sel].real, h[sel].imag], -1), np.concatenate([ref.real, ref.imag], -1)) < TOL, (nt, nr, npkt)
        if npkt > 10:       # persistent walk: every item written, and identical on a second run
            assert np.isfinite(h.view(np.float32)).all() and np.abs(h).sum(axis=(1, 2, 3)).min() > 0
            assert np.array_equal(h, e.ls_estimate(ltf))


@pytest.mark.parametrize('nt,nr,npkt', [(16, 2, 5), (32, 3, 300), (64, 2, 7), (128, 2, 3), (16, 4, 400), (64, 4, 300), (128, 2, 200)])
def test_ls_walsh_hadamard_despread(pkg, oracle, nt, nr, npkt):
    """With the Sylvester Hadamard pilot matrix the LS despread is a fast Walsh-Hadamard transform
    (chosen automatically): same answer as the oracle and as the MFMA despread (ls_kernel 2) up to the
    summation order; a P that is not exactly that matrix must not take it."""
    rng = np.random.default_rng(nt + npkt)
    P = oracle.hadamard(nt)
    ltf = (rng.standard_normal((npkt, nr, 320 * nt)) + 1j * rng.standard_normal((npkt, nr, 320 * nt))).astype(np.complex64)
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(P)
    h = e.ls_estimate(ltf)                       # automatic -> Walsh-Hadamard kernel
    sel = slice(None) if npkt <= 10 else np.r_[0:2, npkt - 2:npkt]
    ref = oracle.ls_estimate(ltf[sel], P)
    assert rel_rows(np.concatenate([h[sel].real, h[sel].imag], -1), np.concatenate([ref.real, ref.imag], -1)) < TOL
    e.set_option('ls_kernel', 2)
    h2 = e.ls_estimate(ltf)                      # MFMA despread
    assert not np.array_equal(h, h2)             # really another kernel (summation order differs) ...
    assert rel_rows(np.concatenate([h.real, h.imag], -1).reshape(-1, 468), np.concatenate([h2.real, h2.imag], -1).reshape(-1, 468)) < 2e-6
    e.set_option('ls_kernel', 0)
    assert np.array_equal(h, e.ls_estimate(ltf))                 # deterministic
    # the two generations of the kernel (4: register prefetch, 5 = automatic: LDS-DMA ring) and both shapes of the
    # second (16- and 8-symbol chunks group the additions differently) agree to rounding; every item is written
    for opt, val in (('ls_kernel', 4), ('ls_v2', 1)):
        e.set_option('ls_kernel', 0)
        e.set_option(opt, val)
        h4 = e.ls_estimate(ltf)
        assert rel_rows(np.concatenate([h.real, h.imag], -1).reshape(-1, 468), np.concatenate([h4.real, h4.imag], -1).reshape(-1, 468)) < 1e-6, (opt, val)
    e.set_option('ls_v2', 0)
    e.set_option('ls_kernel', 0)
    # a pilot matrix that differs from the Sylvester matrix in one sign: generic path, still right
    P2 = P.copy()
    P2[3, 5] = -P2[3, 5]
    e2 = pkg.CsiEngine(nt, nr, hidden=(8,))
    e2.set_pilot(P2)
    e2.set_option('ls_kernel', 4)                # forcing it is refused silently (falls back)
    g = e2.ls_estimate(ltf[:2])
    ref2 = oracle.ls_estimate(ltf[:2], P2)
    assert rel_rows(np.concatenate([g.real, g.imag], -1), np.concatenate([ref2.real, ref2.imag], -1)) < TOL


@pytest.mark.parametrize('nt,nr,npkt', [(4, 2, 2), (32, 2, 1), (40, 1, 1)])
def test_lmmse_matches_reference_formula(pkg, oracle, nt, nr, npkt):
    """LMMSE smoothing (LMMSE_ce.m, one 234x234 inverse per link in the reference; one Levinson solve
    per (packet, rx) here) against the literal restatement of the reference formula in fp64."""
    rng = np.random.default_rng(900 + nt)
    P = oracle.hadamard(nt) if nt & (nt - 1) == 0 else rng.integers(-2, 3, (nt, nt)).astype(np.float64)
    ltf = rng.standard_normal((npkt, nr, 320 * nt)) + 1j * rng.standard_normal((npkt, nr, 320 * nt))
    e = pkg.CsiEngine(nt, nr, hidden=(8,))
    e.set_pilot(P)
    h_ls = e.ls_estimate(ltf)
    hvec = np.sort(np.abs(rng.standard_normal((npkt, 100)))).astype(np.float32) * 1e-7     # like the delays h_tau
    snr_db = rng.choice([-10.0, 0.0, 10.0, 25.0], size=(npkt, nr)).astype(np.float32)
    got = e.lmmse_estimate(h_ls, hvec, snr_db)
    assert got.shape == h_ls.shape and got.dtype == np.complex64
    ref = oracle.lmmse_estimate(h_ls, hvec.astype(np.float64), snr_db.astype(np.float64))
    assert rel_rows(np.concatenate([got.real, got.imag], -1), np.concatenate([ref.real, ref.imag], -1)) < TOL
    # smoothing must actually change the estimate, and shrink it
    assert np.linalg.norm(got - h_ls) > 1e-2 * np.linalg.norm(h_ls)
    assert np.linalg.norm(got) < np.linalg.norm(h_ls)


def test_ls_empty_batch(pkg):
    e = pkg.CsiEngine(4, 2, hidden=(8,))
    e.set_pilot(np.eye(4))
    h = e.ls_estimate(np.zeros((0, 2, 1280), dtype=np.complex128))
    assert h.shape == (0, 2, 4, 234)


@pytest.mark.parametrize('seed,cases', [(5, 10), (11, 10)])
def test_fuzz_ls_cases(seed, cases):
    """tests/fuzz_ls.py inside the suite: random antenna / rx / packet counts, Hadamard or generic pilots, every LS kernel
    that can serve the shape."""
    import fuzz_ls
    rng = np.random.default_rng(seed)
    log = []
    fails = sum(fuzz_ls.run_case(rng, c, log.append) for c in range(cases))
    assert fails == 0, '\n'.join(l for l in log if l.startswith('FAIL'))


@pytest.mark.parametrize('nt,nr,npkt', FAST_PILOT_CASES)
@pytest.mark.parametrize('kind', ['vht', 'signed_perm'])
def test_ls_hadamard_equivalent_pilot_takes_the_fwht_kernel(pkg, oracle, nt, nr, npkt, kind):
    rng = np.random.default_rng(nt * 7 + len(kind))
    P = vht_pilot(oracle, nt) if kind == 'vht' else signed_perm_pilot(oracle, rng, nt)
    assert np.allclose(P @ P.T, nt * np.eye(nt)) and not np.array_equal(P, oracle.hadamard(nt))
    ltf, H = oracle.make_structured_packets(rng, npkt, nr, P, snr_db=20.0)
    e = pkg.CsiEngine(nt, nr, hidden=(64, 64))
    e.set_pilot(P)
    assert e.get_option('ls_pilot_fast') == 2 and e.get_option('ls_mode') == 5
    h = e.ls_estimate(ltf)
    ref = oracle.ls_estimate(ltf, P)
    cat = lambda z: np.concatenate([z.real, z.imag], -1)
    assert rel_rows(cat(h), cat(ref)) < TOL
    h2 = e.ls_estimate(ltf)
    assert np.array_equal(h, h2)
    # the generic kernels on the same pilot (what round 3 ran): agreement to rounding
    e.set_option('ls_fast_perm', 0)
    assert e.get_option('ls_mode') in (6, 7)
    g = e.ls_estimate(ltf)
    assert rel_rows(cat(h), cat(g)) < 1e-6
    e.set_option('ls_fast_perm', 1)
    assert e.get_option('ls_mode') == 5
    # known answer: without noise the estimate IS the channel (P P^T = nt I)
    ltf0, H0 = oracle.make_structured_packets(rng, 3, nr, P, snr_db=None)
    assert rel_rows(cat(e.ls_estimate(ltf0)), cat(H0)) < TOL
    # the Sylvester matrix itself keeps the table-free kernel
    e.set_pilot(oracle.hadamard(nt))
    assert e.get_option('ls_pilot_fast') == 1 and e.get_option('ls_mode') == 5
    ltf2, _ = oracle.make_structured_packets(rng, 3, nr, oracle.hadamard(nt), snr_db=20.0)
    assert rel_rows(cat(e.ls_estimate(ltf2)), cat(oracle.ls_estimate(ltf2, oracle.hadamard(nt)))) < TOL


def test_ls_not_every_sign_matrix_is_taken(pkg, oracle):
    """A random +-1 matrix (not Hadamard) stays on the generic kernels; a Hadamard matrix obtained from Sylvester's by switching a
    closed quadruple (negate a constant 4 x 4 block: still Hadamard, the rows no longer closed under products in the same way) is
    served by whatever kernel the decomposition's VERIFIED answer allows - and both are right."""
    rng = np.random.default_rng(5)
    nt, nr = 16, 2
    e = pkg.CsiEngine(nt, nr, hidden=(64, 64))
    cat = lambda z: np.concatenate([z.real, z.imag], -1)
    Pn = rng.choice([-1.0, 1.0], (nt, nt))
    Hs = oracle.hadamard(nt).copy()
    Hs[np.ix_([0, 4, 8, 12], [0, 1, 2, 3])] *= -1           # rows whose index has bits 0, 1 clear are constant on columns 0..3
    assert np.allclose(Hs @ Hs.T, nt * np.eye(nt))
    ltf = (rng.standard_normal((4, nr, 320 * nt)) + 1j * rng.standard_normal((4, nr, 320 * nt))).astype(np.complex64)
    for P in (Pn, Hs):
        e.set_pilot(P)
        h = e.ls_estimate(ltf)
        assert rel_rows(cat(h), cat(oracle.ls_estimate(ltf, P))) < TOL
        assert (e.get_option('ls_mode') == 5) == (e.get_option('ls_pilot_fast') in (1, 2))
    e.set_pilot(Pn)
    assert e.get_option('ls_pilot_fast') == 0 and e.get_option('ls_mode') != 5


def test_stress_ls_generic_bounded(pkg, oracle):
    """tests/stress_ls_generic.py, bounded: the bf16-split generic-P kernel (and the ring kernels) on every item, bit for bit over
    repeated runs, with two waves per SIMD - the configuration in which the first version of that kernel raced."""
    import stress_ls_generic
    bad = stress_ls_generic.run(runs=3, budget_s=30.0, quiet=True)
    assert bad == 0


def test_ls_side_stream_option_is_refused_and_the_serial_order_matches_the_oracle(pkg, oracle):
    """"ls_overlap_cus" > 0 - the LS kernel on a CU-masked side stream beside the DNN kernels (measured slower, and the one
    arrangement that put LS workgroups beside other kernels' MFMA waves) - left the library: the option is refused with text and reads 0,
    and csi_estimate_device runs the serial order, whose results are checked against the fp64 oracle."""
    rng = np.random.default_rng(31)
    nt, nr, npkt, hidden = 32, 4, 96, (256, 256)
    w_re, w_im = _weights(oracle, 55, nt, hidden)
    P = vht_pilot(oracle, nt)
    ltf = oracle.make_structured_packets(rng, npkt, nr, P, snr_db=3.0)[0].astype(np.complex64)
    e = pkg.CsiEngine(nt, nr, hidden=hidden)
    e.load_weights('real', w_re)
    e.load_weights('imag', w_im)
    e.set_pilot(P)
    d_re, d_im = e.to_device(np.ascontiguousarray(ltf.real)), e.to_device(np.ascontiguousarray(ltf.imag))
    outs = [e.empty((npkt, nr, nt, 234)) for _ in range(4)]

    def run():
        for o in outs:
            o.upload(np.zeros((npkt, nr, nt, 234), np.float32))
        e.estimate_device(d_re, d_im, npkt, *outs)
        e.synchronize()
        return [o.download().copy() for o in outs]

    with pytest.raises(pkg.CsiError) as err:
        e.set_option('ls_overlap_cus', 8)
    assert 'not part of the product build' in str(err.value) and e.get_option('ls_overlap_cus') == 0
    ref = run()                                           # ... and the serial order is what csi_estimate_device runs
    r_re, r_im = oracle.predict_packets(ltf[:2], P, w_re, w_im, np.float64, pkt_batch=2)
    assert rel_rows(ref[0][:2], r_re) < TOL and rel_rows(ref[1][:2], r_im) < TOL
