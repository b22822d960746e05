"""CPU tests of the multi-user downlink (csi_mu_precoder_device / csi_mu_link_sim_device, csrc/mu_link.hip.h): the C-ABI
surface, the fp64 restatement tests/mu_link_ref.py against known answers, the user-seed rule, the fp32 budget of the precoder that the
GPU test's bound rests on, and the sweep's --users arguments."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import link_ref as L        # noqa: E402
import mu_link_ref as MU    # noqa: E402
import train_streams as ts  # noqa: E402

NEW = ['csi_mu_precoder_device', 'csi_mu_link_sim_device']


def _planes(rng, *shape):
    return rng.standard_normal(shape + (L.N,)) + 1j * rng.standard_normal(shape + (L.N,))


def test_new_entry_points_in_header_table_and_library(pkg):
    pkg.build_library()
    lib = pkg.load_library()
    header = open(os.path.join(REPO, 'include', 'csi_mamimo.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(csi_[a-z0-9_]+)\s*\(', header))
    from dl_channel_estimation_mamimo_amd import _lib
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.csi_abi_version() == 1            # the change is additive
    blob = open(pkg.library_path(), 'rb').read()
    assert b'mu_precoder_kernel' in blob and b'mu_txrx_kernel' in blob
    for m in ('mu_precoder', 'mu_precoder_device', 'mu_link_sim', 'mu_link_sim_device'):
        assert hasattr(pkg.CsiEngine, m), m
    assert pkg.MuLinkResult._fields == ('bit_errors', 'evm_rms', 'sinr_db', 'n_info', 'g', 'xeq', 'csi', 'llr', 'bits')
    names = [lib.csi_profile_kernel_name(i).decode() for i in range(lib.csi_profile_num_kernels())]
    assert 'mu_precoder' in names and 'mu_txrx' in names


def test_null_context(pkg):
    lib = pkg.load_library()
    assert lib.csi_mu_precoder_device(None, 2, None, None, 1, 1, None, None, None) == -1
    assert lib.csi_mu_link_sim_device(None, 2, None, None, None, None, None, 0, 0, 1, 1, 1, 2, *[None] * 10) == -1


def test_user_seed_rule():
    """seed_0 = seed; seed_u = splitmix64(seed ^ splitmix64(u)), restated here on Python integers"""
    mask = (1 << 64) - 1

    def sm(x):
        x = (x + 0x9E3779B97F4A7C15) & mask
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & mask
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & mask
        return x ^ (x >> 31)

    assert int(ts.splitmix64(np.uint64(12345))) == sm(12345)
    for seed in (0, 7, 2 ** 63 + 5):
        assert MU.user_seed(seed, 0) == seed
        seeds = [MU.user_seed(seed, u) for u in range(8)]
        assert len(set(seeds)) == 8
        for u in range(1, 8):
            assert seeds[u] == sm(seed ^ sm(u))
    b0 = L.info_bits(MU.user_seed(3, 0), 5, 300)
    assert np.array_equal(b0, L.info_bits(3, 5, 300))
    assert not np.array_equal(b0, L.info_bits(MU.user_seed(3, 1), 5, 300))


@pytest.mark.parametrize('nt,nr,nu,ns,reg', [(4, 2, 2, 1, 0.0), (4, 2, 2, 2, 0.0), (8, 4, 2, 4, 0.0), (32, 4, 4, 4, 0.0), (8, 2, 4, 1, 0.3)])
def test_reference_precoder_properties(nt, nr, nu, ns, reg):
    """|W|_F^2 = Nt, equal column norms; with perfect CSI and reg = 0 the other users' columns of G vanish to rounding and G_uu is diagonal"""
    rng = np.random.default_rng(nt + nu)
    h = [_planes(rng, nr, nt) for _ in range(nu)]
    W, cond = MU.precoder(h, ns, reg)
    M = nu * ns
    assert W.shape == (M, nt, L.N) and np.isfinite(cond).all()
    col = (np.abs(W) ** 2).sum(1)                                                        # [M, 234]
    assert np.abs(col - nt / M).max() <= 1e-12 * nt
    assert np.abs((np.abs(W) ** 2).sum((0, 1)) - nt).max() <= 1e-12 * nt
    for u in range(nu):
        G = MU.effective_channel(h[u], W, ns)
        own = G[:, :, u * ns:(u + 1) * ns]
        other = np.delete(G, np.s_[u * ns:(u + 1) * ns], axis=2)
        scale = np.abs(own).max()
        if reg == 0.0:
            assert np.abs(other).max() <= 1e-9 * cond.max() ** 2 * scale
            off = own - np.einsum('kii->ki', own)[:, :, None] * np.eye(ns)
            assert np.abs(off).max() <= 1e-9 * cond.max() ** 2 * scale
            assert MU.sinr_db(G, u, ns, 0.0) > 150.0
        else:
            assert np.abs(other).max() > 1e-3 * scale                                    # regularised: interference is traded for power


def test_reference_singular_rule():
    rng = np.random.default_rng(5)
    h0 = _planes(rng, 2, 4)
    h0[0, :, :100] = np.array([1, 1j, -1, -1j])[rng.integers(0, 4, (4, 100))]           # |b|^2 = 4: the arithmetic of the pivots is exact
    h1 = h0.copy()
    h1[:, :, 100:] = _planes(rng, 2, 4)[:, :, 100:]
    W, cond = MU.precoder([h0, h1], 1, 0.0)
    assert (W[:, :, :100] == 0).all() and (np.abs(W[:, :, 100:]).sum((0, 1)) > 0).all()
    Wr, _ = MU.precoder([h0, h1], 1, 0.1)
    assert np.isfinite(Wr).all() and (np.abs(Wr).sum((0, 1)) > 0).all()
    Wz, _ = MU.precoder([np.zeros_like(h0), np.zeros_like(h0)], 1, 0.0)
    assert (Wz == 0).all()


@pytest.mark.parametrize('ns,bps', [(2, 2), (4, 4)])
def test_one_user_is_the_single_user_link(ns, bps):
    """U = 1, ns = Nr: fed the W that link_ref.simulate builds, the multi-user model has its bits, symbols, noise and y exactly, and its x"""
    nt, nr, n_sym, seed, pkt, nv = 8, ns, 2, 11, 6, 0.2
    rng = np.random.default_rng(ns)
    h = _planes(rng, nr, nt)
    fbb = rng.standard_normal((L.N, ns, nt)) + 1j * rng.standard_normal((L.N, ns, nt))
    a = L.simulate(seed, pkt, h, np.eye(nt), fbb, nv, n_sym, bps)
    W = np.ascontiguousarray(a['W'].transpose(2, 1, 0))                                   # [234, nt, ns] -> [M, nt, 234]
    b = MU.simulate(seed, pkt, [h], W, [nv], ns, n_sym, bps)[0]
    assert np.array_equal(a['bits'], b['bits']) and np.array_equal(a['d'], b['d']) and np.array_equal(a['w'], b['w'])
    assert np.abs(a['G'] - b['G']).max() <= 1e-12 * np.abs(a['G']).max()
    assert np.abs(a['x'] - b['x']).max() <= 1e-9 * a['cond'].max() ** 2
    assert np.abs(a['llr'] - b['llr']).max() <= 1e-8 * a['cond'].max() ** 2 * np.abs(a['llr']).max()
    assert b['sinr_db'] == pytest.approx(10 * np.log10((np.abs(b['G']) ** 2).sum() / (L.N * ns * nv)), abs=1e-9)


@pytest.mark.parametrize('nt,m', [(8, 4), (32, 16), (4, 4), (8, 8)])
def test_fp32_budget_of_the_precoder(nt, m):
    """The yardstick of the GPU test (a): an fp32 emulation of Gram, Cholesky, inverse, product and normalisation (numpy keeps complex64
    through matmul, cholesky and inv) over 2000 seeded items against fp64, per item |W - Wref|_F / |Wref|_F over max(1e-5, 1e-6 cond(B)^2).
    With these seeds: at most 0.036 of the bound; cond(B) up to 8.3 / 6.7 / 161 / 513 for the four shapes.  The assertion leaves the
    emulation a quarter of the bound: the device sums in another order."""
    rng = np.random.default_rng(1000 * nt + m)
    n = 2000
    B = (rng.standard_normal((n, m, nt)) + 1j * rng.standard_normal((n, m, nt))).astype(np.complex64)

    def zf(b):
        bh = np.conj(np.swapaxes(b, 1, 2))
        li = np.linalg.inv(np.linalg.cholesky(b @ bh))
        v = bh @ (np.conj(np.swapaxes(li, 1, 2)) @ li)
        return v * (np.sqrt(b.real.dtype.type(nt) / m) / np.sqrt((np.abs(v) ** 2).sum(1, keepdims=True)))

    w32, w64 = zf(B), zf(B.astype(np.complex128))
    assert w32.dtype == np.complex64
    sv = np.linalg.svd(B.astype(np.complex128), compute_uv=False)
    cond = sv[:, 0] / sv[:, -1]
    err = np.sqrt((np.abs(w32 - w64) ** 2).sum((1, 2)) / (np.abs(w64) ** 2).sum((1, 2)))
    ratio = (err / np.maximum(1e-5, 1e-6 * cond ** 2)).max()
    print('(Nt, M) = (%d, %d): cond(B) up to %.1f, fp32 error / bound at most %.4f' % (nt, m, cond.max(), ratio))
    assert ratio <= 0.25


def test_sweep_arguments_and_field_order():
    from dl_channel_estimation_mamimo_amd import sweep
    args = sweep.parse_args(['-d', 'x', '--ber', '--users', '3'])
    assert args.users == 3 and args.muReg == 'zf' and args.userSpacing == 15.0
    assert sweep.parse_args(['-d', 'x', '--ber', '--users', '2', '--muReg', 'rzf', '--userSpacing', '20']).muReg == 'rzf'
    assert sweep.parse_args(['-d', 'x']).users == 1
    for bad in (['--users', '2'], ['--ber', '--users', '9'], ['--ber', '--users', '0'], ['--ber', '--users', '2', '--muReg', 'mmse'],
                ['--ber', '--users', '4', '--nTX', '4', '--numSTS', '2'], ['--ber', '--users', '8', '--nTX', '64', '--numSTS', '4']):
        with pytest.raises(SystemExit):
            sweep.parse_args(['-d', 'x'] + bad)
    one = np.zeros(3)
    mse = {'MSE_' + e: one for e in sweep.ESTIMATORS}
    mse.update({f + x: one for x in sweep.SOURCES for f in sweep.LINK_FIELDS}, MSE_perfect=one)
    mse.update({f + x: one for x in sweep.SOURCES for f in sweep.RX_FIELDS})
    mse['MSE_' + sweep.DELAY] = one
    before = sweep.metric_fields(mse)
    assert sweep.MU_FIELDS == ('bersMU_', 'EVM_rmsMU_', 'sinrMU_')
    mse.update({f + x: one for x in sweep.SOURCES + (sweep.DELAY,) for f in sweep.MU_FIELDS})
    after = sweep.metric_fields(mse)
    assert after[:len(before)] == before                                   # the new fields are written behind every existing one
    assert after[len(before):] == [f + x for x in sweep.SOURCES + (sweep.DELAY,) for f in sweep.MU_FIELDS]
    with pytest.raises(ValueError, match='users needs the data phase'):
        sweep.run_sweep(None, '/nonexistent', users=2)
