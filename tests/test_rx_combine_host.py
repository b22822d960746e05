"""CPU tests of receive combining (csi_rx_combiner_device, csi_rx_apply_combiner_device, csrc/rx_combine.hip.h): the
C-ABI surface, the fp64 statement tests/rx_combine_ref.py against its defining properties and against the feedback report and the
multi-user data phase it has to fit (tests/feedback_ref.py, tests/mu_link_ref.py), the sweep's --rxCombine argument, and the sweep with
the option on, on the recording engine of tests/sweep_fake.py."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feedback_ref as R           # noqa: E402
import rx_combine_ref as C         # noqa: E402
import sweep_fake as F             # noqa: E402

N = R.N
SHAPES = [(8, 2, 1, 2), (8, 4, 2, 2)]          # (Nt, Nr, ns, U)


def test_entry_points_in_header_table_and_library(pkg):
    pkg.build_library()
    lib = pkg.load_library()
    header = open(os.path.join(REPO, 'include', 'csi_mamimo.h')).read()
    assert 'would colour the noise' in header
    listed = header.split('Device pointers (')[1].split(')')[0]
    assert 'csi_rx_combiner_device' in listed and 'csi_rx_apply_combiner_device' in listed
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(csi_[a-z0-9_]+)\s*\(', header))
    from dl_channel_estimation_mamimo_amd import _lib
    for name, nargs in (('csi_rx_combiner_device', 8), ('csi_rx_apply_combiner_device', 9)):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
        assert len(_lib.SYMBOLS[name][1]) == nargs                                         # the prototype of the header, argument by argument
        proto = re.search(r'\b%s\s*\(([^;]*)\);' % name, header).group(1)
        assert len(proto.split(',')) == nargs
    assert lib.csi_abi_version() == 1            # the change is additive
    blob = open(pkg.library_path(), 'rb').read()
    for k in (b'rx_combiner_kernel', b'rx_apply_kernel'):
        assert k in blob, k
    for m in ('rx_combiner', 'rx_combiner_device', 'rx_apply_combiner', 'rx_apply_combiner_device'):
        assert hasattr(pkg.CsiEngine, m), m
    names = [lib.csi_profile_kernel_name(i).decode() for i in range(lib.csi_profile_num_kernels())]
    assert 'rx_combiner' in names and 'rx_combine' in names
    assert lib.csi_rx_combiner_device(None, None, None, 1, 1, None, None, None) == -1          # a null context
    assert lib.csi_rx_apply_combiner_device(None, None, None, None, None, 1, 1, None, None) == -1


@pytest.mark.parametrize('nt,nr,ns,nu', SHAPES)
def test_the_combiner_diagonalises_and_is_the_report(nt, nr, ns, nu):
    H = C.items(R.planes(40 + nt + nr, 1, nr, nt)).astype(np.complex128)
    Cm, s = C.combiner(H, ns)
    Ch = np.conj(Cm.transpose(0, 2, 1))
    assert np.abs(Cm @ Ch - np.eye(ns)).max() <= 1e-12
    gram = Cm @ H @ np.conj(H.transpose(0, 2, 1)) @ Ch
    diag = np.einsum('nss->ns', gram).real
    assert np.abs(gram - diag[:, :, None] * np.eye(ns)).max() <= 1e-12 * diag.max()
    assert np.abs(diag - s ** 2).max() <= 1e-12 * diag.max() and (np.diff(s, axis=1) <= 0).all()
    E = C.apply(Cm, H)
    assert (E[:, ns:] == 0).all()
    last = E[:, :ns, -1]
    assert np.abs(last.imag).max() <= 1e-12 and (last.real >= 0).all()
    # C H is the feedback's rebuilt S V^H at continuous angles: decompose the report's vectors, expand them again, scale
    V, sv = R.svd_vectors(H, ns)
    phi, psi, _ = R.decompose(R.column_phases(V))
    svh = sv[:, :, None] * np.conj(R.expand_angles(phi, psi, nt, ns)).transpose(0, 2, 1)
    assert np.abs(E[:, :ns] - svh).max() <= 1e-12 * sv.max()


def test_the_rank_rule():
    H = np.zeros((3, 4, 8), np.complex128)
    H[1, :] = np.arange(1, 9) + 1j                    # four equal rows: rank 1
    H[2, :3] = np.arange(1, 9)
    H[2, 3] = np.arange(8, 0, -1) * 1j                # three equal rows and one more: rank 2
    Cm, s = C.combiner(H, 3)
    assert np.isfinite(Cm).all() and np.isfinite(s).all()
    assert not Cm[0].any() and not s[0].any()
    assert Cm[1, 0].any() and not Cm[1, 1:].any() and s[1, 0] > 0 and not s[1, 1:].any()
    assert Cm[2, 0].any() and Cm[2, 1].any() and not Cm[2, 2].any() and (s[2, :2] > 0).all() and s[2, 2] == 0


@pytest.mark.parametrize('nt,nr,ns,nu', SHAPES)
def test_combining_removes_the_leakage_of_the_feedback_arrangement(nt, nr, ns, nu):
    """The experiment of DESIGN.md 4.25: i.i.d. channels, two users, perfect CSI, zero forcing, noise_var 0.01, one packet"""
    hs = [R.planes(70 + 10 * nt + nr + u, 1, nr, nt)[0] for u in range(nu)]
    got = C.arrangements(hs, ns, 0.01)
    print({k: ('%.2f dB' % v[0], '%.3g' % v[1]) for k, v in got.items()})
    assert got['MUC'][1] < 1e-24
    assert got['MUFB'][1] > 1e-3                              # the mismatch: per cent of the signal power
    assert got['MUC'][0] > got['MUFB'][0] + 10.0
    assert got['MUC'][0] > got['MU'][0]                       # the combining gain


def test_sweep_arguments():
    from dl_channel_estimation_mamimo_amd import sweep
    assert sweep.parse_args(['-d', 'x', '--ber', '--feedback', '9', '7', '--rxCombine']).rxCombine
    assert sweep.parse_args(['-d', 'x', '--ber', '--users', '2', '--rxCombine']).rxCombine
    assert not sweep.parse_args(['-d', 'x', '--ber', '--users', '2']).rxCombine
    for bad in (['--rxCombine', '--feedback', '9', '7'], ['--rxCombine', '--users', '2'],          # without --ber
                ['--ber', '--rxCombine'],                                                          # neither --feedback nor --users
                ['--ber', '--users', '2', '--rxCombine', '--numSTS', '3', '--nRX', '2'],
                ['--ber', '--users', '2', '--rxCombine', '--numSTS', '5', '--nRX', '8']):
        with pytest.raises(SystemExit):
            sweep.parse_args(['-d', 'x'] + bad)
    assert sweep.combine_problem(2, 4) is None and 'outside' in sweep.combine_problem(3, 2)
    with pytest.raises(ValueError, match='rx_combine needs the data phase'):
        sweep.run_sweep(None, '/nonexistent', rx_combine=True)
    assert sweep.FBC_FIELDS == ('bersFBC_', 'EVM_rmsFBC_', 'sinrFBC_') and sweep.MUC_FIELDS == ('bersMUC_', 'EVM_rmsMUC_', 'sinrMUC_')
    assert sweep.MUFBC_FIELDS == ('bersMUFBC_', 'EVM_rmsMUFBC_', 'sinrMUFBC_')
    assert list(sweep.FAMILIES)[-3:] == ['FBC', 'MUC', 'MUFBC']


def test_sweep_on_the_recording_engine(tmp_path):
    """All options on, with and without rx_combine: the combined families' calls stand behind every other call of a level, in the order
    FBC, MUC, MUFBC; their fields behind every other field; nothing leaked; everything else as without the option."""
    import json
    from dl_channel_estimation_mamimo_amd import sweep
    base = F.combinations()[F.ALL_ON]
    off = F.record(sweep, dict(base), str(tmp_path / 'off'))
    on = F.record(sweep, dict(base, rx_combine=True), str(tmp_path / 'on'))
    assert all(lv == dict(leaked=[], double_free=[], use_after_free=[]) for lv in on['clean']), on['clean']
    # the old part of the run: the same events at the same places, the same fields with the same values
    ev_off, ev_on = off['events'], on['events']
    synth_at = lambda ev: [i for i, e in enumerate(ev) if e[0].startswith('synth_') and e[2].get('snr_db') is not None      # noqa: E731
                           and e[2]['seed'] == F.SEED + 1]
    starts_off, starts_on = synth_at(ev_off) + [len(ev_off)], synth_at(ev_on) + [len(ev_on)]
    assert len(starts_off) == len(starts_on) == len(F.LEVELS) + 1
    assert ev_on[:starts_on[0]] == ev_off[:starts_off[0]]
    for lv in range(len(F.LEVELS)):
        a, b = ev_off[starts_off[lv]:starts_off[lv + 1]], ev_on[starts_on[lv]:starts_on[lv + 1]]
        names = lambda ev: [e[0] for e in ev]                                    # noqa: E731
        assert names(b[:len(a)]) == names(a)
        assert not any(e[0].startswith('rx_') for e in b[:len(a)])
        tail = [e[0] for e in b[len(a):] if e[0].endswith('_device') and e[0] != 'to_device']
        # FBC per source: compress, expand (the W of FB), combiner, apply on the true planes, data phase
        fbc = ['feedback_compress_device', 'feedback_expand_device', 'rx_combiner_device', 'rx_apply_combiner_device', 'mu_link_sim_device']
        single = [x for x in sweep.SINGLE]
        assert tail[:len(fbc) * len(single)] == fbc * len(single)
        rest = tail[len(fbc) * len(single):]
        # MUC per source: per user combiner + apply on the true planes, per user apply on the estimate, precoder, data phase
        muc = ['rx_combiner_device', 'rx_apply_combiner_device'] * 2 + ['rx_apply_combiner_device'] * 2 + ['mu_precoder_device', 'mu_link_sim_device']
        every = [x for x in sweep.EVERY]
        assert rest[:len(muc) * len(every)] == muc * len(every)
        # MUFBC per source: the same channel, the reports of both users, precoder, data phase
        mufbc = (['rx_combiner_device', 'rx_apply_combiner_device'] * 2 + ['feedback_compress_device', 'feedback_expand_device'] * 2
                 + ['mu_precoder_device', 'mu_link_sim_device'])
        assert rest[len(muc) * len(every):] == mufbc * len(every)
    # (the recording engine derives a download's numbers from the array's name and the index of the event that wrote it; both are those of
    # the run without the option throughout the first level, and shifted by the first level's tail in the second)
    assert on['metrics'][0][:len(off['metrics'][0])] == off['metrics'][0]        # names, order and values of every old field
    for m_off, m_on in zip(off['metrics'], on['metrics']):
        assert [k for k, _ in m_on[:len(m_off)]] == [k for k, _ in m_off]
        new = [k for k, _ in m_on[len(m_off):]]
        assert new == ([f + x for x in sweep.SINGLE for f in sweep.FBC_FIELDS] + [f + x for x in sweep.EVERY for f in sweep.MUC_FIELDS]
                       + [f + x for x in sweep.EVERY for f in sweep.MUFBC_FIELDS])
    j_off, j_on = json.loads(off['sweep_json']), json.loads(on['sweep_json'])
    assert 'rx_combine' not in j_off and j_on['rx_combine'] is True
    assert [k for k in j_on if k != 'rx_combine'] == list(j_off)
    assert all(j_on['levels'][0][k] == v for k, v in j_off['levels'][0].items())
    for l_off, l_on in zip(j_off['levels'], j_on['levels']):
        keys = list(l_on)
        assert keys[:len(l_off)] == list(l_off)
        assert 'muc_users' in keys and 'mufbc_users' in keys and 'sinrMUFBC_perfect' in keys and 'sinrFBC_LS' in keys
    for k_off, k_on in zip(off['per_packet_keys'], on['per_packet_keys']):
        assert k_on[:len(k_off)] == k_off
    # off: no key of evaluate_level's, no field, no call
    assert not any(e[0].startswith('rx_') for e in ev_off)
