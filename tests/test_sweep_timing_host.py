"""The sweep with the symbol timing (--timing SPAN [--timingRho RHO]), without a device: run_sweep on the recording
engine of tests/sweep_fake.py (its *_device calls are recorded by name).  The parser's refusals, the starts, seeds and planes handed to
embed, extract, correct and the estimators with and without --cfo, the field names and their position in metrics.mat and sweep.json;
without the option everything is what it was."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_fake as F      # noqa: E402

TIMING = dict(span=64, rho=0.5)
CFO = dict(max_eps=0.05, cp_skip=16)
BER = dict(ns=1, ntrf=1, n_sym=2, bps=2)
AGED = dict(channel=dict(az_deg=-40.0), ber=dict(BER), users=2, aging=dict(delay_ms=2.0))
CASES = dict(taps=dict(), taps_cfo=dict(cfo=dict(CFO)), scattering_aged=dict(AGED), scattering_aged_cfo=dict(AGED, cfo=dict(CFO)),
             combined=dict(ber=dict(BER), users=2, rx_combine=True))
NEW = [f + x for f in ('MSET_', 'MSETC_') for x in ('LS', 'MMSE', 'DNN')]
BEHIND = ('FBC', 'MUC', 'MUFBC', 'MSEO', 'MSEOC', 'MSEA', 'LINKA', 'MUA', 'MSEF', 'MUF')      # the families the new fields stand in front of


@pytest.fixture(scope='module')
def runs(pkg, tmp_path_factory):
    from dl_channel_estimation_mamimo_amd import sweep
    tmp = tmp_path_factory.mktemp('timing')
    return {tag: (F.record(sweep, dict(kw), str(tmp / (tag + '-off'))), F.record(sweep, dict(kw, timing=dict(TIMING)), str(tmp / (tag + '-on'))))
            for tag, kw in CASES.items()}


def test_family_table(pkg):
    from dl_channel_estimation_mamimo_amd import sweep
    assert list(sweep.FAMILIES)[-7:-5] == ['MSET', 'MSETC'] and sweep.TIMING == ('MSET', 'MSETC')
    for k in sweep.TIMING:
        assert sweep.FAMILIES[k].sources == sweep.ESTIMATORS and sweep.FAMILIES[k].needs == ('timing',) and sweep.FAMILIES[k].users is None
        assert sweep.FAMILIES[k].fields == sweep.FAMILIES[k].json == (k + '_',)
    for order in (sweep.MAT_ORDER, sweep.JSON_ORDER):      # whole, in front of the receive-combining families
        names = [k for k, _ in order]
        i = names.index('MSET')
        assert names[i - 1] == 'MUFB' and names[i:i + 5] == ['MSET', 'MSET', 'MSETC', 'MSETC', 'FBC']
        assert names.count('MSET') == names.count('MSETC') == 2


@pytest.mark.parametrize('tag', list(CASES))
def test_new_fields_and_nothing_else_moves(pkg, runs, tag):
    from dl_channel_estimation_mamimo_amd import sweep
    off, on = runs[tag]
    behind = tuple(f for k in BEHIND for f in sweep.FAMILIES[k].fields)
    assert on['clean'] == [dict(leaked=[], double_free=[], use_after_free=[])] * len(F.LEVELS), on['clean']
    for lv in range(len(F.LEVELS)):
        old = [k for k, _ in off['metrics'][lv]]
        got = [k for k, _ in on['metrics'][lv]]
        cut = min([i for i, k in enumerate(old) if k.startswith(behind)] + [len(old)])
        assert got == old[:cut] + NEW + old[cut:], (tag, lv)
        if lv == 0 and 'ber' in CASES[tag]:                # the first level's values too: nothing in front of the new calls moved (without
            assert on['metrics'][lv][:cut] == off['metrics'][lv][:cut]      # ber the level newly asks for its noise deviation)
        keys_off, keys_on = off['per_packet_keys'][lv], on['per_packet_keys'][lv]
        assert [k for k in keys_on if k in keys_off] == keys_off
        assert sorted(k for k in keys_on if k not in keys_off) == sorted(NEW + ['timing_err', 'timing_quality'])
    j_off, j_on = json.loads(off['sweep_json']), json.loads(on['sweep_json'])
    assert 'timing' not in j_off and j_on['timing'] == dict(span=64, rho=0.5)
    assert [k for k in j_on if k != 'timing'] == list(j_off) and all(j_on[k] == j_off[k] for k in j_off if k != 'levels')
    for l_off, l_on in zip(j_off['levels'], j_on['levels']):
        assert [k for k in l_on if k in l_off] == list(l_off)
        assert [k for k in l_on if k not in l_off] == NEW + ['timing_exact', 'timing_rmse', 'timing_quality']
        assert list(l_on)[-3:] == ['timing_exact', 'timing_rmse', 'timing_quality']
        follower = [k for k in l_off if k.startswith(behind) or k in ('cfo_rmse', 'cfo_quality')]
        if follower:
            assert list(l_on).index('MSETC_DNN') + 1 == list(l_on).index(follower[0])
        assert sorted(l_on['MSET_LS']) == ['ci_high', 'ci_low', 'mean']
        assert 0.0 <= l_on['timing_exact'] <= 1.0 and isinstance(l_on['timing_rmse'], float) and isinstance(l_on['timing_quality'], float)
    assert 'MSET_LS' in on['table'] and 'MSETC_LS' in on['table'] and 'MSET_LS' not in off['table']
    assert not [e for e in off['events'] if e[0].startswith('sync_')]


@pytest.mark.parametrize('tag', list(CASES))
def test_starts_seeds_and_planes_handed_to_the_engine(pkg, runs, tag):
    from dl_channel_estimation_mamimo_amd import synth
    off, on = runs[tag]
    with_cfo = 'cfo' in CASES[tag]
    synth_name = 'synth_scattering' if 'channel' in CASES[tag] else 'synth_structured'

    def levels(events):
        starts = [i for i, e in enumerate(events) if e[0] == synth_name and e[2]['snr_db'] is not None and e[2]['seed'] == F.SEED + 1]
        return [events[a:b] for a, b in zip(starts, starts[1:] + [len(events)])]

    for lv, (a, b) in enumerate(zip(levels(off['events']), levels(on['events']))):
        first = F.N_TRAIN + lv * F.N_TEST
        theta = synth.timing_offsets(F.SEED + 1, first, F.N_TEST, TIMING['span'])
        up = F._host(theta.view(np.float32))                                            # int32 words
        i0 = [i for i, e in enumerate(b) if e[0] == 'to_device' and e[2] == up][0]      # the starts go up first
        cor = [e for e in b if e[0] == 'sync_correct_device'][0]
        i1 = max(i for i, e in enumerate(b) if e[0] == 'download' and e[1] == cor[2]['d_quality']) + 1
        head, new, tail = b[:i0], b[i0:i1], b[i1:]
        assert [e[0] for e in head + tail] == [e[0] for e in a]          # every call of the level without the option, in its order
        assert [e[0] for e in tail[:1]] == (['scatter_channel_at_device'] if 'aging' in CASES[tag] else [])      # in front of the aged block
        assert ('cfo_correct_device' in [e[0] for e in head]) == with_cfo and 'cfo_correct_device' not in [e[0] for e in tail]      # behind the CFO block
        sounding = [e for e in head if e[0] == synth_name][0][2]['out']
        ltf, truth, noise_std = sounding[:2], sounding[2:4], sounding[4]
        assert noise_std is not None
        assert [e[0] for e in new if e[0] not in ('nmse_device', 'download')] == (
            ['to_device', 'to_device', 'to_device'] + (['to_device', 'cfo_rotate_device'] if with_cfo else []) +
            ['sync_embed_device', 'sync_extract_device', 'estimate_device', 'lmmse_estimate_device', 'sync_correct_device', 'estimate_device',
             'lmmse_estimate_device'])
        ups = [e for e in new if e[0] == 'to_device']
        assert ups[1][2] == F._host(np.full(F.N_TEST, TIMING['span'] // 2, np.int32).view(np.float32))
        assert new[2] == ['download', noise_std] and new[3] is ups[2]                    # the margins: the level's own noise deviation
        emb = [e for e in new if e[0] == 'sync_embed_device'][0]
        ext = [e for e in new if e[0] == 'sync_extract_device'][0]
        source = ltf
        if with_cfo:
            eps = synth.cfo_offsets(F.SEED + 1, first, F.N_TEST, CFO['max_eps'])
            assert ups[3][2] == F._host(eps.view(np.float32).reshape(F.N_TEST, 2))      # the offsets of the CFO block
            rot = [e for e in new if e[0] == 'cfo_rotate_device'][0]
            assert rot[1][:3] == ltf + [F.N_TEST] and rot[1][3] == ups[3][1] and rot[1][4] == 1.0
            source = rot[1][5:7]
        assert emb[1][:5] == [F.SEED + 1, first, F.N_TEST, TIMING['span'], ups[0][1]] and emb[1][5:7] == source
        assert emb[2] == dict(d_margin_std=ups[2][1])
        cap = emb[1][7:9]
        assert ext[1][:4] == cap + [F.N_TEST, TIMING['span']] and ext[1][4] == ups[1][1] and ext[2] == {}      # the fixed start, no offset removed
        cut_planes, fixed_planes = ext[1][5:7], cor[1][4:6]
        assert cor[1][:4] == cap + [F.N_TEST, TIMING['span']]
        assert cor[2]['rho'] == 0.5 and cor[2]['remove_cfo'] is with_cfo and sorted(cor[2]) == ['d_quality', 'd_theta', 'remove_cfo', 'rho']
        assert len(set(ltf + source + cap + cut_planes + fixed_planes)) == (10 if with_cfo else 8)      # planes of their own
        est = [e for e in new if e[0] == 'estimate_device']
        assert [e[1][:3] for e in est] == [cut_planes + [F.N_TEST], fixed_planes + [F.N_TEST]]
        lm_old = [e for e in head if e[0] == 'lmmse_estimate_device'][0]
        lm = [e for e in new if e[0] == 'lmmse_estimate_device']
        assert all(e[1][3:6] == lm_old[1][3:6] for e in lm)                                           # the level's own LMMSE inputs
        assert [e[1][:2] for e in lm] == [e[1][5:7] for e in est]                                     # on the LS planes of the same call
        nm = [e for e in new if e[0] == 'nmse_device']
        assert len(nm) == 6 and all(e[1][:2] == truth for e in nm)                                    # against the unchanged true planes
        for k, e in enumerate(est):                                                                   # LS, MMSE, DNN
            assert [n[1][2:4] for n in nm[3 * k:3 * k + 3]] == [e[1][5:7], lm[k][1][6:8], e[1][3:5]]
        assert new[-2] == ['download', cor[2]['d_theta']] and new[-1] == ['download', cor[2]['d_quality']]


def test_refusals_and_flags(pkg, tmp_path, capsys):
    from dl_channel_estimation_mamimo_amd import sweep
    for bad, text in ((dict(rho=0.5), 'span None is no multiple'), (dict(span=0), 'span 0 is no multiple of 4 in 4 .. 256'),
                      (dict(span=6), 'span 6 is no multiple'), (dict(span=260), 'span 260 is no multiple'), (dict(span=320), 'span 320 is no multiple'),
                      (dict(span=64.5), 'span 64.5 is no multiple'), (dict(span=64, rho=1.5), 'rho 1.5 outside \\[0, 1\\]'),
                      (dict(span=64, rho=-0.1), 'rho -0.1 outside'), (dict(span=64, rho=float('nan')), 'rho nan outside'),
                      (dict(span=64, colour=1), 'unknown timing parameters')):
        with pytest.raises(ValueError, match=text):
            sweep.run_sweep(F.FakeEngine(), str(tmp_path), timing=bad)
    for argv, text in ((['-d', 'x', '--timingRho', '0.5'], '--timingRho needs --timing'), (['-d', 'x', '--timing', '0'], 'span 0 is no multiple of 4 in 4 .. 256'),
                       (['-d', 'x', '--timing', '62'], 'span 62 is no multiple'), (['-d', 'x', '--timing', '320'], 'span 320 is no multiple'),
                       (['-d', 'x', '--timing', '-4'], 'span -4 is no multiple'), (['-d', 'x', '--timing', '64', '--timingRho', '2'], 'rho 2.0 outside [0, 1]')):
        with pytest.raises(SystemExit):
            sweep.parse_args(argv)
        assert text in capsys.readouterr().err, argv
    a = sweep.parse_args(['-d', 'x', '--timing', '64'])
    assert sweep.timing_from_args(a) == dict(span=64, rho=1.0) and sweep.timing_args(sweep.timing_from_args(a)) == dict(span=64, rho=1.0)
    b = sweep.parse_args(['-d', 'x', '--channel', 'scattering', '--cfo', '0.01', '--timing', '256', '--timingRho', '0'])
    assert sweep.timing_from_args(b) == dict(span=256, rho=0.0) and sweep.cfo_from_args(b) == dict(max_eps=0.01, cp_skip=0)
    assert sweep.timing_from_args(sweep.parse_args(['-d', 'x', '--timing', '4'])) == dict(span=4, rho=1.0)
    assert sweep.timing_from_args(sweep.parse_args(['-d', 'x'])) is None and sweep.timing_args(None) is None
    for flag in ('--timing', '--timingRho'):
        assert flag in sweep.__doc__
