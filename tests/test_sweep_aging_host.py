"""The sweep with channel aging (--aging), without a device: run_sweep on the recording engine of tests/sweep_fake.py -
whose catch-all for *_device calls already serves scatter_channel_at_device, so the engine needs no extension - with and without the
option.  The aged families' calls stand behind every other call of a level, their fields behind every other field in metrics.mat and
in sweep.json, everything that exists without the option keeps its value, and the option is refused off the scattering channel."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_fake as F      # noqa: E402

AGING = dict(delay_ms=2.0, speed_mps=1.5, heading_deg=20.0)
ALL = dict(channel={}, blind=True, delay_taps=6, delay_pre=1, beams=True, rx_estimate=True, ber=dict(ns=1, ntrf=1, n_sym=2, bps=2),
           feedback=dict(b_phi=4, b_psi=2), users=2, mu_hybrid=3, mu_jsdm=dict(b=2, r_star=2), rx_combine=True)


@pytest.fixture(scope='module')
def runs(pkg, tmp_path_factory):
    from dl_channel_estimation_mamimo_amd import sweep
    tmp = tmp_path_factory.mktemp('aging')
    out = {}
    for tag, kw in (('all', ALL), ('plain', dict(channel={})), ('ber', dict(channel=dict(az_deg=-40.0), ber=dict(ns=1, ntrf=1, n_sym=2, bps=2)))):
        out[tag] = (F.record(sweep, kw, str(tmp / (tag + '-off'))), F.record(sweep, dict(kw, aging=dict(AGING)), str(tmp / (tag + '-on'))))
    return out


def _expected_new(sweep, sources_single, sources_every, ber, mu):
    new = ['MSEA_' + x for x in sweep.FAMILIES['MSEA'].sources if x in sources_every + ('DLYANG',)]
    if ber:
        new += [f + x for x in sources_single for f in sweep.LINKA_FIELDS]
    if mu:
        new += [f + x for x in sources_every for f in sweep.MUA_FIELDS]
    return new


@pytest.mark.parametrize('tag', ['all', 'plain', 'ber'])
def test_new_fields_stand_at_the_end_and_nothing_else_moves(pkg, runs, tag):
    from dl_channel_estimation_mamimo_amd import sweep
    off, on = runs[tag]
    assert on['clean'] == [dict(leaked=[], double_free=[], use_after_free=[])] * len(F.LEVELS), on['clean']
    full = tag == 'all'
    single = tuple(x for x in sweep.SINGLE if full or x != sweep.BLIND)
    every = single + ((sweep.DELAY, sweep.BEAMS) if full else ())
    new = _expected_new(sweep, single, every if full else single, ber=tag != 'plain', mu=full)
    if not full:
        new = [k for k in new if not k.endswith('DLYANG')]
    for lv in range(len(F.LEVELS)):
        # metrics.mat: the fields without the option, with their values, then the new ones in the order of the family table.  (The
        # recording engine derives a download's numbers from the array's name and the index of the event that wrote it; both are those
        # of the run without the option throughout the first level, and shifted by the first level's tail in the second.)
        n_old = len(off['metrics'][lv])
        assert [k for k, _ in on['metrics'][lv][:n_old]] == [k for k, _ in off['metrics'][lv]]
        if lv == 0:
            assert on['metrics'][lv][:n_old] == off['metrics'][lv]
        assert [k for k, _ in on['metrics'][lv][len(off['metrics'][lv]):]] == new, (tag, lv)
        # the per-packet dict: the old keys in their order, the new ones (and the per-user record) behind them
        keys_off, keys_on = off['per_packet_keys'][lv], on['per_packet_keys'][lv]
        assert keys_on[:len(keys_off)] == keys_off
        assert sorted(keys_on[len(keys_off):]) == sorted(new + (['mua_users'] if full else []))
    # sweep.json: the option's record, and per level the old keys with their values followed by the new ones
    j_off, j_on = json.loads(off['sweep_json']), json.loads(on['sweep_json'])
    assert 'aging' not in j_off
    assert j_on['aging'] == dict(delay_ms=2.0, speed_mps=1.5, heading_deg=20.0, random_heading=False, carrier_hz=28e9)
    assert [k for k in j_on if k != 'aging'] == list(j_off) and all(j_on[k] == j_off[k] for k in j_off if k != 'levels')
    assert all(j_on['levels'][0][k] == v for k, v in j_off['levels'][0].items())
    for l_off, l_on in zip(j_off['levels'], j_on['levels']):
        assert list(l_on)[:len(l_off)] == list(l_off)
        tail = list(l_on)[len(l_off):]
        assert tail == new + (['mua_users'] if full else []), (tag, tail)      # a per-user record stands behind its family's fields
        if full:
            assert sorted(l_on['mua_users']) == sorted(every) and sorted(l_on['mua_users']['LS']) == ['EVM_rms', 'bers', 'sinr']
    assert 'MSEA_LS' in on['table'] and 'MSEA_LS' not in off['table']


@pytest.mark.parametrize('tag', ['all', 'plain', 'ber'])
def test_aged_calls_stand_behind_every_other_call_of_a_level(runs, tag):
    off, on = runs[tag]

    def levels(events):      # the events of every level: a level starts with its first synth_scattering call that makes noisy packets
        starts = [i for i, e in enumerate(events) if e[0] == 'synth_scattering' and e[2]['snr_db'] is not None
                  and e[2]['seed'] == F.SEED + 1]
        return [events[a:b] for a, b in zip(starts, starts[1:] + [len(events)])]

    def shape(e):            # an event without the names of its arrays, which count from the first appearance in the whole run
        return json.loads(__import__('re').sub(r'"a\d+\(', '"a(', json.dumps(e)))

    l_off, l_on = levels(off['events']), levels(on['events'])
    assert len(l_off) == len(l_on) == len(F.LEVELS)
    users = 2 if tag == 'all' else 1
    for lv, (a, b) in enumerate(zip(l_off, l_on)):
        assert [e[0] for e in b[:len(a)]] == [e[0] for e in a]
        if lv == 0:          # (an upload computed from downloads carries their numbers, which the first level's tail shifts in the second)
            assert [shape(e) for e in b[:len(a)]] == [shape(e) for e in a]
        tail = b[len(a):]
        kinds = [e[0] for e in tail]
        assert kinds[:users] == ['scatter_channel_at_device'] * users and 'scatter_channel_at_device' not in kinds[users:]
        sounding = [e for e in a if e[0] == 'synth_scattering']
        for u, e in enumerate(tail[:users]):      # the same stream, packets and azimuth as the user's sounding call; the motion as configured
            assert e[1][:4] == [F.SEED + 1 + u, F.N_TRAIN + lv * F.N_TEST, F.N_TEST, [2e-3]]
            assert e[2]['az_deg'] == sounding[u][2]['az_deg'] and e[2]['n_scat'] == sounding[u][2]['n_scat']
            assert (e[2]['speed_mps'], e[2]['heading_az_deg'], e[2]['carrier_hz'], e[2]['random_heading']) == (1.5, 20.0, 28e9, False)
        n_src = dict(all=8, plain=4, ber=4)[tag]
        assert kinds.count('nmse_device') == n_src
        assert kinds.count('link_sim_device') == (0 if tag == 'plain' else (5 if tag == 'all' else 4))
        assert kinds.count('mu_link_sim_device') == (7 if tag == 'all' else 0) and 'link_sim_rx_device' not in kinds
        # the aged planes are what the data phases and the metric read as the truth
        aged0 = tail[0][1][4:6]
        assert all(e[1][:2] == aged0 for e in tail if e[0] in ('nmse_device', 'link_sim_device'))
        if tag == 'all':
            aged = [[t[1][4] for t in tail[:2]], [t[1][5] for t in tail[:2]]]
            assert all(e[1][:2] == aged for e in tail if e[0] == 'mu_link_sim_device')


def test_aging_is_refused_off_the_scattering_channel(pkg, tmp_path, capsys):
    from dl_channel_estimation_mamimo_amd import sweep
    with pytest.raises(ValueError, match='aging needs the scattering channel'):
        sweep.run_sweep(F.FakeEngine(), str(tmp_path), aging=dict(delay_ms=1.0))
    for bad, text in ((dict(), 'delay_ms'), (dict(delay_ms=1.0, speed_mps=-1.0), 'speed_mps'), (dict(delay_ms=1.0, carrier_hz=0.0), 'carrier_hz'),
                      (dict(delay_ms=1.0, colour=3), 'unknown aging parameters')):
        with pytest.raises(ValueError, match=text):
            sweep.run_sweep(F.FakeEngine(), str(tmp_path), channel={}, aging=bad)
    with pytest.raises(SystemExit):
        sweep.parse_args(['-d', 'x', '--aging', '2'])
    assert '--aging needs --channel scattering' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        sweep.parse_args(['-d', 'x', '--channel', 'scattering', '--aging', '2', '--speed', '-3'])
    assert 'speed_mps' in capsys.readouterr().err
    a = sweep.parse_args(['-d', 'x', '--channel', 'scattering', '--aging', '2.5', '--speed', '3', '--heading', '-45', '--randomHeading', '--carrier', '6e9'])
    assert sweep.aging_from_args(a) == dict(delay_ms=2.5, speed_mps=3.0, heading_deg=-45.0, random_heading=True, carrier_hz=6e9)
    assert sweep.aging_args(dict(delay_ms=2)) == dict(delay_ms=2.0, speed_mps=1.0, heading_deg=0.0, random_heading=False, carrier_hz=28e9)
    assert sweep.aging_from_args(sweep.parse_args(['-d', 'x', '--channel', 'scattering'])) is None and sweep.aging_args(None) is None
    for flag in ('--aging', '--speed', '--heading', '--randomHeading', '--carrier'):
        assert flag in sweep.__doc__
