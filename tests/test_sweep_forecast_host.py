"""The sweep with the channel forecast (--forecast P M [--forecastSteps D]), without a device: run_sweep on a subclass
of the recording engine of tests/sweep_fake.py that adds the one call the base lacks (view: a time slice of the history as a plane of
its own).  The parser's refusals, the times and seeds handed to the engine, the field names and their position in metrics.mat and
sweep.json; without the option everything is what it was."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_fake as F      # noqa: E402

AGING = dict(delay_ms=2.0, speed_mps=1.5, heading_deg=20.0)
FORECAST = dict(soundings=6, order=2, steps=3)
BER = dict(ns=1, ntrf=1, n_sym=2, bps=2)
CASES = dict(plain=dict(channel={}), mu=dict(channel=dict(az_deg=-40.0), ber=dict(BER), users=2, user_spacing=10.0))


class ViewArray(F.FakeArray):
    """slice `index` of a recorded array: named after its parent, freed with it"""

    def __init__(self, engine, parent, index):
        F.FakeArray.__init__(self, engine, parent.shape[1:])
        engine.arrays.remove(self)            # it owns nothing: not a leak when the level ends
        self.parent, self.index = parent, index


_Base = F.FakeEngine


class ForecastEngine(_Base):
    def view(self, array, index):
        return ViewArray(self, array, index)

    def _use(self, a, index=None):
        if isinstance(a, ViewArray):
            if a.parent.freed:
                self.use_after_free.append('view of ' + str(a.parent.name))
            return '%s[%d]' % (_Base._use(self, a.parent, index), a.index)
        return _Base._use(self, a, index)


@pytest.fixture(scope='module')
def runs(pkg, tmp_path_factory):
    from dl_channel_estimation_mamimo_amd import sweep
    tmp = tmp_path_factory.mktemp('forecast')
    out = {}
    try:
        F.FakeEngine = ForecastEngine         # record() builds its engine by this name
        for tag, kw in CASES.items():
            kw = dict(kw, aging=dict(AGING))
            out[tag] = (F.record(sweep, kw, str(tmp / (tag + '-off'))), F.record(sweep, dict(kw, forecast=dict(FORECAST)), str(tmp / (tag + '-on'))))
    finally:
        F.FakeEngine = _Base
    return out


@pytest.mark.parametrize('tag', list(CASES))
def test_new_fields_stand_at_the_end_and_nothing_else_moves(pkg, runs, tag):
    from dl_channel_estimation_mamimo_amd import sweep
    off, on = runs[tag]
    mu = tag == 'mu'
    assert on['clean'] == [dict(leaked=[], double_free=[], use_after_free=[])] * len(F.LEVELS), on['clean']
    new = ['MSEF_LS', 'MSEF_perfect'] + ([f + x for x in ('LS', 'perfect') for f in ('bersMUF_', 'EVM_rmsMUF_', 'sinrMUF_')] if mu else [])
    assert sweep.FAMILIES['MSEF'].sources == sweep.FAMILIES['MUF'].sources == ('LS', 'perfect')
    assert sweep.FAMILIES['MSEF'].needs == ('aging', 'forecast') and sweep.FAMILIES['MUF'].needs == ('aging', 'forecast', 'mu')
    assert sweep.FAMILIES['MUF'].users == 'muf_users'
    for order in (sweep.MAT_ORDER, sweep.JSON_ORDER):      # behind the aged families in both orders, and last
        names = [k for k, _ in order]
        assert names[-4:] == ['MSEF', 'MSEF', 'MUF', 'MUF'] and names[-6:-4] == ['MUA', 'MUA']
    for lv in range(len(F.LEVELS)):
        n_old = len(off['metrics'][lv])
        assert [k for k, _ in on['metrics'][lv][:n_old]] == [k for k, _ in off['metrics'][lv]]
        if lv == 0:                                        # the first level's values too: nothing in front of the new calls moved
            assert on['metrics'][lv][:n_old] == off['metrics'][lv]
        assert [k for k, _ in on['metrics'][lv][n_old:]] == new, (tag, lv)
        assert off['metrics'][lv][-1][0].startswith('sinrMUA_' if mu else 'MSEA_')
        keys_off, keys_on = off['per_packet_keys'][lv], on['per_packet_keys'][lv]
        assert keys_on[:len(keys_off)] == keys_off
        assert sorted(keys_on[len(keys_off):]) == sorted(new + (['muf_users'] if mu else []))
    j_off, j_on = json.loads(off['sweep_json']), json.loads(on['sweep_json'])
    assert 'forecast' not in j_off and j_on['forecast'] == dict(soundings=6, order=2, steps=3, ridge=1e-5)
    assert [k for k in j_on if k != 'forecast'] == list(j_off) and all(j_on[k] == j_off[k] for k in j_off if k != 'levels')
    assert all(j_on['levels'][0][k] == v for k, v in j_off['levels'][0].items())
    for l_off, l_on in zip(j_off['levels'], j_on['levels']):
        assert list(l_on)[:len(l_off)] == list(l_off)
        tail = list(l_on)[len(l_off):]
        assert tail == new + (['muf_users'] if mu else []), (tag, tail)
        assert sorted(l_on['MSEF_LS']) == ['ci_high', 'ci_low', 'mean']
        if mu:
            assert sorted(l_on['muf_users']) == ['LS', 'perfect'] and sorted(l_on['muf_users']['LS']) == ['EVM_rms', 'bers', 'sinr']
    assert 'MSEF_LS' in on['table'] and 'MSEF_LS' not in off['table']


@pytest.mark.parametrize('tag', list(CASES))
def test_times_seeds_and_planes_handed_to_the_engine(runs, tag):
    off, on = runs[tag]
    users = 2 if tag == 'mu' else 1
    P, M, D = FORECAST['soundings'], FORECAST['order'], FORECAST['steps']
    want_times = [-1e-3 * (P - 1 - i) * AGING['delay_ms'] / D for i in range(P - 1)]

    def levels(events):
        starts = [i for i, e in enumerate(events) if e[0] == 'synth_scattering' and e[2]['snr_db'] is not None and e[2]['seed'] == F.SEED + 1]
        return [events[a:b] for a, b in zip(starts, starts[1:] + [len(events)])]

    for lv, (a, b) in enumerate(zip(levels(off['events']), levels(on['events']))):
        assert [e[0] for e in b[:len(a)]] == [e[0] for e in a]                # every call of the level without the option, then the new ones
        head, tail = b[:len(a)], b[len(a):]      # (array names count through a whole run: the level's own head is the reference)
        first = F.N_TRAIN + lv * F.N_TEST
        sounding = [e for e in head if e[0] == 'synth_scattering']
        aged = [e for e in head if e[0] == 'scatter_channel_at_device']
        assert len(aged) == users
        hist = [e for e in tail if e[0] == 'scatter_channel_at_device']
        assert len(hist) == 2 * users                                          # per user: one history for 'LS', one for 'perfect'
        for u in range(users):
            seed = F.SEED + 1 + u
            for e in hist[2 * u:2 * u + 2]:
                assert e[1][:3] == [seed, first, F.N_TEST] and e[1][3] == pytest.approx(want_times, abs=1e-15)
                assert e[2]['az_deg'] == sounding[u][2]['az_deg'] == aged[u][2]['az_deg']
                assert (e[2]['speed_mps'], e[2]['heading_az_deg'], e[2]['carrier_hz']) == (1.5, 20.0, 28e9)
            ls_hist = hist[2 * u][1][4:6]                                      # FORECAST_SOURCES: LS first
            noise = [e for e in tail if e[0] == 'sounding_noise_device' and e[1][4].startswith(ls_hist[0] + '[')]
            assert [e[1][0] for e in noise] == [seed ^ ((i + 1) << 32) for i in range(P - 1)]
            assert all(e[1][1:3] == [first, F.N_TEST] for e in noise)
            assert [e[1][4:6] for e in noise] == [['%s[%d]' % (ls_hist[0], i), '%s[%d]' % (ls_hist[1], i)] for i in range(P - 1)]      # in place
            assert len({e[1][3] for e in noise}) == 1                          # one error variance per user: null_noise / Nt
        nn = [e for e in tail if e[0] == 'null_noise_device']
        assert len(nn) == users and [e[1][:2] for e in nn] == [s[2]['out'][:2] for s in sounding[:users]]
        fc = [e for e in tail if e[0] == 'forecast_device']
        assert len(fc) == 2 * users and len([e for e in tail if e[0] == 'sounding_noise_device']) == (P - 1) * users
        ls_plane, true_plane = [e for e in head if e[0] == 'estimate_device'][0][1][5:7], sounding[0][2]['out'][2:4]
        for k, e in enumerate(fc[:2]):                                         # user 0: P soundings, the newest the source's own plane
            x_re, x_im = e[1][0], e[1][1]
            assert len(x_re) == len(x_im) == P and e[1][2:5] == [F.N_TEST, M, D] and e[2] == dict(ridge=1e-5)
            assert [x_re[-1], x_im[-1]] == (ls_plane if k == 0 else true_plane)
            assert x_re[:-1] == ['%s[%d]' % (hist[k][1][4], i) for i in range(P - 1)]
        # the metric and the data phase read the aged planes as the truth and the forecast planes as the estimate
        nm = [e for e in tail if e[0] == 'nmse_device']
        assert [e[1][:2] for e in nm] == [aged[0][1][4:6]] * 2 and [e[1][2:4] for e in nm] == [e[1][5:7] for e in fc[:2]]
        mul = [e for e in tail if e[0] == 'mu_link_sim_device']
        pre = [e for e in tail if e[0] == 'mu_precoder_device']
        assert len(mul) == len(pre) == (2 if users == 2 else 0)
        if users == 2:
            assert all(e[1][:2] == [[t[1][4] for t in aged], [t[1][5] for t in aged]] for e in mul)
            assert pre[0][1][0] == [fc[0][1][5], fc[2][1][5]] and pre[1][1][0] == [fc[1][1][5], fc[3][1][5]]
            mua = [e for e in head if e[0] == 'mu_link_sim_device'][-1]
            assert mul[0][1][5:9] == mua[1][5:9]                               # seed, first packet, packets, streams: the bits and noise of MUA


def test_the_option_is_refused_without_its_channel_and_aging(pkg, tmp_path, capsys):
    from dl_channel_estimation_mamimo_amd import sweep
    with pytest.raises(ValueError, match='forecast needs aging'):
        sweep.run_sweep(ForecastEngine(), str(tmp_path), channel={}, forecast=dict(FORECAST))
    with pytest.raises(ValueError, match='aging needs the scattering channel'):
        sweep.run_sweep(ForecastEngine(), str(tmp_path), aging=dict(AGING), forecast=dict(FORECAST))
    for bad, text in ((dict(order=2), 'soundings and order'), (dict(soundings=17, order=2), 'soundings 17 outside 2 .. 16'),
                      (dict(soundings=8, order=9), 'order 9 outside 1 .. 8'), (dict(soundings=6, order=3, steps=4), 'at most soundings 6'),
                      (dict(soundings=6, order=2, steps=0), 'steps 0 must be at least 1'), (dict(soundings=6, order=2, ridge=-1.0), 'ridge'),
                      (dict(soundings=6, order=2, colour=1), 'unknown forecast parameters')):
        with pytest.raises(ValueError, match=text):
            sweep.run_sweep(ForecastEngine(), str(tmp_path), channel={}, aging=dict(AGING), forecast=bad)
    ok = ['-d', 'x', '--channel', 'scattering', '--aging', '2']
    for argv, text in ((['-d', 'x', '--forecast', '8', '4'], '--forecast needs --channel scattering --aging MS'),
                       (['-d', 'x', '--channel', 'scattering', '--forecast', '8', '4'], '--forecast needs --channel scattering --aging MS'),
                       (['-d', 'x', '--aging', '2', '--forecast', '8', '4'], '--aging needs --channel scattering'),
                       (ok + ['--forecast', '8', '5'], 'at most soundings 8'), (ok + ['--forecast', '17', '4'], 'soundings 17'),
                       (ok + ['--forecast', '8', '4', '--forecastSteps', '0'], 'steps 0'), (ok + ['--forecastSteps', '2'], '--forecastSteps needs --forecast')):
        with pytest.raises(SystemExit):
            sweep.parse_args(argv)
        assert text in capsys.readouterr().err, argv
    a = sweep.parse_args(ok + ['--forecast', '12', '4'])
    assert sweep.forecast_from_args(a) == dict(soundings=12, order=4, steps=4)
    assert sweep.forecast_args(sweep.forecast_from_args(a)) == dict(soundings=12, order=4, steps=4, ridge=1e-5)
    assert sweep.forecast_from_args(sweep.parse_args(ok + ['--forecast', '8', '4', '--forecastSteps', '2']))['steps'] == 2
    assert sweep.forecast_from_args(sweep.parse_args(ok)) is None and sweep.forecast_args(None) is None
    for flag in ('--forecast', '--forecastSteps'):
        assert flag in sweep.__doc__
