"""The orchestration of the sweep as a whole, without a device: run_sweep on the recording engine of tests/sweep_fake.py for the full
valid option matrix (336 runs at ns = 1) and two all-on runs, against tests/golden/sweep_plan.json and sweep_plan_full.json.gz - recorded by
tools/record_sweep_plan.py from the sweep.py of the commit before the family table.  A record holds the device calls, uploads,
downloads and syncs with their arguments in order, sweep.json as text, the fields of every metrics.mat in file order with their
values, the printed table, the key order of the per-packet dicts, and what every evaluate_level left unfreed, freed twice or used
after its free (nothing).  The fixture keeps a SHA-256 per run and three records whole."""
import gzip
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_fake      # noqa: E402

COMBINATIONS = sweep_fake.combinations()


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'sweep_plan.json')) as f, gzip.open(os.path.join(golden_dir, 'sweep_plan_full.json.gz'), 'rt') as g:
        return dict(digests=json.load(f), full=json.load(g))


def test_the_matrix_is_the_one_recorded(golden):
    assert len(COMBINATIONS) == 336 + 2 and list(golden['digests']) == list(COMBINATIONS)
    assert set(golden['full']) == set(sweep_fake.FULL_RECORDS)
    kinds = {e[0] for e in golden['full'][sweep_fake.ALL_ON]['events']}
    assert {'to_device', 'download', 'synchronize', 'synth_scattering', 'mu_jsdm_precoder_device', 'feedback_expand_device', 'beam_set_basis'} <= kinds


def test_download_values():
    """float32 in [1, 5), the same for the same name and last call, positive as int32 and finite as float64"""
    import numpy as np
    e = sweep_fake.FakeEngine()
    a, b = e.empty((3, 2, 2)), e.empty((3, 2, 2))
    e.some_kernel_device(a, 7, d_out=b)
    x, y = a.download(), b.download()
    assert x.dtype == np.float32 and x.shape == (3, 2, 2) and x.min() >= 1.0 and x.max() < 5.0 and not np.array_equal(x, y)
    assert np.array_equal(x, a.download()) and (x.view(np.int32) > 0).all() and np.isfinite(x.view(np.float64)).all()
    e.some_kernel_device(a, 7, d_out=b)
    assert not np.array_equal(x, a.download())
    assert e.events[0] == ['some_kernel_device', ['a0(3, 2, 2)', 7], {'d_out': 'a1(3, 2, 2)'}] and e.events[1] == ['download', 'a0(3, 2, 2)']
    a.free(), a.free(), e.other_device(a)
    assert e.end_of_level() == dict(leaked=['a1(3, 2, 2)'], double_free=['a0(3, 2, 2)'], use_after_free=['a0(3, 2, 2)'])


@pytest.mark.parametrize('combo', list(COMBINATIONS))
def test_run_sweep_does_what_it_did(pkg, golden, tmp_path, combo):
    from dl_channel_estimation_mamimo_amd import sweep
    rec = sweep_fake.record(sweep, COMBINATIONS[combo], str(tmp_path))
    assert rec['clean'] == [dict(leaked=[], double_free=[], use_after_free=[])] * len(sweep_fake.LEVELS), (combo, rec['clean'])
    want = golden['full'].get(combo)
    if want is not None:                       # the whole record: a difference shows where
        for part in ('events', 'sweep_json', 'metrics', 'table', 'per_packet_keys'):
            assert rec[part] == want[part], (combo, part)
    assert sweep_fake.digest(rec) == golden['digests'][combo], (
        '%s: the sweep no longer does what the recorded one did.  To see where, dump both records and diff them: '
        'git show <recorded commit>:dl-channel-estimation-mamimo_amd/sweep.py > old_sweep.py; python tools/record_sweep_plan.py old_sweep.py --dump %s > old.json; '
        'python tools/record_sweep_plan.py dl-channel-estimation-mamimo_amd/sweep.py --dump %s > new.json; diff old.json new.json' % (combo, combo, combo))
