#!/usr/bin/env python
"""record_sweep_plan.py SWEEP.py [--dump ID] - run a sweep module on the recording engine of tests/sweep_fake.py, no device needed.

Without --dump: every combination of sweep_fake.combinations() goes through run_sweep and the fixture is rewritten:
tests/golden/sweep_plan.json, a SHA-256 per combination, and tests/golden/sweep_plan_full.json.gz, the whole record of
sweep_fake.FULL_RECORDS (0.4 MB of JSON as text).  The fixture states what the sweep did BEFORE a change, so
SWEEP.py is the file of the commit the change starts from, never the changed one:

    git show <parent>:dl-channel-estimation-mamimo_amd/sweep.py > /tmp/sweep_parent.py
    python tools/record_sweep_plan.py /tmp/sweep_parent.py

With --dump ID: print the record of one combination as indented JSON, to diff two versions of the module
(tests/test_sweep_plan_host.py names the ID when a digest differs)."""
import argparse
import gzip
import importlib.util
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
import sweep_fake      # noqa: E402


def load_sweep(path):
    """The file `path` as one more submodule of the package, so that its relative imports resolve."""
    import dl_channel_estimation_mamimo_amd as pkg
    name = pkg.__name__ + '._recorded_sweep'
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('sweep', help='the sweep.py to record')
    p.add_argument('--dump', metavar='ID', help='print the record of this combination instead of writing the fixture')
    args = p.parse_args(argv)
    sweep, combos = load_sweep(args.sweep), sweep_fake.combinations()
    with tempfile.TemporaryDirectory() as tmp:
        if args.dump:
            print(json.dumps(sweep_fake.record(sweep, combos[args.dump], tmp), indent=1))
            return 0
        records = {k: sweep_fake.record(sweep, kw, os.path.join(tmp, k)) for k, kw in combos.items()}
    dirty = {k: r['clean'] for k, r in records.items() if any(v for lv in r['clean'] for v in lv.values())}
    if dirty:
        raise SystemExit('leaks / double frees / uses after free, nothing written: %r' % dirty)
    path = os.path.join(REPO, 'tests', 'golden', 'sweep_plan.json')
    with open(path, 'w') as f:
        json.dump({k: sweep_fake.digest(r) for k, r in records.items()}, f, indent=0)
        f.write('\n')
    full = json.dumps({k: records[k] for k in sweep_fake.FULL_RECORDS}, separators=(',', ':')).encode()
    with open(path[:-5] + '_full.json.gz', 'wb') as raw, gzip.GzipFile(fileobj=raw, mode='wb', filename='', mtime=0) as f:      # the same bytes every time
        f.write(full)
    print('%d combinations, %d events in %s, %d + %d bytes -> %s, %s' % (len(records), len(records[sweep_fake.ALL_ON]['events']), sweep_fake.ALL_ON,
                                                                       os.path.getsize(path), os.path.getsize(raw.name), path, raw.name))
    return 0


if __name__ == '__main__':
    sys.exit(main())
