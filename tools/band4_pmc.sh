#!/bin/bash
# Split-f16 band kernel of fp32 contexts (csi_band4, headline shape Nt = 32, Nr = 4, 4000 packets): variants of band4_kernel_gen.py through the
# library's code-object hook under rocprofv3 COUNTER passes (no tracing beside them) - time per launch, shader clock (GRBM_GUI_ACTIVE, a pass of its
# own), matrix-pipe utilisation, share of the wave cycles spent in waits (any / on an instruction / on LDS), LDS instructions per launch.
# Sibling of tools/bf16_band_pmc.sh.  Needs tools/band8.hsaco (tools/build_band8.sh).
#   usage: [OUT=dir] tools/band4_pmc.sh [variant ...]  -> stdout; raw files under $OUT (default build/band4pmc)       (default variants: csi_band4_oldwaits csi_band4)
cd "$(dirname "$0")/.."
R=$(pwd)
export CSI_DEBUG_HOOKS=1 CSI_BAND8_HSACO=tools/band8.hsaco
cd /tmp && export TMPDIR=/tmp && cd $R
CTR="${CTR:-SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT}"
BENCH="python bench.py --steps 3 --warmup 2 --check 0 --no-cpu-baseline --no-latency --no-other-configs --no-regimes --host-path 0 --no-next-rows --full-line --option band4=0"
for v in ${@:-csi_band4_oldwaits csi_band4}; do
  D=${OUT:-build/band4pmc}/$v
  rm -rf $D; mkdir -p $D/sq $D/clk
  # (the hook puts the named kernel in the place of the 8-wave staged form, which "band4" = 0 selects: a name csi_band4* makes it a 256-thread launch on tiled weights)
  CSI_BAND8_NAME=$v timeout -k 10 300 rocprofv3 --pmc $CTR --output-format csv -d $D/sq -o pmc -- $BENCH > $D/bench.json 2> $D/err.txt || { echo "$v: counter pass failed ($?)"; tail -5 $D/err.txt; exit 1; }
  CSI_BAND8_NAME=$v timeout -k 10 300 rocprofv3 --pmc GRBM_GUI_ACTIVE --output-format csv -d $D/clk -o pmc -- $BENCH > $D/bench_clk.json 2> $D/err_clk.txt || { echo "$v: clock pass failed ($?)"; tail -5 $D/err_clk.txt; exit 1; }
  python - $v $D <<'PY'
import csv, sys, collections, glob, json
v, d = sys.argv[1], sys.argv[2]


def load(sub):
    f = glob.glob(d + '/' + sub + '/**/pmc_counter_collection.csv', recursive=True)
    agg, dur, seen, names = collections.defaultdict(list), [], set(), set()
    for r in csv.DictReader(open(f[0])) if f else ():
        if 'csi_band' not in r['Kernel_Name'] or 'skeleton' in r['Kernel_Name']:
            continue
        names.add(r['Kernel_Name'])
        agg[r['Counter_Name']].append(float(r['Counter_Value']))
        if r['Dispatch_Id'] not in seen:
            seen.add(r['Dispatch_Id']); dur.append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))
    return agg, sum(dur) / max(len(dur), 1) / 1e3, names


sq, us, names = load('sq')
clk, us_clk, _ = load('clk')
if not sq:
    print(v, 'no counter file;', open(d + '/err.txt').read()[-300:]); sys.exit(1)
m = lambda a, k: sum(a[k]) / max(len(a[k]), 1)
try:
    ev = json.loads(open(d + '/bench.json').read().strip().splitlines()[-1])['roofline']['avg_launch_ms']
except Exception:
    ev = float('nan')
wc = max(m(sq, 'SQ_WAVE_CYCLES'), 1)
bz = m(sq, 'SQ_BUSY_CYCLES') / 32.0
print('%-28s kernel %s: %8.1f us per launch under counters (events, no counters: n/a under rocprofv3; bench line %.3f ms)' % (v, '/'.join(sorted(names)), us, ev))
# (GRBM_GUI_ACTIVE comes back summed over the part's 8 XCDs)
print('    clock %.3f GHz (GRBM_GUI_ACTIVE %.0f summed over 8 XCDs, %.1f us)   busy cycles per SE %.0f' % (m(clk, 'GRBM_GUI_ACTIVE') / 8.0 / max(us_clk, 1e-9) / 1e3, m(clk, 'GRBM_GUI_ACTIVE'), us_clk, bz))
print('    mfma busy / busy %.3f   wait_any / wave cycles %.3f   wait_inst_any %.3f   wait_inst_lds %.3f   lds instructions %.0f   bank conflict cycles %.0f' % (
    (m(sq, 'SQ_VALU_MFMA_BUSY_CYCLES') / 1024.0) / max(bz, 1), m(sq, 'SQ_WAIT_ANY') / wc, m(sq, 'SQ_WAIT_INST_ANY') / wc, m(sq, 'SQ_WAIT_INST_LDS') / wc,
    m(sq, 'SQ_INSTS_LDS'), m(sq, 'SQ_LDS_BANK_CONFLICT')))
print('    raw: ' + '  '.join('%s=%.4g' % (k, m(sq, k)) for k in sorted(sq)))
PY
  rm -rf $D/sq/*/ $D/clk/*/ 2>/dev/null
done
