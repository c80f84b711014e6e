#!/bin/bash
# copy a round's evidence from $OUT (scratch, default: evidence/; tools/gpu_round.sh) into profiles/ (tracked) and refresh the
# summaries: bash tools/collect.sh r05
T=${1:-r06}
O=${OUT:-evidence}
set -e
python tools/summarize_prof.py $O/prof_${T} profiles/${T}_rocprof.md f16 > /dev/null
cp "$(ls -t $O/prof_${T}/trace/runc/*_kernel_stats.csv | head -1)" profiles/${T}_kernel_stats.csv      # ($O accumulates: the newest run's)
cp "$(ls -t $O/prof_${T}/trace1/runc/*_kernel_stats.csv | head -1)" profiles/${T}_kernel_stats_1stream.csv
cp $O/${T}_sweep_mc.jsonl profiles/
TAG=$T O=$O python - <<'PY'
import json, os
T, O = os.environ['TAG'], os.environ['O']
for f in (f'{T}_bench', f'{T}_bench_cfg3_share'):
    j = json.loads([l for l in open(f'{O}/{f}.json') if l.startswith('{')][-1])
    json.dump(j, open(f'profiles/{f}.json', 'w'), indent=1)
    print(f, round(j['value']), round(j['ms_per_step'], 3), (j.get('roofline') or {}).get('frac'), (j.get('roofline') or {}).get('traffic'))
PY
grep "Dominant" profiles/${T}_rocprof.md
