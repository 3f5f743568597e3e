# `python bench.py $FLAGS` N times in a row on one box: the scalars of every line (run-to-run spread).
#   bash tools/bench_repeats.sh [N] [FLAGS]      FLAGS default: --full; "" = the default run (headline only, ~15 s each)
# SVO_LIB_PATH=<another build of the library> gives the same for that build (A/B on one box, back to back).
N=${1:-5}
FLAGS=${2---full}
for i in $(seq 1 $N); do python bench.py $FLAGS 2>/dev/null | tail -1 | python -c "
import json,sys
d=json.loads(sys.stdin.read())
keep=('value','ms_per_step','frontend','multi_sequence','sharded','semantic_elas','elas','msa','host_feed','host_feed_pageable','frontend_host_feed','with_null_stream_cotenant','with_pooled_stream_cotenant','two_contexts_one_gpu','frame_period_us')
o={k:d.get(k) for k in keep}; r=d.get('roofline') or {}; o['roofline_frac']=r.get('frac'); o['kernel_seconds_per_launch']=r.get('kernel_seconds_per_launch'); o['cpu_baseline']=(d.get('cpu_baseline') or {}).get('value'); o['checks_all_true']=all(v is True or v==0 for v in (d.get('checks') or {}).values())
print(json.dumps(o))"; done
