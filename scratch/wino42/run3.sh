#!/bin/bash
O=${1:?usage: run3.sh OUTPUT_DIR}
mkdir -p $O
timeout -k 10 900 python -m pytest tests -x -q -m gpu > $O/gputests.log 2>&1
echo "tests rc=$?"; tail -3 $O/gputests.log
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $O/bench.json 2> $O/bench.err
echo "bench rc=$?"; O=$O python - <<'P'
import json, os
l = [x for x in open(os.path.join(os.environ['O'], 'bench.json')) if x.startswith('{')]
d = json.loads(l[-1]); print(d['value'], d['ms_per_step'], d['roofline']['frac'], d.get('roofline', {}).get('step'))
P
