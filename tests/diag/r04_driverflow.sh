#!/bin/bash
# what the driver runs at round end: smoke, then the full bench line (timed), written under the directory given
cd "$(dirname "$0")/../.."
O=${1:?usage: tests/diag/r04_driverflow.sh OUTDIR}
mkdir -p "$O"
python3 __graft_entry__.py smoke 2>&1 | tail -2
SECONDS=0
python3 bench.py --full > "$O/driverflow_bench.json" 2> "$O/driverflow_bench.err"
echo "bench rc=$? wall=${SECONDS}s"
python3 - "$O/driverflow_bench.json" <<'PY'
import json, sys
d=json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1])
print(d['metric'], d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['traffic'], d['cpu_baseline']['value'])
print({k: v.get('ms_per_step') for k, v in d['extra_workloads'].items()})
PY
