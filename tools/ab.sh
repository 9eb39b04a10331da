#!/bin/bash
# Run ON THE GPU BOX: A/B of prebuilt libraries ab_libs/*.so on the default benchmark, interleaved, same box.
#   tools/ab.sh prev cur [rounds]
# Stops at the first run that fails: what has faulted is not started again.
set -u -o pipefail
cd $GRAFT_REPO_ROOT
R=${3:-3}
for r in $(seq 1 $R); do
  for v in $1 $2; do
    cp ab_libs/$v.so dagl_amd/csrc/libdagl_ce.so || exit 1
    python bench.py --full --steps 300 --warmup 30 --no-cpu-baseline --no-quality --no-extra 2>/dev/null | python -c "
import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$v', round(d['ms_per_step'],4), {k: round(x*1e3,1) for k,x in d['stage_ms'].items()})" || { echo "$v: run failed, stopping"; exit 1; }
  done
done
