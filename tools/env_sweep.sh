#!/bin/bash
# Secondary bench lines ($SEC) under each value of the environment variable $VAR in $VALS: one line per value.
set -e
cd "$(dirname "$0")/.."; export TMPDIR=/tmp; T=${TAG:-sweep}; OUT=${OUT:-bench_out}; mkdir -p $OUT/$T
for v in $VALS; do
  env $VAR=$v YM_SECONDARY="$SEC" timeout -k 10 200 python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/$T/b_$v.json 2> $OUT/$T/b_$v.err || { tail -5 $OUT/$T/b_$v.err; exit 1; }
  python3 -c "
import json; l=[json.loads(x) for x in open('$OUT/$T/b_$v.json') if x.startswith('{')][-1]
print('$VAR=$v', ' '.join(f'{k}={v.get(\"ms_per_step\", v)}' for k,v in l['secondary'].items()))"
done
