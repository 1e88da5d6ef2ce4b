#!/bin/bash
# round-end artifacts: bench JSON + rocprofv3 kernel stats of every mode (tools/prof_r2.sh), default bench line
# usage (GPU box): bash tools/final_profiles.sh <tag>
tag=${1:-r03_i}
root=$(cd "$(dirname "$0")/.." && pwd)
res=${ICK_RESULTS:-$root/results}      # where the outputs go
mkdir -p "$res"
cd $root
for spec in "train" "forward" "greedy --config cfg5" "beam --config cfg5" "train --config cfg4"; do
  set -- $spec
  mode=$1; shift
  t=$tag; [ "$1" = "--config" ] && [ "$2" = "cfg4" ] && t=${tag}_cfg4
  timeout -k 10 400 bash tools/prof_r2.sh $mode $t "$@" > $res/${t}_${mode}.log 2>&1 || { tail -5 $res/${t}_${mode}.log; exit 1; }
  tail -3 $res/${t}_${mode}.log | cut -c1-150
done
timeout -k 10 400 python bench.py --full > $res/${tag}_bench_default.json 2> $res/${tag}_bench_default.err && cut -c1-300 $res/${tag}_bench_default.json
