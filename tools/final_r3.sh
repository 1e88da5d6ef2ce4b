#!/bin/bash
# round-end validation: full GPU suite, smoke, default bench (artifact of the round)
set -o pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
res=${ICK_RESULTS:-$root/results}      # where the outputs go
mkdir -p "$res"
cd $root
mkdir -p $res/final
timeout -k 10 1000 python -m pytest tests -m gpu -x -q > $res/final/pytest_gpu.log 2>&1; rc=$?
tail -3 $res/final/pytest_gpu.log
[ $rc -eq 0 ] || exit $rc
python -c "import __graft_entry__ as g; g.smoke()" > $res/final/smoke.log 2>&1 && tail -2 $res/final/smoke.log &&
python bench.py --full > $res/final/bench_default.json 2> $res/final/bench_default.err && cut -c1-600 $res/final/bench_default.json
