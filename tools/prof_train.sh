set -e
root=$(cd "$(dirname "$0")/.." && pwd)
res=${ICK_RESULTS:-$root/results}      # where the outputs go
mkdir -p "$res"
python -m pytest tests -x -q -m gpu > $res/gpu_tests.log 2>&1 || { tail -30 $res/gpu_tests.log; exit 1; }
tail -2 $res/gpu_tests.log
cd /tmp && export TMPDIR=/tmp
rm -rf $res/prof_train2
rocprofv3 --kernel-trace --stats --output-format csv -d $res/prof_train2 -o runc -- python3 $root/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-modes --min-seconds 0 > $res/prof_train2.log 2>&1
tail -1 $res/prof_train2.log | cut -c1-200
