set -e
root=$(cd "$(dirname "$0")/.." && pwd)
res=${ICK_RESULTS:-$root/results}      # where the outputs go
mkdir -p "$res"
cd /tmp && export TMPDIR=/tmp
out=$res/prof_greedy_$1
rm -rf $out
rocprofv3 --kernel-trace --stats --output-format csv -d $out -o runc -- python3 $root/bench.py --full --mode greedy --steps 5 --warmup 2 --no-cpu-baseline --no-modes --min-seconds 0 > $out.log 2>&1
tail -1 $out.log | cut -c1-100
