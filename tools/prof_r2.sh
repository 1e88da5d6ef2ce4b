# usage (on the GPU box, from the repo root): bash tools/prof_r2.sh <mode> <tag> [extra bench args]
# (outputs under $ICK_RESULTS, default results/ in the repo)
# 1) bench.py --full -> <tag>_bench_<mode>.json (with roofline.by_kernel + cpu_baseline)
# 2) the same command under rocprofv3 --kernel-trace --stats (no eager profile pass, no CPU leg)
#    -> <tag>_<mode>_kernel_stats.txt
set -e
mode=$1; tag=$2; shift 2
root=$(cd "$(dirname "$0")/.." && pwd)
res=${ICK_RESULTS:-$root/results}      # where the outputs go
mkdir -p "$res"
python3 $root/bench.py --full --mode $mode --no-modes "$@" > $res/${tag}_bench_${mode}.json 2> $res/${tag}_bench_${mode}.err || { tail -20 $res/${tag}_bench_${mode}.err; exit 1; }
cut -c1-400 $res/${tag}_bench_${mode}.json
cd /tmp && export TMPDIR=/tmp
out=$res/prof_${tag}_${mode}
rm -rf $out
steps=10; warm=3
rocprofv3 --kernel-trace --stats --output-format csv -d $out -o runc -- python3 $root/bench.py --mode $mode --steps $steps --warmup $warm --no-cpu-baseline --no-profile --no-modes --min-seconds 0 "$@" > $out.log 2>&1 || { tail -20 $out.log; exit 1; }
python3 $root/tools/profile_summary.py $out $((steps + warm)) > $res/${tag}_${mode}_kernel_stats.txt
head -24 $res/${tag}_${mode}_kernel_stats.txt | cut -c1-170
