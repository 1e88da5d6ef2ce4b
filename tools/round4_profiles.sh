#!/bin/bash
# Round-4 measurement artifacts (GPU box): per mode bench JSON + rocprofv3 kernel stats, the in-step table of the train and
# forward steps, PMC traffic tables, device-timestamp timeline of the captured train step.   bash tools/round4_profiles.sh <tag>
tag=${1:-r04_x}
root=$(cd "$(dirname "$0")/.." && pwd)
res=${ICK_RESULTS:-$root/results}      # where the outputs go
mkdir -p "$res"
cd $root
for spec in "train" "forward" "greedy --config cfg5" "beam --config cfg5" "train --config cfg4"; do
  set -- $spec
  mode=$1; shift
  t=$tag; [ "$1" = "--config" ] && [ "$2" = "cfg4" ] && t=${tag}_cfg4
  timeout -k 10 400 bash tools/prof_r2.sh $mode $t "$@" > $res/${t}_${mode}.log 2>&1 || { tail -5 $res/${t}_${mode}.log; exit 1; }
  tail -2 $res/${t}_${mode}.log | cut -c1-150
done
python3 tools/in_step_table.py $res/prof_${tag}_train 13 $res/${tag}_in_step_train.json > $res/${tag}_in_step_train.txt 2>&1 || tail -3 $res/${tag}_in_step_train.txt
python3 tools/in_step_table.py $res/prof_${tag}_forward 13 $res/${tag}_in_step_forward.json > $res/${tag}_in_step_forward.txt 2>&1 || tail -3 $res/${tag}_in_step_forward.txt
python3 tools/timeline.py $res/prof_${tag}_train > $res/${tag}_train_kernel_timeline.txt 2>&1
for mode in train forward greedy; do
  timeout -k 10 500 bash tools/pmc_traffic.sh $mode $tag > $res/${tag}_pmc_${mode}.log 2>&1 || { tail -5 $res/${tag}_pmc_${mode}.log; }
done
python3 tools/traffic_table.py $res/${tag}_traffic.json $res/pmc_${tag}_train_FETCH_SIZE $res/pmc_${tag}_train_WRITE_SIZE $res/pmc_${tag}_greedy_FETCH_SIZE $res/pmc_${tag}_greedy_WRITE_SIZE > $res/${tag}_traffic.txt 2>&1; tail -20 $res/${tag}_traffic.txt | cut -c1-160
ICK_TIMESTAMPS=1 timeout -k 10 200 python3 tools/host_bound.py > $res/${tag}_train_device_timestamps.txt 2>&1; tail -45 $res/${tag}_train_device_timestamps.txt
