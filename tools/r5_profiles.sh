#!/bin/bash
# Round-5 measurement artifacts (GPU box).  Per workload: the bench line (with roofline.by_kernel + its trace keys), rocprofv3
# kernel stats of the same command, the in-step table and the PMC traffic table joined through that line -- for ALL FIVE
# workloads the default bench line reports (train cfg2, forward cfg2, greedy cfg5, beam cfg5, train cfg4), so that no `modes`
# entry carries a null frac_in_step / traffic.  Then the device-timestamp timeline of the captured train step.
#   bash tools/r5_profiles.sh <tag> [workloads: "train:cfg2 forward:cfg2 ..."]
tag=${1:-r05_a}
todo=${2:-"train:cfg2 forward:cfg2 greedy:cfg5 beam:cfg5 train:cfg4"}
root=$(cd "$(dirname "$0")/.." && pwd)
res=${ICK_RESULTS:-$root/results}      # where the outputs go
mkdir -p "$res"
cd $root
for spec in $todo; do
  mode=${spec%%:*}; cfg=${spec##*:}
  t=${tag}_${cfg}
  marker=packed_ce_rows_kernel      # once per pass, eager warm-up passes included (the optimizer kernel is not: flushes, no-op launches)
  [ $mode = forward ] && marker=caption_embed_kernel
  [ $mode = greedy ] && marker=dec_init
  [ $mode = beam ] && marker=dec_init
  timeout -k 10 400 bash tools/prof_r2.sh $mode $t --config $cfg --no-cpu-baseline > $res/${t}_${mode}.log 2>&1 || { tail -5 $res/${t}_${mode}.log; exit 1; }
  tail -2 $res/${t}_${mode}.log | cut -c1-150
  python3 tools/in_step_table.py $res/prof_${t}_${mode} $res/r05_in_step_${mode}_${cfg}.json $res/${t}_bench_${mode}.json $marker > $res/${t}_in_step_${mode}.txt 2>&1 || { tail -3 $res/${t}_in_step_${mode}.txt; exit 1; }
  timeout -k 10 500 bash tools/pmc_traffic.sh $mode $t --config $cfg > $res/${t}_pmc_${mode}.log 2>&1 || { tail -5 $res/${t}_pmc_${mode}.log; exit 1; }
  python3 tools/traffic_table.py $res/r05_traffic_${mode}_${cfg}.json $res/${t}_bench_${mode}.json $res/pmc_${t}_${mode}_FETCH_SIZE $res/pmc_${t}_${mode}_WRITE_SIZE > $res/${t}_traffic_${mode}.txt 2>&1 || { tail -3 $res/${t}_traffic_${mode}.txt; exit 1; }
  head -6 $res/${t}_traffic_${mode}.txt | cut -c1-150
  rm -rf $res/pmc_${t}_${mode}_FETCH_SIZE $res/pmc_${t}_${mode}_WRITE_SIZE      # large CSVs: the tables are what is kept
done
python3 tools/timeline.py $res/prof_${tag}_cfg2_train packed_ce_reduce > $res/${tag}_train_kernel_timeline.txt 2>&1
ICK_TIMESTAMPS=1 timeout -k 10 200 python3 tools/host_bound.py > $res/${tag}_train_device_timestamps.txt 2>&1; tail -42 $res/${tag}_train_device_timestamps.txt
