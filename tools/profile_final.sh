cd "$(dirname "$0")/.." && export TMPDIR=/tmp
res=${BENCH_RESULTS:-bench_results}
mkdir -p $res
bash tools/profile_round.sh r03
python tools/step_sequence.py $res/prof_r03/bench_kernel_trace.csv 40 > $res/r03_step_sequence.txt 2>&1; tail -3 $res/r03_step_sequence.txt
for R in 230 20; do
  for c in FETCH_SIZE WRITE_SIZE; do
    rocprofv3 --pmc $c --output-format csv -d $res/pmc_shbm${R}_$c -o pmc -- python bench.py --workload S-hbm --shbm-relations $R --steps 2 --warmup 1 --trace-steps 0 > $res/pmc_shbm${R}_$c.log 2>&1
  done
  f=$(find $res/pmc_shbm${R}_FETCH_SIZE -name '*counter_collection.csv' | head -1)
  w=$(find $res/pmc_shbm${R}_WRITE_SIZE -name '*counter_collection.csv' | head -1)
  python tools/pmc_summary.py $f $w $res/pmc_traffic_shbm_$R.json > $res/pmc_shbm_$R.txt 2>&1
  head -8 $res/pmc_shbm_$R.txt
  rm -rf $res/pmc_shbm${R}_FETCH_SIZE $res/pmc_shbm${R}_WRITE_SIZE
done
