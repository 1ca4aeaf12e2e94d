# (every bench.py run under the profiler with --no-cpu-baseline: the baseline's worker processes start under the profiler's
# preloaded tool too, and a run hung there once)
# Round-3 profiles: kernel traces of the bench step and of workload c3, PMC passes (HBM bytes) of the resident-basis evaluation.
OUT=$(realpath -m "${1:?usage: bash tools/run_profiles_r3.sh OUTDIR}")
export TMPDIR=/tmp && cd "$(dirname "$0")/.."
mkdir -p $OUT
rocprofv3 --kernel-trace -d $OUT/bench -o b -- python3 bench.py --full --no-cpu-baseline --no-batched > $OUT/bench.json 2> $OUT/bench.err
python tools/rocpd_stats.py $(find $OUT/bench -name "*.db" | tail -1) --csv $OUT/bench_kernel_stats.csv --step 2 > $OUT/bench_kernel_trace.txt
rocprofv3 --kernel-trace -d $OUT/c3 -o c -- python3 bench.py --workload c3 --records 2000 --steps 1 --warmup 1 --full --no-cpu-baseline > $OUT/c3.json 2> $OUT/c3.err
python tools/rocpd_stats.py $(find $OUT/c3 -name "*.db" | tail -1) --csv $OUT/c3_kernel_stats.csv > $OUT/c3_kstats.txt
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_f -o f -- python3 tools/perf_eval_resident.py > $OUT/pmc_f.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_w -o w -- python3 tools/perf_eval_resident.py > $OUT/pmc_w.log 2>&1
for f in $(find $OUT/pmc_f $OUT/pmc_w -name "*counter_collection.csv"); do python tools/pmc_sum.py $f k_eval_resident; done > $OUT/pmc_resident.txt
python3 tools/exp_hull_phases.py 2>&1 | tail -5 > $OUT/hull_phases.txt
python3 tools/exp_brent_stamps.py 1000 2>&1 | tail -14 > $OUT/brent_stamps.txt
rm -rf $OUT/bench/*/*.db $OUT/c3/*/*.db 2>/dev/null; find $OUT -name "*.db" -size +20M -delete
