# Round-4 profiles (run on the GPU box through gpurun; every bench.py run under the profiler with --no-cpu-baseline: the
# baseline's worker processes would start under the profiler's preloaded tool too).  Summaries are copied to profiles/r4_*.
OUT=$(realpath -m "${1:?usage: bash tools/run_profiles_r4.sh OUTDIR}")
export TMPDIR=/tmp && cd "$(dirname "$0")/.."
mkdir -p $OUT
# 1. kernel trace of the default bench (workload c3 at N = 1), one warm-up + one timed step
rocprofv3 --kernel-trace -d $OUT/c3 -o c -- python3 bench.py --no-cpu-baseline --no-secondary --steps 1 --warmup 1 > $OUT/c3.json 2> $OUT/c3.err
python tools/rocpd_stats.py $(find $OUT/c3 -name "*.db" | tail -1) --csv $OUT/c3_kernel_stats.csv > $OUT/c3_kstats.txt
# 2. one pipeline's share of it (2500 records, one stream: launch durations are not inflated by concurrent launches)
rocprofv3 --kernel-trace -d $OUT/b1 -o b -- python3 tools/trace_batch.py 2500 > $OUT/b1.log 2>&1
python tools/rocpd_stats.py $(find $OUT/b1 -name "*.db" | tail -1) --csv $OUT/b1_kernel_stats.csv > $OUT/b1_kstats.txt
# 3. the single-record latency path (bench --workload c1)
rocprofv3 --kernel-trace -d $OUT/c1 -o s -- python3 bench.py --workload c1 --full --no-cpu-baseline --no-batched --no-eval-many > $OUT/c1.json 2> $OUT/c1.err
python tools/rocpd_stats.py $(find $OUT/c1 -name "*.db" | tail -1) --csv $OUT/c1_kernel_stats.csv --step 2 > $OUT/c1_kernel_trace.txt
# 4. configs[4] order (N = 1152), 8 records
rocprofv3 --kernel-trace -d $OUT/c5 -o k -- python3 tools/perf_c5.py 8 > $OUT/c5.log 2>&1
python tools/rocpd_stats.py $(find $OUT/c5 -name "*.db" | tail -1) --csv $OUT/c5_kernel_stats.csv > $OUT/c5_kstats.txt
find $OUT -name "*.db" -delete
# 5. stamped build: where k_brent_warm spends its cycles (1000 records)
python3 tools/exp_brent_stamps.py 1000 2>&1 | tail -14 > $OUT/brent_stamps.txt
# (K3 and K3p are the kernels of round 3, bit for bit: their PMC passes are profiles/r3_cold_solve_pmc.json)
