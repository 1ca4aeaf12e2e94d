OUT=$(realpath -m "${1:?usage: bash tools/run_profiles_r3_rest.sh OUTDIR}")
export TMPDIR=/tmp && cd "$(dirname "$0")/.."
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace -d $OUT/c3 -o c -- python3 bench.py --workload c3 --records 2000 --steps 1 --warmup 1 --full --no-cpu-baseline > $OUT/c3.json 2> $OUT/c3.err
echo c3 done rc=$?
python tools/rocpd_stats.py $(find $OUT/c3 -name "*.db" | tail -1) --csv $OUT/c3_kernel_stats.csv > $OUT/c3_kstats.txt
timeout -k 10 120 python3 tools/exp_hull_phases.py 2>&1 | tail -5 > $OUT/hull_phases.txt
timeout -k 10 120 python3 tools/exp_brent_stamps.py 1000 2>&1 | tail -14 > $OUT/brent_stamps.txt
echo stamps done
timeout -k 10 300 bash tools/run_fitprof.sh
echo fitprof done
find $OUT -name "*.db" -size +20M -delete
