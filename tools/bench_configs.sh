# bench lines of the non-headline configs (one GPU), then their rocprofv3
# kernel stats (no CPU baseline under the profiler); results under $OUT
# (default bench_out/ in the repository root)
R=$PWD
OUT=${OUT:-$R/bench_out}
mkdir -p $OUT
for c in "$@"; do
  timeout -k 10 600 python3 -u bench.py --full --config $c --steps 2 --warmup 1 > $OUT/bench_$c.json 2> $OUT/bench_$c.err || exit $?
done
cd /tmp && export TMPDIR=/tmp
for c in "$@"; do
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$c -o run -- python3 -u $R/bench.py --full --config $c --steps 1 --warmup 1 --no-cpu-baseline > $OUT/bench_${c}_under_rocprof.json 2>> $OUT/bench_$c.err || exit $?
done
