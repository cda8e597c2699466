set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
mkdir -p bench_out
timeout -k 10 900 python -m pytest tests -m gpu -x -q -p no:cacheprovider > bench_out/gpu_tests.log 2>&1 || { echo "TESTS FAILED"; tail -5 bench_out/gpu_tests.log; exit 1; }
tail -2 bench_out/gpu_tests.log
timeout -k 10 600 python bench.py --full > bench_out/bench.json 2> bench_out/bench.err || { echo "BENCH FAILED"; tail -20 bench_out/bench.err; exit 1; }
cat bench_out/bench.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $R/bench_out/prof_kt -o run --output-format csv -- python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-extras > $R/bench_out/prof_kt.log 2>&1 || { echo "PROF FAILED"; tail -20 $R/bench_out/prof_kt.log; exit 1; }
echo done
