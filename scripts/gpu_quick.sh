# tests + bench (no profiler); outputs under bench_out/
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
mkdir -p bench_out
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 120 --timeout-method thread > bench_out/gpu_tests.log 2>&1 || { echo "TESTS FAILED"; tail -30 bench_out/gpu_tests.log; exit 1; }
tail -2 bench_out/gpu_tests.log
timeout -k 10 600 python bench.py --full ${BENCH_ARGS:-} > bench_out/bench.json 2> bench_out/bench.err || { echo "BENCH FAILED"; tail -20 bench_out/bench.err; exit 1; }
cat bench_out/bench.json
