# Frames in flight x bounce grid sweep of the C5 headline (bench.py --full --no-cpu-baseline --no-extras).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R && mkdir -p bench_out
for cfg in ${CFGS:-"3 2048" "4 2048" "3 1536" "4 1536" "3 1024" "4 1024" "3 2048"}; do
  set -- $cfg
  RTBVH_BOUNCE_BLOCKS=$2 timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-extras --inflight $1 --steps 30 > bench_out/sw_$1_$2.json 2> bench_out/sw_$1_$2.err || { echo "BENCH $cfg FAILED"; tail -20 bench_out/sw_$1_$2.err; exit 1; }
  python3 -c "import json;d=json.load(open('bench_out/sw_$1_$2.json'));print('inflight $1 blocks $2', 'value', d['value'], 'ms', d['ms_per_step'], 'lat', d['traversal']['one_frame_latency_ms'], 'ident', d['traversal']['inflight_frame_identical'])"
done
