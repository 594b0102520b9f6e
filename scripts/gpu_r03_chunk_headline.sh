set -o pipefail
OUT=${1:?usage: $0 OUT_DIR}/r03aw; mkdir -p $OUT
pick='import json,sys; d=json.loads(sys.stdin.read()); r=d["roofline"]; print(sys.argv[1], "value %.0f" % d["value"], "ms/set %.3f" % r["pipeline"]["ms_per_launch_set"], "chunk", d["config"]["blocks_per_launch"])'
for c in 4096 2048 8192 4096 3072 6144; do
  timeout -k 10 300 python bench.py --full --chunk $c --steps 6 --warmup 2 --no-cpu-baseline --no-extras --no-exclusive-pass 2>/dev/null | python -c "$pick" chunk$c | tee -a $OUT/chunk.txt
done
