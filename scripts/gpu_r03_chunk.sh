set -o pipefail
OUT=gpurun_out/r03h; mkdir -p $OUT
pick='import json,sys; d=json.loads(sys.stdin.read()); r=d["roofline"]; print(sys.argv[1], "value %.0f" % d["value"], "ms/set %.4f" % r["pipeline"]["ms_per_launch_set"], "chunk", d["config"]["blocks_per_launch"], "exclusive", {k: round(v,3) for k,v in r["exclusive_launch_ms"].items()}, "parity", d.get("parity_rel_err_vs_oracle"))'
for wl in plugin_2ch_65536tap_L1024_fp64_f32frames plugin_2ch_65536tap_L1024_fp32 cfg5_2ch_262144tap_L4096_fp64 cfg2_2ch_65536tap_L8192_fp32; do
for c in 4096 8192 16384 32768; do
  timeout -k 10 300 python bench.py --full --workload $wl --chunk $c --blocks 65536 --steps 4 --warmup 1 --no-cpu-timing --no-extras 2>$OUT/err.log | python -c "$pick" ${wl}_c$c | tee -a $OUT/chunk.txt
done; done
