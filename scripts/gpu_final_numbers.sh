# the round's numbers on one box: bench line, per-config table, scaling projection, first call, host boundary
# usage: bash scripts/gpu_final_numbers.sh <output directory>; then python scripts/install_final_numbers.py <tag> <that directory>
OUT="${1:?usage: bash scripts/gpu_final_numbers.sh <output directory>}"
mkdir -p "$OUT"
python bench.py --full > "$OUT/bench_line.json" 2> "$OUT/bench.err"; echo "bench rc $?"
python scripts/bench_configs.py > "$OUT/bench_configs.json" 2> "$OUT/bench_configs.err"; echo "configs rc $?"
python scripts/scaling_projection.py > "$OUT/scaling_projection.json" 2> "$OUT/scaling.err"; echo "scaling rc $?"
python scripts/first_call_breakdown.py > "$OUT/first_call.json" 2> /dev/null; echo "first call rc $?"
python scripts/host_boundary_rate.py > "$OUT/host_boundary.json" 2> /dev/null; echo "host boundary rc $?"
python bench.py --fanout --gpus 1 > "$OUT/bench_fanout_1.json" 2> /dev/null; echo "fanout rc $?"
python bench.py --gpus 2 --backend gloo --full --no-cpu-baseline > "$OUT/bench_2ranks_gloo_one_gpu.json" 2> /dev/null; echo "2 ranks rc $?"
