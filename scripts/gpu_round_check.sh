# usage: bash scripts/gpu_round_check.sh <output directory>
set -x
OUT="${1:?usage: bash scripts/gpu_round_check.sh <output directory>}"
mkdir -p "$OUT"
python -m pytest tests -m gpu -x -q > "$OUT/pytest.log" 2>&1; echo "pytest rc $?" >> "$OUT/pytest.log"
tail -5 "$OUT/pytest.log"
python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"; echo "bench rc $?"
AB_VARIANTS=0 AB_ROUNDS=3 python scripts/ab_tuning.py > "$OUT/ab_sphere100k.log" 2>&1
AB_VARIANTS=0 AB_ROUNDS=3 AB_SCENE=random python scripts/ab_tuning.py > "$OUT/ab_random100k.log" 2>&1
AB_VARIANTS=0 AB_ROUNDS=3 AB_TRIS=1000000 AB_SIZE=4096 AB_SPP=4 python scripts/ab_tuning.py > "$OUT/ab_sphere1m.log" 2>&1
tail -2 "$OUT"/ab_*.log
