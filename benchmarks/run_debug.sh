cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout 900 python -m pytest tests -m gpu -x -q 2>&1 | tail -5 > "$OUT/r03_gputests.log"
timeout 1500 python bench.py --full --others-scale 0.25 > "$OUT/r03_bench_debug.log" 2>&1
tail -c 6000 "$OUT/r03_bench_debug.log"; cat "$OUT/r03_gputests.log"
