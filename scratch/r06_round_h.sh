#!/bin/bash
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
timeout -k 10 1000 python -m pytest tests -m gpu -x -q > $OUT/r06_gputests.log 2>&1; tail -8 $OUT/r06_gputests.log
timeout -k 10 500 python bench.py --full > "$OUT/r06_bench_32x4.json" 2> "$OUT/r06_bench_32x4.err"; tail -c 600 "$OUT/r06_bench_32x4.json"
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
