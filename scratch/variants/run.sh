#!/bin/bash
# A/B of library variants: bench headline (+ optional args) for each scratch/variants/lib_*.so and the shipped library
ERR=$(mktemp); echo "stderr of the variant runs: $ERR"
P='import json,sys; d=json.loads(sys.stdin.readline()); print(round(d["value"]), d["ms_per_step"], {k: v["avg_ms"] for k, v in d["roofline"]["kernels"].items()})'
for f in scratch/variants/lib_*.so; do
  echo "== $f"; RR_LIB=$PWD/$f python bench.py --full --steps 60 --warmup 10 --no-cpu-baseline --no-secondary "$@" 2>"$ERR" | python -c "$P"
done
echo "== shipped"; python bench.py --full --steps 60 --warmup 10 --no-cpu-baseline --no-secondary "$@" 2>/dev/null | python -c "$P"
