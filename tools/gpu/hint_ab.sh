#!/bin/bash
# A/B of a global GEMM tile_hint on the bench (same box, back to back): 0 = heuristics, 32 = two LDS stages everywhere
# usage: hint_ab.sh <output dir>   (the bench lines run with --full for the GEMM roofline)
out=${1:?usage: hint_ab.sh <output dir>}; mkdir -p $out
for h in ${HINTS:-0 32 0 32}; do
  CMDA_BENCH_GEMM_HINT=$h timeout 600 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $out/bench_$h.json 2> $out/err_$h
  python -c "
import json;d=json.loads(open('$out/bench_$h.json').read().strip().splitlines()[-1]);print('hint $h', d['ms_per_step'], d['roofline']['gemm_ms_per_step'])"
done
