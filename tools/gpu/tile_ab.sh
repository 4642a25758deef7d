#!/bin/bash
# usage: tile_ab.sh <output dir>   -- GEMM tile sweep, two bench lines with the GEMM roofline (--full), the GEMM / DACS tests
out=${1:?usage: tile_ab.sh <output dir>}; mkdir -p $out
timeout 600 python tools/gemm_sweep.py > $out/sweep.txt 2> $out/err; grep " 1 1 1 " $out/sweep.txt | cut -c1-60
for i in 1 2; do
timeout 600 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $out/bench_$i.json 2> $out/err_$i
python -c "
import json;d=json.loads(open('$out/bench_$i.json').read().strip().splitlines()[-1]);print('run $i', d['ms_per_step'], d['roofline']['gemm_ms_per_step'])"
done
timeout 900 python -m pytest tests/test_gemm.py tests/test_dacs.py -x -q -m gpu > $out/tests.log 2>&1; tail -2 $out/tests.log
