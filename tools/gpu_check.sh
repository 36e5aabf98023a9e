#!/bin/bash
# Runs on the GPU box: parity tests, smoke, bench (both configs, --full), rocprofv3 kernel trace of the headline.
# Everything lands in $OUT (default: check_out/); what is judged is copied into profiles/ afterwards (in the build container).
set -u
OUT=${OUT:-check_out}
mkdir -p $OUT
export TMPDIR=/tmp
rocminfo 2>/dev/null | grep -E "Marketing Name|gfx9|Compute Unit" | head -6 > $OUT/rocminfo.txt
echo "== pytest -m gpu" ; timeout 2400 python -m pytest tests -x -q -m gpu 2>&1 | tail -15 | tee $OUT/pytest_gpu.log
echo "== smoke" ; timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -5 | tee $OUT/smoke.log
echo "== bench" ; timeout 900 python bench.py --full "$@" 2> $OUT/bench.err | tee $OUT/bench.json ; tail -5 $OUT/bench.err
echo "== bench array512 (forced dist, one rank)" ; BENCH_FORCE_DIST=1 timeout 900 python bench.py --full --config array512 --steps 20 --warmup 3 2> $OUT/bench_array512.err | tee $OUT/bench_array512.json ; tail -5 $OUT/bench_array512.err
echo "== rocprofv3 kernel trace"
rm -rf $OUT/prof && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python3 bench.py --full --steps 512 --warmup 64 --headline-only > $OUT/bench_prof.json 2> $OUT/prof.err
find $OUT/prof -name "*kernel_stats*.csv" | head -2 | while read f; do echo "-- $f"; head -12 "$f" | cut -c1-300; done
