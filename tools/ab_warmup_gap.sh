#!/bin/bash
# The driver's command (--steps 20 --warmup 5) with the warm-up steps straight before the timed region (build v68) / with the run's checks and the clock probe between
# them (up to v67).  Same box, alternating; every line: the timed region and the two identical regions after it, the clock readings around them.
OUT=${OUT:-bench_out}; mkdir -p "$OUT"      # where the runs' lines and logs go
for rep in 1 2 3 4; do
for mode in new gap; do
  fl=""; [ $mode = gap ] && fl="--gap-before-timed"
  python bench.py --full --no-cpu-baseline --parity-frames 0 --stream-input 0 --no-extra-passes --steps 20 --warmup 5 $fl > $OUT/wg_${mode}_$rep.json 2> $OUT/wg_${mode}_$rep.err
  python - <<PY
import json
try:
    d = json.load(open("$OUT/wg_${mode}_$rep.json"))
    print("$mode", $rep, [round(x, 3) for x in d["repeats_ms_per_step"]], [round(x) for x in d["clock_mhz"]])
except Exception as e:
    print("$mode failed", e)
PY
done; done
