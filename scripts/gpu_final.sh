#!/bin/bash
# GPU-box round record: parity tests, smoke, bench with the CPU baseline, kernel trace, PMC traffic,
# configs 3 and 5, and a 2-rank torchrun rehearsal of the multi-GPU path (gloo, both ranks on the one GPU)
# (FBA_OUT_DIR: where the logs go, default bench_out/)
cd "$(dirname "$0")/.."
export FBA_OUT_DIR=${FBA_OUT_DIR:-bench_out}
OUT=$FBA_OUT_DIR
bash scripts/gpu_check.sh tests smoke bench prof pmc || exit $?
for cfg in 3 5; do
  timeout -k 10 400 python bench.py --config $cfg --steps 10 --warmup 2 --full --no-cpu > "$OUT/bench_c$cfg.log" 2>&1
  rc=$?; echo "== config $cfg rc=$rc"; tail -1 "$OUT/bench_c$cfg.log" | cut -c1-300
  [ $rc -ne 0 ] && exit $rc
done
bash scripts/gpu_gloo2.sh  # both ranks on the one GPU: the flow kernels take their records from start-order tickets
