#!/bin/bash
# GPU test-suite, the 2-rank rehearsal of `bench.py --gpus 2 --full` (self-spawned ranks, parity gate,
# host-staged point-to-point transport), then the N = 1 --full bench line.  Outputs under $OUT (default out/).
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-$PWD/out}; mkdir -p "$OUT"
export TMPDIR=/tmp
timeout 1500 python -m pytest tests -m gpu -x -q > $OUT/pytest_gpu.log 2>&1
echo "pytest rc=$?" | tee -a $OUT/pytest_gpu.log
tail -5 $OUT/pytest_gpu.log
LF_BENCH_REHEARSE=1 timeout 900 python bench.py --gpus 2 --steps 5 --warmup 2 --full > $OUT/bench_rehearse2.json 2> $OUT/bench_rehearse2.err
echo "rehearsal rc=$?"
tail -c 1500 $OUT/bench_rehearse2.json
tail -5 $OUT/bench_rehearse2.err
timeout 900 python bench.py --full > $OUT/bench_n1.json 2> $OUT/bench_n1.err
echo "bench rc=$?"
OUT=$OUT python - <<'PY'
import json, os
j = json.loads(open(os.path.join(os.environ["OUT"], "bench_n1.json")).read().strip().splitlines()[-1])
print("value", j["value"], "roofline", j["roofline"]["frac"], j["roofline"]["avg_launch_ms"], j["roofline"]["column_pass_launch_ms"])
print({k: round(v, 1) for k, v in j["extra"].items() if isinstance(v, float)})
PY
