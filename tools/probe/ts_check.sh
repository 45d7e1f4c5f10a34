#!/bin/bash
# GPU box: the parity suite, then GlomeView's default scene in both render modes (a quick A/B for generic-tier changes)
tag=${1:-ts}
out=${OUT_DIR:-bench_out}; mkdir -p $out  # the pytest log, the bench lines and their stderr
PYTHONUNBUFFERED=1 timeout -k 10 600 python -m pytest tests -m gpu -x -v > $out/${tag}_pytest.log 2>&1 || { tail -30 $out/${tag}_pytest.log; exit 1; }
tail -1 $out/${tag}_pytest.log
for mode in 0 1; do
  timeout -k 10 200 python bench.py --full --scene TS --mode $mode --no-cpu > $out/${tag}_TS$mode.json 2> $out/${tag}_TS$mode.err || exit 1
done
python - <<PY
import json
for mode in (0, 1):
    j = json.loads(open("$out/${tag}_TS%d.json" % mode).read().strip().splitlines()[-1])
    print("TS mode", mode, j["ms_per_step"], "ms", j["value"], "Mrays/s, single frame", j["latency"]["single_frame_ms"])
PY
