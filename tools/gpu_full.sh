#!/bin/bash
# the round-end checks: every GPU test, smoke, then the full bench line
# (bench.py --full: the timed steps, every secondary leg, the CPU baseline).
# Logs and the line go to $OUT_DIR (default build/out).
set -o pipefail
export O=${OUT_DIR:-build/out}
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/pytest_gpu_full.log 2>&1
rc=$?; tail -3 $O/pytest_gpu_full.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
rc=$?; tail -2 $O/smoke.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > $O/bench_full.json 2> $O/bench_full.err
rc=$?; [ $rc -eq 0 ] || { tail -5 $O/bench_full.err; exit $rc; }
python - <<'PY'
import json
import os
d = json.load(open(os.path.join(os.environ["O"], "bench_full.json")))
print("value %.4g ms/step %.4f frac %.3f" % (d["value"], d["ms_per_step"], d["roofline"]["frac"]))
print("crash_leg", {k: d["crash_leg"][k] for k in ("call_ms", "fast_kernel_ms", "gap_kernel_ms")})
print("hot_key", d["hot_key"])
print("oversized", {k: d["oversized_key"][k] for k in ("fx_ms", "configs_explored", "max_frontier")})
print("c3", [(x["n_gpus"], round(x["implied_ms_per_step"], 4), round(x["implied_speedup"], 2)) for x in d["c3_shards"]])
print("model", {k: d["model_leg"].get(k) for k in ("call_ms", "hbm_kernel_ms")})
print("cpu", d["cpu_baseline"]["value"] if d.get("cpu_baseline") else None)
PY
