#!/bin/bash
# bench.py --full without the CPU baseline, summarised: value, ms/step, per-kernel ms of the headline and the secondary workloads.
# Usage: tools/bench_summary.sh [steps] [output directory for bench.json / bench.err; default: a new temporary directory]
O=${2:-$(mktemp -d)}; mkdir -p "$O"
python bench.py --full --steps ${1:-100} --warmup 10 --no-cpu-baseline > "$O/bench.json" 2> "$O/bench.err" || { tail -5 "$O/bench.err"; exit 1; }
python - "$O/bench.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print("headline %.0f env-steps/s %.4f ms/step" % (d["value"], d["ms_per_step"]), {k: v["avg_ms"] for k, v in d["roofline"]["kernels"].items()})
for s in d.get("secondary", []):
    if "value" in s:            # (config 1 reports camera_off / camera_on instead, config 5 end to end no kernel times)
        print("  %.0f env-steps/s %.4f ms/step" % (s["value"], s["ms_per_step"]), s.get("kernels_ms", ""), "|", s["workload"][:40])
    else:
        print("  ", {k: v for k, v in s.items() if k in ("camera_off", "camera_on", "error")}, "|", s["workload"][:40])
PY
