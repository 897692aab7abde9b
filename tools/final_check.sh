#!/bin/bash
# Run on an MI355X: smoke, the whole GPU suite, the full bench line -- each under a time limit, stopping at the first failure.
# Usage: tools/final_check.sh <output dir>
set -e -o pipefail
OUT=$(mkdir -p "${1:?usage: tools/final_check.sh <output dir>}" && cd "$1" && pwd)
cd "$(dirname "$0")/.."
timeout -k 10 600 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.txt" 2>&1; tail -1 "$OUT/smoke.txt"
timeout -k 10 2400 python -m pytest tests -m gpu -q -x > "$OUT/pytest.txt" 2>&1; tail -3 "$OUT/pytest.txt"
timeout -k 10 900 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"
python - "$OUT/bench.json" <<'PY'
import json, sys
j=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("value", j["value"], "one", j.get("value_one_in_flight"), "kernel_ms", j["roofline"]["kernel_ms"], "frac", j["roofline"]["frac"], "h2d", j["value_incl_h2d"]["value"])
e=j["extra"]
print("config1", e["config1"]["value"], e["config1"]["sampler_ms"], "at_scale", e["config1"]["at_scale"]["value"], e["config1"]["at_scale"]["units_per_s"])
print("dedup", e["config2_dedup"]["value"]); print("moving", e["moving"]["reads_16"]["value"], e["moving"]["reads_40"]["value"]); print("c4", e["config4"]["value"], "c5", e["config5"]["value"], e["config5"]["value_one_in_flight"], "e2e", e["program_e2e"]["value"])
print("cpu", j["cpu_baseline"]["value"], j["cpu_baseline"].get("mode_call_concordance"))
PY
