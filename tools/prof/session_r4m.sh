bash tools/prof/ab_round.sh r4m 50000000 new lsd:ELP_TUNE=tie_rounds=1
OUT=${OUT:-$PWD/session_out/r4m}; mkdir -p $OUT; export OUT
timeout 600 python bench.py --full > $OUT/bench_full.json 2> $OUT/bench_full.err; echo "full rc=$?"
python - <<'PY'
import json, os
d=json.load(open(os.path.join(os.environ["OUT"], "bench_full.json")))
print(d["ms_per_step"], d["value"], d["stage_ms_per_step"], d.get("host_finalize_ms_per_step"), d.get("host_finalize_exposed_ms_per_step"))
for k,e in d["extra"].items():
    if isinstance(e,dict) and "value" in e: print(k, e["value"], e.get("ms_per_step"), e.get("host_finalize_ms_per_step"), e.get("host_finalize_exposed_ms_per_step"))
print(d["verify"]["ok"])
PY
