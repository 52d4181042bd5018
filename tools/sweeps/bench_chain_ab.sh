# headline + configs[4] leg with the fp16-only chain on / off, from the repo root: bash tools/sweeps/bench_chain_ab.sh OUTDIR
OUT=${1:?usage: bench_chain_ab.sh OUTDIR}
mkdir -p "$OUT"
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-exact > "$OUT/b2.json" 2> "$OUT/b2.err"
python - <<PY
import json
d=json.loads(open("$OUT/b2.json").read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], {k: d["config4_fp16"][k] for k in ("value", "ms_per_step")}, d.get("round1_workload"))
PY
JTSM_CHAIN16=0 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-exact --no-roofline > "$OUT/b3.json" 2> "$OUT/b3.err"
python - <<PY
import json
d=json.loads(open("$OUT/b3.json").read().strip().splitlines()[-1])
print("chain off:", d["value"], d["ms_per_step"], {k: d["config4_fp16"][k] for k in ("value", "ms_per_step")})
PY
