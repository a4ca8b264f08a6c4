#!/bin/bash
# Same-box A/B of library builds (development): each line of output = one arm's headline numbers.  The other tree is built
# into a second library first (EBFI_LIB_OUT=... EBFI_OBJ_DIR=... bash ebfi-be_amd/csrc/build.sh).
# usage (GPU box; files under $AB_OUT, default output/ab): tools/ab_bench.sh "NAME=ENV1=v ENV2=v" ...   e.g.  tools/ab_bench.sh "prev=EBFI_LIB_PATH=$PWD/ebfi-be_amd/lib/libebfi_hip_prev.so" "new="
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT="${AB_OUT:-output/ab}"
mkdir -p "$OUT"
for round in 1 2; do
for spec in "$@"; do
  name="${spec%%=*}"; envs="${spec#*=}"
  env EBFI_DEV=1 $envs timeout -k 10 200 python bench.py --steps 20 --warmup 3 --full --no-cpu-baseline --no-extra-legs --no-ops --no-inference --detail "$OUT/$name.$round.detail.json" > "$OUT/$name.$round.json" 2> "$OUT/$name.$round.err" || { echo "$name failed"; tail -3 "$OUT/$name.$round.err"; continue; }
  python3 - "$name" "$round" "$OUT" <<'PY'
import json,sys
d=json.load(open("%s/%s.%s.detail.json"%(sys.argv[3],sys.argv[1],sys.argv[2])))
k=d["kernels"]
top=sorted(k.items(), key=lambda kv:-kv[1]["total_ms"])[:4]
print("%-12s round %s: %7.3f ms/step  %s" % (sys.argv[1], sys.argv[2], d["ms_per_step"], "  ".join("%s %.1fx%.4f"%(n,v["launches_per_step"],v["avg_ms"]) for n,v in top)), flush=True)
PY
done; done
