#!/bin/bash
# Same-box A/B of library builds or of whole trees (development): each line of output = one arm's headline numbers.  The other
# tree is built into a second library first (EBFI_LIB_OUT=... EBFI_OBJ_DIR=... bash ebfi-be_amd/csrc/build.sh) -- or, when its
# C ABI differs (the binding refuses a library that lacks a declared symbol), exported and built as a tree of its own and named
# with AB_TREE=<path>: that arm then runs ITS bench.py over ITS package.  The arms alternate inside every round, so a drift of
# the box shows in both.  The first run that fails ends the script: nothing more is started on a device that may have faulted.
# usage (GPU box; files under $AB_OUT, default output/ab): tools/ab_bench.sh "NAME=ENV1=v ENV2=v" ...   e.g.
#   tools/ab_bench.sh "prev=EBFI_LIB_PATH=$PWD/ebfi-be_amd/lib/libebfi_hip_prev.so" "new="
#   AB_ROUNDS=3 tools/ab_bench.sh "parent=AB_TREE=/tmp/parent_tree" "new="
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT="${AB_OUT:-output/ab}"
mkdir -p "$OUT"
OUT="$(cd "$OUT" && pwd)"
for round in $(seq 1 "${AB_ROUNDS:-2}"); do
for spec in "$@"; do
  name="${spec%%=*}"; envs="${spec#*=}"
  tree="."
  for kv in $envs; do case "$kv" in AB_TREE=*) tree="${kv#AB_TREE=}";; esac; done
  ( cd "$tree" && env EBFI_DEV=1 $envs timeout -k 10 200 python bench.py --steps 20 --warmup 3 --full --no-cpu-baseline --no-extra-legs --no-ops --no-inference --detail "$OUT/$name.$round.detail.json" > "$OUT/$name.$round.json" 2> "$OUT/$name.$round.err" ) || { echo "$name failed"; tail -3 "$OUT/$name.$round.err"; exit 1; }
  python3 - "$name" "$round" "$OUT" <<'PY'
import json,sys
d=json.load(open("%s/%s.%s.detail.json"%(sys.argv[3],sys.argv[1],sys.argv[2])))
k=d["kernels"]
top=sorted(k.items(), key=lambda kv:-kv[1]["total_ms"])[:4]
print("%-12s round %s: %7.3f ms/step  %s" % (sys.argv[1], sys.argv[2], d["ms_per_step"], "  ".join("%s %.1fx%.4f"%(n,v["launches_per_step"],v["avg_ms"]) for n,v in top)), flush=True)
PY
done; done
