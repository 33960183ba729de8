#!/bin/bash
# Issue counters of the rollout's actor launch (actor_sample_kernel and, where the build has it, actor_pack_kernel): ONE counter-only pass of rocprofv3
# (no tracing beside it) over bench.py --steps 3 --warmup 2; means per launch.   bash tools/actor_pmc.sh <tag> [repository root]  ->  <out>/<tag>_actor_pmc.json
set -e
TAG=${1:-actor}
R=$(cd "${2:-$(dirname "$0")/..}" && pwd)
OUT=${BG_PROFILE_OUT:-$R/logs/profile}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_VMEM SQ_WAIT_INST_ANY --output-format csv \
  -d "$OUT/prof_${TAG}_actor_pmc" -- python3 "$R/bench.py" --steps 3 --warmup 2 > "$OUT/prof_${TAG}_actor_pmc.log" 2>&1
python3 - "$TAG" "$OUT" <<'PY'
import collections, csv, glob, json, os, sys
tag, out = sys.argv[1:3]
f = sorted(glob.glob(f"{out}/prof_{tag}_actor_pmc/**/*counter_collection.csv", recursive=True), key=os.path.getmtime)[-1]
acc = collections.defaultdict(lambda: collections.defaultdict(list))
for r in csv.DictReader(open(f)):
    name = r["Kernel_Name"].split("(")[0].replace("void ", "").strip()
    if name in ("actor_sample_kernel", "actor_pack_kernel"):
        acc[name][r["Counter_Name"]].append(float(r["Counter_Value"]))
res = {k: dict(launches=len(next(iter(cs.values()))), **{c: sum(v) / len(v) for c, v in cs.items()}) for k, cs in acc.items()}
json.dump({"command": "tools/actor_pmc.sh: rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_VMEM SQ_WAIT_INST_ANY -- python3 bench.py --steps 3 --warmup 2",
           "units": "means per launch of the sums rocprofv3 reports over the chip", "kernels": res}, open(f"{out}/{tag}_actor_pmc.json", "w"), indent=1)
for k, v in res.items():
    print(k, " ".join(f"{c}={x:.0f}" for c, x in v.items()))
PY
