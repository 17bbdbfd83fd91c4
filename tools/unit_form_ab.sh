#!/bin/bash
# A/B of the headline step between built trees that differ in how the fast tile kernel applies its dense gates
# (unit-pivot form): alternating runs, one tree after the other in every round.
#   usage: tools/unit_form_ab.sh OUT_DIR ROUNDS NAME=TREE [NAME=TREE ...]     (the first tree is the reference)
#          tools/unit_form_ab.sh OUT_DIR ROUNDS --full NAME=TREE ...          (bench.py --full: every named leg)
# Per round and tree: bench.py --gpus 1 --steps 20 --warmup 5; then one --dump-outputs run per tree, and per tree the
# median and spread of ms_per_step and of the measuring pass's avg_launch_ms, the largest difference of its expval.npy
# from the first tree's, and each tree's largest error against oracle.c_port on rows 0, 511 and 1023.  With --full:
# median and spread of every leg's ms per tree, and the legs of a later tree slower than the first tree's median by
# more than its spread.  Every GPU step has its own time limit and the script stops at the first step that fails.
set -o pipefail
mkdir -p "$1" && OUT=$(cd "$1" && pwd) || exit 2
ROUNDS=$2
shift 2
FULL=
if [ "$1" = "--full" ]; then FULL=--full; shift; fi
NAMES=(); TREES=()
for nt in "$@"; do
  NAMES+=("${nt%%=*}")
  TREES+=("$(cd "${nt#*=}" && pwd)") || exit 2
done
bench() {  # name tree
  local name=$1 tree=$2 limit=150
  [ -n "$FULL" ] && limit=420
  ( cd "$tree" && timeout -k 10 $limit python bench.py --gpus 1 --steps 20 --warmup 5 $FULL 2>"$OUT/$name.err" | tail -1 >"$OUT/$name.json" ) || return $?
  python -c "import json; d = json.load(open('$OUT/$name.json')); print('$name', d['ms_per_step'], d['roofline'].get('avg_launch_ms'))"
}
dump() {  # name tree
  ( cd "$2" && timeout -k 10 150 python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs "$OUT/dump_$1" 2>"$OUT/dump_$1.err" | tail -1 >"$OUT/dump_$1.json" ) || return $?
}
for r in $(seq 1 "$ROUNDS"); do
  for i in "${!NAMES[@]}"; do
    bench "${NAMES[$i]}_$r" "${TREES[$i]}" || { echo "bench failed in round $r (${NAMES[$i]})"; exit 1; }
  done
done
if [ -z "$FULL" ]; then
  for i in "${!NAMES[@]}"; do
    dump "${NAMES[$i]}" "${TREES[$i]}" || { echo "dump failed"; exit 1; }
  done
fi
OUT="$OUT" NAMES="${NAMES[*]}" FULL="$FULL" TREE0="${TREES[0]}" python - <<'PY'
import glob, json, os, statistics, sys
import numpy as np
O, names, full = os.environ["OUT"], os.environ["NAMES"].split(), bool(os.environ["FULL"])
runs = {name: [json.load(open(f)) for f in sorted(glob.glob(os.path.join(O, name + "_[0-9]*.json")))] for name in names}
def stat(v):
    return f"{v} median {statistics.median(v):.4f} spread {max(v) - min(v):.4f}"
for name in names:
    print(f"{name}: ms_per_step {stat([d['ms_per_step'] for d in runs[name]])}")
    print(f"{name}: measuring pass avg_launch_ms {stat([d['roofline']['avg_launch_ms'] for d in runs[name]])}")
if full:
    def legs(d, prefix=""):  # every numeric field whose name ends in ms, by path
        out = {}
        for k, v in d.items():
            if isinstance(v, dict):
                out.update(legs(v, prefix + k + "."))
            elif isinstance(v, (int, float)) and not isinstance(v, bool) and (k == "ms" or k.endswith("_ms") or k == "ms_per_step"):
                out[prefix + k] = float(v)
        return out
    tables = {name: [legs(d) for d in runs[name]] for name in names}
    ref = names[0]
    for key in sorted(tables[ref][0]):
        if not all(key in t for name in names for t in tables[name]):
            continue
        row, slow = [], False
        base = [t[key] for t in tables[ref]]
        for name in names:
            v = [t[key] for t in tables[name]]
            row.append(f"{name} {statistics.median(v):.4f} (+-{max(v) - min(v):.4f})")
            if name != ref and statistics.median(v) > statistics.median(base) + (max(base) - min(base)):
                slow = True
        print(("SLOWER  " if slow else "        ") + key + ": " + " | ".join(row))
    sys.exit(0)
first = np.load(os.path.join(O, "dump_" + names[0], "expval.npy"))
for name in names[1:]:
    other = np.load(os.path.join(O, "dump_" + name, "expval.npy"))
    print(f"expval.npy {names[0]} vs {name}: max |diff| {float(np.abs(first - other).max())}, identical {np.array_equal(first, other)}")
sys.path.insert(0, os.environ["TREE0"])
from oracle import c_port, circuits as OC
from qml_essentials_amd.model import Model
shape = Model(24, 1, "Hardware_Efficient", data_reupload=False).params.shape[1:]
params = np.random.default_rng(1000).uniform(0, 2 * np.pi, (1024, *shape)).astype(np.float32)
spec = OC.ModelSpec(24, 1, "Hardware_Efficient", data_reupload=False)
rows = (0, 511, 1023)
want = [c_port.expval_z(c_port.simulate(OC.model_tape(spec, params[k], [0.0]), 24), 24, list(range(24))) for k in rows]
for name in names:
    ev = np.load(os.path.join(O, "dump_" + name, "expval.npy"))
    print(f"{name}: max |err| vs oracle.c_port on rows {rows}: {max(float(np.abs(w - ev[k]).max()) for w, k in zip(want, rows))}")
PY
