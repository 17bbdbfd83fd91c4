#!/bin/bash
# A/B of the headline step for a change of the host run path: two built trees side by side, alternating runs.
#   usage: tools/fill_reuse_ab.sh PARENT_TREE OUT_DIR [rounds]      (run from the root of the tree under test)
# Per round: bench.py of the parent | of this tree | of this tree on one stream (QMLE_NO_CHUNK_OVERLAP=1); then one
# `rocprofv3 --kernel-trace --stats` run of each (k_fill_zero calls per step, per-kernel times) and one --dump-outputs
# run of each plus a second one of the parent (what two runs of the same code differ by).  Every GPU step has its own
# time limit and the script stops at the first step that fails.
set -o pipefail
PARENT=$(cd "$1" && pwd) || exit 2
mkdir -p "$2" && OUT=$(cd "$2" && pwd) || exit 2
ROUNDS=${3:-3}
HERE=$(pwd)
bench() {  # name tree [VAR=value]
  local name=$1 tree=$2; shift 2
  ( cd "$tree" && env "$@" timeout -k 10 150 python bench.py --gpus 1 --steps 20 --warmup 3 2>"$OUT/$name.err" | tail -1 >"$OUT/$name.json" ) || return $?
  python -c "import json; d = json.load(open('$OUT/$name.json')); print('$name', d['ms_per_step'], d['hbm_bytes_moved_per_state'], d['step_moved_frac_of_8TBps'])"
}
trace() {  # name tree
  ( cd "$2" && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_$1" -- python bench.py --gpus 1 --steps 5 --warmup 1 >"$OUT/trace_$1.json" 2>"$OUT/trace_$1.err" ) || return $?
  echo "trace $1 ok"
}
dump() {  # name tree
  ( cd "$2" && timeout -k 10 150 python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs "$OUT/dump_$1" 2>"$OUT/dump_$1.err" | tail -1 >"$OUT/dump_$1.json" ) || return $?
}
for r in $(seq 1 "$ROUNDS"); do
  bench parent_$r "$PARENT" && bench this_$r "$HERE" &&
    bench this_one_stream_$r "$HERE" QMLE_NO_CHUNK_OVERLAP=1 || { echo "bench failed in round $r"; exit 1; }
done
trace parent "$PARENT" && trace this "$HERE" &&
  dump parent_a "$PARENT" && dump parent_b "$PARENT" && dump this "$HERE" || { echo "trace / dump failed"; exit 1; }
OUT="$OUT" python - <<'PY'
import glob, json, os, statistics
import numpy as np
O = os.environ["OUT"]
for name in ("parent", "this", "this_one_stream"):
    ms = [json.load(open(f))["ms_per_step"] for f in sorted(glob.glob(os.path.join(O, name + "_[0-9]*.json")))]
    print(f"{name}: ms_per_step {ms} median {statistics.median(ms):.3f} spread {max(ms) - min(ms):.3f}")
a, b, c = (np.load(os.path.join(O, "dump_" + k, "expval.npy")) for k in ("parent_a", "parent_b", "this"))
print("expval.npy max |diff|: parent vs parent", float(np.abs(a - b).max()), "parent vs this", float(np.abs(a - c).max()))
import csv
for k in ("parent", "this"):  # per kernel of the step: calls per step (5 timed + 1 warm-up step) and average launch time
    for f in glob.glob(os.path.join(O, "trace_" + k, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Name", "")
            if name.startswith(("k_fill_zero", "k_tile", "void k_fill_zero", "void k_tile", "k_expval_final", "k_build")) or "k_tile" in name[:40]:
                print(f"{k}: {name[:70]:70s} calls/step {int(row['Calls']) / 6:7.1f}  avg {float(row['AverageNs']) / 1e6:.4f} ms  total {float(row['TotalDurationNs']) / 1e6:.1f} ms")
PY
