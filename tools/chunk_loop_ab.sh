#!/bin/bash
# A/B of the headline step between built trees that differ in how ChunkPipeline orders the chunks:
# alternating runs, one tree after the other in every round.
#   usage: tools/chunk_loop_ab.sh OUT_DIR ROUNDS NAME=TREE [NAME=TREE ...]
# Per round and tree: bench.py --gpus 1 --steps 20 --warmup 5; then one run of the first tree on one stream
# (QMLE_NO_CHUNK_OVERLAP=1), one --dump-outputs run per tree, and per tree median and spread of ms_per_step and the
# largest difference of its expval.npy from the first tree's.  Every GPU step has its own time limit and the script
# stops at the first step that fails.  (Kernel traces: tools/fill_reuse_ab.sh `trace`, read with tools/chunk_gaps.py.)
set -o pipefail
mkdir -p "$1" && OUT=$(cd "$1" && pwd) || exit 2
ROUNDS=$2
shift 2
NAMES=(); TREES=()
for nt in "$@"; do
  NAMES+=("${nt%%=*}")
  TREES+=("$(cd "${nt#*=}" && pwd)") || exit 2
done
bench() {  # name tree [VAR=value]
  local name=$1 tree=$2; shift 2
  ( cd "$tree" && env "$@" timeout -k 10 150 python bench.py --gpus 1 --steps 20 --warmup 5 2>"$OUT/$name.err" | tail -1 >"$OUT/$name.json" ) || return $?
  python -c "import json; d = json.load(open('$OUT/$name.json')); print('$name', d['ms_per_step'])"
}
dump() {  # name tree
  ( cd "$2" && timeout -k 10 150 python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs "$OUT/dump_$1" 2>"$OUT/dump_$1.err" | tail -1 >"$OUT/dump_$1.json" ) || return $?
}
for r in $(seq 1 "$ROUNDS"); do
  for i in "${!NAMES[@]}"; do
    bench "${NAMES[$i]}_$r" "${TREES[$i]}" || { echo "bench failed in round $r"; exit 1; }
  done
done
bench "${NAMES[0]}_one_stream" "${TREES[0]}" QMLE_NO_CHUNK_OVERLAP=1 || exit 1
for i in "${!NAMES[@]}"; do
  dump "${NAMES[$i]}" "${TREES[$i]}" || { echo "dump failed"; exit 1; }
done
OUT="$OUT" NAMES="${NAMES[*]}" python - <<'PY'
import glob, json, os, statistics
import numpy as np
O, names = os.environ["OUT"], os.environ["NAMES"].split()
for name in names:
    ms = [json.load(open(f))["ms_per_step"] for f in sorted(glob.glob(os.path.join(O, name + "_[0-9]*.json")))]
    print(f"{name}: ms_per_step {ms} median {statistics.median(ms):.3f} spread {max(ms) - min(ms):.3f}")
first = np.load(os.path.join(O, "dump_" + names[0], "expval.npy"))
for name in names[1:]:
    other = np.load(os.path.join(O, "dump_" + name, "expval.npy"))
    print(f"expval.npy {names[0]} vs {name}: max |diff| {float(np.abs(first - other).max())}, identical {np.array_equal(first, other)}")
PY
