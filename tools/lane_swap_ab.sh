#!/bin/bash
# A/B of the headline step between built trees that differ in how the measuring walk runs its last gate group (through
# lane swaps on the registers of the group in front of it, or through the LDS tile: DESIGN 4.7, 9k).  The protocol is
# tools/unit_form_ab.sh's -- alternating runs, one tree after the other in every round, then the outputs of each tree
# against the first tree's and against oracle.c_port -- and so are the arguments:
#   usage: tools/lane_swap_ab.sh OUT_DIR ROUNDS [--full] NAME=TREE [NAME=TREE ...]     (the first tree is the reference)
# The summary lines also go to OUT_DIR/summary.txt (summary_full.txt with --full).
set -o pipefail
[ $# -ge 3 ] || { sed -n '2,7p' "$0"; exit 2; }
mkdir -p "$1" || exit 2
name=summary.txt
[ "$3" = "--full" ] && name=summary_full.txt
"$(dirname "$0")/unit_form_ab.sh" "$@" | tee "$1/$name"
