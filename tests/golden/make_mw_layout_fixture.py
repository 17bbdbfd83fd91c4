"""Writes mw_layout_parent.json: ``python tests/golden/make_mw_layout_fixture.py --lib PATH`` on a machine WITHOUT a GPU.

PATH is a libqmle_sv.so built from the commit before the Meyer-Wallach host path got its own unit: the numbers are
that library's answers (reads per call, workspace sizes, ``mw_lean`` of the route, status codes, and by bisection
the largest workspace ``qmle_meyer_wallach`` refuses), not this tree's.  tests/test_mw_layout_cpu.py defines the
cases and recomputes them from the tree."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from qml_essentials_amd import _native as N  # noqa: E402


def main(argv):
    import torch

    assert not torch.cuda.is_available(), "accepted calls must fail at their first HIP call: run this without a GPU"
    N.LIB_PATH = os.path.abspath(argv[argv.index("--lib") + 1])
    handle = C.CDLL(N.LIB_PATH)
    N.SYMBOLS = [s for s in N.SYMBOLS if hasattr(handle, s[0])]  # (an older library lacks the newer entries)
    from tests import test_mw_layout_cpu as T

    plans = {name: (n, N.Plan(ops, n, slots, consts=consts, flags=flags))
             for name, n, ops, slots, consts, flags in T.plan_cases()}
    with open(os.path.join(HERE, "mw_layout_parent.json"), "w") as f:
        json.dump(T.public_numbers(plans, with_thresholds=True), f, indent=0, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
