"""The Meyer-Wallach host path without a GPU (csrc/qmle_mw.hip): its public numbers against a table recorded from
the library before the path was given one read plan and one workspace layout (tests/golden/mw_layout_parent.json,
written by tests/golden/make_mw_layout_fixture.py from that build), the invariants of ``qmle_meyer_wallach_describe``,
and the status codes of the checks that come before the first HIP call."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from qml_essentials_amd import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mw_layout_parent.json")
BATCHES = (1, 2, 3, 7, 64, 1000)
MEAS_MW = N.MEAS["mw"]
DUMMY = C.c_void_p(0x1000)  # non-null, never dereferenced: every call below is refused before the first HIP call
ERR_INVALID_ARG, ERR_WORKSPACE = -1, -7


def plan_cases():
    """(name, n, ops, slots, consts, flags): one and two Hardware-Efficient layers at n = 12..32, and the random tapes
    of test_meyer_wallach_out_of_the_producing_pass at n = 15..24, with and without known-zero tracking."""
    from tests.helpers import random_tape, tape_to_native
    from tests.test_abi_cpu import he_layer_ops

    for n in range(12, 33):
        for layers in (1, 2):
            ops, slots = [], 0
            for _ in range(layers):
                o, sl = he_layer_ops(n)
                ops += [(g, w, [x + slots for x in k], m) for g, w, k, m in o]
                slots += sl
            yield "he%d_n%d" % (layers, n), n, ops, slots, None, 0
    for n in range(15, 25):
        rng = np.random.default_rng(100 + n)
        ops, values, consts = tape_to_native(random_tape(n, 3 * n, rng, three_q=n <= 12), n)
        for flags in (0, N.PLAN_NO_SPARSE):
            yield "random_n%d_f%d" % (n, flags), n, ops, len(values), consts, flags


@pytest.fixture(scope="module")
def plans():
    return {name: (n, N.Plan(ops, n, slots, consts=consts, flags=flags))
            for name, n, ops, slots, consts, flags in plan_cases()}


def last_tile_route(plan, batch, flags=0):
    """how a batch run's Meyer-Wallach pass would run the executed plan's last stage (None: no tile stage there)"""
    ex = plan.executed("mw")
    stages = ex.describe()["stages"]
    if not stages or stages[-1]["kind"] != "tile":
        return None
    return ex.tile_route(len(stages) - 1, batch, N.Plan.TM_STORE_MW, 0,
                         N.Plan.ROUTE_FROM_ZERO | N.Plan.ROUTE_MULTI_ROWS | flags)


def mw_call(states, n, batch, out, ws, ws_bytes):
    return N.lib().qmle_meyer_wallach(states, n, batch, out, None, ws, ws_bytes, None)


def largest_refused_workspace(n, batch):
    """the largest workspace qmle_meyer_wallach answers QMLE_ERR_WORKSPACE to (bisection; only for a machine without
    a GPU, where an accepted call fails at its first HIP call: the fixture's writer runs it, no test does)"""
    lo, hi = 0, int(N.lib().qmle_meyer_wallach_workspace_bytes(n, batch))  # lo: refused, hi: accepted
    assert mw_call(DUMMY, n, batch, DUMMY, DUMMY, lo) == ERR_WORKSPACE
    assert mw_call(DUMMY, n, batch, DUMMY, DUMMY, hi) != ERR_WORKSPACE
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if mw_call(DUMMY, n, batch, DUMMY, DUMMY, mid) == ERR_WORKSPACE:
            lo = mid
        else:
            hi = mid
    return lo


STATUS_CASES = {  # name -> (states, n, batch, out, workspace, bytes)
    "null_states": (None, 14, 1, DUMMY, DUMMY, 1 << 30), "null_out": (DUMMY, 14, 1, None, DUMMY, 1 << 30),
    "null_workspace": (DUMMY, 14, 1, DUMMY, None, 1 << 30), "n_0": (DUMMY, 0, 1, DUMMY, DUMMY, 1 << 30),
    "n_33": (DUMMY, 33, 1, DUMMY, DUMMY, 1 << 30), "batch_0": (DUMMY, 14, 0, DUMMY, DUMMY, 1 << 30),
    "batch_65536": (DUMMY, 14, 65536, DUMMY, DUMMY, 1 << 40), "no_workspace_n5": (DUMMY, 5, 3, DUMMY, DUMMY, 0),
    "no_workspace_n20": (DUMMY, 20, 3, DUMMY, DUMMY, 0),
}
SHORT_CASES = [(n, b) for n in (1, 5, 11, 12, 13, 17, 20, 24, 28, 32) for b in (1, 3, 64)]


def public_numbers(plans, with_thresholds=False):
    """what the fixture records and the first test recomputes"""
    L = N.lib()
    rec = {"reads": [int(L.qmle_meyer_wallach_reads(n)) for n in range(34)],
           "workspace_bytes": {"%d,%d" % (n, b): int(L.qmle_meyer_wallach_workspace_bytes(n, b))
                               for n in range(1, 33) for b in BATCHES},
           "plans": {}, "status": {k: int(mw_call(*v)) for k, v in STATUS_CASES.items()}}
    for name, (n, plan) in plans.items():
        lean = [None if r is None else bool(r["mw_lean"])
                for r in (last_tile_route(plan, 1), last_tile_route(plan, 1, N.Plan.ROUTE_NO_MW_LEAN))]
        rec["plans"][name] = {"workspace_bytes": [int(L.qmle_workspace_bytes(plan._h, b, MEAS_MW, 0, 0)) for b in BATCHES],
                              "mw_lean": lean[0], "mw_lean_switched_off": lean[1]}
    if with_thresholds:
        rec["largest_refused_workspace"] = {"%d,%d" % nb: largest_refused_workspace(*nb) for nb in SHORT_CASES}
    return rec


def test_public_numbers_are_the_parents(plans):
    """Reads per call, workspace sizes of the stand-alone entry and of batch runs, the route's ``mw_lean`` with and
    without QMLE_ROUTE_NO_MW_LEAN, and the status codes of refused calls: what the library returned before."""
    want = json.load(open(GOLDEN))
    got = public_numbers(plans)
    assert got["reads"] == want["reads"]
    assert got["workspace_bytes"] == want["workspace_bytes"]
    assert got["status"] == want["status"]
    assert sorted(got["plans"]) == sorted(want["plans"])
    for name in want["plans"]:
        assert got["plans"][name] == want["plans"][name], name
    assert got["status"]["n_33"] == ERR_INVALID_ARG and got["status"]["no_workspace_n20"] == ERR_WORKSPACE


def check_description(d, n, batch, tile_bits=None):
    """invariants of one description; tile_bits: the producing tile's positions (fused route)"""
    reads, pos = d["reads"], d["positions"]
    assert d["n"] == n and d["batch"] == batch and len(pos) == n
    for r in reads:  # a read's tile: positions 0..3 and two runs of four
        assert 4 <= r["lo"] and r["lo"] + 4 <= r["lo2"] and r["lo2"] + 4 <= n, r
        assert r["rows"] == (2 ** (n - 12)) >> r["q"] and r["stride"] == {"later": 16, "later_low": 24}[r["kind"]], r
        assert r["nt"] == (batch * 8 * 2 ** n >= 2 ** 30)
    assert [r["kind"] for r in reads[1:]].count("later_low") == 0 and d["lean"] == (bool(reads) and reads[0]["kind"] == "later_low")
    for p, src in enumerate(pos):  # exactly one source each, and that source does report the position
        if src["read"] < 0:
            assert (p in tile_bits) if tile_bits is not None else (p < 12 or n < 12), (p, src)
            continue
        r, c = reads[src["read"]], src["col"]
        assert p == (r["lo"] + c if c < 4 else r["lo2"] + c - 4 if c < 8 else c - 8), (p, src, r)
        assert c < 8 or r["kind"] == "later_low"
        assert tile_bits is None or p not in tile_bits or (d["lean"] and p < 4), (p, src)
    regs = sorted(d["regions"], key=lambda g: g["offset"])
    for g in regs:
        assert g["bytes"] > 0 and g["offset"] % (8 if g["doubles"] else 4) == 0, g
    for a, b in zip(regs, regs[1:]):
        assert a["offset"] + a["bytes"] <= b["offset"], (a, b)
    assert max(g["offset"] + g["bytes"] for g in regs) == d["end"] <= d["total_bytes"]


def test_description_of_resident_states():
    """Every position has one source, every later read the kernel's shape, the regions are aligned, disjoint and
    inside the reported size -- which is the public one --, the read count is the public one, and the layout of a
    batch fits into that many layouts of one state (what the engine's chunk workspace relies on)."""
    L = N.lib()
    for n in range(1, 33):
        one = N.mw_describe(n, 1)
        for b in BATCHES:
            d = N.mw_describe(n, b)
            assert d["route"] == "standalone" and not d["fusable"] and not d["lean"]
            check_description(d, n, b)
            assert d["total_bytes"] == L.qmle_meyer_wallach_workspace_bytes(n, b)
            assert d["total_bytes"] <= b * (-(-one["total_bytes"] // 256) * 256), (n, b)
            if n >= 12:
                assert d["first"]["kind"] == "first" and d["first"]["rows"] == (2 ** (n - 12)) >> d["first"]["q"]
                assert 1 + len(d["reads"]) == L.qmle_meyer_wallach_reads(n) and d["finish"] == "standalone"
            else:
                assert d["first"] is None and not d["reads"] and d["finish"] == "per-wire-sweeps"


def test_description_of_the_fused_route(plans):
    """The same invariants behind a producing pass, with and without the lean split, for every plan of the table;
    ``fusable`` means fewer later reads than the stand-alone route; the three finishes all occur.  The smallest shape
    of the table whose finish is "per-position" is one Hardware-Efficient layer at n = 29 (tile of 12 positions, 17
    signed totals: more than the column kernels' 64-column map holds); tests/test_gpu_mw_finishes.py runs that finish
    there (test_fused_route_at_its_natural_sizes) and, with QMLE_MW_FINISH_PER_POSITION=1, at n = 15..26
    (test_per_position_finish_forced).  With QMLE_ROUTE_MW_PER_POSITION every tiled plan of the table describes that
    finish, with and without the lean split, inside the workspace that was sized without the flag."""
    PP = N.Plan.ROUTE_MW_PER_POSITION
    finishes, smallest = set(), None
    for name, (n, plan) in plans.items():
        route = last_tile_route(plan, 1)
        stage = plan.executed("mw").describe()["stages"][-1]
        for flags in (0, N.Plan.ROUTE_NO_MW_LEAN):
            one = N.mw_describe(0, 1, plan=plan, flags=flags)
            for b in BATCHES:
                d = N.mw_describe(0, b, plan=plan, flags=flags)
                assert d["total_bytes"] <= b * (-(-one["total_bytes"] // 256) * 256), (name, b)
                if d["route"] == "resident":
                    assert not d["fusable"] and d["finish_threads"] == 0
                    check_description(d, n, b)
                    assert N.mw_describe(0, b, plan=plan, flags=flags | PP) == d  # nothing to switch
                    continue
                assert d["route"] == "fused" and d["fusable"] and route is not None and d["first"] is None
                check_description(d, n, b, tile_bits=set(stage["bits"]))
                assert len(d["reads"]) < N.mw_reads(n) or stage["T"] == n
                assert d["lean"] == (bool(route["mw_lean"]) and not flags)
                finishes.add(d["finish"])
                if d["finish"] == "per-position" and b == 1 and (smallest is None or n < smallest[0]):
                    smallest = (n, name)
                assert (d["finish"] == "whole-state") == (stage["T"] == n)
                assert d["finish_threads"] == 64 or d["finish"] != "whole-state"
                assert d["finish_threads"] == 256 or d["finish"] != "columns"
                # the same call with the per-position finish asked for
                f = N.mw_describe(0, b, plan=plan, flags=flags | PP)
                check_description(f, n, b, tile_bits=set(stage["bits"]))
                assert f["finish"] == ("whole-state" if stage["T"] == n else "per-position"), (name, b, f["finish"])
                assert f["end"] <= f["total_bytes"] == d["total_bytes"], (name, b)
                assert f["total_bytes"] <= b * (-(-one["total_bytes"] // 256) * 256), (name, b)
                assert (f["reads"], f["positions"], f["lean"]) == (d["reads"], d["positions"], d["lean"])
                if f["finish"] == "per-position":
                    most = max([2 ** (n - stage["T"])] + [r["rows"] for r in f["reads"]])
                    per = most // f["slices"]
                    assert f["finish_threads"] == (1024 if per >= 1024 else 256 if per >= 256 else 64), (name, b)
                    names = [g["name"] for g in f["regions"]]
                    assert "purities" in names and ("partial" in names) == (f["slices"] > 1), (name, b, names)
                    assert not any(g.startswith("colsum") for g in names)
                if d["finish"] == "per-position":
                    assert f == d
    assert finishes == {"whole-state", "columns", "per-position"}
    assert smallest == (29, "he1_n29"), smallest


def test_description_refuses_bad_arguments(plans):
    L = N.lib()
    assert L.qmle_meyer_wallach_describe(None, 0, 1, 0, 0, None, 0) == ERR_INVALID_ARG
    assert L.qmle_meyer_wallach_describe(None, 33, 1, 0, 0, None, 0) == ERR_INVALID_ARG
    assert L.qmle_meyer_wallach_describe(None, 20, 0, 0, 0, None, 0) == ERR_INVALID_ARG
    assert L.qmle_meyer_wallach_describe(None, 20, 65536, 0, 0, None, 0) == ERR_INVALID_ARG
    assert L.qmle_meyer_wallach_describe(plans["he1_n20"][1]._h, 0, 1, 99, 0, None, 0) == ERR_INVALID_ARG


def test_workspace_check_comes_first_and_is_exact():
    """One byte less than the call needs (the description's "end") is QMLE_ERR_WORKSPACE -- as it was before: the
    table holds the largest workspace the parent refused, never smaller than that -- and every refusal of the table's
    bad arguments comes before any HIP call (dummy pointers).  The accepted sizes need a GPU:
    tests/test_gpu_kernels.py::test_meyer_wallach_workspace_of_the_reported_size."""
    want = json.load(open(GOLDEN))["largest_refused_workspace"]
    for n, b in SHORT_CASES:
        end = N.mw_describe(n, b)["end"]
        assert mw_call(DUMMY, n, b, DUMMY, DUMMY, end - 1) == ERR_WORKSPACE, (n, b)
        assert end - 1 <= want["%d,%d" % (n, b)] < N.lib().qmle_meyer_wallach_workspace_bytes(n, b), (n, b)
