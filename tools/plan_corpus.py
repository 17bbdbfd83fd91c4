#!/usr/bin/env python3
"""What the plan compiler (csrc/qmle_plan.cpp) makes of a fixed corpus of tapes, one line per case: the case name, the
compile status and the SHA-256 of everything a plan reports without a GPU -- describe() of the plan, of executed(m) for
every measurement, and the tile routes of the executed <Z> view -- and one digest over all lines.  A change that is not
meant to change any plan is checked by running this against the library before and after it: the outputs must be equal
byte for byte (profiles/plan_refactor.md).

    python tools/plan_corpus.py [--lib PATH/libqmle_sv.so] [--out FILE]

tests/test_plan_corpus_cpu.py imports cases(), compile_text() and missing_branches()."""
import ctypes as C
import hashlib
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from qml_essentials_amd import _native as N  # noqa: E402

SWITCHES = ("QMLE_FORCE_CAND", "QMLE_NO_TOP_FIRST", "QMLE_PAD_HIGH")  # what a compile reads from the environment
N_CANDIDATES, CANDIDATES_PER_VARIANT, N_VARIANTS = 60, 12, 5
ROUTE_BATCHES = (1, 6, 64)


class Case:
    """`make()` -> (ops, n_qubits, n_slots, consts or None, flags); `env`: the switches set around the compile."""

    def __init__(self, name, make, env=None):
        self.name, self.make, self.env = name, make, dict(env or {})


def _he(n, flags=0):
    def make():
        from tests.test_abi_cpu import he_layer_ops

        ops, slots = he_layer_ops(n)
        return ops, n, slots, None, flags
    return make


def _fuzz(seed, n, flags):
    def make():
        from tests.test_measure_in_registers_cpu import fuzz_struct, to_native

        ops, slots = to_native(fuzz_struct(seed, n))
        return ops, n, slots, None, flags
    return make


def _random(n, seed):
    """helpers.random_tape with a constant 2x2 and a constant 4x4 in it, and one DIAG_ALL entry where the marks are
    cheap to come by (the real ruler at n = 5, a blob of zeros at 9, 14 and 18: a plan does not look at the marks; past
    the whole-state limit the entry is a stage of its own)."""
    def make():
        import helpers

        rng = np.random.default_rng(4000 + 100 * n + seed)
        tape = helpers.random_tape(n, 60, rng)
        eye2, eye4 = np.eye(2, dtype=np.complex64), np.eye(4, dtype=np.complex64)
        tape.insert(20, ("Matrix", [int(rng.integers(n))], (eye2,)))
        tape.insert(40, ("Matrix", [int(w) for w in rng.choice(n, 2, replace=False)], (eye4,)))
        if n == 5:
            tape.insert(30, ("Golomb", [], (0.37,)))
        ops, angles, consts = helpers.tape_to_native(tape, n)
        slots = len(angles)
        if n in (9, 14, 18):
            off = len(consts)
            consts = np.concatenate([consts, np.zeros(1 << n, dtype=np.float32)])
            ops.insert(30, ("DIAG_ALL", [], [slots], off))
            slots += 1
        return ops, n, slots, consts, 0
    return make


def _noisy(case, flags=0):
    """A doubled tape of tests/noise_reference.py, lowered the way tests/test_noise_reference_cpu.py lowers it."""
    def make():
        import noise_reference as R
        from qml_essentials_amd import simulation

        tape = R.route_tape(*case).without_wide_channels()
        low = simulation.LoweredTape(simulation.doubled_tape(tape.ops, tape.n), 2 * tape.n)
        return low.ops, 2 * tape.n, low.n_slots, (low.consts if len(low.consts) else None), flags
    return make


def _tape(ops, n, slots=0, consts=None, flags=0):
    return lambda: (ops, n, slots, consts, flags)


def _unmergeable(count):
    return lambda: ([("CX", [k % 3, k % 3 + 1], [], -1) for k in range(count)], 4, 0, None, 0)


def _invalid_cases():
    mat1 = np.zeros(8, dtype=np.float32)
    good = ("RX", [0], [0], -1)
    bad = {
        "unknown_op": (99, [0], [], -1),
        "wire_count": ("CX", [0], [], -1),
        "wire_range": ("RX", [5], [0], -1),
        "duplicate_wires": ("CX", [1, 1], [], -1),
        "slot_range": ("RX", [0], [7], -1),
        "const_range": ("MAT1", [0], [], 4),
        "diag_all_range": ("DIAG_ALL", [], [0], 0),
    }
    out = [Case("invalid-" + k, _tape([good, op], 4, 1, mat1)) for k, op in bad.items()]
    out.append(Case("invalid-no_qubits", _tape([], 0)))
    out.append(Case("invalid-too_many_qubits", _tape([good], 33, 1)))
    out.append(Case("invalid-tile_bits_3", _he(16, N.plan_flags(tile_bits=3))))
    for a, b in (("wire_count", "slot_range"), ("unknown_op", "duplicate_wires"), ("wire_range", "const_range")):
        out.append(Case(f"invalid-{a}-then-{b}", _tape([good, bad[a], bad[b]], 4, 1, mat1)))
        out.append(Case(f"invalid-{b}-then-{a}", _tape([good, bad[b], bad[a]], 4, 1, mat1)))
    return out


def cases():
    from tests.test_measure_in_registers_cpu import ALL_LIVE, FUZZ_SEEDS
    import noise_reference as R

    out = []
    he_flags = {"default": 0, "all_live": ALL_LIVE, "no_fusion": N.PLAN_NO_FUSION, "force_tile": N.PLAN_FORCE_TILE,
                "force_global": N.PLAN_FORCE_GLOBAL, "no_regtile": N.PLAN_NO_REGTILE, "no_merge": N.PLAN_NO_MERGE,
                "tape_order": N.PLAN_TAPE_ORDER}
    for n in (4, 10, 13, 14, 15, 16, 20, 23, 24, 26, 28):  # (15: just past the whole-state limit)
        for tag, flags in he_flags.items():
            out.append(Case(f"he-{n}-{tag}", _he(n, flags)))
        for tile_bits in (12, 13):
            for low_bits in (4, 7):
                out.append(Case(f"he-{n}-T{tile_bits}-L{low_bits}", _he(n, N.plan_flags(tile_bits=tile_bits, low_bits=low_bits))))
    for n in (12, 16, 24):
        for seed in FUZZ_SEEDS:
            out.append(Case(f"fuzz-{n}-{seed}-default", _fuzz(seed, n, 0)))
            out.append(Case(f"fuzz-{n}-{seed}-all_live", _fuzz(seed, n, ALL_LIVE)))
    for n in (5, 9, 14, 18, 24):
        for seed in range(10):
            out.append(Case(f"random-{n}-{seed}", _random(n, seed)))
    for case in R.ENGINE_CASES + R.WIDE_CASES:
        out.append(Case("noisy-" + "-".join(map(str, case)), _noisy(case)))
    for case in R.ENGINE_CASES[3:5]:  # (16 and 18 doubled wires: several tile stages)
        out.append(Case("noisy-" + "-".join(map(str, case)) + "-all_live", _noisy(case, ALL_LIVE)))
    for n in (24, 20):
        for tag, flags in (("all_live", ALL_LIVE), ("default", 0)):
            for k in range(N_CANDIDATES):
                out.append(Case(f"cand-{n}-{tag}-{k}", _he(n, flags), {"QMLE_FORCE_CAND": str(k)}))
            out.append(Case(f"cand-{n}-{tag}-no_top_first", _he(n, flags), {"QMLE_NO_TOP_FIRST": "1"}))
            for pad in (1, 2, 9):
                out.append(Case(f"cand-{n}-{tag}-pad_high-{pad}", _he(n, flags), {"QMLE_PAD_HIGH": str(pad)}))
    out.append(Case("edge-empty", _tape([], 4)))
    out.append(Case("edge-identities", _tape([("Id", [w], [], -1) for w in range(4)], 4)))
    out.append(Case("edge-16384-operators", _unmergeable(16384)))
    out.append(Case("edge-16385-operators", _unmergeable(16385)))
    return out + _invalid_cases()


def _describe_text(plan):
    L = N.lib()
    need = L.qmle_plan_describe(plan._h, None, 0)
    buf = C.create_string_buffer(need + 1)
    L.qmle_plan_describe(plan._h, buf, need + 1)
    return buf.value.decode()


def _route_text(plan, stage, batch, meas, n_obs, flags):
    buf = C.create_string_buffer(1024)
    rc = N.lib().qmle_plan_tile_route(plan._h, stage, batch, meas, n_obs, flags, buf, 1024)
    return buf.value.decode() if rc >= 0 else "status %d" % rc


def compile_text(case):
    """-> (status, texts): 0 and the texts the digest is taken over (the descriptions first: top plan, then one per
    measurement), or the error code of qmle_plan_create and no text."""
    ops, n, slots, consts, flags = case.make()
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(case.env)
    try:
        try:
            top = N.Plan(ops, n, slots, consts, flags)
        except (ValueError, RuntimeError, NotImplementedError) as e:
            m = re.search(r"qmle status (-?\d+)", str(e))
            if not m:
                raise
            return int(m.group(1)), []
        texts = [_describe_text(top)] + [_describe_text(top.executed(m)) for m in N.MEAS]
        ex = top.executed("expval")
        stages = json.loads(_describe_text(ex))["stages"]
        P = N.Plan
        for si, st in enumerate(stages):
            if st["kind"] != "tile":
                continue
            last = si + 1 == len(stages)
            for batch in ROUTE_BATCHES:
                texts.append(_route_text(ex, si, batch, P.TM_EXPVAL_PARTIAL if last else P.TM_STORE, n if last else 0,
                                         P.ROUTE_FROM_ZERO | P.ROUTE_MULTI_ROWS))
        return 0, texts
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def descriptions(texts):
    """The plan descriptions among a case's texts, the folded <Z> child of each among them."""
    out = []
    for t in texts[:1 + len(N.MEAS)]:
        d = json.loads(t)
        out.append(d)
        if "expval_plan" in d:
            out.append(d["expval_plan"])
    return out


def _fast_groups(d):
    return [g for s in d["stages"] for g in s.get("fast_groups", [])]


BRANCHES = {
    "a direct stage": lambda d: any(s["kind"] == "direct" for s in d["stages"]),
    "a diag_all stage": lambda d: any(s["kind"] == "diag_all" for s in d["stages"]),
    "a stage with shift > 0": lambda d: any(s["shift"] > 0 for s in d["stages"]),
    "product: true": lambda d: any(s["product"] for s in d["stages"]),
    "a 12-bit last tile under a 13-bit schedule": lambda d: (d["tile_bits"] == 13 and len(d["stages"]) > 1
                                                            and d["stages"][-1]["kind"] == "tile"
                                                            and d["stages"][-1]["T"] == 12),
    "lane swap, straight": lambda d: any(s["last_group_lane_swap"] and not s["lane_swap_crossed"] for s in d["stages"]),
    "lane swap, crossed": lambda d: any(s["last_group_lane_swap"] and s["lane_swap_crossed"] for s in d["stages"]),
    "staging: dma": lambda d: any(s.get("staging") == "dma" for s in d["stages"]),
    "staging: registers": lambda d: any(s.get("staging") == "registers" for s in d["stages"]),
    "a non-empty measure_after": lambda d: any(s.get("measure_after") for s in d["stages"]),
    "relayout: 1": lambda d: any(g["relayout"] == 1 for g in _fast_groups(d)),
    "a non-empty unit_form_ops": lambda d: any(s.get("unit_form_ops") for s in d["stages"]),
    "a product-form group": lambda d: any(any(s.get("product_form_groups", [])) for s in d["stages"]),
    "whole_state_lds": lambda d: d["whole_state_lds"],
}
for _v in range(N_VARIANTS):
    BRANCHES["a chosen candidate of variant %d" % _v] = (
        lambda d, v=_v: d["candidate"] >= 0 and d["candidate"] // CANDIDATES_PER_VARIANT == v)


def missing_branches(all_descriptions):
    """The compiler branches (BRANCHES) that none of the descriptions shows."""
    left = dict(BRANCHES)
    for d in all_descriptions:
        for name in [k for k, seen in left.items() if seen(d)]:
            del left[name]
        if not left:
            break
    return sorted(left)


def main(argv):
    out = sys.stdout
    if "--lib" in argv:
        N.LIB_PATH = os.path.abspath(argv[argv.index("--lib") + 1])
    if "--out" in argv:
        out = open(argv[argv.index("--out") + 1], "w")
    total, seen, statuses = hashlib.sha256(), [], set()
    for case in cases():
        status, texts = compile_text(case)
        statuses.add(status)
        seen += descriptions(texts)
        line = "%s %d %s\n" % (case.name, status, hashlib.sha256("".join(texts).encode()).hexdigest())
        total.update(line.encode())
        out.write(line)
    out.write("corpus %s\n" % total.hexdigest())
    out.flush()
    missing = missing_branches(seen)
    assert not missing, "the corpus does not reach: " + "; ".join(missing)
    assert {-1, -2, -3, -4, -5, -11} <= statuses, statuses


if __name__ == "__main__":
    main(sys.argv[1:])
