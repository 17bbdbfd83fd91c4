"""Plan-compiler side of "<Z> from the last gate group's registers" (k_tile2's multi-tile measuring walk), no GPU:
which stages are marked, and that the per-position records -- Walsh-Hadamard index over the four in-thread bits, lane
mask, wave mask, sign -- reproduce the layout map behind the last group: the X / CX peeled off it, applied here to
every local index of the tile."""
import numpy as np
import pytest

from qml_essentials_amd import _native as N

N_PARAMS = {"RX": 1, "RY": 1, "RZ": 1, "Rot": 3, "CRX": 1}
FUZZ_GATES = ["RX", "RY", "RZ", "Rot", "CX", "CZ", "PauliX", "CRX"]
ALL_LIVE = N.PLAN_NO_SPARSE | N.PLAN_NO_ABSORB
# Seeds of fuzz_struct at 16 qubits whose plans end in a fast tile stage under 10- and 12-bit tiles, and whose executed
# plan under the default geometry ends in a 12-bit tile stage measured by k_tile2 (a tape whose last gate lands in a
# one-gate direct pass, or whose last stage is one small register group, is measured by another kernel; a 13-bit last
# tile leaves too few tiles for the walk at the batch the GPU tests use); the tests assert that, so a change of the scheduler that breaks it shows up as a failure, not as a pass on another path.
FUZZ_SEEDS = [2, 3, 13, 14, 16, 19, 20, 26, 31, 35, 39, 42, 45, 48, 51, 57, 59, 60, 65, 66, 70, 72, 73, 74]


def to_native(struct):
    """[(name, wires)] -> (ops, n_slots): every parameter gets an angle slot of its own."""
    ops, k = [], 0
    for name, wires in struct:
        p = N_PARAMS.get(name, 0)
        ops.append((name, list(wires), list(range(k, k + p)), -1))
        k += p
    return ops, k


def fuzz_struct(seed, n, n_gates=48):
    """A seeded random tape over RX / RY / RZ / Rot / CX / CZ / X / CRX; a rotation on every wire first, so that no
    wire stays in |0>."""
    rng = np.random.default_rng(9000 + seed)
    struct = [("Rot", [w]) for w in range(n)]
    for _ in range(n_gates):
        name = FUZZ_GATES[int(rng.integers(len(FUZZ_GATES)))]
        k = 2 if name in ("CX", "CZ", "CRX") else 1
        struct.append((name, [int(w) for w in rng.choice(n, k, replace=False)]))
    return struct


def expected_mark(desc, si, sparse):
    """Part of the contract: the LAST stage of a plan of several, run by the fast tile kernel (its gate groups are
    Group2 groups), whose input has no known-zero tiles."""
    st = desc["stages"][si]
    if st["kind"] != "tile" or not st["fast"] or si == 0 or si + 1 != len(desc["stages"]):
        return False
    if sparse:
        outer = set(range(desc["n_qubits"])) - set(st["bits"])
        if any((st["zero_in"] >> p) & 1 for p in outer):
            return False
    return True


def check_records(st):
    """The records of a marked stage against the X / CX behind its last group, on all 2^T local indices."""
    T = st["T"]
    gb, tb = st["measure_group_bits"], st["measure_thread_bits"]
    assert len(gb) == 4 and len(tb) == T - 4
    assert sorted(gb + tb) == list(range(T)), "in-thread and thread bits together are the tile's positions"
    e = np.arange(1 << T, dtype=np.uint32)
    f = e.copy()  # logical index behind the group: the peeled-off gates in order
    for c, t in st["measure_after"]:
        assert 0 <= t < T and -1 <= c < T
        f ^= np.uint32(1 << t) if c < 0 else ((f >> np.uint32(c)) & np.uint32(1)) << np.uint32(t)
    cidx = np.zeros_like(e)  # which of its 16 amplitudes, which work item
    for i, b in enumerate(gb):
        cidx |= ((e >> np.uint32(b)) & np.uint32(1)) << np.uint32(i)
    tid = np.zeros_like(e)
    for k, b in enumerate(tb):
        tid |= ((e >> np.uint32(b)) & np.uint32(1)) << np.uint32(k)

    def parity(x):
        x = x.copy()
        for s in (16, 8, 4, 2, 1):
            x ^= x >> np.uint32(s)
        return x & np.uint32(1)

    assert len(st["measure_records"]) == T
    for j, (wht, lane, wave, neg) in enumerate(st["measure_records"]):
        assert 0 <= wht < 16 and 0 <= lane < 64 and 0 <= wave < (1 << max(T - 10, 0)) and neg in (0, 1)
        got = parity(cidx & np.uint32(wht)) ^ parity(tid & np.uint32(lane | (wave << 6))) ^ np.uint32(neg)
        assert np.array_equal(got, (f >> np.uint32(j)) & np.uint32(1)), (j, st["measure_records"][j])


@pytest.mark.parametrize("tile_bits", [10, 12])
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_records_reproduce_the_layout_behind_the_last_group(seed, tile_bits):
    n = 16
    ops, slots = to_native(fuzz_struct(seed, n))
    plan = N.Plan(ops, n, slots, flags=ALL_LIVE | N.plan_flags(tile_bits=tile_bits))
    desc = plan.describe()
    marked = 0
    for si, st in enumerate(desc["stages"]):
        assert st["register_measure_qualifies"] == expected_mark(desc, si, sparse=False), (si, st["kind"], st["fast"])
        if st["register_measure_qualifies"]:
            assert st["T"] == tile_bits
            check_records(st)
            marked += 1
        else:
            assert "measure_records" not in st
    assert marked == 1, [(s["kind"], s["T"], s["fast"]) for s in desc["stages"]]


def test_hardware_efficient_ring_keeps_its_wrap_around_cx_behind_the_group():
    """The headline's layer: the last stage is one group, the CX ring -- the wrap-around CX onto the tile's top
    position included -- sits behind it, and a position's <Z> becomes a parity over in-thread, lane and wave bits."""
    from tests.test_abi_cpu import he_layer_ops

    for n in (16, 17, 24):
        ops, slots = he_layer_ops(n)
        desc = N.Plan(ops, n, slots, flags=ALL_LIVE).describe()
        for si, st in enumerate(desc["stages"]):
            assert st["register_measure_qualifies"] == expected_mark(desc, si, sparse=False)
        last = desc["stages"][-1]
        assert last["register_measure_qualifies"] and len(last["fast_groups"]) == 1
        T = last["T"]
        assert any(c >= 0 and t == T - 1 for c, t in last["measure_after"]), last["measure_after"]
        kinds = set()
        for wht, lane, wave, _neg in last["measure_records"]:
            kinds |= {"thread" if wht else None, "lane" if lane else None, "wave" if wave else None}
            assert wht or lane or wave
        assert {"thread", "lane", "wave"} <= kinds
        assert any(bin(wht).count("1") + bin(lane).count("1") + bin(wave).count("1") > 1
                   for wht, lane, wave, _ in last["measure_records"]), "a folded CX makes a parity of several bits"
        check_records(last)


def test_trailing_x_flips_the_sign_of_its_position():
    from tests.test_abi_cpu import he_layer_ops

    n = 16
    struct = [(name, wires) for name, wires, _s, _c in he_layer_ops(n)[0]]
    struct += [("PauliX", [0]), ("PauliX", [5]), ("PauliX", [n - 1])]
    ops, slots = to_native(struct)
    last = N.Plan(ops, n, slots, flags=ALL_LIVE).describe()["stages"][-1]
    assert last["register_measure_qualifies"]
    assert any(c < 0 for c, _t in last["measure_after"]), last["measure_after"]
    assert any(neg for *_m, neg in last["measure_records"])
    check_records(last)


def test_stages_with_known_zero_tiles_and_single_stage_plans_are_not_marked():
    from tests.test_abi_cpu import he_layer_ops

    for n in (12, 16, 20):
        ops, slots = he_layer_ops(n)
        for flags in (0, N.PLAN_NO_ABSORB, ALL_LIVE):
            desc = N.Plan(ops, n, slots, flags=flags).describe()
            seen = [desc]
            while "expval_plan" in seen[-1]:
                seen.append(seen[-1]["expval_plan"])
            for d in seen:
                for si, st in enumerate(d["stages"]):
                    sparse = not (flags & N.PLAN_NO_SPARSE)
                    assert st["register_measure_qualifies"] == expected_mark(d, si, sparse), (n, flags, si)
                    if st["register_measure_qualifies"]:
                        check_records(st)
                if len(d["stages"]) == 1:
                    assert not d["stages"][0]["register_measure_qualifies"]
