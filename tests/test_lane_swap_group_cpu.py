"""Plan-compiler side of "the measuring walk's last gate group through lane swaps" (k_tile2's register-measuring
instantiations), no GPU.

Where the last group of a wave-private DMA walk holds only uncontrolled 1-qubit ops on the two positions that are lane
bits 4 and 5 of the group in front of it, the kernel runs both groups on one gather: behind the first group's ops it
trades in-thread bit 2 and in-thread bit 3 of a work item's 16 amplitudes for those two lane bits with
v_permlane16_swap / v_permlane32_swap and applies the last group's ops where the amplitudes then are.  The X / CX that
the table form applies to the layout between the two groups move behind the ops (`measure_between`, then
`measure_after`), and the measurement reads a second set of records, `measure_records_swap`.

This file models the two instructions in NumPy, builds the index every (wave, lane, register) holds from the report of
the group in front of the last, swaps, applies the X / CX in tape order and asks of the records what
tests/test_measure_in_registers_cpu.py::check_records asks of the table form's."""
import numpy as np
import pytest

from qml_essentials_amd import _native as N
from tests.test_abi_cpu import he_layer_ops
from tests.test_measure_in_registers_cpu import ALL_LIVE, FUZZ_SEEDS, N_PARAMS, check_records, fuzz_struct, to_native
from tests.test_wave_private_walk_cpu import touched_later_struct

U32 = np.uint32


def permlane32_swap(a, b):
    """v_permlane32_swap_b32 on two registers [.., 64 lanes]: lanes 32..63 of the first trade with lanes 0..31 of the
    second."""
    a, b = a.copy(), b.copy()
    hi = a[..., 32:].copy()
    a[..., 32:] = b[..., :32]
    b[..., :32] = hi
    return a, b


def permlane16_swap(a, b):
    """v_permlane16_swap_b32: the odd 16-lane rows of the first trade with the even rows of the second."""
    a, b = a.copy(), b.copy()
    for row in (0, 2):
        odd = a[..., 16 * (row + 1):16 * (row + 2)].copy()
        a[..., 16 * (row + 1):16 * (row + 2)] = b[..., 16 * row:16 * (row + 1)]
        b[..., 16 * row:16 * (row + 1)] = odd
    return a, b


def test_the_models_trade_one_register_bit_for_one_lane_bit():
    lane = np.arange(64, dtype=U32)
    a, b = lane | U32(0 << 8), lane | U32(1 << 8)  # value = lane it came from | register it came from << 8
    for swap, bit in ((permlane16_swap, 4), (permlane32_swap, 5)):
        x, y = swap(a, b)
        for reg, out in enumerate((x, y)):
            src_lane, src_reg = out & U32(63), out >> U32(8)
            # what sits in (reg, lane) came from (lane bit, reg): the two bits traded, every other lane bit in place
            assert np.array_equal(src_reg, (lane >> U32(bit)) & U32(1))
            assert np.array_equal((src_lane >> U32(bit)) & U32(1), np.full(64, reg, dtype=U32))
            assert np.array_equal(src_lane & ~U32(1 << bit), lane & ~U32(1 << bit))


def held_indices(st):
    """Index (in the frame of the group in front of the last) of amplitude c of lane l of wave w, shaped [w, c, l],
    behind the kernel's swaps."""
    T = st["T"]
    prev = st["fast_groups"][-2]
    nw = 1 << (T - 10)
    w = np.arange(nw, dtype=U32)[:, None, None]
    c = np.arange(16, dtype=U32)[None, :, None]
    lane = np.arange(64, dtype=U32)[None, None, :]
    tid = lane | (w << U32(6))
    e = np.zeros((nw, 16, 64), dtype=U32)
    for k, pos in enumerate(prev["thread_bits"]):
        e |= ((tid >> U32(k)) & U32(1)) << U32(pos)
    for i, pos in enumerate(prev["bits"]):
        e |= ((c >> U32(i)) & U32(1)) << U32(pos)
    # swap_lanes_45 (qmle_tile.hip): the row swap on the pairs of in-thread bit 2 and the half swap on those of bit 3
    # -- crossed: the other way round
    row_bit, half_bit = (3, 2) if st["lane_swap_crossed"] else (2, 3)
    for bit, swap in ((2, permlane16_swap if row_bit == 2 else permlane32_swap),
                      (3, permlane16_swap if row_bit == 3 else permlane32_swap)):
        assert bit in (row_bit, half_bit)
        for q in range(16):
            if not q & (1 << bit):
                e[:, q], e[:, q | (1 << bit)] = swap(e[:, q], e[:, q | (1 << bit)])
    return e


def parity(x):
    x = x.copy()
    for s in (16, 8, 4, 2, 1):
        x ^= x >> U32(s)
    return x & U32(1)


def check_swap_records(st):
    """The swap-form records of a stage that takes the form, on every amplitude the workgroup holds."""
    T = st["T"]
    assert st["last_group_lane_swap"] and st["staging"] == "dma" and st["wave_private_walk"]
    groups = st["fast_groups"]
    assert len(groups) >= 2
    prev, last = groups[-2], groups[-1]
    sb, stb = st["measure_swap_bits"], st["measure_swap_thread_bits"]
    assert len(sb) == 4 and len(stb) == T - 4 and sorted(sb + stb) == list(range(T))
    e = held_indices(st)
    assert np.array_equal(np.sort(e.ravel()), np.arange(1 << T, dtype=U32)), "the swaps permute the tile"
    # the frame the report names is the frame the swaps give
    nw = 1 << (T - 10)
    w = np.arange(nw, dtype=U32)[:, None, None]
    c = np.arange(16, dtype=U32)[None, :, None]
    lane = np.arange(64, dtype=U32)[None, None, :]
    tid = np.broadcast_to(lane | (w << U32(6)), e.shape)
    named = np.zeros_like(e)
    for k, pos in enumerate(stb):
        named |= ((tid >> U32(k)) & U32(1)) << U32(pos)
    for i, pos in enumerate(sb):
        named |= ((c >> U32(i)) & U32(1)) << U32(pos)
    assert np.array_equal(named, e)
    # the last group's ops find their targets at the in-thread index their dispatch codes carry
    n_last = last["n_ops"]
    members = set()
    for code, _off in st["fast_ops"][-n_last:]:
        assert code < 4 or 16 <= code < 20 or 48 <= code < 56, "uncontrolled dense, diagonal, unit-form"
        tb = code & 3
        assert tb in (2, 3) and sb[tb] == last["bits"][tb], (code, sb, last["bits"])
        members.add(sb[tb])
    assert members <= {prev["thread_bits"][4], prev["thread_bits"][5]}
    # X / CX between the two groups, then those behind the last, in tape order
    f = e.copy()
    for cc, t in st["measure_between"]:
        assert cc not in members and t not in members, "they commute with the last group's ops"
    for cc, t in st["measure_between"] + st["measure_after"]:
        assert 0 <= t < T and -1 <= cc < T
        f ^= U32(1 << t) if cc < 0 else ((f >> U32(cc)) & U32(1)) << U32(t)
    cidx = np.broadcast_to(c, e.shape)
    assert len(st["measure_records_swap"]) == T
    for j, (wht, lm, wm, neg) in enumerate(st["measure_records_swap"]):
        assert 0 <= wht < 16 and 0 <= lm < 64 and 0 <= wm < nw and neg in (0, 1)
        got = parity(cidx & U32(wht)) ^ parity(tid & U32(lm | (wm << 6))) ^ U32(neg)
        assert np.array_equal(got, (f >> U32(j)) & U32(1)), (j, st["measure_records_swap"][j])
    check_records(st)  # the table form's stay right: known-zero walks take them


def executed_last(ops, slots, n, flags=ALL_LIVE):
    return N.Plan(ops, n, slots, flags=flags).executed("expval").describe()["stages"][-1]


# What the parent commit reports for the last stage of the headline layers under all-live flags (its `fast_groups`,
# `fast_ops`, `measure_records`, and the plan's `mat_floats`): the swap form adds to the report and changes none of it.
PARENT = {23: {'fast_groups': [{'bits': [0, 1, 2, 3],
                       'layout_cols': [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048],
                       'layout_const': 0,
                       'n_ops': 4,
                       'relayout': 0,
                       'sync_before': False,
                       'thread_bits': [5, 6, 7, 4, 8, 9, 10, 11]},
                      {'bits': [4, 5, 6, 7],
                       'layout_cols': [1, 3, 6, 8, 16, 32, 64, 128, 256, 512, 1024, 2048],
                       'layout_const': 0,
                       'n_ops': 4,
                       'relayout': 0,
                       'sync_before': False,
                       'thread_bits': [0, 1, 2, 3, 8, 9, 10, 11]},
                      {'bits': [5, 6, 7, 8],
                       'layout_cols': [1, 3, 6, 14, 24, 56, 96, 128, 256, 512, 1024, 2048],
                       'layout_const': 0,
                       'n_ops': 1,
                       'relayout': 1,
                       'sync_before': False,
                       'thread_bits': [0, 1, 2, 3, 4, 9, 10, 11]}],
      'fast_ops': [[48, 368], [49, 376], [50, 384], [51, 392], [48, 400], [49, 408], [50, 416], [51, 424], [3, 432]],
      'mat_floats': 440,
      'measure_records': [[0, 1, 0, 0], [0, 2, 0, 0], [0, 4, 0, 0], [0, 8, 0, 0], [0, 16, 0, 0], [1, 0, 0, 0],
                          [14, 0, 0, 0], [12, 0, 0, 0], [8, 32, 0, 0], [0, 32, 0, 0], [0, 0, 1, 0], [0, 1, 2, 0]]},
 24: {'fast_groups': [{'bits': [0, 1, 2, 3],
                       'layout_cols': [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048],
                       'layout_const': 0,
                       'n_ops': 4,
                       'relayout': 0,
                       'sync_before': False,
                       'thread_bits': [5, 6, 7, 4, 8, 9, 10, 11]},
                      {'bits': [4, 5, 6, 7],
                       'layout_cols': [1, 3, 7, 12, 16, 32, 64, 128, 256, 512, 1024, 2048],
                       'layout_const': 0,
                       'n_ops': 4,
                       'relayout': 0,
                       'sync_before': False,
                       'thread_bits': [0, 1, 2, 3, 8, 9, 10, 11]},
                      {'bits': [5, 6, 8, 9],
                       'layout_cols': [1, 3, 7, 12, 28, 48, 112, 192, 256, 512, 1024, 2048],
                       'layout_const': 0,
                       'n_ops': 2,
                       'relayout': 1,
                       'sync_before': False,
                       'thread_bits': [0, 1, 2, 3, 4, 7, 10, 11]}],
      'fast_ops': [[48, 384], [49, 392], [50, 400], [51, 408], [48, 416], [49, 424], [50, 432], [51, 440], [50, 448],
                   [3, 456]],
      'mat_floats': 464,
      'measure_records': [[0, 1, 0, 0], [0, 2, 0, 0], [0, 4, 0, 0], [0, 8, 0, 0], [0, 16, 0, 0], [1, 0, 0, 0],
                          [2, 0, 0, 0], [12, 32, 0, 0], [12, 0, 0, 0], [8, 0, 1, 0], [0, 0, 1, 0], [0, 1, 2, 0]]}}


@pytest.mark.parametrize("n", [23, 24])
def test_headline_layers_take_the_form_and_keep_the_table_form_as_it_was(n):
    ops, slots = he_layer_ops(n)
    desc = N.Plan(ops, n, slots, flags=ALL_LIVE).executed("expval").describe()
    st = desc["stages"][-1]
    assert st["last_group_lane_swap"] is True
    assert desc["mat_floats"] == PARENT[n]["mat_floats"]
    for key in ("fast_ops", "fast_groups", "measure_records"):
        assert st[key] == PARENT[n][key], key
    # 24 qubits: in-thread bit 2 <-> lane bit 4, bit 3 <-> lane bit 5; the one op of the 23-qubit layer's last group sits
    # at in-thread index 3 on lane bit 4: crossed
    assert st["lane_swap_crossed"] is (n == 23)
    prev = st["fast_groups"][-2]
    assert prev["bits"] == [4, 5, 6, 7] and prev["thread_bits"][4:6] == [8, 9]
    assert st["measure_swap_bits"] == ([4, 5, 9, 8] if n == 23 else [4, 5, 8, 9])
    assert all(max(c, t) <= 7 for c, t in st["measure_between"]) and st["measure_between"], "CX below the targets only"
    check_swap_records(st)
    assert all("last_group_lane_swap_last_run" not in s for s in desc["stages"][:-1])
    assert st["last_group_lane_swap_last_run"] is False, "nothing has run"


@pytest.mark.parametrize("n", [16, 17, 20, 22])
def test_a_last_group_on_wave_index_positions_keeps_the_table_form(n):
    ops, slots = he_layer_ops(n)
    st = executed_last(ops, slots, n)
    assert st["register_measure_qualifies"] and not st["wave_private_walk"]
    assert st["last_group_lane_swap"] is False and "measure_records_swap" not in st


def test_a_one_group_last_pass_keeps_the_table_form(monkeypatch):
    """The low-first schedule of the headline (bench.py's k2_three_pass leg): its measuring pass is one group."""
    monkeypatch.setenv("QMLE_NO_TOP_FIRST", "1")
    ops, slots = he_layer_ops(24)
    st = executed_last(ops, slots, 24)
    assert st["register_measure_qualifies"] and len(st["fast_groups"]) == 1
    assert st["last_group_lane_swap"] is False


@pytest.mark.parametrize("name", ["target_rotated", "x_read_by_a_cx_whose_target_rotates"])
def test_a_stage_with_a_barrier_mark_keeps_the_table_form(name):
    ops, slots = to_native(touched_later_struct(name))
    st = executed_last(ops, slots, 23)
    assert st["register_measure_qualifies"] and len(st["fast_groups"]) >= 2
    assert any(g["sync_before"] for g in st["fast_groups"]) or st["sync_tile_end"]
    assert st["last_group_lane_swap"] is False


def test_known_zeros_inside_the_tile_keep_the_table_form():
    """Default flags: the walk zero-fills and loads selectively -- no DMA staging, so no swap form either."""
    n = 18
    struct = ([("RX", [w]) for w in range(n)] + [("CX", [w, w + 1]) for w in range(0, n - 1, 2)]
              + [("RY", [w]) for w in range(n)])
    ops, slots = to_native(struct)
    st = N.Plan(ops, n, slots, flags=0).executed("expval").describe()["stages"][-1]
    assert st["staging"] == "registers" and st["last_group_lane_swap"] is False


# ---- hand-built tapes --------------------------------------------------------------------------------------------------
# No tape of FUZZ_SEEDS takes the form at 16 qubits in 10- or 12-bit tiles (asserted below): a forced tile geometry
# schedules from the low positions up, and a random tape does not leave its last stage with a group on four
# positions followed by uncontrolled gates on exactly that group's lane bits 4 and 5.  These tapes do, under
# PLAN_TAPE_ORDER (the scheduler takes commuting gates in the order given): the top positions first, so that they fill the
# earlier stages; then, behind a rotation on position 7 that no earlier tile holds, controlled phases from 7 onto 4, 5
# and 6 and a rotation on each -- the group {4, 5, 6, 7}, whose lane bits 4 and 5 are positions 8 and 9 --, two CX inside
# that group (`between`), the last group's gates on 8 and / or 9, and two CX behind them.  12-bit tiles: position 10
# carries no gate, so that the last tile's wave-index positions 10 and 11 are in no group.
LANE_SWAP_FUZZ_SEEDS = []  # (none of FUZZ_SEEDS: see above)
M_NON_UNITARY = np.array([[0.9 + 0.1j, 0.3 - 0.2j], [-0.25 + 0.15j, 1.05 - 0.05j]])  # a caller's constant matrix
HAND_BUILT = {
    # name: (gates of the last group as (gate, position), crossed)
    "two_dense": ([("Rot", 8), ("Rot", 9)], False),            # a unit-form dense op and the carrier
    "unit_diagonal": ([("RZ", 8), ("Rot", 9)], False),         # a unit-form diagonal op and the carrier
    "carrier_alone": ([("Rot", 9)], False),
    "carrier_alone_on_lane_4": ([("Rot", 8)], True),           # the 23-qubit layer's case: in-thread index 3, lane bit 4
    "two_plain_dense": ([("MAT1", 8), ("MAT1", 9)], False),    # not from the unitary gate set: no unit form, no carrier
}


def hand_built(name, tile_bits, between=(("CX", 5, 4), ("CX", 7, 6)), n=16):
    """(struct, ops, n_slots, consts) of a hand-built tape; struct entries are (gate, wires), wire = n - 1 - position."""
    def P(pos):
        return n - 1 - pos

    top = list(range(15, 9 if tile_bits == 10 else 10, -1))
    t = [("Rot", [P(p)]) for p in top + [0, 1, 2, 3, 4, 5, 6]]
    t += [("CZ", [P(p), P(i % 4)]) for i, p in enumerate(top)] + [("CX", [P(3), P(4)]), ("CX", [P(2), P(5)])]
    t += [("Rot", [P(7)]), ("CZ", [P(7), P(4)]), ("CZ", [P(7), P(5)]), ("CZ", [P(7), P(6)])]
    t += [("RY", [P(p)]) for p in (4, 5, 6, 7)]
    t += [(g, [P(c), P(tt)]) for g, c, tt in between]
    t += [(g, [P(pos)]) for g, pos in HAND_BUILT[name][0]]
    t += [("CX", [P(9), P(8)]), ("CX", [P(8), P(7)])]
    ops, k = [], 0
    consts = np.stack([M_NON_UNITARY.real, M_NON_UNITARY.imag], axis=-1).reshape(-1).astype(np.float32)
    for g, wires in t:
        if g == "MAT1":
            ops.append(("MAT1", list(wires), [], 0))
        else:
            npar = N_PARAMS.get(g, 0)
            ops.append((g, list(wires), list(range(k, k + npar)), -1))
            k += npar
    return t, ops, k, consts


def hand_built_plan(name, tile_bits, **kw):
    _t, ops, slots, consts = hand_built(name, tile_bits, **kw)
    return N.Plan(ops, 16, slots, consts=consts, flags=ALL_LIVE | N.PLAN_TAPE_ORDER | N.plan_flags(tile_bits=tile_bits))


@pytest.mark.parametrize("tile_bits", [10, 12])
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_tapes(seed, tile_bits):
    n = 16
    ops, slots = to_native(fuzz_struct(seed, n))
    desc = N.Plan(ops, n, slots, flags=ALL_LIVE | N.plan_flags(tile_bits=tile_bits)).describe()
    took = 0
    for st in desc["stages"]:
        if st["last_group_lane_swap"]:
            check_swap_records(st)
            took += 1
        else:
            assert "measure_records_swap" not in st
    assert (took == 1) == (seed in LANE_SWAP_FUZZ_SEEDS), (seed, tile_bits, took)


@pytest.mark.parametrize("tile_bits", [10, 12])
@pytest.mark.parametrize("name", sorted(HAND_BUILT))
def test_hand_built_tapes_take_the_form(name, tile_bits):
    st = hand_built_plan(name, tile_bits).executed("expval").describe()["stages"][-1]
    assert st["T"] == tile_bits and st["last_group_lane_swap"] is True
    assert st["lane_swap_crossed"] is HAND_BUILT[name][1]
    assert [g["bits"] for g in st["fast_groups"]][-2] == [4, 5, 6, 7] and len(st["fast_groups"]) == 2
    assert st["measure_between"] == [[5, 4], [7, 6]] and st["measure_after"] == [[9, 8], [8, 7]]
    n_last = st["fast_groups"][-1]["n_ops"]
    codes = [c for c, _o in st["fast_ops"][-n_last:]]
    want = {"two_dense": [50, 3], "unit_diagonal": [54, 3], "carrier_alone": [3], "carrier_alone_on_lane_4": [3],
            "two_plain_dense": [2, 3]}[name]
    assert codes == want, codes
    n_all = len(st["fast_ops"])
    carriers = st["scale_carriers"]
    assert (carriers == [n_all - 1]) == (name != "two_plain_dense"), carriers
    check_swap_records(st)


@pytest.mark.parametrize("tile_bits", [10, 12])
def test_a_cx_between_the_groups_that_touches_a_target_keeps_the_table_form(tile_bits):
    """CX 7 -> 8 in place of CX 7 -> 6: applied to the layout in front of the last group, it does not commute with the
    rotation on 8.  Same groups, same ops."""
    good = hand_built_plan("two_dense", tile_bits).executed("expval").describe()["stages"][-1]
    bad = hand_built_plan("two_dense", tile_bits, between=(("CX", 5, 4), ("CX", 7, 8))).executed("expval").describe()["stages"][-1]
    assert [g["bits"] for g in bad["fast_groups"]] == [g["bits"] for g in good["fast_groups"]]
    assert [c for c, _o in bad["fast_ops"]] == [c for c, _o in good["fast_ops"]]
    assert bad["wave_private_walk"] and bad["staging"] == "dma"
    assert good["last_group_lane_swap"] is True and bad["last_group_lane_swap"] is False
    check_records(bad)
