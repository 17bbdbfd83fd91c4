"""Plan-compiler side of the barrier-free measuring walk (k_tile2's register-measuring instantiations), no GPU.

A phase of the walk -- staging the loaded tile, a gate group's gather / gates / in-place scatter -- partitions the tile's
2^T LDS slots among the workgroup's waves.  A workgroup barrier between two consecutive phases is needed exactly when
their partitions differ.  The describe fields of a fast group (its positions, its thread bits, the layout map its tables
were emitted from) are enough to recompute every slot here; the partitions derived from them must agree with the
`sync_before` / `sync_tile_end` / `wave_private_walk` marks the library computed on its own tables."""
import numpy as np
import pytest

from qml_essentials_amd import _native as N
from tests.test_abi_cpu import he_layer_ops
from tests.test_measure_in_registers_cpu import ALL_LIVE, FUZZ_SEEDS, check_records, fuzz_struct, to_native


def sw(e):
    """The XOR swizzle of the tile in LDS (sw() in qmle_dev.h): bits 5..8 onto bits 1..4."""
    return e ^ (((e >> np.uint32(5)) & np.uint32(15)) << np.uint32(1))


def staging_owner(T, load_map):
    """Wave that stages each slot: a lane writes 8 float4 (two slots each)."""
    nt = 1 << (T - 4)
    t = np.arange(nt, dtype=np.uint32)[:, None]
    u = np.arange(8, dtype=np.uint32)[None, :]
    if load_map == "slab":  # lane bits at local bits 1..6, u at 7..9, the wave index on top
        e = (np.uint32(2) * (t & np.uint32(63))) | (u << np.uint32(7)) | ((t >> np.uint32(6)) << np.uint32(10))
    else:  # thread bits at local bits 1..T-4, u on top
        assert load_map == "rows"
        e = (np.uint32(2) * t) | (u << np.uint32(T - 3))
    own = np.full(1 << T, -1, dtype=np.int64)
    wave = np.broadcast_to(t >> np.uint32(6), e.shape)
    own[sw(e)] = wave
    own[sw(e) ^ np.uint32(1)] = wave
    assert (own >= 0).all(), "staging covers the tile"
    return own


def group_owner(T, grp):
    """Wave that gathers (and scatters in place) each slot in one group, from the fields its tables came from."""
    nt = 1 << (T - 4)
    assert sorted(grp["bits"] + grp["thread_bits"]) == list(range(T))
    t = np.arange(nt, dtype=np.uint32)[:, None]
    c = np.arange(16, dtype=np.uint32)[None, :]
    e = np.zeros((nt, 16), dtype=np.uint32)
    for k, pos in enumerate(grp["thread_bits"]):
        e |= ((t >> np.uint32(k)) & np.uint32(1)) << np.uint32(pos)
    for i, pos in enumerate(grp["bits"]):
        e |= ((c >> np.uint32(i)) & np.uint32(1)) << np.uint32(pos)
    slot = np.full((nt, 16), grp["layout_const"], dtype=np.uint32)
    for j, col in enumerate(grp["layout_cols"]):
        slot ^= ((e >> np.uint32(j)) & np.uint32(1)) * np.uint32(col)
    own = np.full(1 << T, -1, dtype=np.int64)
    own[sw(slot)] = np.broadcast_to(t >> np.uint32(6), slot.shape)
    assert (own >= 0).all(), "a group's work items cover the tile"
    return own


def check_stage(st):
    """The marks of one fast stage against the recomputed partitions; returns its wave_private_walk."""
    T, groups = st["T"], st["fast_groups"]
    if not st["register_measure_qualifies"]:  # every other stage keeps all its barriers
        assert st["load_map"] == "rows" and st["sync_tile_end"] and not st["wave_private_walk"]
        assert all(g["sync_before"] for g in groups)
        return False
    parts = [group_owner(T, g) for g in groups]
    slab = np.array_equal(parts[0], staging_owner(T, "slab"))
    assert st["load_map"] == ("slab" if slab else "rows")
    staged = staging_owner(T, st["load_map"])
    prev = staged
    for g, part in zip(groups, parts):
        assert g["sync_before"] == (not np.array_equal(part, prev)), "elided only where the partitions are equal"
        prev = part
    assert st["sync_tile_end"] == (not np.array_equal(parts[-1], staged))
    no_barrier = not st["sync_tile_end"] and not any(g["sync_before"] for g in groups)
    assert st["wave_private_walk"] == no_barrier
    check_records(st)
    return st["wave_private_walk"]


def last_stage(ops, slots, n, flags):
    desc = N.Plan(ops, n, slots, flags=flags).executed("expval").describe()
    for st in desc["stages"][:-1]:
        if st["fast"]:
            check_stage(st)
    return desc["stages"][-1]


@pytest.mark.parametrize("n", [23, 24])
def test_headline_shape_walks_without_a_barrier(n):
    ops, slots = he_layer_ops(n)
    st = last_stage(ops, slots, n, ALL_LIVE)
    assert st["register_measure_qualifies"] and st["T"] == 12 and len(st["fast_groups"]) == 3
    assert check_stage(st), [g["sync_before"] for g in st["fast_groups"]]
    assert st["load_map"] == "slab"
    # the wrap-around CX onto the tile's top position is kept back: it sits behind the last group
    assert [0, st["T"] - 1] in st["measure_after"], st["measure_after"]


@pytest.mark.parametrize("n", [16, 17, 20, 22])
def test_a_last_group_on_the_top_positions_keeps_its_barriers(n):
    ops, slots = he_layer_ops(n)
    st = last_stage(ops, slots, n, ALL_LIVE)
    assert st["register_measure_qualifies"]
    assert not check_stage(st)
    assert max(st["fast_groups"][-1]["bits"]) >= 10, "the last group sits on a wave-index position"


@pytest.mark.parametrize("tile_bits", [10, 12])
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_tapes(seed, tile_bits):
    n = 16
    ops, slots = to_native(fuzz_struct(seed, n))
    desc = N.Plan(ops, n, slots, flags=ALL_LIVE | N.plan_flags(tile_bits=tile_bits)).describe()
    marked = 0
    for st in desc["stages"]:
        if st["fast"]:
            private = check_stage(st)
            marked += st["register_measure_qualifies"]
            if st["register_measure_qualifies"] and tile_bits == 10:
                assert private, "a one-wave workgroup has one partition"
    assert marked == 1


def local_of_wire(st, n, wire):
    """Tile-local position of a wire in a stage (wire 0 is the top position)."""
    return st["bits"].index(n - 1 - wire)


# Tails behind the 23-qubit headline layer, whose last stage holds wire 0 at tile-local position 11 -- a wave-index
# position of its 12-bit tile -- and wire 22 at position 0.  The ring's wrap-around CX (control 0, target 11) is what the
# bare layer keeps back (test_headline_shape_walks_without_a_barrier); behind each tail a LATER op of the stage touches
# its bits, so applying it behind the last group would reorder it against that op.  `perms`: every X / CX of the tape,
# as tile-local (control or -1, target), that must therefore NOT sit behind the last group.
TOUCHED_LATER_TAILS = {
    "target_rotated": ([("RY", [0])], [(0, 11)]),
    "control_rotated": ([("RY", [22])], [(0, 11)]),
    "x_then_rotation": ([("PauliX", [0]), ("RY", [0])], [(0, 11), (-1, 11)]),
    "x_read_by_a_cx_whose_target_rotates": ([("PauliX", [0]), ("CX", [0, 22]), ("RY", [22])],
                                            [(0, 11), (-1, 11), (11, 0)]),
}


def touched_later_struct(name):
    return [(g, w) for g, w, _s, _c in he_layer_ops(23)[0]] + TOUCHED_LATER_TAILS[name][0]


@pytest.mark.parametrize("name", sorted(TOUCHED_LATER_TAILS))
def test_a_permutation_whose_bits_are_touched_later_is_not_kept_back(name):
    n = 23
    ops, slots = to_native(touched_later_struct(name))
    st = last_stage(ops, slots, n, ALL_LIVE)
    assert st["register_measure_qualifies"] and st["T"] == 12
    assert local_of_wire(st, n, 0) == 11 and local_of_wire(st, n, 22) == 0, "wire 0 sits on a wave-index position"
    behind = [tuple(ct) for ct in st["measure_after"]]
    for c, t in TOUCHED_LATER_TAILS[name][1]:
        assert max(c, t) >= 10, "the slab condition is in play: the permutation involves a top position"
        assert (c, t) not in behind, (name, (c, t), behind)
    # the boundary the wrap-around CX now changes the partition at keeps its barrier
    assert not check_stage(st) and any(g["sync_before"] for g in st["fast_groups"])


def test_an_x_onto_the_top_position_with_nothing_behind_it_is_kept_back():
    """The counterpart: the same X with no later op on its position waits behind the last group (the wrap-around CX in
    front of it, whose target it touches, does not)."""
    n = 23
    struct = [(g, w) for g, w, _s, _c in he_layer_ops(n)[0]] + [("PauliX", [0])]
    st = last_stage(*to_native(struct), n, ALL_LIVE)
    behind = [tuple(ct) for ct in st["measure_after"]]
    assert (-1, 11) in behind and (0, 11) not in behind, behind
    check_stage(st)
