"""Plan-compiler side of the measuring walk's LDS-DMA staging (k_tile2's register-measuring instantiations), no GPU.

A global_load_lds instruction writes a wave's 64 x 16 bytes to a wave-uniform LDS base plus lane x 16, so the DMA form
cannot swizzle on the destination: lane l of wave w fetches, for piece u, the amplitude pair whose SWIZZLED local index
is the slot it lands in.  Everything the kernel adds up for that address is in the plan's report -- the per-lane offsets
(as a table and as the runs the kernel takes when there are at most four), the four per-piece deltas, the tile's bit
positions -- so the map is recomputed here and compared, pair by pair, with what the register-staged slab form loads
and where it stores it.  A wrong source address is a memory fault on the device; this file comes first."""
import numpy as np
import pytest

from qml_essentials_amd import _native as N
from tests.test_abi_cpu import he_layer_ops
from tests.test_measure_in_registers_cpu import ALL_LIVE, FUZZ_SEEDS, fuzz_struct, to_native
from tests.test_wave_private_walk_cpu import sw, touched_later_struct

U32 = np.uint32


def global_of(st, e):
    """Byte offset inside the tile's span of the state of local index e (a bit permutation: linear over XOR)."""
    e = np.asarray(e, dtype=U32)
    g = np.zeros_like(e)
    for j, pos in enumerate(st["bits"]):
        g |= ((e >> U32(j)) & U32(1)) << U32(pos)
    return g.astype(np.uint64) << np.uint64(3)


def by_runs(runs, e):
    g = np.zeros_like(e)
    for off, mask, pos in runs:
        g |= ((e >> U32(off)) & U32(mask)) << U32(pos)
    return g.astype(np.uint64) << np.uint64(3)


def dma_pairs(st):
    """(global byte offset, LDS byte address) of every 16-byte access of the DMA form, shaped [wave, piece, lane],
    added up the way the kernel does: (lane offset ^ delta[u & 3]) + offset of u's three bits; LDS: wave-uniform piece
    base + 16 lane."""
    T = st["T"]
    nw = 1 << (T - 10)
    lane_off = np.asarray(st["dma_lane_offsets"], dtype=np.uint64).reshape(nw, 1, 64)
    w = np.arange(nw, dtype=U32)[:, None, None]
    u = np.arange(8, dtype=U32)[None, :, None]
    lane = np.arange(64, dtype=U32)[None, None, :]
    # the table and the runs are two forms of the same per-lane part: offset of sw(2 lane | wave << 10)
    jg = sw((U32(2) * lane) | (w << U32(10)))
    assert np.array_equal(lane_off, global_of(st, jg))
    if st["dma_lane_runs"] is not None:
        assert len(st["dma_lane_runs"]) <= 4
        assert np.array_equal(lane_off, by_runs(st["dma_lane_runs"], jg))
    deltas = np.asarray(st["dma_deltas"], dtype=np.uint64)
    assert np.array_equal(deltas, global_of(st, np.arange(4, dtype=U32) << U32(3))), "local bits 3 and 4, moved"
    uoff = global_of(st, u << U32(7))
    assert not (lane_off & uoff).any() and not (deltas[:, None, None, None] & uoff).any(), "u's bits are its own: + is ^"
    goff = (lane_off ^ deltas[(u & U32(3)).astype(np.int64)]) + uoff
    lds = (w.astype(np.uint64) << np.uint64(13)) + (u.astype(np.uint64) << np.uint64(10)) + np.uint64(16) * lane
    return np.broadcast_to(goff, (nw, 8, 64)), np.broadcast_to(lds, (nw, 8, 64))


def register_pairs(st):
    """The same for the register-staged slab form: lane l of wave w loads local index e = 2 l | u << 7 | w << 10 (and
    e + 1) into v[u] and stores it at LDS byte 8 sw(e)."""
    T = st["T"]
    nw = 1 << (T - 10)
    w = np.arange(nw, dtype=U32)[:, None, None]
    u = np.arange(8, dtype=U32)[None, :, None]
    lane = np.arange(64, dtype=U32)[None, None, :]
    e = (U32(2) * lane) | (u << U32(7)) | (w << U32(10))
    return global_of(st, e), sw(e).astype(np.uint64) << np.uint64(3)


def as_set(goff, lds):
    pairs = set(zip(goff.ravel().tolist(), lds.ravel().tolist()))
    assert len(pairs) == goff.size, "no access twice"
    return pairs


def eligible(st, sparse):
    """The conditions of the DMA form, from the fields that were there before it."""
    if not st["fast"] or not st["register_measure_qualifies"]:
        return False
    zeros_inside = sparse and any((st["zero_in"] >> p) & 1 for p in st["bits"])
    return (st["load_map"] == "slab" and not st["fast_groups"][0]["sync_before"] and not st["sync_tile_end"]
            and not zeros_inside)


def check_staging(st, sparse):
    want = eligible(st, sparse)
    assert st["staging"] == ("dma" if want else "registers"), (st["staging"], want)
    assert ("dma_deltas" in st) == want
    return want


@pytest.mark.parametrize("n", [23, 24])
def test_headline_plan_fetches_what_register_staging_stores_slot_for_slot(n):
    ops, slots = he_layer_ops(n)
    st = N.Plan(ops, n, slots, flags=ALL_LIVE).executed("expval").describe()["stages"][-1]
    assert st["T"] == 12 and st["wave_private_walk"] and check_staging(st, sparse=False)
    goff, lds = dma_pairs(st)
    assert as_set(goff, lds) == as_set(*register_pairs(st))
    # inside the tile's span, 16-byte aligned: bit positions of the tile only
    span = np.uint64(0)
    for pos in st["bits"]:
        span |= np.uint64(8) << np.uint64(pos)
    assert not (goff & ~span).any() and not (goff & np.uint64(15)).any()
    # every piece: 1 KiB contiguous in lane order, inside its wave's 8 KiB slab
    nw = 1 << (st["T"] - 10)
    for w in range(nw):
        for u in range(8):
            base = int(lds[w, u, 0])
            assert base % 1024 == 0 and np.array_equal(lds[w, u], base + 16 * np.arange(64, dtype=np.uint64))
            assert w << 13 <= base and base + 1024 <= (w + 1) << 13
    assert int(lds.max()) + 16 == 8 << st["T"], "the pieces fill the tile exactly"


@pytest.mark.parametrize("tile_bits", [10, 12])
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_tapes_take_the_dma_form_exactly_when_eligible(seed, tile_bits):
    """10-bit tiles: the workgroup is one wave, which owns every slot in every phase -- the measuring stage always
    stages by DMA.  12-bit tiles: those tapes do whose first and last group leave the top two positions alone."""
    n = 16
    ops, slots = to_native(fuzz_struct(seed, n))
    desc = N.Plan(ops, n, slots, flags=ALL_LIVE | N.plan_flags(tile_bits=tile_bits)).describe()
    took = 0
    for st in desc["stages"]:
        assert st["fast"] or "staging" not in st
        if st["fast"] and check_staging(st, sparse=False):
            assert as_set(*dma_pairs(st)) == as_set(*register_pairs(st))
            took += 1
    assert took <= 1 and (took == 1 or tile_bits == 12)


def test_more_than_four_runs_leave_the_lane_offsets_to_the_table():
    """Fuzz tape 10 at 20 qubits in 11-bit tiles: the measuring stage sits on five runs of positions, so the report has
    no runs and the kernel reads the table (tests/test_gpu_dma_staging.py runs it); the headline plans have runs."""
    ops, slots = to_native(fuzz_struct(10, 20))
    st = N.Plan(ops, 20, slots, flags=ALL_LIVE | N.plan_flags(tile_bits=11)).executed("expval").describe()["stages"][-1]
    assert st["T"] == 11 and check_staging(st, sparse=False) and st["dma_lane_runs"] is None
    assert as_set(*dma_pairs(st)) == as_set(*register_pairs(st))
    for n in (23, 24):
        ops, slots = he_layer_ops(n)
        assert N.Plan(ops, n, slots, flags=ALL_LIVE).executed("expval").describe()["stages"][-1]["dma_lane_runs"]


@pytest.mark.parametrize("name", ["target_rotated", "x_read_by_a_cx_whose_target_rotates"])
def test_touched_later_tails(name):
    """The 23-qubit layer with a rotation behind the wrap-around CX: a barrier stays somewhere in the tile loop; the
    DMA form asks only that none stays in front of the first group or at the tile's end."""
    n = 23
    ops, slots = to_native(touched_later_struct(name))
    st = N.Plan(ops, n, slots, flags=ALL_LIVE).executed("expval").describe()["stages"][-1]
    assert st["register_measure_qualifies"] and not st["wave_private_walk"]
    if check_staging(st, sparse=False):
        assert as_set(*dma_pairs(st)) == as_set(*register_pairs(st))


def test_known_zeros_inside_the_tile_keep_register_staging():
    """Default flags: the walk zero-fills and loads selectively, which a DMA piece cannot."""
    n = 18
    struct = ([("RX", [w]) for w in range(n)] + [("CX", [w, w + 1]) for w in range(0, n - 1, 2)]
              + [("RY", [w]) for w in range(n)])
    ops, slots = to_native(struct)
    st = N.Plan(ops, n, slots, flags=0).executed("expval").describe()["stages"][-1]
    assert st["register_measure_qualifies"] and any((st["zero_in"] >> p) & 1 for p in st["bits"])
    assert st["load_map"] == "slab" and not st["fast_groups"][0]["sync_before"]
    assert not check_staging(st, sparse=True) and st["staging"] == "registers"
