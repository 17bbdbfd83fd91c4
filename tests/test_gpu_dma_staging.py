"""The measuring walk with its tiles staged by LDS DMA, one tile ahead (k_tile2's register-measuring instantiations),
against the complex128 oracle at the 1e-6 of tests/test_gpu_measure_in_registers.py.  Every case asserts, from the
executed plan's report of its last run, which staging form ran; the source map itself is compared with the
register-staged one, pair by pair, in tests/test_dma_staging_cpu.py.

Walk lengths (launch_tile: grid.x / 2 x batch >= 5120 workgroups per halving): the 23-qubit layer walks 2 tiles per
workgroup at a batch of 6 and 4 at a batch of 16; 16 qubits in 12-bit tiles walk 2 at 640 rows, in 11-bit
tiles 2 at 320, in 10-bit tiles 2 / 4 / 8 at 160 / 320 / 640."""
import numpy as np
import pytest

from tests.test_gpu_measure_in_registers import TOL, _assert_walk, _reference, _run
from tests.test_gpu_wave_private_walk import _mixed_fuzz_seeds
from tests.test_measure_in_registers_cpu import ALL_LIVE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _headline(n, batch, tpw):
    """The headline's layer at n qubits against oracle.c_port on the first and the last row."""
    from oracle import c_port
    from qml_essentials_amd import _native as N
    from tests.test_abi_cpu import he_layer_ops

    ops, slots = he_layer_ops(n)
    ang = np.random.default_rng(8000 + n + batch).uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)
    plan = N.Plan(ops, n, slots, flags=ALL_LIVE)
    got = plan.run(torch.from_numpy(ang).cuda(), "expval", list(range(n))).cpu().numpy()
    last = _assert_walk(plan.executed("expval").describe(), tpw)
    assert last["staging"] == "dma" and last["staging_dma_last_run"] is True
    assert last["wave_private_walk"] and last["wave_private_walk_last_run"] is True
    assert last["dma_lane_runs"] is not None, "the kernel computes the lane offsets from the runs here"
    for b in (0, batch - 1):
        tape = [(name, wires, tuple(float(ang[b, s]) for s in sl)) for name, wires, sl, _ in ops]
        want = c_port.expval_z(c_port.simulate(tape, n), n, list(range(n)))
        err = np.abs(got[b] - want).max()
        print(n, batch, b, "max |err| vs oracle", err)
        assert err <= TOL, err


@pytest.mark.parametrize("n,batch", [(23, 6), (24, 3)])
def test_plain_load_instantiation(n, batch):
    """The smallest batches at which the walk runs at all: two tiles per workgroup, the first issued in the prologue,
    the second from inside the first's last group, nothing behind it."""
    _headline(n, batch, 2)


def test_streaming_instantiation():
    """16 states of 2^23 amplitudes are 1 GiB, where launch_tile turns the streaming policy on (TileArgs::nt): the
    instantiation the benchmark runs, four tiles per workgroup."""
    _headline(23, 16, 4)


def test_a_mixed_barrier_tape_keeps_register_staging():
    """Fuzz tape 13 (16 qubits; the executed plan measures in 12-bit tiles with five groups): the barrier in front of
    the last group is elided; the ones in front of the first four groups and the one at the tile's end stay.  Other
    waves touch a wave's slab between its last gather and its next staging, so the walk stages through registers;
    same numbers as before."""
    seed = 13
    assert seed in _mixed_fuzz_seeds()
    struct, ang, rows, want = _reference(seed, 16, 640)
    got, desc = _run(struct, 16, ang, list(range(16)))
    last = _assert_walk(desc, 2)
    marks = [g["sync_before"] for g in last["fast_groups"]] + [last["sync_tile_end"]]
    assert marks == [True, True, True, True, False, True], marks
    assert last["staging"] == "registers" and last["staging_dma_last_run"] is False
    assert last["wave_private_walk_last_run"] is False
    err = np.abs(got[rows] - want).max()
    print(seed, marks, "max |err| vs oracle", err)
    assert err <= TOL, err


def test_known_zeros_inside_the_tile_keep_register_staging():
    """Default flags: the walk zero-fills and loads selectively; the tables alone would allow the DMA form's first
    condition (slab load map, no barrier in front of the first group)."""
    n, batch = 18, 160
    struct, ang, rows, want = _reference("rx_cx_ry", n, batch)
    got, desc = _run(struct, n, ang, list(range(n)), flags=0)
    last = _assert_walk(desc, 2)
    assert any((last["zero_in"] >> p) & 1 for p in last["bits"])
    assert last["load_map"] == "slab" and not last["fast_groups"][0]["sync_before"]
    assert last["staging"] == "registers" and last["staging_dma_last_run"] is False
    err = np.abs(got[rows] - want).max()
    print("max |err| vs oracle", err)
    assert err <= TOL, err


@pytest.mark.parametrize("batch,tpw", [(160, 2), (320, 4), (640, 8)])
def test_short_and_long_walks(batch, tpw):
    """Walks of 2, 4 and 8 tiles on a DMA-eligible fuzz tape (tape 13 in 10-bit tiles: one wave per workgroup, three
    groups): the prologue's tile, the tiles issued from inside the last group, and no issue behind the walk's last tile
    (tile_zr_finish's scratch aliases the tile)."""
    from qml_essentials_amd import _native as N

    struct, ang, rows, want = _reference(13, 16, batch)
    got, desc = _run(struct, 16, ang, list(range(16)), flags=ALL_LIVE | N.plan_flags(tile_bits=10))
    last = _assert_walk(desc, tpw)
    assert last["T"] == 10 and len(last["fast_groups"]) == 3 and last["dma_lane_runs"] is not None
    assert last["staging"] == "dma" and last["staging_dma_last_run"] is True
    assert last["wave_private_walk"] and last["wave_private_walk_last_run"] is True
    err = np.abs(got[rows] - want).max()
    print(batch, tpw, "max |err| vs oracle", err)
    assert err <= TOL, err


@pytest.mark.parametrize("tile_bits,T,batch,tpw", [(13, 12, 640, 2), (11, 11, 320, 2)])
def test_barriers_between_the_groups_do_not_stand_in_the_way(tile_bits, T, batch, tpw):
    """Fuzz tape 3, four waves in 12-bit tiles (the measuring stage of the 13-bit plan) and two in 11-bit tiles: the
    barriers in front of the second and later groups stay -- slots change owners inside the tile -- but the last group
    gathers the partition the staging has and none stays in front of the first group or at the tile's end: the wave
    that gathered a slot last stages it next, which is all the DMA form asks.  Not a wave-private walk."""
    from qml_essentials_amd import _native as N

    struct, ang, rows, want = _reference(3, 16, batch)
    got, desc = _run(struct, 16, ang, list(range(16)), flags=ALL_LIVE | N.plan_flags(tile_bits=tile_bits))
    last = _assert_walk(desc, tpw)
    marks = [g["sync_before"] for g in last["fast_groups"]]
    assert last["T"] == T and not marks[0] and all(marks[1:]) and len(marks) >= 3 and not last["sync_tile_end"]
    assert last["staging"] == "dma" and last["staging_dma_last_run"] is True
    assert not last["wave_private_walk"] and last["wave_private_walk_last_run"] is False
    err = np.abs(got[rows] - want).max()
    print(tile_bits, batch, tpw, marks, "max |err| vs oracle", err)
    assert err <= TOL, err


def test_lane_offsets_read_from_the_table():
    """The kernel takes a lane's source offset from runs of contiguous tile positions when there are at most four and
    from the plan's table otherwise.  Every other DMA case of this file has at most four (asserted there); fuzz tape 10
    at 20 qubits in 11-bit tiles measures on positions {0..6, 9, 13, 15, 17}, five runs: the table.  Two waves, two
    groups, no barrier; 512 tiles walk 2 per workgroup at a batch of 20.  Rows 0 and last against oracle.c_port."""
    from oracle import c_port
    from qml_essentials_amd import _native as N
    from tests.test_measure_in_registers_cpu import N_PARAMS, fuzz_struct

    n, batch = 20, 20
    struct = fuzz_struct(10, n)
    slots = sum(N_PARAMS.get(name, 0) for name, _w in struct)
    ang = np.random.default_rng(8100).uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)
    got, desc = _run(struct, n, ang, list(range(n)), flags=ALL_LIVE | N.plan_flags(tile_bits=11))
    last = _assert_walk(desc, 2)
    assert last["T"] == 11 and last["staging"] == "dma" and last["staging_dma_last_run"] is True
    assert last["wave_private_walk"] and last["wave_private_walk_last_run"] is True
    assert last["dma_lane_runs"] is None, last["dma_lane_runs"]
    for b in (0, batch - 1):
        tape, k = [], 0
        for name, wires in struct:
            p = N_PARAMS.get(name, 0)
            tape.append((name, list(wires), tuple(float(x) for x in ang[b, k:k + p])))
            k += p
        want = c_port.expval_z(c_port.simulate(tape, n), n, list(range(n)))
        err = np.abs(got[b] - want).max()
        print(b, "max |err| vs oracle", err)
        assert err <= TOL, err
