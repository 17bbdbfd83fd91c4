"""The measuring walk with its workgroup barriers elided (k_tile2's register-measuring instantiations) against the
complex128 oracle at the 1e-6 of tests/test_gpu_measure_in_registers.py.  Every case asserts, from the executed plan's
report of its last run, that the walk ran, measured from registers and elided the barriers the case is about; the marks
themselves are checked against recomputed partitions in tests/test_wave_private_walk_cpu.py.

The headline's structure -- three groups below the wave-index positions, the wrap-around CX kept back, no barrier in
the tile loop -- first appears at 23 qubits.  The walk needs grid.x / 2 x batch >= 5120 workgroups (launch_tile), which
at 2^11 / 2^12 tiles of 2^12 amplitudes is a batch of 6 at 23 qubits and of 3 at 24: the smallest at which the path
under test runs at all (a batch of 4 resp. 2 keeps one tile per workgroup and the barriers with it)."""
import numpy as np
import pytest

from tests.test_gpu_measure_in_registers import TOL, _assert_walk, _reference, _run
from tests.test_measure_in_registers_cpu import ALL_LIVE, FUZZ_SEEDS, fuzz_struct, to_native
from tests.test_wave_private_walk_cpu import TOUCHED_LATER_TAILS, check_stage, touched_later_struct

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _mixed_fuzz_seeds():
    """The 16-qubit fuzz tapes whose measuring stage (12-bit tiles) elides some barriers and keeps others."""
    from qml_essentials_amd import _native as N

    picked = []
    for seed in FUZZ_SEEDS:
        ops, slots = to_native(fuzz_struct(seed, 16))
        last = N.Plan(ops, 16, slots, flags=ALL_LIVE).executed("expval").describe()["stages"][-1]
        marks = [g["sync_before"] for g in last["fast_groups"]] + [last["sync_tile_end"]]
        if last["T"] == 12 and last["register_measure_qualifies"] and any(marks) and not all(marks):
            picked.append(seed)
    return picked


@pytest.mark.parametrize("n,batch", [(23, 6), (24, 3)])
def test_headline_structure_walks_without_a_barrier(n, batch):
    from oracle import c_port
    from qml_essentials_amd import _native as N
    from tests.test_abi_cpu import he_layer_ops

    ops, slots = he_layer_ops(n)
    ang = np.random.default_rng(7000 + n).uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)
    plan = N.Plan(ops, n, slots, flags=ALL_LIVE)
    got = plan.run(torch.from_numpy(ang).cuda(), "expval", list(range(n))).cpu().numpy()
    last = _assert_walk(plan.executed("expval").describe(), 2)
    assert last["measure_tiles_per_workgroup_last_run"] >= 2, "one tile per workgroup is another kernel: no walk"
    assert last["wave_private_walk"] and last["wave_private_walk_last_run"] is True
    assert last["load_map"] == "slab" and not any(g["sync_before"] for g in last["fast_groups"])
    assert check_stage(last)
    for b in (0, batch - 1):
        tape = [(name, wires, tuple(float(ang[b, s]) for s in sl)) for name, wires, sl, _ in ops]
        want = c_port.expval_z(c_port.simulate(tape, n), n, list(range(n)))
        err = np.abs(got[b] - want).max()
        print(n, b, "max |err| vs oracle", err)
        assert err <= TOL, err


def test_some_fuzz_tapes_mix_elided_and_kept_barriers():
    seeds = _mixed_fuzz_seeds()
    assert len(seeds) >= 4, seeds
    maps = set()
    for seed in seeds:
        struct, ang, rows, want = _reference(seed, 16, 640)
        got, desc = _run(struct, 16, ang, list(range(16)))
        last = _assert_walk(desc, 2)
        marks = [g["sync_before"] for g in last["fast_groups"]] + [last["sync_tile_end"]]
        assert any(marks) and not all(marks) and last["wave_private_walk_last_run"] is False
        check_stage(last)
        maps.add(last["load_map"])
        err = np.abs(got[rows] - want).max()
        print(seed, last["load_map"], marks, "max |err| vs oracle", err)
        assert err <= TOL, err
    assert maps == {"slab", "rows"}, maps


def test_idle_waves_skip_groups_between_elided_barriers():
    """Default flags: known zeros inside the tile, so whole waves idle through gate groups; the first group's barrier
    is elided (slab load map), the next one stays."""
    n, batch = 18, 160
    struct, ang, rows, want = _reference("rx_cx_ry", n, batch)
    got, desc = _run(struct, n, ang, list(range(n)), flags=0)
    last = _assert_walk(desc, 2)
    zero_tile = [p for p in last["bits"][10:] if (last["zero_in"] >> p) & 1]
    assert zero_tile, "a wave-index position is known zero on input: idle waves"
    assert last["load_map"] == "slab" and not last["fast_groups"][0]["sync_before"]
    assert any(g["sync_before"] for g in last["fast_groups"]) and last["wave_private_walk_last_run"] is False
    check_stage(last)
    err = np.abs(got[rows] - want).max()
    print("max |err| vs oracle", err)
    assert err <= TOL, err


@pytest.mark.parametrize("name", ["target_rotated", "x_read_by_a_cx_whose_target_rotates"])
def test_a_permutation_touched_later_stays_in_front_of_the_op_that_touches_it(name):
    """The 23-qubit layer with a rotation behind the wrap-around CX (resp. an X, a CX reading it and a rotation): had the
    permutation been kept back behind the last group it would act after the rotation and the numbers would be wrong,
    which neither the marks nor the records can show."""
    from oracle import c_port
    from qml_essentials_amd import _native as N

    n, batch = 23, 6
    struct = touched_later_struct(name)
    ops, slots = to_native(struct)
    ang = np.random.default_rng(7100 + len(struct)).uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)
    plan = N.Plan(ops, n, slots, flags=ALL_LIVE)
    got = plan.run(torch.from_numpy(ang).cuda(), "expval", list(range(n))).cpu().numpy()
    last = _assert_walk(plan.executed("expval").describe(), 2)
    behind = [tuple(ct) for ct in last["measure_after"]]
    assert not any(ct in behind for ct in TOUCHED_LATER_TAILS[name][1]), behind
    assert last["load_map"] == "slab" and any(g["sync_before"] for g in last["fast_groups"])
    assert last["wave_private_walk_last_run"] is False
    for b in (0, batch - 1):
        tape = [(g, w, tuple(float(ang[b, s]) for s in sl)) for g, w, sl, _ in ops]
        want = c_port.expval_z(c_port.simulate(tape, n), n, list(range(n)))
        err = np.abs(got[b] - want).max()
        print(name, b, "max |err| vs oracle", err)
        assert err <= TOL, err
