"""The measuring walk's last gate group through lane swaps (k_tile2's register-measuring instantiations):
<Z> of every wire against the complex128 oracle at the 1e-6 of tests/test_gpu_measure_in_registers.py.  Every case
asserts `last_group_lane_swap_last_run is True` from the executed plan's report of its last run, so none passes on the
table form; the records it measures with are checked against a NumPy model of the two swap instructions in
tests/test_lane_swap_group_cpu.py.

Shapes.  No tape of the project's fuzz seeds takes the form at 16 qubits (tests/test_lane_swap_group_cpu.py asserts
it), so the small cases are that file's hand-built tapes: 16 qubits in 10-bit tiles (one wave per workgroup, 64 tiles:
walks of 2 and 8 tiles at 160 and 640 rows) and in 12-bit tiles (four waves, 16 tiles: 2 tiles at 640 rows).  The
headline layers run at the batch sizes of tests/test_gpu_dma_staging.py: 23 qubits x 6 and 24 x 3 (plain loads, 2 tiles),
23 x 16 (1 GiB of states: the streaming instantiation, 4 tiles) -- both instantiations are reached."""
import functools

import numpy as np
import pytest

from oracle import einsum_sim as OE
from tests.test_gpu_measure_in_registers import TOL, _assert_walk, _rows
from tests.test_lane_swap_group_cpu import HAND_BUILT, M_NON_UNITARY, check_swap_records, hand_built, hand_built_plan
from tests.test_measure_in_registers_cpu import ALL_LIVE, N_PARAMS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _assert_swap_walk(desc, tpw):
    last = _assert_walk(desc, tpw)
    assert last["last_group_lane_swap"] is True and last["last_group_lane_swap_last_run"] is True
    assert last["staging_dma_last_run"] is True and last["wave_private_walk_last_run"] is True
    check_swap_records(last)
    return last


def _special_rows(ang, struct):
    """Row 1: every angle 0 (identities; unit forms with pivot 1).  Row 2: RY = pi on every wire, every other angle 0
    (m00 = 0 up to the rounding of the float32 pi: the anti-diagonal unit form)."""
    ang[1] = 0.0
    ang[2] = 0.0
    k = 0
    for name, _w in struct:
        if name == "RY":
            ang[2, k] = np.pi
        elif name == "Rot":
            ang[2, k + 1] = np.pi  # Rot(phi, theta, omega) = RZ(omega) RY(theta) RZ(phi)
        k += N_PARAMS.get(name, 0)


@functools.lru_cache(maxsize=None)
def _hand_built_reference(name, tile_bits, batch):
    """Angles (rows 1 and 2 special) and the oracle's <Z> on the sampled rows, once per (tape, batch)."""
    struct, _ops, slots, _consts = hand_built(name, tile_bits)
    ang = np.random.default_rng(8500 + tile_bits + batch).uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)
    _special_rows(ang, struct)
    rows = _rows(batch)
    want = []
    for r in rows:
        tape, k = [], 0
        for g, wires in struct:
            if g == "MAT1":
                tape.append(("Matrix", list(wires), (M_NON_UNITARY,)))
                continue
            p = N_PARAMS.get(g, 0)
            tape.append((g, list(wires), tuple(float(x) for x in ang[r, k:k + p])))
            k += p
        want.append(OE.simulate_and_measure(tape, 16, "expval", [("PauliZ", [q]) for q in range(16)], np.complex128))
    want = np.asarray(want, dtype=np.float64)
    ang.setflags(write=False)
    want.setflags(write=False)
    return ang, rows, want


def _hand_built_case(name, tile_bits, batch, tpw):
    ang, rows, want = _hand_built_reference(name, tile_bits, batch)
    plan = hand_built_plan(name, tile_bits)
    got = plan.run(torch.from_numpy(np.array(ang)).cuda(), "expval", list(range(16))).cpu().numpy()
    last = _assert_swap_walk(plan.executed("expval").describe(), tpw)
    assert last["T"] == tile_bits and last["lane_swap_crossed"] is HAND_BUILT[name][1]
    err = np.abs(got[rows] - want).max()
    print(name, tile_bits, batch, tpw, "max |err| vs oracle", err)
    assert err <= TOL, err


@pytest.mark.parametrize("name", sorted(HAND_BUILT))
def test_one_wave_per_workgroup(name):
    """10-bit tiles, the smallest at which the form is taken; a walk of 2 tiles: the first from the prologue, the
    second issued from inside the first's fused iteration, nothing behind it.  Rows 1 and 2: all-zero angles, RY = pi."""
    _hand_built_case(name, 10, 160, 2)


@pytest.mark.parametrize("name", ["two_dense", "carrier_alone_on_lane_4"])
def test_a_walk_of_eight_tiles(name):
    _hand_built_case(name, 10, 640, 8)


@pytest.mark.parametrize("name", sorted(HAND_BUILT))
def test_four_waves_per_workgroup(name):
    """12-bit tiles: positions 10 and 11 are the wave index, in no group."""
    _hand_built_case(name, 12, 640, 2)


def _headline(n, batch, tpw, rows):
    from oracle import c_port
    from qml_essentials_amd import _native as N
    from tests.test_abi_cpu import he_layer_ops
    from tests.test_gpu_unit_form_gates import _he_angles

    ops, slots = he_layer_ops(n)
    ang = _he_angles(n, batch, 8600 + n + batch)  # row 1: all-zero angles; row 2: the first RY = pi on every wire
    plan = N.Plan(ops, n, slots, flags=ALL_LIVE)
    got = plan.run(torch.from_numpy(ang).cuda(), "expval", list(range(n))).cpu().numpy()
    last = _assert_swap_walk(plan.executed("expval").describe(), tpw)
    assert last["lane_swap_crossed"] is (n == 23)
    for b in rows:
        tape = [(name, wires, tuple(float(ang[b, s]) for s in sl)) for name, wires, sl, _ in ops]
        want = c_port.expval_z(c_port.simulate(tape, n), n, list(range(n)))
        err = np.abs(got[b] - want).max()
        print(n, batch, b, "max |err| vs oracle", err)
        assert err <= TOL, (b, err)


@pytest.mark.parametrize("n,batch", [(23, 6), (24, 3)])
def test_headline_layers_plain_load_instantiation(n, batch):
    """23 qubits: a last group of one op, the crossed swaps.  24: two ops.  Every row, the special ones among them."""
    _headline(n, batch, 2, range(min(batch, 3)))


def test_headline_layer_streaming_instantiation():
    _headline(23, 16, 4, (0, 1, 2, 15))
