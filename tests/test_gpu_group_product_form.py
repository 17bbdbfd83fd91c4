"""Product form of k_tile2's gate groups on the GPU: opening diagonal, one real step per gate, closing
diagonal, against the complex128 oracle at the project's 1e-6 (tests/test_gpu_unit_form_gates.py).  Every case asserts
`group_product_form_last_run is True` from the report of the stage that ran, and which of its groups are marked, so
none passes on the gate-by-gate form.

Shapes.  The small cases are hand-built 16-qubit tapes under PLAN_TAPE_ORDER, after tests/test_lane_swap_group_cpu.py:
10-bit tiles (one wave per workgroup; walks of 2 and 8 tiles at 160 and 640 rows) and 12-bit tiles (four waves).  The
measuring stage of each is two groups:

  both            4 ops | 2 ops   lane-swap fused iteration, straight; both groups in product form
  front           4 ops | 1 op    ... straight; the front group in product form, the carrier alone behind the swaps
  front_crossed   4 ops | 1 op    ... crossed swaps (the 23-qubit layer's case)
  last            8 ops with CZ | 2 ops   ... the last group in product form, and it holds the carrier
  last_diagonal   the same with a diagonal op (RZ) in the last group
  crx             8 ops with a CRX | 2 ops
  three_and_four  3 ops | 4 ops   no lane swaps: two gathers, both groups in product form

(A crossed fused iteration has a last group of one op, which stays gate by gate: there is no crossed case with the last
group in product form.)  Rows 1..4 of every batch: all angles 0; every rotation angle pi (m00 = 0 up to the rounding of
the float32 pi); 2.2 (c < s: every gate mirrored); pi / 2 (c = s up to rounding).  The headline layers run at 23 and 24
qubits, a handful of states below 1 GiB (plain loads) and 1 GiB of states (the streaming instantiation)."""
import functools

import numpy as np
import pytest

from oracle import einsum_sim as OE
from tests.test_gpu_measure_in_registers import TOL, _rows
from tests.test_lane_swap_group_cpu import check_swap_records
from tests.test_measure_in_registers_cpu import ALL_LIVE, N_PARAMS, check_records

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_Q = 16
THETA = {"RY": 0, "RX": 0, "Rot": 1, "CRX": 0}   # which parameter of a gate is the rotation angle that sets c and s
SPECIAL = ((1, 0.0), (2, np.pi), (3, 2.2), (4, np.pi / 2))

# name: (front-group gates in front of its four RY, last-group gates, what the last stage must report:
#        marks of its two groups, lane swap, crossed)
VARIANTS = {
    "both": ("cx", [("Rot", 8), ("Rot", 9)], [True, True], True, False),
    "front": ("cx", [("Rot", 9)], [True, False], True, False),
    "front_crossed": ("cx", [("Rot", 8)], [True, False], True, True),
    "last": ("cz", [("Rot", 8), ("Rot", 9)], [False, True], True, False),
    "last_diagonal": ("cz", [("RZ", 8), ("Rot", 9)], [False, True], True, False),
    "crx": ("crx", [("Rot", 8), ("Rot", 9)], [False, True], True, False),
    "three_and_four": ("rot_cx", [("Rot", 8), ("Rot", 9)], [True, True], False, False),
}


def tape(name, tile_bits, n=N_Q):
    """struct of a hand-built tape, entries (gate, wires), wire = n - 1 - position (tests/test_lane_swap_group_cpu.py,
    hand_built: the top positions first, so that they fill the earlier stages; then the group {4, 5, 6, 7}, two CX inside
    it, the last group's gates on positions 8 and / or 9 -- lane bits 4 and 5 of the group in front --, two CX)."""
    def P(pos):
        return n - 1 - pos

    front, last = VARIANTS[name][:2]
    top = list(range(15, 9 if tile_bits == 10 else 10, -1))
    t = [("Rot", [P(p)]) for p in top + [0, 1, 2, 3, 4, 5, 6]]
    t += [("CZ", [P(p), P(i % 4)]) for i, p in enumerate(top)] + [("CX", [P(3), P(4)]), ("CX", [P(2), P(5)])]
    if front == "cx":        # CX live in the address tables: the group holds the four RY and nothing else
        t += [("CX", [P(7), P(4)]), ("CX", [P(7), P(5)]), ("CX", [P(7), P(6)])]
    elif front == "rot_cx":  # a rotation on 7 first: it opens a group that takes the gates on 8 and 9 along
        t += [("Rot", [P(7)]), ("CX", [P(7), P(4)]), ("CX", [P(7), P(5)]), ("CX", [P(7), P(6)])]
    else:
        t += [("Rot", [P(7)]), ("CRX" if front == "crx" else "CZ", [P(7), P(4)]), ("CZ", [P(7), P(5)]), ("CZ", [P(7), P(6)])]
    t += [("RY", [P(p)]) for p in (4, 5, 6, 7)]
    t += [("CX", [P(5), P(4)]), ("CX", [P(7), P(6)])]
    t += [(g, [P(pos)]) for g, pos in last]
    t += [("CX", [P(9), P(8)]), ("CX", [P(8), P(7)])]
    return t


def to_ops(struct):
    ops, k = [], 0
    for g, wires in struct:
        npar = N_PARAMS.get(g, 0)
        ops.append((g, list(wires), list(range(k, k + npar)), -1))
        k += npar
    return ops, k


def special_rows(ang, struct):
    for row, theta in SPECIAL:
        if row >= len(ang):
            continue
        ang[row] = 0.0
        k = 0
        for g, _w in struct:
            if g in THETA:
                ang[row, k + THETA[g]] = theta
            k += N_PARAMS.get(g, 0)


def oracle_tape(struct, ang_row):
    out, k = [], 0
    for g, wires in struct:
        p = N_PARAMS.get(g, 0)
        out.append((g, list(wires), tuple(float(x) for x in ang_row[k:k + p])))
        k += p
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, tile_bits, batch):
    """Angles (rows 1..4 special) and the oracle's <Z> on the sampled rows, once per (tape, tile, batch)."""
    struct = tape(name, tile_bits)
    _ops, slots = to_ops(struct)
    ang = np.random.default_rng(9100 + tile_bits + batch).uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)
    special_rows(ang, struct)
    rows = sorted(set(_rows(batch)) | {3, 4})
    want = np.asarray([OE.simulate_and_measure(oracle_tape(struct, ang[r]), N_Q, "expval",
                                               [("PauliZ", [q]) for q in range(N_Q)], np.complex128) for r in rows],
                      dtype=np.float64)
    ang.setflags(write=False)
    want.setflags(write=False)
    return struct, ang, rows, want


def _plan(struct, tile_bits):
    from qml_essentials_amd import _native as N

    ops, slots = to_ops(struct)
    return N.Plan(ops, N_Q, slots, flags=ALL_LIVE | N.PLAN_TAPE_ORDER | N.plan_flags(tile_bits=tile_bits))


def _assert_product_walk(last, tpw, marks, swap, crossed):
    assert last["kind"] == "tile" and last["fast"] and last["register_measure_qualifies"]
    assert last["measured_from_registers_last_run"] is True
    assert last["measure_tiles_per_workgroup_last_run"] == tpw, last["measure_tiles_per_workgroup_last_run"]
    assert last["product_form_groups"] == marks, last["product_form_groups"]
    assert last["group_product_form_last_run"] is True
    assert last["last_group_lane_swap"] is swap and last["last_group_lane_swap_last_run"] is swap
    if swap:
        assert last["lane_swap_crossed"] is crossed
        check_swap_records(last)
    else:
        check_records(last)


def _case(name, tile_bits, batch, tpw):
    struct, ang, rows, want = _reference(name, tile_bits, batch)
    plan = _plan(struct, tile_bits)
    got = plan.run(torch.from_numpy(np.array(ang)).cuda(), "expval", list(range(N_Q))).cpu().numpy()
    last = plan.executed("expval").describe()["stages"][-1]
    assert last["T"] == tile_bits and len(last["fast_groups"]) == 2
    _assert_product_walk(last, tpw, *VARIANTS[name][2:])
    err = np.abs(got[rows] - want).max(axis=1)
    print(name, tile_bits, batch, "max |err| vs oracle per row", dict(zip(rows, err)))
    assert err.max() <= TOL, err


def test_the_variants_are_what_their_names_say():
    """Group sizes, and where the carrier sits: in a product-form group (`last`) and in an ordinary one (`front`)."""
    for name, want in (("both", [4, 2]), ("front", [4, 1]), ("front_crossed", [4, 1]), ("last", [8, 2]), ("crx", [8, 2]),
                       ("three_and_four", [3, 4])):
        last = _plan(tape(name, 10), 10).executed("expval").describe()["stages"][-1]
        assert [g["n_ops"] for g in last["fast_groups"]] == want, name
        codes = [c for c, _o in last["fast_ops"]]
        assert last["scale_carriers"] == [len(codes) - 1]
        if name == "crx":
            assert any(4 <= c < 16 for c in codes[:8]), "a controlled dense gate in the front group"
        if name == "last_diagonal":
            assert 52 <= codes[-2] < 56


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_one_wave_per_workgroup(name):
    _case(name, 10, 160, 2)


@pytest.mark.parametrize("name", ["both", "front_crossed", "three_and_four"])
def test_a_walk_of_eight_tiles(name):
    _case(name, 10, 640, 8)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_four_waves_per_workgroup(name):
    _case(name, 12, 640, 2)


@pytest.mark.parametrize("name,tile_bits", [("both", 10), ("crx", 10), ("three_and_four", 12)])
def test_a_stored_state_keeps_scale_and_phase(name, tile_bits):
    """qmle_apply_inplace on live states (the plan's own stages, every one a storing k_tile2 pass): the state amplitude
    by amplitude as complex numbers -- a scale or a phase left in a closing diagonal would show."""
    from qml_essentials_amd import _native as N

    batch = 6
    struct = tape(name, tile_bits)
    _ops, slots = to_ops(struct)
    ang = np.random.default_rng(9300 + tile_bits).uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)
    special_rows(ang, struct)
    plan = _plan(struct, tile_bits)
    st = torch.zeros((batch, 1 << N_Q), dtype=torch.complex64, device="cuda")
    st[:, 0] = 1.0
    N.apply_inplace(plan, torch.from_numpy(ang).cuda(), st)
    torch.cuda.synchronize()
    got = st.cpu().numpy().astype(np.complex128)
    stages = plan.describe()["stages"]
    marked = [s for s in stages if s["kind"] == "tile" and s["fast"] and any(s["product_form_groups"])]
    assert marked and all(s["group_product_form_last_run"] is True for s in marked)
    assert any(not all(s["product_form_groups"]) for s in marked), "product-form and ordinary groups in one stage"
    for r in range(batch):
        want = np.asarray(OE.simulate_and_measure(oracle_tape(struct, ang[r]), N_Q, "state", (), np.complex128)).reshape(-1)
        err = np.abs(got[r] - want).max()
        print(name, tile_bits, r, "max |amplitude err| vs oracle", err)
        assert err <= TOL, (r, err)


def _he_angles(n, batch, seed):
    """The headline layer's angles (RY, RZ, RY per wire, the first RY in columns [0, n)): rows 1..4 special."""
    ang = np.random.default_rng(seed).uniform(0, 2 * np.pi, (batch, 3 * n)).astype(np.float32)
    for row, theta in SPECIAL:
        if row < batch:
            ang[row] = 0.0
            ang[row, :n] = theta
    return ang


@pytest.mark.parametrize("n,batch,rows", [(23, 6, range(6)), (24, 5, range(5)), (23, 16, (0, 1, 2, 3, 4, 15)),
                                          (24, 8, (0, 1, 2, 3, 4, 7))])
def test_headline_layers(n, batch, rows):
    """23 qubits: groups of 4 | 4 | 1 ops, crossed swaps; 24: 4 | 4 | 2, straight.  6 and 5 states: plain loads; 16
    and 8 states are 1 GiB: the streaming instantiation."""
    from oracle import c_port
    from qml_essentials_amd import _native as N
    from tests.test_abi_cpu import he_layer_ops

    ops, slots = he_layer_ops(n)
    assert slots == 3 * n
    ang = _he_angles(n, batch, 9400 + n + batch)
    plan = N.Plan(ops, n, slots, flags=ALL_LIVE)
    got = plan.run(torch.from_numpy(ang).cuda(), "expval", list(range(n))).cpu().numpy()
    last = plan.executed("expval").describe()["stages"][-1]
    tpw = last["measure_tiles_per_workgroup_last_run"]
    assert tpw >= 2
    _assert_product_walk(last, tpw, [True, True, n == 24], True, n == 23)
    assert last["staging_dma_last_run"] is True and last["wave_private_walk_last_run"] is True
    for b in rows:
        t = [(name, wires, tuple(float(ang[b, s]) for s in sl)) for name, wires, sl, _ in ops]
        want = c_port.expval_z(c_port.simulate(t, n), n, list(range(n)))
        err = np.abs(got[b] - want).max()
        print(n, batch, b, "max |err| vs oracle", err)
        assert err <= TOL, (b, err)
