"""<Z> out of the last gate group's registers (k_tile2's multi-tile measuring walk) against the complex128 oracle at
1e-6 -- the bound tests/test_gpu_kernels.py holds -- on small states with a wide batch: the walk needs
grid.x / 2 x batch >= 5120 workgroups, so 16 qubits (16 tiles of 2^12) with 640 rows walk 2 tiles per workgroup and
17 qubits with 320 / 640 / 1280 rows walk 2 / 4 / 8.  Every test that means the walk asserts, from the executed plan's
report of its last run, that the walk ran with that many tiles and measured from registers."""
import functools

import numpy as np
import pytest

from oracle import einsum_sim as OE
from tests.test_measure_in_registers_cpu import ALL_LIVE, FUZZ_SEEDS, N_PARAMS, check_records, fuzz_struct, to_native

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-6


def _he(n):
    from tests.test_abi_cpu import he_layer_ops

    return [(name, list(wires)) for name, wires, _s, _c in he_layer_ops(n)[0]]


def _case(name, n):
    """Layouts behind the last group: (a) dense gates last, (b) the ring of CX with its wrap-around, (c) trailing X,
    (d) a CX between dense gates of the last stage plus trailing CX, (e) = (b): that stage is ONE group."""
    he = _he(n)
    if name == "dense_last":
        return he + [("RX", [w]) for w in range(n)]
    if name == "cx_ring":
        return he
    if name == "trailing_x":
        return he + [("PauliX", [0]), ("PauliX", [5]), ("PauliX", [n - 1])]
    if name == "cx_sandwich":
        return he + [("RX", [n - 1]), ("RX", [n - 2]), ("CX", [n - 1, n - 2]), ("RX", [n - 2]), ("RX", [n - 1]),
                     ("CX", [n - 2, n - 3]), ("CX", [n - 3, n - 4])]
    # default-engine cases: rotations last, so that the plan keeps a measuring tile stage with known zeros inside it
    if name == "ring_rx":
        return he + [("RX", [w]) for w in range(n)]
    if name == "rx_cx_ry":
        return ([("RX", [w]) for w in range(n)] + [("CX", [w, w + 1]) for w in range(0, n - 1, 2)]
                + [("RY", [w]) for w in range(n)])
    if name == "two_rings_rx":
        return he + he + [("RX", [w]) for w in range(n)]
    raise KeyError(name)


def _angles(struct, batch, seed):
    slots = sum(N_PARAMS.get(name, 0) for name, _w in struct)
    return np.random.default_rng(seed).uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)


def _rows(batch):
    """A fixed sample of rows: both ends and the middle of the batch."""
    return sorted({0, 1, 2, batch // 2 - 1, batch // 2, batch - 3, batch - 2, batch - 1} & set(range(batch)))


def _oracle(struct, ang, rows, n, wires):
    out = []
    for r in rows:
        tape, k = [], 0
        for name, w in struct:
            p = N_PARAMS.get(name, 0)
            tape.append((name, list(w), tuple(float(x) for x in ang[r, k:k + p])))
            k += p
        out.append(OE.simulate_and_measure(tape, n, "expval", [("PauliZ", [q]) for q in wires], np.complex128))
    return np.asarray(out, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _reference(name, n, batch, n_rows=8):
    """Angles and the oracle's <Z> of all n wires on the sampled rows, computed once per (circuit, size, batch)."""
    struct = _case(name, n) if isinstance(name, str) else fuzz_struct(name, n)
    ang = _angles(struct, batch, seed=4000 + n + batch)
    rows = _rows(batch)[:n_rows]
    want = _oracle(struct, ang, rows, n, list(range(n)))
    ang.setflags(write=False)
    want.setflags(write=False)
    return struct, ang, rows, want


def _run(struct, n, ang, wires, flags=ALL_LIVE, meas="expval"):
    from qml_essentials_amd import _native as N

    ops, slots = to_native(struct)
    plan = N.Plan(ops, n, slots, flags=flags)
    out = plan.run(torch.from_numpy(np.array(ang, dtype=np.float32)).cuda(), meas, wires)
    torch.cuda.synchronize()
    return out.cpu().numpy(), plan.executed(meas).describe()


def _assert_walk(desc, tpw):
    """The run measured with k_tile2's multi-tile walk, `tpw` tiles per workgroup, from the last group's registers."""
    last = desc["stages"][-1]
    assert len(desc["stages"]) > 1 and last["kind"] == "tile" and last["fast"], (last["kind"], last["fast"])
    assert last["expval_kernel"] == "k_tile" and last["register_measure_qualifies"]
    assert last["measure_tiles_per_workgroup_last_run"] == tpw, last["measure_tiles_per_workgroup_last_run"]
    assert last["measured_from_registers_last_run"] is True
    check_records(last)
    return last


@pytest.mark.parametrize("name", ["dense_last", "cx_ring", "trailing_x", "cx_sandwich"])
def test_layouts_behind_the_last_group(name):
    n, batch = 16, 640
    struct, ang, rows, want = _reference(name, n, batch)
    got, desc = _run(struct, n, ang, list(range(n)))
    last = _assert_walk(desc, 2)
    after = last["measure_after"]
    if name == "dense_last":
        assert after == [] and len(last["fast_groups"]) > 1
    elif name == "cx_ring":  # one group: the first is the last; the wrap-around CX targets the tile's top position
        assert len(last["fast_groups"]) == 1 and any(c >= 0 and t == last["T"] - 1 for c, t in after)
    elif name == "trailing_x":
        assert any(c < 0 for c, _t in after) and any(neg for *_m, neg in last["measure_records"])
    else:
        assert len(last["fast_groups"]) > 1 and any(c >= 0 for c, _t in after)
    err = np.abs(got[rows] - want).max()
    print(name, "max |err| vs oracle", err)
    assert err <= TOL, err


@pytest.mark.parametrize("batch,tpw", [(320, 2), (640, 4), (1280, 8)])
def test_every_walk_length_and_where_a_positions_bit_lives(batch, tpw):
    """17 qubits, the ring: measured positions sit on in-thread bits, lane bits, wave bits, walk bits (the lowest
    outer positions) and workgroup-index bits (the other outer positions); all wires, then a shuffled strict subset."""
    n = 17
    struct, ang, rows, want = _reference("cx_ring", n, batch)
    got, desc = _run(struct, n, ang, list(range(n)))
    last = _assert_walk(desc, tpw)
    T = last["T"]
    outer = sorted(set(range(n)) - set(last["bits"]))
    walk_bits = tpw.bit_length() - 1
    assert len(outer) > walk_bits, "some outer positions are walk bits, the others workgroup-index bits"
    kinds = {"thread": 0, "lane": 0, "wave": 0}
    for wht, lane, wave, _neg in last["measure_records"]:
        kinds["thread"] += bool(wht)
        kinds["lane"] += bool(lane)
        kinds["wave"] += bool(wave)
    assert all(kinds.values()) and len(last["measure_records"]) == T, kinds
    err = np.abs(got[rows] - want).max()
    print(batch, tpw, "max |err| vs oracle", err)
    assert err <= TOL, err
    # a strict subset of the wires, shuffled: one wire of each kind of position
    pos_of_wire = lambda w: n - 1 - w
    subset = [n - 1 - outer[0], n - 1 - outer[-1], n - 1 - last["bits"][0], n - 1 - last["bits"][T - 1],
              n - 1 - last["bits"][6], 3]
    subset = list(dict.fromkeys(subset))
    assert 0 < len(subset) < n and {pos_of_wire(w) for w in subset} & set(outer)
    got_s, desc_s = _run(struct, n, ang, subset)
    _assert_walk(desc_s, tpw)
    err_s = np.abs(got_s[rows] - want[:, subset]).max()
    assert err_s <= TOL, err_s


def test_default_flags_on_the_ring_take_their_own_kernel_and_agree():
    """Known-zero tracking and CX folding on (the default), the ring last: the folded CX leave one small group, which a
    register-measuring kernel takes -- not this walk; same numbers."""
    n, batch = 16, 640
    struct, ang, rows, want = _reference("cx_ring", n, batch)
    got, desc = _run(struct, n, ang, list(range(n)), flags=0)
    assert desc["stages"][-1]["measured_from_registers_last_run"] is False
    err = np.abs(got[rows] - want).max()
    assert err <= TOL, err


@pytest.mark.parametrize("absorb", [True, False])
@pytest.mark.parametrize("name,n,batch,tpw,T,n_rows", [
    ("ring_rx", 16, 640, 2, 12, 8), ("ring_rx", 17, 640, 4, 12, 8),
    ("rx_cx_ry", 18, 160, 2, 12, 8),      # the last group scatters in place (no re-layout): idle waves skip its gather
    ("two_rings_rx", 18, 320, 2, 13, 4),  # 13-bit tiles: 8 waves, the upper ones idle (4 oracle rows: 110 gates)
])
def test_default_engine_walks_over_known_zeros_measure_from_registers(name, n, batch, tpw, T, n_rows, absorb):
    """Known-zero tracking ON (the default engine, with and without observable folding): the last stage starts with
    known zeros INSIDE its tile, so work items -- whole waves of them -- idle through gate groups and the last group
    of an idle wave hands zeros to the accumulate step instead of gathering.  Same walk, same records, same bound."""
    from qml_essentials_amd import _native as N

    struct, ang, rows, want = _reference(name, n, batch, n_rows)
    got, desc = _run(struct, n, ang, list(range(n)), flags=0 if absorb else N.PLAN_NO_ABSORB)
    last = _assert_walk(desc, tpw)
    assert last["T"] == T
    zero_tile = [p for p in last["bits"] if (last["zero_in"] >> p) & 1]
    zero_outer = [p for p in range(n) if p not in last["bits"] and (last["zero_in"] >> p) & 1]
    assert len(zero_tile) >= 4 and not zero_outer, (zero_tile, zero_outer)
    if name == "rx_cx_ry":
        assert last["fast_groups"][-1]["relayout"] == 0 and last["fast_groups"][-1]["n_ops"] > 0
    err = np.abs(got[rows] - want).max()
    print(name, n, absorb, "max |err| vs oracle", err)
    assert err <= TOL, err


def test_a_batch_too_small_for_the_walk_keeps_one_tile_per_workgroup():
    n, batch = 16, 640
    struct, ang, rows, want = _reference("cx_ring", n, batch)
    got, desc = _run(struct, n, ang[rows], list(range(n)))
    last = desc["stages"][-1]
    assert last["register_measure_qualifies"]  # the stage qualifies; this run's grid does not
    assert last["measure_tiles_per_workgroup_last_run"] == 1 and last["measured_from_registers_last_run"] is False
    err = np.abs(got - want).max()
    assert err <= TOL, err


def test_state_and_probabilities_of_the_same_plan_keep_the_identity_layout():
    """<Z> taken on the host from the probabilities (and from the state) of the same circuit equals the walk's."""
    n, batch = 16, 640
    struct, ang, rows, want = _reference("trailing_x", n, batch)
    got, desc = _run(struct, n, ang, list(range(n)))
    _assert_walk(desc, 2)
    probs, _ = _run(struct, n, ang[rows], (), meas="probs")
    state, _ = _run(struct, n, ang[rows], (), meas="state")
    idx = np.arange(1 << n)
    signs = np.stack([1.0 - 2.0 * ((idx >> (n - 1 - w)) & 1) for w in range(n)], axis=1)  # wire 0 = MSB
    z_probs = probs.astype(np.float64) @ signs
    z_state = (np.abs(state.astype(np.complex128)) ** 2) @ signs
    assert np.abs(z_probs - got[rows]).max() <= TOL, np.abs(z_probs - got[rows]).max()
    assert np.abs(z_state - got[rows]).max() <= TOL, np.abs(z_state - got[rows]).max()
    assert np.abs(z_probs - want).max() <= TOL


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_tapes(seed):
    n, batch = 16, 640
    struct, ang, rows, want = _reference(seed, n, batch)
    got, desc = _run(struct, n, ang, list(range(n)))
    _assert_walk(desc, 2)
    err = np.abs(got[rows] - want).max()
    print(seed, "max |err| vs oracle", err)
    assert err <= TOL, err
