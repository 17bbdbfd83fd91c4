"""Gates in unit-pivot form (k_tile2's FC_UDENSE / FC_UDIAG, the pivots folded into a carrier gate per chain) against
the complex128 oracle at the 1e-6 of tests/test_gpu_measure_in_registers.py: the measuring walk in both load
instantiations and the streaming one, storing passes (the state comes back with its scale AND its phase), the
whole-state regime, groups that mix the forms with every other kind of gate, chains cut at 32, known zeros.  Every
case asserts from the executed plan's description that unit-form ops ran where it means them to."""
import numpy as np
import pytest

from oracle import einsum_sim as OE
from tests.test_gpu_measure_in_registers import TOL, _assert_walk, _reference, _run
from tests.test_gpu_wave_private_walk import _mixed_fuzz_seeds
from tests.test_measure_in_registers_cpu import ALL_LIVE, N_PARAMS, fuzz_struct

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FC_CDENSE, FC_DIAG, FC_CDIAG, FC_X, FC_CX, FC_UDENSE, FC_UDIAG, FC_COUNT = 4, 16, 20, 32, 36, 48, 52, 56


def _kind(code):
    for name, lo in (("udiag", FC_UDIAG), ("udense", FC_UDENSE), ("cx", FC_CX), ("x", FC_X), ("cdiag", FC_CDIAG),
                     ("diag", FC_DIAG), ("cdense", FC_CDENSE)):
        if code >= lo:
            return name
    return "dense"


def _he_angles(n, batch, seed):
    """Row 0 random; row 1 all angles 0 (identities: form 1, pivot 1); row 2 the first RY = pi on every wire (m00 = 0
    up to the rounding of the float32 pi: every op in form 2); row 3 the first RY = pi / 2 (|m00| = |m01|, the tie);
    every other row, the last one among them, random.  (A batch of 3 ends with row 2.)"""
    ang = np.random.default_rng(seed).uniform(0, 2 * np.pi, (batch, 3 * n)).astype(np.float32)
    for row, ry in ((1, 0.0), (2, np.pi), (3, np.pi / 2)):
        if row < batch:
            ang[row] = 0.0
            ang[row, :n] = ry
    return ang


def _he_case(n, batch, tpw, rows):
    from oracle import c_port
    from qml_essentials_amd import _native as N
    from tests.test_abi_cpu import he_layer_ops

    ops, slots = he_layer_ops(n)
    assert slots == 3 * n
    ang = _he_angles(n, batch, 8200 + n + batch)
    plan = N.Plan(ops, n, slots, flags=ALL_LIVE)
    got = plan.run(torch.from_numpy(ang).cuda(), "expval", list(range(n))).cpu().numpy()
    last = _assert_walk(plan.executed("expval").describe(), tpw)
    assert last["staging"] == "dma" and last["staging_dma_last_run"] is True
    assert len(last["unit_form_ops"]) >= 8 and len(last["scale_carriers"]) == 1   # (9 + 1 at 24 qubits, 8 + 1 at 23)
    assert len(last["unit_form_ops"]) + 1 == sum(g["n_ops"] for g in last["fast_groups"])
    for b in rows:
        tape = [(name, wires, tuple(float(ang[b, s]) for s in sl)) for name, wires, sl, _ in ops]
        want = c_port.expval_z(c_port.simulate(tape, n), n, list(range(n)))
        err = np.abs(got[b] - want).max()
        print(n, batch, b, "max |err| vs oracle", err)
        assert err <= TOL, (b, err)


@pytest.mark.parametrize("n,batch", [(23, 6), (24, 3)])
def test_measuring_walk_plain_load_every_row(n, batch):
    _he_case(n, batch, 2, range(batch))


def test_measuring_walk_streaming_instantiation():
    _he_case(23, 16, 4, (0, 15))


def _tape(struct, ang_row):
    tape, k = [], 0
    for name, w in struct:
        p = N_PARAMS.get(name, 0)
        tape.append((name, list(w), tuple(float(x) for x in ang_row[k:k + p])))
        k += p
    return tape


@pytest.mark.parametrize("seed,probs", [(3, True), (13, False)])
@pytest.mark.parametrize("three_stage", [True, False])
def test_a_storing_pass_restores_scale_and_phase(seed, probs, three_stage):
    """The state itself, amplitude by amplitude as complex numbers: a pivot left behind in a stage would show as a
    global factor.  (a) all-live in 10-bit tiles: >= 3 stages, storing stages with chains; (b) default flags."""
    from qml_essentials_amd import _native as N

    n, batch = 16, 160
    struct, ang, _rows, _want = _reference(seed, n, batch)
    flags = ALL_LIVE | N.plan_flags(tile_bits=10) if three_stage else 0
    rows = [0, batch - 1]
    state, desc = _run(struct, n, ang, (), flags=flags, meas="state")
    stages = desc["stages"]
    storing = [s for s in stages[:-1] if s["unit_form_ops"]]
    if three_stage:
        assert len(stages) >= 3 and storing and all(len(s["scale_carriers"]) >= 1 for s in storing)
    assert any(s["unit_form_ops"] for s in stages)
    want = [OE.simulate_and_measure(_tape(struct, ang[r]), n, "state", (), np.complex128) for r in rows]
    for r, w in zip(rows, want):
        err = np.abs(state[r].astype(np.complex128) - np.asarray(w).reshape(-1)).max()
        print(seed, three_stage, r, "max |amplitude err| vs oracle", err)
        assert err <= TOL, (r, err)
    if probs:
        pr, desc_p = _run(struct, n, ang, (), flags=flags, meas="probs")
        assert any(s["unit_form_ops"] for s in desc_p["stages"])
        for r, w in zip(rows, want):
            err = np.abs(pr[r].astype(np.float64) - np.abs(np.asarray(w).reshape(-1)) ** 2).max()
            assert err <= TOL, (r, err)


@pytest.mark.parametrize("n", [10, 12])
@pytest.mark.parametrize("meas", ["state", "expval"])
def test_whole_state_regime(n, meas):
    from qml_essentials_amd import _native as N
    from tests.test_abi_cpu import he_layer_ops

    batch = 8
    ops, slots = he_layer_ops(n)
    ang = _he_angles(n, batch, 8300 + n)
    plan = N.Plan(ops, n, slots, flags=ALL_LIVE)
    wires = list(range(n)) if meas == "expval" else ()
    got = plan.run(torch.from_numpy(ang).cuda(), meas, wires).cpu().numpy()
    desc = plan.executed(meas).describe()
    assert desc["whole_state_lds"] and len(desc["stages"]) == 1 and desc["stages"][0]["fast"]
    assert desc["stages"][0]["unit_form_ops"] and desc["stages"][0]["scale_carriers"]
    for b in range(batch):
        tape = [(name, wires_, tuple(float(ang[b, s]) for s in sl)) for name, wires_, sl, _ in ops]
        obs = [("PauliZ", [q]) for q in range(n)] if meas == "expval" else ()
        want = np.asarray(OE.simulate_and_measure(tape, n, meas, obs, np.complex128)).reshape(-1)
        err = np.abs(got[b].astype(want.dtype) - want).max()
        assert err <= TOL, (n, meas, b, err)


def test_a_group_mixing_unit_forms_with_every_other_kind():
    """Fuzz tape 42 (16 qubits, 12-bit tiles): the last group of its first fast stage holds unit-form dense gates beside
    a controlled dense, a controlled diagonal, a plain diagonal gate and an in-register CX; tape 13's measuring stage
    has a group with an in-register X beside them.  Both measured by the walk."""
    need = {42: {"udense", "cdense", "cdiag", "diag", "cx"}, 13: {"udense", "cdense", "cdiag", "x"}}
    for seed, kinds in need.items():
        assert seed in _mixed_fuzz_seeds()
        struct, ang, rows, want = _reference(seed, 16, 640)
        got, desc = _run(struct, 16, ang, list(range(16)))
        _assert_walk(desc, 2)
        found = False
        for st in desc["stages"]:
            k = 0
            for g in st["fast_groups"]:
                found |= kinds <= {_kind(c) for c, _o in st["fast_ops"][k:k + g["n_ops"]]}
                k += g["n_ops"]
        assert found, (seed, kinds)
        assert {_kind(c) for st in desc["stages"] for c, _o in st["fast_ops"]} >= {"udense", "udiag", "dense"}
        err = np.abs(got[rows] - want).max()
        print(seed, "max |err| vs oracle", err)
        assert err <= TOL, (seed, err)


@pytest.mark.parametrize("force", [None, "9"])
def test_a_chain_longer_than_32(force, monkeypatch):
    """20 qubits, 4 layers, all-live, batch 8.  The schedule the batch run picks keeps 31 + 1 eligible ops in its
    fullest stage; candidate 9 (13-bit tiles, the plan's own schedule for live states) puts 35 into one stage: a chain
    of 32, a carrier, and a second chain behind it."""
    from oracle import c_port
    from qml_essentials_amd import _native as N
    from tests.test_abi_cpu import he_layer_ops

    n, batch = 20, 8
    ops, slots = [], 0
    for _layer in range(4):
        layer, k = he_layer_ops(n)
        ops += [(name, w, [s + slots for s in sl], c) for name, w, sl, c in layer]
        slots += k
    ang = np.random.default_rng(8400).uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)
    if force is not None:
        monkeypatch.setenv("QMLE_FORCE_CAND", force)
    plan = N.Plan(ops, n, slots, flags=ALL_LIVE)
    got = plan.run(torch.from_numpy(ang).cuda(), "expval", list(range(n))).cpu().numpy()
    desc = plan.executed("expval").describe()
    carriers = [len(s["scale_carriers"]) for s in desc["stages"]]
    units = [len(s["unit_form_ops"]) for s in desc["stages"]]
    if force is not None:
        assert max(carriers) >= 2 and max(units) > 32, (carriers, units)
    assert sum(units) >= 32
    for b in (0, batch - 1):
        tape = [(name, wires, tuple(float(ang[b, s]) for s in sl)) for name, wires, sl, _ in ops]
        want = c_port.expval_z(c_port.simulate(tape, n), n, list(range(n)))
        err = np.abs(got[b] - want).max()
        print(force, b, carriers, units, "max |err| vs oracle", err)
        assert err <= TOL, (b, err)


def test_known_zeros_inside_the_tile():
    """Default flags: idle waves skip whole groups of a chain, their zeros need no carrier."""
    n, batch = 18, 160
    struct, ang, rows, want = _reference("rx_cx_ry", n, batch)
    got, desc = _run(struct, n, ang, list(range(n)), flags=0)
    last = _assert_walk(desc, 2)
    assert any((last["zero_in"] >> p) & 1 for p in last["bits"])
    assert last["unit_form_ops"] and last["scale_carriers"]
    err = np.abs(got[rows] - want).max()
    print("max |err| vs oracle", err)
    assert err <= TOL, err
