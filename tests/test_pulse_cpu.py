"""CPU: the pulse-level front end (``pulses.py`` and its wiring through ``gates.py`` / ``ansaetze.py``) and the NumPy
reference the GPU tests compare against (``tests/pulse_reference.py``).

Bars.  lab == drive: 1e-13 (the product-to-sum identities, a few roundings of numbers below 2).  Variant separation:
1e-6, far above the 1e-12 to which the kernel must agree with the right scheme.  Grid against truth: 2.8e-8 = atol +
rtol of the complex64 mode, the tolerance the step-doubling rule promises."""
import numpy as np
import pytest
from scipy.linalg import expm

import evolution_reference as ER
import pulse_reference as P
from qml_essentials_amd import operations as op
from qml_essentials_amd.ansaetze import _TABLE, Ansaetze, Circuit
from qml_essentials_amd.batching import Batched
from qml_essentials_amd.gates import (Gates, PulseEnvelope, PulseGates, PulseInformation, PulseParamManager,
                                      PulseParams)
from qml_essentials_amd.pulses import PulseRotation
from qml_essentials_amd.tape import recording
from qml_essentials_amd.topologies import Topology
from qml_essentials_amd.utils import PRNGKey


@pytest.fixture(autouse=True)
def _default_pulse_state():
    PulseInformation.reset_defaults()
    yield
    PulseInformation.reset_defaults()


# ---- the reference itself --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("envelope", P.ENVELOPES)
def test_lab_and_drive_are_the_same_coefficients(envelope):
    rng = np.random.default_rng(3)
    solves = P.seeded_solves(envelope, 21, 6)
    t = rng.uniform(0.0, 3.2, size=(6, 40))
    lab = P.coefficients(envelope, "lab", solves[:, None, :], t)
    drive = P.coefficients(envelope, "drive", solves[:, None, :], t)
    for a, b in zip(lab, drive):
        assert np.abs(a - b).max() <= 1e-13


@pytest.mark.parametrize("envelope", P.ENVELOPES)
def test_front_end_coefficient_functions_equal_the_reference(envelope):
    """``build_coeff_fns`` (what the generic ``evolve()`` integrates) against the reference's closed forms, for plain
    arrays and for ``Batched`` arguments."""
    solves = P.seeded_solves(envelope, 22, 4)
    n_env = PulseEnvelope.get(envelope)["n_envelope_params"]
    t = np.linspace(0.0, 3.0, 17)
    for mode in P.MODES:
        fns = PulseEnvelope.build_coeff_fns(PulseEnvelope.get(envelope)["fn"], P.OMEGA, P.OMEGA, rwa=mode == "rwa",
                                            frame="lab" if mode == "lab" else "drive")
        for axis in (0, 1):
            rows = solves.copy()
            rows[:, 5] = axis
            want = P.coefficients(envelope, mode, rows[:, None, :], t[None, :])
            packed = np.concatenate([rows[:, :n_env], rows[:, 3:4]], axis=1)  # [envelope parameters..., w]
            for k, fn in enumerate(fns[2 * axis:2 * axis + 2]):
                one = np.stack([np.broadcast_to(fn(packed[r], t), t.shape) for r in range(len(rows))])
                assert np.abs(one - want[k]).max() <= 1e-13, (mode, axis, k)
                res = fn(Batched(packed, []), t)
                got = np.broadcast_to(res.data if isinstance(res, Batched) else res, want[k].shape)
                assert np.abs(got - want[k]).max() <= 1e-13, (mode, axis, k, "batched")


@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("envelope", P.ENVELOPES)
def test_every_wrong_variant_is_far_from_the_scheme(envelope, mode):
    solves = P.seeded_solves(envelope, 23, 6)
    right = P.scheme(envelope, mode, solves, 4, 64)
    for name in P.VARIANTS:
        wrong = P.scheme(envelope, mode, solves, 4, 64, variant=name)
        for k, row in enumerate(solves):
            if P.variant_applies(name, envelope, mode, int(row[5]), row):
                d = np.abs(wrong[k] - right[k]).max()
                assert d >= 1e-6, (envelope, mode, name, k, d)


@pytest.mark.parametrize("mode", ["rwa", "drive"])
@pytest.mark.parametrize("envelope", P.ENVELOPES)
def test_accepted_grid_is_within_tolerance_of_the_truth(envelope, mode):
    """The optimised defaults at w = pi / 2, RX and RY: the grid the doubling rule accepts at 2.8e-8 is that close to
    the truth, and needs at most 1024 steps."""
    solves = np.stack([P.default_solve(envelope, axis, np.pi / 2) for axis in (0, 1)])
    U, n, err = P.doubling(envelope, mode, solves, 2.8e-8)
    print(envelope, mode, "accepted", n, "steps; last distance", err.max())
    assert n <= 1024 and (err / 15.0 <= 2.8e-8).all()
    for k in range(2):
        d = np.abs(U[k] - P.truth(envelope, mode, solves[k])).max()
        print("   axis", k, "error against the truth", d)
        assert d <= 2.8e-8, (envelope, mode, k, d)


def test_lanes_change_the_scheme_through_rounding_only():
    solves = P.seeded_solves("drag", 24, 3)
    one = P.scheme("drag", "lab", solves, 4, 37)
    for lanes in (4, 16, 64):
        assert np.abs(P.scheme("drag", "lab", solves, 4, 37, lanes=lanes) - one).max() <= 1e-13


def test_default_drag_pulses_are_the_rotations_they_are_named_after():
    """The optimised drag defaults reach fidelity 1 - 1e-6 with t_c = t / 2, the definition they were tuned for; with
    t_c = T / 2 the derivative term integrates to zero and the same numbers lose 2e-5 and more."""
    for axis, gen in ((0, ER.X), (1, ER.Y)):
        row = P.default_solve("drag", axis, np.pi / 2)
        target = expm(-1j * np.pi / 4 * gen)
        fid = abs(np.trace(target.conj().T @ P.truth("drag", "rwa", row)) / 2) ** 2
        wrong = P.scheme("drag", "rwa", row[None], 4, 256, variant="centre_T")[0]
        fid_wrong = abs(np.trace(target.conj().T @ wrong) / 2) ** 2
        print("axis", axis, "fidelity", fid, "with t_c = T / 2", fid_wrong)
        assert fid >= 1 - 1e-6 and fid_wrong <= 1 - 2e-5


# ---- PulseParams / PulseInformation -----------------------------------------------------------------------------------
def test_pulse_params_sizes():
    want = dict(RX=4, RY=4, RZ=1, CZ=1, H=5, CX=11, CY=13, CRX=32, CRY=30, CRZ=24, CPhase=25, Rot=6)
    for name, n in want.items():
        assert PulseInformation.num_params(name) == n == len(PulseInformation.gate_by_name(name).params), name
    assert PulseInformation.num_params(Gates.CRX) == 32
    PulseInformation.set_envelope("gaussian")
    assert [PulseInformation.num_params(g) for g in ("RX", "H", "CX")] == [3, 4, 9]
    assert PulseEnvelope.available() == ["gaussian", "square", "cosine", "drag", "sech", "general"]
    with pytest.raises(ValueError):
        PulseEnvelope.get("triangle")
    with pytest.raises(ValueError):
        PulseInformation.set_frame("rotating")


def test_pulse_params_tree_splits_and_assigns():
    cx = PulseInformation.CX
    assert not cx.is_leaf and [c.name for c in cx.childs] == ["H", "CZ", "H"]
    assert sorted(leaf.name for leaf in cx.leafs) == ["CZ", "RY", "RZ"]
    parts = cx.split_params(np.arange(11.0))
    assert [list(p) for p in parts] == [[0, 1, 2, 3, 4], [5], [6, 7, 8, 9, 10]]
    assert np.array_equal(cx.params[:5], np.concatenate([PulseInformation.RZ.params, PulseInformation.RY.params]))
    with pytest.raises(AssertionError):
        PulseParams(name="both", params=np.ones(1), decomposition=[])


def assert_default_pulse_state():
    assert PulseInformation.get_envelope() == PulseInformation.DEFAULT_ENVELOPE == "drag"
    assert PulseInformation.get_rwa() is PulseInformation.DEFAULT_RWA is True
    assert PulseInformation.get_frame() == PulseInformation.DEFAULT_FRAME == "drive"
    assert PulseGates._active_envelope == "drag" and PulseGates._active_rwa is True
    assert PulseGates._active_frame == "drive"


def test_snapshot_restore_restores_config_and_leaf_params():
    snapshot = PulseInformation.snapshot_state()
    original_rx = PulseInformation.RX.params
    PulseInformation.set_envelope("gaussian", rwa=False, frame="lab")
    PulseInformation.RX.params = np.ones_like(PulseInformation.RX.params) * 0.123
    PulseInformation.restore_state(snapshot)
    assert PulseInformation.get_envelope() == snapshot.envelope
    assert PulseInformation.get_rwa() is snapshot.rwa and PulseInformation.get_frame() == snapshot.frame
    assert PulseGates._active_envelope == snapshot.envelope and PulseGates._active_rwa is snapshot.rwa
    assert PulseGates._active_frame == snapshot.frame
    assert np.allclose(PulseInformation.RX.params, original_rx)


def test_preserve_state_restores_after_exception():
    snapshot = PulseInformation.snapshot_state()
    with pytest.raises(RuntimeError, match="boom"):
        with PulseInformation.preserve_state():
            PulseInformation.set_envelope("gaussian", rwa=False, frame="lab")
            PulseInformation.RY.params = np.ones_like(PulseInformation.RY.params) * 0.456
            raise RuntimeError("boom")
    assert PulseInformation.get_envelope() == snapshot.envelope
    assert PulseInformation.get_rwa() is snapshot.rwa and PulseInformation.get_frame() == snapshot.frame
    assert np.allclose(PulseInformation.RY.params, snapshot.leaf_params["RY"])


def test_00_fixture_allows_unrestored_mutation():
    PulseInformation.set_envelope("gaussian", rwa=False, frame="lab")
    PulseInformation.RX.params = np.ones_like(PulseInformation.RX.params) * 0.789
    assert (PulseInformation.get_envelope(), PulseInformation.get_rwa(), PulseInformation.get_frame()) == \
        ("gaussian", False, "lab")


def test_01_fixture_restores_after_previous_test():
    assert_default_pulse_state()
    assert np.array_equal(PulseInformation.RX.params, PulseEnvelope.get("drag")["defaults"]["RX"])


def test_reset_and_shuffle():
    PulseInformation.reset_defaults(envelope="sech", rwa=False)
    assert (PulseInformation.get_envelope(), PulseInformation.get_rwa(), PulseInformation.get_frame()) == \
        ("sech", False, "drive")
    PulseInformation.shuffle_params(PRNGKey(3))
    for gate in PulseInformation.unique_gate_set:
        assert np.all((0 <= gate.params) & (gate.params < 1)) and len(gate.params) == len(gate)
    PulseInformation.reset_defaults()
    assert_default_pulse_state()


# ---- the router -------------------------------------------------------------------------------------------------------
def test_router_rules():
    with pytest.raises(NotImplementedError, match="PulseGates.RX"):
        Gates.RX(0.1, wires=0, gate_mode="pulse")
    with pytest.raises(ValueError, match="Unknown gate mode"):
        Gates.RX(0.1, wires=0, gate_mode="analog")
    for bad in (np.array(["10", 5, "1", 2]), [10, 5, "1", 2], (10, 5, "1", 2)):
        with pytest.raises(TypeError):
            Gates.RX(np.pi, 0, pulse_params=bad, gate_mode="pulse")
    with pytest.raises(TypeError):
        Gates.RX(np.pi, 0, pulse_params="1,2,3,4", gate_mode="pulse")
    for bad in (np.array([10.0, 5, 1]), [10, 10, 5, 5, 1, 1], (10,)):
        with pytest.raises(ValueError, match="expects 4 pulse parameters"):
            Gates.RX(np.pi, 0, pulse_params=bad, gate_mode="pulse")
    with recording() as tape:
        Gates.RX(0.3, wires=1, pulse_params=PulseInformation.RX, gate_mode="pulse")  # a PulseParams object
        Gates.RZ(0.3, wires=0, pulse_params=[0.25], gate_mode="pulse", not_a_gate_argument=1)
    assert isinstance(tape[0], PulseRotation) and tape[0].axis == "X" and tape[0].wires == [1]
    assert np.array_equal([*tape[0].env_params, tape[0].T], PulseInformation.RX.params) and tape[0].w == 0.3
    assert type(tape[1]) is op.RZ and np.isclose(tape[1].theta, 2 * 0.25 * 0.3)
    with pytest.raises(NotImplementedError):
        PulseGates.PauliRot("XX", 0.1, wires=[0, 1])


def test_pulse_manager_scales_the_optimised_parameters():
    scalers = np.array([2.0, 1.0, 0.5, 1.0, 3.0])
    with recording() as tape:
        with Gates.pulse_manager_context(scalers):
            Gates.RX(0.3, wires=0, gate_mode="pulse", pulse_params=scalers)  # (what Block.apply passes: ignored)
            Gates.RZ(0.2, wires=0, gate_mode="pulse")
            with pytest.raises(ValueError, match="Not enough pulse parameters"):
                Gates.RZ(0.2, wires=0, gate_mode="pulse")
    assert Gates._pulse_mgr is None
    base = PulseInformation.RX.params
    assert np.allclose([*tape[0].env_params, tape[0].T], base * scalers[:4])
    assert np.isclose(tape[1].theta, 2 * 0.5 * 3.0 * 0.2)
    mgr = PulseParamManager(np.arange(3.0))
    assert list(mgr.get(2)) == [0.0, 1.0] and list(mgr.get(1)) == [2.0]


# ---- ansaetze ---------------------------------------------------------------------------------------------------------
def _structure_count(name: str, n_qubits: int) -> int:
    """Pulse parameters per layer from the structure table: gate size x (wires | pairs of the topology)."""
    total = 0
    for row in _TABLE[name]:
        size = PulseInformation.num_params(row[0])
        if len(row) == 1:
            total += size * n_qubits
        else:
            kw = row[2]
            span = kw.get("span", 1)
            span = span(n_qubits) if callable(span) else span
            if n_qubits >= 2 and n_qubits > span:
                total += size * len(getattr(Topology, row[1])(n_qubits=n_qubits, **kw))
    return total


@pytest.mark.parametrize("n_qubits", [2, 4])
def test_pulse_parameter_counts_of_every_ansatz(n_qubits):
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name in _TABLE:
            got = getattr(Ansaetze, name).n_pulse_params_per_layer(n_qubits)
            assert got == _structure_count(name, n_qubits), name
        assert Ansaetze.GHZ.n_pulse_params_per_layer(n_qubits) == 5 + (n_qubits - 1) * 11
    assert Ansaetze.Circuit_19.n_pulse_params_per_layer(4) == 4 * 4 + 4 * 1 + 4 * 32
    PulseInformation.set_envelope("gaussian")
    assert Ansaetze.Circuit_19.n_pulse_params_per_layer(4) == 4 * 3 + 4 * 1 + 4 * 26


def test_circuit_build_checks_the_length_and_abstract_count_raises():
    n = Ansaetze.Circuit_19.n_pulse_params_per_layer(2)
    with pytest.raises(ValueError, match="does not match expected"):
        Ansaetze.Circuit_19()(np.zeros(6), 2, gate_mode="pulse", pulse_params=np.ones(n - 1))
    with recording() as tape:
        Ansaetze.Circuit_19()(np.arange(6.0), 2, gate_mode="pulse", pulse_params=np.ones(n))
    assert sum(isinstance(o, PulseRotation) for o in tape) == 2 + 2 * 6  # 2 RX, and 6 RY per CRX
    assert Gates._pulse_mgr is None

    class Bare(Circuit):
        def n_params_per_layer(self, n_qubits):
            return 0

        def get_control_indices(self, n_qubits):
            return None

        def build(self, w, n_qubits, **kw):
            return None

    with pytest.raises(NotImplementedError):
        Bare().n_pulse_params_per_layer(2)


# ---- leaves -----------------------------------------------------------------------------------------------------------
def test_recorded_tape_of_crx():
    with recording() as tape:
        PulseGates.CRX(0.6, wires=[2, 0])
    cx = [("RZ", [0]), ("RY", [0]), ("H_phase", [0]), ("ControlledPhaseShift", [2, 0]), ("RZ", [0]), ("RY", [0]),
          ("H_phase", [0])]
    want = [("RZ", [0]), ("RY", [0])] + cx + [("RY", [0])] + cx + [("RZ", [0])]
    assert [(o.name, o.wires) for o in tape] == want
    ry = [o for o in tape if isinstance(o, PulseRotation)]
    assert [o.w for o in ry] == [0.3, np.pi / 2, np.pi / 2, -0.3, np.pi / 2, np.pi / 2]
    assert all(o.axis == "Y" and o.envelope == "drag" and o.mode == "rwa" for o in ry)
    assert tape[0].theta == 2 * 0.5 * (np.pi / 2) and tape[-1].theta == 2 * 0.5 * (-np.pi / 2)


def test_closed_form_leaves_against_expm():
    with recording() as tape:
        PulseGates.RZ(0.7, wires=0, pulse_params=np.array([0.3]))
        PulseGates.CZ(wires=[0, 1], pulse_params=np.array([0.21]))
        PulseGates.CZ(wires=[0, 1])
        PulseGates.H(wires=0)
    assert np.allclose(tape[0].matrix, expm(-1j * 0.3 * 0.7 * ER.Z), atol=1e-15)
    assert np.allclose(tape[1].matrix, expm(-1j * 0.21 * np.pi * PulseGates._H_CZ), atol=1e-14)
    assert np.allclose(tape[2].matrix, np.diag([1, 1, 1, -1]), atol=1e-7)  # the default is 1 / pi to ten digits
    assert np.allclose(tape[-1].matrix, expm(+1j * PulseGates._H_corr), atol=1e-15)
    assert [o.name for o in tape[3:]] == ["RZ", "RY", "H_phase"]


def test_batched_arguments_make_per_sample_requests_and_keep_rz_tangents():
    w = Batched.leaf(np.array([0.1, 0.2, 0.3]), 0)
    with recording() as tape:
        PulseGates.RX(w, wires=0)
        PulseGates.RZ(w, wires=0)
        PulseGates.RY(0.4, wires=0, pulse_params=Batched(np.ones((3, 4)), []) * PulseInformation.RY.params)
    rx, rz, ry = tape
    assert rx.rows == 3 and rx.batched_request and rx._matrix_tangent is None  # no derivative through the solver
    assert np.array_equal(rx.solves()[:, 3], [0.1, 0.2, 0.3]) and np.all(rx.solves()[:, 5] == 0)
    assert rz.parameter_tangents[0] and np.allclose(rz.parameter_tangents[0][0][2], 1.0)  # d(2 * 0.5 * w) / dw
    assert ry.rows == 3 and ry._matrix_tangent == [] and np.all(ry.solves()[:, 5] == 1)
    assert np.allclose(ry.solves()[:, :3], PulseInformation.RY.params[:3])


@pytest.mark.parametrize("envelope", P.ENVELOPES)
def test_jacobian_terms_map_the_kernel_slots_onto_the_leaf_indices(envelope):
    """Arguments in the order envelope parameters, T, w sit in the kernel's derivative slots 0..n_env-1, 4, 3."""
    PulseInformation.set_envelope(envelope)
    n_env = PulseEnvelope.get(envelope)["n_envelope_params"]
    leaf = Batched.leaf(np.random.default_rng(5).uniform(0.5, 1.5, size=(2, n_env + 2)), 0)  # C = 2 candidates
    with recording() as tape:
        PulseGates.RX(leaf[n_env + 1], wires=0, pulse_params=leaf[:n_env + 1])
        PulseGates.RX(np.cos(leaf[n_env + 1]), wires=0, pulse_params=leaf[:n_env + 1])
    terms = tape[0].jacobian_terms()
    assert [slot for slot, _, _ in terms] == list(range(n_env)) + [4, 3]
    assert [index for _, index, _ in terms] == list(range(n_env + 2))
    assert all(np.array_equal(coef, np.ones(2)) for _, _, coef in terms)
    with pytest.raises(NotImplementedError, match="does not track"):
        tape[1].jacobian_terms()


# ---- the ABI (no device work: every call below is refused before the first one) ---------------------------------------
def test_pulse_entry_point_refuses_bad_arguments_before_touching_a_device():
    import ctypes as C

    from qml_essentials_amd import _native as N

    solves, out, err = np.zeros((2, 8)), np.zeros((2, 2, 2), dtype=np.complex128), np.zeros(2)
    good = dict(solves=solves.ctypes.data, n=2, env=3, mode=0, oc=P.OMEGA, oq=P.OMEGA, order=4, steps=8, lanes=0,
                f64=1, out=out.ctypes.data, prev=None, err=None)

    def call(**kw):
        a = {**good, **kw}
        return N.lib().qmle_pulse_unitaries(C.c_void_p(a["solves"]), a["n"], a["env"], a["mode"], a["oc"], a["oq"],
                                            a["order"], a["steps"], a["lanes"], a["f64"], C.c_void_p(a["out"]),
                                            C.c_void_p(a["prev"]), C.c_void_p(a["err"]), None)

    invalid, unsupported = -1, -10
    for kw in (dict(order=3), dict(order=0), dict(env=5), dict(env=-1), dict(mode=3), dict(mode=-1)):
        assert call(**kw) == unsupported, kw
    for kw in (dict(solves=None), dict(out=None), dict(n=0), dict(steps=0), dict(lanes=2), dict(lanes=128),
               dict(f64=2), dict(f64=-1), dict(err=err.ctypes.data), dict(oc=float("nan")), dict(oq=float("inf")),
               dict(n=2 ** 30, lanes=64)):
        assert call(**kw) == invalid, kw
    assert not out.any()
    assert N.PULSE_ENVELOPES == ("gaussian", "square", "cosine", "drag", "sech") == tuple(P.ENVELOPES)
    assert N.PULSE_MODES == ("rwa", "lab", "drive") == tuple(P.MODES)


def test_pulse_kernels_have_no_spills_and_no_dynamic_stack():
    import json

    import __graft_entry__ as G

    res = {k: v for k, v in json.load(open(G.RESOURCES)).items() if "k_pulse_unitaries" in k}
    assert len(res) == 30  # <order 2, 4> x <5 envelopes> x <3 modes>
    for name, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, name
        assert r["Dynamic Stack"] == "False" and r["VGPRs"] <= 128, (name, r)
