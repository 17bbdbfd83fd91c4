"""GPU: ``qmle_compose_circuits`` on hand-built tables against the NumPy interpreter ``tests/compose_reference.py``,
and the evaluator, cost and joint paths of ``qoc`` with ``compose="device"`` against host composition.

Bar.  1e-12 x the column scale max(1, max |reference column|), the project's bar for these quantities
(``profiles/qoc.md``); it holds on condition that the interpreter in float64 stays within a quarter of it of the
interpreter in longdouble on the same tables, which ``tests/test_qoc_joint_cpu.py`` asserts.  Overlaps are sums of d^2
products of entries of size <= the scale: same bar x max(1, max |reference|).  Worst distances measured on the MI355X:
``profiles/qoc.md``."""
import numpy as np
import pytest

import compose_reference as CR
import pulse_jac_reference as PJ
import pulse_reference as P
from qml_essentials_amd import _native as N
from qml_essentials_amd import pulses, qoc
from qml_essentials_amd.evolution import Evolution
from qml_essentials_amd.gates import PulseInformation
from qml_essentials_amd.script import Script

pytestmark = pytest.mark.gpu
BAR = 1e-12
ANGLES = np.array([0.3, 1.7, 4.0])


@pytest.fixture(autouse=True)
def _state():
    saved = dict(Evolution._solver_defaults)
    with PulseInformation.preserve_state():
        yield
    Evolution._solver_defaults.clear()
    Evolution._solver_defaults.update(saved)


def launch(tables, ov_len, full_len, mask, want_ov=True, want_full=True):
    ov, full = N.compose_circuits(tables["circuits"], tables["ops"], tables["terms"], tables["rows"],
                                  tables["n_candidates"], tables["mats"], tables["coefs"], tables["targets"],
                                  tables["jac"], mask, ov_len=ov_len if want_ov else 0,
                                  full_len=full_len if want_full else 0)
    return (None if ov is None else N.to_host(ov)), (None if full is None else N.to_host(full))


def distances(got, ref):
    """Worst distance / scale over the four outputs of every circuit."""
    worst = 0.0
    for g, r in zip(got, ref):
        for key in ("U", "dU"):
            if g[key] is not None and r[key].size:
                worst = max(worst, float((np.abs(g[key] - r[key]) / CR.column_scale(r[key])).max()))
        for key in ("ov", "dov"):
            if r[key] is not None and g[key] is not None and r[key].size:
                worst = max(worst, float(np.abs(g[key] - r[key]).max() / max(1.0, np.abs(r[key]).max())))
    return worst


# ---- hand-built tables --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (1, 5, 32))
@pytest.mark.parametrize("C", (1, 3, 65))
def test_hand_built_tables_against_the_interpreter(C, P):
    tables, ov_len, full_len = CR.hand_built_tables(C, P)
    lanes = [C * (P + 1) * 2 ** int(K["n_wires"]) for K in tables["circuits"]]
    assert any(n % 64 for n in lanes)  # circuits share waves
    for mask in (0b1, 0b1111):
        ref = CR.interpret(**tables, column_mask=mask)
        ov, full = launch(tables, ov_len, full_len, mask)
        got = CR.unpack(tables["circuits"], C, ov, full)
        worst = distances(got, ref)
        print(f"compose C={C} P={P} mask={mask:04b}: worst distance / scale {worst:.3e}")
        assert worst <= BAR
        assert got[3]["ov"] is None and np.array_equal(got[3]["U"], np.broadcast_to(np.eye(4), (C, 4, 4)))
        assert not got[3]["dU"].any() and not got[2]["dU"].any() and not got[2]["dov"].any()
        if P >= 3:  # the parameter that occurs in no op
            assert not got[0]["dU"][:, P - 1].any() and not got[1]["dov"][:, P - 1].any()
        # either output alone gives the same bits
        ov_only, none = launch(tables, ov_len, full_len, mask, want_full=False)
        none2, full_only = launch(tables, ov_len, full_len, mask, want_ov=False)
        assert none is None and none2 is None
        assert ov_only.tobytes() == ov.tobytes() and full_only.tobytes() == full.tobytes()


def test_runs_are_bit_equal_and_do_not_depend_on_the_number_of_candidates():
    tables, ov_len, full_len = CR.hand_built_tables(65, 5)
    ov, full = launch(tables, ov_len, full_len, 0b1111)
    ov2, full2 = launch(tables, ov_len, full_len, 0b1111)
    assert ov.tobytes() == ov2.tobytes() and full.tobytes() == full2.tobytes()
    got = CR.unpack(tables["circuits"], 65, ov, full)
    for c in (0, 37, 64):
        alone, ov_len1, full_len1 = CR.single_candidate(tables, c)
        one = CR.unpack(alone["circuits"], 1, *launch(alone, ov_len1, full_len1, 0b1111))
        for g, o in zip(got, one):
            for key in ("U", "dU", "ov", "dov"):
                if o[key] is not None:
                    assert g[key][c].tobytes() == o[key][0].tobytes(), (c, key)


def test_a_nan_row_reaches_exactly_the_candidates_that_read_it():
    C, P, bad = 65, 5, 2
    tables, ov_len, full_len = CR.hand_built_tables(C, P)
    clean = CR.unpack(tables["circuits"], C, *launch(tables, ov_len, full_len, 0b1111))
    jac = tables["jac"].copy()
    jac[bad] = np.nan
    got = CR.unpack(tables["circuits"], C, *launch(dict(tables, jac=jac), ov_len, full_len, 0b1111))
    rows = tables["rows"].reshape(-1, C)
    hit_any = False
    for K, g, ok in zip(tables["circuits"], got, clean):
        ops = tables["ops"][int(K["op_begin"]):int(K["op_end"])]
        hit = np.zeros(C, dtype=bool)
        for o in ops[ops["kind"] == CR.PULSE]:
            hit |= rows[int(o["mat_off"]) // C] == bad
        hit_any |= hit.any() and not hit.all()
        for key in ("U", "dU", "ov", "dov"):
            if g[key] is None or not g[key].size:
                continue
            flat = g[key].reshape(C, -1)
            assert not np.isfinite(flat[hit]).any(), key
            assert flat[~hit].tobytes() == ok[key].reshape(C, -1)[~hit].tobytes(), key
    assert hit_any


# ---- pulses.solve_with_jacobian(on_device=True) ---------------------------------------------------------------------
def test_solve_with_jacobian_on_device_masks_what_the_host_result_masks_under_an_adaptive_solver():
    """The step doubling with few steps allowed and ``throw`` off (what a scan runs under): the solves it rejects are
    NaN in all six slots of the device result, the others carry the host result's bits; nothing accepted: all NaN."""
    solves = P.seeded_solves("gaussian", 5, 7)
    solves[0, 3] = 0.0  # w = 0: the identity on every grid, accepted at once
    args = (solves, "gaussian", "lab", P.OMEGA, P.OMEGA)
    Evolution._solver_defaults.update(solver="dopri8", max_steps=64, throw=False)
    U, J, steps = pulses.solve_with_jacobian(*args)
    dev, steps_dev = pulses.solve_with_jacobian(*args, on_device=True)
    assert dev.is_cuda and tuple(dev.shape) == (7, 6, 4) and steps_dev == steps >= 32
    got = dev.cpu().numpy().reshape(7, 6, 2, 2)
    rejected = np.isnan(U).any(axis=(1, 2))
    print("adaptive, max_steps 64: steps", steps, "rejected", rejected)
    assert rejected.any() and not rejected.all()
    assert np.isnan(got[rejected]).all() and np.isnan(J[rejected]).all()
    want = np.concatenate([U[:, None], J], axis=1)
    assert np.isfinite(want[~rejected]).all() and got[~rejected].tobytes() == want[~rejected].tobytes()
    with_throw = dict(Evolution._solver_defaults, throw=True)
    Evolution._solver_defaults.update(max_steps=8)  # below the first grid: nothing is accepted
    dev, steps_dev = pulses.solve_with_jacobian(*args, on_device=True)
    U, J, steps = pulses.solve_with_jacobian(*args)
    assert steps_dev == steps < 1 and dev.is_cuda and tuple(dev.shape) == (7, 6, 4)
    assert np.isnan(dev.cpu().numpy()).all() and np.isnan(U).all() and np.isnan(J).all()
    Evolution._solver_defaults.update(with_throw)
    with pytest.raises(RuntimeError, match="max_steps"):
        pulses.solve_with_jacobian(*args, on_device=True)


# ---- the evaluator and the cost functions ----------------------------------------------------------------------------
def fixed_grid():  # the grid of the NumPy solver that the CPU tests inject: order 4, 64 steps
    Evolution._solver_defaults.update(solver="magnus4", magnus_steps=64)


def make_qoc(**kw):
    return qoc.QOC(**{**qoc.default_qoc_params, "n_steps": 50, "scan_steps": 0, **kw})


def basis_scripts(fn, wires):
    return [Script(qoc._with_basis_prep(fn, k, wires), n_qubits=wires) for k in range(2 ** wires)]


@pytest.mark.parametrize("gate", ["CRX", "CPhase"])
def test_circuit_unitaries_on_the_device_with_an_injected_solver(gate):
    q = make_qoc()
    pulse_circuit, _ = getattr(q, "create_" + gate)()
    script = Script(pulse_circuit, n_qubits=2)
    pp = np.asarray(PulseInformation.gate_by_name(gate).params, dtype=np.float64)
    cand = np.stack([pp, pp * 1.07, pp * 0.93])
    (U, dU), = qoc.circuit_unitaries([script], ANGLES, cand, PJ.solve_with_jacobian, compose="host")
    groups, launches = qoc.LAUNCH_GROUPS, qoc.COMPOSE_LAUNCHES
    (Ud, dUd), = qoc.circuit_unitaries([script], ANGLES, cand, PJ.solve_with_jacobian, compose="device")
    assert qoc.LAUNCH_GROUPS == groups + 1 and qoc.COMPOSE_LAUNCHES == launches + 1
    assert Ud.shape == U.shape and dUd.shape == dU.shape
    worst = max(float((np.abs(Ud - U) / CR.column_scale(U)).max()), float((np.abs(dUd - dU) / CR.column_scale(dU)).max()))
    print(f"circuit_unitaries {gate}: device - host, worst distance / scale {worst:.3e}")
    assert worst <= BAR


def compare_costs(label, got, want):
    for v, g, wv, wg in zip(*got, *want):
        scale = max(1.0, float(np.abs(wg).max()))
        print(f"{label}: value distance {np.abs(v - wv).max():.3e}, gradient distance / scale "
              f"{np.abs(g - wg).max() / scale:.3e}, scale {scale:.3g}")
        assert np.abs(v - wv).max() <= BAR and np.abs(g - wg).max() <= BAR * scale


@pytest.mark.parametrize("gate,wires", [("CRX", 2), ("RX", 1)])
def test_cost_functions_on_the_device_against_host_composition(gate, wires):
    fixed_grid()
    q = make_qoc(n_samples=4)
    pulse_circuit, target_circuit = getattr(q, "create_" + gate)()
    pp = np.asarray(PulseInformation.gate_by_name(gate).params, dtype=np.float64)
    args = (basis_scripts(pulse_circuit, wires), basis_scripts(target_circuit, wires), 4, wires)

    def plus(fn):
        def prepared(*a):
            for w in range(wires):
                qoc.op.H(wires=w)
            fn(*a)
        return prepared

    fid = ([Script(pulse_circuit, n_qubits=wires), Script(plus(pulse_circuit), n_qubits=wires)],
           [Script(target_circuit, n_qubits=wires), Script(plus(target_circuit), n_qubits=wires)], 4)
    for cand in (pp, np.stack([pp, pp * 1.05, pp * 0.95])):
        for label, fn, a in (("unitary", qoc.unitary_cost_fn, args), ("fidelity", qoc.fidelity_cost_fn, fid)):
            groups, launches = qoc.LAUNCH_GROUPS, qoc.COMPOSE_LAUNCHES
            got = fn(cand, *a, value_and_grad=True, compose="device")
            assert qoc.LAUNCH_GROUPS == groups + 1 and qoc.COMPOSE_LAUNCHES == launches + 1
            want = fn(cand, *a, value_and_grad=True, solver=PJ.solve_with_jacobian, compose="host")
            compare_costs(f"{gate} {label} cost", got, want)
            plain = fn(cand, *a, compose="device")
            assert all(np.array_equal(p, v) for p, v in zip(plain, got[0]))


def joint_specs(q, targets, leaves):
    theta, slices, _ = q._build_joint_layout(tuple(leaves))
    specs = []
    for name in targets:
        wires = 1 if name in q.GATES_1Q else 2
        pulse_circuit, target_circuit = q._create_joint_pair_for(name)
        specs.append({"name": name, "n_qubits": wires, "weight": qoc.QOC.JOINT_WEIGHTS_DEFAULT[name],
                      "assembler": qoc._JointAssembler(PulseInformation.gate_by_name(name), slices),
                      "pulse_basis_scripts": basis_scripts(pulse_circuit, wires),
                      "target_basis_scripts": basis_scripts(target_circuit, wires)})
    return theta, specs


def test_joint_cost_is_one_solver_call_and_one_composition_launch_for_all_gates():
    fixed_grid()
    q = make_qoc()
    theta, specs = joint_specs(q, ("RX", "H", "CX", "CRX"), ("RX", "RY", "RZ", "CZ"))
    cand = np.stack([theta, theta * 1.05, theta * 0.95])
    groups, launches = qoc.LAUNCH_GROUPS, qoc.COMPOSE_LAUNCHES
    got = qoc.joint_unitary_cost_fn(cand, specs, 3, value_and_grad=True)  # default solver: composed on the device
    assert qoc.LAUNCH_GROUPS == groups + 1 and qoc.COMPOSE_LAUNCHES == launches + 1
    want = qoc.joint_unitary_cost_fn(cand, specs, 3, value_and_grad=True, solver=PJ.solve_with_jacobian)
    assert qoc.COMPOSE_LAUNCHES == launches + 1  # an injected solver: composed on the host
    compare_costs("joint cost", got, want)
    assert got[1][0].shape == cand.shape and np.abs(want[1][0][1:]).max() > 1e-3


def test_joint_cost_of_the_eight_default_targets_against_the_host_route():
    """RY, RZ (no pulse solve at all: per-candidate closed-form matrices), CRY and CRZ beside the four above."""
    fixed_grid()
    q = make_qoc()
    theta, specs = joint_specs(q, q.JOINT_TARGETS_DEFAULT, q.JOINT_LEAVES_DEFAULT)
    cand = np.stack([theta, theta * 1.2, theta * 0.8])
    groups, launches = qoc.LAUNCH_GROUPS, qoc.COMPOSE_LAUNCHES
    got = qoc.joint_unitary_cost_fn(cand, specs, 3, value_and_grad=True)
    assert qoc.LAUNCH_GROUPS == groups + 1 and qoc.COMPOSE_LAUNCHES == launches + 1
    compare_costs("joint cost, default targets", got,
                  qoc.joint_unitary_cost_fn(cand, specs, 3, value_and_grad=True, solver=PJ.solve_with_jacobian))


JOINT = dict(envelope="gaussian", n_steps=30, n_samples=3, n_restarts=1, scan_steps=0, learning_rate=0.003)


def test_optimize_joint_end_to_end_against_the_host_run(tmp_path):
    """The configuration of tests/test_qoc_joint_cpu.py.  How far two correct runs may part is measured by the host
    run itself, rerun from a start moved by 1e-13 relative; 100 x that is allowed (the rule of
    ``test_stage_1_end_to_end_against_the_cpu_run``; measured on the MI355X: ``profiles/qoc.md``)."""
    fixed_grid()
    PulseInformation.set_envelope("gaussian")
    defaults = {leaf: np.asarray(PulseInformation.gate_by_name(leaf).params, dtype=np.float64) for leaf in ("RX", "RY")}

    def run(solver, factor, where):
        where.mkdir()
        q = make_qoc(file_dir=str(where), solver=solver, **JOINT)
        for leaf, value in defaults.items():
            PulseInformation.gate_by_name(leaf).params = value * factor
        best, slices, history = q.optimize_joint(target_gates=["RX", "RY", "H"], leaf_names=["RX", "RY"])
        return best, np.asarray(history)

    groups, launches = qoc.LAUNCH_GROUPS, qoc.COMPOSE_LAUNCHES
    best, history = run(None, 1.1, tmp_path / "gpu")
    assert qoc.LAUNCH_GROUPS - groups == 31 and qoc.COMPOSE_LAUNCHES - launches == 31  # n_steps + 1 evaluations
    _, host_history = run(PJ.solve_with_jacobian, 1.1, tmp_path / "host")
    _, moved_history = run(PJ.solve_with_jacobian, 1.1 * (1 + 1e-13), tmp_path / "moved")
    assert len(history) == 31 and np.isfinite(best).all() and history.min() < history[0]
    rows = open(tmp_path / "gpu" / "qoc_results_gaussian.csv").read().strip().splitlines()
    assert [r.split(",")[0] for r in rows] == ["RX", "RY"]
    sensitivity = abs(moved_history.min() - host_history.min())
    distance = abs(history.min() - host_history.min())
    print("optimize_joint: first loss", history[0], "lowest", history.min(), "host lowest", host_history.min(),
          "distance", distance, "host sensitivity to 1e-13 of the start", sensitivity)
    assert distance <= 100 * sensitivity
