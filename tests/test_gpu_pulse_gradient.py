"""Adjoint gradients through pulse gates: ``Script.vjp`` and ``Model.gradient(gate_mode="pulse")``.

``Script.vjp`` on a two-wire tape.  The tape holds ``PulseGates.RX``, ``RY``, ``RZ``, ``CZ`` and the composite ``CRX``
with the rotation angles ``w`` and all pulse parameters as leaves.  The expected gradient is built from parts that are
tested elsewhere: ``G_ref`` of tests/matrix_cotangent_reference.py (forward simulations of the recorded tape's own
matrices) contracted with the device's own ``solve_with_jacobian`` output (held to tests/pulse_jac_reference.py by
tests/test_gpu_qoc.py), plus the two-term shift rule on the closed-form leaves (the virtual ``RZ`` and the
``ControlledPhaseShift`` of ``CZ``), folded onto the leaves by the recorder's own tangents.  So the test isolates the
sweep and the chain rule.  Bound per leaf element, derived: the sweep returns every entry of ``G`` and every angle
gradient within ``t = tolerance(n, x64) max(1, sum |w|)`` (tests/test_gpu_matrix_cotangent.py), and the element is
``sum 2 Re(G . dU/dslot) coef + sum dC/dangle coef``, so its error is at most
``2 t sum |coef| sum_ac |dU_ac/dslot|  +  t sum |coef|`` over the terms that feed it.

Measured on the MI355X: the largest error was 0.029 of its bound (gaussian / rwa / magnus4 / complex64; 0.013 cosine /
lab and drag / dopri8; 1e-3 .. 1e-2 in complex128), the x64 ``Model`` gradients met the difference quotient within its
own ``|D(2h) - D(h)|`` <= 6.2e-10 (profiles/pulse_gradient.md).

``Model``: the tuple form of ``wrt`` against the single calls, the x64 gradient against a central difference of
``model(...)`` along random directions of the joint space (bounded by step doubling), shapes, and the agreement of
``force_mean``, an explicit ``cotangent`` and the Jacobian.
"""
import numpy as np
import pytest

from qml_essentials_amd import operations as op
from qml_essentials_amd import utils
from qml_essentials_amd.evolution import Evolution
from qml_essentials_amd.gates import PulseGates, PulseInformation
from qml_essentials_amd.model import Model
from qml_essentials_amd.pulses import PulseRotation
from qml_essentials_amd.script import Script
from tests import adjoint_reference as R
from tests import matrix_cotangent_reference as M
from tests.test_gpu_adjoint_routes import tolerance

pytestmark = pytest.mark.gpu

STEPS = 64


@pytest.fixture(autouse=True)
def _default_state():
    PulseInformation.reset_defaults()
    prev = dict(Evolution._solver_defaults)
    yield
    Evolution._solver_defaults.update(prev)
    PulseInformation.reset_defaults()
    utils.enable_x64(False)


GATES = ("RX", "RY", "RZ", "CZ", "CRX")


def two_wire_circuit():
    sizes = [len(np.asarray(PulseInformation.gate_by_name(g).params).reshape(-1)) for g in GATES]
    cuts = np.cumsum([0] + sizes)

    def f(w, pp):
        part = lambda k: pp[int(cuts[k]):int(cuts[k + 1])]  # noqa: E731
        PulseGates.RY(0.7, wires=0)  # (a constant pulse leaf in front: no leaf dependence, an ordinary MAT1)
        PulseGates.RX(w[0], wires=0, pulse_params=part(0))
        PulseGates.RY(w[1], wires=1, pulse_params=part(1))
        PulseGates.RZ(w[2], wires=1, pulse_params=part(2))  # (on the CRX target: on its control it would commute out)
        PulseGates.CZ(wires=[0, 1], pulse_params=part(3))
        PulseGates.CRX(w[3], wires=[0, 1], pulse_params=part(4))
        PulseGates.RX(w[0] * 0.5, wires=1, pulse_params=part(0))  # (shared leaves: two solves feed one element)

    pp0 = np.concatenate([np.asarray(PulseInformation.gate_by_name(g).params, dtype=np.float64).reshape(-1)
                          for g in GATES])
    return f, pp0


def closed_form_matrix(o, angle):
    if o.name == "RZ":
        return np.diag([np.exp(-0.5j * angle), np.exp(0.5j * angle)])
    assert o.name in ("ControlledPhaseShift", "CPhase"), o.name
    return np.diag([1.0, 1.0, 1.0, np.exp(1j * angle)])


def expected_gradient(script, obs_mats, w_obs, args, n):
    """-> (gradient per leaf {leaf: flat array}, bound per leaf element {leaf: flat array} / (tolerance x scale))"""
    mat_ops = []
    tape, low, n_q, B, slots, leaf_shapes, _ = script._trace_for_gradient([], args, None, None, (0, 1), mat_ops=mat_ops)
    assert n_q == n and B == 1
    gates = [o for o in tape if o.lower(n) is not None]
    oracle = []
    for o in gates:
        m = np.asarray(o.matrix, dtype=np.complex128)
        oracle.append(("Matrix", list(o.wires), (m[0] if m.ndim == 3 else m,)))
    grad = {k: np.zeros(int(np.prod(shp))) for k, shp in leaf_shapes.items()}
    bound = {k: np.zeros(int(np.prod(shp))) for k, shp in leaf_shapes.items()}
    assert len(mat_ops) >= 4 and all(isinstance(o, PulseRotation) for _k, o in mat_ops)
    for k_op, o in mat_ops:
        assert gates[k_op] is o
        g_ref = M.reference_cotangent(oracle, k_op, n, obs_mats, w_obs)
        jac = np.asarray(o.jacobian, dtype=np.complex128)[0]  # [5, 2, 2]: the device's own sensitivities
        for lid, slot, flat, coef in o.leaf_jacobian_terms():
            c = float(np.asarray(coef).reshape(-1)[0])
            grad[lid][flat] += 2.0 * np.real(np.sum(g_ref * jac[slot])) * c
            bound[lid][flat] += 2.0 * abs(c) * np.abs(jac[slot]).sum()
    angle_ops = 0
    for k_op, o in enumerate(gates):
        tans = [t for t in o.parameter_tangents if t] if not isinstance(o, PulseRotation) else []
        if not tans:
            continue
        angle_ops += 1
        (tangent,) = tans
        angle = float(np.asarray(o.parameters[0]).reshape(-1)[0])
        cost = lambda a: M.cost_of(R.run_from(R.zero_state(n), M.replaced(oracle, k_op, closed_form_matrix(o, a)), n),  # noqa: E731
                                   n, obs_mats, w_obs)
        assert abs(cost(angle) - M.cost_of(R.run_from(R.zero_state(n), oracle, n), n, obs_mats, w_obs)) <= 1e-12
        d = 0.5 * (cost(angle + np.pi / 2) - cost(angle - np.pi / 2))
        for lid, flat, coef in tangent:
            c = float(np.asarray(coef).reshape(-1)[0])
            grad[lid][int(flat)] += d * c
            bound[lid][int(flat)] += abs(c)
    assert angle_ops >= 2  # the virtual RZ (several: the composites hold more) and the CZ phase
    return grad, bound


# every envelope once; rwa and two non-RWA frames; magnus4 and two adaptive names; complex64 and x64
CONFIGS = [("gaussian", "rwa", "magnus4", False), ("square", "rwa", "magnus4", True),
           ("cosine", "lab", "magnus4", False), ("drag", "rwa", "dopri8", False),
           ("sech", "drive", "magnus4", True), ("gaussian", "lab", "dopri5", True)]


@pytest.mark.parametrize("envelope,mode,solver,x64", CONFIGS)
def test_vjp_through_pulse_leaves_on_a_two_wire_tape(envelope, mode, solver, x64):
    if mode == "rwa":
        PulseInformation.set_envelope(envelope, rwa=True)
    else:
        PulseInformation.set_envelope(envelope, rwa=False, frame=mode)
    Evolution.set_solver_defaults(solver=solver, magnus_steps=STEPS)
    utils.enable_x64(x64)
    f, pp0 = two_wire_circuit()
    rng = np.random.default_rng(21)
    w = rng.uniform(0.3, 2.5, 4)
    pp = pp0 * rng.uniform(0.95, 1.05, pp0.shape)
    obs = [op.PauliZ(wires=0, record=False), op.PauliZ(wires=1, record=False)]
    w_obs = np.array([0.8, -1.1])
    obs_mats = R.z_mats([[0], [1]])
    script = Script(f=f, n_qubits=2)
    g_w, g_pp = script.vjp(obs, w_obs, args=(w, pp), argnums=(0, 1))
    assert g_w.shape == w.shape and g_pp.shape == pp.shape
    want, bound = expected_gradient(script, obs_mats, w_obs, (w, pp), 2)
    t = tolerance(2, x64) * max(1.0, np.abs(w_obs).sum())
    worst = 0.0
    for got, lid in ((g_w, 0), (g_pp, 1)):
        err = np.abs(np.asarray(got).reshape(-1) - want[lid])
        fed = bound[lid] > 0
        assert fed.any() and not np.asarray(got).reshape(-1)[~fed].any()
        worst = max(worst, (err[fed] / (t * bound[lid][fed])).max())
        assert (err <= t * bound[lid]).all(), (envelope, mode, solver, x64, lid, int(np.argmax(err - t * bound[lid])))
    print(envelope, mode, solver, "x64" if x64 else "c64", "largest error as a fraction of its bound", worst)
    assert np.abs(want[1]).max() > 1e-3 and np.abs(want[0]).min() > 1e-3  # (nothing to compare: a vacuous tape)


def test_an_argument_the_recorder_lost_track_of_is_refused():
    def f(w):
        PulseGates.RX(w[0] ** 2, wires=0)  # (a power: the recorder tracks sums, constant factors and products only)

    with pytest.raises(NotImplementedError, match="does not track"):
        Script(f=f, n_qubits=1).vjp([op.PauliZ(wires=0, record=False)], np.array([1.0]), args=(np.array([0.3]),))


# ---- Model ---------------------------------------------------------------------------------------------------------
def model_case(n, layers, circuit, n_inputs, seed=3):
    model = Model(n_qubits=n, n_layers=layers, circuit_type=circuit)
    rng = np.random.default_rng(seed)
    params = rng.uniform(0, 2 * np.pi, model.params.shape)
    scalers = rng.uniform(0.95, 1.05, model.pulse_params.shape)
    inputs = np.linspace(-1.0, 1.0, n_inputs)
    return model, params, scalers, inputs


@pytest.mark.parametrize("n,layers,circuit", [(2, 1, "Hardware_Efficient"), (3, 1, "Circuit_19")])
def test_model_gradient_in_pulse_mode(n, layers, circuit):
    Evolution.set_solver_defaults(solver="magnus4", magnus_steps=STEPS)
    model, params, scalers, inputs = model_case(n, layers, circuit, 3)
    kw = dict(params=params, inputs=inputs, pulse_params=scalers, gate_mode="pulse", method="adjoint")
    both = model.gradient(wrt=("params", "pulse_params"), force_mean=True, **kw)
    assert isinstance(both, tuple) and len(both) == 2
    g_p = model.gradient(wrt="params", force_mean=True, **kw)
    g_s = model.gradient(wrt="pulse_params", force_mean=True, **kw)
    assert both[0].shape == g_p.shape == (3,) + model.params.shape[1:]
    assert both[1].shape == g_s.shape == (3,) + model.pulse_params.shape
    assert np.array_equal(both[0], g_p) and np.array_equal(both[1], g_s)  # the same trace, sweep and chain rule
    assert np.abs(g_s).max() > 1e-4
    # force_mean, the explicit cotangent that it stands for, and the mean of the Jacobian's rows
    n_out = n
    cot = np.full((3, n_out), 1.0 / n_out)
    by_cot = model.gradient(wrt=("params", "pulse_params"), cotangent=cot, **kw)
    jac = model.gradient(wrt=("params", "pulse_params"), **kw)
    assert jac[0].shape == (3, n_out) + model.params.shape[1:] and jac[1].shape == (3, n_out) + model.pulse_params.shape
    t = 2 * tolerance(n, False)  # two sweeps of the same numbers, each within the route tolerance (sum |w| = 1)
    for k in range(2):
        scale = max(1.0, np.abs(both[k]).max())
        assert np.abs(by_cot[k] - both[k]).max() <= t * scale
        assert np.abs(jac[k].mean(axis=1) - both[k]).max() <= t * scale * 10  # (ten-fold: the chain rule's factors)
    auto = model.gradient(wrt="pulse_params", force_mean=True, **{**kw, "method": "auto"})
    assert np.array_equal(auto, g_s)


@pytest.mark.parametrize("n,layers,circuit", [(2, 1, "Hardware_Efficient"), (3, 1, "Circuit_19")])
def test_model_gradient_x64_equals_the_difference_quotient(n, layers, circuit):
    """along three random directions of the joint (params, pulse_params) space; the quotient is bounded by comparing
    the step with its double, and the gradient must meet it within that bound (plus 1e-9 of rounding)"""
    Evolution.set_solver_defaults(solver="magnus4", magnus_steps=STEPS)
    model, params, scalers, inputs = model_case(n, layers, circuit, 2)
    rng = np.random.default_rng(4)
    with utils.x64_scope(True):
        g_p, g_s = model.gradient(params=params, inputs=inputs, pulse_params=scalers, gate_mode="pulse",
                                  method="adjoint", wrt=("params", "pulse_params"), force_mean=True)
        assert g_p.dtype == np.float64
        for _ in range(3):
            dp, ds = rng.standard_normal(params.shape), rng.standard_normal(scalers.shape)
            ds *= 0.1  # (scalers move the pulse duration: a smaller step keeps the quotient's error down)

            def f(s):
                return np.asarray(model(params=params + s * dp, inputs=inputs, pulse_params=scalers + s * ds,
                                        gate_mode="pulse", force_mean=True), dtype=np.float64)

            want = (g_p * dp[0]).reshape(2, -1).sum(axis=1) + (g_s * ds).reshape(2, -1).sum(axis=1)
            d1, d2 = R.central_difference(f, 1e-3), R.central_difference(f, 2e-3)
            quotient = np.abs(d2 - d1).max()
            print(circuit, "gradient . direction", want, "D(h)", d1, "|D(2h) - D(h)|", quotient)
            assert quotient <= 1e-6
            assert np.abs(want - d1).max() <= quotient + 1e-9
