"""GPU: ``qmle_pulse_unitaries_jac`` against the NumPy forward-mode scheme of ``tests/pulse_jac_reference.py`` on the same
grid, ``pulses.solve_with_jacobian``, and ``qoc`` with the default (GPU) solver against the same code with the NumPy
solver injected.

Bars.  Slot 0 (U): 1e-12, the project's complex128 bar.  Slot k: 1e-12 x max(1, max |J_ref column|) -- an entry of
dU/dT carries the factor omega t that an entry of U does not.  The reference's own distance between float64 and
``np.longdouble`` is at most 5.8e-14 of that scale over the seeded cases below (``tests/test_qoc_cpu.py`` asserts that
it stays under a quarter of the bar; ``profiles/qoc.md`` has the figures), so the scale factor stands as it is.
"""
import ctypes as C

import numpy as np
import pytest

import pulse_jac_reference as PJ
import pulse_reference as P
from pulse_jac_reference import column_scale
from qml_essentials_amd import _native as N
from qml_essentials_amd import pulses, qoc, utils
from qml_essentials_amd.evolution import Evolution
from qml_essentials_amd.gates import PulseEnvelope, PulseInformation
from qml_essentials_amd.script import Script

pytestmark = pytest.mark.gpu

SEED, N_SOLVES, N_STEPS = 5, 7, 37  # (the cases of tests/test_qoc_cpu.py)
BAR = 1e-12


@pytest.fixture(autouse=True)
def _default_state():
    PulseInformation.reset_defaults()
    prev = dict(Evolution._solver_defaults)
    yield
    Evolution._solver_defaults.update(prev)
    PulseInformation.reset_defaults()
    utils.enable_x64(False)


def jac(solves, envelope, mode, order, steps, lanes=0):
    return N.pulse_unitaries_jac(solves, envelope, mode, P.OMEGA, P.OMEGA, order, steps,
                                 lanes_per_solve=lanes).cpu().numpy()


# ---- the kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("envelope", P.ENVELOPES)
def test_kernel_matches_the_forward_mode_scheme_on_the_same_grid(envelope, mode):
    """Both orders, every lane split (37 steps on 64 lanes leaves lanes empty; 7 x 64 work items are two blocks)."""
    solves = P.seeded_solves(envelope, SEED, N_SOLVES)
    worst = np.zeros(6)
    for order in (2, 4):
        want = PJ.scheme_jac(envelope, mode, solves, order, N_STEPS)
        scale = column_scale(want)
        for lanes in (1, 4, 16, 64):
            got = jac(solves, envelope, mode, order, N_STEPS, lanes)
            assert got.shape == (N_SOLVES, 6, 2, 2) and got.dtype == np.complex128
            err = np.abs(got - want).max(axis=(0, 2, 3)) / scale
            worst = np.maximum(worst, err)
            print(envelope, mode, order, lanes, "distance / scale per slot", err)
            assert (err <= BAR).all(), (envelope, mode, order, lanes, err)
            if envelope != "drag":
                assert not got[:, 3].any()  # the p2 slot of a two-parameter envelope
    print(envelope, mode, "worst distance / scale per slot", worst)


@pytest.mark.parametrize("envelope", P.ENVELOPES)
def test_slot_0_is_the_result_of_the_plain_solve(envelope):
    solves = P.seeded_solves(envelope, SEED, N_SOLVES)
    for mode in P.MODES:
        for order in (2, 4):
            for lanes in (1, 16, 0):
                U = N.pulse_unitaries(solves, envelope, mode, P.OMEGA, P.OMEGA, order, N_STEPS,
                                      lanes_per_solve=lanes).cpu().numpy()
                got = jac(solves, envelope, mode, order, N_STEPS, lanes)[:, 0]
                assert np.abs(got - U).max() <= BAR, (envelope, mode, order, lanes)


def test_a_solve_beyond_the_norm_bound_is_nan_in_six_slots_and_its_neighbours_are_untouched():
    solves = P.seeded_solves("gaussian", SEED, N_SOLVES)
    bad = solves.copy()
    bad[3, 0] = 1e40
    for lanes in (1, 16, 64):
        clean = jac(solves, "gaussian", "lab", 4, N_STEPS, lanes)
        got = jac(bad, "gaussian", "lab", 4, N_STEPS, lanes)
        assert np.isnan(got[3].real).all() and np.isnan(got[3].imag).all()
        keep = np.arange(N_SOLVES) != 3
        assert np.isfinite(got[keep]).all()
        assert np.array_equal(got[keep], clean[keep])  # bit for bit what the clean table gives at this lane count
    inf = solves.copy()
    inf[0, 3] = np.inf
    got = jac(inf, "gaussian", "rwa", 2, N_STEPS, 4)
    assert np.isnan(got[0].real).all() and np.isfinite(got[1:]).all()


@pytest.mark.parametrize("envelope", ("square", "cosine"))
def test_a_width_equal_to_T_counts_as_the_T_side(envelope):
    """Rows 1 and 4 of the seeded solves have width == T: no grid term in the width slot (square: the slot is zero),
    the full one in the T slot; a width one ulp below T moves the grid term over."""
    solves = P.seeded_solves(envelope, SEED, N_SOLVES)
    ties = np.flatnonzero(solves[:, 1] == solves[:, 4])
    assert list(ties) == [1, 4]
    got = jac(solves, envelope, "lab", 4, N_STEPS, 4)
    want = PJ.scheme_jac(envelope, "lab", solves, 4, N_STEPS)
    scale = column_scale(want)[:, None, None]
    assert (np.abs(got - want)[ties] / scale).max() <= BAR
    assert np.abs(got[ties, 5]).max() > 1e-3
    if envelope == "square":
        assert not got[ties, 2].any()
    below = solves[ties].copy()
    below[:, 1] = np.nextafter(below[:, 1], 0.0)
    moved = jac(below, envelope, "lab", 4, N_STEPS, 4)
    assert not moved[:, 5].any()  # dS/dT = 0 on the width side
    want_b = PJ.scheme_jac(envelope, "lab", below, 4, N_STEPS)
    assert (np.abs(moved - want_b) / scale).max() <= BAR
    if envelope == "square":  # (its width slot is the grid term alone: what the T slot held at the tie)
        assert np.abs(moved[:, 2] - got[ties, 5]).max() <= 1e-9


@pytest.mark.parametrize("mode", P.MODES)
def test_the_w_slot_is_finite_and_right_at_w_equal_to_zero(mode):
    for envelope in ("gaussian", "drag", "cosine"):
        solves = P.seeded_solves(envelope, SEED, N_SOLVES)
        solves[[0, 3], 3] = 0.0
        got = jac(solves, envelope, mode, 4, N_STEPS, 4)
        want = PJ.scheme_jac(envelope, mode, solves, 4, N_STEPS)
        assert np.isfinite(got).all()
        assert np.abs(got[[0, 3], 0] - np.eye(2)).max() == 0.0  # no rotation: U = I exactly
        assert np.abs(got[[0, 3], 4]).max() > 1e-2  # ... and yet a derivative by w
        assert (np.abs(got - want).max(axis=(0, 2, 3)) / column_scale(want) <= BAR).all()


def test_every_refusal_returns_its_status_code():
    torch = N.require_gpu()
    lib = N.lib()
    solves = torch.zeros((2, 8), dtype=torch.float64, device=N.current_device())
    out = torch.zeros((2, 6, 2, 2), dtype=torch.complex128, device=N.current_device())
    sp, outp = C.c_void_p(solves.data_ptr()), C.c_void_p(out.data_ptr())
    INVALID, UNSUPPORTED = -1, -10  # (the codes of qmle_pulse_unitaries: tests/test_gpu_pulse.py)

    def call(d_solves=sp, n=2, env=0, mode=0, oc=1.0, oq=1.0, order=4, steps=8, lanes=0, d_out=outp):
        return lib.qmle_pulse_unitaries_jac(d_solves, n, env, mode, oc, oq, order, steps, lanes, d_out, None)

    for kw in (dict(order=3), dict(order=8), dict(env=5), dict(env=-1), dict(mode=3), dict(mode=-1)):
        assert call(**kw) == UNSUPPORTED, kw
    for kw in (dict(d_solves=None), dict(d_out=None), dict(n=0), dict(steps=0), dict(lanes=2), dict(lanes=128),
               dict(oc=float("inf")), dict(oq=float("nan")), dict(n=2 ** 30, lanes=64)):
        assert call(**kw) == INVALID, kw
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0  # nothing was launched
    with pytest.raises(N.Unsupported):
        N.pulse_unitaries_jac(np.zeros((2, 8)), "drag", "rwa", 1.0, 1.0, 3, 8)
    with pytest.raises(ValueError, match="unknown envelope"):
        N.pulse_unitaries_jac(np.zeros((1, 8)), "triangle", "rwa", 1.0, 1.0, 4, 8)
    with pytest.raises(ValueError, match="unknown mode"):
        N.pulse_unitaries_jac(np.zeros((1, 8)), "drag", "rotating", 1.0, 1.0, 4, 8)
    with pytest.raises(ValueError, match=r"\[n >= 1, 8\]"):
        N.pulse_unitaries_jac(np.zeros((1, 7)), "drag", "rwa", 1.0, 1.0, 4, 8)


# ---- pulses.solve_with_jacobian ----------------------------------------------------------------------------------------
def test_solve_with_jacobian_under_fixed_and_adaptive_solver_names():
    solves = P.seeded_solves("drag", SEED, N_SOLVES)
    Evolution._solver_defaults.update(solver="magnus4", magnus_steps=N_STEPS)
    U, J, steps = pulses.solve_with_jacobian(solves, "drag", "drive", P.OMEGA, P.OMEGA)
    want = PJ.scheme_jac("drag", "drive", solves, 4, N_STEPS)
    assert steps == N_STEPS and U.shape == (N_SOLVES, 2, 2) and J.shape == (N_SOLVES, 5, 2, 2)
    assert (np.abs(np.concatenate([U[:, None], J], 1) - want).max(axis=(0, 2, 3)) / column_scale(want) <= BAR).all()
    Evolution._solver_defaults.update(solver="magnus2")
    U2, J2, _ = pulses.solve_with_jacobian(solves, "drag", "drive", P.OMEGA, P.OMEGA)
    want2 = PJ.scheme_jac("drag", "drive", solves, 2, N_STEPS)
    assert (np.abs(np.concatenate([U2[:, None], J2], 1) - want2).max(axis=(0, 2, 3)) / column_scale(want2) <= BAR).all()
    Evolution._solver_defaults.update(solver="dopri8")
    Ua, Ja, steps_a = pulses.solve_with_jacobian(solves, "drag", "rwa", P.OMEGA, P.OMEGA)
    Ud, n, _ = P.doubling("drag", "rwa", solves, 2 * Evolution._options({})[0], first=32)
    assert steps_a == n  # the grid that the doubling accepted
    want_a = PJ.scheme_jac("drag", "rwa", solves, 4, n)
    assert (np.abs(np.concatenate([Ua[:, None], Ja], 1) - want_a).max(axis=(0, 2, 3)) / column_scale(want_a) <= BAR).all()


# ---- qoc with the default solver ---------------------------------------------------------------------------------------
# The NumPy solver that the CPU tests inject runs order 4 on 64 steps; the comparisons below put the GPU on that grid.
def fixed_grid():
    Evolution._solver_defaults.update(solver="magnus4", magnus_steps=64)


def make_qoc(**kw):
    return qoc.QOC(**{**qoc.default_qoc_params, "n_steps": 50, "scan_steps": 0, **kw})


def basis_scripts(fn, wires):
    return [Script(qoc._with_basis_prep(fn, k, wires), n_qubits=wires) for k in range(2 ** wires)]


def test_unitary_cost_gradient_of_crx_with_one_launch_per_evaluation():
    fixed_grid()
    q = make_qoc(n_samples=4)  # drag, rwa
    pulse_circuit, target_circuit = q.create_CRX()
    pp = np.asarray(PulseInformation.CRX.params, dtype=np.float64)
    args = (basis_scripts(pulse_circuit, 2), basis_scripts(target_circuit, 2), 4, 2)
    for cand in (pp, np.stack([pp, pp * 1.05, pp * 0.95])):
        before = qoc.LAUNCH_GROUPS
        values, grads = qoc.unitary_cost_fn(cand, *args, value_and_grad=True)
        assert qoc.LAUNCH_GROUPS == before + 1  # whatever the number of candidates
        want_v, want_g = qoc.unitary_cost_fn(cand, *args, value_and_grad=True, solver=PJ.solve_with_jacobian)
        for v, g, wv, wg in zip(values, grads, want_v, want_g):
            scale = max(1.0, float(np.abs(wg).max()))
            print("CRX unitary cost: value distance", np.abs(v - wv).max(), "gradient distance / scale",
                  np.abs(g - wg).max() / scale, "scale", scale)
            assert np.abs(v - wv).max() <= BAR and np.abs(g - wg).max() <= BAR * scale
            assert np.ndim(wv) == 0 or np.abs(wg[1:]).max() > 1e-3  # (the defaults themselves sit at an optimum)


STAGE_1 = dict(envelope="gaussian", n_steps=50, n_samples=4, n_restarts=3, learning_rate=0.003)  # tests/test_qoc_cpu.py


def stage_1_start():
    return np.asarray(PulseEnvelope.get("gaussian")["defaults"]["RX"], dtype=np.float64) * 1.1


def test_stage_1_end_to_end_against_the_cpu_run(tmp_path):
    """The case chosen in tests/test_qoc_cpu.py.  The final loss is compared with the CPU run's; how far two correct
    runs may part is measured by the CPU run itself, rerun from a start moved by 1e-13 relative, and 100 x that is
    allowed (measured on the MI355X: ``profiles/qoc.md``)."""
    fixed_grid()

    def run(solver, start, where):
        q = make_qoc(file_dir=str(where), solver=solver, **STAGE_1)
        best, history = q.optimize(wires=1)(q.create_RX)(start)
        return q, best, np.asarray(history)

    (tmp_path / "gpu").mkdir()
    before = qoc.LAUNCH_GROUPS
    q, best, history = run(None, stage_1_start(), tmp_path / "gpu")
    assert qoc.LAUNCH_GROUPS - before == 51  # the restarts' first losses, then one per step
    _, cpu_best, cpu_history = run(PJ.solve_with_jacobian, stage_1_start(), tmp_path / "cpu")
    _, _, moved_history = run(PJ.solve_with_jacobian, stage_1_start() * (1 + 1e-13), tmp_path / "cpu2")
    assert len(history) == STAGE_1["n_steps"] + 1 and np.isfinite(best).all()
    assert history.min() <= history[0] / 2
    rows = open(tmp_path / "gpu" / "qoc_results_gaussian.csv").read().strip().splitlines()
    assert len(rows) == 1 and rows[0].startswith("RX,")
    # the first step's gradient (all restarts) at the kernel bar
    pulse_circuit, target_circuit = q.create_RX()
    args = (basis_scripts(pulse_circuit, 1), basis_scripts(target_circuit, 1), 4, 1)
    starts = q._perturb_starts(stage_1_start())
    (_, _), grads = qoc.unitary_cost_fn(starts, *args, value_and_grad=True)
    (_, _), want = qoc.unitary_cost_fn(starts, *args, value_and_grad=True, solver=PJ.solve_with_jacobian)
    for g, w in zip(grads, want):
        assert np.abs(g - w).max() <= BAR * max(1.0, float(np.abs(w).max()))
    sensitivity = abs(moved_history.min() - cpu_history.min())
    distance = abs(history.min() - cpu_history.min())
    print("stage 1: first loss", history[0], "lowest", history.min(), "CPU lowest", cpu_history.min(),
          "distance", distance, "CPU sensitivity to 1e-13 of the start", sensitivity)
    assert distance <= 100 * sensitivity


def test_stage_0_costs_one_launch_per_scan_step_and_skips_non_finite_candidates(tmp_path):
    fixed_grid()
    q = make_qoc(file_dir=str(tmp_path), **{**STAGE_1, "scan_steps": 3, "scan_grid_size": 2,
                                            "scan_ranges": [(0.35, 1e40), (1.5, 1.8), (2.8, 3.1)]})
    pulse_circuit, target_circuit = q.create_RX()
    total = qoc.Cost(qoc.unitary_cost_fn, (0.5, 0.5), dict(
        pulse_basis_scripts=basis_scripts(pulse_circuit, 1), target_basis_scripts=basis_scripts(target_circuit, 1),
        n_samples=4, n_qubits=1)) + None
    before = qoc.LAUNCH_GROUPS
    best, (axes, landscape) = q.stage_0_opt(stage_1_start(), total)
    assert qoc.LAUNCH_GROUPS - before == 3 + 2  # scan_steps, the raw and the final evaluation: 8 candidates each
    assert len(landscape) == 4  # the four candidates of amplitude 1e40 come back NaN from the kernel and are skipped
    assert np.isfinite(best).all() and all(c[1][0] < 1.0 for c in landscape)
    assert Evolution._options({})[3] is True  # throw is restored


# ---- the reference's smoke and fidelity tests (tests/test_qoc.py) -------------------------------------------------------
def test_optimize_returns_params_and_history(tmp_path):
    """With the reference's defaults: the adaptive solver chooses the grid of every step."""
    params = {**qoc.default_qoc_params, "n_steps": 50, "scan_steps": 0, "file_dir": str(tmp_path)}
    q = qoc.QOC(**params)
    best_params, loss_history = q.optimize(wires=1)(q.create_RX)()
    assert best_params is not None and np.isfinite(best_params).all()
    assert len(loss_history) == params["n_steps"] + 1  # initial + n_steps


@pytest.mark.parametrize("w", [0.0, np.pi / 2])
@pytest.mark.parametrize("gate,wires", [("RX", 1), ("H", 1), ("CX", 2), ("CRX", 2)])
def test_pulse_gate_fidelity(gate, wires, w):
    q = qoc.QOC(**{**qoc.default_qoc_params, "n_steps": 50, "scan_steps": 0})
    pulse_circuit, target_circuit = getattr(q, "create_" + gate)()
    state_pulse = np.asarray(Script(pulse_circuit, n_qubits=wires).execute(
        type="state", args=(w, PulseInformation.gate_by_name(gate).params)))
    state_target = np.asarray(Script(target_circuit, n_qubits=wires).execute(type="state", args=(w,)))
    overlap = np.vdot(state_target, state_pulse)
    fidelity = np.abs(overlap) ** 2
    assert fidelity <= 1.0 + 1e-6, f"Fidelity of {gate} can't be larger 1 for w={w}"
    assert np.isclose(fidelity, 1.0, atol=1e-2), f"Fidelity too low for w={w}: {fidelity}"
    assert np.isclose(np.angle(overlap), 0.0, atol=1e-2), f"Phase off for w={w}: {np.angle(overlap)}"
