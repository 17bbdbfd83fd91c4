"""CPU-only: the fixed-grid Magnus schemes and the step-doubling rule of ``tests/evolution_reference.py`` against
the DOP853 truth, the ``ParametrizedHamiltonian`` algebra (the cases of the reference's
``tests/test_jaqsi.py:999-1075``), ``Evolution`` options, tape behaviour, lowering of per-sample matrices to
``MAT1_ROW`` / ``MAT2_ROW``, plan validation and merging of the two opcodes, and the argument errors of
``qmle_evolve_magnus`` (statuses, no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import evolution_reference as R
from qml_essentials_amd import _native as N
from qml_essentials_amd import jaqsi as js
from qml_essentials_amd import operations as op
from qml_essentials_amd.batching import Batched
from qml_essentials_amd.evolution import Evolution
from qml_essentials_amd.simulation import LoweredTape
from qml_essentials_amd.tape import recording

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.seeded_cases()
_TRUTH = {}


def truth(name, case):
    if name not in _TRUTH:
        _TRUTH[name] = R.truth(case["H"], case["fns"], case["t0"], case["t1"])
    return _TRUTH[name]


# ---- the schemes against the truth -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_order_four_converges_at_fourth_order(name, case):
    """Error ratios above 8 per doubling of the grid (16 in the limit), measured at 32, 64 and 128 steps: on these
    pulses the error at 128 steps is 4e-9 .. 1e-7, above the 1e-10 where the truth's own error would show (the
    reference's criterion, tests/test_jaqsi.py:2593-2596)."""
    T = truth(name, case)
    errs = [np.abs(R.solve_fixed(case["H"], case["fns"], case["t0"], case["t1"], n, 4)[0] - T).max()
            for n in (32, 64, 128)]
    print(name, errs)
    assert errs[-1] > 1e-10
    assert errs[0] / errs[1] > 8 and errs[1] / errs[2] > 8, errs


@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_order_two_converges_at_second_order(name, case):
    T = truth(name, case)
    errs = [np.abs(R.solve_fixed(case["H"], case["fns"], case["t0"], case["t1"], n, 2)[0] - T).max()
            for n in (64, 128, 256)]
    assert errs[0] / errs[1] > 3 and errs[1] / errs[2] > 3, errs


@pytest.mark.parametrize("lanes", [4, 16, 64])
@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_the_split_over_lanes_changes_rounding_only(name, case, lanes):
    for order, n_steps in ((2, 65), (4, 63), (4, 3)):
        one = R.solve_fixed(case["H"], case["fns"], case["t0"], case["t1"], n_steps, order)
        cut = R.solve_fixed(case["H"], case["fns"], case["t0"], case["t1"], n_steps, order, lanes=lanes)
        assert np.abs(one - cut).max() < 1e-13


def rows_case(case, rows=3):
    """The case with `rows` rows that differ in pulse scale, start and step."""
    c = (R.case_dim2 if case["dim"] == 2 else R.case_dim4)(CASE_SEED[id(case)], rows)
    t0 = c["t0"] + 0.01 * np.arange(rows)
    t1 = c["t1"] + 0.3 * np.arange(rows)
    return c, t0, t1


CASE_SEED = {id(case): int(name.split("seed")[1]) for name, case in CASES}


@pytest.mark.parametrize("variant", sorted(R.VARIANTS))
@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_every_wrong_variant_is_far_from_the_right_answer(name, case, variant):
    """On every seeded case a variant applies to, it moves U by more than 1e-6 (measured: >= 1.9e-3) -- so a kernel
    that agrees with the right scheme to 1e-12 on these cases has none of these mistakes."""
    c, t0, t1 = rows_case(case)
    for order in (2, 4):
        if not R.variant_applies(variant, order, 3, 4):
            continue
        right = R.solve_fixed(c["H"], c["fns"], t0, t1, 64, order, lanes=4)
        wrong = R.solve_fixed(c["H"], c["fns"], t0, t1, 64, order, lanes=4, variant=variant)
        diff = np.abs(wrong - right).reshape(3, -1).max(axis=1)
        print(name, variant, order, diff)
        which = slice(1, None) if variant == "h_row0" else slice(None)  # (row 0 keeps its own h)
        assert diff[which].min() > 1e-6, (variant, order, diff)


@pytest.mark.parametrize("tol", [1e-6, 1.4e-8, 1e-10])
@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_doubling_rule_meets_its_tolerance_against_the_truth(name, case, tol):
    U, n, ok = R.doubling(case["H"], case["fns"], case["t0"], case["t1"], atol=tol, rtol=tol)
    err = np.abs(U[0] - truth(name, case)).max()
    print(name, tol, n, err)
    assert ok.all() and 32 <= n <= 2 ** 13
    assert err <= 2 * tol


def test_doubling_rule_fails_on_a_small_step_budget():
    name, case = CASES[0]
    U, n, ok = R.doubling(case["H"], case["fns"], case["t0"], case["t1"], 1e-10, 1e-10, max_steps=64)
    assert n == 64 and not ok.any() and np.isnan(U).all()
    U, n, ok = R.doubling(case["H"], case["fns"], case["t0"], case["t1"], 1e-2, 1e-2, max_steps=31)
    assert n == 0 and not ok.any() and np.isnan(U).all()


# ---- ParametrizedHamiltonian (reference tests/test_jaqsi.py:999-1075) ---------------------------------------------------
def herm(m, wires=0):
    return op.Hermitian(matrix=m, wires=wires, record=False)


def test_parametrized_hamiltonian_creation():
    def coeff(p, t):
        return p * t

    ph = coeff * herm(R.Z)
    assert isinstance(ph, op.ParametrizedHamiltonian) and isinstance(ph, js.ParametrizedHamiltonian)
    assert ph.n_terms == 1 and ph.coeff_fns == (coeff,) and ph.wires == [0]
    assert np.allclose(ph.H_mats[0], R.Z)


def test_parametrized_hamiltonian_non_callable_raises():
    with pytest.raises(TypeError, match="callable"):
        _ = 3.14 * herm(R.Z)


def test_parametrized_hamiltonian_multi_term_addition():
    def fx(p, t):
        return p[0]

    def fy(p, t):
        return p[0] * t

    ph = fx * herm(R.X) + fy * herm(R.Y)
    assert isinstance(ph, op.ParametrizedHamiltonian)
    assert ph.n_terms == 2 and ph.wires == [0] and ph.coeff_fns == (fx, fy)
    assert np.allclose(ph.H_mats[1], R.Y)


def test_parametrized_hamiltonian_wire_and_shape_mismatch_raise():
    def f(p, t):
        return 1.0

    with pytest.raises(ValueError, match="same wires"):
        _ = (f * herm(R.X, 0)) + (f * herm(R.X, 1))
    with pytest.raises(ValueError, match="same shape"):
        op.ParametrizedHamiltonian([(f, R.X, [0, 1]), (f, np.kron(R.X, R.X), [0, 1])])
    with pytest.raises(ValueError, match="at least one term"):
        op.ParametrizedHamiltonian([])


def test_parametrized_hamiltonian_neg_and_sub():
    def f(p, t):
        return 2.0

    ph = f * herm(R.X)
    neg = -ph
    assert neg.n_terms == 1 and np.isclose(neg.coeff_fns[0](None, 0.0), -2.0)
    sub = ph - ph
    assert sub.n_terms == 2
    assert np.isclose(sub.coeff_fns[0](None, 0.0) + sub.coeff_fns[1](None, 0.0), 0.0)
    with pytest.raises(TypeError):
        _ = ph + 1.0


# ---- Evolution options ---------------------------------------------------------------------------------------------------
def test_evolution_defaults_and_set_solver_defaults():
    assert Evolution is js.Evolution
    assert Evolution._valid_solvers == ("dopri8", "dopri5", "magnus2", "magnus4")
    assert Evolution._solver_defaults == {"max_steps": 2 ** 13, "throw": True, "solver": "dopri8",
                                          "magnus_steps": 256}
    prev = Evolution.set_solver_defaults(max_steps=100, throw=False, solver="magnus4", magnus_steps=8)
    try:
        assert prev == {"max_steps": 2 ** 13, "throw": True, "solver": "dopri8", "magnus_steps": 256}
        assert Evolution._solver_defaults == {"max_steps": 100, "throw": False, "solver": "magnus4",
                                              "magnus_steps": 8}
        assert Evolution.set_solver_defaults() == {}
    finally:
        Evolution.set_solver_defaults(**prev)
    assert Evolution._solver_defaults["solver"] == "dopri8"
    with pytest.raises(ValueError, match="Unknown solver"):
        Evolution.set_solver_defaults(solver="rk4")
    assert Evolution._solver_defaults["solver"] == "dopri8"


def test_evolution_option_errors():
    def f(p, t):
        return 1.0

    ph = f * herm(R.X)
    with pytest.raises(ValueError, match="Unknown solver"):
        ph.evolve(solver="euler")
    with pytest.raises(TypeError, match="evolve"):
        Evolution.evolve(op.PauliX(wires=0, record=False))
    with pytest.raises(TypeError, match="evolve"):
        Evolution.evolve("H")
    gate = (f * herm(R.X) + f * herm(R.Y)).evolve(solver="magnus4")
    with pytest.raises(ValueError, match="parameter set"):
        gate([None], 1.0)
    atol, rtol, max_steps, throw, solver, steps = Evolution._options({})
    assert (atol, rtol, max_steps, throw, solver, steps) == (1.4e-8, 1.4e-8, 2 ** 13, True, "dopri8", 256)
    from qml_essentials_amd import utils

    if hasattr(utils, "enable_x64"):
        utils.enable_x64(True)
        try:
            assert Evolution._options({})[:2] == (1e-10, 1e-10)
        finally:
            utils.enable_x64(False)


def test_coefficient_functions_are_called_once_on_all_node_times():
    from qml_essentials_amd import evolution as ev

    calls = []

    def f(p, t):
        calls.append(np.shape(t))
        return p * np.cos(t)

    t = ev._node_times(np.array([0.0, 0.5]), np.array([0.1, 0.2]), 4, 4)
    assert np.allclose(t, R.node_times([0.0, 0.5], [0.1, 0.2], 4, 4))
    got = ev._coefficients(f, Batched(np.array([1.0, 2.0])), t, True)
    assert len(calls) == 1 and got.shape == (2, 8)
    assert np.allclose(got, np.array([1.0, 2.0])[:, None] * np.cos(t))
    assert np.allclose(ev._coefficients(lambda p, t: 1.0, None, t, False), 1.0)  # a scalar result broadcasts
    assert np.allclose(ev._coefficients(lambda p, t: p, Batched(np.array([3.0, 4.0])), t, False),
                       np.array([[3.0], [4.0]]))

    def scalar_only(p, t):  # raises on an array: one call per node
        calls.append("s")
        return float(t) ** 2

    calls.clear()
    got = ev._coefficients(scalar_only, None, t[:1], False)
    assert np.allclose(got, t[:1] ** 2) and calls.count("s") == 1 + 8


# ---- tape behaviour, lowering ---------------------------------------------------------------------------------------
def test_a_hamiltonian_built_while_recording_leaves_nothing_on_the_tape():
    def f(p, t):
        return 1.0

    with recording() as tape:
        h = op.Hermitian(matrix=R.Z, wires=0)
        assert len(tape) == 1
        ph = f * h + f * op.Hermitian(matrix=R.X, wires=0)
        gate = op.Hermitian(matrix=R.Z, wires=0).evolve()
    assert len(tape) == 0 and ph.n_terms == 2 and callable(gate)
    with recording() as tape:  # a Hermitian that stays a gate / observable is recorded as before
        op.Hermitian(matrix=R.Z, wires=0)
    assert len(tape) == 1


def batch_of_unitaries(B, d, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(B, d, d)) + 1j * rng.normal(size=(B, d, d))
    return np.linalg.qr(a)[0]


def test_an_operation_with_a_per_sample_matrix_is_one_op_on_the_tape_and_lowers_to_row_opcodes():
    U1, U2 = batch_of_unitaries(5, 2), batch_of_unitaries(5, 4, 1)
    with recording() as tape:
        a = op.Operation(wires=1, matrix=U1, name="evolved")
        b = op.Operation(wires=[2, 0], matrix=U2)
    assert len(tape) == 2 and a.is_batched and b.is_batched
    name, wires, params, blob = a.lower(3)
    assert (name, wires, blob) == ("MAT1_ROW", [1], None) and len(params) == 8
    assert np.array_equal(np.stack(params, axis=1).reshape(5, 2, 2, 2)[..., 0], U1.real)
    assert np.array_equal(np.stack(params, axis=1).reshape(5, 2, 2, 2)[..., 1], U1.imag)
    name, wires, params, blob = b.lower(3)
    assert (name, wires, blob) == ("MAT2_ROW", [2, 0], None) and len(params) == 32
    assert np.array_equal(np.stack(params, axis=1).reshape(5, 4, 4, 2)[..., 1], U2.imag)
    low = LoweredTape([op.RZ(20.0, wires=1, record=False), a, b], 3)
    assert low.n_slots == 1 + 8 + 32
    assert low.ops_periodic == [True] + [False] * 40          # a matrix entry is never reduced mod 4 pi
    table = low.angle_table(5, dtype=np.float64)
    assert np.array_equal(table[:, 1:9].reshape(5, 2, 2, 2)[..., 0], U1.real)
    assert abs(table[0, 0]) < 2 * np.pi + 1e-9
    big = op.Operation(wires=0, matrix=30.0 * U1, record=False)  # entries beyond 4 pi stay what they are
    assert np.array_equal(LoweredTape([big], 1).angle_table(5, dtype=np.float64).reshape(5, 2, 2, 2)[..., 0],
                          30.0 * U1.real)
    from qml_essentials_amd.simulation import _tape_batch

    assert _tape_batch([a]) == 5
    with pytest.raises(ValueError, match="does not match"):
        op.Operation(wires=[0, 1], matrix=U1, record=False).lower(2)
    with pytest.raises(NotImplementedError):
        op.Operation(wires=[0, 1, 2], matrix=batch_of_unitaries(2, 8), record=False).lower(3)
    assert a.parameter_tangents == [[]] * 8  # a matrix given by the caller: a constant for every gradient
    a._matrix_tangent = None
    assert a.parameter_tangents == [None] * 8


def test_header_opcodes_of_the_row_gates_match_the_binding():
    header = open(os.path.join(ROOT, "include", "qmle_sv.h")).read()
    codes = dict(re.findall(r"QMLE_OP_([A-Z0-9_]+) = (\d+)", header))
    assert int(codes["MAT1_ROW"]) == N.OPCODES["MAT1_ROW"] == 28
    assert int(codes["MAT2_ROW"]) == N.OPCODES["MAT2_ROW"] == 29
    assert int(codes["_COUNT"]) == 30


def test_plan_validation_of_the_row_opcodes():
    N.Plan([("MAT1_ROW", [0], [0], -1)], 1, 8)
    N.Plan([("MAT1_ROW", [1], [3], -1)], 2, 11)          # the upper edge: slots 3 .. 10 of 11
    N.Plan([("MAT2_ROW", [0, 1], [2], -1)], 2, 34)
    with pytest.raises(ValueError, match="slot"):
        N.Plan([("MAT1_ROW", [1], [4], -1)], 2, 11)      # one past it
    with pytest.raises(ValueError, match="slot"):
        N.Plan([("MAT2_ROW", [0, 1], [3], -1)], 2, 34)
    with pytest.raises(ValueError, match="slot"):
        N.Plan([("MAT1_ROW", [0], [-1], -1)], 1, 8)
    with pytest.raises(ValueError, match="wires"):
        N.Plan([("MAT1_ROW", [0, 1], [0], -1)], 2, 8)
    with pytest.raises(ValueError, match="wires"):
        N.Plan([("MAT2_ROW", [0], [0], -1)], 2, 32)
    with pytest.raises(ValueError, match="duplicate"):
        N.Plan([("MAT2_ROW", [1, 1], [0], -1)], 2, 32)
    with pytest.raises(ValueError, match="range"):
        N.Plan([("MAT1_ROW", [2], [0], -1)], 2, 8)


def test_a_row_gate_merges_like_an_explicit_matrix():
    """Between two RZ on its wire a 1-qubit row gate becomes part of ONE 2x2 build group, exactly like MAT1; a
    2-qubit row gate takes the pending 1-qubit matrices of its wires, like MAT2."""
    for mat, slots, consts in (("MAT1_ROW", [1], None), ("MAT1", [], np.zeros(8, dtype=np.float32))):
        ops = [("RZ", [1], [0], -1), (mat, [1], slots, -1 if consts is None else 0), ("RZ", [1], [9], -1),
               ("RX", [0], [10], -1)]
        p = N.Plan(ops, 3, 11, consts)
        assert p.stats()["n_lowered"] == 2 and p.describe()["build_groups"] == 2, mat
    for mat, slots, consts in (("MAT2_ROW", [2], None), ("MAT2", [], np.zeros(32, dtype=np.float32))):
        ops = [("RX", [0], [0], -1), ("RY", [2], [1], -1), (mat, [2, 0], slots, -1 if consts is None else 0),
               ("RZ", [0], [34], -1)]
        p = N.Plan(ops, 3, 35, consts)
        assert p.stats()["n_lowered"] == 1 and p.describe()["build_groups"] == 1, mat
    # dense, not diagonal, not a permutation: nothing of a row gate is folded into the observables
    tail = [("H", [0], [], -1), ("MAT1_ROW", [0], [0], -1)]
    assert N.Plan(tail, 1, 8).expval_child() is None


def test_refusals_without_a_device():
    """A noisy tape and the adjoint sweep refuse a per-sample matrix with the errors they document."""
    from qml_essentials_amd import adjoint
    from qml_essentials_amd.simulation import doubled_tape

    a = op.Operation(wires=0, matrix=batch_of_unitaries(3, 2), record=False)
    with pytest.raises(NotImplementedError, match="density-matrix mode"):
        doubled_tape([a, op.BitFlip(0.1, wires=0)], 1)
    low = LoweredTape([a], 1)
    with pytest.raises(adjoint.AdjointUnsupported, match="MAT1_ROW"):
        adjoint.build_reverse(low, [None], [False] * 8)


def test_evolve_magnus_argument_errors_are_statuses_without_a_device():
    lib = N.lib()
    null = C.c_void_p(None)
    H = np.zeros((1, 2, 2), dtype=np.complex128)
    hp = C.c_void_p(H.ctypes.data)
    one = C.c_void_p(8)  # a non-NULL pointer that is never followed: every call below is refused first

    def call(h=hp, n_terms=1, dim=2, coef=one, hh=one, rows=1, order=4, n_steps=1, lanes=0, f64=1, out=one):
        return lib.qmle_evolve_magnus(h, n_terms, dim, coef, hh, rows, order, n_steps, lanes, f64, out, null)

    assert call(dim=3) == -10 and call(dim=8) == -10 and call(dim=0) == -10   # QMLE_ERR_UNSUPPORTED
    assert call(order=3) == -10
    assert call(n_steps=0) == -1 and call(n_steps=-4) == -1                    # QMLE_ERR_INVALID_ARG
    assert call(rows=0) == -1 and call(n_terms=0) == -1 and call(n_terms=17) == -1
    assert call(lanes=2) == -1 and call(lanes=128) == -1 and call(f64=2) == -1
    assert call(h=null) == -1 and call(coef=null) == -1 and call(hh=null) == -1 and call(out=null) == -1
    assert call(rows=2 ** 30, lanes=64) == -1
    # lanes_per_row = 0: one lane per row when the rows fill the card, else the widest split without idle lanes
    assert lib.qmle_evolve_lanes(102400, 256) == 1
    assert lib.qmle_evolve_lanes(1, 8192) == 64 and lib.qmle_evolve_lanes(1, 3) == 1
    assert lib.qmle_evolve_lanes(1, 16) == 16 and lib.qmle_evolve_lanes(5000, 256) == 16
    assert lib.qmle_evolve_lanes(0, 1) == -1
    with pytest.raises(NotImplementedError):
        N.check(-10, "qmle_evolve_magnus")
