"""The matrix-cotangent reference of tests/matrix_cotangent_reference.py on its own, and the host side of the feature.

* ``2 Re sum G_ref D`` against a 4th-order central difference of the complex128 cost along random directions ``D``
  of the gate's matrix.  The cost is a quadratic polynomial in the step (the state is linear in the entries), so the
  quotient has no truncation error: what is left is rounding, ``~ 1e-16 |C| / h``, bounded by comparing the step with
  its double as tests/test_adjoint_reference_cpu.py does.  Bound 1e-9 at h = 1e-3, |C| <= sum |w| <= 8.
* Every named wrong variant of ``G`` differs from ``G_ref`` by at least 100 x the complex64 tolerance of the GPU
  route tests (4e-6 up to 13 qubits, 1e-5 at 14, times ``max(1, sum |w|)`` of the row), in every row of every case
  under both seeds: a kernel that computes one of them cannot pass tests/test_gpu_matrix_cotangent.py.
* ``adjoint.build_reverse`` reverses a per-sample one-wire matrix into the daggered column map and its sign vector.
* ``Model.gradient`` refuses the parameter-shift rule in pulse mode, naming the reason.
"""
import numpy as np
import pytest

from tests import adjoint_reference as R
from tests import matrix_cotangent_reference as M

CPU_CASES = [name for name, c in M.cases().items() if not name.startswith("lds_deep")]
VARIANTS = ["transposed", "conjugated", "psi behind the gate", "lambda in front of the gate", "factor 1 instead of 2",
            "wire order reversed"]


def c64_tolerance(n):
    """tests/test_gpu_adjoint_routes.tolerance(n, False), restated (that module needs a GPU to import)"""
    return 4e-6 if n <= 13 else 1e-5


@pytest.mark.parametrize("seed", ["z", "pauli"])
@pytest.mark.parametrize("name", ["lds_n2_b3", "lds_n3_b3", "stream_n5"])
def test_reference_cotangent_equals_the_difference_quotient(name, seed):
    case = M.cases()[name]
    mats, w = M.seed_observables(case, seed)
    _grad, cot = M.case_reference(name, seed)
    rng = np.random.default_rng(11)
    worst = 0.0
    for b in range(case.theta.shape[0]):
        tape = M.tape_of(case.spec, case.theta[b], b)
        for k, g in enumerate(case.mats):
            u = np.asarray(tape[g][2][0], dtype=np.complex128)
            for _ in range(3):
                d = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
                want = 2.0 * np.real(np.sum(cot[b, k] * d))

                def f(s):
                    return M.cost_of(R.run_from(R.zero_state(case.n), M.replaced(tape, g, u + s * d), case.n), case.n,
                                     mats, w[b])

                d1, d2 = R.central_difference(f, 1e-3), R.central_difference(f, 2e-3)
                worst = max(worst, abs(want - d1), abs(d2 - d1))
                assert abs(want - d1) <= 1e-9 and abs(d2 - d1) <= 1e-9, (name, seed, b, k, want, d1, d2)
    print(name, seed, "max |2 Re sum G_ref D - D(h)|, |D(2h) - D(h)|", worst)


@pytest.mark.parametrize("seed", ["z", "pauli"])
@pytest.mark.parametrize("name", CPU_CASES)
def test_wrong_variants_are_told_apart(name, seed):
    """the sweep's own construction agrees with G_ref to rounding; each wrong variant is far from it in every row"""
    case = M.cases()[name]
    mats, w = M.seed_observables(case, seed)
    _grad, cot = M.case_reference(name, seed)
    for b in range(case.theta.shape[0]):
        tape = M.tape_of(case.spec, case.theta[b], b)
        scale = max(1.0, np.abs(w[b]).sum())
        gap = dict.fromkeys(VARIANTS, 0.0)
        for k, g in enumerate(case.mats):
            forms = M.adjoint_style(tape, g, case.n, mats, w[b])
            assert np.abs(forms["right"] - cot[b, k]).max() <= 1e-13 * scale
            assert np.abs(cot[b, k]).max() <= scale * (1 + 1e-12)  # |G[a][c]| <= |lambda| |psi| <= sum |w|
            for v in VARIANTS:
                gap[v] = max(gap[v], np.abs(forms[v] - cot[b, k]).max() / scale)
        print(name, seed, "row", b, {v: round(x, 4) for v, x in gap.items()})
        for v in VARIANTS:
            assert gap[v] >= 100 * c64_tolerance(case.n), (name, seed, b, v, gap[v])


def test_angle_gradients_of_the_cases_are_not_vacuous():
    """the angle columns that the same sweep returns: no differentiated angle of the small cases vanishes"""
    for name in ("lds_n2_b3", "lds_n3_b3", "stream_n5"):
        case = M.cases()[name]
        for seed in ("z", "pauli"):
            grad, _ = M.case_reference(name, seed)
            assert np.abs(grad[:, case.wanted]).max(axis=0).min() >= 1e-3, (name, seed)


def test_build_reverse_daggers_a_per_sample_matrix():
    """MAT1_ROW -> MAT1_ROW on the daggered columns: reverse entry (r, c, re) = forward (c, r, re), reverse entry
    (r, c, im) = - forward (c, r, im); angles keep sign -1; the flagged gates are numbered in tape order"""
    from qml_essentials_amd import adjoint
    from qml_essentials_amd import operations as op
    from qml_essentials_amd.batching import Batched
    from qml_essentials_amd.simulation import LoweredTape

    rng = np.random.default_rng(3)
    u = np.stack([R.unitary(rng, 1) for _ in range(3)])
    const = R.unitary(rng, 1)
    tape = [op.RX(0.3, wires=0, record=False), op.Operation(wires=1, matrix=u, record=False),
            op.Operation(wires=0, matrix=const, record=False),
            op.RY(Batched(np.array([0.1, 0.2, 0.3])), wires=1, record=False)]
    low = LoweredTape(tape, 2)
    assert [o[0] for o in low.ops] == ["RX", "MAT1_ROW", "MAT1", "RY"] and low.n_slots == 10
    rev_ops, terms, rev_src, rev_sign, mat_out = adjoint.build_reverse(
        low, adjoint._op_blobs(low, True), [True] + [False] * 8 + [True], [False, True, True, False])
    assert [o.name for o in rev_ops] == ["RY", "MAT1", "MAT1_ROW", "RX"] and len(terms) == 4
    assert mat_out == [-1, 1, 0, -1]
    # forward slots: RX 0, matrix entries 1..8 ((r, c, part) -> 1 + (2 r + c) 2 + part), RY 9
    assert rev_src == [9] + [1 + (2 * c + r) * 2 + part for r in range(2) for c in range(2) for part in range(2)] + [0]
    assert rev_sign == [-1.0] + [1.0, -1.0] * 4 + [-1.0]
    table = low.angle_table(3, dtype=np.float64)
    rev_table = table[:, rev_src] * np.asarray(rev_sign)
    got = (rev_table[:, 1:9:2] + 1j * rev_table[:, 2:9:2]).reshape(3, 2, 2)
    assert np.array_equal(got, np.conj(np.swapaxes(u, 1, 2)))
    blob = np.asarray(rev_ops[1].lower(2)[3]).reshape(2, 2, 2)
    assert np.array_equal(blob[..., 0] + 1j * blob[..., 1], const.conj().T)
    # the values the reverse tape itself carries are those of the table rule
    assert np.array_equal(LoweredTape(rev_ops, 2).angle_table(3, dtype=np.float64), rev_table)
    with pytest.raises(adjoint.AdjointUnsupported, match="one-wire matrix"):
        adjoint.build_reverse(low, adjoint._op_blobs(low, True), [False] * 10, [True, False, False, False])
    two = LoweredTape([op.Operation(wires=[0, 1], matrix=np.stack([R.unitary(rng, 2)] * 3), record=False)], 2)
    with pytest.raises(adjoint.AdjointUnsupported, match="two-wire"):
        adjoint.build_reverse(two, [None], [False] * 32, [False])


def test_pulse_mode_refuses_the_parameter_shift_rule():
    from qml_essentials_amd.model import Model

    model = Model(n_qubits=2, n_layers=1, circuit_type="Hardware_Efficient")
    with pytest.raises(NotImplementedError, match="no shift rule"):
        model.gradient(inputs=np.array([0.5]), gate_mode="pulse", method="parameter-shift")
    with pytest.raises(NotImplementedError, match="no shift rule"):
        model.gradient(inputs=np.array([0.5]), gate_mode="pulse", wrt="pulse_params")  # (the default method)
    with pytest.raises(ValueError, match="gate_mode='pulse'"):
        model.gradient(inputs=np.array([0.5]), wrt="pulse_params", method="adjoint")
