"""Quantum geometric tensor / QFI / Fubini-Study metric and the distance helpers: the parts that need
no GPU -- the state-derivative rules, the fold of the Gram matrix, the finite-difference fallback of
``qml_essentials_amd.math``, the distances, the argument checks of qmle_gram and the memory planner."""
import ctypes as C

import numpy as np
import pytest

from oracle import gates as OG
from qml_essentials_amd import _native as N
from qml_essentials_amd import math as qm
from qml_essentials_amd import memory
from qml_essentials_amd.script import Script

# every gate with a differentiable angle, its shift-rule class on the Operation side, and a matrix builder
GATES = [
    ("RX", "two", lambda t: OG.matrix("RX", (t,))),
    ("RY", "two", lambda t: OG.matrix("RY", (t,))),
    ("RZ", "two", lambda t: OG.matrix("RZ", (t,))),
    ("RXX", "two", lambda t: OG.matrix("RXX", (t,))),
    ("RYY", "two", lambda t: OG.matrix("RYY", (t,))),
    ("RZZ", "two", lambda t: OG.matrix("RZZ", (t,))),
    ("RZX", "two", lambda t: OG.matrix("RZX", (t,))),
    ("PauliRot", "two", lambda t: OG.matrix("PauliRot", (t, "XYZ"))),
    ("Rot[0]", "two", lambda t: OG.matrix("Rot", (t, 0.4, -1.1))),
    ("Rot[1]", "two", lambda t: OG.matrix("Rot", (0.3, t, -1.1))),
    ("Rot[2]", "two", lambda t: OG.matrix("Rot", (0.3, 0.4, t))),
    ("CRX", "four", lambda t: OG.matrix("CRX", (t,))),
    ("CRY", "four", lambda t: OG.matrix("CRY", (t,))),
    ("CRZ", "four", lambda t: OG.matrix("CRZ", (t,))),
    ("ControlledPhaseShift", "two", lambda t: OG.matrix("CPhase", (t,))),
]


@pytest.mark.parametrize("name,shift_rule,mat", GATES, ids=[g[0] for g in GATES])
@pytest.mark.parametrize("theta", [0.0, 0.83, -2.9, 7.1])
def test_state_derivative_rules_match_finite_differences(name, shift_rule, mat, theta):
    """dU/dtheta = sum_k c_k U(theta + s_k) as OPERATORS (not only for expectation values)."""
    rule = Script._STATE_RULES[Script.state_rule(name.split("[")[0], shift_rule)]
    got = sum(c * mat(theta + s) for s, c in rule)
    h = 1e-4
    want = (-mat(theta + 2 * h) + 8 * mat(theta + h) - 8 * mat(theta - h) + mat(theta - 2 * h)) / (12 * h)
    np.testing.assert_allclose(got, want, atol=1e-11)


def test_gates_without_a_state_rule_are_refused_by_name():
    with pytest.raises(NotImplementedError, match="DiagonalQubitUnitary"):
        Script.state_rule("DiagonalQubitUnitary", None)


def _qgt_direct(jac, psi):
    A = np.conj(jac.T) @ jac
    v = np.conj(jac.T) @ psi
    return A - np.outer(v, np.conj(v))


def test_fold_of_the_gram_matrix_equals_the_jacobian_form():
    """Q = C Gamma C^T - (C Gamma)_{:,0} (C Gamma)_{:,0}^H on random rows, against J^H J - v v^H."""
    rng = np.random.default_rng(3)
    B, R1, P, d = 3, 7, 4, 16
    S = rng.normal(size=(B, R1, d)) + 1j * rng.normal(size=(B, R1, d))
    Cf = rng.normal(size=(B, P, R1))
    Cf[:, :, 0] = 0.0  # (the unshifted row carries no derivative)
    gram = np.einsum("brk,bsk->brs", np.conj(S), S)
    got = Script.fold_qgt(Cf, gram)
    for b in range(B):
        jac = (Cf[b] @ S[b]).T  # (d, P): d_i psi = sum_r C_ir S_r
        np.testing.assert_allclose(got[b], _qgt_direct(jac, S[b, 0]), atol=1e-10)


# ---- the host fallback on the reference's known answers (tests/test_math.py:36-118) ----
def _ry_state(theta):
    t = theta[0]
    return np.array([np.cos(t / 2), np.sin(t / 2)], dtype=np.complex128)


def _two_ry_state(theta):
    q0 = np.array([np.cos(theta[0] / 2), np.sin(theta[0] / 2)], dtype=np.complex128)
    q1 = np.array([np.cos(theta[1] / 2), np.sin(theta[1] / 2)], dtype=np.complex128)
    return np.kron(q0, q1)


def _rho(p):
    psi = _two_ry_state(p)
    return np.outer(psi, np.conj(psi))


@pytest.mark.parametrize("theta", [0.0, 0.7, 1.3, np.pi / 2])
def test_fallback_single_ry(theta):
    F = qm.quantum_fisher_information(_ry_state, np.array([theta]))
    assert F.shape == (1, 1) and np.allclose(F, 1.0, atol=1e-8)
    assert qm.last_path == "fallback"
    g = qm.fubini_study_metric(_ry_state, np.array([theta]))
    assert g.shape == (1, 1) and np.allclose(g, 0.25, atol=1e-8)


def test_fallback_two_ry_identity_relation_symmetry_and_mixed_consistency():
    theta = np.array([0.7, 1.3])
    F = qm.quantum_fisher_information(_two_ry_state, theta)
    np.testing.assert_allclose(F, np.eye(2), atol=1e-8)
    g = qm.fubini_study_metric(_two_ry_state, np.array([0.4, 2.1]))
    F2 = qm.quantum_fisher_information(_two_ry_state, np.array([0.4, 2.1]))
    np.testing.assert_allclose(F2, 4 * g, atol=1e-8)
    np.testing.assert_allclose(F2, F2.T, atol=1e-8)
    assert np.min(np.linalg.eigvalsh(F2)) >= -1e-8
    np.testing.assert_allclose(qm.quantum_fisher_information(_rho, theta), F, atol=1e-8)


def test_fallback_shape_errors_and_density_rejection():
    with pytest.raises(ValueError):
        qm.quantum_fisher_information(lambda _p: np.ones((2, 3), dtype=np.complex128), np.array([0.1]))
    with pytest.raises(ValueError):
        qm.fubini_study_metric(_rho, np.array([0.7, 1.3]))


# ---- distances (math.py:60-208) ----
def test_fidelity_trace_distance_phase_difference_analytic():
    zero, one = np.array([1, 0], complex), np.array([0, 1], complex)
    plus = np.array([1, 1], complex) / np.sqrt(2)
    assert np.isclose(qm.fidelity(zero, plus), 0.5)
    assert np.isclose(qm.fidelity(zero, 3 * zero), 1.0)  # normalised first
    np.testing.assert_allclose(qm.fidelity(np.stack([zero, one, plus]), plus), [0.5, 0.5, 1.0])  # (3, 2): batch
    rz, ro = np.outer(zero, zero.conj()), np.outer(one, one.conj())
    rm = np.eye(2) / 2
    assert np.isclose(qm.fidelity(rz, rm), 0.5)
    assert np.isclose(qm.fidelity(rz, ro), 0.0, atol=1e-12)
    np.testing.assert_allclose(qm.fidelity(np.stack([rz, rz]), np.stack([rz, rm])), [1.0, 0.5])
    assert np.isclose(qm.trace_distance(rz, ro), 1.0)
    assert np.isclose(qm.trace_distance(rz, rm), 0.5)
    np.testing.assert_allclose(qm.trace_distance(np.stack([rz, rz]), np.stack([rz, ro])), [0.0, 1.0])
    assert np.isclose(qm.phase_difference(zero, np.exp(0.7j) * zero), 0.7)
    np.testing.assert_allclose(qm.phase_difference(np.stack([zero, plus, one]), np.stack([-1j * zero, plus, one])),
                               [-np.pi / 2, 0.0, 0.0], atol=1e-12)
    with pytest.raises(ValueError):
        qm.fidelity(zero, rz)
    with pytest.raises(ValueError):
        qm.trace_distance(rz, np.eye(4))
    assert qm.logm_v is not None


# ---- native entry points refuse bad arguments without a device ----
def test_gram_entry_points_refuse_bad_arguments_before_touching_a_device():
    lib = N.lib()
    null = C.c_void_p(None)
    fake = C.c_void_p(1 << 20)  # never dereferenced: every case below fails its host-side check
    out = C.c_void_p(2 << 20)
    for fn in (lib.qmle_gram, lib.qmle_gram_f64):
        assert fn(null, fake, 4, 1, 3, 3, 48, 48, out, null, 0, null) == -1       # no a
        assert fn(fake, fake, 4, 1, 3, 3, 48, 48, null, null, 0, null) == -1      # no out
        assert fn(fake, fake, 4, 1, 0, 3, 48, 48, out, null, 0, null) == -1       # rows_a 0
        assert fn(fake, fake, 4, 1, 3, -2, 48, 48, out, null, 0, null) == -1      # rows_b < 0
        assert fn(fake, fake, 0, 1, 3, 3, 48, 48, out, null, 0, null) == -1       # n_qubits 0
        assert fn(fake, fake, 31, 1, 3, 3, 48, 48, out, null, 0, null) == -1      # n_qubits 31
        assert fn(fake, fake, 4, 65536, 3, 3, 48, 48, out, null, 0, null) == -1   # too many groups
        assert fn(fake, fake, 4, 2, 3, 3, 16, 16, out, null, 0, null) == -1       # groups overlap
    # long rows: a partial per chunk -- a workspace smaller than the query's answer is refused
    wsb = lib.qmle_gram_workspace_bytes(20, 1, 241, 241)
    assert wsb > 0
    assert lib.qmle_gram(fake, fake, 20, 1, 241, 241, 0, 0, out, fake, wsb - 1, null) == -1
    assert lib.qmle_gram_workspace_bytes_f64(20, 1, 241, 241) > 0
    # many short groups: one chunk per row, the result is written directly
    assert lib.qmle_gram_workspace_bytes(6, 10000, 37, 37) == 0
    assert lib.qmle_gram_workspace_bytes(0, 1, 3, 3) == 0


# ---- memory planner ----
def test_metric_plan_chunks_points_and_splits_rows(monkeypatch):
    monkeypatch.setattr(memory, "available_memory_bytes", lambda: 64 << 30)
    chunk, block = memory.metric_plan(10, 37, 100000)
    assert block == 37 and 1 <= chunk <= 65535
    chunk, block = memory.metric_plan(20, 241, 4)
    assert block == 241 and 1 <= chunk <= 4
    per = memory.estimate_peak_bytes(20, 241, "state")
    assert chunk * per <= 0.8 * (64 << 30)
    # 28 qubits: one state is 2 GiB, 241 of them do not fit in 51 GiB -> row blocks, two at a time
    chunk, block = memory.metric_plan(28, 241, 3)
    assert chunk == 1 and 1 <= block < 241
    assert 2 * block * (2**28) * 8 <= 0.8 * (64 << 30)
    # complex128 amplitudes: half as many rows per block
    _, block64 = memory.metric_plan(28, 241, 3, x64=True)
    assert block64 < block
