"""CPU: ``operations.PauliWord`` against dense matrices -- products, commutation and Clifford conjugation in both
directions, exhaustively over every word (all four phases) on 1 and 2 qubits and on a seeded sample on 3 -- and the
three ``TestPauliCircuit`` cases of the reference's ``tests/test_pauli.py``."""
import itertools

import numpy as np
import pytest

from fourier_dag_reference import dense_expectations
from qml_essentials_amd.operations import (CX, CY, CZ, H, RX, RY, RZ, S, SWAP, PauliRot, PauliWord, PauliX, PauliY,
                                           PauliZ, _pauli_word_matrix, embed_matrix)
from qml_essentials_amd.pauli import PauliCircuit


def dense(word: PauliWord) -> np.ndarray:
    """The word as a matrix, by another road than ``to_matrix``: the bare string's Kronecker product times its phase."""
    label, lead = word.to_pauli_string_and_phase()
    return lead * _pauli_word_matrix(label)


def all_words(n):
    return [PauliWord.from_string_and_phase("".join(s), 1j ** k)
            for s in itertools.product("IXYZ", repeat=n) for k in range(4)]


def sample_words(n, count, seed):
    rng = np.random.default_rng(seed)
    return [PauliWord.from_string_and_phase("".join(rng.choice(list("IXYZ"), size=n)), 1j ** int(rng.integers(4)))
            for _ in range(count)]


WORDS = {1: all_words(1), 2: all_words(2), 3: sample_words(3, 40, seed=3)}


@pytest.mark.parametrize("n", [1, 2, 3])
def test_compose_and_commutation_match_dense_matrices(n):
    words = WORDS[n]
    partners = words if n == 1 else words[::5]
    for w in words:
        assert np.array_equal(dense(w), w.to_matrix())
        for v in partners:
            assert np.array_equal(dense(w.compose(v)), dense(w) @ dense(v)), (w, v)
            commute = np.array_equal(dense(w) @ dense(v), dense(v) @ dense(w))
            assert w.commutes_with(v) == commute, (w, v)


def _gates(n):
    last = n - 1
    gates = [H(wires=0, record=False), S(wires=last, record=False), PauliX(wires=0, record=False),
             PauliY(wires=last, record=False), PauliZ(wires=0, record=False)]
    if n >= 2:
        gates += [CX(wires=[0, last], record=False), CX(wires=[last, 0], record=False),
                  CZ(wires=[0, 1], record=False), SWAP(wires=[0, last], record=False),
                  CY(wires=[0, 1], record=False), CY(wires=[last, 0], record=False)]  # CY: the matrix fallback
    return gates


@pytest.mark.parametrize("adjoint_left", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_clifford_conjugation_matches_dense_matrices_in_both_directions(n, adjoint_left):
    for gate in _gates(n):
        c = embed_matrix(gate.matrix, gate.wires, list(range(n)))
        cd = np.conj(c).T
        for w in WORDS[n]:
            want = cd @ dense(w) @ c if adjoint_left else c @ dense(w) @ cd
            got = w.conjugate_by_clifford(gate, adjoint_left=adjoint_left)
            assert np.allclose(dense(got), want, atol=1e-14), (gate, w, got)


def test_only_cy_of_these_gates_takes_the_matrix_fallback(monkeypatch):
    calls = []
    original = PauliWord._conjugate_via_matrix
    monkeypatch.setattr(PauliWord, "_conjugate_via_matrix",
                        lambda self, c, adj: calls.append(c.name) or original(self, c, adj))
    word = PauliWord.from_pauli_string("XY", [0, 1], 2)
    for gate in _gates(2):
        word.conjugate_by_clifford(gate)
    assert calls == ["CY", "CY"]


def test_zero_expectation_and_round_trips():
    for n in (1, 2, 3):
        zero = np.zeros(2**n)
        zero[0] = 1.0
        for w in WORDS[n]:
            assert w.zero_expectation() == pytest.approx(zero @ dense(w) @ zero)
            assert w.is_diagonal == (not set(w.to_pauli_string()) & {"X", "Y"})
            label, lead = w.to_pauli_string_and_phase()
            assert PauliWord.from_string_and_phase(label, lead) == w
            assert PauliWord.from_matrix(w.to_matrix()) == w
            assert np.array_equal(w.xy_mask, [c in "XY" for c in label])
    w = PauliWord.from_pauli_string("YZ", [2, 0], 3)
    assert (w.to_pauli_string(), w.phase, w.n_qubits) == ("ZIY", 1, 3)
    assert repr(w) == "PauliWord(+iZIY)" and w.leading_phase() == 1
    assert PauliWord.identity(3).to_pauli_string() == "III"
    assert PauliWord.from_operation(PauliRot(0.1, "XZ", wires=[2, 0], record=False), 3).to_pauli_string() == "ZIX"
    assert PauliWord.from_operation(RY(0.1, wires=1, record=False), 2).to_pauli_string() == "IY"
    with pytest.raises(ValueError):
        PauliWord.from_matrix(np.array([[1, 1], [1, -1]]) / np.sqrt(2))


# ---- the reference's TestPauliCircuit --------------------------------------------------------------------------
def test_h_rz_commutes_to_rx():
    ops = [H(wires=0, record=False), RZ(0.7, wires=0, record=False)]
    pauli_gates, cliffords = PauliCircuit.commute_all_cliffords_to_the_end(ops, 1)
    assert len(pauli_gates) == 1
    assert PauliWord.from_operation(pauli_gates[0], 1).to_pauli_string() == "X"
    assert np.isclose(float(pauli_gates[0].parameters[0]), 0.7)
    assert len(cliffords) == 1 and cliffords[0].name == "H"


def test_evolved_observable_carries_symbolic_word():
    obs = PauliCircuit.cliffords_in_observable([CX(wires=[0, 1], record=False)], [PauliZ(wires=0, record=False)], 2)
    assert len(obs) == 1
    word = obs[0]._pauli_word
    assert isinstance(word, PauliWord)
    assert word.to_pauli_string() == "ZI"


def test_cz_is_clifford_and_commuted():
    ops = [RX(0.3, wires=0, record=False), CZ(wires=[0, 1], record=False), RY(0.5, wires=1, record=False)]
    obs = [PauliZ(wires=0, record=False)]
    ref = dense_expectations(ops, obs, 2)
    operations, observables = PauliCircuit.from_parameterised_circuit(list(ops), obs, n_qubits=2)
    assert all(PauliCircuit._is_pauli_rotation(o) for o in operations)
    got = dense_expectations(operations, observables, 2)
    assert np.allclose(got, ref, atol=1e-14)


def test_s_gate_moves_with_the_adjoint_on_the_left():
    """``R_X(t) S = S R_(S^+ X S)(t) = S R_Y(-t)``: S is the one tableau Clifford that is not its own inverse, so the
    direction of the conjugation shows."""
    ops = [S(wires=0, record=False), RX(0.3, wires=0, record=False)]
    rotations, cliffords = PauliCircuit.commute_all_cliffords_to_the_end(list(ops), 1)
    assert rotations[0].pauli_word == "Y" and rotations[0].parameters[0] == pytest.approx(-0.3)
    for ob in (PauliX, PauliY, PauliZ):
        obs = [ob(wires=0, record=False)]
        evolved = PauliCircuit.cliffords_in_observable(cliffords, obs, 1)
        assert np.allclose(dense_expectations(rotations, evolved, 1), dense_expectations(ops, obs, 1), atol=1e-14)
