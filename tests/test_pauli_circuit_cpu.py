"""CPU: ``pauli.PauliCircuit`` on recorded model tapes.  The canonical form -- Pauli rotations alone, the Clifford gates
absorbed into the observables -- must give the expectation values of the original tape, both computed as dense
complex128 ``<0| U^+ O U |0>`` from ``Operation.matrix``; 1e-13 is a hundred times the rounding of ~50 gates on 8
amplitudes."""
import warnings

import numpy as np
import pytest

from fourier_dag_reference import dense_expectations
from qml_essentials_amd.ansaetze import Ansaetze
from qml_essentials_amd.model import Model
from qml_essentials_amd.operations import CCX, CX, RX, RY, ControlledPhaseShift, PauliRot, PauliWord, PauliZ
from qml_essentials_amd.pauli import PauliCircuit

CASES = [(cls.__name__, 3, 1) for cls in Ansaetze.get_available()] + [("Circuit_19", 3, 2)]


def _model(name, n_qubits, n_layers, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (topologies that skip a block at 3 qubits say so)
        return Model(n_qubits=n_qubits, n_layers=n_layers, circuit_type=name, output_qubit=-1, **kw)


@pytest.mark.parametrize("name, n_qubits, n_layers", CASES, ids=[f"{c[0]}-{c[1]}q-{c[2]}l" for c in CASES])
def test_canonical_form_keeps_every_expectation_value(name, n_qubits, n_layers):
    model = _model(name, n_qubits, n_layers)
    tape, batch = model.record_tape(model.params, np.array([0.7]))
    assert batch == 1
    _, obs = model._build_obs()
    rotations, evolved = PauliCircuit.from_parameterised_circuit(list(tape), obs, n_qubits)  # every ansatz decomposes
    assert all(PauliCircuit._is_pauli_rotation(o) for o in rotations)
    assert all(hasattr(o, "_pauli_word") for o in evolved) and len(evolved) == len(obs) == n_qubits
    want = dense_expectations(tape, obs, n_qubits)
    got = dense_expectations(rotations, evolved, n_qubits)
    assert np.max(np.abs(got - want)) < 1e-13
    assert np.max(np.abs(got.imag)) < 1e-13
    assert len(PauliCircuit.get_parameters(rotations)) == len(rotations)


@pytest.mark.parametrize("gate", [lambda: CCX(wires=[0, 1, 2], record=False),
                                  lambda: ControlledPhaseShift(0.3, wires=[0, 1], record=False)], ids=["CCX", "CPhase"])
def test_a_gate_without_a_decomposition_raises(gate):
    tape = [RX(0.1, wires=0, record=False), gate(), RY(0.2, wires=1, record=False)]
    with pytest.raises(NotImplementedError, match="cannot be decomposed"):
        PauliCircuit.from_parameterised_circuit(tape, [PauliZ(wires=0, record=False)], 3)


def test_a_batched_tape_keeps_its_columns_and_signs():
    """One recording for B = 3 parameter sets: every canonical rotation of the batched tape carries, sample by sample,
    the angle that the canonical form of that sample's own tape carries -- including the columns whose sign a
    commutation flipped (Circuit_19's controlled rotations decompose into RZ(-t/2) between CX gates)."""
    model = _model("Circuit_19", 3, 1)
    model.initialize_params(repeat=3)
    params = np.array(model.params)
    tape, batch = model.record_tape(params, np.array([0.4]))
    assert batch == 3
    rotations, _ = PauliCircuit.from_parameterised_circuit(list(tape), [], 3)
    cols = PauliCircuit.get_parameters(rotations)
    assert any(np.ndim(c) == 1 for c in cols)
    for b in range(3):
        single, _ = model.record_tape(params[b], np.array([0.4]))
        ref_rot, _ = PauliCircuit.from_parameterised_circuit(list(single), [], 3)
        assert len(ref_rot) == len(rotations)
        for got, ref, raw in zip(rotations, ref_rot, cols):
            assert PauliWord.from_operation(got, 3) == PauliWord.from_operation(ref, 3)
            assert np.broadcast_to(raw, (3,))[b] == pytest.approx(float(ref.parameters[0]), abs=1e-15)
    # the hand-made case: a CX in front flips nothing, an S in front turns RX(t) into RY(-t), column and all
    from qml_essentials_amd.batching import Batched
    from qml_essentials_amd.operations import S

    column = np.array([0.1, -0.7, 2.0])
    hand = [S(wires=0, record=False), CX(wires=[0, 1], record=False), RX(Batched(column), wires=0, record=False)]
    rot, _ = PauliCircuit.commute_all_cliffords_to_the_end(hand, 2)
    assert isinstance(rot[0], PauliRot) and rot[0].pauli_word == "YX" and rot[0].wires == [0, 1]
    assert np.array_equal(rot[0].parameters[0], -column)


def test_pauli_rot_decomposition_equals_its_matrix():
    """``PauliRot.decompose()`` -- the form in which the engine runs words without an opcode -- against
    ``PauliRot.matrix`` for every word over X, Y, Z (and I) on 1 to 3 wires, global phase included; the angle and its
    tangents sit on the one RZ."""
    import itertools

    from qml_essentials_amd.batching import Batched
    from qml_essentials_amd.operations import RZ, embed_matrix

    wires_of = {1: [1], 2: [2, 0], 3: [1, 2, 0]}
    for k in (1, 2, 3):
        for letters in itertools.product("IXYZ", repeat=k):
            word = "".join(letters)
            if set(word) == {"I"}:
                with pytest.raises(NotImplementedError):
                    PauliRot(0.37, word, wires=wires_of[k], record=False).decompose()
                continue
            gate = PauliRot(-1.23, word, wires=wires_of[k], record=False)
            u = np.eye(8, dtype=np.complex128)
            parts = gate.decompose()
            for g in parts:
                assert len(g.wires) <= 2
                u = embed_matrix(g.matrix, g.wires, [0, 1, 2]) @ u
            assert np.max(np.abs(u - embed_matrix(gate.matrix, gate.wires, [0, 1, 2]))) < 1e-14, word
            assert sum(isinstance(g, RZ) for g in parts) == 1
    leaf = Batched.leaf(np.array([[0.1], [0.7]]), 0)
    gate = PauliRot(leaf[0] * 3.0, "XZY", wires=[0, 1, 2], record=False)
    (core,) = [g for g in gate.decompose() if isinstance(g, RZ)]
    assert np.array_equal(core.parameters[0], np.array([0.1, 0.7]) * 3.0)
    assert core.parameter_tangents == gate.parameter_tangents and gate.parameter_tangents[0]


def test_engine_tape_expands_only_words_without_an_opcode():
    from qml_essentials_amd.batching import Batched
    from qml_essentials_amd.script import Script

    column = Batched(np.array([0.1, 0.2]))

    def circuit(theta):
        RX(0.3, wires=0)
        PauliRot(0.4, "XZ", wires=[0, 1])      # batch-constant, two wires: stays (an explicit matrix)
        PauliRot(theta, "YY", wires=[0, 1])    # has an opcode: stays
        PauliRot(theta, "XZ", wires=[0, 1])    # per-sample angle, no opcode: expanded
        PauliRot(0.5, "XZX", wires=[0, 1, 2])  # three wires: expanded

    script = Script(circuit, n_qubits=3)
    raw = script._record(column)
    tape = script._record_for_engine(column)
    assert [o.name for o in raw] == ["RX", "PauliRot", "PauliRot", "PauliRot", "PauliRot"]
    assert [(o.name, getattr(o, "pauli_word", None)) for o in tape[:3]] == [("RX", None), ("PauliRot", "XZ"),
                                                                            ("PauliRot", "YY")]
    assert len(tape) > len(raw) and not any(isinstance(o, PauliRot) for o in tape[3:])
    assert all(len(o.wires) <= 2 for o in tape) and all(o.lower(3) is not None for o in tape)
    plain = Script(lambda: RX(0.3, wires=0), n_qubits=1)
    assert [o.name for o in plain._record_for_engine()] == ["RX"]
