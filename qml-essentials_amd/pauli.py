"""Pauli-Clifford normal form of a recorded circuit (``PauliCircuit``, API of ``qml_essentials/pauli.py``).

A circuit of Pauli rotations and Clifford gates (what the common ansaetze are made of, Nemkov et al.,
Phys. Rev. A 108, 032406) is rewritten as Pauli rotations alone followed by Clifford gates alone, and the
Clifford gates are then absorbed into the observables: ``<0| U^+ O U |0>`` becomes the expectation of one evolved
Pauli word behind a sequence of rotations ``exp(-i theta_k P_k / 2)``.  That sequence is what
``coefficients.FourierTree`` expands.  Everything here is symbolic host bookkeeping on
:class:`operations.PauliWord`; angles are carried along untouched except for their sign, so a batched tape --
rotations whose angle is a ``(B,)`` column -- comes out with its columns (negated where a commutation flips the
generator's sign).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from .operations import RX, RY, RZ, Barrier, Hermitian, Operation, PauliRot, PauliWord, _gate_arg


class PauliCircuit:
    PAULI_ROTATION_GATES = (RX, RY, RZ, PauliRot)
    SKIPPABLE_OPERATIONS = (Barrier,)

    @staticmethod
    def from_parameterised_circuit(tape: List[Operation], observables: Optional[List[Operation]] = None,
                                   n_qubits: Optional[int] = None) -> Tuple[List[Operation], List[Operation]]:
        """``(rotations, observables)`` of the canonical circuit: the Pauli rotations in tape order and the
        observables with every Clifford gate of the tape absorbed."""
        observables = [] if observables is None else observables
        operations = PauliCircuit.get_clifford_pauli_gates(tape)
        if n_qubits is None:
            n_qubits = 1 + max((w for o in list(operations) + list(observables) for w in o.wires), default=-1)
        rotations, cliffords = PauliCircuit.commute_all_cliffords_to_the_end(operations, n_qubits)
        return rotations, PauliCircuit.cliffords_in_observable(cliffords, observables, n_qubits)

    @staticmethod
    def get_parameters(operations: List[Operation]) -> list:
        """The parameters of a tape, flattened: floats, or ``(B,)`` columns of a batched tape."""
        return [p for o in operations for p in o.parameters]

    @staticmethod
    def get_clifford_pauli_gates(tape: List[Operation]) -> List[Operation]:
        """The tape with barriers dropped and every composite gate replaced by its own decomposition into Clifford
        gates and Pauli rotations; a gate that has none raises ``NotImplementedError``."""
        out: List[Operation] = []
        for o in tape:
            if PauliCircuit._is_clifford(o) or PauliCircuit._is_pauli_rotation(o):
                out.append(o)
            elif PauliCircuit._is_skippable(o):
                continue
            else:
                try:
                    parts = o.decompose()
                except NotImplementedError:
                    raise NotImplementedError(
                        f"Gate {o.name} cannot be decomposed into Pauli rotations and Clifford gates. Consider using "
                        "a circuit ansatz that only uses RX, RY, RZ, PauliRot, Rot, and standard Clifford gates.")
                out.extend(PauliCircuit.get_clifford_pauli_gates(parts))
        return out

    @staticmethod
    def _is_skippable(operation: Operation) -> bool:
        return isinstance(operation, PauliCircuit.SKIPPABLE_OPERATIONS)

    @staticmethod
    def _is_clifford(operation: Operation) -> bool:
        return bool(getattr(operation, "is_clifford", False))

    @staticmethod
    def _is_pauli_rotation(operation: Operation) -> bool:
        return isinstance(operation, PauliCircuit.PAULI_ROTATION_GATES)

    @staticmethod
    def commute_all_cliffords_to_the_end(operations: List[Operation], n_qubits: int
                                         ) -> Tuple[List[Operation], List[Operation]]:
        """``(rotations, cliffords)`` with the same product as ``operations``: rotations first, Cliffords last, both in
        their tape order.  A rotation that stands behind the Cliffords ``C_1 .. C_m`` (tape order) satisfies
        ``R_P(t) C_m .. C_1 = C_m .. C_1 R_P'(t)`` with ``P' = C_1^+ .. C_m^+ P C_m .. C_1``: its generator is
        conjugated by the Cliffords in front of it, the nearest first.  ``P'`` is a bare word times +-1, and the sign
        goes into the angle."""
        rotations: List[Operation] = []
        cliffords: List[Operation] = []
        for o in operations:
            if PauliCircuit._is_clifford(o):
                cliffords.append(o)
                continue
            word = PauliWord.from_operation(o, n_qubits)
            for c in reversed(cliffords):
                if np.any(word.x[c.wires] | word.z[c.wires]):  # (a Clifford off the word's support commutes with it)
                    word = word.conjugate_by_clifford(c, adjoint_left=True)
            rotations.append(PauliCircuit._rotation_from_word(o.parameters[0], word) if cliffords else o)
        return rotations, cliffords

    @staticmethod
    def _evolve_clifford_rotation(clifford: Operation, pauli: Operation, n_qubits: int
                                  ) -> Tuple[Operation, Operation]:
        """Swap one Clifford (first on the tape) and one Pauli rotation (second): ``R_P C = C R_(C^+ P C)``."""
        if not set(clifford.wires) & set(pauli.wires):
            return pauli, clifford
        word = PauliWord.from_operation(pauli, n_qubits).conjugate_by_clifford(clifford, adjoint_left=True)
        return PauliCircuit._rotation_from_word(pauli.parameters[0], word), clifford

    @staticmethod
    def _rotation_from_word(theta, word: PauliWord) -> Operation:
        bare, lead = word.to_pauli_string_and_phase()
        if abs(lead.imag) > 1e-9:
            raise ValueError(f"conjugated generator {word!r} is not Hermitian")
        label, wires = PauliCircuit._remove_identities_from_paulistr(bare, list(range(word.n_qubits)))
        # (the (B,) column of a batched tape goes on as the batched scalar it is)
        return PauliRot(_gate_arg(theta * float(np.sign(lead.real))), label, wires=wires, record=False)

    @staticmethod
    def _remove_identities_from_paulistr(pauli_str: str, qubits: List[int]) -> Tuple[str, List[int]]:
        keep = [(c, q) for c, q in zip(pauli_str, qubits) if c != "I"]
        return "".join(c for c, _ in keep), [q for _, q in keep]

    @staticmethod
    def cliffords_in_observable(operations: List[Operation], original_obs: List[Operation], n_qubits: int
                                ) -> List[Operation]:
        """The observables in front of the Clifford tail ``C_m .. C_1``: ``O -> C_1^+ .. C_m^+ O C_m .. C_1``, the
        last Clifford first.  Each comes back as an explicit-matrix observable that also carries its symbolic word
        (``_pauli_word``) and, where its sign is +, its bare label (``_pauli_label``: the engine reads that tag as
        "the matrix IS this word", which a word with a minus sign is not)."""
        out = []
        for ob in original_obs:
            word = PauliWord.from_operation(ob, n_qubits)
            for c in reversed(operations):
                word = word.conjugate_by_clifford(c, adjoint_left=True)
            out.append(PauliCircuit._pauli_operation_from_word(word))
        return out

    @staticmethod
    def _pauli_operation_from_word(word: PauliWord) -> Operation:
        bare, lead = word.to_pauli_string_and_phase()
        label, wires = PauliCircuit._remove_identities_from_paulistr(bare, list(range(word.n_qubits)))
        if not label:
            obs = Hermitian(matrix=lead * np.eye(2, dtype=np.complex128), wires=[0], record=False)
        else:
            local = PauliWord.from_pauli_string(label, list(range(len(label))), len(label))
            obs = Hermitian(matrix=lead * local.to_matrix(), wires=wires, record=False)
        if lead == 1:
            obs._pauli_label = label or "I"
        obs._pauli_word = word
        return obs
