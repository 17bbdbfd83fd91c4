"""Quantum optimal control: tune the pulse parameters of a gate until its pulse-level circuit reproduces the target
unitary -- the per-gate API of ``qml_essentials/qoc.py`` (``Cost``, ``CostFnRegistry``, the cost functions, ``QOC`` with
``stage_0_opt`` / ``stage_1_opt`` / ``optimize`` / ``create_<G>``, ``default_qoc_params``).

Derivatives.  The reference differentiates through its ODE solver with ``jax.grad``.  Here every cost function has a
hand-written gradient (``value_and_grad=True`` -> ``(values, grads)``, ``grads`` ``[..., n_params]`` per value), and
the one expensive ingredient -- the pulse solves -- comes with its exact grid sensitivities from ONE launch of
``qmle_pulse_unitaries_jac`` (:func:`pulses.solve_with_jacobian`).

The evaluator (:func:`circuit_unitaries`).  A <= 2-qubit pulse circuit is recorded once per rotation angle with the
ordinary tape recorder; the pulse parameters pass as a ``Batched.leaf`` whose batch axis holds the candidates, so the
closed-form leaves (``RZ(2 p w)``, ``ControlledPhaseShift(-pi^2 p)``) carry their linear tangents as they always do.
Both routes share steps 1 and 2 and the classification of step 3; step 4 exists twice, on purpose:
  1. :func:`_record_tapes` records, and every ``PulseRotation`` request of all scripts, angles and candidates goes
     into one table per launch group, identical rows once (:func:`_unique_solves`);
  2. the tables are solved by the ``solver`` callable (default :func:`pulses.solve_with_jacobian`; tests inject a
     NumPy one) in :func:`_solve_groups` -- :data:`LAUNCH_GROUPS` counts these calls, normally one per evaluation
     whatever the number of candidates;
  3. :func:`_op_terms` names an op's kind and maps its derivatives onto the leaf indices its arguments came from (a
     request's five argument derivatives: ``PulseRotation.jacobian_terms``), :func:`_placement` its wires;
  4. the circuit's ``d x d`` unitary and its ``[P, d, d]`` Jacobian are composed densely in NumPy complex128 by the
     product rule (:func:`_op_matrices` and the loop of :func:`circuit_unitaries`: the independent check of the
     device route's tables and kernel).
Basis-state preparations are columns of that unitary and ``|+>`` preparations ordinary constant gates of the tape: no
script is executed ``2^n`` times.

All candidates of a stage-0 scan step and all restarts of a stage-1 step advance together through one solver call.
The optimiser is AdamW with optax's defaults, global-norm clipping per candidate row and the warmup-cosine schedule,
written out in NumPy; parameters optimised in log space use ``d/d log p = p d/dp``.

Composition on the device (``compose="device"``).  Step 4 also exists as one launch of
``qmle_compose_circuits``: :func:`_compose_tables` turns the recorded tapes of any number of jobs into a circuit, an op
and a tangent-term table, the solver's ``[n, 6, 4]`` result stays on the device, and only overlaps (the cost
functions, through :func:`_overlaps` on either route) or matrices (:func:`circuit_unitaries`) come back --
:data:`COMPOSE_LAUNCHES` counts these launches.  The
per-gate entry points default to ``"host"``; the joint path (:func:`joint_unitary_cost_fn`, ``QOC.optimize_joint``:
one shared leaf vector against the weighted unitary costs of several target gates) defaults to ``"device"`` with the
default solver and evaluates all its gates with one solver call and one composition launch.

Not included: plots, the command line, ``profile_pulse_pipeline``.  (Gradients of a CIRCUIT's expectation values by
pulse parameters are not this module's: ``Script.vjp`` / ``Model.gradient(gate_mode="pulse")`` serve them from the
backward sweep's matrix cotangents and the same solver Jacobian, :mod:`pulses`.)
"""
from __future__ import annotations

import csv
import itertools
import logging
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import operations as op
from . import pulses
from .batching import Batched
from .evolution import Evolution
from .gates import Gates, PulseEnvelope, PulseInformation
from .operations import Barrier, ControlledPhaseShift, Operation, _Rotation
from .pulses import PulseRotation, _tracked_terms
from .script import Script
from .tape import batch_context
from .utils import as_key

log = logging.getLogger(__name__)

LAUNCH_GROUPS = 0  # calls of the solver since import (one per evaluation and launch group)
COMPOSE_LAUNCHES = 0  # launches of qmle_compose_circuits since import (one per evaluation with compose="device")

_PAULI = {"X": np.array([[0, 1], [1, 0]], dtype=np.complex128), "Y": np.array([[0, -1j], [1j, 0]]),
          "Z": np.array([[1, 0], [0, -1]], dtype=np.complex128)}


# ---- the evaluator ----------------------------------------------------------------------------------------------------
# (wires of the circuit, wires of the op) -> ``qmle_compose_op.placement``: 0 the one wire of a 1-wire circuit; of two
# wires 1 / 2 wire 0 / 1 and 3 / 4 the pair in the order (0, 1) / (1, 0)
_PLACEMENTS = {(1, (0,)): 0, (2, (0,)): 1, (2, (1,)): 2, (2, (0, 1)): 3, (2, (1, 0)): 4}


def _placement(wires: Sequence[int], n: int) -> int:
    at = _PLACEMENTS.get((n, tuple(wires)))
    if at is None:
        raise NotImplementedError(f"qoc evaluates circuits on 1 or 2 wires; got wires {list(wires)} of {n}")
    return at


def _embed(m: np.ndarray, wires: Sequence[int], n: int) -> np.ndarray:
    """``[..., 2^k, 2^k]`` on ``wires`` -> ``[..., 2^n, 2^n]`` on wires 0..n-1 (wire 0 the most significant)."""
    at = _placement(wires, n)
    if at in (0, 3):
        return m
    if at == 4:
        t = m.reshape(m.shape[:-2] + (2, 2, 2, 2))
        return np.swapaxes(np.swapaxes(t, -4, -3), -2, -1).reshape(m.shape[:-2] + (4, 4))
    eye = np.eye(2, dtype=np.complex128)
    if at == 1:
        return np.einsum("...ab,cd->...acbd", m, eye).reshape(m.shape[:-2] + (4, 4))
    return np.einsum("ab,...cd->...acbd", eye, m).reshape(m.shape[:-2] + (4, 4))


def _op_terms(o: Operation):
    """``(kind, [(slot, index, coef)])`` of one recorded operation: its name among ``_native.COMPOSE_KINDS`` and the
    leaf elements its matrix depends on (slot: the solve's derivative for a pulse, 0 otherwise)."""
    if isinstance(o, PulseRotation):
        return "PULSE", o.jacobian_terms()
    terms = [(0, index, coef) for name, tans in o.__dict__.get("_tangents", {}).items()
             for _, index, coef in _tracked_terms(tans, f"{name} of {o!r}")]
    if not terms:
        return "CONST", terms
    if isinstance(o, _Rotation):
        return "ROT_" + o._axis, terms
    if isinstance(o, ControlledPhaseShift):
        return "CPHASE", terms
    raise NotImplementedError(f"qoc: no derivative rule for {o!r} with parameters that depend on the pulse parameters")


def _op_matrices(o: Operation, solved: Optional[tuple], n_params: int, C: int):
    """(M [1 or C, dk, dk], {param index: dM [C, dk, dk]}) of one recorded operation."""
    d_m: Dict[int, np.ndarray] = {}
    kind, terms = _op_terms(o)
    if kind == "PULSE":
        m, J = solved
    else:
        m = np.asarray(o.matrix, dtype=np.complex128)
        m = m[None] if m.ndim == 2 else m
        if kind == "CPHASE":
            dm = np.zeros_like(m)
            dm[..., 3, 3] = 1j * m[..., 3, 3]
        elif terms:
            dm = (-0.5j * _PAULI[o._axis]) @ m
    for slot, index, coef in terms:
        term = coef[:, None, None] * (J[:, slot] if kind == "PULSE" else dm)
        term = np.broadcast_to(term, (C,) + term.shape[-2:])
        d_m[index] = d_m[index] + term if index in d_m else np.array(term)
    return m, d_m


def _check_compose(compose: str) -> str:
    if compose not in ("host", "device"):
        raise ValueError(f"compose must be 'host' or 'device', got {compose!r}")
    return compose


class _ComposeTables:
    """The tables of ``qmle_compose_circuits`` for a list of jobs, and the solve table of every launch group."""

    def __init__(self, C: int):
        from . import _native as N

        self.N, self.C = N, C
        self.circuits, self.ops, self.terms, self.rows = [], [], [], []
        self.mats, self.coefs, self.targets = [], [], []
        self._n_mats = self._n_coefs = self._n_targets = 0
        self._mat_at: Dict[bytes, int] = {}
        self._coef_at: Dict = {}
        self.requests: List[PulseRotation] = []  # the pulse ops, in the order of their entries in ``rows``
        self.index: List[List[List[int]]] = []  # [job][script][angle] -> circuit
        self.ov_len = self.full_len = 0

    def matrix(self, m: np.ndarray) -> Tuple[int, int]:
        """(offset, per-candidate stride) of ``m`` ``[k, k]`` or ``[1 or C, k, k]`` in the matrix pool."""
        m = np.ascontiguousarray(m, dtype=np.complex128)
        if m.ndim == 3 and m.shape[0] == 1:
            m = m[0]
        if m.ndim == 3 and m.shape[0] != self.C:
            raise ValueError(f"qoc: a matrix batch of {m.shape[0]} does not fit {self.C} candidates")
        key = m.tobytes()
        if key not in self._mat_at:
            self._mat_at[key] = self._n_mats
            self.mats.append(m.reshape(-1))
            self._n_mats += m.size
        return self._mat_at[key], (m.shape[-1] * m.shape[-2] if m.ndim == 3 else 0)

    def coef(self, coef: np.ndarray) -> int:
        coef = np.ascontiguousarray(np.broadcast_to(np.asarray(coef, dtype=np.float64).reshape(-1), (self.C,)))
        key = float(coef[0]) if (coef == coef[0]).all() else coef.tobytes()
        if key not in self._coef_at:
            self._coef_at[key] = self._n_coefs
            self.coefs.append(coef)
            self._n_coefs += self.C
        return self._coef_at[key]

    def target(self, V: Optional[np.ndarray]) -> int:
        if V is None:
            return -1
        V = np.ascontiguousarray(V, dtype=np.complex128).reshape(-1)
        self.targets.append(V)
        self._n_targets += V.size
        return self._n_targets - V.size

    def add_op(self, o: Operation, n: int) -> None:
        placement, t0 = _placement(o.wires, n), len(self.terms)
        kind, terms = _op_terms(o)
        if kind == "PULSE":
            at, stride = len(self.requests) * self.C, 0  # (its C entries of ``rows``, which solve_tables fills)
            self.requests.append(o)
        else:
            at, stride = self.matrix(o.matrix)
        for slot, index, coef in terms:
            self.terms.append((slot, int(index), self.coef(coef)))
        self.ops.append((self.N.COMPOSE_KINDS[kind], placement, at, stride, t0, len(self.terms)))

    def add_circuit(self, tape: Sequence[Operation], n: int, P: int, V: Optional[np.ndarray]) -> int:
        b, d, C = len(self.ops), 2 ** n, self.C
        for o in tape:
            self.add_op(o, n)
        ov, dov = self.ov_len, self.ov_len + C
        u, du = self.full_len, self.full_len + C * d * d
        self.ov_len += C * (1 + P)
        self.full_len += C * (1 + P) * d * d
        self.circuits.append((b, len(self.ops), n, P, self.target(V), ov, dov, u, du))
        return len(self.circuits) - 1

    def solve_tables(self):
        """-> [(launch group, its table of distinct solves)]; fills ``rows`` with indices into the tables stacked in
        that order."""
        tables, rows = _unique_solves(self.requests)
        base = np.cumsum([0] + [len(table) for _, table in tables])
        self.rows = [np.broadcast_to(idx + base[g], (self.C,)).astype(np.int32) for g, idx in rows]
        return tables

    def arrays(self):
        N = self.N
        cat = lambda parts, dtype: np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)  # noqa: E731
        return (np.array(self.circuits, dtype=N.COMPOSE_CIRCUIT), np.array(self.ops, dtype=N.COMPOSE_OP),
                np.array(self.terms, dtype=N.COMPOSE_TERM), cat(self.rows, np.int32), cat(self.mats, np.complex128),
                cat(self.coefs, np.float64), cat(self.targets, np.complex128))


def _record_tapes(scripts: Sequence[Script], ws: np.ndarray, pulse_params: Optional[np.ndarray], C: int):
    tapes = []
    for script in scripts:
        per_angle = []
        for w in ws:
            with batch_context(C):
                tape = (script._record(float(w), Batched.leaf(pulse_params, 0)) if pulse_params is not None
                        else script._record(float(w)))
            per_angle.append([o for o in tape if not isinstance(o, Barrier)])
        tapes.append(per_angle)
    return tapes


def _n_wires(script: Script, per_angle) -> int:
    return script._n_qubits or 1 + max(w for tape in per_angle for o in tape for w in o.wires)


def _unique_solves(requests: Sequence[PulseRotation]):
    """Every request of an evaluation in one table per launch group, identical rows once -> ``([(launch group, its
    table of distinct solves)], per request (number of its table, indices of its rows in that table))``."""
    groups: Dict[tuple, list] = {}
    for k, o in enumerate(requests):
        groups.setdefault(o.group(), []).append((k, o.solves()))
    tables, rows = [], [None] * len(requests)
    for g, (key, members) in enumerate(groups.items()):
        table, inverse = np.unique(np.concatenate([s for _, s in members]), axis=0, return_inverse=True)
        inverse = np.asarray(inverse).reshape(-1)
        at = 0
        for k, solves in members:
            rows[k] = (g, inverse[at:at + len(solves)])
            at += len(solves)
        tables.append((key, table))
    return tables, rows


def _solve_groups(tables, solver: Optional[Callable], on_device: bool = False) -> list:
    """ONE solver call per launch group of :func:`_unique_solves`, counted in :data:`LAUNCH_GROUPS` -> per group
    ``(U [n, 2, 2], J [n, 5, 2, 2])`` on the host; ``on_device`` (the default solver only): the ``[n, 6, 4]`` device
    tensor of :func:`pulses.solve_with_jacobian` instead."""
    global LAUNCH_GROUPS
    parts = []
    for (envelope, mode, omega_c, omega_q), table in tables:
        LAUNCH_GROUPS += 1
        if on_device:
            parts.append(pulses.solve_with_jacobian(table, envelope, mode, omega_c, omega_q, on_device=True)[0])
        else:
            U, J, _ = (solver or pulses.solve_with_jacobian)(table, envelope, mode, omega_c, omega_q)
            parts.append((np.asarray(U), np.asarray(J)))
    return parts


def _compose_tables(jobs: Sequence[tuple], ws: np.ndarray) -> _ComposeTables:
    """Record the tapes of every job ``(scripts, pulse_params [C, P_g])`` or ``(scripts, pulse_params, targets)`` --
    ``targets[i]`` ``[S, d, d]`` the target unitaries of script i -- at the angles ``ws`` and emit ONE set of tables:
    a circuit per (job, script, angle), every pulse request of every job in one solve table per launch group."""
    C = int(np.asarray(jobs[0][1]).shape[0])
    tab = _ComposeTables(C)
    for job in jobs:
        scripts, pp = job[0], np.asarray(job[1], dtype=np.float64)
        targets = job[2] if len(job) > 2 else None
        if pp.ndim != 2 or pp.shape[0] != C:
            raise ValueError(f"qoc: every job needs pulse_params [{C}, P], got shape {pp.shape}")
        per_script = []
        for i, (script, per_angle) in enumerate(zip(scripts, _record_tapes(scripts, ws, pp, C))):
            n = _n_wires(script, per_angle)
            per_script.append([tab.add_circuit(tape, n, pp.shape[1], None if targets is None else targets[i][s])
                               for s, tape in enumerate(per_angle)])
        tab.index.append(per_script)
    return tab


def _solve_tables(tab: _ComposeTables, solver: Optional[Callable]) -> list:
    """ONE solver call per launch group of ``tab`` -> the groups' ``[n, 6, 4]`` results in the order that ``tab.rows``
    indexes: device tensors from the default solver, host arrays from an injected one."""
    if solver is None:
        return _solve_groups(tab.solve_tables(), None, on_device=True)
    return [np.ascontiguousarray(np.concatenate([U[:, None], J], axis=1).reshape(len(U), 6, 4), dtype=np.complex128)
            for U, J in _solve_groups(tab.solve_tables(), solver)]


def _compose_on_device(tab: _ComposeTables, solver: Optional[Callable], column_mask: int, want_ov: bool,
                       want_full: bool):
    """Solve every launch group of ``tab`` (:func:`_solve_tables`; an injected solver's host result is uploaded) and
    compose in ONE launch.  -> (ov, full) host arrays or None."""
    global COMPOSE_LAUNCHES
    N = tab.N
    torch = N.require_gpu()
    parts = [x if hasattr(x, "is_cuda") else torch.from_numpy(x).to(N.current_device())
             for x in _solve_tables(tab, solver)]
    jac = None if not parts else (parts[0] if len(parts) == 1 else torch.cat(parts))
    circuits, ops, terms, rows, mats, coefs, targets = tab.arrays()
    COMPOSE_LAUNCHES += 1
    ov, full = N.compose_circuits(circuits, ops, terms, rows, tab.C, mats if mats.size else None,
                                  coefs if coefs.size else None, targets if targets.size else None, jac, column_mask,
                                  ov_len=tab.ov_len if want_ov else 0, full_len=tab.full_len if want_full else 0)
    return (None if ov is None else N.to_host(ov)), (None if full is None else N.to_host(full))


def _overlaps(jobs: Sequence[tuple], ws: np.ndarray, solver: Optional[Callable], column_mask: int, compose: str):
    """For jobs ``(scripts, pulse_params, targets)``: per job and script ``(ov [C, S], dov [C, S, P])``, the overlaps
    ``sum_{j in mask} sum_i conj(V[i][j]) U[i][j]`` -- of :func:`_compose_on_device` for all jobs at once, or
    contracted here from the host route's unitaries, job by job."""
    out = []
    if compose == "host":
        for scripts, pp, targets in jobs:
            res = []
            for (U, dU), V in zip(circuit_unitaries(scripts, ws, pp, solver, "host"), targets):
                k = min(U.shape[-1], int(column_mask).bit_length())  # up to the last selected column: views, no copy
                Vc = np.conj(np.asarray(V)[..., :k]) * [column_mask >> j & 1 for j in range(k)]
                res.append((np.einsum("sij,csij->cs", Vc, U[..., :k]), np.einsum("sij,cspij->csp", Vc, dU[..., :k])))
            out.append(res)
        return out
    tab = _compose_tables(jobs, ws)
    ov, _ = _compose_on_device(tab, solver, column_mask, True, False)
    C = tab.C
    for job, per_script in zip(jobs, tab.index):
        P = np.asarray(job[1]).shape[1]
        res = []
        for ids in per_script:
            at = [tab.circuits[k][5] for k in ids]
            res.append((np.stack([ov[a:a + C] for a in at], axis=1),
                        np.stack([ov[a + C:a + C * (1 + P)].reshape(C, P) for a in at], axis=1)))
        out.append(res)
    return out


def circuit_unitaries(scripts: Sequence[Script], ws: np.ndarray, pulse_params: Optional[np.ndarray],
                      solver: Optional[Callable] = None, compose: str = "host"
                      ) -> List[Tuple[np.ndarray, Optional[np.ndarray]]]:
    """The unitaries of ``scripts`` at the rotation angles ``ws`` ``[S]``.  With ``pulse_params`` ``[C, P]`` a script
    is called as ``f(w, pulse_params)`` and gives ``(U [C, S, d, d], dU [C, S, P, d, d])``; with ``None`` it is
    called as ``f(w)`` and gives ``(U [S, d, d], None)``.  Every pulse solve of the call goes through ONE call of
    ``solver(table, envelope, mode, omega_c, omega_q) -> (U, J, steps)`` per launch group.  ``compose``: ``"host"``
    composes in NumPy, ``"device"`` in one launch of ``qmle_compose_circuits`` (circuits without pulse parameters
    have nothing to differentiate and are composed on the host either way)."""
    _check_compose(compose)
    ws = np.asarray(ws, dtype=np.float64).reshape(-1)
    if compose == "device" and pulse_params is not None:
        pulse_params = np.asarray(pulse_params, dtype=np.float64)
        (C, P), S = pulse_params.shape, len(ws)
        tab = _compose_tables([(scripts, pulse_params)], ws)
        _, full = _compose_on_device(tab, solver, 1, False, True)
        out = []
        for ids in tab.index[0]:
            d = 2 ** tab.circuits[ids[0]][2]
            U = np.stack([full[tab.circuits[k][7]:][:C * d * d].reshape(C, d, d) for k in ids], axis=1)
            dU = np.stack([full[tab.circuits[k][8]:][:C * P * d * d].reshape(C, P, d, d) for k in ids], axis=1)
            out.append((U, dU.reshape(C, S, P, d, d)))
        return out
    with_pp = pulse_params is not None
    if with_pp:
        pulse_params = np.asarray(pulse_params, dtype=np.float64)
        C, P = pulse_params.shape
    else:
        C, P = 1, 0
    tapes = _record_tapes(scripts, ws, pulse_params, C)
    requests = [o for per_angle in tapes for tape in per_angle for o in tape if isinstance(o, PulseRotation)]
    tables, rows = _unique_solves(requests)
    parts = _solve_groups(tables, solver)
    solved = {id(o): (parts[g][0][idx], parts[g][1][idx]) for o, (g, idx) in zip(requests, rows)}
    out = []
    for script, per_angle in zip(scripts, tapes):
        n = _n_wires(script, per_angle)
        d = 2 ** n
        U_all = np.empty((C, len(ws), d, d), dtype=np.complex128)
        dU_all = np.zeros((C, len(ws), P, d, d), dtype=np.complex128) if with_pp else None
        for s, tape in enumerate(per_angle):
            U = np.broadcast_to(np.eye(d, dtype=np.complex128), (C, d, d)).copy()
            dU = np.zeros((C, P, d, d), dtype=np.complex128)
            for o in tape:
                m, d_m = _op_matrices(o, solved.get(id(o)), P, C)
                m = _embed(m, o.wires, n)
                if P:
                    dU = m[:, None] @ dU
                    for index, dm in d_m.items():
                        dU[:, index] += _embed(dm, o.wires, n) @ U
                U = m @ U
            U_all[:, s] = U
            if with_pp:
                dU_all[:, s] = dU
        out.append((U_all, dU_all) if with_pp else (U_all[0], None))
    return out


# ---- cost functions ---------------------------------------------------------------------------------------------------
def _sample_rotation_angles(n_samples: int) -> np.ndarray:
    """Rotation angles in ``[0, 2 pi)``: a uniform sweep plus about a third of the samples packed into
    ``[pi / 2, 3 pi / 2]`` (``qoc.py:63-88``); one sample: ``w = 0``."""
    if n_samples <= 1:
        return np.linspace(0.0, 2.0 * np.pi, max(n_samples, 1), endpoint=False)
    k_focus = max(1, n_samples // 3)
    k_uniform = n_samples - k_focus
    return np.concatenate([np.linspace(0.0, 2.0 * np.pi, k_uniform, endpoint=False),
                           np.linspace(0.5 * np.pi, 1.5 * np.pi, k_focus, endpoint=False)])


def _candidates(pulse_params):
    """-> (params [C, P], whether the caller passed a single vector)."""
    p = np.asarray(pulse_params, dtype=np.float64)
    if p.ndim == 1:
        return p[None], True
    if p.ndim != 2:
        raise ValueError(f"pulse_params must be [P] or [C, P], got shape {p.shape}")
    return p, False


def _result(values, grads, single: bool, value_and_grad: bool):
    """Values ``[C]`` (a tuple of them for a two-component cost) and their gradients ``[C, P]`` in the caller's
    shape."""
    if isinstance(values, tuple):
        parts = [_result(v, g, single, value_and_grad) for v, g in zip(values, grads)]
        return (tuple(p[0] for p in parts), tuple(p[1] for p in parts)) if value_and_grad else tuple(parts)
    v = np.float64(values[0]) if single else np.asarray(values, dtype=np.float64)
    if not value_and_grad:
        return v
    return v, (np.array(grads[0]) if single else np.asarray(grads, dtype=np.float64))


def _overlap_losses(ov: np.ndarray, dov: np.ndarray, scale: float):
    """For the complex overlaps ``ov`` ``[C, S]`` with derivatives ``dov`` ``[C, S, P]``: the angle means of
    ``1 - |ov|^2 / scale`` and ``1 - cos(angle(ov))`` with their gradients ``[C, P]``."""
    mag2 = np.abs(ov) ** 2
    d_mag2 = 2.0 * np.real(np.conj(ov)[..., None] * dov)
    loss_a = np.mean(1.0 - mag2 / scale, axis=1)
    grad_a = np.mean(-d_mag2 / scale, axis=1)
    mag = np.sqrt(mag2)
    safe = np.where(mag > 0, mag, 1.0)
    cosine = np.where(mag > 0, np.real(ov) / safe, 1.0)  # (angle(0) = 0)
    d_cos = np.real(dov) / safe[..., None] - (np.real(ov) / safe ** 3)[..., None] * (0.5 * d_mag2)
    d_cos = np.where((mag > 0)[..., None], d_cos, 0.0)
    return (loss_a, np.mean(1.0 - cosine, axis=1)), (grad_a, np.mean(-d_cos, axis=1))


def fidelity_cost_fn(pulse_params, pulse_scripts, target_scripts, n_samples: int, value_and_grad: bool = False,
                     solver: Optional[Callable] = None, compose: str = "host"):
    """``(1 - fidelity, 1 - cos(phase difference))`` of the states that the pulse and the target circuits prepare from
    ``|0..0>``, averaged over the rotation angles and over the (pulse, target) script pairs (``qoc.py:171-256``)."""
    if not isinstance(pulse_scripts, (list, tuple)):
        pulse_scripts = [pulse_scripts]
    if not isinstance(target_scripts, (list, tuple)):
        target_scripts = [target_scripts]
    assert len(pulse_scripts) == len(target_scripts), (
        f"pulse_scripts and target_scripts must have the same length ({len(pulse_scripts)} vs "
        f"{len(target_scripts)}).")
    params, single = _candidates(pulse_params)
    ws = _sample_rotation_angles(n_samples)
    target = circuit_unitaries(target_scripts, ws, None, solver)
    values, grads = [], []
    # column 0, of |0..0>, gives <phi|psi>; this cost reads <psi|phi>
    (overlaps,) = _overlaps([(pulse_scripts, params, [V for V, _ in target])], ws, solver, 0b1, _check_compose(compose))
    for ov, dov in overlaps:
        v, g = _overlap_losses(np.conj(ov), np.conj(dov), 1.0)
        values.append(v)
        grads.append(g)
    mean = lambda k, parts: np.mean(np.stack([p[k] for p in parts]), axis=0)  # noqa: E731
    return _result((mean(0, values), mean(1, values)), (mean(0, grads), mean(1, grads)), single, value_and_grad)


def unitary_cost_fn(pulse_params, pulse_basis_scripts, target_basis_scripts, n_samples: int, n_qubits: int,
                    value_and_grad: bool = False, solver: Optional[Callable] = None, compose: str = "host",
                    target_unitaries: Optional[np.ndarray] = None):
    """``(1 - |Tr E|^2 / d^2, 1 - cos(angle(Tr E)))`` for ``E = U_target^+ U_pulse``, averaged over the rotation
    angles (``qoc.py:259-341``); column k of a unitary is the state that the k-th basis script gives.  Scripts that
    :func:`_with_basis_prep` built from ONE circuit (what :meth:`QOC.optimize` passes) prepare ``|k>`` and apply that
    circuit, so all columns are read off the unitary of script 0; any other list of scripts is composed script by
    script (still one solver call)."""
    d = 2 ** n_qubits
    assert len(pulse_basis_scripts) == d, (
        f"pulse_basis_scripts must have {d} entries (one per basis state); got {len(pulse_basis_scripts)}.")
    assert len(target_basis_scripts) == d, (
        f"target_basis_scripts must have {d} entries (one per basis state); got {len(target_basis_scripts)}.")
    params, single = _candidates(pulse_params)
    ws = _sample_rotation_angles(n_samples)

    def unitaries(scripts, pp):
        if _one_circuit_with_basis_preps(scripts, n_qubits):
            return circuit_unitaries(scripts[:1], ws, pp, solver, compose)[0]
        cols = circuit_unitaries(scripts, ws, pp, solver, compose)  # column 0 of script k is column k
        U = np.stack([u[..., 0] for u, _ in cols], axis=-1)
        return U, (np.stack([du[..., 0] for _, du in cols], axis=-1) if pp is not None else None)

    _check_compose(compose)
    # (the targets do not depend on the pulse parameters: a caller that evaluates often may pass them, [S, d, d])
    V = unitaries(target_basis_scripts, None)[0] if target_unitaries is None else np.asarray(target_unitaries)
    if _one_circuit_with_basis_preps(pulse_basis_scripts, n_qubits):
        tr, dtr = _overlaps([(pulse_basis_scripts[:1], params, [V])], ws, solver, (1 << d) - 1, compose)[0][0]
    else:
        U, dU = unitaries(pulse_basis_scripts, params)
        tr = np.einsum("sji,csji->cs", np.conj(V), U)
        dtr = np.einsum("sji,cspji->csp", np.conj(V), dU)
    values, grads = _overlap_losses(tr, dtr, float(d) ** 2)
    return _result(values, grads, single, value_and_grad)


class _JointAssembler:
    """``theta -> the flat pulse parameters of one gate`` (``QOC._assemble_for_gate`` as an index map): parameter k of
    the gate is ``theta[..., gather[k]]``, or the constant ``frozen[k]`` of a leaf outside the joint vector where
    ``gather[k] == -1``.  ``scatter`` is its transpose: per-gate gradients ``[C, P_g]`` added into ``[C, T]``."""

    def __init__(self, pp_obj, leaf_slices: Dict[str, slice]):
        gather, frozen = [], []

        def walk(node):
            if not node.is_leaf:
                for child in node.childs:
                    walk(child)
                return
            sl = leaf_slices.get(node.name)
            values = np.asarray(node.params, dtype=np.float64).reshape(-1)
            gather.extend([-1] * len(values) if sl is None else range(sl.start, sl.stop))
            frozen.extend(values if sl is None else [0.0] * (sl.stop - sl.start))

        walk(pp_obj)
        self.gather, self.frozen = np.array(gather, dtype=np.int64), np.array(frozen, dtype=np.float64)

    def __call__(self, theta):
        theta = np.asarray(theta, dtype=np.float64)
        live = self.gather >= 0
        return np.where(live, theta[..., np.where(live, self.gather, 0)], self.frozen)

    def scatter(self, grads: np.ndarray, n_theta: int) -> np.ndarray:
        grads = np.asarray(grads, dtype=np.float64)
        out = np.zeros(grads.shape[:-1] + (n_theta,), dtype=np.float64)
        for k, at in enumerate(self.gather):  # (in parameter order: a tied element sums its members')
            if at >= 0:
                out[..., at] += grads[..., k]
        return out


def _target_unitaries(scripts, ws: np.ndarray, n_qubits: int) -> np.ndarray:
    """``[S, d, d]``: column k from basis script k (all from script 0 when the scripts are basis preparations of one
    circuit)."""
    if _one_circuit_with_basis_preps(scripts, n_qubits):
        return circuit_unitaries(scripts[:1], ws, None)[0][0]
    return np.stack([u[..., 0] for u, _ in circuit_unitaries(scripts, ws, None)], axis=-1)


def _spec_targets(spec: dict, n_samples: int) -> np.ndarray:
    """The target unitaries ``[S, d, d]`` of a joint spec at the ``n_samples`` rotation angles: the spec's optional
    entry ``"target_unitaries": (n_samples, V)`` (what ``QOC._joint_specs`` computes once) when it is for these
    angles, else computed here.  The spec is not modified."""
    given = spec.get("target_unitaries")
    if given is not None and given[0] == n_samples:
        return given[1]
    return _target_unitaries(spec["target_basis_scripts"], _sample_rotation_angles(n_samples), spec["n_qubits"])


def joint_unitary_cost_fn(pulse_params, gate_specs: List[dict], n_samples: int, value_and_grad: bool = False,
                          solver: Optional[Callable] = None, compose: Optional[str] = None):
    """The unitary cost of several target gates that share the joint leaf vector ``theta`` (``qoc.py:344-403``): both
    components are ``sum_g w_g loss_g / sum_g w_g``.  A spec is ``{"name", "n_qubits", "weight", "assembler",
    "pulse_basis_scripts", "target_basis_scripts"}`` and optionally ``"target_unitaries": (n_samples, V [S, d, d])``,
    the targets computed ahead (they do not depend on ``theta``; both routes use them); the assembler maps ``theta``
    ``[T]`` or ``[C, T]`` to the gate's flat parameters.  Gradients need an assembler that exposes its index map (``scatter``, see
    :class:`_JointAssembler`): the gradient by ``theta`` is the scatter-add of the per-gate gradients.  ``compose``:
    ``"device"`` (the default with the default solver) evaluates ALL gates with one solver call per launch group and
    one composition launch; ``"host"`` (the default with an injected solver) one gate after the other in NumPy."""
    theta, single = _candidates(pulse_params)
    compose = _check_compose(compose if compose is not None else ("device" if solver is None else "host"))
    if value_and_grad and not all(hasattr(spec["assembler"], "scatter") for spec in gate_specs):
        raise NotImplementedError("joint_unitary_cost_fn: a gradient needs assemblers that expose their index map "
                                  "(the specs of QOC.optimize_joint do); a plain callable cannot be differentiated")
    per_gate = [np.asarray(spec["assembler"](theta), dtype=np.float64) for spec in gate_specs]
    parts = []  # per gate ((process, phase) [C], their gradients [C, P_g])
    if gate_specs and all(
            _one_circuit_with_basis_preps(spec["pulse_basis_scripts"], spec["n_qubits"]) for spec in gate_specs):
        ws = _sample_rotation_angles(n_samples)
        jobs = []
        for spec, pp in zip(gate_specs, per_gate):
            jobs.append((spec["pulse_basis_scripts"][:1], pp, [_spec_targets(spec, n_samples)]))
        for spec, res in zip(gate_specs, _overlaps(jobs, ws, solver, 0xf, compose)):
            parts.append(_overlap_losses(res[0][0], res[0][1], float(2 ** spec["n_qubits"]) ** 2))
    else:
        for spec, pp in zip(gate_specs, per_gate):
            parts.append(unitary_cost_fn(pp, spec["pulse_basis_scripts"], spec["target_basis_scripts"], n_samples,
                                         spec["n_qubits"], value_and_grad=True, solver=solver, compose=compose,
                                         target_unitaries=_spec_targets(spec, n_samples)))
    C, T = theta.shape
    values, grads = [np.zeros(C), np.zeros(C)], [np.zeros((C, T)), np.zeros((C, T))]
    total_w = 0.0
    for spec, (v, g) in zip(gate_specs, parts):
        w = float(spec["weight"])
        total_w += w
        for k in range(2):
            values[k] = values[k] + w * v[k]
            if value_and_grad:
                grads[k] = grads[k] + w * spec["assembler"].scatter(g[k], T)
    if total_w > 0:
        values, grads = [v / total_w for v in values], [g / total_w for g in grads]
    return _result(tuple(values), tuple(grads), single, value_and_grad)


def pulse_width_cost_fn(pulse_params, envelope: str, value_and_grad: bool = False):
    """The pulse width: the last envelope parameter (zero for an envelope without parameters)."""
    params, single = _candidates(pulse_params)
    n_env = PulseEnvelope.get(envelope)["n_envelope_params"]
    grads = np.zeros_like(params)
    if n_env > 0:
        values = params[:, n_env - 1].copy()
        grads[:, n_env - 1] = 1.0
    else:
        values = np.zeros(params.shape[0])
    return _result(values, grads, single, value_and_grad)


def evolution_time_cost_fn(pulse_params, t_target: float, value_and_grad: bool = False):
    """``((t - t_target) / t_target)^2`` for the evolution time ``t``, the last pulse parameter."""
    params, single = _candidates(pulse_params)
    t = params[:, -1]
    grads = np.zeros_like(params)
    grads[:, -1] = 2.0 * (t - t_target) / t_target ** 2
    return _result(((t - t_target) / t_target) ** 2, grads, single, value_and_grad)


def _envelope_partials(envelope: str, p: np.ndarray, d: np.ndarray):
    """(f, [df/dp_k], df/dd) of the envelope at the distances ``d = t - t_c`` from its centre."""
    zero = np.zeros_like(d)
    if envelope == "gaussian":
        x = d / p[1]
        f = np.exp(-0.5 * x * x)
        return p[0] * f, [f, p[0] * f * x * x / p[1]], -p[0] * f * x / p[1]
    if envelope == "square":
        on = (np.abs(d) <= p[1] / 2).astype(np.float64)
        return p[0] * on, [on, zero], zero  # (piecewise constant in the width: the derivative almost everywhere)
    if envelope == "cosine":
        x = d / p[1]
        xc = np.clip(x, -0.5, 0.5)
        dx = -np.pi * p[0] * np.sin(np.pi * xc) * (np.abs(x) <= 0.5)
        return p[0] * np.cos(np.pi * xc), [np.cos(np.pi * xc), dx * (-x / p[1])], dx / p[1]
    if envelope == "drag":
        x = d / p[2]
        f = np.exp(-0.5 * x * x)
        g, u = p[0] * f, d / p[2] ** 2
        k = 1.0 - p[1] * u
        return g * k, [f * k, -g * u, g * x * x / p[2] * k + 2.0 * g * p[1] * u / p[2]], -g * u * k - g * p[1] / p[2] ** 2
    if envelope == "sech":
        u = d / p[1]
        s, th = 1.0 / np.cosh(u), np.tanh(u)
        return p[0] * s, [s, p[0] * s * th * u / p[1]], -p[0] * s * th / p[1]
    raise ValueError(f"no derivative rule for the envelope {envelope!r}")


def spectral_density_cost_fn(pulse_params, envelope: str, n_fft: int = 1024, value_and_grad: bool = False):
    """The RMS bandwidth of the envelope's power spectrum on ``[0, t_evol]`` (``n_fft`` samples, the envelope centred
    at ``t_evol / 2``), normalised by the Nyquist frequency (``qoc.py:462-519``).  The gradient is analytic: the
    ``rfft`` of the envelope's partial derivatives, the sample times ``linspace(0, t_evol, n_fft)`` moving with
    ``t_evol``."""
    params, single = _candidates(pulse_params)
    info = PulseEnvelope.get(envelope)
    n_env, fn = info["n_envelope_params"], info["fn"]
    values, grads = np.zeros(params.shape[0]), np.zeros_like(params)
    if n_env == 0 or fn is None:
        return _result(values, grads, single, value_and_grad)
    u = np.linspace(0.0, 1.0, n_fft)
    for c, row in enumerate(params):
        t_evol = row[-1]
        signal = fn(row[:n_env], u * t_evol, t_evol / 2.0) * np.ones(n_fft)
        spectrum = np.fft.rfft(signal)
        raw = np.abs(spectrum) ** 2
        norm = np.sum(raw) + 1e-12
        psd = raw / norm
        freqs = np.linspace(0.0, 1.0, len(psd))
        mean = np.sum(freqs * psd)
        var = np.sum((freqs - mean) ** 2 * psd)
        values[c] = np.sqrt(var)
        if not value_and_grad or not values[c] > 0:
            continue
        _, d_p, d_d = _envelope_partials(envelope, row[:n_env], t_evol * (u - 0.5))
        d_signals = {k: d_p[k] for k in range(n_env)}
        d_signals[len(row) - 1] = d_d * (u - 0.5)
        for k, ds in d_signals.items():
            d_raw = 2.0 * np.real(np.conj(spectrum) * np.fft.rfft(ds))
            d_psd = d_raw / norm - raw * np.sum(d_raw) / norm ** 2
            d_mean = np.sum(freqs * d_psd)
            d_var = np.sum((freqs - mean) ** 2 * d_psd) - 2.0 * d_mean * np.sum((freqs - mean) * psd)
            grads[c, k] += d_var / (2.0 * values[c])
    return _result(values, grads, single, value_and_grad)


class Cost:
    """A cost function with its weight(s) and constant keyword arguments; ``+`` composes terms into one callable
    (``qoc.py:128-168``).  Called with ``value_and_grad=True`` the weighted sum applies to values and gradients
    alike."""

    def __init__(self, cost: Callable, weight: Union[float, Tuple], ckwargs: Optional[dict] = None):
        self.cost = cost
        self.weight = weight
        self.ckwargs = ckwargs if ckwargs is not None else {}

    def _weighted(self, cost):
        if isinstance(self.weight, tuple):
            return np.array([c * w for c, w in zip(cost, self.weight, strict=True)]).sum(axis=0)
        return cost * self.weight

    def __call__(self, *args, **kwargs):
        cost = self.cost(*args, **kwargs, **self.ckwargs)
        if kwargs.get("value_and_grad"):
            values, grads = cost
            return self._weighted(values), self._weighted(grads)
        return self._weighted(cost)

    def __add__(self, other):
        if other is None:
            return lambda *args, **kwargs: self(*args, **kwargs)
        if callable(other):
            def total(*args, **kwargs):
                a, b = self(*args, **kwargs), other(*args, **kwargs)
                if kwargs.get("value_and_grad"):
                    return a[0] + b[0], a[1] + b[1]
                return a + b

            return total
        raise TypeError(f"Cannot add Cost and {type(other)}")


class CostFnRegistry:
    """The cost functions that ``QOC`` can be asked for by name (``qoc.py:522-631``)."""

    _REGISTRY: Dict[str, dict] = {
        "fidelity": {"fn": fidelity_cost_fn, "default_weight": (0.5, 0.5),
                     "ckwargs_keys": ["pulse_scripts", "target_scripts", "n_samples", "solver", "compose"]},
        "unitary": {"fn": unitary_cost_fn, "default_weight": (0.5, 0.5),
                    "ckwargs_keys": ["pulse_basis_scripts", "target_basis_scripts", "n_samples", "n_qubits", "solver",
                                     "compose"]},
        "joint_unitary": {"fn": joint_unitary_cost_fn, "default_weight": (0.5, 0.5),
                          "ckwargs_keys": ["gate_specs", "n_samples", "solver", "compose"]},
        "pulse_width": {"fn": pulse_width_cost_fn, "default_weight": 1.0, "ckwargs_keys": ["envelope"]},
        "evolution_time": {"fn": evolution_time_cost_fn, "default_weight": 1.0, "ckwargs_keys": ["t_target"]},
        "spectral_density": {"fn": spectral_density_cost_fn, "default_weight": 1.0, "ckwargs_keys": ["envelope"]},
    }

    @classmethod
    def available(cls) -> List[str]:
        return list(cls._REGISTRY.keys())

    @classmethod
    def get(cls, name: str) -> dict:
        if name not in cls._REGISTRY:
            raise ValueError(f"Unknown cost function '{name}'. Available: {cls.available()}")
        return cls._REGISTRY[name]

    @classmethod
    def parse_cost_arg(cls, spec: Union[str, Tuple]) -> Tuple[str, Union[float, Tuple[float, ...]]]:
        """``"name"`` or ``"name:w1,w2,..."`` -> ``(name, weight)``; a tuple is returned as it is."""
        if isinstance(spec, tuple):
            return spec
        if ":" in spec:
            name, weight_str = spec.split(":", 1)
            parts = [float(x) for x in weight_str.split(",")]
            weight: Union[float, Tuple[float, ...]] = parts[0] if len(parts) == 1 else tuple(parts)
        else:
            name = spec
            weight = cls.get(name)["default_weight"]
        got = len(weight) if isinstance(weight, tuple) else 1
        default_weight = cls.get(name)["default_weight"]
        expected = len(default_weight) if isinstance(default_weight, tuple) else 1
        if got != expected:
            raise ValueError(f"Cost function '{name}' expects {expected} weight(s), got {got}.")
        return name, weight


# ---- the optimiser ----------------------------------------------------------------------------------------------------
def warmup_cosine_schedule(init_value: float, peak_value: float, warmup_steps: int, decay_steps: int,
                           end_value: float) -> Callable[[int], float]:
    """optax's ``warmup_cosine_decay_schedule``: linear from ``init_value`` to ``peak_value`` over ``warmup_steps``,
    then a cosine from the peak to ``end_value`` at step ``decay_steps``."""
    cosine_steps = max(decay_steps - warmup_steps, 1)
    alpha = end_value / peak_value if peak_value else 0.0

    def schedule(count: int) -> float:
        if count < warmup_steps:
            return init_value + (peak_value - init_value) * count / warmup_steps
        frac = min(count - warmup_steps, cosine_steps) / cosine_steps
        return peak_value * ((1.0 - alpha) * 0.5 * (1.0 + np.cos(np.pi * frac)) + alpha)

    return schedule


class _Adam:
    """AdamW over the rows of ``[C, P]`` (optax's defaults; ``weight_decay=0`` is optax's ``adam``), each row with
    its own global-norm clipping.  ``clip``: a positive finite bound, or None."""

    def __init__(self, shape, schedule, clip: Optional[float], weight_decay: float = 1e-4, b1: float = 0.9,
                 b2: float = 0.999, eps: float = 1e-8):
        self.m, self.v, self.count = np.zeros(shape), np.zeros(shape), 0
        self.schedule = schedule if callable(schedule) else (lambda count, lr=float(schedule): lr)
        self.clip, self.weight_decay, self.b1, self.b2, self.eps = clip, weight_decay, b1, b2, eps

    def step(self, params: np.ndarray, grads: np.ndarray, frozen: Optional[np.ndarray] = None) -> np.ndarray:
        """The next parameters; rows marked ``frozen`` keep parameters and moments."""
        if self.clip is not None:
            norm = np.sqrt(np.sum(grads * grads, axis=1, keepdims=True))
            grads = np.where(norm < self.clip, grads, grads / np.where(norm > 0, norm, 1.0) * self.clip)
        m = self.b1 * self.m + (1.0 - self.b1) * grads
        v = self.b2 * self.v + (1.0 - self.b2) * grads * grads
        t = self.count + 1
        update = (m / (1.0 - self.b1 ** t)) / (np.sqrt(v / (1.0 - self.b2 ** t)) + self.eps)
        update = update + self.weight_decay * params
        new = params - self.schedule(self.count) * update
        if frozen is not None:
            keep = frozen[:, None]
            new, m, v = np.where(keep, params, new), np.where(keep, self.m, m), np.where(keep, self.v, v)
        self.m, self.v, self.count = m, v, t
        return new


def _use_clip(grad_clip) -> bool:
    return bool(grad_clip) and grad_clip > 0 and np.isfinite(grad_clip)


def _safe(loss: np.ndarray) -> np.ndarray:
    return np.where(np.isfinite(loss), loss, np.inf)


def _with_basis_prep(circuit_fn: Callable, k: int, n_wires: int) -> Callable:
    bits = [(k >> (n_wires - 1 - i)) & 1 for i in range(n_wires)]

    def prepared(*args, **kwargs):
        for i, bit in enumerate(bits):
            if bit:
                op.PauliX(wires=i)
        circuit_fn(*args, **kwargs)

    prepared.__name__ = f"basis{k}_{circuit_fn.__name__}"
    prepared._basis_of = (circuit_fn, k, n_wires)  # (read by _one_circuit_with_basis_preps)
    return prepared


def _one_circuit_with_basis_preps(scripts, n_wires: int) -> bool:
    """Whether script k is ``_with_basis_prep(f, k, n_wires)`` of one and the same circuit ``f`` for every k."""
    marks = [getattr(getattr(s, "f", None), "_basis_of", None) for s in scripts]
    return all(m is not None and m[0] is marks[0][0] and m[1] == k and m[2] == n_wires for k, m in enumerate(marks))


def _chain_gate_stages(*stages: Callable) -> Callable:
    def chained(w):
        for stage in stages:
            stage(w)

    return chained


def _make_gate_pair(pulse_gate: Callable, target_gate: Callable, prep: Optional[Callable] = None,
                    post: Optional[Callable] = None) -> Tuple[Callable, Callable]:
    def pulse_circuit(w, pp):
        if prep is not None:
            prep(w)
        pulse_gate(w, pp)
        if post is not None:
            post(w)

    def target_circuit(w):
        if prep is not None:
            prep(w)
        target_gate(w)
        if post is not None:
            post(w)

    return pulse_circuit, target_circuit


class QOC:
    """Pulse-level gate synthesis in two stages (``qoc.py:634-2114``, the per-gate path): a coarse grid scan whose
    candidates are refined together by a few Adam steps, then multi-restart AdamW on the full weighted cost."""

    GATES_1Q: List[str] = ["RX", "RY", "RZ", "Rot", "H"]
    GATES_2Q: List[str] = ["CX", "CY", "CZ", "CRX", "CRY", "CRZ"]
    DEFAULT_PARAM_RANGES = {
        1: [(0.05, 3.0)],
        2: [(0.05, 3.0), (0.05, 3.0)],
        3: [(0.05, 3.0), (0.05, 3.0), (0.05, 3.0)],
        4: [(0.05, 3.0), (0.05, 3.0), (0.05, 3.0), (0.05, 3.0)],
    }
    SCAN_REL_FACTORS: Tuple[float, ...] = (0.5, 0.75, 1.0, 1.25, 1.5)

    def __init__(self, envelope: str, cost_fns: List[Tuple[str, Union[float, Tuple[float, ...]]]], t_target: float,
                 n_steps: int, n_samples: int, learning_rate: float, log_interval: int = 50, file_dir: str = None,
                 warmup_ratio: float = 0.0, end_lr_ratio: float = 1.0, n_restarts: int = 1,
                 restart_noise_scale: float = 0.5, grad_clip: float = 1.0, random_seed: int = 42, scan_steps: int = 0,
                 scan_grid_size: int = 5, scan_ranges: Optional[List[Tuple[float, float]]] = None,
                 log_scale_params: Optional[List[int]] = None, early_stop_patience: int = 0,
                 early_stop_min_delta: float = 0.0, plot: bool = False, solver: Optional[Callable] = None,
                 compose: Optional[str] = None):
        """The reference's arguments (``qoc.py:656-777``), ``solver``: the pulse solver of the evaluator (default
        :func:`pulses.solve_with_jacobian`), and ``compose``: where circuits are composed -- ``None`` keeps the
        defaults (``"host"`` per gate; joint: ``"device"`` with the default solver, else ``"host"``).  ``plot`` is
        stored and not acted on."""
        self.envelope = envelope
        self.n_steps = n_steps
        self.n_samples = n_samples
        self.learning_rate = learning_rate
        self.warmup_ratio = warmup_ratio
        self.end_lr_ratio = end_lr_ratio
        self.log_interval = log_interval
        self.file_dir = file_dir if file_dir else os.path.dirname(os.path.realpath(__file__))
        self.t_target = t_target
        self.n_restarts = max(1, n_restarts)
        self.restart_noise_scale = restart_noise_scale
        self.grad_clip = grad_clip
        self.random_seed = int(random_seed)
        self.random_key = as_key(self.random_seed)
        self.scan_steps = scan_steps
        self.scan_grid_size = scan_grid_size
        self.scan_ranges = scan_ranges
        self.solver = solver
        self.compose = None if compose is None else _check_compose(compose)
        n_env = PulseEnvelope.get(envelope)["n_envelope_params"]
        if log_scale_params is not None:
            self.log_scale_params = log_scale_params
        elif n_env >= 2:
            self.log_scale_params = [0, -1]  # amplitude and evolution time
        else:
            self.log_scale_params = []
        self.early_stop_patience = max(0, int(early_stop_patience))
        self.early_stop_min_delta = float(early_stop_min_delta)
        self.plot = plot
        log.info(f"Training parameters: {self.n_steps} steps, {self.n_samples} samples, {self.learning_rate} "
                 "learning rate")
        summed_weights = 0
        for name, _weight in cost_fns:
            CostFnRegistry.get(name)  # raises ValueError if unknown
            summed_weights += sum(_weight) if isinstance(_weight, tuple) else _weight
        assert np.isclose(summed_weights, 1.0, rtol=1e-8), f"Cost function weights must sum to 1. Got {summed_weights}"
        self.cost_fns = cost_fns
        PulseInformation.set_envelope(self.envelope)

    def save_results(self, gate: str, fidelity: float, pulse_params) -> None:
        """Write ``gate, fidelity, parameters...`` to ``qoc_results_<envelope>.csv``; an existing entry of the gate is
        overwritten (with a warning when its fidelity was higher)."""
        if self.file_dir is None:
            return
        os.makedirs(self.file_dir, exist_ok=True)
        filename = os.path.join(self.file_dir, f"qoc_results_{self.envelope}.csv")
        rows = None
        if os.path.isfile(filename):
            with open(filename, mode="r", newline="") as f:
                rows = list(csv.reader(f.readlines()))
        entry = [gate] + [fidelity] + list(map(float, pulse_params))
        with open(filename, mode="w", newline="") as f:
            writer = csv.writer(f)
            match = False
            for row in rows or []:
                if row and row[0] == gate:
                    if fidelity <= float(row[1]):
                        log.warning(f"Pulse parameters for {gate} already exist with higher fidelity ({row[1]} >= "
                                    f"{fidelity})")
                    writer.writerow(entry)
                    match = True
                else:
                    writer.writerow(row)
            if not match:
                writer.writerow(entry)

    # -- log space
    def _log_mask(self, n: int) -> np.ndarray:
        mask = np.zeros(n, dtype=bool)
        for idx in self.log_scale_params:
            i = idx if idx >= 0 else n + idx
            if 0 <= i < n:
                mask[i] = True
        return mask

    def _to_log_space(self, params: np.ndarray) -> np.ndarray:
        """``log(|p| + 1e-12)`` at the indices of ``log_scale_params`` (last axis), the rest unchanged."""
        params = np.asarray(params, dtype=np.float64)
        if not self.log_scale_params:
            return params
        return np.where(self._log_mask(params.shape[-1]), np.log(np.abs(params) + 1e-12), params)

    def _from_log_space(self, log_params: np.ndarray) -> np.ndarray:
        log_params = np.asarray(log_params, dtype=np.float64)
        if not self.log_scale_params:
            return log_params
        mask = self._log_mask(log_params.shape[-1])
        with np.errstate(over="ignore"):
            return np.where(mask, np.exp(np.where(mask, log_params, 0.0)), log_params)

    def _value_and_grad_log(self, total_cost: Callable, log_params: np.ndarray):
        """Loss ``[C]`` and its gradient by the log-space parameters ``[C, P]``: ``d/d log p = p d/dp``."""
        params = self._from_log_space(log_params)
        loss, grads = total_cost(params, value_and_grad=True)
        if self.log_scale_params:
            grads = np.where(self._log_mask(params.shape[-1]), grads * params, grads)
        return np.asarray(loss, dtype=np.float64), np.asarray(grads, dtype=np.float64)

    def _build_scan_grid(self, n_params: int, init_pulse_params: Optional[np.ndarray] = None):
        """``(grid [n_candidates, n_params], axes)``: log-spaced inside ``scan_ranges`` when given, otherwise the
        multiplicative grid ``init * factors`` around the initial parameters (``SCAN_REL_FACTORS`` for five points,
        else ``linspace(0.5, 1.5)``), otherwise log-spaced inside ``DEFAULT_PARAM_RANGES``."""
        if self.scan_ranges is not None:
            ranges = self.scan_ranges
            assert len(ranges) == n_params, (
                f"scan_ranges has {len(ranges)} entries but gate has {n_params} parameters.")
            axes = [np.logspace(np.log10(lo), np.log10(hi), self.scan_grid_size) for lo, hi in ranges]
        elif init_pulse_params is not None:
            if self.scan_grid_size == len(self.SCAN_REL_FACTORS):
                factors = np.array(self.SCAN_REL_FACTORS, dtype=np.float64)
            elif (self.scan_grid_size - 1) / 2.0 <= 0:
                factors = np.array([1.0])
            else:
                factors = np.linspace(0.5, 1.5, self.scan_grid_size)
            axes = [factors * float(p) for p in init_pulse_params]
        else:
            ranges = self.DEFAULT_PARAM_RANGES.get(n_params, [(0.1, 10.0)] * n_params)
            axes = [np.logspace(np.log10(lo), np.log10(hi), self.scan_grid_size) for lo, hi in ranges]
        return np.array(list(itertools.product(*axes)), dtype=np.float64), axes

    # -- stage 0
    def stage_0_opt(self, init_pulse_params: np.ndarray, total_cost: Callable):
        """The grid scan: every candidate is evaluated raw, refined by ``scan_steps`` Adam steps (learning rate x 2)
        and evaluated again; the better of the two counts.  All candidates advance together -- one solver call per
        scan step, plus one evaluation of the raw candidates (with the initial parameters) and a final one.  Candidates with a non-finite loss or update
        are skipped; the solver runs with ``throw=False`` meanwhile.  Returns ``(best parameters, (axes,
        [(candidate index, candidate, loss)]) or None)``."""
        init_pulse_params = np.asarray(init_pulse_params, dtype=np.float64)
        best_params = init_pulse_params
        if self.scan_steps <= 0:  # (nothing to compare the start with: stage 1 evaluates it first thing)
            return best_params, None
        grid, axes = self._build_scan_grid(len(init_pulse_params), init_pulse_params=init_pulse_params)
        log.info(f"Stage 0: grid scan with {len(grid)} candidates, {self.scan_steps} steps each")
        landscape: list = []
        prev = Evolution.set_solver_defaults(throw=False)
        try:
            with np.errstate(all="ignore"):
                # the initial parameters and every raw candidate in one evaluation
                raw_loss = _safe(np.asarray(total_cost(np.concatenate([init_pulse_params[None], grid]))))
                best_loss, raw_loss = float(raw_loss[0]), raw_loss[1:]
                if not np.isfinite(best_loss):
                    log.warning("Stage 0: initial pulse parameters produced a non-finite loss; falling back to +inf.")
                log_p = self._to_log_space(grid)
                adam = _Adam(grid.shape, self.learning_rate * 2, self.grad_clip if self.grad_clip > 0 else 1.0,
                             weight_decay=0.0)
                failed = np.zeros(len(grid), dtype=bool)
                for _ in range(self.scan_steps):
                    _, grads = self._value_and_grad_log(total_cost, log_p)
                    new = adam.step(log_p, np.where(failed[:, None], 0.0, grads), frozen=failed)
                    bad = ~np.isfinite(new).all(axis=1)
                    failed |= bad
                    log_p = np.where(failed[:, None], log_p, new)  # frozen from the first non-finite update on
                physical = self._from_log_space(log_p)
                usable = ~failed & np.isfinite(physical).all(axis=1)
                physical = np.where(usable[:, None], physical, grid)
                loss = np.where(usable, _safe(np.asarray(total_cost(physical))), raw_loss)
        finally:
            if prev:
                Evolution.set_solver_defaults(**prev)
        raw_better = np.isfinite(raw_loss) & (~np.isfinite(loss) | (raw_loss < loss))
        physical = np.where(raw_better[:, None], grid, physical)
        loss = np.where(raw_better, raw_loss, loss)
        n_skipped = 0
        for ci in range(len(grid)):
            if not np.isfinite(loss[ci]):
                n_skipped += 1
                continue
            landscape.append((ci, grid[ci], float(loss[ci])))
            if loss[ci] < best_loss:
                best_loss, best_params = float(loss[ci]), physical[ci]
        if n_skipped:
            log.warning(f"Stage 0: skipped {n_skipped}/{len(grid)} candidates due to solver failure or non-finite loss.")
        log.info(f"Stage 0 complete. Best loss: {best_loss:.6e}, params: {best_params}")
        return best_params, (axes, landscape)

    # -- stage 1
    def _perturb_starts(self, start_params: np.ndarray) -> np.ndarray:
        """``[n_restarts, n_params]``: restart 0 is the start itself, the others add Gaussian noise of scale
        ``max(|start|, 0.1) * restart_noise_scale`` (one child key of ``random_seed`` per restart); the evolution time
        and the log-scaled parameters are kept positive."""
        start_params = np.asarray(start_params, dtype=np.float64)
        n_params = start_params.shape[0]
        keys = as_key(self.random_seed).split(self.n_restarts)  # (a fresh key: the same starts on every call)
        noise = np.stack([k.generator().standard_normal(n_params) for k in keys])
        noise[0] = 0.0
        scale = np.maximum(np.abs(start_params), 0.1) * self.restart_noise_scale
        starts = start_params[None, :] + noise * scale[None, :]
        positive = self._log_mask(n_params)
        positive[-1] = True
        return np.where(positive[None, :], np.abs(starts), starts)

    def stage_1_opt(self, best_scan_params: np.ndarray, total_costs: Callable):
        """``n_restarts`` AdamW runs of ``n_steps`` steps on the full cost, all advancing together (one solver call
        per step).  With one restart ``early_stop_patience`` freezes parameters and optimiser state once the loss
        has not improved by more than ``early_stop_min_delta`` for that many steps (the steps still run).  Returns
        ``(best parameters, loss history of the winning restart with n_steps + 1 entries, best loss)``; the best
        parameters are those that produced the lowest recorded loss."""
        warmup_steps = int(self.n_steps * self.warmup_ratio)
        end_value = self.learning_rate * self.end_lr_ratio
        if warmup_steps > 0 or self.end_lr_ratio < 1.0:
            schedule = warmup_cosine_schedule(end_value if warmup_steps > 0 else self.learning_rate,
                                              self.learning_rate, warmup_steps, self.n_steps, end_value)
        else:
            schedule = self.learning_rate
        start = np.asarray(best_scan_params, dtype=np.float64)
        single = self.n_restarts <= 1
        params = start[None] if single else self._perturb_starts(start)
        log_p = self._to_log_space(params)
        adam = _Adam(log_p.shape, schedule, self.grad_clip if _use_clip(self.grad_clip) else None)
        init_losses = np.asarray(total_costs(params), dtype=np.float64).reshape(-1)
        best_loss, best_log_p = init_losses.copy(), log_p.copy()
        patience = self.early_stop_patience if single and self.early_stop_patience > 0 else self.n_steps + 1
        min_delta = self.early_stop_min_delta if single else 0.0
        since = np.zeros(len(log_p), dtype=np.int64)
        stopped = np.zeros(len(log_p), dtype=bool)
        history = [init_losses]
        for step in range(self.n_steps):
            loss, grads = self._value_and_grad_log(total_costs, log_p)
            improved = loss < best_loss - min_delta
            best_loss = np.where(improved, loss, best_loss)
            best_log_p = np.where(improved[:, None], log_p, best_log_p)  # (the parameters that produced the loss)
            since = np.where(improved, 0, since + 1)
            if (~stopped & (since >= patience)).any():
                log.info(f"Early stop at step {step + 1}/{self.n_steps}")
            stopped |= since >= patience
            log_p = adam.step(log_p, grads, frozen=stopped)
            history.append(loss)
            if step % max(1, self.log_interval) == 0:
                log.info(f"Step {step}/{self.n_steps}, loss min/mean/max: {loss.min():.3e} / {loss.mean():.3e} / "
                         f"{loss.max():.3e}")
        winner = int(np.argmin(best_loss))
        return (self._from_log_space(best_log_p[winner]), [np.float64(h[winner]) for h in history],
                np.float64(best_loss[winner]))

    # -- the driver
    def optimize(self, wires: int) -> Callable:
        """Decorator factory: ``qoc.optimize(wires=1)(qoc.create_RX)(init_pulse_params=None)`` runs stage 0 and
        stage 1 for the gate, saves the result and returns ``(best parameters, loss history)``."""

        def decorator(create_circuits):
            def wrapper(init_pulse_params: np.ndarray = None):
                pulse_circuit, target_circuit = create_circuits()

                def _with_plus_prep(circuit_fn):
                    def prepared(*args, **kwargs):
                        for q in range(wires):
                            op.H(wires=q)
                        circuit_fn(*args, **kwargs)

                    prepared.__name__ = f"plus_{circuit_fn.__name__}"
                    return prepared

                d_basis = 2 ** wires
                all_ckwargs = {
                    "pulse_scripts": [Script(pulse_circuit, n_qubits=wires),
                                      Script(_with_plus_prep(pulse_circuit), n_qubits=wires)],
                    "target_scripts": [Script(target_circuit, n_qubits=wires),
                                       Script(_with_plus_prep(target_circuit), n_qubits=wires)],
                    "pulse_basis_scripts": [Script(_with_basis_prep(pulse_circuit, k, wires), n_qubits=wires)
                                            for k in range(d_basis)],
                    "target_basis_scripts": [Script(_with_basis_prep(target_circuit, k, wires), n_qubits=wires)
                                             for k in range(d_basis)],
                    "envelope": self.envelope,
                    "n_samples": self.n_samples,
                    "n_qubits": wires,
                    "t_target": self.t_target,
                    "solver": self.solver,
                    "compose": self.compose or "host",
                }
                gate_name = create_circuits.__name__.split("_")[1]
                if init_pulse_params is None:
                    init_pulse_params = PulseInformation.gate_by_name(gate_name).params
                init_pulse_params = np.asarray(init_pulse_params, dtype=np.float64)
                total_costs = None
                for name, weight in self.cost_fns:
                    meta = CostFnRegistry.get(name)
                    ckwargs = {k: v for k, v in all_ckwargs.items() if k in meta["ckwargs_keys"]}
                    total_costs = Cost(cost=meta["fn"], weight=weight, ckwargs=ckwargs) + total_costs
                best_scan_params, _ = self.stage_0_opt(init_pulse_params, total_costs)
                best_params, history, best_loss = self.stage_1_opt(best_scan_params, total_costs)
                self.save_results(gate=gate_name, fidelity=1 - float(best_loss), pulse_params=best_params)
                return best_params, history

            return wrapper

        return decorator

    @staticmethod
    def _gate_factories() -> Dict[str, Tuple[Callable, Callable]]:
        """``{gate: (pulse circuit (w, pp), target circuit (w))}`` with the preparations of ``qoc.py:1907-1995``."""
        def pulse(name, *angles, wires):
            return lambda w, pp: getattr(Gates, name)(*[a(w) for a in angles], wires=wires, pulse_params=pp,
                                                      gate_mode="pulse")

        same = lambda w: w  # noqa: E731
        h0, h1 = (lambda w: op.H(wires=0)), (lambda w: op.H(wires=1))
        return {
            "RX": _make_gate_pair(pulse("RX", same, wires=0), lambda w: op.RX(w, wires=0)),
            "RY": _make_gate_pair(pulse("RY", same, wires=0), lambda w: op.RY(w, wires=0)),
            "RZ": _make_gate_pair(pulse("RZ", same, wires=0), lambda w: op.RZ(w, wires=0), prep=h0, post=h0),
            "H": _make_gate_pair(pulse("H", wires=0), lambda w: op.H(wires=0), prep=lambda w: op.RY(w, wires=0)),
            "Rot": _make_gate_pair(pulse("Rot", same, lambda w: w * 2, lambda w: w * 3, wires=0),
                                   lambda w: op.Rot(w, w * 2, w * 3, wires=0), prep=h0),
            "CX": _make_gate_pair(pulse("CX", wires=[0, 1]), lambda w: op.CX(wires=[0, 1]),
                                  prep=_chain_gate_stages(lambda w: op.RY(w, wires=0), h1)),
            "CY": _make_gate_pair(pulse("CY", wires=[0, 1]), lambda w: op.CY(wires=[0, 1]),
                                  prep=_chain_gate_stages(lambda w: op.RX(w, wires=0), h1)),
            "CZ": _make_gate_pair(pulse("CZ", wires=[0, 1]), lambda w: op.CZ(wires=[0, 1]),
                                  prep=_chain_gate_stages(lambda w: op.RY(w, wires=0), h1)),
            "CRX": _make_gate_pair(pulse("CRX", same, wires=[0, 1]), lambda w: op.CRX(w, wires=[0, 1]), prep=h0),
            "CRY": _make_gate_pair(pulse("CRY", same, wires=[0, 1]), lambda w: op.CRY(w, wires=[0, 1]), prep=h0),
            "CRZ": _make_gate_pair(pulse("CRZ", same, wires=[0, 1]), lambda w: op.CRZ(w, wires=[0, 1]),
                                   prep=_chain_gate_stages(h0, h1)),
        }

    def _create_pair(self, gate_name: str) -> Tuple[Callable, Callable]:
        try:
            return self._gate_factories()[gate_name]
        except KeyError as exc:
            raise ValueError(f"No factory for gate {gate_name!r}.") from exc


    def create_CPhase(self) -> Tuple[Callable, Callable]:
        """``(pulse circuit, target circuit)`` of CPhase, both wires prepared in ``|+>`` (``qoc.py:2101-2114``)."""
        def pulse_circuit(w, pulse_params):
            op.H(wires=0)
            op.H(wires=1)
            Gates.CPhase(w, wires=[0, 1], pulse_params=pulse_params, gate_mode="pulse")

        def target_circuit(w):
            op.H(wires=0)
            op.H(wires=1)
            op.ControlledPhaseShift(w, wires=[0, 1])

        return pulse_circuit, target_circuit

    def optimize_all(self, sel_gates: str, make_log: bool) -> Dict[str, list]:
        """The per-gate loop (``qoc.py:2116-2145``): optimise every gate of ``GATES_1Q + GATES_2Q`` that ``sel_gates``
        (comma-separated names, a list of names, or ``"all"``) names -- whole names: the reference tests
        ``gate in sel_gates`` on the string itself, so that its ``"CRX"`` selects RX as well; with ``make_log`` the loss histories go to ``qoc_logs.csv``
        under ``file_dir``, one column per gate.  Returns the histories."""
        log_history: Dict[str, list] = {}
        selected = [g.strip() for g in sel_gates.split(",")] if isinstance(sel_gates, str) else list(sel_gates)
        for gate in self.GATES_1Q + self.GATES_2Q:
            if gate in selected or "all" in selected:
                n_wires = 1 if gate in self.GATES_1Q else 2
                log.info(f"Optimizing {gate} gate...")
                best_params, history = self.optimize(wires=n_wires)(getattr(self, f"create_{gate}"))()
                log.info(f"Optimized parameters for {gate}: {best_params}")
                log.info(f"Best achieved fidelity: {(1 - min(float(h) for h in history)) * 100:.5f}%")
                log_history[gate] = log_history.get(gate, []) + [float(h) for h in history]
        if make_log:
            os.makedirs(self.file_dir, exist_ok=True)
            with open(os.path.join(self.file_dir, "qoc_logs.csv"), "w", newline="") as f:
                writer = csv.writer(f)
                writer.writerow(log_history.keys())
                writer.writerows(zip(*log_history.values()))
        return log_history

    # -- joint optimisation: one shared leaf vector against a weighted sum of target gates (``qoc.py:2147-2605``)
    JOINT_LEAVES_DEFAULT: Tuple[str, ...] = ("RX", "RY", "RZ", "CZ")  # (the order lays out theta)
    JOINT_TARGETS_DEFAULT: Tuple[str, ...] = ("RX", "RY", "RZ", "H", "CX", "CRX", "CRY", "CRZ")
    JOINT_WEIGHTS_DEFAULT: Dict[str, float] = {"RX": 0.3, "RY": 0.3, "RZ": 0.3, "H": 1.0, "CX": 2.0, "CRX": 3.0,
                                               "CRY": 3.0, "CRZ": 3.0}
    JOINT_TIED_GROUPS_DEFAULT: Tuple[Tuple[str, ...], ...] = (("RX", "RY"),)  # same envelope, carrier phase apart

    def _build_joint_layout(self, leaf_names: Sequence[str],
                            tied_groups: Optional[Sequence[Sequence[str]]] = None):
        """``(init_theta, leaf_slices, log_scale_indices)``: the leaves' current parameters concatenated in the given
        order.  The present members of a tied group (two or more) share ONE slice, initialised with their mean; only
        the RX / RY amplitude and evolution time are optimised in log space."""
        tied_groups = self.JOINT_TIED_GROUPS_DEFAULT if tied_groups is None else tied_groups
        rep_of = {name: name for name in leaf_names}
        for group in tied_groups:
            present = [name for name in group if name in rep_of]
            for member in present[1:] if len(present) >= 2 else []:
                rep_of[member] = present[0]
                log.info(f"  Joint layout: tying leaf {member!r} to {present[0]!r} (shared slice in theta).")
        n_env = PulseEnvelope.get(self.envelope)["n_envelope_params"]
        leaf_slices: Dict[str, slice] = {}
        chunks, log_idx, offset = [], [], 0
        for name in leaf_names:
            if rep_of[name] != name:
                leaf_slices[name] = leaf_slices[rep_of[name]]
                continue
            pp = PulseInformation.gate_by_name(name)
            assert pp is not None and pp.is_leaf, f"_build_joint_layout: {name!r} is not a leaf gate"
            members = [m for m in leaf_names if rep_of[m] == name]
            chunk = np.mean(np.stack([np.asarray(PulseInformation.gate_by_name(m).params, dtype=np.float64)
                                      for m in members]), axis=0) if len(members) > 1 else \
                np.asarray(pp.params, dtype=np.float64)
            leaf_slices[name] = slice(offset, offset + len(chunk))
            chunks.append(chunk)
            if name in ("RX", "RY") and n_env >= 2:
                log_idx += [offset, offset + len(chunk) - 1]
            offset += len(chunk)
        return np.concatenate(chunks), leaf_slices, log_idx

    @staticmethod
    def _assemble_for_gate(theta, pp_obj, leaf_slices: Dict[str, slice]) -> np.ndarray:
        """The gate's flat parameters from ``theta`` ``[T]`` or ``[C, T]``: the slice of every leaf occurrence in
        tree order; a leaf without a slice is frozen at its ``PulseInformation`` value."""
        return _JointAssembler(pp_obj, leaf_slices)(theta)

    @staticmethod
    def _joint_gate_factories() -> Dict[str, Tuple[Callable, Callable]]:
        """``{gate: (pulse circuit, target circuit)}`` without preparations: the unitary cost sees every column, and
        a preparation can hide an error (``qoc.py:1998-2057``).  No ``Rot`` and no ``CY``."""
        def pulse(name, with_angle, wires):
            if with_angle:
                return lambda w, pp: getattr(Gates, name)(w, wires=wires, pulse_params=pp, gate_mode="pulse")
            return lambda w, pp: getattr(Gates, name)(wires=wires, pulse_params=pp, gate_mode="pulse")

        pair = lambda name, with_angle, wires, target: _make_gate_pair(pulse(name, with_angle, wires), target)  # noqa: E731
        return {
            "RX": pair("RX", True, 0, lambda w: op.RX(w, wires=0)),
            "RY": pair("RY", True, 0, lambda w: op.RY(w, wires=0)),
            "RZ": pair("RZ", True, 0, lambda w: op.RZ(w, wires=0)),
            "H": pair("H", False, 0, lambda w: op.H(wires=0)),
            "CZ": pair("CZ", False, [0, 1], lambda w: op.CZ(wires=[0, 1])),
            "CX": pair("CX", False, [0, 1], lambda w: op.CX(wires=[0, 1])),
            "CRX": pair("CRX", True, [0, 1], lambda w: op.CRX(w, wires=[0, 1])),
            "CRY": pair("CRY", True, [0, 1], lambda w: op.CRY(w, wires=[0, 1])),
            "CRZ": pair("CRZ", True, [0, 1], lambda w: op.CRZ(w, wires=[0, 1])),
        }

    def _create_joint_pair_for(self, gate_name: str) -> Tuple[Callable, Callable]:
        table = self._joint_gate_factories()
        if gate_name in table:
            return table[gate_name]
        log.warning(f"_create_joint_pair_for: no prep-free factory for {gate_name!r}; falling back to "
                    f"create_{gate_name} (preps may hide errors).")
        return self._create_pair(gate_name)

    def _joint_stage_0_coord_descent(self, init_theta: np.ndarray, leaf_slices: Dict[str, slice],
                                     total_cost: Callable) -> np.ndarray:
        """Coordinate descent over the leaves: per unique slice the multiplicative grid of :meth:`_build_scan_grid`
        around the current values, everything else held.  Within one leaf every trial overwrites the same slice, so
        the reference's candidate-by-candidate greedy loop equals: evaluate the whole grid as ONE ``[C, T]`` batch,
        take its first minimum, accept it if it is below the best so far.  One evaluation per unique slice plus one
        for the start; non-finite losses count as +inf; the solver runs with ``throw=False`` meanwhile."""
        current = np.array(init_theta, dtype=np.float64)
        if self.scan_steps <= 0:
            log.info("Joint Stage 0: scan disabled (scan_steps=0); skipping.")
            return current
        prev = Evolution.set_solver_defaults(throw=False)
        try:
            with np.errstate(all="ignore"):
                best_loss = float(_safe(np.asarray(total_cost(current[None]), dtype=np.float64).reshape(-1))[0])
                log.info(f"Joint Stage 0: coordinate-descent over {len(leaf_slices)} leaves, init_loss={best_loss:.6e}")
                seen = set()
                for leaf_name, sl in leaf_slices.items():
                    if (sl.start, sl.stop) in seen or sl.stop == sl.start:
                        continue
                    seen.add((sl.start, sl.stop))
                    grid, _ = self._build_scan_grid(sl.stop - sl.start, init_pulse_params=current[sl])
                    batch = np.repeat(current[None], len(grid), axis=0)
                    batch[:, sl] = grid
                    losses = _safe(np.asarray(total_cost(batch), dtype=np.float64).reshape(-1))
                    first = int(np.argmin(losses))
                    if losses[first] < best_loss:
                        best_loss, current = float(losses[first]), batch[first].copy()
                    log.info(f"  Joint scan after leaf {leaf_name} ({len(grid)} candidates): best_loss={best_loss:.6e}")
        finally:
            if prev:
                Evolution.set_solver_defaults(**prev)
        return current

    def _joint_specs(self, target_gates: Sequence[str], leaf_slices: Dict[str, slice],
                     weights: Dict[str, float]) -> List[dict]:
        """The specs of :func:`joint_unitary_cost_fn` for ``target_gates``: prep-free basis scripts, the gate's weight
        (1 where ``weights`` has none), its assembler over ``leaf_slices`` and its target unitaries at this object's
        ``n_samples`` angles."""
        gate_specs: List[dict] = []
        for name in target_gates:
            pp_obj = PulseInformation.gate_by_name(name)
            if pp_obj is None:
                log.warning(f"  Skipping unknown gate {name!r}.")
                continue
            n_wires = 1 if name in self.GATES_1Q else 2
            pulse_circuit, target_circuit = self._create_joint_pair_for(name)
            gate_specs.append({
                "name": name, "n_qubits": n_wires, "weight": float(weights.get(name, 1.0)),
                "assembler": _JointAssembler(pp_obj, leaf_slices),
                "pulse_basis_scripts": [Script(_with_basis_prep(pulse_circuit, k, n_wires), n_qubits=n_wires)
                                        for k in range(2 ** n_wires)],
                "target_basis_scripts": [Script(_with_basis_prep(target_circuit, k, n_wires), n_qubits=n_wires)
                                         for k in range(2 ** n_wires)],
            })
            spec = gate_specs[-1]  # the targets once, for every evaluation of either route
            spec["target_unitaries"] = (self.n_samples, _target_unitaries(
                spec["target_basis_scripts"], _sample_rotation_angles(self.n_samples), n_wires))
        return gate_specs

    def optimize_joint(self, target_gates: Optional[Sequence[str]] = None, leaf_names: Optional[Sequence[str]] = None,
                       weights: Optional[Dict[str, float]] = None):
        """Tune ONE shared vector ``theta`` -- the parameters of ``leaf_names`` (default ``JOINT_LEAVES_DEFAULT``) --
        against the weighted unitary costs of ``target_gates`` (default ``JOINT_TARGETS_DEFAULT``; ``weights`` are
        merged over ``JOINT_WEIGHTS_DEFAULT``): coordinate-descent scan, then :meth:`stage_1_opt` unchanged with
        ``log_scale_params`` pointing at the joint indices meanwhile.  Writes one CSV row per leaf (with the joint
        fidelity), updates ``PulseInformation`` in place and returns ``(best_theta, leaf_slices, loss history)``."""
        target_gates = list(target_gates) if target_gates else list(self.JOINT_TARGETS_DEFAULT)
        leaf_names = list(leaf_names) if leaf_names else list(self.JOINT_LEAVES_DEFAULT)
        merged = dict(self.JOINT_WEIGHTS_DEFAULT)
        merged.update({k: float(v) for k, v in (weights or {}).items()})
        log.info(f"Joint optimisation: leaves={leaf_names}, targets={target_gates}")
        init_theta, leaf_slices, joint_log_idx = self._build_joint_layout(tuple(leaf_names))
        gate_specs = self._joint_specs(target_gates, leaf_slices, merged)
        weight = next((w for n, w in self.cost_fns if n == "unitary"), (0.5, 0.5))
        joint_cost = Cost(cost=joint_unitary_cost_fn, weight=weight,
                          ckwargs={"gate_specs": gate_specs, "n_samples": self.n_samples, "solver": self.solver,
                                   "compose": self.compose})
        prev_log_scale = self.log_scale_params
        self.log_scale_params = joint_log_idx
        try:
            best_scan_theta = self._joint_stage_0_coord_descent(init_theta, leaf_slices, joint_cost)
            best_theta, history, best_loss = self.stage_1_opt(best_scan_theta, joint_cost)
        finally:
            self.log_scale_params = prev_log_scale
        log.info(f"Joint optimisation done. final loss={float(best_loss):.6e}")
        for leaf_name, sl in leaf_slices.items():
            self.save_results(gate=leaf_name, fidelity=float(1.0 - best_loss), pulse_params=best_theta[sl])
        for leaf_name, sl in leaf_slices.items():
            PulseInformation.gate_by_name(leaf_name).params = np.array(best_theta[sl])
        return best_theta, leaf_slices, history


def _factory(gate_name: str):
    def create(self):
        return self._create_pair(gate_name)

    create.__name__ = "create_" + gate_name
    create.__doc__ = f"``(pulse circuit, target circuit)`` of {gate_name}."
    return create


for _gate in ("RX", "RY", "RZ", "H", "Rot", "CX", "CY", "CZ", "CRX", "CRY", "CRZ"):
    setattr(QOC, "create_" + _gate, _factory(_gate))


default_qoc_params = {
    "envelope": "drag",
    "cost_fns": [("unitary", (0.5, 0.5))],
    "t_target": 0.5,
    "n_steps": 800,
    "n_samples": 20,
    "learning_rate": 0.0001,
    "warmup_ratio": 0.05,
    "end_lr_ratio": 0.01,
    "log_interval": 50,
    "file_dir": None,
    "n_restarts": 5,
    "restart_noise_scale": 0.01,
    "grad_clip": 1.0,
    "random_seed": 1000,
    "scan_steps": 20,
    "scan_grid_size": 4,
    "scan_ranges": None,
    "log_scale_params": None,
    "early_stop_patience": 0,
    "early_stop_min_delta": 0.0,
}
