"""Hamiltonian time evolution: a (static or time-dependent) Hamiltonian becomes a gate factory by solving
``dU/dt = -i H(t) U`` -- API mirror of ``qml_essentials/evolution.py``.

The reference integrates one small matrix ODE per gate and per sample with diffrax / ``jax.lax.scan``.  Here every
solve of a call -- one row per sample -- runs in ONE launch of ``qmle_evolve_magnus`` (``csrc/qmle_evolve.hip``): the
fixed-grid commutator-free Magnus schemes of the reference (``evolution.py:204-231``), float64 throughout.  The kernel
evaluates no coefficient function; the host evaluates each ``f_i(params_i, t)`` once on the array of all node times
and sends the table.

Solvers.  ``"magnus2"`` / ``"magnus4"`` are the reference's fixed grids of ``magnus_steps`` steps.  ``"dopri8"`` /
``"dopri5"`` are accepted names with the reference's contract (``atol``, ``rtol``, ``max_steps``, ``throw``) but a
DIFFERENT integrator: step doubling on the order-4 grid.  N starts at 32 and doubles; U_N is accepted when
``max |U_N - U_{N/2}| / 15 <= atol + rtol`` for every row (Richardson's estimate of an order-4 method's error); N never
exceeds ``max_steps``.  If no grid is accepted -- always the case for ``max_steps < 32`` -- the solve fails:
``RuntimeError`` naming ``max_steps`` with ``throw=True``, NaN-filled rows with ``throw=False``.

Gradients.  By default tangents are dropped through ``evolve``: an evolved gate whose arguments depend on a
differentiated leaf carries "derivative unknown", and ``Script.gradient`` (parameter shift) refuses it as it refuses
every untracked transformation.  ``Script.vjp(..., through_evolve=True)`` records its tape inside
:func:`gradient_trace`; an evolved gate whose arguments depend on a leaf is then solved by ``qmle_evolve_magnus_jac``
-- the same grid with the EXACT derivative of its result, one launch per gate call -- and recorded as an
:class:`EvolvedGate` that carries the Jacobian ``dU / d(leaf element)`` for the sweep's matrix cotangent.  The
directions are the distinct leaf elements the coefficient table or the step depends on (at most 64 per gate): the
evolution time and the interval ends keep their tangents, the node times ``t0 + (n + c) h`` are built as tracked
values -- so a coefficient function's own time dependence carries the moving-node term -- and every ``f_i(params_i,
t)`` is evaluated under ``batching.elementwise_tangents()``, ONE call with the array of node times (no per-node
fallback).  A coefficient the recorder cannot track raises ``NotImplementedError`` before any device work.  Adaptive
solver names run the doubling as always, then one Jacobian launch on the accepted grid.

Wires.  Hamiltonians on one and two wires are solved by ``qmle_evolve_magnus``, on three and four wires (8x8, 16x16) by
``qmle_evolve_magnus_wide``; five wires and more are refused.  The evolved gate of a three- or four-wire Hamiltonian
is an explicit matrix on that many wires: ``simulation.simulate_and_measure`` runs it through ``qmle_apply_matrix``
between the plans of the gates around it.  The Jacobian solve serves 1 or 2 wires and says so, and every consumer
that lowers a whole tape (the parameter shift, compiled calls, noisy tapes, the adjoint sweep by default) refuses the
gate as it refuses any explicit matrix on more than two wires.  ``Script.vjp(..., wide_gates=True,
through_evolve=True)`` records inside ``gradient_trace(wide=True)``: a STATIC evolved gate on three or four wires
whose time depends on a leaf is then one step ``U = exp(-i t H)`` with ``dU/dt = -i H U`` (:func:`static_jacobian`),
formed on the host from ``H`` and the solver's ``U`` -- the exact derivative of the exponential, which differs from
the derivative of the solver's truncated series by that series' own 1e-13.  A ``ParametrizedHamiltonian`` on three or
four wires that depends on a leaf stays refused: ``qmle_evolve_magnus_wide`` has no Jacobian form.

Pulse-level gates (:mod:`pulses`) do not come through ``evolve``: their RX / RY leaves are solved by a kernel of their
own that evaluates the envelopes on the device, all leaves of a tape in one launch.  They share the solver defaults
below and the step-doubling rule (``_doubling``).
"""
from __future__ import annotations

import contextlib
from typing import Any, Callable, Optional, Union

import numpy as np

from . import _native as N
from .batching import Batched, elementwise_tangents
from .operations import Hermitian, Operation, ParametrizedHamiltonian

_SQRT3 = np.sqrt(3.0)
_C1, _C2 = 0.5 - _SQRT3 / 6.0, 0.5 + _SQRT3 / 6.0
_FIRST_GRID = 32  # step doubling starts here


_gradient_trace = 0  # > 0 while a tape is recorded for Script.vjp(through_evolve=True)
_wide_trace = 0      # > 0 while that caller also sweeps tapes with three- and four-wire gates (wide_gates=True)

_TRACKED = ("sums, products, quotients, powers with a constant exponent and sin, cos, tan, exp, expm1, log, log1p, "
            "sqrt, square, reciprocal, sinh, cosh, tanh, arctan of one tracked value")


@contextlib.contextmanager
def gradient_trace(wide: bool = False):
    """While active, ``evolve`` keeps the tangents of its arguments and records gates that carry the Jacobian of
    their solve (module docstring).  Only a caller that asks the adjoint sweep for matrix cotangents enters it.
    ``wide``: the caller's sweep serves explicit matrices on three and four wires, so a static evolved gate on that
    many wires is recorded with its Jacobian too."""
    global _gradient_trace, _wide_trace
    _gradient_trace += 1
    _wide_trace += int(bool(wide))
    try:
        yield
    finally:
        _gradient_trace -= 1
        _wide_trace -= int(bool(wide))


def static_jacobian(H: np.ndarray, U: np.ndarray) -> np.ndarray:
    """``dU/dt = -i H U`` of the one-step evolution ``U = exp(-i t H)``: ``H`` ``[d, d]``, ``U`` ``[rows, d, d]``
    -> ``[rows, d, d]`` complex128.  Host only."""
    return -1j * np.einsum("ab,rbc->rac", np.asarray(H, dtype=np.complex128), np.asarray(U, dtype=np.complex128))


WIDE_JACOBIAN_LIMIT = ("evolve(): a ParametrizedHamiltonian on three or four wires that depends on a differentiated "
                       "argument is not differentiated: the Jacobian solve (qmle_evolve_magnus_jac) serves 1 or 2 "
                       "wires, and wide_gates=True adds static Hamiltonians (Hermitian.evolve()) on 3 or 4 wires only")


class EvolvedGate(Operation):
    """An evolved unitary whose arguments depend on differentiated leaves: one matrix per sample, ``jacobian``
    ``[rows, D, d, d]`` = its exact grid derivative by the leaf elements ``directions`` ``[(leaf, flat index)]``."""

    wants_matrix_cotangent = True

    def __init__(self, U: np.ndarray, wires, name, jacobian: np.ndarray, directions: list, steps: int,
                 record: bool = True) -> None:
        super().__init__(wires=wires, matrix=U, name=name or "Operation", record=record)
        self._matrix_tangent = None  # (every consumer that differentiates angles only refuses it, as before)
        self.jacobian, self.directions, self.evolve_steps = jacobian, list(directions), steps

    def leaf_jacobian_terms(self) -> list:
        """``[(leaf, direction, flat index, 1.0)]``: slot ``direction`` of ``jacobian`` is the derivative by that
        element of that leaf."""
        return [(leaf, k, flat, 1.0) for k, (leaf, flat) in enumerate(self.directions)]

    def dagger(self) -> "EvolvedGate":
        new = EvolvedGate(np.conj(np.swapaxes(self.matrix, -1, -2)), self.wires, self.name,
                          np.conj(np.swapaxes(self.jacobian, -1, -2)), self.directions, self.evolve_steps, record=False)
        self._replace_on_tape(new)
        return new

    def power(self, power: int):
        raise NotImplementedError("a power of an evolved gate inside a gradient trace: its Jacobian is not carried")

    def __mul__(self, other):
        raise NotImplementedError("a multiple of an evolved gate inside a gradient trace: its Jacobian is not carried")

    __rmul__ = __mul__


def _tracked_nodes(t0, h, n_steps: int, order: int):
    """The node times of ``_node_times`` from a start and a step that may be tracked 0-d ``Batched`` values ->
    a ``Batched`` of visible shape ``[nodes]`` (a plain array when neither is batched)."""
    n = np.arange(n_steps, dtype=np.float64)
    if order == 2:
        offs = n + 0.5
    else:
        offs = np.empty(2 * n_steps, dtype=np.float64)
        offs[0::2], offs[1::2] = n + _C1, n + _C2
    return t0 + offs * h


def _tracked_table(res, rows: int, nodes: int, what: str):
    """A coefficient function's result or a time -> ``(values [rows, nodes], tangent terms)``; the index arrays
    of the terms are broadcast to ``[nodes]`` and their coefficients to ``[rows, nodes]``."""
    if not isinstance(res, Batched):
        return np.broadcast_to(np.asarray(res, dtype=np.float64), (rows, nodes)).copy(), []
    if res.tan is None:
        raise NotImplementedError(f"evolve(): {what} depends on a differentiated argument through an operation the "
                                  f"recorder does not track; tracked are {_TRACKED}")
    if res.ndim > 1 or res.batch not in (1, rows):
        raise ValueError(f"evolve(): {what} has shape {res.shape}; expected a scalar or one value per node")
    terms = [(lid, np.broadcast_to(np.asarray(idx).reshape(-1), (nodes,)),
              np.broadcast_to(np.asarray(coef, dtype=np.float64).reshape(res.batch, -1), (rows, nodes)))
             for lid, idx, coef in res.tan]
    return np.broadcast_to(np.asarray(res.data, dtype=np.float64).reshape(res.batch, -1), (rows, nodes)).copy(), terms


def _rows_of(values) -> int:
    """Batch size of a list of (possibly nested) arguments: that of its Batched members, else 1."""
    b = 1
    for v in values:
        if isinstance(v, (list, tuple)):
            k = _rows_of(v)
        elif isinstance(v, Batched):
            k = v.batch
        else:
            continue
        if b not in (1, k) and k != 1:
            raise ValueError(f"inconsistent batch sizes in evolve(): {b} vs {k}")
        b = max(b, k)
    return b


def _has_batched(values) -> bool:
    return any(_has_batched(v) if isinstance(v, (list, tuple)) else isinstance(v, Batched) for v in values)


def _tangent_state(values):
    """[] when no argument depends on a differentiated leaf (the unitary is a constant for every gradient), None
    otherwise: the solver does not carry derivatives."""
    for v in values:
        if isinstance(v, (list, tuple)):
            if _tangent_state(v) is None:
                return None
        elif isinstance(v, Batched) and v.tan != []:
            return None
    return []


def _per_row(x, rows: int) -> np.ndarray:
    """A scalar time (float or 0-d Batched) as a float64 column [rows]."""
    if isinstance(x, Batched):
        x = x.data.reshape(x.batch, -1)
        if x.shape[1] != 1:
            raise ValueError("evolution times must be scalars")
        x = x[:, 0]
    return np.broadcast_to(np.asarray(x, dtype=np.float64).reshape(-1), (rows,)).copy()


def _node_times(t0: np.ndarray, h: np.ndarray, n_steps: int, order: int) -> np.ndarray:
    """[rows, nodes]: t_n + h/2 (order 2) or t_n + c1 h, t_n + c2 h (order 4), in node order."""
    n = np.arange(n_steps, dtype=np.float64)[None, :]
    if order == 2:
        return t0[:, None] + (n + 0.5) * h[:, None]
    t = np.empty((t0.shape[0], 2 * n_steps), dtype=np.float64)
    t[:, 0::2] = t0[:, None] + (n + _C1) * h[:, None]
    t[:, 1::2] = t0[:, None] + (n + _C2) * h[:, None]
    return t


def _coefficients(fn: Callable, params, t: np.ndarray, per_row_times: bool) -> np.ndarray:
    """f(params, t) at every node, [rows, nodes].  ONE call with the array of all node times (a Batched value
    when the rows have different grids); a scalar result broadcasts.  A function that cannot take an array -- it
    raises, or returns a shape that does not broadcast -- is called once per node instead."""
    rows, nodes = t.shape

    def value(res):
        if isinstance(res, Batched):
            res = res.data
            if res.ndim == 1:  # one number per sample: constant in time
                res = res[:, None]
        return np.broadcast_to(np.asarray(res, dtype=np.float64), (rows, nodes))

    try:
        return value(fn(params, Batched(t, []) if per_row_times else t[0])).copy()
    except Exception:  # noqa: BLE001  (any failure of the one-call form: fall back, errors of the function resurface)
        out = np.empty((rows, nodes), dtype=np.float64)
        for j in range(nodes):
            res = fn(params, Batched(t[:, j], []) if per_row_times else float(t[0, j]))
            res = res.data if isinstance(res, Batched) else res
            out[:, j] = np.broadcast_to(np.asarray(res, dtype=np.float64).reshape(-1), (rows,))
        return out


class Evolution:
    """Solver defaults and the ``evolve`` engine behind ``Hermitian.evolve`` / ``ParametrizedHamiltonian.evolve``."""

    _solver_defaults: dict = {"max_steps": 2 ** 13, "throw": True, "solver": "dopri8", "magnus_steps": 256}
    _valid_solvers = ("dopri8", "dopri5", "magnus2", "magnus4")

    @classmethod
    def set_solver_defaults(cls, max_steps: Optional[int] = None, throw: Optional[bool] = None,
                            solver: Optional[str] = None, magnus_steps: Optional[int] = None) -> dict:
        """Update the class-level defaults; returns the previous values of the updated keys, suitable for
        ``set_solver_defaults(**prev)``."""
        if solver is not None and solver not in cls._valid_solvers:
            raise ValueError(f"Unknown solver {solver!r}; expected one of {cls._valid_solvers}")
        prev: dict = {}
        for key, val, cast in (("max_steps", max_steps, int), ("throw", throw, bool), ("solver", solver, str),
                               ("magnus_steps", magnus_steps, int)):
            if val is not None:
                prev[key] = cls._solver_defaults[key]
                cls._solver_defaults[key] = cast(val)
        return prev

    @classmethod
    def _options(cls, kw: dict) -> tuple:
        from .utils import x64_enabled

        kw = dict(kw)
        tol = 1.0e-10 if x64_enabled() else 1.4e-8
        atol, rtol = float(kw.pop("atol", tol)), float(kw.pop("rtol", tol))
        max_steps = int(kw.pop("max_steps", cls._solver_defaults["max_steps"]))
        throw = bool(kw.pop("throw", cls._solver_defaults["throw"]))
        solver = str(kw.pop("solver", cls._solver_defaults["solver"]))
        if solver not in cls._valid_solvers:
            raise ValueError(f"Unknown solver {solver!r}; expected one of {cls._valid_solvers}")
        magnus_steps = int(kw.pop("magnus_steps", cls._solver_defaults["magnus_steps"]))
        if magnus_steps < 1:
            raise ValueError(f"magnus_steps must be at least 1, got {magnus_steps}")
        return atol, rtol, max_steps, throw, solver, magnus_steps

    @classmethod
    def evolve(cls, hamiltonian: Union[Hermitian, ParametrizedHamiltonian], name: Optional[str] = None,
               **kw: Any) -> Callable:
        """Gate factory for Hamiltonian time evolution.

        * ``Hermitian`` -> ``gate(t, wires=0)`` with ``U = exp(-i t H)`` (one constant term, one step of the order-2
          grid -- exact for a constant Hamiltonian);
        * ``ParametrizedHamiltonian`` -> ``gate(coeff_args, T)``: ``T`` a scalar (integrate on ``[0, T]``) or
          ``[t0, t1]``; ``coeff_args`` one parameter set per term.  Options: ``atol``, ``rtol`` (default 1.4e-8,
          1e-10 in x64 mode), ``max_steps``, ``throw``, ``solver``, ``magnus_steps`` (see the module docstring).

        ``t``, ``T`` and every parameter set may be ``batching.Batched``: the solve then has one row per sample and
        the gate carries one matrix per sample.  Tangents are dropped (module docstring)."""
        if isinstance(hamiltonian, Hermitian):
            return cls._evolve_static(hamiltonian, name)
        if isinstance(hamiltonian, ParametrizedHamiltonian):
            return cls._evolve_parametrized(hamiltonian, name, **kw)
        raise TypeError(f"evolve() expects a Hermitian or ParametrizedHamiltonian, got {type(hamiltonian)}")

    @staticmethod
    def _solve(H: np.ndarray, coef: np.ndarray, h: np.ndarray, order: int) -> np.ndarray:
        """[rows, d, d] complex128 on the host: one launch of the solver kernel (``qmle_evolve_magnus`` on one and
        two wires, ``qmle_evolve_magnus_wide`` on three and four)."""
        if H.shape[-1] not in (2, 4, 8, 16):
            raise NotImplementedError(f"evolve(): Hamiltonians on {H.shape[-1]}x{H.shape[-1]} matrices are not "
                                      "supported (at most 4 wires, 16x16)")
        if H.shape[0] > N.EVOLVE_MAX_TERMS:
            raise NotImplementedError(f"evolve(): at most {N.EVOLVE_MAX_TERMS} terms, got {H.shape[0]}")
        if H.shape[-1] > 4:
            return N.evolve_magnus_wide(H, coef, h, order).cpu().numpy()
        return N.evolve_magnus(H, coef, h, order).cpu().numpy()

    @staticmethod
    def _operation(U: np.ndarray, batched: bool, wires, name, tangent, steps: int) -> Operation:
        """The evolved gate, recorded on the active tape: one matrix per sample when an argument was batched.
        ``evolve_steps``: the steps of the grid that produced it."""
        op_ = Operation(wires=wires, matrix=U if batched else U[0], name=name)
        if batched:
            op_._matrix_tangent = tangent
        op_.evolve_steps = steps
        return op_

    @classmethod
    def _with_jacobian(cls, H: np.ndarray, tables: list, step, order: int, wires, name, steps: int,
                       failed=None) -> Operation:
        """One launch of the solver with its derivatives -> the :class:`EvolvedGate`.  ``tables``: per term ``(values
        [rows, nodes], tangent terms)`` of :func:`_tracked_table`; ``step``: the same for the step, ``[rows, 1]``.  The
        directions are the distinct ``(leaf, flat index)`` pairs of all tangent terms, in order of appearance.
        ``failed``: rows the step doubling did not accept (NaN in every slot)."""
        if H.shape[-1] not in (2, 4):
            raise NotImplementedError(f"evolve(): Hamiltonians on {H.shape[-1]}x{H.shape[-1]} matrices are not "
                                      "supported (1 or 2 wires)")
        if H.shape[0] > N.EVOLVE_MAX_TERMS:
            raise NotImplementedError(f"evolve(): at most {N.EVOLVE_MAX_TERMS} terms, got {H.shape[0]}")
        rows, nodes = tables[0][0].shape
        directions: dict = {}
        for _vals, terms in tables + [step]:
            for lid, idx, _coef in terms:
                for v in np.unique(idx):
                    directions.setdefault((lid, int(v)), len(directions))
        if len(directions) > N.EVOLVE_MAX_DIRS:
            raise NotImplementedError(f"evolve(): {name or 'the gate'} depends on {len(directions)} leaf elements; at "
                                      f"most {N.EVOLVE_MAX_DIRS} per evolved gate are differentiated")
        D = max(1, len(directions))  # (a gate whose tangents are all empty: one zero direction)
        coef = np.stack([vals for vals, _terms in tables], axis=-1)
        dcoef, dh = np.zeros((rows, D, nodes, len(tables))), np.zeros((rows, D))
        for i, (_vals, terms) in enumerate(tables):
            for lid, idx, c in terms:
                for v in np.unique(idx):
                    m = idx == v
                    dcoef[:, directions[lid, int(v)], m, i] += c[:, m]
        for lid, idx, c in step[1]:
            dh[:, directions[lid, int(idx[0])]] += c[:, 0]
        out = N.evolve_magnus_jac(H, coef, step[0][:, 0], dcoef, dh, order).cpu().numpy()
        if failed is not None:
            out[failed] = np.nan
        return EvolvedGate(out[:, 0], wires, name, out[:, 1:1 + len(directions)], list(directions), steps)

    @classmethod
    def _static_wide_jacobian(cls, H: np.ndarray, t, rows: int, wires, name) -> Operation:
        """The :class:`EvolvedGate` of a static Hamiltonian on three or four wires whose time depends on a leaf: the
        solver's ``U`` and, per leaf element ``e`` the time depends on, ``dU/de = (dt/de) (-i H U)``."""
        _vals, terms = _tracked_table(t, rows, 1, "the time t")
        directions: dict = {}
        for lid, idx, _coef in terms:
            directions.setdefault((lid, int(idx[0])), len(directions))
        if len(directions) > N.EVOLVE_MAX_DIRS:
            raise NotImplementedError(f"evolve(): {name or 'the gate'} depends on {len(directions)} leaf elements; at "
                                      f"most {N.EVOLVE_MAX_DIRS} per evolved gate are differentiated")
        dt = np.zeros((rows, max(1, len(directions))))
        for lid, idx, coef in terms:
            dt[:, directions[lid, int(idx[0])]] += coef[:, 0]
        U = cls._solve(H, np.ones((rows, 1, 1)), _per_row(t, rows), 2)
        jac = dt[:, :, None, None] * static_jacobian(H[0], U)[:, None]
        return EvolvedGate(U, wires, name, jac[:, :len(directions)], list(directions), 1)

    @classmethod
    def _evolve_static(cls, hermitian: Hermitian, name: Optional[str]) -> Callable:
        H = np.asarray(hermitian.matrix, dtype=np.complex128)[None]

        def _apply(t, wires=0) -> Operation:
            rows = _rows_of([t])
            h = _per_row(t, rows)
            if _gradient_trace and _wide_trace and H.shape[-1] in (8, 16) and _tangent_state([t]) is None:
                return cls._static_wide_jacobian(H, t, rows, wires, name)
            if _gradient_trace and _tangent_state([t]) is None:  # one step of order 2, dcoef = 0, dh = dt
                return cls._with_jacobian(H, [(np.ones((rows, 1)), [])], _tracked_table(t, rows, 1, "the time t"), 2,
                                          wires, name, 1)
            U = cls._solve(H, np.ones((rows, 1, 1)), h, 2)
            return cls._operation(U, isinstance(t, Batched), wires, name, _tangent_state([t]), 1)

        return _apply

    @classmethod
    def _evolve_parametrized(cls, ph: ParametrizedHamiltonian, name: Optional[str], **kw: Any) -> Callable:
        atol, rtol, max_steps, throw, solver, magnus_steps = cls._options(kw)
        H = np.stack([np.asarray(m, dtype=np.complex128) for m in ph.H_mats])
        fns, wires, n_terms = ph.coeff_fns, ph.wires, ph.n_terms

        def _apply(coeff_args, T) -> Operation:
            params = tuple(coeff_args) if isinstance(coeff_args, (list, tuple)) else (coeff_args,)
            if len(params) != n_terms:
                raise ValueError(f"Expected {n_terms} parameter set(s) for a {n_terms}-term ParametrizedHamiltonian, "
                                 f"got {len(params)}.")
            if isinstance(T, Batched):
                span = [T] if T.ndim == 0 else [T[0], T[1]]
            else:
                span = [T] if np.ndim(T) == 0 else [T[0], T[1]]
            rows = _rows_of(list(params) + span)
            t1 = _per_row(span[-1], rows)
            t0 = _per_row(span[0], rows) if len(span) == 2 else np.zeros(rows)
            per_row_times = any(isinstance(x, Batched) for x in span)

            def fixed(n_steps: int, order: int) -> np.ndarray:
                h = (t1 - t0) / n_steps
                t = _node_times(t0, h, n_steps, order)
                coef = np.stack([_coefficients(f, p, t, per_row_times) for f, p in zip(fns, params)], axis=-1)
                return cls._solve(H, coef, h, order)

            def tracked_tables(n_steps: int, order: int):
                """(per term (values, tangent terms), the same for the step): host work only; raises what the
                recorder cannot track."""
                if any(isinstance(x, Batched) and x.tan is None for x in span):
                    raise NotImplementedError("evolve(): the evolution time depends on a differentiated argument "
                                              f"through an operation the recorder does not track; tracked are {_TRACKED}")
                a, b = (span[0], span[1]) if len(span) == 2 else (0.0, span[0])
                step = (b - a) / n_steps
                t = _tracked_nodes(a, step, n_steps, order)
                nodes = n_steps * (2 if order == 4 else 1)
                tables = []
                for i, (f, p_) in enumerate(zip(fns, params)):
                    with elementwise_tangents():
                        res = f(p_, t)
                    tables.append(_tracked_table(res, rows, nodes, f"the coefficient of term {i} of {name or 'the gate'}"))
                return tables, _tracked_table(step, rows, 1, "the step")

            def with_jacobian(n_steps: int, order: int, failed=None) -> Operation:
                tables, step = tracked_tables(n_steps, order)
                return cls._with_jacobian(H, tables, step, order, wires, name, n_steps, failed)

            tracked = _gradient_trace and _tangent_state(list(params) + span) is None
            if tracked and _wide_trace and H.shape[-1] in (8, 16):  # (before any device work)
                raise NotImplementedError(WIDE_JACOBIAN_LIMIT)
            steps = magnus_steps
            if solver in ("magnus2", "magnus4"):
                if tracked:
                    return with_jacobian(magnus_steps, 2 if solver == "magnus2" else 4)
                U = fixed(magnus_steps, 2 if solver == "magnus2" else 4)
            else:
                if tracked:  # what cannot be differentiated is refused before any device work
                    tracked_tables(_FIRST_GRID // 2, 4)
                U, ok, steps = cls._doubling(fixed, rows, H.shape[-1], atol + rtol, max_steps)
                if not ok.all():
                    if throw:
                        raise RuntimeError(
                            f"evolve(): step doubling reached max_steps={max_steps} without meeting atol + rtol = "
                            f"{atol + rtol:.3g} ({int((~ok).sum())} of {rows} row(s)); raise max_steps or loosen "
                            "the tolerances")
                    U[~ok] = np.nan
                if tracked and not steps:  # (throw=False and max_steps below the first grid: no grid was ever run)
                    raise RuntimeError(
                        f"evolve() inside a gradient trace: the solve failed before any grid ran (max_steps={max_steps} "
                        f"is below the first grid of {_FIRST_GRID} steps), so there is no grid to differentiate; raise "
                        "max_steps")
                if tracked:  # the accepted grid once more, with its derivatives
                    return with_jacobian(steps, 4, ~ok)
            return cls._operation(U, _has_batched(list(params) + span), wires, name,
                                  _tangent_state(list(params) + span), steps)

        return _apply

    @staticmethod
    def _doubling(fixed: Callable, rows: int, dim: int, tol: float, max_steps: int, on_device: bool = False):
        """-> (U of the last grid tried, accepted [rows], its steps), host arrays; see the module docstring.
        ``on_device``: ``fixed(n, 4)`` returns a device tensor and ``fixed(n, 4, prev)`` the pair ``(U_n, max |U_n -
        prev| per row)``, both on the device (the pulse solver): the previous grid never leaves it, one number -- the
        worst row's distance, NaN if any row is NaN -- crosses to the host per round and the matrices once at the end."""
        if max_steps < _FIRST_GRID:
            return np.full((rows, dim, dim), np.nan + 0j), np.zeros(rows, dtype=bool), 0
        prev, n = fixed(_FIRST_GRID // 2, 4), _FIRST_GRID
        while True:
            if on_device:
                import torch

                cur, err = fixed(n, 4, prev)
                accepted = float(torch.amax(err)) / 15.0 <= tol
            else:
                cur = fixed(n, 4)
                err = np.max(np.abs(cur - prev), axis=(1, 2))
                accepted = bool((err / 15.0 <= tol).all())
            if accepted or 2 * n > max_steps:
                if on_device:
                    cur, err = cur.cpu().numpy(), err.cpu().numpy()
                return cur, err / 15.0 <= tol, n
            prev, n = cur, 2 * n
