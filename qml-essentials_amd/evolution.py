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

Gradients.  Tangents are dropped through ``evolve``: an evolved gate whose arguments depend on a differentiated leaf
carries "derivative unknown", and ``Script.gradient`` refuses it as it refuses every untracked transformation.
Differentiating through the solver is out of scope, as are matrices larger than 4x4.

Pulse-level gates (:mod:`pulses`) do not come through ``evolve``: their RX / RY leaves are solved by a kernel of their
own that evaluates the envelopes on the device, all leaves of a tape in one launch.  They share the solver defaults
below and the step-doubling rule (``_doubling``).
"""
from __future__ import annotations

from typing import Any, Callable, Optional, Union

import numpy as np

from . import _native as N
from .batching import Batched
from .operations import Hermitian, Operation, ParametrizedHamiltonian

_SQRT3 = np.sqrt(3.0)
_C1, _C2 = 0.5 - _SQRT3 / 6.0, 0.5 + _SQRT3 / 6.0
_FIRST_GRID = 32  # step doubling starts here


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
        """[rows, d, d] complex128 on the host: one launch of the solver kernel."""
        if H.shape[-1] not in (2, 4):
            raise NotImplementedError(f"evolve(): Hamiltonians on {H.shape[-1]}x{H.shape[-1]} matrices are not "
                                      "supported (1 or 2 wires)")
        if H.shape[0] > N.EVOLVE_MAX_TERMS:
            raise NotImplementedError(f"evolve(): at most {N.EVOLVE_MAX_TERMS} terms, got {H.shape[0]}")
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
    def _evolve_static(cls, hermitian: Hermitian, name: Optional[str]) -> Callable:
        H = np.asarray(hermitian.matrix, dtype=np.complex128)[None]

        def _apply(t, wires=0) -> Operation:
            rows = _rows_of([t])
            h = _per_row(t, rows)
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

            steps = magnus_steps
            if solver in ("magnus2", "magnus4"):
                U = fixed(magnus_steps, 2 if solver == "magnus2" else 4)
            else:
                U, ok, steps = cls._doubling(fixed, rows, H.shape[-1], atol + rtol, max_steps)
                if not ok.all():
                    if throw:
                        raise RuntimeError(
                            f"evolve(): step doubling reached max_steps={max_steps} without meeting atol + rtol = "
                            f"{atol + rtol:.3g} ({int((~ok).sum())} of {rows} row(s)); raise max_steps or loosen "
                            "the tolerances")
                    U[~ok] = np.nan
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
