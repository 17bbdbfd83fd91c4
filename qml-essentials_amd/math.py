"""Quantum information helpers: the quantum Fisher information, the Fubini-Study metric, fidelity,
trace distance and phase difference.

API mirror of ``qml_essentials/math.py``.  Where the reference differentiates ``state_fn`` with
``jax.jacfwd`` and forms ``J^H J`` on one CPU, ``quantum_fisher_information`` /
``fubini_study_metric`` first look at what ``state_fn`` did: when it returned the result of exactly
one ``Model.__call__`` / ``Script.execute`` of type ``"state"`` / ``"density"`` whose differentiable
argument is ``params``, the metric is computed on the GPU (shifted circuits + ``qmle_gram``,
:meth:`script.Script.quantum_geometric_tensor`).  Anything else -- a plain NumPy callable -- is
differentiated on the host by a 4th-order central difference in fp64.
"""
from __future__ import annotations

from typing import Callable

import numpy as np

from .entanglement import logm_v  # noqa: F401  (math.py:7-28)

MAX_MIXED_QFI_QUBITS = 7  # the SLD formula runs eigh(rho) on the host
FD_STEP = 1e-3  # 4th-order central difference: truncation ~ h^4, rounding ~ eps / h

# which route the last call took, and how often each was taken ("gpu" / "fallback")
PATH_COUNTS = {"gpu": 0, "fallback": 0}
last_path = None


def _count(path: str) -> None:
    global last_path
    last_path = path
    PATH_COUNTS[path] += 1


def _to_numpy(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


# ---------------------------------------------------------------- pure / mixed formulas (host, fp64)
def _fubini_study_statevector(jac: np.ndarray, state: np.ndarray) -> np.ndarray:
    """``g = Re[<d_i psi|d_j psi> - <d_i psi|psi><psi|d_j psi>]`` for ``jac`` ``(d, P)``."""
    A = np.conj(jac.T) @ jac
    v = np.conj(jac.T) @ state
    return np.real(A - np.outer(v, np.conj(v)))


def _qfi_density(jac: np.ndarray, state: np.ndarray, eps: float = 1e-12) -> np.ndarray:
    """SLD quantum Fisher information of ``rho`` = ``state`` ``(d, d)`` with ``d rho / d theta_i`` =
    ``jac[:, :, i]`` (math.py:268-309): ``F_ij = sum_{kl} 2 Re(<k|d_i rho|l><l|d_j rho|k>) / (p_k + p_l)``
    over eigenvalue pairs with ``p_k + p_l > eps``."""
    evals, evecs = np.linalg.eigh(state)
    evals = np.where(np.real(evals) > 0.0, np.real(evals), 0.0)
    drho = np.moveaxis(jac, -1, 0)
    M = np.conj(evecs.T)[None] @ drho @ evecs[None]
    s = evals[:, None] + evals[None, :]
    weights = np.where(s > eps, 2.0 / np.where(s > eps, s, 1.0), 0.0)
    return np.real(np.einsum("ikl,jkl->ij", M * weights[None], np.conj(M)))


def _finite_difference(state_fn: Callable, params) -> tuple:
    """``(state, jac)`` with ``jac`` of shape ``state.shape + (P,)`` by the 4th-order central difference."""
    p0 = np.asarray(_to_numpy(params), dtype=np.float64)
    state = np.asarray(_to_numpy(state_fn(p0.copy())), dtype=np.complex128)
    flat = p0.reshape(-1)
    cols = []
    for i in range(flat.size):
        f = []
        for k in (2, 1, -1, -2):
            q = flat.copy()
            q[i] += k * FD_STEP
            f.append(np.asarray(_to_numpy(state_fn(q.reshape(p0.shape))), dtype=np.complex128))
        cols.append((-f[0] + 8.0 * f[1] - 8.0 * f[2] + f[3]) / (12.0 * FD_STEP))
    jac = np.stack(cols, axis=-1) if cols else np.zeros(state.shape + (0,), dtype=np.complex128)
    return state, jac


# ---------------------------------------------------------------- the GPU route
def _same_param(a, params) -> bool:
    if a is params:
        return True
    if a is None or not hasattr(a, "shape") and not isinstance(a, (list, tuple)):
        return False
    x, y = _to_numpy(a), _to_numpy(params)
    return x.shape == y.shape and x.dtype.kind in "fiu" and np.array_equal(x, y)


def _captured_metric(state_fn: Callable, params, want: str):
    """Run ``state_fn(params)`` under a capture.  Returns ``(result, Q or None, kind)``: ``Q`` is the
    GPU quantum geometric tensor (complex ``(P, P)``; for a noisy circuit the real mixed-state QFI / 4)
    when the capture applies, ``kind`` is ``"state"`` / ``"density"``."""
    from .tape import capturing

    with capturing() as recs:
        result = state_fn(params)
    if len(recs) != 1 or recs[0]["result"] is not result:
        return result, None, None
    rec = recs[0]
    if rec["type"] not in ("state", "density"):
        return result, None, None
    if rec["kind"] == "model":
        model = rec["model"]
        if rec["force_mean"] or not _same_param(rec["params"], params):
            return result, None, None
        if rec["type"] == "density" and not model.all_qubit_measurement:
            return result, None, None
        if np.ndim(_to_numpy(result)) != (1 if rec["type"] == "state" else 2):
            return result, None, None  # batched calls: the reference's shape rules decide
        if rec["noise_params"] is not None:
            model.noise_params = rec["noise_params"]
        if want == "fs" and rec["type"] == "density":
            return result, None, "density"
        q = model.quantum_geometric_tensor(params=rec["params"], inputs=rec["inputs"],
                                           enc_params=rec["enc_params"])
        return result, np.asarray(q), rec["type"]
    if rec["in_axes"] is not None or rec["shots"] is not None:
        return result, None, None
    args = tuple(rec["args"])
    hits = [k for k, a in enumerate(args) if a is params]
    if not hits:
        hits = [k for k, a in enumerate(args) if _same_param(a, params)]
    if len(hits) > 1:
        raise ValueError(f"params matches {len(hits)} arguments of the captured Script.execute call "
                         f"(positions {hits}); pass distinct arrays")
    if not hits:
        return result, None, None
    if want == "fs" and rec["type"] == "density":
        return result, None, "density"
    q = rec["script"].quantum_geometric_tensor(args=args, kwargs=rec["kwargs"], argnums=(hits[0],))
    return result, np.asarray(q), rec["type"]


def _shape_error(shape) -> ValueError:
    return ValueError("state_fn must return a state vector of shape (d,) or a density "
                      f"matrix of shape (d, d), got shape {tuple(shape)}.")


def _fs_density_error(shape) -> ValueError:
    return ValueError("The Fubini-Study metric is only defined for pure states; state_fn must return a "
                      f"state vector of shape (d,), got shape {tuple(shape)}.")


def quantum_fisher_information(state_fn: Callable, params) -> np.ndarray:
    r"""Quantum Fisher information (real, symmetric ``(P, P)``, ``P = params.size``) of the state
    ``state_fn(params)``: ``4 g`` (Fubini-Study) for a state vector ``(d,)``, the symmetric logarithmic
    derivative formula for a density matrix ``(d, d)`` (``math.py:332-384``).

    GPU route: ``state_fn`` returns, unchanged, the result of exactly one ``Model.__call__`` /
    ``Script.execute`` of type ``"state"`` or ``"density"`` that received ``params`` (by identity, else by
    equal value and shape) -- e.g. ``lambda p: model(params=p)``.  The derivative states are shifted
    circuits and their Gram matrix is formed on the device (noisy circuits: the density engine and the
    SLD formula on the host, at most 7 qubits).  Every other callable is differentiated on the host by
    a 4th-order central difference in fp64 (step ``FD_STEP``).  ``PATH_COUNTS`` / ``last_path`` tell which
    route was taken.

    Raises ``ValueError`` when ``state_fn`` returns neither a state vector nor a square matrix."""
    result, q, kind = _captured_metric(state_fn, params, "qfi")
    if q is not None:
        _count("gpu")
        return 4.0 * np.real(q)
    shape = np.shape(_to_numpy(result))
    if not (len(shape) == 1 or (len(shape) == 2 and shape[0] == shape[1])):
        raise _shape_error(shape)
    _count("fallback")
    state, jac = _finite_difference(state_fn, params)
    if state.ndim == 1:
        return 4.0 * _fubini_study_statevector(jac.reshape(state.shape[0], -1), state)
    return _qfi_density(jac.reshape(state.shape[0], state.shape[1], -1), state)


def fubini_study_metric(state_fn: Callable, params) -> np.ndarray:
    r"""Fubini-Study metric ``g = Re Q`` (real, symmetric ``(P, P)``) of the pure state ``state_fn(params)``
    (``math.py:387-431``); ``F = 4 g``.  Routes as in :func:`quantum_fisher_information` (GPU for a
    captured ``"state"`` call, 4th-order central differences on the host otherwise).

    Raises ``ValueError`` when ``state_fn`` does not return a state vector (density matrices included)."""
    result, q, kind = _captured_metric(state_fn, params, "fs")
    shape = np.shape(_to_numpy(result))
    if kind == "density" or len(shape) != 1:
        raise _fs_density_error(shape)
    if q is not None:
        _count("gpu")
        return np.real(q)
    _count("fallback")
    state, jac = _finite_difference(state_fn, params)
    return _fubini_study_statevector(jac.reshape(state.shape[0], -1), state)


# ---------------------------------------------------------------- distances (math.py:60-208)
def _is_statevector(x: np.ndarray) -> bool:
    return x.ndim <= 2 and (x.ndim == 1 or x.shape[-2] != x.shape[-1])


def _sqrt_matrix(rho: np.ndarray) -> np.ndarray:
    evs, vecs = np.linalg.eigh(rho)
    evs = np.where(np.real(evs) > 0.0, np.real(evs), 0.0)
    return (vecs * np.sqrt(evs)[..., None, :]) @ np.conj(np.swapaxes(vecs, -1, -2))


def _pair_einsum(s0: np.ndarray, s1: np.ndarray) -> np.ndarray:
    i0 = "ab" if s0.ndim > 1 else "b"
    i1 = "ab" if s1.ndim > 1 else "b"
    target = "a" if (s0.ndim > 1 or s1.ndim > 1) else ""
    return np.einsum(f"{i0},{i1}->{target}", np.conj(s0), s1)


def fidelity(state0, state1) -> np.ndarray:
    """Fidelity of two state vectors ``|<psi|phi>|^2`` (normalised first) or two density matrices
    ``(Tr sqrt(sqrt(rho) sigma sqrt(rho)))^2``; scalar or ``(B,)``."""
    s0 = np.asarray(_to_numpy(state0), dtype=np.complex128)
    s1 = np.asarray(_to_numpy(state1), dtype=np.complex128)
    if s0.shape[-1] != s1.shape[-1]:
        raise ValueError("The two states must have the same number of wires.")
    sv0, sv1 = _is_statevector(s0), _is_statevector(s1)
    if sv0 != sv1:
        raise ValueError("Both states must be of the same kind "
                         "(both state vectors or both density matrices).")
    if sv0:
        n0 = np.linalg.norm(s0, axis=-1, keepdims=True)
        n1 = np.linalg.norm(s1, axis=-1, keepdims=True)
        s0 = s0 / np.where(n0 > 0, n0, 1.0)
        s1 = s1 / np.where(n1 > 0, n1, 1.0)
        return np.abs(_pair_einsum(s0, s1)) ** 2
    r = _sqrt_matrix(s0)
    evs = np.real(np.linalg.eigvalsh(r @ s1 @ r))
    evs = np.where(evs > 0.0, evs, 0.0)
    return np.sum(np.sqrt(evs), axis=-1) ** 2


def trace_distance(state0, state1) -> np.ndarray:
    """``Tr|rho - sigma| / 2`` of density matrices ``(d, d)`` or ``(B, d, d)``."""
    s0 = np.asarray(_to_numpy(state0), dtype=np.complex128)
    s1 = np.asarray(_to_numpy(state1), dtype=np.complex128)
    if s0.shape[-1] != s1.shape[-1]:
        raise ValueError("The two states must have the same number of wires.")
    return np.sum(np.abs(np.linalg.eigvalsh(s0 - s1)), axis=-1) / 2


def phase_difference(state0, state1) -> np.ndarray:
    """``angle(<psi|phi>)`` of state vectors ``(d,)`` or ``(B, d)``."""
    s0 = np.asarray(_to_numpy(state0), dtype=np.complex128)
    s1 = np.asarray(_to_numpy(state1), dtype=np.complex128)
    if s0.shape[-1] != s1.shape[-1]:
        raise ValueError("The two states must have the same number of wires.")
    return np.angle(_pair_einsum(s0, s1))
