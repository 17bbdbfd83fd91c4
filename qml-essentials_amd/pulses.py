"""Pulse-level gates: every gate of a circuit as a sequence of shaped microwave pulses -- API mirror of
``qml_essentials/pulses.py`` (``PulseParams``, ``PulseEnvelope``, ``PulseInformation``, ``PulseGates``,
``PulseParamManager``).

Leaves.  A pulse circuit decomposes into four leaf gates.  Three of them have a constant Hamiltonian and need no
solver; they are recorded as the ordinary operations they are equal to and keep their angle slots and tangents:
  ``RZ(w; p)``   exp(-i p0 w Z)                    = ``op.RZ(2 p0 w)``
  ``CZ(p)``      exp(-i pi^2 p |11><11|)           = ``ControlledPhaseShift(-pi^2 p)``
  H correction   exp(+i pi/2 I)                    = the constant matrix ``i I``
``RX`` / ``RY`` are driven by a shaped pulse, ``H(t) = cx(t) X + cy(t) Y``, and record a :class:`PulseRotation`: an
operation that carries a *solve request* (axis, envelope parameters, ``w`` and the duration ``T = pulse_params[-1]``,
each a float or a per-sample column) instead of a matrix.

One launch per tape.  :func:`resolve` collects the unresolved requests of a tape -- one solve for an unbatched
request, one per sample for a batched one, identical unbatched requests once -- and hands them to
``qmle_pulse_unitaries`` (``csrc/qmle_evolve.hip``) in ONE launch per grid; the kernel evaluates the envelope and the
carrier itself, so no coefficient table is built.  ``Script.execute`` and ``simulation.LoweredTape`` resolve a tape
before they read it; a request whose ``matrix`` is read earlier resolves by a solve of its own.  An unbatched request
lowers as a constant ``MAT1``, a batched one as ``MAT1_ROW``.  Solver choice follows ``Evolution._solver_defaults``:
``magnus2`` / ``magnus4`` run the grid of ``magnus_steps`` steps, ``dopri8`` / ``dopri5`` the step-doubling rule of
:mod:`evolution` (16, 32, 64, ... steps of order 4) with the previous grid kept on the device -- one number, the
worst ``max |U_N - U_{N/2}|``, crosses to the host per round.

The centre time.  The reference's coefficient functions centre the envelope at ``t_c = t / 2`` with ``t`` the RUNNING
time, not the duration: ``gaussian`` is ``A exp(-(t / 2 sigma)^2 / 2)``, ``square`` is ``A`` for ``t <= width``,
``cosine`` is ``A cos(pi clip(t / (2 width), +-1/2))``, the ``drag`` derivative term is ``g (-(t / 2) / sigma^2)``.
Its optimised default parameters are tuned to exactly this definition, which is therefore reproduced here.

The support rule.  ``square`` and ``cosine`` vanish identically for ``t > width``; the grid covers ``[0, min(T,
width)]`` for them (``[0, T]`` otherwise), so that neither the jump nor the kink falls inside a step.

Gradients.  ``Script.vjp`` and ``Model.gradient(gate_mode="pulse", method="adjoint")`` differentiate through a pulse
solve: a request whose arguments depend on a differentiated leaf reports itself as a MATRIX-COTANGENT op
(:attr:`PulseRotation.wants_matrix_cotangent`), :func:`resolve_for_gradient` fills ``U`` and keeps the exact grid
sensitivities ``J = dU/d(p0, p1, p2, w, T)`` of all such requests of a tape from one :func:`solve_with_jacobian` call
per launch group, the backward sweep returns ``G`` with ``dC/dtheta = 2 Re sum_ac G[a][c] dU[a][c]/dtheta``
(:func:`adjoint.adjoint_slot_and_matrix_gradient`), and :meth:`PulseRotation.leaf_jacobian_terms` is the chain rule
onto the leaves.  The virtual ``RZ`` and the ``ControlledPhaseShift`` of ``CZ`` are ordinary angle slots of the same
sweep.  Everywhere else -- ``Script.gradient`` (parameter shift: a pulse leaf has no shift rule), the quantum
geometric tensor, the compiled device path, the torch bridge -- such a request still has "derivative unknown" and is
refused, as for ``evolve()``.  :mod:`qoc` composes the same sensitivities into the gradients of its cost functions.
Out of scope: pulse-event tapes / ``draw_pulse``, ``PulseInformation.update_params`` from CSV, ``PauliRot``.
"""
from __future__ import annotations

import logging
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from . import operations as op
from .batching import Batched, as_param, param_tangent
from .evolution import Evolution, _tangent_state
from .operations import Operation
from .unitary import UnitaryGates
from .utils import as_key, safe_random_split

log = logging.getLogger(__name__)


@dataclass
class DecompositionStep:
    """One step of a composite pulse gate: the child gate, its wires (``"all"``, ``"target"`` or ``"control"`` of the
    parent's) and the map from the parent's angle(s) to the child's (``None``: unchanged)."""

    gate: "PulseParams"
    wire_fn: str = "all"
    angle_fn: Optional[Callable] = None


@dataclass(frozen=True)
class PulseStateSnapshot:
    """Snapshot of the mutable global pulse configuration."""

    envelope: str
    rwa: bool
    frame: str
    leaf_params: Dict[str, np.ndarray]


class PulseParams:
    """Hierarchical pulse parameters: a leaf holds its own array, a composite a list of
    :class:`DecompositionStep` whose children's arrays it concatenates (``pulses.py:44-300``)."""

    def __init__(self, name: str = "", params=None, decomposition: Optional[List[DecompositionStep]] = None) -> None:
        assert (params is None) != (decomposition is None), \
            "Exactly one of `params` or `decomposition` must be provided."
        self.decomposition = decomposition
        self._pulse_obj = [step.gate for step in decomposition] if decomposition else None
        if params is not None:
            self._params = params
        self.name = name

    def __len__(self) -> int:
        return len(self.params)

    def __getitem__(self, idx):
        return self.params[idx] if self.is_leaf else self.childs[idx].params

    def __str__(self) -> str:
        return self.name

    __repr__ = __str__

    @property
    def is_leaf(self) -> bool:
        return self._pulse_obj is None

    @property
    def size(self) -> int:
        return len(self)

    @property
    def leafs(self) -> List["PulseParams"]:
        """The distinct leaves below this node."""
        if self.is_leaf:
            return [self]
        out: List[PulseParams] = []
        for child in self._pulse_obj:
            for leaf in child.leafs:
                if not any(leaf is seen for seen in out):
                    out.append(leaf)
        return out

    @property
    def childs(self) -> List["PulseParams"]:
        return [] if self.is_leaf else self._pulse_obj

    @property
    def shape(self) -> list:
        return [len(self.params)] if self.is_leaf else [child.shape for child in self.childs]

    @property
    def params(self):
        if self.is_leaf:
            return self._params
        return np.concatenate([np.asarray(p) for p in self.split_params(None, leafs=False)])

    @params.setter
    def params(self, value) -> None:
        if self.is_leaf:
            assert isinstance(value, (np.ndarray, Batched)), "params must be an array"
            self._params = value
            return
        idx = 0
        for child in self.childs:
            child.params = value[idx:idx + child.size]
            idx += child.size

    @property
    def leaf_params(self):
        if self.is_leaf:
            return self._params
        return np.concatenate([np.asarray(p) for p in self.split_params(None, leafs=True)])

    @leaf_params.setter
    def leaf_params(self, value) -> None:
        if self.is_leaf:
            self._params = value
            return
        idx = 0
        for leaf in self.leafs:
            leaf.params = value[idx:idx + leaf.size]
            idx += leaf.size

    def split_params(self, params=None, leafs: bool = False):
        """``params`` (default: the stored ones) cut into one array per child (or per leaf)."""
        if self.is_leaf:
            return self._params if params is None else params
        objs = self.leafs if leafs else self.childs
        if params is None:
            return [o.params for o in objs]
        out, idx = [], 0
        for o in objs:
            out.append(params[idx:idx + o.size])
            idx += o.size
        return out


def _le(a, b):
    return np.less_equal(a, b)  # (a ufunc call: Batched values take part through __array_ufunc__)


class PulseEnvelope:
    """Registry of envelope shapes ``(p, t, t_c) -> amplitude`` (no carrier) and of their optimised per-gate default
    parameters.  The functions take NumPy arrays and ``batching.Batched`` values alike."""

    @staticmethod
    def gaussian(p, t, t_c):
        """``p = [A, sigma]``."""
        return p[0] * np.exp(-0.5 * ((t - t_c) / p[1]) ** 2)

    @staticmethod
    def square(p, t, t_c):
        """``p = [A, width]``."""
        return p[0] * _le(np.abs(t - t_c), p[1] / 2)

    @staticmethod
    def cosine(p, t, t_c):
        """``p = [A, width]``."""
        x = np.minimum(np.maximum((t - t_c) / p[1], -0.5), 0.5)
        return p[0] * np.cos(np.pi * x)

    @staticmethod
    def drag(p, t, t_c):
        """``p = [A, beta, sigma]``."""
        g = p[0] * np.exp(-0.5 * ((t - t_c) / p[2]) ** 2)
        dg = g * (-(t - t_c) / p[2] ** 2)
        return g + p[1] * dg

    @staticmethod
    def sech(p, t, t_c):
        """``p = [A, sigma]``."""
        return p[0] / np.cosh((t - t_c) / p[1])

    # n_envelope_params: the envelope's own parameters; the evolution time is always the last element of the full
    # pulse parameter vector
    REGISTRY = {
        "gaussian": {"fn": gaussian.__func__, "n_envelope_params": 2, "defaults": {
            "RX": np.array([0.38009941846766804, 1.631698142660167, 3.007403822238108]),
            "RY": np.array([0.3836652338514791, 1.616595983505249, 2.9794135093698966])}},
        "square": {"fn": square.__func__, "n_envelope_params": 2, "defaults": {
            "RX": np.array([1.209655637514602, 0.8266815576721239, 1.1483122857413859]),
            "RY": np.array([1.0287942142779052, 0.9860505130182093, 0.9720116870310977])}},
        "cosine": {"fn": cosine.__func__, "n_envelope_params": 2, "defaults": {
            "RX": np.array([1.0, 1.0, 1.0]), "RY": np.array([1.0, 1.0, 1.0])}},
        "drag": {"fn": drag.__func__, "n_envelope_params": 3, "defaults": {
            "RX": np.array([0.326562746114197, 0.4002767596709071, 5.3228107728890315, 3.141300761986467]),
            "RY": np.array([0.323287924190616, 0.4065017233024265, 7.00299644871222, 3.139481229843545])}},
        "sech": {"fn": sech.__func__, "n_envelope_params": 2, "defaults": {
            "RX": np.array([1.0, 1.0, 1.0]), "RY": np.array([1.0, 1.0, 1.0])}},
        "general": {"fn": None, "n_envelope_params": 0, "defaults": {
            "RZ": np.array([0.5]), "CZ": np.array([0.3183098783513154])}},
    }

    @staticmethod
    def available() -> List[str]:
        return list(PulseEnvelope.REGISTRY.keys())

    @staticmethod
    def get(name: str) -> dict:
        if name not in PulseEnvelope.REGISTRY:
            raise ValueError(f"Unknown pulse envelope '{name}'. Available: {PulseEnvelope.available()}")
        return PulseEnvelope.REGISTRY[name]

    @staticmethod
    def build_coeff_fns(envelope_fn: Callable, omega_c: float, omega_q: float, rwa: bool = True,
                        frame: str = "drive") -> Tuple[Callable, Callable, Callable, Callable]:
        """``(RX_X, RX_Y, RY_X, RY_Y)``: the X and Y coefficients ``(p, t)`` of the interaction-picture drive
        Hamiltonians of RX (carrier phase 0) and RY (carrier phase +pi/2), ``p = [envelope parameters..., w]``.
        ``rwa``: the rotating-wave form ``(env / 2) w`` on the gate's own axis; otherwise the exact coefficients,
        literally (``frame="lab"``) or through the product-to-sum identities (``"drive"``) -- the same numbers.
        The envelope is centred at ``t_c = t / 2`` (module docstring)."""
        if frame not in ("lab", "drive"):
            raise ValueError(f"Unknown frame {frame!r}; expected 'lab' or 'drive'.")

        def env(p, t):
            return envelope_fn(p, t, t / 2)

        if rwa:
            def rx_x(p, t):
                return 0.5 * env(p, t) * p[-1]

            def rx_y(p, t):
                return 0.0 * (0.5 * env(p, t) * p[-1])

            def ry_x(p, t):
                return 0.0 * (0.5 * env(p, t) * p[-1])

            def ry_y(p, t):
                return 0.5 * env(p, t) * p[-1]

            return rx_x, rx_y, ry_x, ry_y

        if frame == "drive":
            omega_d, omega_s = omega_c - omega_q, omega_c + omega_q

            def rx_x(p, t):
                return env(p, t) * (0.5 * (np.cos(omega_d * t) + np.cos(omega_s * t))) * p[-1]

            def rx_y(p, t):
                return env(p, t) * (-0.5 * (np.sin(omega_s * t) - np.sin(omega_d * t))) * p[-1]

            def ry_x(p, t):
                return env(p, t) * (-0.5 * (np.sin(omega_s * t) + np.sin(omega_d * t))) * p[-1]

            def ry_y(p, t):
                return env(p, t) * (-0.5 * (np.cos(omega_s * t) - np.cos(omega_d * t))) * p[-1]

            return rx_x, rx_y, ry_x, ry_y

        def rx_x(p, t):
            return env(p, t) * np.cos(omega_c * t) * np.cos(omega_q * t) * p[-1]

        def rx_y(p, t):
            return -env(p, t) * np.cos(omega_c * t) * np.sin(omega_q * t) * p[-1]

        def ry_x(p, t):
            return env(p, t) * np.cos(omega_c * t + np.pi / 2) * np.cos(omega_q * t) * p[-1]

        def ry_y(p, t):
            return -env(p, t) * np.cos(omega_c * t + np.pi / 2) * np.sin(omega_q * t) * p[-1]

        return rx_x, rx_y, ry_x, ry_y


class PulseInformation:
    """The active envelope, the RWA / frame flags and the :class:`PulseParams` trees of every gate.
    :meth:`set_envelope` rebuilds the trees so that counts and defaults match the envelope."""

    DEFAULT_ENVELOPE: str = "drag"
    DEFAULT_RWA: bool = True
    DEFAULT_FRAME: str = "drive"
    LEAF_GATE_NAMES: Tuple[str, ...] = ("RX", "RY", "RZ", "CZ")

    _envelope: str = DEFAULT_ENVELOPE
    _rwa: bool = DEFAULT_RWA
    _frame: str = DEFAULT_FRAME

    @classmethod
    def _build_leaf_gates(cls) -> None:
        defaults = PulseEnvelope.get(cls._envelope)["defaults"]
        general = PulseEnvelope.get("general")["defaults"]
        cls.RX = PulseParams(name="RX", params=np.array(defaults["RX"]))
        cls.RY = PulseParams(name="RY", params=np.array(defaults["RY"]))
        cls.RZ = PulseParams(name="RZ", params=np.array(general["RZ"]))
        cls.CZ = PulseParams(name="CZ", params=np.array(general["CZ"]))

    @classmethod
    def _build_composite_gates(cls) -> None:
        S, pi = DecompositionStep, np.pi
        zero = lambda w: 0.0  # noqa: E731
        cls.H = PulseParams(name="H", decomposition=[S(cls.RZ, "all", lambda w: pi), S(cls.RY, "all", lambda w: pi / 2)])
        cls.CX = PulseParams(name="CX", decomposition=[S(cls.H, "target", zero), S(cls.CZ, "all", zero),
                                                       S(cls.H, "target", zero)])
        cls.CY = PulseParams(name="CY", decomposition=[S(cls.RZ, "target", lambda w: -pi / 2), S(cls.CX, "all"),
                                                       S(cls.RZ, "target", lambda w: pi / 2)])
        cls.CRX = PulseParams(name="CRX", decomposition=[
            S(cls.RZ, "target", lambda w: pi / 2), S(cls.RY, "target", lambda w: w / 2), S(cls.CX, "all", zero),
            S(cls.RY, "target", lambda w: -w / 2), S(cls.CX, "all", zero), S(cls.RZ, "target", lambda w: -pi / 2)])
        cls.CRY = PulseParams(name="CRY", decomposition=[
            S(cls.RY, "target", lambda w: w / 2), S(cls.CX, "all", zero), S(cls.RY, "target", lambda w: -w / 2),
            S(cls.CX, "all", zero)])
        cls.CRZ = PulseParams(name="CRZ", decomposition=[
            S(cls.RZ, "target", lambda w: w / 2), S(cls.CX, "all", zero), S(cls.RZ, "target", lambda w: -w / 2),
            S(cls.CX, "all", zero)])
        cls.CPhase = PulseParams(name="CPhase", decomposition=[
            S(cls.RZ, "control", lambda w: w / 2), S(cls.RZ, "target", lambda w: w / 2), S(cls.CX, "all", zero),
            S(cls.RZ, "target", lambda w: -w / 2), S(cls.CX, "all", zero)])
        cls.RZZ = PulseParams(name="RZZ", decomposition=[
            S(cls.CX, "all", zero), S(cls.RZ, "target", lambda w: w), S(cls.CX, "all", zero)])
        cls.RXX = PulseParams(name="RXX", decomposition=[
            S(cls.H, "control", zero), S(cls.H, "target", zero), S(cls.CX, "all", zero),
            S(cls.RZ, "target", lambda w: w), S(cls.CX, "all", zero), S(cls.H, "control", zero),
            S(cls.H, "target", zero)])
        cls.RYY = PulseParams(name="RYY", decomposition=[
            S(cls.RX, "control", lambda w: pi / 2), S(cls.RX, "target", lambda w: pi / 2), S(cls.CX, "all", zero),
            S(cls.RZ, "target", lambda w: w), S(cls.CX, "all", zero), S(cls.RX, "control", lambda w: -pi / 2),
            S(cls.RX, "target", lambda w: -pi / 2)])
        cls.RZX = PulseParams(name="RZX", decomposition=[
            S(cls.H, "target", zero), S(cls.CX, "all", zero), S(cls.RZ, "target", lambda w: w),
            S(cls.CX, "all", zero), S(cls.H, "target", zero)])
        cls.Rot = PulseParams(name="Rot", decomposition=[
            S(cls.RZ, "all", lambda w: w[0]), S(cls.RY, "all", lambda w: w[1]), S(cls.RZ, "all", lambda w: w[2])])
        cls.unique_gate_set = [cls.RX, cls.RY, cls.RZ, cls.CZ]

    @classmethod
    def set_envelope(cls, name: str, rwa: Optional[bool] = None, frame: Optional[str] = None) -> None:
        """Switch the envelope (and optionally the RWA flag and the frame), rebuild every tree with the envelope's
        defaults and the coefficient functions of :class:`PulseGates`."""
        info = PulseEnvelope.get(name)  # validates the name
        if frame is not None and frame not in ("lab", "drive"):
            raise ValueError(f"Unknown frame {frame!r}; expected 'lab' or 'drive'.")
        cls._envelope = name
        if rwa is not None:
            cls._rwa = bool(rwa)
        if frame is not None:
            cls._frame = frame
        cls._build_leaf_gates()
        cls._build_composite_gates()
        rx_x, rx_y, ry_x, ry_y = PulseEnvelope.build_coeff_fns(info["fn"], PulseGates.omega_c, PulseGates.omega_q,
                                                               rwa=cls._rwa, frame=cls._frame)
        PulseGates._coeff_RX_X, PulseGates._coeff_RX_Y = staticmethod(rx_x), staticmethod(rx_y)
        PulseGates._coeff_RY_X, PulseGates._coeff_RY_Y = staticmethod(ry_x), staticmethod(ry_y)
        PulseGates._coeff_Sx, PulseGates._coeff_Sy = staticmethod(rx_x), staticmethod(ry_y)
        PulseGates._active_envelope, PulseGates._active_rwa, PulseGates._active_frame = name, cls._rwa, cls._frame
        log.info(f"Pulse envelope set to '{name}' (RWA {'on' if cls._rwa else 'off'}, frame={cls._frame})")

    @classmethod
    def set_rwa(cls, rwa: bool) -> None:
        cls.set_envelope(cls._envelope, rwa=bool(rwa))

    @classmethod
    def get_envelope(cls) -> str:
        return cls._envelope

    @classmethod
    def get_rwa(cls) -> bool:
        return cls._rwa

    @classmethod
    def set_frame(cls, frame: str) -> None:
        cls.set_envelope(cls._envelope, frame=str(frame))

    @classmethod
    def get_frame(cls) -> str:
        return cls._frame

    @classmethod
    def snapshot_state(cls) -> PulseStateSnapshot:
        leaf_params = {}
        for name in cls.LEAF_GATE_NAMES:
            gate = getattr(cls, name, None)
            if gate is not None:
                leaf_params[name] = np.array(gate.params)
        return PulseStateSnapshot(envelope=cls._envelope, rwa=cls._rwa, frame=cls._frame, leaf_params=leaf_params)

    @classmethod
    def restore_state(cls, snapshot: PulseStateSnapshot) -> None:
        cls.set_envelope(snapshot.envelope, rwa=snapshot.rwa, frame=snapshot.frame)
        for name, params in snapshot.leaf_params.items():
            gate = cls.gate_by_name(name)
            if gate is None or not gate.is_leaf:
                raise ValueError(f"Cannot restore unknown leaf pulse gate {name!r}.")
            if np.shape(gate.params) != np.shape(params):
                raise ValueError(f"Snapshot for {name!r} has shape {np.shape(params)}, but active gate expects "
                                 f"{np.shape(gate.params)}.")
            gate.params = np.array(params)

    @classmethod
    @contextmanager
    def preserve_state(cls):
        """Keep the global pulse state across the mutations made inside the block."""
        snapshot = cls.snapshot_state()
        try:
            yield snapshot
        finally:
            cls.restore_state(snapshot)

    @classmethod
    def reset_defaults(cls, envelope: Optional[str] = None, rwa: Optional[bool] = None,
                       frame: Optional[str] = None) -> None:
        cls.set_envelope(cls.DEFAULT_ENVELOPE if envelope is None else envelope,
                         rwa=cls.DEFAULT_RWA if rwa is None else rwa,
                         frame=cls.DEFAULT_FRAME if frame is None else frame)

    @staticmethod
    def gate_by_name(gate):
        name = gate if isinstance(gate, str) else gate.__name__
        found = getattr(PulseInformation, name, None)
        return found if isinstance(found, PulseParams) else None

    @staticmethod
    def num_params(gate) -> int:
        return len(PulseInformation.gate_by_name(gate))

    @staticmethod
    def shuffle_params(random_key) -> None:
        """Uniform random parameters in [0, 1) for the four leaf gates."""
        for gate in PulseInformation.unique_gate_set:
            random_key, sub_key = safe_random_split(random_key)
            gate.params = as_key(sub_key).generator().uniform(size=len(gate))


# ---- the solve request ------------------------------------------------------------------------------------------------
def _first(pulse_params):
    """The single parameter of an RZ / CZ leaf (a scalar or a one-element vector, possibly batched)."""
    if isinstance(pulse_params, Batched):
        return pulse_params.reshape(-1)[0]
    return float(np.asarray(pulse_params, dtype=np.float64).reshape(-1)[0])


def _tracked_terms(terms, what: str):
    """The tangent terms ``[(leaf, index, coef)]`` of a recorded argument, refused when the recorder lost track."""
    if terms is None:
        raise NotImplementedError(f"qoc: {what} depends on the pulse parameters in a way the tape recorder does not "
                                  "track (only sums, constant factors and products are)")
    return terms


# kernel slot (0-based among the five derivatives p0, p1, p2, w, T) of the PulseRotation arguments T and w; the
# envelope parameters come first, in order (PulseRotation._arg_tangents: envelope parameters, then T, then w)
_SLOT_T, _SLOT_W = 4, 3


class PulseRotation(Operation):
    """An RX / RY pulse leaf: the request ``(axis, envelope parameters, w, T)`` under the envelope, the coefficient
    mode (``"rwa"``, ``"lab"`` or ``"drive"``) and the frequencies that were active when it was recorded.  Its matrix
    -- 2x2, or ``[B, 2, 2]`` when an argument is batched -- is filled in by :func:`resolve`."""

    _num_wires = 1

    def __init__(self, axis: str, w, pulse_params, wires=0, record: bool = True) -> None:
        if axis not in ("X", "Y"):
            raise ValueError(f"PulseRotation: axis must be 'X' or 'Y', got {axis!r}")
        envelope = PulseInformation.get_envelope()
        n_env = PulseEnvelope.get(envelope)["n_envelope_params"]
        if len(pulse_params) != n_env + 1:
            raise ValueError(f"R{axis} with the '{envelope}' envelope expects {n_env + 1} pulse parameters, got "
                             f"{len(pulse_params)}")
        values = [pulse_params[k] for k in range(n_env + 1)] + [w]
        self.axis, self.envelope = axis, envelope
        self.mode = "rwa" if PulseInformation.get_rwa() else PulseInformation.get_frame()
        self.omega_c, self.omega_q = float(PulseGates.omega_c), float(PulseGates.omega_q)
        self.env_params = [as_param(v) for v in values[:n_env]]
        self.T, self.w = as_param(values[n_env]), as_param(values[n_env + 1])
        # (None = "derivative unknown" for every consumer that differentiates angles only: parameter shift, the
        # quantum geometric tensor, compiled calls; ``Script.vjp`` reads ``wants_matrix_cotangent`` instead)
        self._matrix_tangent = _tangent_state(values)
        # per argument (envelope parameters..., T, w): the leaf elements it depends on -- what ``qoc`` and
        # ``Script.vjp`` map the columns of the solve's Jacobian onto
        self._arg_tangents = [param_tangent(v) for v in values]
        self._jacobian = None  # [rows, 5, 2, 2] complex128 once resolve_for_gradient solved the request
        self.evolve_steps = None
        super().__init__(wires=wires, record=record, name="R" + axis)

    @property
    def rows(self) -> int:
        """1 for an unbatched request, else the batch size."""
        b = 1
        for v in self.env_params + [self.T, self.w]:
            if isinstance(v, np.ndarray) and v.ndim:
                if b not in (1, v.shape[0]):
                    raise ValueError(f"{self.name}: inconsistent batch sizes {b} vs {v.shape[0]}")
                b = v.shape[0]
        return b

    @property
    def batched_request(self) -> bool:
        return any(isinstance(v, np.ndarray) and v.ndim for v in self.env_params + [self.T, self.w])

    def group(self) -> tuple:
        """What has to agree for two requests to share a launch."""
        return self.envelope, self.mode, self.omega_c, self.omega_q

    def solves(self) -> np.ndarray:
        """``[rows, 8]``: the kernel's columns ``p0, p1, p2, w, T, axis`` and padding."""
        t = np.zeros((self.rows, 8), dtype=np.float64)
        for k, v in enumerate(self.env_params):
            t[:, k] = v
        t[:, 3], t[:, 4], t[:, 5] = self.w, self.T, 0.0 if self.axis == "X" else 1.0
        return t

    @property
    def wants_matrix_cotangent(self) -> bool:
        """True when an argument depends on a differentiated leaf: the gradient of a cost by that leaf goes through
        the matrix cotangent of this gate and :meth:`leaf_jacobian_terms` (also when the recorder lost track of
        the dependence -- the chain rule then raises)."""
        return self._matrix_tangent is None

    def leaf_jacobian_terms(self) -> list:
        """``[(leaf, slot, index, coef)]``: the solve's derivative in kernel slot ``slot``, times ``coef`` ``[C]``,
        adds to the derivative by element ``index`` of leaf ``leaf`` -- argument by argument (envelope parameters,
        ``T``, ``w``)."""
        slots = list(range(len(self.env_params))) + [_SLOT_T, _SLOT_W]
        return [(leaf, slot, index, coef) for slot, terms in zip(slots, self._arg_tangents)
                for leaf, index, coef in _tracked_terms(terms, f"an argument of {self!r}")]

    def jacobian_terms(self) -> list:
        """:meth:`leaf_jacobian_terms` without the leaf (``qoc``: one leaf) -> ``[(slot, index, coef)]``."""
        return [(slot, index, coef) for _leaf, slot, index, coef in self.leaf_jacobian_terms()]

    @property
    def jacobian(self) -> np.ndarray:
        """``[rows, 5, 2, 2]`` complex128: ``dU/d(p0, p1, p2, w, T)`` per solve, kept by
        :func:`resolve_for_gradient`."""
        if self._jacobian is None:
            resolve_for_gradient([self])
        return self._jacobian

    def _resolved(self) -> None:
        if self._matrix is None:
            resolve([self])

    @property
    def matrix(self) -> np.ndarray:
        self._resolved()
        return self._matrix

    def matrix_columns(self) -> list:
        self._resolved()
        return super().matrix_columns()

    def __repr__(self) -> str:
        return f"Pulse{self.name}(envelope={self.envelope}, mode={self.mode}, wires={self.wires})"


def _launch_all(table: np.ndarray, envelope: str, mode: str, omega_c: float, omega_q: float):
    """Every solve of ``table`` under the solver defaults of :class:`Evolution` -> (U ``[n, 2, 2]`` complex128 on the
    host, steps of the grid that produced it)."""
    atol, rtol, max_steps, throw, solver, magnus_steps = Evolution._options({})
    solves = N.require_gpu().from_numpy(np.ascontiguousarray(table)).to(N.current_device())

    def fixed(n_steps: int, order: int, prev=None):
        return N.pulse_unitaries(solves, envelope, mode, omega_c, omega_q, order, n_steps, prev=prev,
                                 want_err=prev is not None)

    if solver in ("magnus2", "magnus4"):
        return fixed(magnus_steps, 2 if solver == "magnus2" else 4).cpu().numpy(), magnus_steps
    U, ok, steps = Evolution._doubling(fixed, table.shape[0], 2, atol + rtol, max_steps, on_device=True)
    if not ok.all():
        if throw:
            raise RuntimeError(
                f"pulse gates: step doubling reached max_steps={max_steps} without meeting atol + rtol = "
                f"{atol + rtol:.3g} ({int((~ok).sum())} of {table.shape[0]} solve(s)); raise max_steps or loosen the "
                "tolerances")
        U[~ok] = np.nan
    return U, steps


def solve_with_jacobian(table: np.ndarray, envelope: str, mode: str, omega_c: float, omega_q: float,
                        on_device: bool = False):
    """Every solve of ``table`` ``[n, 8]`` with its sensitivities -> ``(U [n, 2, 2], J [n, 5, 2, 2], steps)`` on the
    host, complex128; ``J[:, k]`` is the derivative of ``U`` by ``p0, p1, p2, w, T`` (``qmle_pulse_unitaries_jac``: the
    exact derivative of the grid's result, conventions in ``include/qmle_sv.h``).  Under ``magnus2`` / ``magnus4`` the
    grid has ``magnus_steps`` steps; under an adaptive solver name the step doubling of :func:`_launch_all` chooses
    the grid by ``U`` and ONE sensitivity launch follows on the accepted grid.  The Jacobian has no error control of
    its own: it is exact for the grid that ``U`` was accepted on, not bounded against the continuous problem.
    ``on_device=True`` returns ``(result [n, 6, 4] complex128 on the device, steps)`` instead -- slot 0 ``U``, slots
    1..5 ``J``, the layout ``qmle_compose_circuits`` reads -- without a copy to the host; the rejected solves of the
    adaptive path are masked there."""
    atol, rtol, max_steps, throw, solver, magnus_steps = Evolution._options({})
    table = np.ascontiguousarray(table, dtype=np.float64)
    n = table.shape[0]
    if solver in ("magnus2", "magnus4"):
        order, steps = (2 if solver == "magnus2" else 4), magnus_steps
    else:
        order = 4
        accepted, steps = _launch_all(table, envelope, mode, omega_c, omega_q)
        if steps < 1:  # (max_steps below the first grid and throw off: nothing was accepted)
            if on_device:
                torch = N.require_gpu()
                return torch.full((n, 6, 4), float("nan"), dtype=torch.complex128, device=N.current_device()), steps
            nan = np.full((n, 6, 2, 2), np.nan + 0j)
            return nan[:, 0], nan[:, 1:], steps
    out = N.pulse_unitaries_jac(table, envelope, mode, omega_c, omega_q, order, steps)
    rejected = None
    if solver not in ("magnus2", "magnus4"):
        rejected = np.isnan(accepted).any(axis=(1, 2))  # (solves that the doubling rejected, throw off)
    if on_device:
        if rejected is not None and rejected.any():
            out[N.require_gpu().from_numpy(rejected).to(out.device)] = float("nan")
        return out.reshape(n, 6, 4), steps
    out = out.cpu().numpy()
    if rejected is not None:
        out[rejected] = np.nan
    return out[:, 0].copy(), out[:, 1:].copy(), steps


def resolve(tape: Sequence[Operation]) -> int:
    """Solve every unresolved :class:`PulseRotation` of ``tape`` -- all of them in one launch per grid (one launch
    group per distinct envelope / mode / frequencies, normally one).  Returns the number of solves."""
    pending = [o for o in tape if isinstance(o, PulseRotation) and o._matrix is None]
    if not pending:
        return 0
    groups: Dict[tuple, list] = {}
    for o in pending:
        if not any(o is seen for seen in groups.setdefault(o.group(), [])):
            groups[o.group()].append(o)
    total = 0
    for (envelope, mode, omega_c, omega_q), ops in groups.items():
        blocks, where, seen, n = [], [], {}, 0
        for o in ops:
            t = o.solves()
            if o.batched_request:
                where.append((n, n + t.shape[0]))
            else:  # identical unbatched requests are solved once
                key = t.tobytes()
                if key in seen:
                    where.append(seen[key])
                    continue
                where.append((n, None))
                seen[key] = where[-1]
            blocks.append(t)
            n += t.shape[0]
        U, steps = _launch_all(np.concatenate(blocks), envelope, mode, omega_c, omega_q)
        for o, (lo, hi) in zip(ops, where):
            o._matrix = U[lo].copy() if hi is None else U[lo:hi].copy()
            o.evolve_steps = steps
        total += n
    return total


def resolve_for_gradient(tape: Sequence[Operation]) -> int:
    """The gradient-time :func:`resolve`: every :class:`PulseRotation` of ``tape`` that wants a matrix cotangent and
    has no Jacobian yet is solved WITH its sensitivities -- all of them in one :func:`solve_with_jacobian` call per
    launch group (under an adaptive solver name: the step doubling, then one sensitivity launch on the accepted
    grid) -- and keeps ``U`` ``[rows, 2, 2]`` and ``J`` ``[rows, 5, 2, 2]``.  A request whose rows are all the same
    (a leaf shared by the whole batch) is solved once.  Requests without leaf dependence are left to
    :func:`resolve`.  Returns the number of solves."""
    pending = []
    for o in tape:
        if isinstance(o, PulseRotation) and o.wants_matrix_cotangent and o._jacobian is None \
                and not any(o is seen for seen in pending):
            pending.append(o)
    groups: Dict[tuple, list] = {}
    for o in pending:
        groups.setdefault(o.group(), []).append(o)
    total = 0
    for (envelope, mode, omega_c, omega_q), ops in groups.items():
        blocks, where, n = [], [], 0
        for o in ops:
            t = o.solves()
            rows = t.shape[0]
            if rows > 1 and not (t != t[:1]).any():
                t = t[:1]
            where.append((n, n + t.shape[0], rows))
            blocks.append(t)
            n += t.shape[0]
        U, J, steps = solve_with_jacobian(np.concatenate(blocks), envelope, mode, omega_c, omega_q)
        for o, (lo, hi, rows) in zip(ops, where):
            rep_ = rows if hi - lo == 1 and rows > 1 else 1
            o._matrix = np.repeat(U[lo:hi], rep_, axis=0)
            o._jacobian = np.repeat(J[lo:hi], rep_, axis=0)
            o.evolve_steps = steps
        total += n
    return total


# ---- the gates --------------------------------------------------------------------------------------------------------
class PulseGates:
    """Pulse-level implementations of the gate vocabulary (``pulses.py:993-1662``, after
    https://doi.org/10.5445/IR/1000184129): RX, RY, RZ and CZ are leaves, everything else walks its decomposition
    in :class:`PulseInformation`."""

    omega_q = 10 * np.pi
    omega_c = 10 * np.pi

    X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
    Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
    Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)
    Id = np.eye(2, dtype=np.complex128)
    _H_CZ = (np.pi / 4) * (np.kron(Id, Id) - np.kron(Z, Id) - np.kron(Id, Z) + np.kron(Z, Z))
    _H_corr = np.pi / 2 * np.eye(2, dtype=np.complex128)

    _active_envelope: str = "drag"
    _active_rwa: bool = True
    _active_frame: str = "drive"

    # -- leaves
    @staticmethod
    def _drive(axis: str, w, wires, pulse_params, noise_params, random_key) -> None:
        pulse_params = PulseInformation.gate_by_name("R" + axis).split_params(pulse_params)
        w, random_key = UnitaryGates.GateError(w, noise_params, random_key)
        PulseRotation(axis, w, pulse_params, wires=wires)
        UnitaryGates.Noise(wires, noise_params)

    @staticmethod
    def RX(w, wires, pulse_params=None, noise_params=None, random_key=None) -> None:
        """X rotation by a shaped pulse; ``pulse_params = [envelope parameters..., T]`` (default: the optimised
        ones of the active envelope)."""
        PulseGates._drive("X", w, wires, pulse_params, noise_params, random_key)

    @staticmethod
    def RY(w, wires, pulse_params=None, noise_params=None, random_key=None) -> None:
        """Y rotation by a shaped pulse (carrier phase +pi/2)."""
        PulseGates._drive("Y", w, wires, pulse_params, noise_params, random_key)

    @staticmethod
    def RZ(w, wires, pulse_params=None, noise_params=None, random_key=None) -> None:
        """Virtual Z rotation ``exp(-i p0 w Z)``: no pulse, recorded as ``RZ(2 p0 w)``."""
        pulse_params = PulseInformation.RZ.split_params(pulse_params)
        w, random_key = UnitaryGates.GateError(w, noise_params, random_key)
        op.RZ(2.0 * _first(pulse_params) * w, wires=wires)
        UnitaryGates.Noise(wires, noise_params)

    @staticmethod
    def CZ(wires, pulse_params=None, noise_params=None, random_key=None) -> None:
        """ZZ coupling for unit time: ``exp(-i pi^2 p |11><11|)``, recorded as ``ControlledPhaseShift(-pi^2 p)``."""
        if pulse_params is None:
            pulse_params = PulseInformation.CZ.params
        op.ControlledPhaseShift(-(np.pi ** 2) * _first(pulse_params), wires=wires)
        UnitaryGates.Noise(wires, noise_params)

    # -- composites
    @staticmethod
    def _resolve_wires(wire_fn: str, wires):
        wl = [wires] if isinstance(wires, (int, np.integer)) else list(wires)
        if wire_fn == "all":
            return wires if len(wl) > 1 else wl[0]
        if wire_fn == "target":
            return wl[-1]
        if wire_fn == "control":
            return wl[0]
        raise ValueError(f"Unknown wire_fn: {wire_fn!r}")

    _WITH_ANGLE = ("CRX", "CRY", "CRZ", "CPhase", "RXX", "RYY", "RZZ", "RZX")

    @staticmethod
    def _execute_composite(gate_name: str, w, wires, pulse_params=None) -> None:
        """Walk the decomposition of ``gate_name``: every step gets its share of ``pulse_params``."""
        pp_obj = PulseInformation.gate_by_name(gate_name)
        parts = pp_obj.split_params(pulse_params)
        for step, child_params in zip(pp_obj.decomposition, parts):
            child_wires = PulseGates._resolve_wires(step.wire_fn, wires)
            child_w = step.angle_fn(w) if step.angle_fn is not None else w
            child = getattr(PulseGates, step.gate.name)
            if step.gate.name in ("RX", "RY", "RZ") or step.gate.name in PulseGates._WITH_ANGLE:
                child(child_w, wires=child_wires, pulse_params=child_params)
            elif step.gate.name == "Rot":
                child(*child_w, wires=child_wires, pulse_params=child_params)
            else:  # CZ, H, CX, CY
                child(wires=child_wires, pulse_params=child_params)

    @staticmethod
    def H(wires, pulse_params=None, noise_params=None, random_key=None) -> None:
        """RZ(pi) RY(pi/2) and the phase ``exp(+i pi/2)`` that makes it the Hadamard matrix."""
        PulseGates._execute_composite("H", 0.0, wires, pulse_params)
        Operation(wires=wires, matrix=1j * np.eye(2, dtype=np.complex128), name="H_phase")
        UnitaryGates.Noise(wires, noise_params)

    @staticmethod
    def Rot(phi, theta, omega, wires, pulse_params=None, noise_params=None, random_key=None) -> None:
        if noise_params is not None and "GateError" in noise_params:
            phi, random_key = UnitaryGates.GateError(phi, noise_params, random_key)
            theta, random_key = UnitaryGates.GateError(theta, noise_params, random_key)
            omega, random_key = UnitaryGates.GateError(omega, noise_params, random_key)
        PulseGates._execute_composite("Rot", [phi, theta, omega], wires, pulse_params)
        UnitaryGates.Noise(wires, noise_params)

    @staticmethod
    def PauliRot(pauli, theta, wires, pulse_params=None, noise_params=None, random_key=None) -> None:
        raise NotImplementedError("PauliRot gate is not implemented as PulseGate")


def _fixed_composite(name: str):
    def gate(wires, pulse_params=None, noise_params=None, random_key=None) -> None:
        PulseGates._execute_composite(name, 0.0, wires, pulse_params)
        UnitaryGates.Noise(wires, noise_params)

    gate.__name__ = name
    gate.__doc__ = f"``{name}`` through its pulse decomposition (``PulseInformation.{name}``)."
    return staticmethod(gate)


def _angle_composite(name: str, gate_error: bool):
    def gate(w, wires, pulse_params=None, noise_params=None, random_key=None) -> None:
        if gate_error:
            w, random_key = UnitaryGates.GateError(w, noise_params, random_key)
        PulseGates._execute_composite(name, w, wires, pulse_params)
        UnitaryGates.Noise(wires, noise_params)

    gate.__name__ = name
    gate.__doc__ = f"``{name}(w)`` through its pulse decomposition (``PulseInformation.{name}``)."
    return staticmethod(gate)


for _name in ("CX", "CY"):
    setattr(PulseGates, _name, _fixed_composite(_name))
for _name in PulseGates._WITH_ANGLE:  # (the reference applies no GateError to CRX)
    setattr(PulseGates, _name, _angle_composite(_name, gate_error=_name != "CRX"))


class PulseParamManager:
    """Cursor over one layer's pulse parameters: every gate takes the next ``n``."""

    def __init__(self, pulse_params) -> None:
        self.pulse_params = pulse_params
        self.idx = 0

    def get(self, n: int):
        if self.idx + n > len(self.pulse_params):
            raise ValueError("Not enough pulse parameters left for this gate")
        params = self.pulse_params[self.idx:self.idx + n]
        self.idx += n
        return params


# after PulseGates exists: leaf defaults, composite trees, mirrored flags and coefficient functions agree
PulseInformation.reset_defaults()
