"""``Gates.<NAME>(...)`` router.

API mirror of ``qml_essentials/gates.py:24-225``: attribute access on the *class*
returns a handler whose ``__name__`` is the gate name (``Block`` and
``is_rotational/is_entangling`` rely on it), unknown keyword arguments are
dropped, ``gate_mode`` selects the backend: ``"unitary"`` -> :class:`unitary.UnitaryGates`,
``"pulse"`` -> :class:`pulses.PulseGates` (re-exported here with the rest of :mod:`pulses`, as in the reference).

Pulse mode is served whenever pulse parameters are in force -- a ``pulse_params`` keyword that is not ``None``, or an
active pulse manager (:meth:`Gates.pulse_manager_context`, which ``Circuit._build`` opens per layer and which scales
the gate's optimised parameters by the layer's).  Deviation from the reference: the bare call
``Gates.RX(w, wires=0, gate_mode="pulse")`` with neither is refused (``NotImplementedError`` naming
``PulseGates.RX``, the direct entrance that takes the optimised defaults).
"""
from __future__ import annotations

import numbers
from contextlib import contextmanager
from typing import Callable, List, Union

import numpy as np

from . import operations as _op
from .batching import Batched
from .pulses import (DecompositionStep, PulseEnvelope, PulseGates, PulseInformation,  # noqa: F401  (re-exports)
                     PulseParamManager, PulseParams)
from .unitary import UnitaryGates

_FORWARDED = ("w", "wires", "phi", "theta", "omega", "noise_params", "random_key")
_ROTATIONAL = {"RX", "RY", "RZ", "Rot", "CRX", "CRY", "CRZ", "GolombEncoding", "CPhase"}
_ENTANGLING = {"CX", "CY", "CZ", "CRX", "CRY", "CRZ", "CPhase"}


class _GatesMeta(type):
    def __getattr__(cls, gate_name: str) -> Callable:
        if gate_name.startswith("__"):
            raise AttributeError(gate_name)

        def handler(*args, **kwargs):
            return cls._dispatch(gate_name, *args, **kwargs)

        handler.__name__ = gate_name
        return handler


class Gates(metaclass=_GatesMeta):
    """Dynamic accessor: ``Gates.RX(w, wires=0)`` records an RX on the active tape."""

    def __getattr__(self, gate_name: str) -> Callable:
        def handler(**kwargs):
            return type(self)._dispatch(gate_name, **kwargs)

        handler.__name__ = gate_name
        return handler

    @classmethod
    def _dispatch(cls, gate_name: str, *args, **kwargs):
        if gate_name == "Barrier":
            wires = kwargs.get("wires", args[0] if args else 0)
            return _op.Barrier(wires)
        mode = kwargs.pop("gate_mode", "unitary")
        if mode == "pulse":
            return cls._dispatch_pulse(gate_name, *args, **kwargs)
        if mode != "unitary":
            raise ValueError(f"Unknown gate mode: {mode}. Use 'unitary' or 'pulse'.")
        kwargs = {k: v for k, v in kwargs.items() if k in _FORWARDED}
        gate = getattr(UnitaryGates, gate_name, None)
        if gate is None:
            raise AttributeError(f"'UnitaryGates' object has no attribute '{gate_name}'")
        return gate(*args, **kwargs)

    _inner_getattr = _dispatch  # (the reference's name)
    _pulse_mgr = None

    @classmethod
    def _dispatch_pulse(cls, gate_name: str, *args, **kwargs):
        """``gate_mode="pulse"`` (``gates.py:105-161``): type and length checks on ``pulse_params``, then either the
        caller's parameters or -- under a pulse manager -- the gate's optimised ones scaled by the manager's next
        slice."""
        kwargs = {k: v for k, v in kwargs.items() if k in _FORWARDED + ("pulse_params",)}
        pulse_params = kwargs.get("pulse_params")
        managed = isinstance(cls._pulse_mgr, PulseParamManager)
        if pulse_params is None and not managed:
            raise NotImplementedError(
                f"Gates.{gate_name}(..., gate_mode='pulse') without pulse_params and outside a pulse manager is not "
                f"served by the router: call PulseGates.{gate_name} (it takes the optimised default parameters), or "
                "pass pulse_params")
        flat = None
        if pulse_params is not None:
            if isinstance(pulse_params, PulseParams):
                kwargs["pulse_params"] = pulse_params = pulse_params.params
            if isinstance(pulse_params, (list, tuple)):
                flat = list(pulse_params)
            elif isinstance(pulse_params, Batched):
                flat = [0.0] * int(np.prod(pulse_params.shape, dtype=np.int64))  # (numeric by construction)
            elif isinstance(pulse_params, np.ndarray):
                flat = pulse_params.reshape(-1).tolist()
            else:
                raise TypeError(f"Unsupported pulse_params type: {type(pulse_params)}")
            if not all(isinstance(x, numbers.Real) for x in flat):
                raise TypeError("All elements in pulse_params must be int or float, "
                                f"got {pulse_params}, type {type(pulse_params)}. ")
        info = PulseInformation.gate_by_name(gate_name)
        if flat is not None and not managed and info is not None and len(flat) != info.size:
            raise ValueError(f"Gate '{gate_name}' expects {info.size} pulse parameters, got {len(flat)}")
        if managed and info is not None:
            scalers = cls._pulse_mgr.get(info.size)
            kwargs["pulse_params"] = info.params * scalers
        gate = getattr(PulseGates, gate_name, None)
        if gate is None:
            raise AttributeError(f"'PulseGates' object has no attribute '{gate_name}'")
        return gate(*args, **kwargs)

    @classmethod
    @contextmanager
    def pulse_manager_context(cls, pulse_params):
        """Hand out ``pulse_params`` (one layer's scalers) gate by gate while the block records."""
        cls._pulse_mgr = PulseParamManager(pulse_params)
        try:
            yield
        finally:
            cls._pulse_mgr = None

    @classmethod
    def parse_gates(cls, gates: Union[str, Callable, List[Union[str, Callable]], None],
                    set_of_gates=None) -> List[Callable]:
        """Names / callables / lists thereof -> list of gate callables (``gates.py:173-207``)."""
        pool = set_of_gates or cls
        if gates is None:
            return [lambda *a, **k: None]
        if isinstance(gates, str):
            return [getattr(pool, gates)]
        if isinstance(gates, list):
            out = []
            for g in gates:
                if isinstance(g, str):
                    out.append(getattr(pool, g))
                elif callable(g):
                    out.append(g)
                else:
                    raise ValueError(f"Operation {g} is not a valid gate or callable. Got {type(g)}")
            return out
        if callable(gates):
            return [gates]
        raise ValueError(f"Operation {gates} is not a valid gate or callable or list of both.")

    @classmethod
    def is_rotational(cls, gate) -> bool:
        return gate.__name__ in _ROTATIONAL

    @classmethod
    def is_entangling(cls, gate) -> bool:
        return gate.__name__ in _ENTANGLING
