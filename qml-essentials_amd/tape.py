"""Per-thread recording tapes.

Behavioural mirror of ``qml_essentials/tape.py:10-55,92-138``: instantiating an
``Operation`` while a ``recording()`` block is active appends it to the innermost
tape of the current thread.  Pulse-level gates (:mod:`pulses`) record on this same
tape; the pulse-EVENT tapes that feed the reference's pulse-schedule drawing
(``tape.py:58-89``) are out of scope.
"""
from __future__ import annotations

import copy
import threading
from contextlib import contextmanager
from typing import Callable, Iterator, List, Optional

_tls = threading.local()


def _stack() -> list:
    st = getattr(_tls, "tapes", None)
    if st is None:
        st = _tls.tapes = []
    return st


def active_tape() -> Optional[list]:
    """Innermost tape being recorded on this thread, or ``None``."""
    st = _stack()
    return st[-1] if st else None


@contextmanager
def recording() -> Iterator[list]:
    """Open a fresh tape; nested blocks get independent tapes."""
    st = _stack()
    tape: list = []
    st.append(tape)
    try:
        yield tape
    finally:
        # pop *our* tape even if an inner block leaked one
        while st and st[-1] is not tape:
            st.pop()
        if st:
            st.pop()


def shift_and_append(tape_ops: List, offset: int) -> None:
    """Append wire-shifted shallow copies of ``tape_ops`` to the active tape
    (multi-register circuits, ``tape.py:92-114``)."""
    target = active_tape()
    if target is None:
        return
    for op in tape_ops:
        clone = copy.copy(op)
        clone._wires = [w + offset for w in op.wires]
        target.append(clone)


def copy_to_tape(fn: Callable[[], None], offset: int) -> None:
    """Record ``fn`` on a side tape and replay it shifted by ``offset`` wires
    (``tape.py:117-138``)."""
    with recording() as side:
        fn()
    shift_and_append(side, offset)


@contextmanager
def batch_context(batch: int) -> Iterator[None]:
    """Batch size of the recording in progress (per thread).  Gates that draw per-sample
    random numbers while being recorded (``UnitaryGates.GateError``) read it, because a
    batch-constant angle carries no batch axis of its own."""
    prev = getattr(_tls, "batch", 1)
    _tls.batch = int(batch)
    try:
        yield
    finally:
        _tls.batch = prev


def current_batch() -> int:
    return getattr(_tls, "batch", 1)


# ---- call capture (math.quantum_fisher_information / fubini_study_metric) -------------------------
# While a capture is open on this thread, every top-level Model.__call__ / Script.execute appends one
# record (a dict with "kind", the callee, its arguments and its result); calls made from inside another
# recorded call are not recorded again.


def _captures() -> list:
    st = getattr(_tls, "captures", None)
    if st is None:
        st = _tls.captures = []
    return st


@contextmanager
def capturing() -> Iterator[list]:
    """Collect the records of the calls made inside the block (innermost capture only)."""
    st = _captures()
    rec: list = []
    st.append(rec)
    depth, _tls.capture_depth = getattr(_tls, "capture_depth", 0), 0
    try:
        yield rec
    finally:
        _tls.capture_depth = depth
        while st and st[-1] is not rec:
            st.pop()
        if st:
            st.pop()


@contextmanager
def captured_call(make_record: Callable[[], dict]) -> Iterator[dict]:
    """Around one Model.__call__ / Script.execute: yields a dict the caller puts ``result`` into; the
    record is appended to the open capture when this call is not nested in another recorded one."""
    st = _captures()
    if not st:
        yield {}
        return
    depth = getattr(_tls, "capture_depth", 0)
    _tls.capture_depth = depth + 1
    out: dict = {}
    try:
        yield out
    finally:
        _tls.capture_depth = depth
    if depth == 0 and "result" in out:
        rec = make_record()
        rec["result"] = out["result"]
        st[-1].append(rec)
