"""Adjoint differentiation: the gradient of a weighted sum of expectation values -- Z / Z-parities
(``qmle_adjoint_gradient``) or any observables that are sums of Pauli words, X / Y / Hermitian ones included
(``qmle_adjoint_gradient_pauli``) -- with respect to EVERY gate angle in one backward sweep.

What ``jax.grad`` through ``Script.execute`` gives the reference (``tests/test_jaqsi.py:131-141``,
``tests/test_model.py:1097-1145``, ``docs/training.md``).  Cost: one forward simulation, then
per gate one inverse-gate pass over [psi; lambda] and, per differentiable angle, one overlap
``Im <lambda| G |psi>`` -- O(gates + angles) passes instead of the 2 x angles full circuits of
the parameter-shift rule.

One-wire MATRIX gates (constant ``MAT1``, per-sample ``MAT1_ROW``) have no generator; for them the same sweep returns the
matrix cotangent ``G[a][c] = sum_rest conj(lambda[a, rest]) phi[c, rest]`` on the state in front of the gate
(:func:`adjoint_slot_and_matrix_gradient`), from which a caller that knows ``dU/dtheta`` -- the pulse front end: the
solver's Jacobian -- forms ``dC/dtheta = 2 Re sum_ac G[a][c] dU[a][c]/dtheta``.  :func:`adjoint_slot_and_matrices_gradient` does the same for
matrix gates on two wires (``MAT2`` / ``MAT2_ROW``: 4x4 cotangents) beside the one-wire ones.

Explicit matrices on THREE AND FOUR wires are no part of any plan.  A tape that holds them is swept segment by
segment (:func:`plan_segments`, :func:`segmented_gradient`): the forward run of ``simulation.segmented_forward``
and the seed leave psi and lambda resident, ``qmle_adjoint_segment`` sweeps the gates between two wide gates on
them, ``qmle_wide_moment`` reports a wide gate's 8x8 / 16x16 cotangent and ``qmle_apply_matrix`` undoes the gate
on both states.

NOISY tapes (Kraus channels on one and two wires) have a sweep of their own over vec(rho): a channel has no usable
inverse, so the forward states are kept and only the observable is pulled back (:func:`plan_density`,
:func:`density_gradient`, ``qmle_adjoint_density``): one step per wanted angle -- the gate pair and the channels behind it
on its wires -- at five state-sized transfers, the K cotangents of a Jacobian sharing one set of forward states.

This module only prepares the REVERSED, DAGGERED tape and the generator table; the sweep itself
runs in the engine.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from .operations import is_wide_matrix_gate
from .simulation import LoweredTape, _Lowered, get_plan, split_at_wide_gates

# rotation gates exp(-i theta/2 P): generator Pauli word per wire, (control?, word)
_ROT = {"RX": (False, "X"), "RY": (False, "Y"), "RZ": (False, "Z"),
        "CRX": (True, "X"), "CRY": (True, "Y"), "CRZ": (True, "Z"),
        "RXX": (False, "XX"), "RYY": (False, "YY"), "RZZ": (False, "ZZ"), "RZX": (False, "ZX")}
_SELF_INVERSE = {"Id", "PauliX", "PauliY", "PauliZ", "H", "CX", "CY", "CZ", "SWAP", "CCX", "CSWAP"}


class AdjointUnsupported(NotImplementedError):
    pass


def _dagger_blob(blob: np.ndarray, dim: int) -> np.ndarray:
    keep = np.float64 if np.asarray(blob).dtype == np.float64 else np.float32  # (x64 mode: full precision)
    m = np.asarray(blob, dtype=np.float64).reshape(dim, dim, 2)
    m = (m[..., 0] + 1j * m[..., 1]).conj().T
    return np.stack([m.real, m.imag], axis=-1).astype(keep).reshape(-1)


def _term(out_slot=-1, x=0, z=0, proj=0, n_y=0, coef=0.0, marks_off=-1):
    return (int(out_slot), int(x), int(z), int(proj), int(n_y), float(coef), int(marks_off))


_BLOB_LEN = {"MAT1": 8, "MAT2": 32, "MAT4": 512}


def _op_blobs(low: LoweredTape, x64: bool = False) -> List[Optional[np.ndarray]]:
    out = []
    consts = low.consts64 if x64 else low.consts
    for name, _w, _s, off in low.ops:
        if off < 0:
            out.append(None)
        else:
            size = _BLOB_LEN.get(name, 1 << low.n_qubits)  # DIAG_ALL: one mark per amplitude
            out.append(consts[off:off + size])
    return out


def build_reverse(low: LoweredTape, blobs: List[Optional[np.ndarray]], want: Sequence[bool],
                  want_mat: Optional[Sequence[bool]] = None, two_wire: bool = False):
    """From the forward lowered tape: the reversed, daggered primitive tape (as ``_Lowered`` ops),
    its per-slot values (negated forward columns) and one generator term per reverse op.

    ``blobs[k]``: constant blob of forward op k (or None); ``want[s]``: forward slot s needs a
    derivative.  Rot(phi, theta, omega) = RZ(omega) RY(theta) RZ(phi) is split into its three
    rotations so that every primitive has at most one angle.

    -> ``(rev_ops, terms, rev_src)``: reverse slot j holds MINUS forward column ``rev_src[j]``.  That rule cannot
    invert a per-sample matrix, so in this form a ``MAT1_ROW`` is refused (``CompiledCall`` keeps this form).

    ``want_mat`` (one flag per forward op, True only on one-wire matrix gates ``MAT1`` / ``MAT1_ROW``) asks for the
    form that serves matrix gates -> ``(rev_ops, terms, rev_src, rev_sign, mat_out)``: reverse slot j holds
    ``rev_sign[j] *`` forward column ``rev_src[j]``.  The reverse of a ``MAT1_ROW`` is a ``MAT1_ROW`` on the daggered
    columns -- entry (r, c, re) is the forward entry (c, r, re), sign +1; entry (r, c, im) the forward entry
    (c, r, im), sign -1 -- and every angle keeps sign -1.  ``mat_out[r]``: per REVERSE op the index of the matrix
    cotangent it reports (flagged forward ops numbered in tape order), or -1.  ``MAT2_ROW`` stays refused.

    ``two_wire`` (with ``want_mat``): ``MAT2_ROW`` is accepted too -- its reverse is a ``MAT2_ROW`` on the daggered
    columns, the same rule on 32 columns -- and flags may sit on ``MAT2`` / ``MAT2_ROW``
    -> ``(rev_ops, terms, rev_src, rev_sign, mat_out, mat_dim)``, ``mat_dim[k]`` in (2, 4) per flagged op."""
    with_mat = want_mat is not None
    if two_wire and not with_mat:
        raise ValueError("two_wire goes with want_mat")
    row_dim = {"MAT1_ROW": 2, "MAT2_ROW": 4} if two_wire else {"MAT1_ROW": 2}
    flaggable = ("MAT1", "MAT1_ROW", "MAT2", "MAT2_ROW") if two_wire else ("MAT1", "MAT1_ROW")
    mat_dim = []
    if with_mat and len(want_mat) != len(low.ops):
        raise ValueError("want_mat holds one flag per forward op")
    prims = []  # forward order: (name, wires, fwd_slot | None (MAT1_ROW: its 8 slots), blob, matrix index | -1)
    n_mat = 0
    for k, ((name, wires, slots, _off), blob) in enumerate(zip(low.ops, blobs)):
        k_mat = -1
        if with_mat and want_mat[k]:
            if name not in flaggable:
                raise AdjointUnsupported(f"no matrix cotangent for {name}: the sweep reports them for one-wire matrix "
                                         "gates only (two-wire matrices are not served)" if not two_wire else
                                         f"no matrix cotangent for {name}: the sweep reports them for one-wire matrix "
                                         "and two-wire matrix gates only")
            k_mat = n_mat
            n_mat += 1
            mat_dim.append(4 if name.startswith("MAT2") else 2)
        if name == "MAT2_ROW" and not two_wire:
            raise AdjointUnsupported("no adjoint rule for MAT2_ROW: the sweep inverts per-sample matrices on one wire "
                                     "only; two-wire matrices (evolved two-wire unitaries) are not served")
        if name in row_dim:
            if not with_mat:
                raise AdjointUnsupported("no adjoint rule for MAT1_ROW in the angle-only form: a per-sample matrix is "
                                         "not inverted by negating its columns (build_reverse(..., want_mat=...) "
                                         "returns the sign vector that does it)")
            prims.append((name, wires, list(slots), None, k_mat))
            continue
        if name == "Rot":
            prims += [("RZ", wires, slots[0], None, -1), ("RY", wires, slots[1], None, -1),
                      ("RZ", wires, slots[2], None, -1)]
        elif len(slots) > 1:
            raise AdjointUnsupported(f"{name}: more than one angle per gate")
        else:
            prims.append((name, wires, slots[0] if slots else None, blob, k_mat))
    rev_ops, rev_src, rev_sign, terms, mat_out = [], [], [], [], []
    for name, wires, fslot, blob, k_mat in reversed(prims):
        params, out_blob, term = [], None, _term()
        bit = lambda ws: sum(1 << int(w) for w in ws)  # noqa: E731
        mat_out.append(k_mat)
        if name in row_dim:  # U^+: reverse column (r, c, part) <- forward column (c, r, part), imaginary parts negated
            dim = row_dim[name]
            for r in range(dim):
                for c in range(dim):
                    for part, sign in ((0, 1.0), (1, -1.0)):
                        src = fslot[(c * dim + r) * 2 + part]
                        params.append(sign * np.asarray(low.values[src], dtype=np.float64))
                        rev_src.append(src)
                        rev_sign.append(sign)
            rev_ops.append(_Lowered((name, list(wires), params, None)))
            terms.append(term)
            continue
        if fslot is not None:
            params = [-np.asarray(low.values[fslot], dtype=np.float64)]
            rev_src.append(fslot)
            rev_sign.append(-1.0)
        d = want[fslot] if fslot is not None else False
        if name in _ROT:
            ctrl, word = _ROT[name]
            tw = wires[1:] if ctrl else wires
            x = bit(w for w, p in zip(tw, word) if p in "XY")
            z = bit(w for w, p in zip(tw, word) if p in "ZY")
            if d:
                term = _term(fslot, x, z, bit(wires[:1]) if ctrl else 0, word.count("Y"), 1.0)
        elif name in ("CPhase", "ControlledPhaseShift"):
            if d:  # dU = i |11><11| U
                term = _term(fslot, 0, 0, bit(wires), 0, -2.0)
        elif name == "DIAG_ALL":
            out_blob = np.asarray(blob)
            if d:  # U = exp(-i M x): dU = -i M U
                term = _term(fslot, coef=2.0, marks_off=0)  # offset patched below
        elif name in _SELF_INVERSE:
            pass
        elif name == "S":
            name, out_blob = "MAT1", np.array([1, 0, 0, 0, 0, 0, 0, -1], dtype=np.float32)
        elif name in ("MAT1", "MAT2", "MAT4"):
            out_blob = _dagger_blob(blob, 2 ** len(wires))
        else:
            raise AdjointUnsupported(f"no adjoint rule for {name}")
        rev_ops.append(_Lowered((name, list(wires), params, out_blob)))
        terms.append(term)
    if two_wire:
        return rev_ops, terms, rev_src, rev_sign, mat_out, mat_dim
    if with_mat:
        return rev_ops, terms, rev_src, rev_sign, mat_out
    return rev_ops, terms, rev_src


def patch_marks(rev: LoweredTape, terms):
    """Golomb terms point at their marks inside the reverse tape's const blob."""
    return [t[:6] + (off,) if (name == "DIAG_ALL" and t[0] >= 0) else t
            for (name, _w, _s, off), t in zip(rev.ops, terms)]


# one streaming pass per gate (always possible) ...
REV_FLAGS = N.PLAN_NO_FUSION | N.PLAN_FORCE_GLOBAL | N.PLAN_NO_ABSORB
# ... or fused tile passes over [psi; lambda]: every gate stays its own operator (one generator
# per gate), tiles of 2^12 amplitudes so that both states fit in one workgroup's LDS
REV_FLAGS_FUSED = (N.PLAN_NO_MERGE | N.PLAN_FORCE_GLOBAL | N.PLAN_NO_ABSORB
                   | N.plan_flags(tile_bits=12, low_bits=4))


def run_sweep(fwd_plan, rev: LoweredTape, a_f, a_r, w, obs_groups, terms, n_grad_slots, obs_terms=None,
              mat_out=None, n_mat=0, cot_stride=0, two_wire=False):
    """The backward sweep with fused tile passes where the engine supports the tape (1-qubit and
    controlled 1-qubit gates), else with one streaming pass per gate.  float64 tables: the
    complex128 sweep (one streaming launch per operator, like the complex128 forward engine).
    The observables: Z-parity wire groups ``obs_groups``, or (``obs_groups`` None) the Pauli term list
    ``obs_terms`` -- the same routes, another seed.  ``mat_out`` (per reverse op the index of the matrix cotangent
    it reports, or -1; ``n_mat`` of them): -> ``(gradient, cotangents)`` from the same sweep; the fused tile passes
    refuse such a request, so above 13 qubits it takes the streaming route.  ``cot_stride`` > 0: ``mat_out`` holds
    block OFFSETS in a row of that many scalars instead (one- and two-wire matrices, ``N.adjoint_cotangent_at``)
    -> ``(gradient, rows [B, cot_stride])``."""
    if mat_out is None:
        call = lambda flags: N.adjoint_gradient(fwd_plan, get_plan(rev, flags), a_f, a_r, w, obs_groups, terms,  # noqa: E731
                                                n_grad_slots, obs_terms=obs_terms)
    elif cot_stride:
        call = lambda flags: N.adjoint_cotangent_at(fwd_plan, get_plan(rev, flags), a_f, a_r, w, obs_groups, terms,  # noqa: E731
                                                    n_grad_slots, mat_out, cot_stride, two_wire, obs_terms=obs_terms)
    else:
        call = lambda flags: N.adjoint_cotangent(fwd_plan, get_plan(rev, flags), a_f, a_r, w, obs_groups, terms,  # noqa: E731
                                                 n_grad_slots, mat_out, n_mat, obs_terms=obs_terms)
    if w.dtype == N.require_gpu().float64:
        return call(REV_FLAGS)
    try:
        return call(REV_FLAGS_FUSED)
    except N.Unsupported:
        return call(REV_FLAGS)


class RevTables(NamedTuple):
    """What turns the forward angle table into the reverse one, and which reverse ops report a matrix cotangent."""
    perm: object            # int64 CUDA tensor: reverse slot j reads forward column perm[j] ...
    sign: object            # ... times sign[j] (float64 CUDA tensor): -1 for angles, +1 for real parts of matrices
    mat_out: tuple          # per reverse op: index of its matrix cotangent, or -1
    n_mat: int
    mat_dim: tuple = ()     # the two-wire form: 2 or 4 per flagged op, in tape order


_REV_CACHE: "OrderedDict[tuple, tuple]" = OrderedDict()


def _sweep(low: LoweredTape, n_qubits: int, batch: int, obs_groups, weights, want, want_mat, x64, obs_terms,
           two_wire=False):
    torch = N.require_gpu()
    ft, fn = (torch.float64, np.float64) if x64 else (torch.float32, np.float32)
    want_mat = tuple(bool(x) for x in want_mat) if want_mat is not None else (False,) * len(low.ops)
    key = ((low.key, tuple(bool(x) for x in want), bool(x64)) + ((want_mat,) if any(want_mat) else ())
           + (("two_wire",) if two_wire else ()))
    hit = _REV_CACHE.get(key)
    if hit is None:
        rev_ops, terms, rev_src, rev_sign, mat_out, *dims = build_reverse(low, _op_blobs(low, x64), want, want_mat,
                                                                          **({"two_wire": True} if two_wire else {}))
        rev = LoweredTape(rev_ops, n_qubits)
        hit = (rev, patch_marks(rev, terms),
               RevTables(torch.tensor(rev_src if rev_src else [0], dtype=torch.int64, device="cuda"),
                         torch.tensor(rev_sign if rev_sign else [-1.0], dtype=torch.float64, device="cuda"),
                         tuple(mat_out), sum(want_mat), tuple(dims[0]) if dims else ()))
        _REV_CACHE[key] = hit
        if len(_REV_CACHE) > 64:
            _REV_CACHE.popitem(last=False)
    else:
        _REV_CACHE.move_to_end(key)
    rev, fixed, tab = hit
    a_f = torch.from_numpy(low.angle_table(batch, dtype=np.float64) if x64 else low.angle_table(batch)).cuda()
    rep = int(np.shape(weights)[0]) // max(1, batch)
    if rep > 1:  # several cotangents per sample (a Jacobian: one row of weights per output) in ONE sweep
        a_f = a_f.repeat(rep, 1)
        batch = batch * rep
    if rev.n_slots:
        a_r = (a_f.index_select(1, tab.perm) * tab.sign.to(ft)).contiguous()
    else:
        a_r = torch.zeros((batch, 1), dtype=ft, device=a_f.device)
    w = torch.from_numpy(np.ascontiguousarray(weights, dtype=fn)).cuda()
    if two_wire and tab.n_mat:  # blocks of 8 and 32 scalars in one row, in tape order
        starts = np.concatenate([[0], np.cumsum([2 * d * d for d in tab.mat_dim])]).astype(int)
        g, rows = run_sweep(get_plan(low), rev, a_f, a_r, w, obs_groups, fixed, max(1, low.n_slots),
                            obs_terms=obs_terms, mat_out=[int(starts[k]) if k >= 0 else -1 for k in tab.mat_out],
                            cot_stride=int(starts[-1]), two_wire=4 in tab.mat_dim)
        rows = rows.cpu().numpy()
        mats = [rows[:, starts[k]:starts[k + 1]].reshape(-1, d, d, 2) for k, d in enumerate(tab.mat_dim)]
        return g.cpu().numpy()[:, : low.n_slots], [m[..., 0] + 1j * m[..., 1] for m in mats]
    if not tab.n_mat:
        return run_sweep(get_plan(low), rev, a_f, a_r, w, obs_groups, fixed, max(1, low.n_slots),
                         obs_terms=obs_terms).cpu().numpy()[:, : low.n_slots], None
    g, cot = run_sweep(get_plan(low), rev, a_f, a_r, w, obs_groups, fixed, max(1, low.n_slots), obs_terms=obs_terms,
                       mat_out=list(tab.mat_out), n_mat=tab.n_mat)
    return g.cpu().numpy()[:, : low.n_slots], cot.cpu().numpy()


def adjoint_slot_gradient(low: LoweredTape, n_qubits: int, batch: int, obs_groups,
                          weights: np.ndarray, want: Sequence[bool], x64: bool = False,
                          obs_terms=None) -> np.ndarray:
    """d/d(angle slot) of sum_k weights[b, k] <O_k> for every forward slot -> [B, n_slots]; the observables are
    the Z / Z-parity wire groups ``obs_groups`` or, with ``obs_groups`` None, the Pauli term list ``obs_terms``
    (columns of slots that are not wanted stay zero; ``weights`` of shape [K * B, n_obs] -- K cotangents per
    sample, sample-minor -- give [K * B, n_slots] from one sweep over K * B states).  The reversed tape depends only on the
    STRUCTURE of the forward tape (its angles are the forward columns, negated -- the real parts of a per-sample
    one-wire matrix, whose columns are its entries, are not), so it is built
    once per structure.  ``x64``: float64 angle table, complex128 states, float64 gradients."""
    return _sweep(low, n_qubits, batch, obs_groups, weights, want, None, x64, obs_terms)[0]


def adjoint_slot_and_matrix_gradient(low: LoweredTape, n_qubits: int, batch: int, obs_groups, weights: np.ndarray,
                                     want: Sequence[bool], want_mat: Sequence[bool], x64: bool = False,
                                     obs_terms=None) -> Tuple[np.ndarray, np.ndarray]:
    """:func:`adjoint_slot_gradient` that also returns the MATRIX COTANGENTS of the forward ops flagged in
    ``want_mat`` (one flag per op of ``low.ops``; one-wire matrix gates only, constant ``MAT1`` or per-sample
    ``MAT1_ROW``) -> ``(slot gradients [K * B, n_slots], G [K * B, n_mat, 2, 2] complex)``, the flagged ops numbered
    in tape order, from ONE sweep.  With phi the state in front of the gate and lambda the seed with every later gate
    undone, ``G[a][c] = sum_rest conj(lambda[a, rest]) phi[c, rest]`` over the other wires, so that for any
    parameter of the gate's matrix ``dC/dtheta = 2 Re sum_ac G[a][c] dU[a][c]/dtheta``.  complex64, or complex128
    with ``x64``.  Nothing flagged: ``G`` has shape ``[K * B, 0, 2, 2]``."""
    g, cot = _sweep(low, n_qubits, batch, obs_groups, weights, want, want_mat, x64, obs_terms)
    if cot is None:
        cot = np.zeros((g.shape[0], 0, 2, 2), dtype=np.complex128 if x64 else np.complex64)
    return g, cot


def adjoint_slot_and_matrices_gradient(low: LoweredTape, n_qubits: int, batch: int, obs_groups, weights: np.ndarray,
                                       want: Sequence[bool], want_mat: Sequence[bool], x64: bool = False,
                                       obs_terms=None) -> Tuple[np.ndarray, List[np.ndarray]]:
    """:func:`adjoint_slot_and_matrix_gradient` for matrix gates on one AND two wires: ``want_mat`` may flag ``MAT1``,
    ``MAT1_ROW``, ``MAT2`` and ``MAT2_ROW`` ops, and a tape may hold ``MAT2_ROW`` (evolved two-wire unitaries)
    -> ``(slot gradients [K * B, n_slots], [G_k])``: one ``[K * B, d, d]`` complex array per flagged op, in tape
    order, d = 2 or 4, from ONE sweep (``qmle_adjoint_cotangent_at``).  ``G_k`` is written in the index convention of
    the gate's own matrix (row = 2 * value of its first wire + value of its second), so that
    ``dC/dtheta = 2 Re sum_ac G[a][c] dU[a][c]/dtheta`` with ``U`` as the tape holds it."""
    g, cot = _sweep(low, n_qubits, batch, obs_groups, weights, want, want_mat, x64, obs_terms, two_wire=True)
    return g, (cot if cot is not None else [])


# ---- tapes with explicit matrices on three and four wires: the sweep segment by segment ----------------------------
class SweepSegment(NamedTuple):
    """The gates between two wide gates, as the segment sweep takes them."""
    low: LoweredTape        # the segment, forward
    rev: LoweredTape        # its reversed, daggered tape (``build_reverse(..., two_wire=True)``)
    terms: tuple            # one generator term per reverse op; ``out_slot`` is a COLUMN OF THE WHOLE TAPE's gradient
    columns: np.ndarray     # segment-local angle slot -> column of the whole tape's gradient
    perm: np.ndarray        # reverse slot j reads the segment's forward column perm[j] ...
    sign: np.ndarray        # ... times sign[j]
    cot_off: tuple          # per reverse op: offset of its block in the whole tape's cotangent row, or -1
    two_wire: bool          # a 4x4 block is among them


class WideGate(NamedTuple):
    """An explicit matrix on three or four wires between two segments."""
    wires: tuple
    matrix: np.ndarray      # complex128, [d, d] or one per sample [B, d, d]
    flagged: bool           # its matrix cotangent is asked for
    mat_index: int          # its number among the flagged matrix gates of the tape, or -1


class SegmentedSweep(NamedTuple):
    segments: tuple         # ``len(gates) + 1`` entries: SweepSegment, or None for a segment without an op
    gates: tuple            # WideGate
    n_slots: int            # angle slots of the whole tape, in tape order, wide gates skipped
    mat_dims: tuple         # per flagged matrix gate in tape order: 2, 4, 8 or 16
    mat_off: tuple          # one- and two-wire ones: offset of the block in the cotangent row; wide ones: -1
    cot_stride: int         # scalars per cotangent row


def plan_segments(tape, n_qubits: int, want: Sequence[bool], want_mat: Optional[Sequence[bool]] = None,
                  x64: bool = False) -> SegmentedSweep:
    """Host only: the sweep of a tape that holds explicit matrices on 3 or 4 wires, cut at them
    (``simulation.split_at_wide_gates``).  ``want[s]``: angle slot ``s`` of the whole tape needs a derivative --
    slots are numbered in tape order as ``LoweredTape`` numbers them, wide gates holding none.  ``want_mat``: one
    flag per ENTRY of ``tape``; True on a one- or two-wire matrix gate (``MAT1``, ``MAT1_ROW``, ``MAT2``,
    ``MAT2_ROW``) or on a wide gate asks for its matrix cotangent.  Empty segments are kept as None."""
    want_mat = [False] * len(tape) if want_mat is None else [bool(f) for f in want_mat]
    if len(want_mat) != len(tape):
        raise ValueError("want_mat holds one flag per tape entry")
    segs, positions = split_at_wide_gates(tape)
    bounds = [-1] + list(positions) + [len(tape)]
    flagged = [i for i, f in enumerate(want_mat) if f]  # tape order = the numbering of the cotangents
    mat_index = {i: k for k, i in enumerate(flagged)}
    mat_dims, mat_off, stride = [], [], 0
    for i in flagged:
        o = tape[i]
        d = 2 ** len(o.wires)
        mat_dims.append(d)
        if is_wide_matrix_gate(o):
            mat_off.append(-1)
        else:
            mat_off.append(stride)
            stride += 2 * d * d
    segments, slot0 = [], 0
    for k, seg in enumerate(segs):
        low = LoweredTape(seg, n_qubits)
        if not low.ops:
            segments.append(None)
            continue
        if slot0 + low.n_slots > len(want):
            raise ValueError(f"want holds {len(want)} flags, the tape has more angle slots")
        # the flags of the segment's lowered ops (a Barrier lowers to nothing) and the cotangent each one reports
        entries = [i for i in range(bounds[k] + 1, bounds[k + 1]) if tape[i].lower(n_qubits) is not None]
        local_mat = [want_mat[i] for i in entries]
        local_idx = [mat_index[i] for i in entries if want_mat[i]]
        rev_ops, terms, rev_src, rev_sign, mat_out, dims = build_reverse(
            low, _op_blobs(low, x64), list(want[slot0:slot0 + low.n_slots]), local_mat, two_wire=True)
        rev = LoweredTape(rev_ops, n_qubits)
        terms = tuple((t[0] + slot0 if t[0] >= 0 else t[0],) + tuple(t[1:]) for t in patch_marks(rev, terms))
        segments.append(SweepSegment(
            low, rev, terms, np.arange(slot0, slot0 + low.n_slots), np.asarray(rev_src, dtype=np.int64),
            np.asarray(rev_sign, dtype=np.float64),
            tuple(mat_off[local_idx[m]] if m >= 0 else -1 for m in mat_out), 4 in dims))
        slot0 += low.n_slots
    if slot0 != len(want):
        raise ValueError(f"want holds {len(want)} flags, the tape has {slot0} angle slots")
    gates = tuple(WideGate(tuple(tape[i].wires), np.asarray(tape[i]._matrix, dtype=np.complex128), want_mat[i],
                           mat_index.get(i, -1)) for i in positions)
    return SegmentedSweep(tuple(segments), gates, slot0, tuple(mat_dims), tuple(mat_off), max(1, stride))


def tape_slot_count(tape, n_qubits: int) -> int:
    """Angle slots of a tape in the numbering of :func:`plan_segments` (host only)."""
    n = 0
    for o in tape:
        low = None if is_wide_matrix_gate(o) else o.lower(n_qubits)
        n += len(low[2]) if low is not None else 0
    return n


def _z_seed_terms(obs_groups):
    """Z parities as the x = 0 words of the Pauli seed: ``[(coef, x_wire_mask, z_wire_mask, column)]``."""
    return [(1.0, 0, sum(1 << int(q) for q in grp), k) for k, grp in enumerate(obs_groups)]


def segmented_gradient(tape, n_qubits: int, batch: int, obs_groups, weights: np.ndarray, want: Sequence[bool],
                       want_mat: Optional[Sequence[bool]] = None, x64: bool = False,
                       obs_terms=None) -> Tuple[np.ndarray, List[np.ndarray]]:
    """:func:`adjoint_slot_and_matrices_gradient` for a tape that holds explicit matrices on 3 or 4 wires:
    d/d(angle slot) of ``sum_k weights[b, k] <O_k>`` and the matrix cotangents of the flagged gates (``want`` and
    ``want_mat`` as for :func:`plan_segments`) -> ``(slot gradients [K * B, n_slots], [G_k])``, one ``[K * B, d, d]``
    complex array per flagged gate in tape order, d = 2, 4, 8 or 16, in the index convention of the gate's own
    matrix.  ``weights`` ``[K * B, n_obs]``, sample-minor.  Observables: Z-parity wire groups ``obs_groups`` or, with
    ``obs_groups`` None, the Pauli term list ``obs_terms``; both seed the sweep through ``qmle_apply_pauli_sum``.

    Per chunk of samples: the forward run writes psi into the first half of a ``[2 K B, 2^n]`` tensor, the seed writes
    lambda into the second half; then, from the last wide gate to the first, ``qmle_adjoint_segment`` sweeps the
    segment behind the gate, ``qmle_wide_moment`` reports the gate's cotangent if it is flagged, and
    ``qmle_apply_matrix`` applies its dagger to all states; the first segment is swept last.  A wide gate that
    nothing is asked of is simply inverted.  complex64, or complex128 with ``x64``.  The batch is cut so that psi,
    lambda and the workspaces fit, as for a ``"state"`` run with two states per sample and cotangent."""
    torch = N.require_gpu()
    from . import memory
    from .simulation import segmented_forward, segmented_plans

    ft, fn, ct = (torch.float64, np.float64, torch.complex128) if x64 else (torch.float32, np.float32, torch.complex64)
    sw = plan_segments(tape, n_qubits, want, want_mat, x64)
    weights = np.ascontiguousarray(weights, dtype=fn)
    B, n_obs = int(batch), int(weights.shape[1])
    K = int(weights.shape[0]) // max(1, B)
    if weights.shape[0] != K * B:
        raise ValueError(f"weights must be [K * {B}, n_obs], got {weights.shape}")
    w3 = weights.reshape(K, B, n_obs)
    seed = list(obs_terms) if obs_groups is None else _z_seed_terms(obs_groups)
    plans, fwd_gates = segmented_plans(tape, n_qubits, B, x64)
    tables = [None if sg is None or not sg.low.n_slots else sg.low.angle_table(B, dtype=np.float64 if x64 else np.float32)
              for sg in sw.segments]
    grad = np.zeros((K, B, max(1, sw.n_slots)), dtype=fn)
    rows = np.zeros((K, B, sw.cot_stride), dtype=fn)
    wide = {g.mat_index: np.zeros((K, B, 2 ** len(g.wires), 2 ** len(g.wires)), dtype=np.complex128 if x64 else np.complex64)
            for g in sw.gates if g.flagged}
    dev = N.current_device()

    def sweep_segment(i: int, lo: int, hi: int, pair, g_dev, c_dev):
        sg = sw.segments[i]
        if sg is None:
            return
        if tables[i] is None:
            a_r = torch.zeros((K * (hi - lo), 1), dtype=ft, device=dev)
        else:
            a_f = torch.from_numpy(np.ascontiguousarray(tables[i][lo:hi])).to(dev).repeat(K, 1)
            a_r = (a_f.index_select(1, torch.from_numpy(sg.perm).to(dev))
                   * torch.from_numpy(sg.sign).to(device=dev, dtype=ft)).contiguous()
        has_cot = any(o >= 0 for o in sg.cot_off)
        N.adjoint_segment(get_plan(sg.rev, REV_FLAGS), a_r, pair, list(sg.terms), g_dev,
                          cot_off=list(sg.cot_off) if has_cot else None, cot=c_dev if has_cot else None,
                          two_wire=sg.two_wire)

    def run(lo: int, hi: int):
        bc = hi - lo
        pair = torch.empty((2 * K * bc, 1 << n_qubits), dtype=ct, device=dev)
        segmented_forward(plans, fwd_gates, n_qubits, lo, hi, x64, out=pair[:bc])
        for k in range(1, K):  # K cotangents per sample: the forward state once, K copies
            pair[k * bc:(k + 1) * bc].copy_(pair[:bc])
        w = torch.from_numpy(np.ascontiguousarray(w3[:, lo:hi].reshape(K * bc, n_obs))).to(dev)
        N.apply_pauli_sum(pair[:K * bc], seed, w, out=pair[K * bc:])
        g_dev = torch.zeros((K * bc, max(1, sw.n_slots)), dtype=ft, device=dev)
        c_dev = torch.zeros((K * bc, sw.cot_stride), dtype=ft, device=dev)
        for i in range(len(sw.gates) - 1, -1, -1):
            gate = sw.gates[i]
            sweep_segment(i + 1, lo, hi, pair, g_dev, c_dev)
            per_sample = gate.matrix.ndim == 3
            m = torch.from_numpy(np.ascontiguousarray(gate.matrix[lo:hi] if per_sample else gate.matrix)).to(dev)
            if gate.flagged:
                cot = N.wide_moment(pair[:K * bc], pair[K * bc:], gate.wires, m.repeat(K, 1, 1) if per_sample else m)
                wide[gate.mat_index][:, lo:hi] = cot.cpu().numpy().reshape((K, bc) + tuple(cot.shape[1:]))
            md = m.conj().transpose(-1, -2).contiguous()
            N.apply_matrix(pair, gate.wires, md.repeat(2 * K, 1, 1) if per_sample else md)  # (lambda's half: the same rows)
        sweep_segment(0, lo, hi, pair, g_dev, c_dev)
        grad[:, lo:hi] = g_dev.cpu().numpy().reshape(K, bc, -1)
        rows[:, lo:hi] = c_dev.cpu().numpy().reshape(K, bc, -1)

    chunk = memory.compute_chunk_size(n_qubits, 2 * K * B, "state", False, n_obs, n_ops=len(tape), x64=x64)
    chunk = max(1, min(B, chunk // (2 * K), N.ADJOINT_SEGMENT_MAX_BATCH // K))
    for lo in range(0, B, chunk):
        run(lo, min(B, lo + chunk))
    cots = []
    for k, (d, off) in enumerate(zip(sw.mat_dims, sw.mat_off)):
        if off < 0:
            cots.append(wide[k].reshape(K * B, d, d))
        else:
            blk = rows[:, :, off:off + 2 * d * d].reshape(K * B, d, d, 2)
            cots.append(blk[..., 0] + 1j * blk[..., 1])
    return grad.reshape(K * B, -1)[:, : sw.n_slots], cots


# ---- noisy tapes: one backward sweep over vec(rho), forward states kept ------------------------------
# one operator per pass, in tape order: the steps name ranges of the tape's ops
DENSITY_FLAGS = N.PLAN_NO_FUSION | N.PLAN_FORCE_GLOBAL | N.PLAN_NO_ABSORB | N.PLAN_TAPE_ORDER
_STEP_GATES = tuple(_ROT) + ("CPhase", "ControlledPhaseShift")
# the model of a call's state-sized reads and writes (``qmle_adjoint_density_transfers`` counts the same on its plans)
STEP_TRANSFERS_FWD, STEP_TRANSFERS_BWD, FREE_TRANSFERS = 2, 3, 2


class DensitySweep(NamedTuple):
    """What :func:`plan_density` makes of a noisy tape (host only)."""
    fwd: LoweredTape        # the doubled primitive tape: Rot split, every step's channels right behind its gate pair
    rev: LoweredTape        # its reversed, daggered tape (``build_reverse``)
    rev_src: np.ndarray     # reverse slot j holds MINUS forward column rev_src[j]
    steps: tuple            # ``N.density_step_array`` entries, tape order; ``term[0]`` is a slot of the SOURCE tape
    chan: np.ndarray        # float64: the steps' superoperators, [d, d, (re, im)] each, wires ascending
    n_slots: int            # angle slots of the source tape (``LoweredTape`` of the tape without its channels)
    n_free_fwd: int         # operators outside the steps
    n_free_bwd: int         # ... of which behind the first step: the backward sweep runs their daggers
    n_qubits: int

    @property
    def checkpoints(self) -> int:
        """State buffers per SAMPLE (never per cotangent): the working state in front of the first step and one
        behind every step."""
        return len(self.steps) + 1

    def transfers(self, n_cot: int = 1) -> int:
        """Modelled state-sized reads and writes per sample: forward once, backward per cotangent."""
        f = 1 + FREE_TRANSFERS * self.n_free_fwd + STEP_TRANSFERS_FWD * len(self.steps)
        b = 1 + (FREE_TRANSFERS * self.n_free_bwd + STEP_TRANSFERS_BWD * len(self.steps) if self.steps else 0)
        return f + int(n_cot) * b

    def sample_bytes(self, n_cot: int = 1, x64: bool = False) -> int:
        """Bytes one sample keeps resident: its checkpoints and ``n_cot`` rows of lambda."""
        return (self.checkpoints + int(n_cot)) * ((16 if x64 else 8) << (2 * self.n_qubits))


def density_rounds(batch: int, need, max_bytes: int, max_samples: Optional[int] = None) -> List[int]:
    """The batch cut into rounds that fit ``max_bytes`` (and count at most ``max_samples``: the rows of lambda of one
    engine call are one launch's grid rows).  ``need``: bytes per sample (an int: the need grows linearly), or a
    function ``samples -> bytes`` (:func:`density_call_bytes`: the library's own workspace and the call's tables).  One
    sample that does not fit is refused with the bytes it needs."""
    cost = need if callable(need) else (lambda bc: bc * int(need))
    if cost(1) > max_bytes:
        raise AdjointUnsupported(f"adjoint differentiation of this noisy circuit keeps {cost(1)} bytes of forward "
                                 f"states, lambda and workspace per sample resident; the budget is {max_bytes} bytes "
                                 "(recomputation schemes are not served)")
    cap = batch if max_samples is None else max(1, min(batch, int(max_samples)))
    per, over = 1, cap + 1  # the largest count that fits, by bisection (the need grows with the count)
    if cost(cap) <= max_bytes:
        per = cap
    while over - per > 1 and per < cap:
        mid = (per + over) // 2
        per, over = (mid, over) if cost(mid) <= max_bytes else (per, mid)
    return [min(per, batch - lo) for lo in range(0, batch, per)]


def density_call_bytes(sw: "DensitySweep", fwd_plan, rev_plan, samples: int, n_cot: int, n_obs: int,
                       x64: bool = False) -> int:
    """Device bytes of one ``qmle_adjoint_density`` call on ``samples`` samples: the library's workspace (checkpoints,
    lambda, the plans' matrix rows, the partial sums -- its own query, host only) and the tables beside it (angles of
    both tapes, weights, gradient rows, the steps' superoperators)."""
    real = 8 if x64 else 4
    rows = int(samples) * int(n_cot)
    ws = N.adjoint_density_workspace_bytes(fwd_plan, rev_plan, int(samples), int(n_cot), len(sw.steps), f64=x64)
    tables = (int(samples) * max(1, sw.fwd.n_slots) + rows * (max(1, sw.rev.n_slots) + int(n_obs) + max(1, sw.n_slots))
              + sw.chan.size) * real
    return int(ws) + int(tables)


_LAST_SWEEP: list = [None]


def last_density_sweep() -> Optional["DensitySweep"]:
    """Report only: the plan of the last :func:`density_gradient` call (what a benchmark counts transfers on)."""
    return _LAST_SWEEP[0]


def _embed(m: np.ndarray, wires, target) -> np.ndarray:
    """The operator ``m`` on ``wires`` (first wire most significant) as an operator on ``target`` (a superset)."""
    k, t = len(wires), len(target)
    order = list(wires) + [w for w in target if w not in wires]
    full = np.kron(m, np.eye(2 ** (t - k))).reshape([2] * (2 * t))
    perm = [order.index(w) for w in target]
    return full.transpose(perm + [t + p for p in perm]).reshape(2 ** t, 2 ** t)


def plan_density(tape, n_qubits: int, want: Sequence[bool], x64: bool = False) -> DensitySweep:
    """Host only: the sweep of a tape that holds Kraus channels on one and two wires.  ``want[s]``: angle slot ``s``
    of the source tape (numbered as ``LoweredTape`` numbers them, channels holding none) needs a derivative.  Every
    wanted rotation becomes a STEP: its ket and bra operators and the channels that follow it on its wires -- pulled
    forward past the operators on other wires that ``simulation.doubled_tape`` emitted in between -- as one
    superoperator.  Refused, naming the operation: channels on three or four wires, full-register diagonal encodings,
    per-sample matrices (pulse and evolved gates), explicit matrices on three or four wires."""
    from .simulation import _WideChannel, doubled_tape

    n = int(n_qubits)
    for o in tape:
        if is_wide_matrix_gate(o):
            raise AdjointUnsupported(f"adjoint differentiation of noisy circuits: {o.name} is an explicit matrix on "
                                     f"{len(o.wires)} wires")
    prims = []  # (name, wires, params, blob, source slot | None, is_channel)
    slot = 0
    items = doubled_tape(tape, n)
    i = 0
    while i < len(items):
        it = items[i]
        if isinstance(it, _WideChannel):
            raise AdjointUnsupported(f"adjoint differentiation of noisy circuits: a channel on {len(it.wires)} wires "
                                     "(_WideChannel) is applied as a Kraus sum, which the sweep does not pull back")
        name, wires, params, blob = it.lower(2 * n)
        if name == "DIAG_ALL":
            raise AdjointUnsupported("adjoint differentiation of noisy circuits: DIAG_ALL (a full-register diagonal "
                                     "encoding) is not served")
        if name in ("MAT1_ROW", "MAT2_ROW"):
            raise AdjointUnsupported(f"adjoint differentiation of noisy circuits: {name} (a per-sample matrix: pulse "
                                     "and evolved gates) is not served")
        if wires and min(wires) < n <= max(wires):  # a channel's superoperator spans both halves
            prims.append((name, list(wires), [], blob, None, True))
            i += 1
            continue
        bname, bwires, bparams, bblob = items[i + 1].lower(2 * n)  # conj(U) on the bra wires: right behind U
        if name == "Rot":
            for j, g in enumerate(("RZ", "RY", "RZ")):
                prims.append((g, list(wires), [params[j]], None, slot + j, False))
                prims.append((g, list(bwires), [bparams[j]], None, None, False))
        else:
            if len(params) > 1:
                raise AdjointUnsupported(f"{name}: more than one angle per gate")
            prims.append((name, list(wires), list(params), blob, slot if params else None, False))
            prims.append((bname, list(bwires), list(bparams), bblob, None, False))
        slot += len(params)
        i += 2
    if slot != len(want):
        raise ValueError(f"want holds {len(want)} flags, the tape has {slot} angle slots")
    # steps: the wanted rotations with the channels behind them on their wires
    used, seq, spans = [False] * len(prims), [], []  # spans: (first index in seq, count, channel prims, ket prim)
    for i, p in enumerate(prims):
        if used[i]:
            continue
        used[i] = True
        seq.append(p)
        if p[4] is None or not want[p[4]] or p[5]:
            continue
        if p[0] not in _STEP_GATES:
            raise AdjointUnsupported(f"no adjoint rule for {p[0]}")
        used[i + 1] = True
        seq.append(prims[i + 1])
        mine, chans = set(p[1]) | set(prims[i + 1][1]), []
        for j in range(i + 2, len(prims)):
            if used[j]:
                continue
            q = prims[j]
            if q[5] and set(q[1]) <= mine:
                used[j] = True
                seq.append(q)
                chans.append(q)
            elif mine & set(q[1]):
                break
        spans.append((len(seq) - 2 - len(chans), 2 + len(chans), chans, p))
    fwd = LoweredTape([_Lowered((p[0], p[1], p[2], p[3])) for p in seq], 2 * n)
    fslot = {}  # index in seq -> forward slot of the doubled tape
    for k, (_name, _w, slots, _off) in enumerate(fwd.ops):
        if slots:
            fslot[k] = slots[0]
    want2 = [False] * fwd.n_slots
    for first, _cnt, _ch, _p in spans:
        want2[fslot[first]] = True
    rev_ops, terms, rev_src = build_reverse(fwd, _op_blobs(fwd, x64), want2)
    rev = LoweredTape(rev_ops, 2 * n)
    R = len(seq)
    assert len(rev_ops) == R, "the doubled primitive tape reverses operator by operator"
    steps, blobs, off = [], [], 0
    for first, cnt, chans, p in spans:
        ket = sorted(p[1])
        target = ket + [w + n for w in ket]
        chan_off = -1
        if chans:
            c = np.eye(2 ** len(target), dtype=np.complex128)
            for q in chans:
                m = np.asarray(q[3], dtype=np.float64).reshape(-1, 2)
                d = 2 ** len(q[1])
                c = _embed((m[:, 0] + 1j * m[:, 1]).reshape(d, d), q[1], target) @ c
            blobs.append(np.stack([c.real, c.imag], axis=-1).reshape(-1))
            chan_off, off = off, off + blobs[-1].size
        t = terms[R - 1 - first]
        steps.append((N.OPCODES[p[0]], (p[1][0], p[1][1] if len(p[1]) > 1 else -1), fslot[first], chan_off, first, cnt,
                      R - first - cnt, cnt, (p[4],) + tuple(t[1:])))
    in_step = sum(s[5] for s in steps)
    behind = sum(1 for k in range(R) if steps and k >= steps[0][4]) - in_step
    return DensitySweep(fwd, rev, np.asarray(rev_src if rev_src else [0], dtype=np.int64), tuple(steps),
                        np.concatenate(blobs) if blobs else np.zeros(0), slot, R - in_step, behind, n)


def density_gradient(tape, n_qubits: int, batch: int, obs_groups, weights: np.ndarray, want: Sequence[bool],
                     x64: bool = False, obs_terms=None, max_bytes: Optional[int] = None) -> np.ndarray:
    """:func:`adjoint_slot_gradient` for a tape with Kraus channels on one and two wires: d/d(angle slot) of
    ``sum_k weights[b, k] Tr(O_k rho)`` -> ``[K * B, n_slots]`` (``weights`` ``[K * B, n_obs]``, sample-minor; columns
    that are not wanted stay zero), by ``qmle_adjoint_density``: the forward states of every step stay resident, the
    observable alone is pulled back, and K cotangents share one forward run.  Observables: Z-parity wire groups
    ``obs_groups`` or, with ``obs_groups`` None, the Pauli term list ``obs_terms``, both on the ``n_qubits`` system
    wires.  The batch is cut into rounds so that checkpoints, lambda and workspace (:func:`density_call_bytes`) fit
    ``max_bytes`` (default: ``memory.available_memory_bytes()``); a sample that does not fit alone raises :class:`AdjointUnsupported`."""
    torch = N.require_gpu()
    from . import memory

    ft, fn = (torch.float64, np.float64) if x64 else (torch.float32, np.float32)
    sw = plan_density(tape, n_qubits, want, x64)
    weights = np.ascontiguousarray(weights, dtype=fn)
    B, n_obs = int(batch), int(weights.shape[1])
    K = int(weights.shape[0]) // max(1, B)
    if weights.shape[0] != K * B or K < 1:
        raise ValueError(f"weights must be [K * {B}, n_obs], got {weights.shape}")
    budget = int(memory.available_memory_bytes() if max_bytes is None else max_bytes)
    _LAST_SWEEP[0] = sw
    grad = np.zeros((K, B, max(1, sw.n_slots)), dtype=fn)
    if not sw.steps:
        return grad.reshape(K * B, -1)[:, : sw.n_slots]
    dev = N.current_device()
    fwd_plan, rev_plan = get_plan(sw.fwd, DENSITY_FLAGS), get_plan(sw.rev, DENSITY_FLAGS)
    # checkpoints, lambda AND workspace: the rounds are sized by what a call of that many samples really allocates
    rounds = density_rounds(B, lambda bc: density_call_bytes(sw, fwd_plan, rev_plan, bc, K, n_obs, x64), budget,
                            max_samples=max(1, N.MAX_ROWS // K))
    table = sw.fwd.angle_table(B, dtype=np.float64 if x64 else np.float32)
    chan = torch.from_numpy(sw.chan.astype(fn)).to(dev) if sw.chan.size else None
    perm = torch.from_numpy(sw.rev_src).to(dev)
    w3 = weights.reshape(K, B, n_obs)
    lo = 0
    for bc in rounds:
        hi = lo + bc
        a_f = torch.from_numpy(np.ascontiguousarray(table[lo:hi])).to(dev)
        if sw.rev.n_slots:
            a_r = (-a_f.index_select(1, perm)).repeat(K, 1).contiguous()
        else:
            a_r = torch.zeros((K * bc, 1), dtype=ft, device=dev)
        if not sw.fwd.n_slots:
            a_f = torch.zeros((bc, 1), dtype=ft, device=dev)
        w = torch.from_numpy(np.ascontiguousarray(w3[:, lo:hi].reshape(K * bc, n_obs))).to(dev)
        g = N.adjoint_density(fwd_plan, rev_plan, a_f, a_r, w, obs_groups, list(sw.steps), chan, max(1, sw.n_slots),
                              n_cot=K, obs_terms=obs_terms)
        grad[:, lo:hi] = g.cpu().numpy().reshape(K, bc, -1)
        lo = hi
    return grad.reshape(K * B, -1)[:, : sw.n_slots]
