"""Reference, cases and named wrong variants for the forward run of the complex128 engine
(``qmle_run_batch_f64``, ``qmle_apply_inplace_f64``).  Not a test module: tests/test_x64_reference_cpu.py checks it
without a GPU, tests/test_gpu_x64_routes.py runs its cases on one.

A tape here is the oracle's ``[(name, wires, params)]`` with two extensions: a float parameter may be an array
``[B]`` (one angle per row of the batch), and ``("DiagAll", [], (x, marks))`` is the Golomb-style diagonal
``exp(-i * marks * x)`` over the whole register (``marks`` one float per basis state, index = the state's index).
``("Matrix", wires, (M,))`` takes 1, 2 or 4 wires.  Wire ``w`` is axis ``w`` of the state reshaped to ``(2,) * n``,
that is bit position ``n - 1 - w`` of the index; the first wire of an operator is the most significant bit of its row.

Wrong variants (``WRONG``): each is ONE deliberate mistake in that reference, the kind a kernel can make --
  control_target   (a) control and target exchanged (first control <-> first target)
  targets          (b) the two targets of a two-wire operator exchanged
  transpose        (c) every matrix transposed
  conjugate        (d) every matrix conjugated (the Golomb phase with it)
  bit_order        (e) wire w read as bit position w, in gates and in observable masks
  mat4_order       (f) the wire order of a 4-wire matrix reversed
  angles_prev      (g) row b evaluated with the angles of row b - 1
  angles_mod64     (g) row b evaluated with the angles of row b mod 64
  second_round     (h) rows of the second streaming round evaluated with the rows of the first
  golomb_sign      (i) the Golomb phase with the opposite sign
  golomb_bitrev    (i) the Golomb marks in bit-reversed order
  consts_f32       (j) explicit matrices and marks rounded to float32
``applies(case, variant)`` says, from the gates' own symmetries and nothing else, whether the mistake changes the
operator at all (CPhase does not know which wire is the control; RY at n = 5 on wire 2 sits on bit 2 either way)."""
import itertools
from dataclasses import dataclass, field

import numpy as np

from oracle import einsum_sim as OE
from oracle import gates as G

BATCH = 3
TOL = 1e-12         # the project's complex128 bar: max |got - want| for unit-norm states and observables of norm 1
SEE = 1e-6          # what every applicable wrong variant must move the compared quantity by
SEE_F32 = 1e-9      # ... except constants rounded to float32: see_bar()

WRONG = ("control_target", "targets", "transpose", "conjugate", "bit_order", "mat4_order", "angles_prev",
         "angles_mod64", "second_round", "golomb_sign", "golomb_bitrev", "consts_f32")

# what a gate's matrix is blind to
_SYMMETRIC_WIRES = {"CZ", "CPhase", "SWAP", "RXX", "RYY", "RZZ"}       # any order of its wires
_CONTROLLED = {"CX": 1, "CY": 1, "CZ": 1, "CRX": 1, "CRY": 1, "CRZ": 1, "CPhase": 1, "CCX": 2, "CSWAP": 1}
_TWO_TARGETS = {"SWAP", "RXX", "RYY", "RZZ", "RZX", "CSWAP"}             # ("Matrix" on two wires as well)
_SYMMETRIC_MATRIX = {"Id", "PauliX", "PauliZ", "H", "S", "RX", "RZ", "CX", "CZ", "CRX", "CRZ", "CPhase", "SWAP",
                     "RXX", "RYY", "RZZ", "RZX", "CCX", "CSWAP"}         # M^T = M
_REAL_MATRIX = {"Id", "PauliX", "PauliZ", "H", "RY", "CX", "CZ", "CRY", "SWAP", "CCX", "CSWAP"}   # conj M = M


def _canon(name, wires):
    """The operator ``name`` on ``wires`` up to the orders of wires its matrix cannot tell apart."""
    w = tuple(int(x) for x in wires)
    if name in _SYMMETRIC_WIRES:
        return name, frozenset(w)
    if name == "CCX":
        return name, frozenset(w[:2]), w[2]
    if name == "CSWAP":
        return name, w[0], frozenset(w[1:])
    return name, w


def _rewire(name, wires, n, wrong):
    w = [int(x) for x in wires]
    if wrong == "bit_order":
        return [n - 1 - x for x in w]
    if wrong == "control_target" and name in _CONTROLLED:
        nc = _CONTROLLED[name]
        w[0], w[nc] = w[nc], w[0]
    elif wrong == "targets" and (name in _TWO_TARGETS or (name == "Matrix" and len(w) == 2)):
        w[-1], w[-2] = w[-2], w[-1]
    elif wrong == "mat4_order" and name == "Matrix" and len(w) == 4:
        w = w[::-1]
    return w


def bit_reverse(n):
    idx = np.arange(1 << n)
    out = np.zeros_like(idx)
    for b in range(n):
        out |= ((idx >> b) & 1) << (n - 1 - b)
    return out


def _rows(p, B, wrong):
    """One float parameter as the [B] values the rows are evaluated with."""
    a = np.broadcast_to(np.asarray(p, dtype=np.float64), (B,)).copy()
    if wrong == "angles_prev":
        a = np.roll(a, 1)
    elif wrong == "angles_mod64":
        a = a[np.arange(B) % 64]
    return a


def _f32(x):
    x = np.asarray(x)
    if np.iscomplexobj(x):
        return x.astype(np.complex64).astype(np.complex128)
    return x.astype(np.float32).astype(np.float64)


def apply_tape(psi0, tape, n, wrong=None):
    """``tape`` applied to the start states ``psi0`` [B, 2^n], complex128, one ``einsum`` per gate (the oracle's
    subscripts with a batch letter in front).  ``wrong``: one of ``WRONG`` (``second_round`` is a matter of which rows
    a case compares, not of the evolution)."""
    psi = np.array(psi0, dtype=np.complex128)
    B = psi.shape[0]
    assert psi.shape == (B, 1 << n)
    for name, wires, params in tape:
        if name == "Barrier":
            continue
        if name == "DiagAll":
            x, marks = _rows(params[0], B, wrong), np.asarray(params[1], dtype=np.float64)
            if wrong == "consts_f32":
                marks = _f32(marks)
            if wrong == "golomb_bitrev":
                marks = marks[bit_reverse(n)]
            sign = 1.0 if wrong in ("golomb_sign", "conjugate") else -1.0
            psi = psi * np.exp(sign * 1j * marks[None, :] * x[:, None])
            continue
        k = len(wires)
        w = _rewire(name, wires, n, wrong)
        if name == "Matrix":
            M = np.asarray(params[0], dtype=np.complex128)
            mats = (_f32(M) if wrong == "consts_f32" else M)[None]
        elif params:
            cols = [_rows(p, B, wrong) for p in params]
            mats = np.stack([G.matrix(name, tuple(c[b] for c in cols)) for b in range(B)])
        else:
            mats = G.matrix(name, ())[None]
        if wrong == "transpose":
            mats = mats.transpose(0, 2, 1)
        elif wrong == "conjugate":
            mats = mats.conj()
        gate, state, result = OE.einsum_subscript(n, k, tuple(w)).replace("->", ",").split(",")
        mats = np.broadcast_to(mats, (B,) + mats.shape[1:]).reshape((B,) + (2,) * (2 * k))
        psi = np.einsum(f"Z{gate},Z{state}->Z{result}", mats, psi.reshape((B,) + (2,) * n)).reshape(B, 1 << n)
    return psi


def zero_states(B, n):
    psi = np.zeros((B, 1 << n), dtype=np.complex128)
    psi[:, 0] = 1.0
    return psi


def expval_z(psi, groups, n, wrong=None):
    """<Z..Z> of every wire group: sum of +-|psi|^2."""
    idx = np.arange(1 << n)
    p = np.abs(psi) ** 2
    out = np.empty((psi.shape[0], len(groups)))
    for k, g in enumerate(groups):
        sign = np.ones(1 << n)
        for w in g:
            pos = int(w) if wrong == "bit_order" else n - 1 - int(w)
            sign = sign * (1 - 2 * ((idx >> pos) & 1))
        out[:, k] = p @ sign
    return out


# ---- cases ------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """One run of the engine: ``tape`` on ``n`` wires and ``B`` rows, from ``psi0`` (None: |0..0>, the only start
    of ``run64``), behind ``prefix`` (a tape whose evolution the cases of a family share); ``groups``: the <Z..Z>
    wire groups a measuring case compares as well."""
    label: str
    n: int
    tape: list
    B: int = BATCH
    psi0: object = None
    prefix: tuple = ()
    groups: tuple = ()
    compares: tuple = ("state",)
    _native: object = field(default=None, repr=False)

    @property
    def full_tape(self):
        return list(self.prefix) + list(self.tape)

    def native(self):
        """-> (ops, angles float64 [B, slots], consts float64) of the whole tape for ``_native.Plan``."""
        if self._native is None:
            self._native = to_native(self.full_tape, self.n, self.B)
        return self._native


def to_native(tape, n, B):
    ops, cols, consts = [], [], []
    for name, wires, params in tape:
        if name == "Matrix":
            M = np.asarray(params[0], dtype=np.complex128)
            assert M.shape == (1 << len(wires),) * 2 and len(wires) in (1, 2, 4)
            ops.append(({1: "MAT1", 2: "MAT2", 4: "MAT4"}[len(wires)], list(wires), [], len(consts)))
            consts.extend(np.stack([M.real, M.imag], axis=-1).reshape(-1).tolist())
        elif name == "DiagAll":
            marks = np.asarray(params[1], dtype=np.float64)
            assert marks.shape == (1 << n,)
            ops.append(("DIAG_ALL", [], [len(cols)], len(consts)))
            consts.extend(marks.tolist())
            cols.append(_rows(params[0], B, None))
        else:
            ops.append((name, list(wires), list(range(len(cols), len(cols) + len(params))), -1))
            cols.extend(_rows(p, B, None) for p in params)
    angles = np.stack(cols, axis=1) if cols else np.zeros((B, 0))
    return ops, np.ascontiguousarray(angles, dtype=np.float64), np.array(consts, dtype=np.float64)


_prefix_cache = {}


def reference_state(case, wrong=None):
    """The case's final states [B, 2^n] under the reference (``wrong``: under that mistake)."""
    psi = zero_states(case.B, case.n) if case.psi0 is None else case.psi0
    if case.prefix:  # (a family's prefix is one tuple object: evolve it once per variant)
        key = (id(case.prefix), case.n, case.B, wrong)
        if key not in _prefix_cache:
            _prefix_cache[key] = (case.prefix, apply_tape(psi, case.prefix, case.n, wrong))
        psi = _prefix_cache[key][1]
    return apply_tape(psi, case.tape, case.n, wrong)


def compared(case, wrong=None):
    """name -> array: everything the GPU test of this case compares, in its own norm (max |difference|)."""
    psi = reference_state(case, wrong)
    out = {}
    if "state" in case.compares:
        out["state"] = psi
    if "probs" in case.compares:
        out["probs"] = np.abs(psi) ** 2
    if "expval" in case.compares:
        out["expval"] = expval_z(psi, case.groups, case.n, wrong)
    return out


def applies(case, wrong, quantity="state"):
    """Does the mistake change the compared ``quantity`` of the case?  Decided from the gates alone: wires up to the orders their
    matrix cannot tell apart, symmetric / real matrices, angle rows that differ, constants that are no float32 numbers.
    A conjugated circuit from |0..0> ends in the conjugated state: probabilities and <Z> cannot see ``conjugate``."""
    n, B, tape = case.n, case.B, case.full_tape
    gates = [(nm, w, p) for nm, w, p in tape if nm not in ("Barrier", "DiagAll")]
    diags = [p for nm, _, p in tape if nm == "DiagAll"]
    if wrong in ("control_target", "targets", "mat4_order", "bit_order"):
        hit = any(_canon(nm, _rewire(nm, w, n, wrong)) != _canon(nm, w) for nm, w, _ in gates)
        if wrong == "bit_order" and quantity == "expval":
            hit = hit or any({n - 1 - int(w) for w in g} != {int(w) for w in g} for g in case.groups)
        return hit
    if wrong == "transpose":
        return any(nm not in _SYMMETRIC_MATRIX for nm, _, _ in gates)
    if wrong == "conjugate":
        return (quantity == "state" or case.psi0 is not None) and (bool(diags) or any(nm not in _REAL_MATRIX for nm, _, _ in gates))
    if wrong in ("angles_prev", "angles_mod64"):
        if wrong == "angles_mod64" and B <= 64:
            return False
        angles = [np.asarray(p) for nm, _, ps in tape if nm != "Matrix" for p in (ps[:1] if nm == "DiagAll" else ps)]
        return any(a.ndim == 1 and not np.array_equal(_rows(a, B, wrong), a) for a in angles)
    if wrong in ("golomb_sign", "golomb_bitrev"):
        return bool(diags) and (wrong == "golomb_sign" or n > 1)  # (one bit reversed is that bit)
    if wrong == "consts_f32":
        return (any(not np.array_equal(_f32(p[1]), p[1]) for p in diags)
                or any(nm == "Matrix" and not np.array_equal(_f32(p[0]), p[0]) for nm, _, p in gates))
    if wrong == "second_round":
        return False  # (rows, not evolution: test_two_rounds / two_round_case)
    raise KeyError(wrong)


def see_bar(case, wrong):
    """What ``wrong`` must move the case by: 1e-6, a million times the bar -- except ``consts_f32``, the one mistake
    whose size is set by a number format and not by the inputs.  float32 rounds the components of a unitary (at most
    1 in magnitude) by at most 2^-25 = 3e-8 and a mark in [0, 50) by at most 1.9e-6, and an amplitude moves by that
    fraction of ITSELF: no unitary, marks or unit-norm state reach 1e-6 in max |difference| from matrices alone, and
    a state spread over 2^14 amplitudes does not from marks either.  The condition there is 1e-9 -- a thousand
    times the bar, and the figure the constants test asks of the same difference on the GPU."""
    return SEE_F32 if wrong == "consts_f32" else SEE


# ---- seeded inputs -----------------------------------------------------------------------------------------
def generic_angles(rng, size=None):
    """Angles at least 0.2 away from every multiple of pi / 2."""
    return rng.integers(0, 4, size) * (np.pi / 2) + rng.uniform(0.2, np.pi / 2 - 0.2, size)


def haar_states(rng, B, n):
    """Random unit-norm start states: complex normal amplitudes (Haar) under a power-law envelope in a random order
    of the basis states.  Every amplitude is generic and none is zero, and a few stay of order 0.1 at any n -- the
    max-norm comparisons then resolve at n = 14 what they resolve at n = 5 (flat Haar amplitudes are 2^-7 there)."""
    D = 1 << n
    psi = rng.normal(size=(B, D)) + 1j * rng.normal(size=(B, D))
    for b in range(B):
        psi[b] *= (1.0 + rng.permutation(D)) ** -0.75
    return psi / np.linalg.norm(psi, axis=1, keepdims=True)


def random_unitary(rng, d):
    q, r = np.linalg.qr(rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d)))
    return q * (np.diagonal(r) / np.abs(np.diagonal(r)))[None, :]


def random_marks(rng, n):
    return rng.uniform(0.0, 50.0, 1 << n)


KINDS = ("RY", "MAT1", "CRX", "CPhase", "CCX", "RZX", "MAT2", "CSWAP", "MAT4", "DIAG_ALL")
_KIND_WIRES = {"RY": 1, "MAT1": 1, "CRX": 2, "CPhase": 2, "CCX": 3, "RZX": 2, "MAT2": 2, "CSWAP": 3, "MAT4": 4,
               "DIAG_ALL": 0}


def kind_gate(kind, wires, n, rng, B=BATCH):
    """One tape entry of ``kind`` on ``wires`` with per-row generic angles / a random unitary / random marks."""
    if kind == "DIAG_ALL":
        return ("DiagAll", [], (generic_angles(rng, B), random_marks(rng, n)))
    if kind in ("MAT1", "MAT2", "MAT4"):
        return ("Matrix", list(wires), (random_unitary(rng, 1 << len(wires)),))
    if kind in ("CCX", "CSWAP"):
        return (kind, list(wires), ())
    return (kind, list(wires), (generic_angles(rng, B),))


def positions(kind, wire_set):
    """Every ordered choice of the kind's wires from ``wire_set``."""
    k = _KIND_WIRES[kind]
    return [()] if k == 0 else list(itertools.permutations(wire_set, k))


WIRES_5 = (0, 1, 2, 3, 4)
WIRES_10 = (0, 1, 4, 5, 8, 9)
WIRES_14 = (0, 1, 6, 7, 12, 13)
_SEEDS = {}  # (family, n, kind) -> seed; a case that failed the discrimination condition gets another seed here


def _seed(*key):
    import zlib

    return _SEEDS.get(key, zlib.crc32(repr(key).encode()))


_case_cache = {}


def _cached(fn):
    def wrapper(*args):
        key = (fn.__name__,) + args
        if key not in _case_cache:
            _case_cache[key] = fn(*args)
        return _case_cache[key]
    wrapper.__name__ = fn.__name__
    wrapper.__doc__ = fn.__doc__
    return wrapper


@_cached
def resident_cases(n, kind):
    """Family a: one gate of ``kind`` at every position, on 3 random resident states (``apply_inplace64``)."""
    wire_set = {1: (0,), 5: WIRES_5, 14: WIRES_14}[n]
    rng = np.random.default_rng(_seed("a", n, kind))
    psi0 = haar_states(rng, BATCH, n)   # (one set of start states per (n, kind): the positions differ, not the states)
    return [Case(f"a {kind} n={n} wires={list(w)}", n, [kind_gate(kind, w, n, rng)], psi0=psi0)
            for w in positions(kind, wire_set)]


RESIDENT = [(1, k) for k in ("RY", "MAT1", "DIAG_ALL")] + [(5, k) for k in KINDS] + [(14, k) for k in KINDS]


@_cached
def entangling_prefix(n):
    """RY and RZ on every wire, then a CX chain: a generic state, and neighbours to merge with."""
    rng = np.random.default_rng(_seed("prefix", n))
    tape = [(g, [q], (generic_angles(rng, BATCH),)) for g in ("RY", "RZ") for q in range(n)]
    return tuple(tape + [("CX", [q, q + 1], ()) for q in range(n - 1)])


@_cached
def lds_kind_cases(n, kind):
    """Family b, first half: the kinds of family a behind the entangling prefix, through ``run64``."""
    wire_set = {10: WIRES_10, 14: WIRES_14}[n]
    rng = np.random.default_rng(_seed("b", n, kind))
    prefix = entangling_prefix(n)
    return [Case(f"b {kind} n={n} wires={list(w)}", n, [kind_gate(kind, w, n, rng)], prefix=prefix)
            for w in positions(kind, wire_set)]


MERGES = ("1q_onto_1q", "1q_onto_RXX", "1q_onto_MAT2", "4x4_same_pair", "4x4_reversed_pair", "4x4_takes_pending")
PAIRS_14 = ((0, 13), (13, 0), (1, 6), (7, 12), (12, 1), (6, 7))


def merge_tape(merge, a, b, rng, B=BATCH):
    """The gates of one merge case on the ordered pair (a, b); every gate non-symmetric where the case allows."""
    ang = lambda: generic_angles(rng, B)  # noqa: E731
    if merge == "1q_onto_1q":
        return [("RY", [a], (ang(),)), ("RX", [a], (ang(),)), ("Rot", [b], (ang(), ang(), ang())), ("RZ", [b], (ang(),))]
    if merge == "1q_onto_RXX":      # pad 1 (first wire) and pad 2 (second wire)
        return [("RXX", [a, b], (ang(),)), ("RY", [a], (ang(),)), ("Rot", [b], (ang(), ang(), ang()))]
    if merge == "1q_onto_MAT2":
        return [("Matrix", [a, b], (random_unitary(rng, 4),)), ("Rot", [b], (ang(), ang(), ang())),
                ("Matrix", [a], (random_unitary(rng, 2),))]
    if merge == "4x4_same_pair":
        return [("RZX", [a, b], (ang(),)), ("Matrix", [a, b], (random_unitary(rng, 4),))]
    if merge == "4x4_reversed_pair":
        return [("RZX", [a, b], (ang(),)), ("Matrix", [b, a], (random_unitary(rng, 4),))]
    if merge == "4x4_takes_pending":
        return [("RY", [a], (ang(),)), ("RX", [b], (ang(),)), ("RZ", [b], (ang(),)), ("RZX", [a, b], (ang(),))]
    raise KeyError(merge)


@_cached
def merge_cases(n, merge):
    """Family b, second half: what ``lower_tape`` merges (and what it must not), behind the entangling prefix."""
    pairs = list(itertools.permutations(WIRES_10, 2)) if n == 10 else list(PAIRS_14)
    rng = np.random.default_rng(_seed("merge", n, merge))
    prefix = entangling_prefix(n)
    return [Case(f"b {merge} n={n} pair={a, b}", n, merge_tape(merge, a, b, rng), prefix=prefix) for a, b in pairs]


@_cached
def constants_case(n, resident):
    """Family c: MAT1, MAT2, MAT4 and DIAG_ALL whose constants are no float32 numbers, between rotations."""
    rng = np.random.default_rng(_seed("c", n, resident))
    w = [0, n // 3, (2 * n) // 3, n - 1] if n >= 4 else list(range(n))
    tape = [("RY", [q], (generic_angles(rng, BATCH),)) for q in range(n)]
    tape += [("Matrix", [w[1]], (random_unitary(rng, 2),)), ("Matrix", [w[3], w[0]], (random_unitary(rng, 4),)),
             ("CRX", [w[0], w[2]], (generic_angles(rng, BATCH),)),
             ("Matrix", [w[2], w[0], w[3], w[1]], (random_unitary(rng, 16),)),
             ("DiagAll", [], (generic_angles(rng, BATCH), random_marks(rng, n))),
             ("RZX", [w[1], w[3]], (generic_angles(rng, BATCH),))]
    return Case(f"c n={n}{' resident' if resident else ''}", n, tape,
                psi0=haar_states(rng, BATCH, n) if resident else None)


CONSTANTS = [(6, False), (14, False), (6, True)]

ROW_BATCHES = (1, 2, 63, 64, 65, 130)


@_cached
def rows_case(n, B, resident):
    """Family d: about 20 gates of every kind on three wires spread over the register, every row its own angles."""
    rng = np.random.default_rng(_seed("d", n, B, resident))
    w = [0, n // 2, n - 1]
    ang = lambda: generic_angles(rng, B)  # noqa: E731
    tape = [("H", [w[0]], ()), ("RX", [w[1]], (ang(),)), ("RY", [w[2]], (ang(),)), ("CX", [w[0], w[1]], ()),
            ("Rot", [w[1]], (ang(), ang(), ang())), ("CRZ", [w[2], w[0]], (ang(),)), ("RYY", [w[1], w[2]], (ang(),)),
            ("S", [w[0]], ()), ("CY", [w[1], w[2]], ()), ("RZ", [w[0]], (ang(),)), ("CRX", [w[0], w[2]], (ang(),)),
            ("DiagAll", [], (ang(), random_marks(rng, n))), ("RZX", [w[2], w[1]], (ang(),)),
            ("CCX", [w[2], w[0], w[1]], ()), ("CRY", [w[1], w[0]], (ang(),)), ("PauliY", [w[2]], ()),
            ("CPhase", [w[2], w[1]], (ang(),)), ("Matrix", [w[1]], (random_unitary(rng, 2),)),
            ("RXX", [w[0], w[2]], (ang(),)), ("CSWAP", [w[1], w[2], w[0]], ()), ("SWAP", [w[0], w[1]], ()),
            ("Matrix", [w[2], w[0]], (random_unitary(rng, 4),)), ("RZZ", [w[1], w[0]], (ang(),)),
            ("PauliX", [w[0]], ()), ("CZ", [w[0], w[2]], ()), ("PauliZ", [w[1]], ()), ("RY", [w[1]], (ang(),))]
    if resident:
        return Case(f"d rows n={n} B={B} resident", n, tape, B=B, psi0=haar_states(rng, B, n))
    return Case(f"d rows n={n} B={B}", n, tape, B=B, groups=tuple([q] for q in range(n)),
                compares=("state", "probs", "expval"))


ROWS = [(3, B, False) for B in ROW_BATCHES] + [(14, 2, False), (14, 65, False), (5, 65, True)]

MEASURE_N = (1, 2, 3, 7, 10, 12, 13, 14)
DENSITY = ((1, 3), (2, 3), (3, 3), (7, 3), (10, 3), (12, 1))   # (n, B)


def _per_row(tape, rng, B):
    return [(nm, w, tuple(p + rng.uniform(0.25, 0.6) * np.arange(B) for p in ps)) for nm, w, ps in tape]


@_cached
def measure_case(n, B):
    """Family e: a random tape of every gate kind with a Golomb diagonal in the middle, per-row angles."""
    from tests.helpers import random_tape

    rng = np.random.default_rng(_seed("e", n, B))
    head = [("RY", [q], (float(generic_angles(rng)),)) for q in range(n)]
    tape = _per_row(head + random_tape(n, 8, rng), rng, B)
    tape.append(("DiagAll", [], (generic_angles(rng, B), random_marks(rng, n))))
    tape += _per_row(random_tape(n, 6, rng) + [("RX", [q], (float(generic_angles(rng)),)) for q in range(n)], rng, B)
    groups = tuple([q] for q in range(n)) + (((0, n - 1), tuple(range(min(n, 3)))) if n > 1 else ())
    return Case(f"e n={n} B={B}", n, tape, B=B, groups=groups, compares=("state", "probs", "expval"))


@_cached
def observables_case(n):
    """Family e: 32 <Z..Z> observables, the ABI's limit -- single wires, the parity of all wires, random subsets."""
    rng = np.random.default_rng(_seed("obs", n))
    base = measure_case(n, BATCH)
    groups = [(q,) for q in range(n)] + [tuple(range(n))]
    while len(groups) < 32:
        g = tuple(int(x) for x in np.flatnonzero(rng.random(n) < 0.5))
        if g and g not in groups:
            groups.append(g)
    return Case(f"e 32 observables n={n}", n, base.tape, groups=tuple(groups), compares=("expval",))


TWO_ROUND_N, TWO_ROUND_B = 14, 16385


@_cached
def two_round_case():
    """Family f: a dozen gates with controlled rotations and a Golomb diagonal, THREE distinct angle rows (the batch
    of 16385 cycles through them).  -> the 3-row case; row b of the batch is its row b % 3."""
    n = TWO_ROUND_N
    rng = np.random.default_rng(_seed("f"))
    ang = lambda: generic_angles(rng, 3)  # noqa: E731
    tape = [("RY", [q], (ang(),)) for q in (0, 3, 6, 9, 12, 13)]
    tape += [("CRX", [0, 13], (ang(),)), ("CX", [3, 4], ()), ("RZX", [12, 6], (ang(),)),
             ("DiagAll", [], (ang(), random_marks(rng, n))), ("CRY", [9, 1], (ang(),)), ("RX", [4], (ang(),)),
             ("Rot", [12], (ang(), ang(), ang())), ("CRZ", [13, 12], (ang(),)), ("H", [1], ())]
    return Case("f two rounds", n, tape, B=3, groups=((0,), (13,), (1, 4, 12)), compares=("state", "expval"))


def schedule_case():
    """Family g: the two-layer hardware-efficient tape of the autotuner test at n = 16, 4 rows."""
    from oracle.circuits import bricks

    n, B = 16, 4
    rng = np.random.default_rng(_seed("g"))
    tape = []
    for _ in range(2):
        tape += [(g, [q], (generic_angles(rng, B),)) for g in ("RY", "RZ", "RY") for q in range(n)]
        tape += [("CX", list(w), ()) for w in bricks(n, mirror=False) +
                 bricks(n, offset=-1, modulo=True, wrap=True, mirror=False)]
    return Case("g schedule n=16", n, tape, B=B)


def all_cases():
    """Every case the GPU tests run, for the discrimination condition."""
    for n, kind in RESIDENT:
        yield from resident_cases(n, kind)
    for kind in KINDS:
        yield from lds_kind_cases(10, kind)
    for n in (10, 14):
        for merge in MERGES:
            yield from merge_cases(n, merge)
    for n, resident in CONSTANTS:
        yield constants_case(n, resident)
    for n, B, resident in ROWS:
        yield rows_case(n, B, resident)
    for n in MEASURE_N:
        yield measure_case(n, BATCH)
    for n, B in DENSITY:
        if B != BATCH or n not in MEASURE_N:
            yield measure_case(n, B)
    for n in (9, 14):
        yield observables_case(n)
    yield two_round_case()
    yield schedule_case()
