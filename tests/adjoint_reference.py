"""An exact complex128 reference gradient for the adjoint sweep, and the cases the route tests run.

``reference_gradient`` differentiates ``C(theta) = sum_k w_k <psi(theta)| O_k |psi(theta)>`` with forward
simulations alone: the oracle's gate matrices (``oracle/gates.py``) and its contraction
(``oracle/einsum_sim.py``) at shifted angles, combined by the exact rule of the gate that holds the angle.
Nothing here knows a generator, a mask, a reversed tape or a coefficient of ``adjoint.build_reverse``:

* RX, RY, RZ, RXX, RYY, RZZ, RZX, the three angles of Rot and ControlledPhaseShift (frequencies 0, +-1):
  ``(C(t + pi/2) - C(t - pi/2)) / 2``;
* CRX, CRY, CRZ (frequencies 0, +-1/2, +-1): shifts +-pi/2, +-3pi/2 with ``(sqrt2 +- 1) / (4 sqrt2)``;
* the Golomb encoding ``exp(-i marks x)`` (as many frequencies as mark differences): the 4th-order central
  difference.  Its error is ``|C^(5)| h^4 / 30`` and the cost has frequencies up to the largest mark (44 on
  three wires, 1522 on five), so the step is ``5e-4 / max(marks)``: at 1522 a step of ``1e-3`` would leave an
  error of ``1522^5 1e-12 / 30``, more than the gradient.  ``tests/test_adjoint_reference_cpu.py`` bounds what is left by
  comparing the step with its double.  Complex64 comparisons only.

A *spec* is a tape as plain data, ``[(name, wires, angle indices, constant)]``, with the angles numbered in tape
order -- the order in which ``LoweredTape`` numbers its slots, so index k here is slot k there.
``oracle_tape(spec, theta)`` is the tape in the oracle's vocabulary; the GPU test builds the same tape from
``qml_essentials_amd.operations``.  An angle that reaches a gate through arithmetic is not the reference's
business: it differentiates with respect to the angle each gate receives, per gate occurrence (``chain_rule``
folds such a gradient onto the arguments).
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import einsum_sim as OE
from oracle import gates as G
from tests.test_gpu_adjoint_pauli import hermitian, state_cost

SQ2 = np.sqrt(2.0)
TWO_TERM = ((np.pi / 2, 0.5), (-np.pi / 2, -0.5))
FOUR_TERM = ((np.pi / 2, (SQ2 + 1) / (4 * SQ2)), (-np.pi / 2, -(SQ2 + 1) / (4 * SQ2)),
             (3 * np.pi / 2, -(SQ2 - 1) / (4 * SQ2)), (-3 * np.pi / 2, (SQ2 - 1) / (4 * SQ2)))
RULES = {"RX": TWO_TERM, "RY": TWO_TERM, "RZ": TWO_TERM, "Rot": TWO_TERM, "RXX": TWO_TERM, "RYY": TWO_TERM,
         "RZZ": TWO_TERM, "RZX": TWO_TERM, "CPhase": TWO_TERM, "CRX": FOUR_TERM, "CRY": FOUR_TERM,
         "CRZ": FOUR_TERM}


# ---- specs ---------------------------------------------------------------------------------------------------
class Spec(list):
    """``add(name, wires, n_angles, constant)``: the gate's angles get the next indices"""
    n_theta = 0

    def add(self, name, wires, n_angles=0, const=None):
        idx = tuple(range(self.n_theta, self.n_theta + n_angles))
        self.n_theta += n_angles
        self.append((name, [int(w) for w in wires], idx, const))
        return idx


def oracle_tape(spec, theta):
    tape = []
    for name, wires, idx, const in spec:
        if name == "Matrix":
            tape.append(("Matrix", wires, (const,)))
        elif name == "Golomb":
            tape.append(("DiagU", wires, (G.golomb_diag(theta[idx[0]], len(wires)),)))
        else:
            tape.append((name, wires, tuple(theta[i] for i in idx)))
    return tape


def golomb_step(spec, k, h=5e-4):
    """The difference quotient's step for angle k: ``h`` over the highest frequency of its Golomb gate"""
    (wires,) = [w for name, w, idx, _ in spec if k in idx and name == "Golomb"]
    return h / G.golomb_ruler(2 ** len(wires))[-1]


# ---- forward simulation, resumable ---------------------------------------------------------------------------
def _apply_1q(v, u):
    """u (2x2) on the middle axis of v [A, 2, B] (contiguous) as one matrix product"""
    a, _, b = v.shape
    if b >= 16:
        return np.matmul(u, v)
    return (v.reshape(a, 2 * b) @ np.kron(u, np.eye(b)).T).reshape(a, 2, b)


def apply_gate(psi, entry, n, inplace=False):
    """One gate of the oracle's vocabulary on a flat state of 2^n amplitudes, the product ``simulate_pure`` forms
    with einsum (the CPU test holds the two against each other), several times faster at 16 qubits: the oracle's
    matrix (``G.matrix``) as a matrix product along the wire's axis for a 1-wire gate, the same on the half of the
    state whose first wire is 1 where the 4x4 matrix reads [[1, 0], [0, u]], else row by row on slices of the
    state, zero entries skipped.  Diagonals and gates on the whole register take the oracle's einsum itself.
    ``inplace``: ``psi`` may be overwritten (a private intermediate state)."""
    name, wires, params = entry
    k = len(wires)
    m = G.matrix(name, params).astype(np.complex128)
    if k >= n or name == "DiagU":
        return np.einsum(OE.einsum_subscript(n, k, tuple(wires)), m.reshape((2,) * (2 * k)),
                         psi.reshape((2,) * n)).reshape(-1)
    if k == 1:
        w = wires[0]
        return _apply_1q(psi.reshape(2 ** w, 2, 2 ** (n - 1 - w)), m).reshape(-1)
    order = sorted(wires)  # the state as [.., wire, .., wire, ..]: one axis per gate wire, the rest merged
    shape, at = [], 0
    for w in order:
        shape += [2 ** (w - at), 2]
        at = w + 1
    view = psi.reshape(shape + [2 ** (n - at)])
    if k == 2 and np.array_equal(m[:2, :2], np.eye(2)) and not m[:2, 2:].any() and not m[2:, :2].any():
        c_axis, t_axis = (1, 3) if wires[0] < wires[1] else (3, 1)
        out = view if inplace else view.copy()
        half = np.moveaxis(view, c_axis, 0)[1]                       # [.., target, ..]: 4 axes, target now at
        t_at = t_axis - 1 if t_axis > c_axis else t_axis             # this position
        sub = np.ascontiguousarray(half)
        lead = int(np.prod(sub.shape[:t_at]))
        res = _apply_1q(sub.reshape(lead, 2, -1), m[2:, 2:]).reshape(sub.shape)
        np.moveaxis(out, c_axis, 0)[1] = res
        return out.reshape(-1)

    def part(i):
        idx = [slice(None)] * (2 * k + 1)
        for j, w in enumerate(wires):
            idx[2 * order.index(w) + 1] = (i >> (k - 1 - j)) & 1
        return tuple(idx)

    out = np.empty_like(view)
    for o in range(2 ** k):
        acc = None
        for i in np.flatnonzero(m[o]):
            term = view[part(i)] if m[o, i] == 1 else m[o, i] * view[part(i)]
            acc = term if acc is None else acc + term
        out[part(o)] = 0 if acc is None else acc
    return out.reshape(-1)


def zero_state(n):
    psi = np.zeros(2 ** n, dtype=np.complex128)
    psi[0] = 1.0
    return psi


def run_from(psi, tape, n, inplace=False):
    for entry in tape:
        psi, inplace = apply_gate(psi, entry, n, inplace), True
    return psi


# ---- the gradient --------------------------------------------------------------------------------------------
def holder(tape_fn, theta, k):
    """(index of the one gate whose parameters move with angle k, its name)"""
    bumped = np.array(theta, dtype=np.float64)
    bumped[k] += 1.0
    a, b = tape_fn(np.asarray(theta, dtype=np.float64)), tape_fn(bumped)
    moved = [g for g, (x, y) in enumerate(zip(a, b))
             if any(not np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(x[2], y[2]))]
    assert len(moved) == 1, ("angle", k, "is held by gates", moved)
    return moved[0], a[moved[0]][0]


def central_difference(f, h):
    """4th-order central difference of ``f`` at 0"""
    return (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)


def reference_gradient(tape_fn, theta, n, cost, which=None, steps=None):
    """dC/dtheta[k] for k in ``which`` (default: every angle) -> array [len(theta), ...], zero elsewhere.
    ``tape_fn(theta)``: the oracle tape; ``cost(psi)``: a float or an array (one column per observable: a
    Jacobian from the same simulations) of the final state (2^n amplitudes).  ``steps[k]``: difference-quotient
    step of an angle that sits in a DiagU gate (the Golomb encoding); every other gate has a shift rule.  The
    state in front of the gate that holds the angle is computed once and shared by the gate's shifts."""
    theta = np.asarray(theta, dtype=np.float64)
    which = range(theta.size) if which is None else which
    tape = tape_fn(theta)
    by_gate = {}
    for k in which:
        g, name = holder(tape_fn, theta, k)
        by_gate.setdefault(g, []).append((k, name))
    out, psi, at = None, zero_state(n), 0
    for g in sorted(by_gate):
        psi = run_from(psi, tape[at:g], n)
        at = g
        for k, name in by_gate[g]:
            def shifted(s, k=k):
                t = theta.copy()
                t[k] += s
                return np.asarray(cost(run_from(apply_gate(psi, tape_fn(t)[g], n), tape[g + 1:], n, True)))

            if name == "DiagU":
                d = central_difference(shifted, steps[k])
            else:
                d = sum(c * shifted(s) for s, c in RULES[name])
            if out is None:
                out = np.zeros((theta.size,) + np.shape(d))
            out[k] = d
    return out


def difference_gradient(tape_fn, theta, n, cost, k, h):
    """dC/dtheta[k] by the 4th-order central difference with step h, whatever gate holds the angle"""
    theta = np.asarray(theta, dtype=np.float64)

    def f(s):
        t = theta.copy()
        t[k] += s
        return np.asarray(cost(run_from(zero_state(n), tape_fn(t), n)))

    return central_difference(f, h)


def chain_rule(grad, tangents, n_args):
    """Fold a per-angle gradient [n_angles] onto arguments: ``tangents[k] = [(argument index, d angle_k / d
    argument)]`` for an angle that reaches its gate through arithmetic (``th[6] * x``: [(6, x)])."""
    out = np.zeros(n_args)
    for k, terms in tangents.items():
        for a, c in terms:
            out[a] += c * grad[k]
    return out


def chain_case():
    """Three gates whose angles are th[0] * x, th[1] + x and th[0] again: (spec, x, th, angles(th), tangents)"""
    rng = np.random.default_rng(8)
    spec = Spec()
    mix(spec, 3, rng)
    spec.add("RX", [0], 1); spec.add("CRY", [0, 2], 1); spec.add("RZZ", [1, 2], 1); spec.add("CX", [2, 1])
    mix(spec, 3, rng)
    x, th = 0.7, np.array([1.3, 2.1])
    return spec, x, th, (lambda a: np.array([a[0] * x, a[1] + x, a[0]])), {0: [(0, x)], 1: [(1, 1.0)], 2: [(0, 1.0)]}


# ---- observables ---------------------------------------------------------------------------------------------
def z_groups(n):
    """Z on wire 0, Z on wire n - 1 and one 3-wire parity, as far as the register has the wires"""
    if n == 1:
        return [[0]]
    if n == 2:
        return [[0], [1], [0, 1]]
    return [[0], [n - 1], [0, n // 2, n - 1]] if n > 3 else [[0], [2], [0, 1, 2]]


def z_mats(groups):
    return [(G.pauli_word("Z" * len(g)), list(g)) for g in groups]


def pauli_mats(n, rng):
    """The matrices of ``test_gpu_adjoint_pauli.observables(n, rng)`` -- X(0), Y(n // 2), a Hermitian on wires
    [n // 5, 3 n // 5], Z(n - 1), X0 Y1 Z2 -- drawn from ``rng`` as that function draws them"""
    hw = sorted({n // 5, (3 * n) // 5})
    mats = [(G.X, [0]), (G.Y, [n // 2]), (hermitian(rng, len(hw)), hw), (G.Z, [n - 1])]
    if n >= 3:
        mats.append((G.pauli_word("XYZ"), [0, 1, 2]))
    elif n == 2:
        mats.append((G.pauli_word("XY"), [0, 1]))
    return mats


def expectations(psi, n, mats):
    """[<psi| M_k |psi>] with ``test_gpu_adjoint_pauli.state_cost`` (np.tensordot), one observable at a time"""
    return np.array([state_cost(psi, n, [m], [1.0]) for m in mats])


# ---- gate sets -----------------------------------------------------------------------------------------------
def unitary(rng, k):
    q, r = np.linalg.qr(rng.standard_normal((2 ** k, 2 ** k)) + 1j * rng.standard_normal((2 ** k, 2 ** k)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def mix(spec, n, rng, wires=None):
    """an arbitrary 2x2 unitary per wire: no angle, so not differentiated; it keeps every later generator away
    from the axes of the state it acts on (a product state's RZ has no gradient)"""
    for q in (range(n) if wires is None else wires):
        spec.add("Matrix", [q], 0, unitary(rng, 1))


def everything(n, rng, dense2=False, dense4=None, golomb=False):
    """Every differentiated gate kind as far as n wires allow, fixed gates in between.  ``dense2``: an explicit
    2-wire matrix (a dense group in the forward plan); ``dense4``: wires of one 16x16 unitary; ``golomb``: the
    Golomb encoding on three wires."""
    s, last = Spec(), n - 1
    mix(s, n, rng)
    for q in sorted({0, n // 2, last}):
        s.add("RX", [q], 1); s.add("RY", [q], 1); s.add("RZ", [q], 1)
    s.add("H", [0]); s.add("Rot", [last], 3); s.add("S", [n // 2])
    if n >= 2:
        s.add("CRX", [0, last], 1); s.add("CX", [last, 0]); s.add("CRY", [last, 0], 1); s.add("PauliX", [0])
        s.add("CRZ", [0, 1], 1); s.add("CY", [0, last]); s.add("CPhase", [last, n // 2 if n > 2 else 0], 1)
        s.add("PauliY", [last]); s.add("RXX", [0, last], 1); s.add("CZ", [last, 0]); s.add("RYY", [last, 0], 1)
        s.add("PauliZ", [0]); s.add("RZZ", [0, 1], 1); s.add("SWAP", [0, last]); s.add("RZX", [last, 0], 1)
        if dense2:
            s.add("Matrix", [last, 0], 0, unitary(rng, 2))
        mix(s, n, rng, [0, last])
    if golomb:  # (three wires: marks up to 44 -- see the cases below)
        s.add("Golomb", [last, 0, n // 2], 1)
    if n >= 3:
        mid = n // 2 if n // 2 not in (0, last) else 1
        s.add("CCX", [0, mid, last]); s.add("CRX", [last, mid], 1); s.add("RZX", [mid, last], 1)
        s.add("CPhase", [mid, last], 1); s.add("RYY", [mid, 0], 1); s.add("CRY", [mid, last], 1)
        if dense4 is not None:
            s.add("Matrix", dense4, 0, unitary(rng, 4))
            # generators on position 0 (wire n - 1) and controlled from it, behind the 4-wire operator
            s.add("RX", [last], 1); s.add("CRZ", [last, mid], 1); s.add("RZZ", [mid, last], 1)
            s.add("CRX", [last, 0], 1); s.add("RXX", [last, mid], 1); s.add("CPhase", [0, last], 1)
    for q in range(n - 1):
        s.add("CX", [q, q + 1])
    mix(s, n, rng)
    return s


def deep_layers(n, rng, layers):
    """RX on every wire, then a CX ring, ``layers`` times: 2 n operators per layer that no compiler merges"""
    s = Spec()
    for _ in range(layers):
        for q in range(n):
            s.add("RX", [q], 1)
        for q in range(n):
            s.add("CX", [q, (q + 1) % n])
    mix(s, n, rng)
    return s


def position_classes(n):
    """wires whose bit positions (wire w = position n - 1 - w) are in 0-3, 4-11, >= 12: two wires of each"""
    w = lambda p: n - 1 - p  # noqa: E731
    return [[w(0), w(3)], [w(4), w(11)], [w(12), w(n - 1)]]


def tile_tape(n, rng, wide=False, golomb3=False):
    """1-qubit and singly-controlled 1-qubit gates only -- what the fused ``k_tile_adj`` passes take.  One gate
    of each of CRX, CRY, CRZ, CPhase (differentiated) and CX, CY, CZ on every control class x target class of
    ``position_classes``; RX / RY / RZ / Rot on wire 0, a middle wire and wire n - 1; H, S, Paulis and arbitrary
    2x2 matrices in between.  ``wide``: RXX, RYY, RZZ, RZX on pairs with position 0 and a position >= 12, a
    SWAP, a CCX and a 2-wire matrix, for the streaming sweep; ``golomb3``: the Golomb encoding on three wires."""
    s, last, cls = Spec(), n - 1, position_classes(n)
    mix(s, n, rng)
    fixed = ["H", "S", "PauliX", "PauliY", "PauliZ", "Matrix", "Matrix"]
    rot = [(kind, q) for q in (0, n // 2, last) for kind in ("RX", "RY", "RZ", "Rot")]
    for ci, cw in enumerate(cls):
        for ti, tw in enumerate(cls):
            for j, kind in enumerate(("CRX", "CRY", "CRZ", "CPhase", "CX", "CY", "CZ")):
                s.add(kind, [cw[j % 2], tw[(j + 1) % 2]], 1 if j < 4 else 0)
            block = 3 * ci + ti
            if block < len(fixed):  # an undifferentiated neighbour behind the block, on its last target
                s.add(fixed[block], [tw[1]], 0, unitary(rng, 1) if fixed[block] == "Matrix" else None)
            for kind, q in rot[block::9]:
                s.add(kind, [q], 3 if kind == "Rot" else 1)
    if wide:
        s.add("RXX", [last, 0], 1); s.add("RYY", [1, last], 1); s.add("SWAP", [0, last])
        s.add("RZZ", [last, 1], 1); s.add("RZX", [0, last], 1); s.add("CCX", [0, last, n // 2])
        s.add("RZX", [last, 1], 1); s.add("Matrix", [last, 0], 0, unitary(rng, 2)); s.add("RYY", [last, n // 2], 1)
        if golomb3:
            s.add("Golomb", [last, 0, n // 2], 1)
    # every wire a gate above acts on reaches an observed wire, and no observable commutes with the last gates
    seen = [0, n // 2, last]
    mix(s, n, rng, sorted({w for c in cls for w in c} - set(seen)))
    for j, u in enumerate(sorted({w for c in cls for w in c} - set(seen))):
        s.add("CX", [u, seen[j % 3]])
    mix(s, n, rng, sorted(set(seen + [1, 2, n // 5, (3 * n) // 5])))
    return s


def threshold_tape(n, rng):
    """ten gates, four differentiated angles, on positions 0 and n - 1, with one CRY and one RZZ"""
    s, last = Spec(), n - 1
    mix(s, n, rng, [0, last])
    s.add("RX", [last], 1); s.add("CRY", [0, last], 1)
    s.add("Matrix", [0], 0, unitary(rng, 1))
    s.add("RZZ", [last, 0], 1)
    s.add("CX", [last, 0])
    s.add("RY", [0], 1)
    s.add("CX", [0, last])
    mix(s, n, rng, [last])
    return s


# ---- cases ---------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name n spec theta wanted seed golomb wseed")
# ``theta`` [B, n_theta]; ``wanted``: the differentiated angle indices; ``seed`` draws the observables and weights


# Seeds under which no differentiated angle of a case has a gradient below 1e-3 in any row, for either seed of the
# sweep (tests/test_adjoint_reference_cpu.py holds every case to that): CASE_SEEDS draws the matrices and angles,
# WEIGHT_SEEDS the weight rows.  Cases that are not listed use 0.
CASE_SEEDS = {"tile_n14": 2, "tile_n16": 1}
WEIGHT_SEEDS = {"lds_all_n7": 2, "lds_all_n8": 8, "lds_all_n13": 2, "lds_dense_n4": 1, "lds_dense_n13": 5,
                "lds_golomb_n5": 3, "lds_deep_n13": 40, "lds_32_parities_n6": 6, "mat4_n4": 2, "mat4_n6": 10,
                "tile_n14": 1, "tile_third_n14": 1, "tile_n16": 389, "tile_third_n16": 389,
                "wide_golomb_n14": 256, "wide_n15": 310}


def golomb_angles(spec):
    return [idx[0] for name, _w, idx, _c in spec if name == "Golomb"]


def _case(name, n, build, B=3, wanted=None, angles=(0.4, 5.9), **kw):
    seed = CASE_SEEDS.get(name, 0)
    rng = np.random.default_rng([seed, n, sum(map(ord, name))])  # (the name: cases of one size differ)
    spec = build(n, rng, **kw)
    theta = rng.uniform(*angles, (B, spec.n_theta))
    # a Golomb angle stays below 0.03: its phases marks * x are rounded to an ulp of their size, and the
    # difference quotient divides that by a step of 1e-6
    theta[:, golomb_angles(spec)] *= 0.005
    golomb = bool(golomb_angles(spec))
    wanted = list(range(spec.n_theta)) if wanted is None else [k for k in wanted(spec.n_theta)]
    return Case(name, n, spec, theta, wanted, seed, golomb, WEIGHT_SEEDS.get(name, 0))


def _spread(n_theta, count=21):
    """about ``count`` angles spread over the first, middle and last layers"""
    third = count // 3
    mid = n_theta // 2
    return sorted(set(list(range(0, 2 * third, 2)) + list(range(mid - third, mid + third, 2))
                      + list(range(n_theta - 2 * third, n_theta, 2))))


@functools.lru_cache(maxsize=None)
def cases():
    out = {}

    def add(c):
        out[c.name] = c

    for n in (1, 2, 3, 7, 8, 13):
        add(_case(f"lds_all_n{n}", n, everything))
    for n in (4, 13):
        add(_case(f"lds_dense_n{n}", n, everything, dense2=True))
    # The Golomb encoding on three of the five wires, as a diagonal of the whole register.  On all five the marks
    # reach 1522 and the gradient a few hundred; its float32 rounding (2^-24 of that, per operation) is then
    # several times the absolute tolerance of 4e-6 -- measured on the MI355X: 4.9e-5 -- whatever the kernel does.
    add(_case("lds_golomb_n5", 5, everything, golomb=True))
    # (small angles: 26 layers of arbitrary ones scramble the state until no gradient is left to compare)
    add(_case("lds_deep_n13", 13, deep_layers, layers=26, wanted=_spread, angles=(0.05, 0.3)))
    add(_case("lds_32_parities_n6", 6, everything))
    add(_case("mat4_n4", 4, everything, dense4=[2, 0, 3, 1]))
    add(_case("mat4_n6", 6, everything, dense4=[4, 1, 5, 2]))
    for n in (14, 16):
        add(_case(f"tile_n{n}", n, tile_tape))
        add(out[f"tile_n{n}"]._replace(name=f"tile_third_n{n}", wanted=out[f"tile_n{n}"].wanted[::3],
                                        wseed=WEIGHT_SEEDS.get(f"tile_third_n{n}", 0)))
    add(_case("wide_golomb_n14", 14, tile_tape, wide=True, golomb3=True))
    add(_case("wide_n15", 15, tile_tape, wide=True))
    for n in (18, 19, 20):
        add(_case(f"threshold_n{n}", n, threshold_tape, B=1))
    return out


def parities_32(n=6):
    groups = [[q] for q in range(n)] + [[a, b] for a in range(n) for b in range(a + 1, n)] \
        + [[a, b, c] for a in range(n) for b in range(a + 1, n) for c in range(b + 1, n)]
    return groups[:32]


def case_observables(case):
    """(Z-parity wire groups, Pauli-seed matrices [(matrix, wires)], Z weights [B, nz], Pauli weights [B, np]): a
    different weight row per sample"""
    rng = np.random.default_rng([case.seed, case.n, 77, case.wseed])
    groups = parities_32(case.n) if case.name.startswith("lds_32_parities") else z_groups(case.n)
    mats = pauli_mats(case.n, np.random.default_rng([case.seed, case.n, 78]))
    B = case.theta.shape[0]
    sign = lambda shape: rng.choice([-1.0, 1.0], shape)  # noqa: E731
    wz = sign((B, len(groups))) * rng.uniform(0.5, 1.5, (B, len(groups)))
    wp = sign((B, len(mats))) * rng.uniform(0.5, 1.5, (B, len(mats)))
    return groups, mats, wz, wp


@functools.lru_cache(maxsize=None)
def case_jacobians(name):
    """d<O_k>/dtheta for the case's Z groups and Pauli-seed matrices together: [B, n_theta, nz + np], computed
    once per case (tapes that share a spec and angles share it too) and never written to"""
    case = cases()[name]
    if name.startswith("tile_third_"):
        return case_jacobians(name.replace("tile_third_", "tile_"))
    groups, mats, _, _ = case_observables(case)
    every = z_mats(groups) + mats
    steps = {k: golomb_step(case.spec, k) for k in golomb_angles(case.spec)}
    jac = np.stack([reference_gradient(lambda t: oracle_tape(case.spec, t), row, case.n,
                                       lambda psi: expectations(psi, case.n, every), case.wanted, steps)
                    for row in case.theta])
    jac.setflags(write=False)
    return jac


def case_gradients(name):
    """(dC_z/dtheta, dC_pauli/dtheta), each [B, n_theta], zero outside ``wanted``"""
    case = cases()[name]
    groups, _mats, wz, wp = case_observables(case)
    jac = case_jacobians(name)
    keep = np.zeros(case.spec.n_theta)
    keep[case.wanted] = 1.0
    nz = len(groups)
    return (np.einsum("bk,btk->bt", wz, jac[:, :, :nz]) * keep, np.einsum("bk,btk->bt", wp, jac[:, :, nz:]) * keep)
