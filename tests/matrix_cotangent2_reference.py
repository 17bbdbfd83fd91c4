"""An exact complex128 reference for the matrix cotangents of TWO-WIRE matrix gates, and the mixed cases their GPU
tests run.  The one-wire file, tests/matrix_cotangent_reference.py, states the argument; here the gate sits on wires
``(w0, w1)`` and its matrix is written with row = 2 * value of w0 + value of w1, so

    G_ref[a][c] = <psi| H |chi_ac>,   chi_ac = the final state with the gate replaced by |a><c| (a 4x4 unit),

made of forward simulations alone (``tests/adjoint_reference.py``).  ``adjoint_style2`` forms the same matrix the way
the sweep does -- the moment ``M[a][c] = sum_rest conj(lambda[a, rest]) psi[c, rest]`` BEHIND the gate, then
``G = M (U^+)^T`` -- and the named wrong variants of it.

Every case is a MIXED tape: a per-sample one-wire matrix, a constant two-wire matrix, a per-sample two-wire matrix and
angle gates, so one sweep reports blocks of 8 and of 32 scalars in one row.
"""
import functools
from collections import namedtuple

import numpy as np

from tests import adjoint_reference as R
from tests import matrix_cotangent_reference as M1

G = R.G
tape_of, apply_h, cost_of = M1.tape_of, M1.apply_h, M1.cost_of
case_observables, seed_observables = M1.case_observables, M1.seed_observables


def reference_cotangent(tape, g, n, mats, w):
    """G_ref [d, d] of the matrix gate at position g of ``tape``, d = 2 or 4 (forward simulations only)"""
    name, wires, _ = tape[g]
    assert name == "Matrix" and len(wires) in (1, 2)
    d = 2 ** len(wires)
    front = R.run_from(R.zero_state(n), tape[:g], n)
    psi = R.run_from(R.apply_gate(front, tape[g], n), tape[g + 1:], n, True)
    hpsi = apply_h(psi, n, mats, w)
    out = np.zeros((d, d), dtype=np.complex128)
    for a in range(d):
        for c in range(d):
            e = np.zeros((d, d), dtype=np.complex128)
            e[a, c] = 1.0
            chi = R.run_from(R.apply_gate(front, ("Matrix", wires, (e,)), n), tape[g + 1:], n, True)
            out[a, c] = np.vdot(hpsi, chi)
    return out


def moment2(lam, psi, n, w0, w1):
    """M[2 a0 + a1][2 c0 + c1] = sum_rest conj(lam[a0 a1, rest]) psi[c0 c1, rest]; wire q is axis q of the state"""
    lv = np.moveaxis(np.asarray(lam).reshape((2,) * n), (w0, w1), (0, 1)).reshape(4, -1)
    pv = np.moveaxis(np.asarray(psi).reshape((2,) * n), (w0, w1), (0, 1)).reshape(4, -1)
    return lv.conj() @ pv.T


def adjoint_style2(tape, g, n, mats, w):
    """The sweep's own computation for the two-wire gate at g, and its named wrong variants -> dict name -> [4, 4]"""
    w0, w1 = tape[g][1]
    u = np.asarray(tape[g][2][0], dtype=np.complex128)
    ud = u.conj().T
    front = R.run_from(R.zero_state(n), tape[:g], n)
    behind = R.apply_gate(front, tape[g], n)
    psi = R.run_from(behind, tape[g + 1:], n)
    lam = apply_h(psi, n, mats, w)
    for name, wires, params in reversed(tape[g + 1:]):
        lam = R.apply_gate(lam, ("Matrix", wires, (G.matrix(name, params).astype(np.complex128).conj().T,)), n)
    m = moment2(lam, behind, n, w0, w1)
    right = m @ ud.T
    return {"right": right,
            "wires exchanged": moment2(lam, behind, n, w1, w0) @ ud.T,
            "G transposed": right.T.copy(),
            "(U^+)^T missing": m,
            "U in place of U^+": m @ u.T}


# ---- tapes ---------------------------------------------------------------------------------------------------------
def mixed_tape(n, rng, B, pairs, dense4=None):
    """RX / RY / RZ in front; per wire pair alternately a per-sample and a constant two-wire matrix, each behind a
    one-wire matrix on its first wire (per-sample when the two-wire one is constant and the other way round, plus a
    per-sample one in front of the first pair) and followed by a CRZ across the pair and an RY; a CX chain behind.
    -> (spec, spec positions of the matrix gates whose cotangent is asked for)"""
    s, mats = R.Spec(), []
    R.mix(s, n, rng)
    for q in sorted({0, n // 2, n - 1}):
        s.add("RX", [q], 1); s.add("RY", [q], 1); s.add("RZ", [q], 1)
    for j, (w0, w1) in enumerate(pairs):
        per_sample = j % 2 == 0
        mats.append(len(s))
        s.add("Matrix", [w0], 0, R.unitary(rng, 1) if per_sample and j else np.stack([R.unitary(rng, 1) for _ in range(B)]))
        mats.append(len(s))
        s.add("Matrix", [w0, w1], 0, np.stack([R.unitary(rng, 2) for _ in range(B)]) if per_sample else R.unitary(rng, 2))
        s.add("CRZ", [w1, w0], 1)
        s.add("RY", [w1], 1)
        if dense4 is not None and j == 0:
            s.add("Matrix", dense4, 0, R.unitary(rng, 4))
    for q in range(n - 1):
        s.add("CX", [q, q + 1])
    R.mix(s, n, rng)
    return s, mats


Case = M1.Case
SEEDS = {}  # per case: the seed that draws matrices and angles (0 unless the CPU test needed another)


def _case(name, n, B, pairs, **kw):
    seed = SEEDS.get(name, 0)
    rng = np.random.default_rng([seed, n, sum(map(ord, name))])
    spec, mats = mixed_tape(n, rng, B, pairs, **kw)
    theta = rng.uniform(0.4, 5.9, (B, spec.n_theta))
    return Case(name, n, spec, theta, list(range(spec.n_theta)), mats, seed)


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    out["lds_n2"] = _case("lds_n2", 2, 3, [(0, 1), (1, 0)])                 # no other wires
    out["lds_n6"] = _case("lds_n6", 6, 2, [(0, 5), (5, 0), (2, 3)])
    out["lds_n12"] = _case("lds_n12", 12, 2, [(0, 11), (6, 5)])              # the workgroup has all its waves
    out["stream_n5"] = _case("stream_n5", 5, 2, [(0, 4), (2, 1)], dense4=[3, 0, 4, 1])
    # wire q is bit position n - 1 - q: positions (0, 1), (13, 0), (6, 7)
    out["stream_n14"] = _case("stream_n14", 14, 2, [(13, 12), (0, 13), (7, 6)])
    out["x64_n3"] = _case("x64_n3", 3, 2, [(2, 0), (1, 2)])
    return out


@functools.lru_cache(maxsize=None)
def case_reference(name, seed):
    """(angle gradients [B, n_theta], [G_ref [B, d, d] per asked matrix gate]) under the Z or the Pauli seed; computed
    once, never written to"""
    case = cases()[name]
    mats, w = seed_observables(case, seed)
    B = case.theta.shape[0]
    grad = np.zeros((B, case.spec.n_theta))
    cot = [np.zeros((B,) + (2 ** len(case.spec[g][1]),) * 2, dtype=np.complex128) for g in case.mats]
    for b in range(B):
        tape_fn = lambda t, b=b: tape_of(case.spec, t, b)  # noqa: E731
        cost = lambda psi, b=b: cost_of(psi, case.n, mats, w[b])  # noqa: E731
        grad[b] = R.reference_gradient(tape_fn, case.theta[b], case.n, cost, case.wanted)
        tape = tape_fn(case.theta[b])
        for k, g in enumerate(case.mats):
            cot[k][b] = reference_cotangent(tape, g, case.n, mats, w[b])
    grad.setflags(write=False)
    for c in cot:
        c.setflags(write=False)
    return grad, tuple(cot)
