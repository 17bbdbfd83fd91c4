"""An exact complex128 reference for the MATRIX COTANGENTS of the adjoint sweep, and the cases its GPU tests run.

The cost ``C = sum_k w_k <psi| O_k |psi>`` and a one-wire matrix gate ``U`` at position g of the tape, on wire q.  The
final state is LINEAR in the entries of ``U``: with ``chi_ac`` the final state of the tape whose gate g is replaced
by ``|a><c|``, ``psi = sum_ac U[a][c] chi_ac``.  So for any parameter of ``U``

    dC/dtheta = 2 Re <psi| H |dpsi/dtheta> = 2 Re sum_ac G_ref[a][c] dU[a][c]/dtheta,   G_ref[a][c] = <psi| H |chi_ac>

with ``H = sum_k w_k O_k`` -- exact, no difference quotient, and made of forward simulations alone: the oracle's gate
matrices (``oracle/gates.py``) through ``tests/adjoint_reference.py``'s sliced products, which
``tests/test_adjoint_reference_cpu.py`` holds against ``oracle/einsum_sim.py``.  Nothing here reverses a tape.
``G_ref[a][c]`` is the quantity the sweep defines as ``sum_rest conj(lambda_k[a, rest]) phi_k[c, rest]`` (lambda with
every later gate undone, phi the state in front of the gate): ``<psi| H V |a><c| phi> = <V^+ H psi | a><c| phi>``.

``adjoint_style`` computes the same matrix the way the sweep does (lambda pulled back through daggered gates) only to
form the named WRONG variants of it, which the CPU test tells apart from ``G_ref`` on every case.

A spec is that of ``tests/adjoint_reference.py``; a ``Matrix`` entry whose constant has shape ``[B, 2, 2]`` is a
per-sample matrix (``MAT1_ROW`` on the engine), one of shape ``[2, 2]`` a constant (``MAT1``).  ``case.mats`` lists
the spec positions of the gates whose cotangent is asked for, in tape order.
"""
import functools
from collections import namedtuple

import numpy as np

from tests import adjoint_reference as R

G = R.G


def tape_of(spec, theta, b):
    """the oracle tape of batch row b: per-sample matrices take their row"""
    out = []
    for name, wires, idx, const in spec:
        if name == "Matrix":
            const = np.asarray(const)
            out.append(("Matrix", wires, (const[b] if const.ndim == 3 else const,)))
        else:
            out.append((name, wires, tuple(theta[i] for i in idx)))
    return out


def apply_h(psi, n, mats, w):
    """H psi = sum_k w_k O_k psi, each observable as a (non-unitary) matrix gate of the forward simulation"""
    out = np.zeros_like(psi)
    for wk, (m, wires) in zip(w, mats):
        out = out + wk * R.apply_gate(psi, ("Matrix", list(wires), (np.asarray(m, dtype=np.complex128),)), n)
    return out


def cost_of(psi, n, mats, w):
    return float(np.real(np.vdot(psi, apply_h(psi, n, mats, w))))


def reference_cotangent(tape, g, n, mats, w):
    """G_ref [2, 2] of the one-wire matrix gate at position g of ``tape`` (forward simulations only)"""
    name, wires, _ = tape[g]
    assert name == "Matrix" and len(wires) == 1
    front = R.run_from(R.zero_state(n), tape[:g], n)
    psi = R.run_from(R.apply_gate(front, tape[g], n), tape[g + 1:], n, True)
    hpsi = apply_h(psi, n, mats, w)
    out = np.zeros((2, 2), dtype=np.complex128)
    for a in range(2):
        for c in range(2):
            e = np.zeros((2, 2), dtype=np.complex128)
            e[a, c] = 1.0
            chi = R.run_from(R.apply_gate(front, ("Matrix", wires, (e,)), n), tape[g + 1:], n, True)
            out[a, c] = np.vdot(hpsi, chi)
    return out


def replaced(tape, g, u):
    return tape[:g] + [("Matrix", tape[g][1], (u,))] + tape[g + 1:]


def moment(lam, phi, n, wire):
    """M[a][c] = sum_rest conj(lam[a, rest]) phi[c, rest] over the other wires"""
    lv = lam.reshape(2 ** wire, 2, -1)
    pv = phi.reshape(2 ** wire, 2, -1)
    return np.einsum("xay,xcy->ac", lv.conj(), pv)


def adjoint_style(tape, g, n, mats, w):
    """The same matrix as the sweep forms it, and the named wrong variants of it -> dict name -> [2, 2]."""
    wire = tape[g][1][0]
    u = np.asarray(tape[g][2][0], dtype=np.complex128)
    front = R.run_from(R.zero_state(n), tape[:g], n)
    behind = R.apply_gate(front, tape[g], n)
    psi = R.run_from(behind, tape[g + 1:], n)
    lam = apply_h(psi, n, mats, w)
    for name, wires, params in reversed(tape[g + 1:]):
        lam = R.apply_gate(lam, ("Matrix", wires, (G.matrix(name, params).astype(np.complex128).conj().T,)), n)
    lam_front = R.apply_gate(lam, ("Matrix", [wire], (u.conj().T,)), n)
    right = moment(lam, front, n, wire)
    return {"right": right, "transposed": right.T.copy(), "conjugated": right.conj(),
            "psi behind the gate": moment(lam, behind, n, wire),
            "lambda in front of the gate": moment(lam_front, front, n, wire),
            "factor 1 instead of 2": 0.5 * right,
            "wire order reversed": moment(lam, front, n, n - 1 - wire)}


# ---- tapes ---------------------------------------------------------------------------------------------------------
def matrix_tape(n, rng, B, mat_wires, dense4=None, layers=0):
    """One-wire matrix gates on ``mat_wires`` (a wire may come twice), alternately per-sample and constant, each
    followed by CRX / CPhase / CX with a neighbour and an RY; RX / RY / RZ in front, a CX chain behind.  ``dense4``:
    wires of a 16x16 unitary in the middle (keeps the sweep out of the LDS kernel); ``layers``: that many layers of
    RX on every wire and a CX ring in front (more forward operators than fit beside psi and lambda in LDS).
    -> (spec, spec positions of the matrix gates)"""
    s, mats = R.Spec(), []
    for _ in range(layers):
        for q in range(n):
            s.add("RX", [q], 1)
        for q in range(n):
            s.add("CX", [q, (q + 1) % n])
    R.mix(s, n, rng)
    for q in sorted({0, n // 2, n - 1}):
        s.add("RX", [q], 1); s.add("RY", [q], 1); s.add("RZ", [q], 1)
    for j, w in enumerate(mat_wires):
        per_sample = j % 2 == 0
        mats.append(len(s))
        s.add("Matrix", [w], 0, np.stack([R.unitary(rng, 1) for _ in range(B)]) if per_sample else R.unitary(rng, 1))
        if n >= 2:
            other = (w + 1) % n
            s.add("CRX", [other, w], 1); s.add("CPhase", [w, other], 1); s.add("CX", [w, other])
        s.add("RY", [w], 1)
        if dense4 is not None and j == len(mat_wires) // 2 - 1:
            s.add("Matrix", dense4, 0, R.unitary(rng, 4))
    for q in range(n - 1):
        s.add("CX", [q, q + 1])
    R.mix(s, n, rng)
    return s, mats


Case = namedtuple("Case", "name n spec theta wanted mats seed")
SEEDS = {}  # per case: the seed that draws matrices and angles (0 unless the CPU test needed another)


def _case(name, n, B, mat_wires, wanted=None, angles=(0.4, 5.9), **kw):
    seed = SEEDS.get(name, 0)
    rng = np.random.default_rng([seed, n, sum(map(ord, name))])
    spec, mats = matrix_tape(n, rng, B, mat_wires, **kw)
    theta = rng.uniform(*angles, (B, spec.n_theta))
    wanted = list(range(spec.n_theta)) if wanted is None else wanted(spec.n_theta)
    return Case(name, n, spec, theta, wanted, mats, seed)


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for B in (1, 3):
        out[f"lds_n2_b{B}"] = _case(f"lds_n2_b{B}", 2, B, [0, 1, 0])
        out[f"lds_n3_b{B}"] = _case(f"lds_n3_b{B}", 3, B, [0, 1, 2, 1])
        out[f"lds_n13_b{B}"] = _case(f"lds_n13_b{B}", 13, B, [0, 6, 12, 6])
    # 26 layers of 26 operators in front: more than the 658 that fit beside psi and lambda (small angles, as in
    # tests/adjoint_reference.py: arbitrary ones scramble the state until nothing is left to compare)
    out["lds_deep_n13"] = _case("lds_deep_n13", 13, 1, [12, 0], layers=26, angles=(0.05, 0.3),
                                wanted=lambda nt: sorted(set(range(0, 12, 2)) | set(range(nt - 14, nt))))
    out["stream_n5"] = _case("stream_n5", 5, 2, [0, 4, 2, 4], dense4=[3, 0, 4, 1])
    out["stream_n14"] = _case("stream_n14", 14, 2, [0, 7, 13, 7])
    return out


def case_observables(case):
    """(Z-parity wire groups, Pauli-seed matrices, Z weights [B, nz], Pauli weights [B, np]) as the angle cases draw
    them"""
    rng = np.random.default_rng([case.seed, case.n, 79])
    groups = R.z_groups(case.n)
    mats = R.pauli_mats(case.n, np.random.default_rng([case.seed, case.n, 78]))
    B = case.theta.shape[0]
    sign = lambda shape: rng.choice([-1.0, 1.0], shape)  # noqa: E731
    wz = sign((B, len(groups))) * rng.uniform(0.5, 1.5, (B, len(groups)))
    wp = sign((B, len(mats))) * rng.uniform(0.5, 1.5, (B, len(mats)))
    return groups, mats, wz, wp


def seed_observables(case, seed):
    """(matrices [(matrix, wires)], weights [B, n_obs]) of the Z seed or the Pauli seed"""
    groups, mats, wz, wp = case_observables(case)
    return (R.z_mats(groups), wz) if seed == "z" else (mats, wp)


@functools.lru_cache(maxsize=None)
def case_reference(name, seed):
    """(angle gradients [B, n_theta] -- zero outside ``wanted`` --, G_ref [B, n_mat, 2, 2]) of a case under the Z or
    the Pauli seed; computed once, never written to"""
    case = cases()[name]
    mats, w = seed_observables(case, seed)
    B = case.theta.shape[0]
    grad = np.zeros((B, case.spec.n_theta))
    cot = np.zeros((B, len(case.mats), 2, 2), dtype=np.complex128)
    for b in range(B):
        tape_fn = lambda t, b=b: tape_of(case.spec, t, b)  # noqa: E731
        cost = lambda psi, b=b: cost_of(psi, case.n, mats, w[b])  # noqa: E731
        grad[b] = R.reference_gradient(tape_fn, case.theta[b], case.n, cost, case.wanted)
        tape = tape_fn(case.theta[b])
        for k, g in enumerate(case.mats):
            cot[b, k] = reference_cotangent(tape, g, case.n, mats, w[b])
    grad.setflags(write=False)
    cot.setflags(write=False)
    return grad, cot
