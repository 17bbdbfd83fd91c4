"""NumPy complex128 reference for adjoint gradients through tapes that hold explicit matrices on three and four
wires (``qmle_wide_moment``, ``qmle_adjoint_segment``, ``adjoint.segmented_gradient``, ``Script.vjp(wide_gates=True)``),
with named wrong variants of itself and the seeded cases the tests use.

A case is a tape of ordinary gates and wide gates ``U = exp(-i t H)`` (``H`` Hermitian on 3 or 4 wires, one ``t`` per
sample), a list of observables with weights, and the cost ``C_b = sum_k w[b, k] <psi_b| O_k |psi_b>``.

With ``psi_k`` the state in FRONT of step k, ``lambda_K = (sum_k w_k O_k) psi_K`` behind the last step and
``lambda_k = U_k^+ lambda_{k+1}``, the derivative by any parameter of step k is ``2 Re <lambda_{k+1}| dU_k |psi_k>``.
For a wide gate that is ``2 Re sum_ac G[a][c] dU[a][c]`` with the cotangent BY DEFINITION

    G[a][c] = sum_rest conj(lambda_{k+1}[a, rest]) psi_k[c, rest]

-- ``conj(lambda)`` behind the gate against the state in front of it.  The engine forms the same matrix another way,
``G = M (U^+)^T`` from the moment ``M`` of the two states BEHIND the gate; nothing here takes that route.

Convention (``operations.embed_matrix``): the first wire of ``wires`` is the most significant bit of the matrix index,
wire ``w`` is axis ``w`` of the state reshaped to ``(2,) * n``.
"""
from typing import NamedTuple

import numpy as np
from scipy.linalg import expm

import wide_gate_reference as W

X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)
I2 = np.eye(2, dtype=np.complex128)
HAD = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)
CX = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=np.complex128)
P1 = np.diag([0.0, 1.0]).astype(np.complex128)
PAULI = {"X": X, "Y": Y, "Z": Z}

# what an implementation of the wide gate's share of the sweep can get wrong
VARIANTS = {
    "transposed": "G^T for G (row and column of the cotangent exchanged)",
    "unconjugated": "lambda taken without its complex conjugate",
    "reversed_wires": "the wires read least-significant first",
    "moment_for_cotangent": "the moment M of the states behind the gate returned for G (no (U^+)^T)",
    "lambda_not_propagated": "lambda not taken through the wide gate: the gates in front of it see the lambda behind it",
}


class Step(NamedTuple):
    kind: str           # "RX" "RY" "RZ" "CRZ" (one angle), "CX" "H" (none), "WIDE"
    wires: tuple
    angle: int = -1     # column of theta; for a wide gate: column of t
    H: np.ndarray = None  # a wide gate's Hamiltonian


class Case(NamedTuple):
    name: str
    n: int
    steps: tuple
    theta: np.ndarray   # [B, n_angles] gate angles
    t: np.ndarray       # [B, n_wide] evolution times of the wide gates
    obs: tuple          # ((matrix, wires), ...)
    weights: np.ndarray  # [B, n_obs]


def generator(step: Step):
    """(G, wires) with U = exp(-i theta / 2 G) -- for CRZ the projector on the control times Z."""
    if step.kind in ("RX", "RY", "RZ"):
        return PAULI[step.kind[1]], step.wires
    if step.kind == "CRZ":
        return np.kron(P1, Z), step.wires
    raise ValueError(step.kind)


def step_matrix(step: Step, theta_row, t_row):
    if step.kind == "WIDE":
        return expm(-1j * t_row[step.angle] * step.H)
    if step.kind == "CX":
        return CX
    if step.kind == "H":
        return HAD
    G, _w = generator(step)
    return expm(-0.5j * theta_row[step.angle] * G)


def observable_sum(case: Case, b: int, psi):
    out = np.zeros_like(psi)
    for k, (m, wires) in enumerate(case.obs):
        out += case.weights[b, k] * W.apply(psi[None], m, list(wires), case.n)[0]
    return out


def forward(case: Case, b: int, theta=None, t=None):
    """-> the states in front of every step and behind the last one: ``len(steps) + 1`` vectors."""
    theta = case.theta if theta is None else theta
    t = case.t if t is None else t
    psi = np.zeros(1 << case.n, dtype=np.complex128)
    psi[0] = 1.0
    out = [psi]
    for st in case.steps:
        psi = W.apply(psi[None], step_matrix(st, theta[b], t[b]), list(st.wires), case.n)[0]
        out.append(psi)
    return out


def cost(case: Case, theta=None, t=None) -> np.ndarray:
    """C_b for every sample."""
    out = np.empty(case.theta.shape[0])
    for b in range(out.size):
        psi = forward(case, b, theta, t)[-1]
        out[b] = np.real(np.vdot(psi, observable_sum(case, b, psi)))
    return out


def backward(case: Case, b: int, states, variant: str = None):
    """-> lambda behind every step (entry k: behind step k) for the forward ``states``."""
    lam = observable_sum(case, b, states[-1])
    out = [None] * len(case.steps)
    for k in range(len(case.steps) - 1, -1, -1):
        out[k] = lam
        st = case.steps[k]
        if st.kind == "WIDE" and variant == "lambda_not_propagated":
            continue
        U = step_matrix(st, case.theta[b], case.t[b])
        lam = W.apply(lam[None], U.conj().T, list(st.wires), case.n)[0]
    return out


def moment(psi, lam, wires, n: int, conjugate: bool = True) -> np.ndarray:
    """M[a][c] = sum_rest conj(lam[a, rest]) psi[c, rest] for one pair of states."""
    k = len(wires)
    rest = [q for q in range(n) if q not in wires]
    p = np.transpose(psi.reshape((2,) * n), list(wires) + rest).reshape(1 << k, -1)
    l = np.transpose(lam.reshape((2,) * n), list(wires) + rest).reshape(1 << k, -1)
    return (np.conj(l) if conjugate else l) @ p.T


def cotangent(phi, psi_behind, lam, wires, n: int, variant: str = None) -> np.ndarray:
    """G of one wide gate by definition: ``phi`` the state in front of it, ``lam`` the lambda behind it
    (``psi_behind``: the state behind it, which only the wrong variant ``moment_for_cotangent`` reads)."""
    wires = list(wires)
    if variant == "reversed_wires":
        wires = wires[::-1]
    if variant == "moment_for_cotangent":
        return moment(psi_behind, lam, wires, n)
    G = moment(phi, lam, wires, n, conjugate=variant != "unconjugated")
    return G.T if variant == "transposed" else G


def variant_applies(name: str, case: Case) -> bool:
    """Can the variant change what the case's gradients are?  (``lambda_not_propagated`` shows in the angles in front
    of a wide gate; the others in the wide gates' own cotangents.)"""
    wide = [k for k, st in enumerate(case.steps) if st.kind == "WIDE"]
    if not wide:
        return False
    if name == "lambda_not_propagated":
        return any(st.angle >= 0 and st.kind != "WIDE" for st in case.steps[:wide[-1]])
    return True


def gradients(case: Case, variant: str = None):
    """-> ``(dC/dtheta [B, n_angles], dC/dt [B, n_wide], [G of every wide gate in tape order, each [B, d, d]])``."""
    B = case.theta.shape[0]
    g_theta, g_t = np.zeros_like(case.theta), np.zeros_like(case.t)
    wide = [k for k, st in enumerate(case.steps) if st.kind == "WIDE"]
    cots = [np.zeros((B, 1 << len(case.steps[k].wires), 1 << len(case.steps[k].wires)), dtype=np.complex128) for k in wide]
    for b in range(B):
        states = forward(case, b)
        lams = backward(case, b, states, variant)
        for k, st in enumerate(case.steps):
            if st.kind == "WIDE":
                G = cotangent(states[k], states[k + 1], lams[k], st.wires, case.n, variant)
                cots[wide.index(k)][b] = G
                dU = -1j * st.H @ step_matrix(st, case.theta[b], case.t[b])
                g_t[b, st.angle] += 2.0 * np.real(np.sum(G * dU))
            elif st.angle >= 0:  # dU = -i/2 G U: the generator on the state behind the gate
                Gm, wires = generator(st)
                g_theta[b, st.angle] += 2.0 * np.real(
                    np.vdot(lams[k], -0.5j * W.apply(states[k + 1][None], Gm, list(wires), case.n)[0]))
    return g_theta, g_t, cots


def central_differences(case: Case, h: float = 1e-5):
    """dC/dtheta and dC/dt from central differences of :func:`cost` (error ~ h^2 |C'''| / 6: below 1e-9 here)."""
    g_theta, g_t = np.zeros_like(case.theta), np.zeros_like(case.t)
    for arr, out, key in ((case.theta, g_theta, "theta"), (case.t, g_t, "t")):
        for j in range(arr.shape[1]):
            up, dn = arr.copy(), arr.copy()
            up[:, j] += h
            dn[:, j] -= h
            out[:, j] = (cost(case, **{key: up}) - cost(case, **{key: dn})) / (2.0 * h)
    return g_theta, g_t


# ---- seeded cases -----------------------------------------------------------------------------------------------------
def random_hermitian(rng, d: int) -> np.ndarray:
    a = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    return (a + a.conj().T) / (2.0 * np.sqrt(d))


def _layer(n: int, first_angle: int):
    """RX on every wire, then CRZ on neighbours: 2 n - 1 angles."""
    steps = [Step("RX", (q,), first_angle + q) for q in range(n)]
    steps += [Step("CRZ", (q, q + 1), first_angle + n + q) for q in range(n - 1)]
    return steps, first_angle + 2 * n - 1


def make_case(name: str, n: int, B: int = 2, seed: int = 0, pauli: bool = False) -> Case:
    """The tapes of the end-to-end tests: ``middle`` (a wide gate among RX / CRZ layers), ``first``, ``last``,
    ``two`` (two wide gates in a row, a four-wire one on a permuted order and a three-wire one), ``unsorted`` (one
    three-wire gate on an unsorted wire tuple between single rotations)."""
    rng = np.random.default_rng(seed + 17 * n)
    w3 = tuple(int(q) for q in rng.permutation(n)[:3])
    w4 = tuple(int(q) for q in rng.permutation(n)[:4])
    H3, H4 = random_hermitian(rng, 8), random_hermitian(rng, 16)
    l1, a = _layer(n, 0)
    l2, a2 = _layer(n, a)
    if name == "middle":
        steps, n_wide = l1 + [Step("WIDE", w3, 0, H3)] + l2, 1
    elif name == "first":
        steps, n_wide = [Step("WIDE", w3, 0, H3)] + l1, 1
        a2 = a
    elif name == "last":
        steps, n_wide = l1 + [Step("H", (0,)), Step("WIDE", w4, 0, H4)], 1
        a2 = a
    elif name == "two":
        steps, n_wide = l1 + [Step("CX", (0, 1)), Step("WIDE", w4, 0, H4), Step("WIDE", w3, 1, H3)] + l2, 2
    elif name == "unsorted":
        steps = [Step("RY", (q,), q) for q in range(n)] + [Step("WIDE", w3, 0, H3)] + [Step("RZ", (0,), n), Step("RX", (1,), n + 1)]
        n_wide, a2 = 1, n + 2
    else:
        raise ValueError(name)
    if pauli:
        obs = ((X, (0,)), (np.kron(Z, Y), (1, n - 1)), (Z, (2,)))
    else:
        obs = ((Z, (0,)), (np.kron(Z, Z), (1, n - 1)), (Z, (2,)))
    return Case(name, n, tuple(steps), rng.uniform(-np.pi, np.pi, size=(B, a2)), rng.uniform(0.2, 0.9, size=(B, n_wide)),
                obs, rng.uniform(-1.0, 1.0, size=(B, len(obs))))


CASE_NAMES = ("middle", "first", "last", "two", "unsorted")


def moment_reference(psi, lam, wires, n: int, U=None) -> np.ndarray:
    """What ``qmle_wide_moment`` returns for states [B, 2^n] BEHIND a gate ``U`` ([d, d] or [B, d, d]; None: the
    moment itself), by definition: the cotangent against ``U^+ psi``, the state in front of the gate."""
    B = psi.shape[0]
    out = []
    for b in range(B):
        if U is None:
            out.append(moment(psi[b], lam[b], list(wires), n))
            continue
        Ub = U[b] if np.ndim(U) == 3 else U
        phi = W.apply(psi[b][None], Ub.conj().T, list(wires), n)[0]
        out.append(moment(phi, lam[b], list(wires), n))
    return np.stack(out)
