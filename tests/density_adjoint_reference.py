"""Reference side of the noisy adjoint tests (tests/test_density_adjoint_reference_cpu.py, tests/test_gpu_density_adjoint.py).
NumPy only.

The truth is the parameter-shift gradient of ``sum_k w_k Tr(O_k rho)`` on ``noise_reference.simulate_mixed_fast`` in
complex128: two terms for RX / RY / RZ / Rot angles / RXX-type gates and CPhase, four for controlled rotations.  The rule
is exact with channels on the tape because they are linear in rho.

Beside it stands the adjoint rule itself on dense matrices (:func:`adjoint_gradient`) -- forward states kept,
``Lambda_{j-1} = A_j^+ Lambda_j``, ``dC/dtheta = Im Tr(Lambda_j G rho_j)`` -- with three WRONG variants that the
comparisons have to tell from the truth: channels dropped from the pull-back, the overlap taken behind the step's
channels instead of in front of them, the ket-side term halved."""
import numpy as np

from oracle import noise as ON

import noise_reference as NR

TWO_TERM = ("RX", "RY", "RZ", "RXX", "RYY", "RZZ", "RZX", "CPhase", "ControlledPhaseShift")
FOUR_TERM = ("CRX", "CRY", "CRZ")
VARIANTS = ("drop_channels", "overlap_behind", "halved")


def split_rot(oracle_tape):
    """The tape with every Rot(phi, theta, omega) as RZ(phi), RY(theta), RZ(omega): one angle per entry."""
    out = []
    for name, wires, params in oracle_tape:
        if name == "Rot":
            out += [("RZ", wires, (params[0],)), ("RY", wires, (params[1],)), ("RZ", wires, (params[2],))]
        else:
            out.append((name, wires, params))
    return out


def angle_slots(oracle_tape):
    """``[(entry, name)]`` per angle slot of a tape without Rot, in tape order -- the numbering of ``LoweredTape`` on
    the tape without its channels."""
    return [(i, name) for i, (name, _w, _p) in enumerate(oracle_tape) if name in TWO_TERM + FOUR_TERM]


def pauli_matrix(n, x, z):
    """The word of ``qmle_pauli_term`` on n wires (wire masks): P[i, i ^ x] = i^ny (-1)^{|(i ^ x) & z|} in positions."""
    pos = lambda m: sum(1 << (n - 1 - w) for w in range(n) if (m >> w) & 1)  # noqa: E731
    xp, zp = pos(x), pos(z)
    P = np.zeros((2**n, 2**n), dtype=np.complex128)
    ph = 1j ** (bin(x & z).count("1") % 4)
    for i in range(2**n):
        j = i ^ xp
        P[i, j] = ph * (-1) ** bin(j & zp).count("1")
    return P


def cost_matrix(n, w, groups=None, terms=None):
    """Lambda_L = sum_k w_k O_k: Z parities on the wire ``groups``, or the ``terms`` ``(coef, x, z, column)``."""
    L = np.zeros((2**n, 2**n), dtype=np.complex128)
    if groups is not None:
        idx = np.arange(2**n)
        for k, grp in enumerate(groups):
            par = np.zeros_like(idx)
            for q in grp:
                par ^= (idx >> (n - 1 - q)) & 1
            L += np.diag(w[k] * (1.0 - 2.0 * par))
    else:
        for coef, x, z, col in terms:
            L += w[col] * coef * pauli_matrix(n, x, z)
    return L


def cost(oracle_tape, n, L, dtype=np.complex128):
    return float(np.real(np.sum(L.T * NR.simulate_mixed_fast(oracle_tape, n, dtype).astype(np.complex128))))


def _shifted(tape, i, delta):
    name, wires, params = tape[i]
    return tape[:i] + [(name, wires, (params[0] + delta,))] + tape[i + 1:]


def shift_jacobian(oracle_tape, n, Ls, wanted=None, dtype=np.complex128):
    """d Tr(L rho) / d(angle slot) for every L of ``Ls`` by the shift rule -> ``[len(Ls), n_slots]``, zero outside
    ``wanted``, every array stored in ``dtype`` and rounded once per operation (complex64: the reference's own
    single-precision floor).  A shifted circuit differs from the tape at one gate only: the state in front of the gate
    comes from ONE forward run, and what follows the gate is applied to the cost matrices instead, once for all shifts
    (``Tr(L S(rho)) = Tr(S^+(L) rho)``), so the cost does not grow with the number of angles."""
    tape = split_rot(oracle_tape)
    slots = angle_slots(tape)
    g = np.zeros((len(Ls), len(slots)))
    at = {i for s_, (i, _n) in enumerate(slots) if wanted is None or s_ in wanted}
    front, rho = {}, np.zeros((2**n, 2**n), dtype=dtype)
    rho[0, 0] = 1.0
    for j, e in enumerate(tape):
        if j in at:
            front[j] = rho
        rho = _apply(rho, n, e).astype(dtype)
    back = {j: [] for j in at}  # per wanted entry: every L pulled back to the point behind it, transposed
    for L in Ls:
        cur = np.asarray(L).astype(dtype)
        for j in range(len(tape) - 1, -1, -1):
            if j in at:
                back[j].append(cur.T)
            cur = _apply(cur, n, tape[j], dagger=True).astype(dtype)

    def c(i, d):
        name, wires, params = tape[i]
        rho = _apply(front[i], n, (name, wires, (params[0] + d,))).astype(dtype)
        return np.array([np.real(np.sum(LT.astype(np.complex128) * rho.astype(np.complex128))) for LT in back[i]])

    for s, (i, name) in enumerate(slots):
        if wanted is not None and s not in wanted:
            continue
        if name in FOUR_TERM:
            cp, cm = (np.sqrt(2) + 1) / (4 * np.sqrt(2)), (np.sqrt(2) - 1) / (4 * np.sqrt(2))
            g[:, s] = cp * (c(i, np.pi / 2) - c(i, -np.pi / 2)) - cm * (c(i, 3 * np.pi / 2) - c(i, -3 * np.pi / 2))
        else:
            g[:, s] = 0.5 * (c(i, np.pi / 2) - c(i, -np.pi / 2))
    return g


def shift_jacobian_forward(oracle_tape, n, Ls, wanted=None, dtype=np.complex128):
    """:func:`shift_jacobian` with every shifted circuit run forward to its end and measured there (from the state in
    front of its gate): the plain form, which the CPU tests hold the pulled-back form to."""
    tape = split_rot(oracle_tape)
    slots = angle_slots(tape)
    g = np.zeros((len(Ls), len(slots)))
    LT = np.stack([np.asarray(L).T for L in Ls])

    # the state in front of every wanted gate, from ONE run: a shifted circuit differs from the tape at its gate only,
    # so it runs from there (the same operations in the same order and precision as a run from |0..0>)
    at = {i for s_, (i, _n) in enumerate(slots) if wanted is None or s_ in wanted}
    front, rho = {}, np.zeros((2**n, 2**n), dtype=dtype)
    rho[0, 0] = 1.0
    for j, e in enumerate(tape):
        if j in at:
            front[j] = rho
        rho = _apply(rho, n, e).astype(dtype)

    def c(i, d):
        rho = front[i]
        for e in _shifted(tape, i, d)[i:]:
            rho = _apply(rho, n, e).astype(dtype)
        return np.real(np.sum(LT * rho.astype(np.complex128)[None], axis=(1, 2)))

    for s, (i, name) in enumerate(slots):
        if wanted is not None and s not in wanted:
            continue
        if name in FOUR_TERM:
            cp, cm = (np.sqrt(2) + 1) / (4 * np.sqrt(2)), (np.sqrt(2) - 1) / (4 * np.sqrt(2))
            g[:, s] = cp * (c(i, np.pi / 2) - c(i, -np.pi / 2)) - cm * (c(i, 3 * np.pi / 2) - c(i, -3 * np.pi / 2))
        else:
            g[:, s] = 0.5 * (c(i, np.pi / 2) - c(i, -np.pi / 2))
    return g


def shift_gradient(oracle_tape, n, L, wanted=None, dtype=np.complex128):
    """d cost / d(angle slot) of one cost matrix -> ``[n_slots]``."""
    return shift_jacobian(oracle_tape, n, [L], wanted, dtype)[0]


def central_difference(oracle_tape, n, L, h=1e-5):
    tape = split_rot(oracle_tape)
    return np.array([(cost(_shifted(tape, i, h), n, L) - cost(_shifted(tape, i, -h), n, L)) / (2 * h)
                     for i, _ in angle_slots(tape)])


# ---- the adjoint rule on dense matrices, and its wrong variants ------------------------------------------------------
def _apply(rho, n, entry, dagger=False):
    name, wires, params = entry
    if name == "Barrier":
        return rho
    if name == "NQubitDepolarizing":  # its own dual
        return NR._depolarize(rho, n, list(wires), params[0])
    if not dagger:
        return ON.apply_to_density(rho, n, name, wires, params)
    ks = ON.kraus(name, params)
    if ks is None:
        if name == "DiagU" and list(wires) == list(range(n)):
            d = np.asarray(params[0], dtype=np.complex128)
            return np.conj(d)[:, None] * d[None, :] * rho
        ks = [np.asarray(ON.G.matrix(name, params), dtype=np.complex128)]
    return ON.apply_to_density(rho, n, "QubitChannel", wires, ([np.conj(K).T for K in ks],))


def _generator(name, wires, n):
    """G of exp(-i theta G / 2) lifted to n wires."""
    one = {"X": ON.X, "Y": ON.Y, "Z": ON.Z}
    p1 = np.diag([0.0, 1.0]).astype(np.complex128)
    if name in ("RX", "RY", "RZ"):
        g = one[name[1]]
    elif name in ("CRX", "CRY", "CRZ"):
        g = np.kron(p1, one[name[2]])
    elif name in ("CPhase", "ControlledPhaseShift"):
        g = -2.0 * np.kron(p1, p1)
    else:
        g = np.kron(one[name[1]], one[name[2]])
    k = len(wires)
    rest = [w for w in range(n) if w not in wires]
    full = np.kron(g, np.eye(2 ** (n - k))).reshape([2] * (2 * n))
    order = list(wires) + rest
    perm = [order.index(w) for w in range(n)]
    return full.transpose(perm + [n + p for p in perm]).reshape(2**n, 2**n)


def _is_channel(name):
    return name in ON.CHANNELS


def steps_together(tape):
    """The tape with the channels that follow a parametrised gate on its wires moved right behind it, past the entries
    on other wires in between (they commute): the order in which the sweep's steps see them."""
    tape, out = list(tape), []
    while tape:
        e = tape.pop(0)
        out.append(e)
        if e[0] not in TWO_TERM + FOUR_TERM:
            continue
        mine, rest = set(e[1]), []
        while tape:
            q = tape.pop(0)
            if _is_channel(q[0]) and set(q[1]) <= mine:
                out.append(q)
            elif mine & set(q[1]):
                rest.append(q)
                break
            else:
                rest.append(q)
        tape = rest + tape
    return out


def adjoint_jacobians(oracle_tape, n, Ls, variants=(None,)):
    """The adjoint rule in complex128 for every cost matrix of ``Ls`` -> ``{variant: [len(Ls), n_slots]}``; variant None
    is the rule, the others are ``VARIANTS``.  One forward run serves everything, and one pull-back per cost matrix
    serves every variant but "drop_channels", which pulls back differently."""
    assert all(v is None or v in VARIANTS for v in variants)
    tape = steps_together(split_rot(oracle_tape))
    rho = np.zeros((2**n, 2**n), dtype=np.complex128)
    rho[0, 0] = 1.0
    behind = []  # rho behind entry j
    for e in tape:
        rho = _apply(rho, n, e)
        behind.append(rho)
    slots = angle_slots(tape)
    last = []  # per slot: the last channel that follows the gate on its wires (the gate itself if none does)
    for j, _name in slots:
        k = j
        while k + 1 < len(tape) and _is_channel(tape[k + 1][0]) and set(tape[k + 1][1]) <= set(tape[j][1]):
            k += 1
        last.append(k)
    gen = [_generator(name, list(tape[j][1]), n) for j, name in slots]
    grho = {(s_, k): gen[s_] @ behind[k] for s_, (j, _name) in enumerate(slots) for k in {j, last[s_]}}
    out = {v: np.zeros((len(Ls), len(slots))) for v in variants}
    for dropped in (False, True):
        mine = [v for v in variants if (v == "drop_channels") == dropped]
        if not mine:
            continue
        for li, L in enumerate(Ls):
            lam = [None] * len(tape)  # Lambda behind entry j
            cur = np.array(L, dtype=np.complex128)
            for j in range(len(tape) - 1, -1, -1):
                lam[j] = cur
                if not (dropped and _is_channel(tape[j][0])):
                    cur = _apply(cur, n, tape[j], dagger=True)
            for v in mine:
                for s_, (j, _name) in enumerate(slots):
                    k = last[s_] if v == "overlap_behind" else j
                    val = float(np.imag(np.sum(lam[k].T * grho[s_, k])))  # Im Tr(Lambda G rho)
                    out[v][li, s_] = 0.5 * val if v == "halved" else val
    return out


def adjoint_jacobian(oracle_tape, n, Ls, variant=None):
    return adjoint_jacobians(oracle_tape, n, Ls, (variant,))[variant]


def adjoint_gradient(oracle_tape, n, L, variant=None):
    """:func:`adjoint_jacobian` of one cost matrix -> ``[n_slots]``."""
    return adjoint_jacobian(oracle_tape, n, [L], variant)[0]


def metric(got, ref, w):
    """max |got - ref| / max(1, sum |w|): the figure of tests/test_gpu_adjoint_routes.py, per row."""
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max() / max(1.0, float(np.abs(w).sum())))
