"""NumPy / SciPy complex128 reference for the Hamiltonian time evolution (``qmle_evolve_magnus``,
``jaqsi.Evolution``): the two fixed-grid commutator-free Magnus schemes with ``scipy.linalg.expm``, the
step-doubling rule that serves the adaptive solver names, the truth from ``scipy.integrate.solve_ivp`` (DOP853,
rtol = atol = 1e-12, on the real-split ODE), seeded test Hamiltonians, and named wrong variants of the schemes.

The scheme (``qml_essentials/evolution.py:204-231`` of the reference), A(t) = -i sum_i f_i(t) H_i:
  order 2   U <- exp(h A(t_n + h/2)) U
  order 4   U <- exp(Omega_b) exp(Omega_a) U,  Omega_a = h (a1 A1 + a2 A2), Omega_b = h (a2 A1 + a1 A2),
            A_k = A(t_n + c_k h),  c_1,2 = 1/2 -+ sqrt(3)/6,  a_1,2 = 1/4 +- sqrt(3)/6
The coefficient table holds f_i at the node times, in node order: ``coef[row, node, term]``.
"""
import numpy as np
from scipy.integrate import solve_ivp
from scipy.linalg import expm

SQRT3 = np.sqrt(3.0)
C1, C2 = 0.5 - SQRT3 / 6.0, 0.5 + SQRT3 / 6.0
A1, A2 = 0.25 + SQRT3 / 6.0, 0.25 - SQRT3 / 6.0

X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)
I2 = np.eye(2, dtype=np.complex128)

# what a scheme can get wrong; every variant but "reverse_combine" applies to order 4 alone or to both orders as said
VARIANTS = {
    "swap_exp": "exp(Omega_a) exp(Omega_b) U instead of exp(Omega_b) exp(Omega_a) U (order 4)",
    "reverse_combine": "the partial products of the lanes multiplied in reverse time order (lanes > 1)",
    "swap_a": "a1 and a2 exchanged (order 4)",
    "swap_nodes": "the node at c2 read before the node at c1 (order 4)",
    "right_multiply": "U E instead of E U",
    "h_row0": "h of row 0 for every row (rows > 1 with different h)",
}


def variant_applies(name: str, order: int, rows: int, lanes: int) -> bool:
    if name in ("swap_exp", "swap_a", "swap_nodes"):
        return order == 4
    if name == "reverse_combine":
        return lanes > 1
    if name == "h_row0":
        return rows > 1
    return True


def node_times(t0, h, n_steps: int, order: int) -> np.ndarray:
    """[rows, nodes] float64: the node times of the grid that starts at t0[r] with step h[r]."""
    t0 = np.atleast_1d(np.asarray(t0, dtype=np.float64))[:, None]
    h = np.atleast_1d(np.asarray(h, dtype=np.float64))[:, None]
    n = np.arange(n_steps, dtype=np.float64)[None, :]
    if order == 2:
        return t0 + (n + 0.5) * h
    t = np.empty((t0.shape[0], 2 * n_steps), dtype=np.float64)
    t[:, 0::2] = t0 + (n + C1) * h
    t[:, 1::2] = t0 + (n + C2) * h
    return t


def coef_table(fns, t: np.ndarray) -> np.ndarray:
    """[rows, nodes, n_terms]: every coefficient function at the node times ``t`` [rows, nodes] (a function takes
    the array of times and the row index array, so that a test can give every row its own pulse)."""
    rows = np.arange(t.shape[0])[:, None]
    return np.stack([np.broadcast_to(np.asarray(f(t, rows), dtype=np.float64), t.shape) for f in fns], axis=-1)


def _split(n_steps: int, lanes: int):
    return [(lane * n_steps // lanes, (lane + 1) * n_steps // lanes) for lane in range(lanes)]


def magnus(H, coef, h, order: int, lanes: int = 1, variant: str = None) -> np.ndarray:
    """The fixed-grid scheme in complex128: H [n_terms, d, d], coef [rows, nodes, n_terms], h [rows] -> U [rows, d, d].
    ``lanes``: the steps are cut into that many contiguous runs whose ordered products are multiplied in time order,
    later on the left (the split changes the result through rounding only).  ``variant``: one of VARIANTS."""
    H = np.asarray(H, dtype=np.complex128)
    coef = np.asarray(coef, dtype=np.float64)
    rows, nodes, _ = coef.shape
    d = H.shape[-1]
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (rows,)).copy()
    if variant == "h_row0":
        h[:] = h[0]
    A = -1j * np.einsum("rnt,tij->rnij", coef, H)  # [rows, nodes, d, d]
    hh = h[:, None, None, None]
    if order == 2:
        n_steps = nodes
        E = expm(hh * A)[:, :, None]  # [rows, steps, 1, d, d]
    else:
        n_steps = nodes // 2
        Ha, Hb = A[:, 0::2], A[:, 1::2]
        if variant == "swap_nodes":
            Ha, Hb = Hb, Ha
        a1, a2 = (A2, A1) if variant == "swap_a" else (A1, A2)
        Ea, Eb = expm(hh * (a1 * Ha + a2 * Hb)), expm(hh * (a2 * Ha + a1 * Hb))
        if variant == "swap_exp":
            Ea, Eb = Eb, Ea
        E = np.stack([Ea, Eb], axis=2)  # applied in this order
    partial = []
    for lo, hi in _split(n_steps, lanes):
        U = np.broadcast_to(np.eye(d, dtype=np.complex128), (rows, d, d)).copy()
        for s in range(lo, hi):
            for k in range(E.shape[2]):
                U = U @ E[:, s, k] if variant == "right_multiply" else E[:, s, k] @ U
        partial.append(U)
    if variant == "reverse_combine":
        partial = partial[::-1]
    U = partial[0]
    for P in partial[1:]:
        U = P @ U
    return U


def solve_fixed(H, fns, t0, t1, n_steps: int, order: int, **kw) -> np.ndarray:
    """``magnus`` on the grid of n_steps equal steps from t0[r] to t1[r]."""
    t0 = np.atleast_1d(np.asarray(t0, dtype=np.float64))
    t1 = np.atleast_1d(np.asarray(t1, dtype=np.float64))
    h = (t1 - t0) / n_steps
    return magnus(H, coef_table(fns, node_times(t0, h, n_steps, order)), h, order, **kw)


def doubling(H, fns, t0, t1, atol: float, rtol: float, max_steps: int = 2 ** 13, first: int = 32):
    """The rule behind the solver names "dopri8" / "dopri5": the order-4 grid with N = 32, 64, ... steps, accepted
    when max |U_N - U_{N/2}| / 15 <= atol + rtol for every row; N never exceeds max_steps.
    -> (U [rows, d, d], N, ok [rows]); rows that were never accepted are NaN-filled, N is the last grid tried
    (0 when max_steps < 32: nothing can be accepted)."""
    t0 = np.atleast_1d(np.asarray(t0, dtype=np.float64))
    d = np.asarray(H).shape[-1]
    if max_steps < first:
        return np.full((t0.shape[0], d, d), np.nan + 0j), 0, np.zeros(t0.shape[0], dtype=bool)
    prev = solve_fixed(H, fns, t0, t1, first // 2, 4)
    N = first
    while True:
        cur = solve_fixed(H, fns, t0, t1, N, 4)
        ok = np.max(np.abs(cur - prev), axis=(1, 2)) / 15.0 <= atol + rtol
        if ok.all() or 2 * N > max_steps:
            out = cur.copy()
            out[~ok] = np.nan
            return out, N, ok
        prev, N = cur, 2 * N


def truth(H, fns, t0: float, t1: float, row: int = 0) -> np.ndarray:
    """U(t1) of dU/dt = -i sum_i f_i(t) H_i U, U(t0) = I, by DOP853 at rtol = atol = 1e-12 on the real-split ODE."""
    H = np.asarray(H, dtype=np.complex128)
    d = H.shape[-1]
    G = -1j * H
    Ar, Ai = G.real, G.imag
    r = np.array([[row]])

    def rhs(t, y):
        tt = np.array([[t]])
        c = np.array([float(np.broadcast_to(np.asarray(f(tt, r), dtype=np.float64), (1, 1))[0, 0]) for f in fns])
        ar, ai = np.tensordot(c, Ar, axes=1), np.tensordot(c, Ai, axes=1)
        ur, ui = y[: d * d].reshape(d, d), y[d * d:].reshape(d, d)
        return np.concatenate([(ar @ ur - ai @ ui).reshape(-1), (ar @ ui + ai @ ur).reshape(-1)])

    y0 = np.concatenate([np.eye(d).reshape(-1), np.zeros(d * d)])
    sol = solve_ivp(rhs, (float(t0), float(t1)), y0, method="DOP853", rtol=1e-12, atol=1e-12)
    assert sol.success, sol.message
    y = sol.y[:, -1]
    return y[: d * d].reshape(d, d) + 1j * y[d * d:].reshape(d, d)


# ---- seeded test Hamiltonians ---------------------------------------------------------------------------------------
# A pulse of a few Rabi cycles whose three (four) terms do not commute and depend on time differently: exchanging the
# two exponentials of a step, the weights or the nodes then changes U by far more than 1e-6 on a grid of a few dozen
# steps (tests/test_evolution_cpu.py measures it), while 64..256 steps of order 4 reach 1e-6..1e-9.
def _envelope(t, tc, sigma):
    return np.exp(-0.5 * ((t - tc) / sigma) ** 2)


def case_dim2(seed: int, rows: int = 1):
    """X, Y and Z with a Gaussian envelope times cos(w t), the same envelope times sin(w t), and a constant;
    amplitudes, carrier and detuning drawn from ``seed``, and scaled a little differently per row (8 scales)."""
    rng = np.random.default_rng(seed)
    amp = rng.uniform(2.0, 3.0)
    w = rng.uniform(4.0, 6.0)
    det = rng.uniform(0.8, 1.6)
    t0, t1 = rng.uniform(0.1, 0.4), rng.uniform(2.2, 2.8)
    tc, sigma = 0.5 * (t0 + t1), 0.25 * (t1 - t0)
    scale = 1.0 + 0.05 * (np.arange(rows) % 8)

    def fx(t, r):
        return amp * scale[r] * _envelope(t, tc, sigma) * np.cos(w * t)

    def fy(t, r):
        return amp * scale[r] * _envelope(t, tc, sigma) * np.sin(w * t)

    def fz(t, r):
        return det * np.ones_like(t) * np.ones_like(r)

    return dict(H=np.stack([X, Y, Z]), fns=[fx, fy, fz], t0=t0, t1=t1, dim=2)


def case_dim4(seed: int, rows: int = 1):
    """ZZ, XI, IY and a random Hermitian 4x4: a constant coupling, the two quadratures of a Gaussian pulse, and a
    linear ramp."""
    rng = np.random.default_rng(seed)
    R = rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4))
    R = (R + R.conj().T) / 4.0
    J = rng.uniform(0.8, 1.4)
    amp = rng.uniform(1.5, 2.5)
    w = rng.uniform(3.0, 5.0)
    t0, t1 = rng.uniform(0.1, 0.4), rng.uniform(2.2, 2.8)
    tc, sigma = 0.5 * (t0 + t1), 0.25 * (t1 - t0)
    scale = 1.0 + 0.05 * (np.arange(rows) % 8)

    def fzz(t, r):
        return J * np.ones_like(t) * np.ones_like(r)

    def fxi(t, r):
        return amp * scale[r] * _envelope(t, tc, sigma) * np.cos(w * t)

    def fiy(t, r):
        return amp * scale[r] * _envelope(t, tc, sigma) * np.sin(w * t)

    def fr(t, r):
        return scale[r] * (t - t0) / (t1 - t0)

    return dict(H=np.stack([np.kron(Z, Z), np.kron(X, I2), np.kron(I2, Y), R]), fns=[fzz, fxi, fiy, fr],
                t0=t0, t1=t1, dim=4)


SEEDS = (11, 12, 13)


def seeded_cases():
    """Every seeded Hamiltonian: (name, case)."""
    out = []
    for s in SEEDS:
        out.append((f"dim2-seed{s}", case_dim2(s)))
        out.append((f"dim4-seed{s}", case_dim4(s)))
    return out
