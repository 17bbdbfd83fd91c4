"""NumPy / SciPy reference for the pulse-level RX / RY leaves (``qmle_pulse_unitaries``, ``pulses.PulseGates``): the
five envelopes with the centre ``t_c = t / 2`` of the running time, the three coefficient forms, the fixed-grid scheme
on the support grid (through ``tests/evolution_reference.py``, lanes included), the step-doubling rule, the truth,
seeded cases and named wrong variants.

A solve is a row ``[p0, p1, p2, w, T, axis, 0, 0]`` (axis 0 = RX, 1 = RY); H(t) = cx(t) X + cy(t) Y.
"""
import numpy as np
from scipy.integrate import quad
from scipy.linalg import expm

import evolution_reference as ER

ENVELOPES = ("gaussian", "square", "cosine", "drag", "sech")
MODES = ("rwa", "lab", "drive")
OMEGA = 10 * np.pi  # omega_c = omega_q of PulseGates

VARIANTS = {
    "centre_T": "the envelope centred at T / 2 (the duration) instead of t / 2 (the running time)",
    "swap_axis": "RX and RY exchanged",
    "y_sign": "the Y coefficient with the opposite sign",
    "drop_w": "the rotation angle w not multiplied in",
    "drag_sign": "the derivative term of drag added with the opposite sign",
    "ry_phase": "RY without the carrier phase +pi/2 (exact forms)",
    "full_span": "the grid over [0, T] for square / cosine instead of their support [0, min(T, width)]",
    "drive_sd_sign": "the sign of sin((omega_c - omega_q) t) in the product-to-sum form (drive, off resonance)",
}


def variant_applies(name: str, envelope: str, mode: str, axis: int, solve) -> bool:
    """Whether the variant changes this solve AT THE DEFAULT FREQUENCIES (omega_c = omega_q)."""
    if name == "drive_sd_sign":
        # sin(0 t) = 0: exactly invisible on resonance.  tests/test_pulse_mp_reference_cpu.py tells it apart at
        # omega_c != omega_q.
        return False
    if name == "drag_sign":
        return envelope == "drag"
    if name == "ry_phase":
        return axis == 1 and mode != "rwa"
    if name == "full_span":
        return envelope in ("square", "cosine") and solve[1] < solve[4]
    if name == "y_sign":
        return axis == 1 or mode != "rwa"
    if name == "centre_T" and mode == "rwa":
        # U depends on the envelope's integral alone, and a symmetric envelope has the same integral either way:
        # int_0^T f((t - T/2) / s) dt = 2 int_0^(T/2) f(u / s) du = int_0^T f((t / 2) / s) dt.  Only drag's derivative
        # term (odd about its centre) tells the two apart.
        return envelope == "drag"
    if name == "centre_T" and envelope == "square":
        return solve[1] < solve[4]  # (width >= T: the pulse is on for the whole grid under either definition)
    return True


def envelope_value(envelope: str, p, t, t_c, variant=None):
    """p = (p0, p1, p2) broadcastable against t."""
    p0, p1, p2 = p
    d = t - t_c
    if envelope == "gaussian":
        return p0 * np.exp(-0.5 * (d / p1) ** 2)
    if envelope == "square":
        return p0 * (np.abs(d) <= p1 / 2)
    if envelope == "cosine":
        return p0 * np.cos(np.pi * np.clip(d / p1, -0.5, 0.5))
    if envelope == "drag":
        g = p0 * np.exp(-0.5 * (d / p2) ** 2)
        dg = g * (-d / p2 ** 2)
        return g - p1 * dg if variant == "drag_sign" else g + p1 * dg
    if envelope == "sech":
        return p0 / np.cosh(d / p1)
    raise ValueError(envelope)


def coefficients(envelope: str, mode: str, solve, t, omega_c=OMEGA, omega_q=OMEGA, variant=None):
    """(cx, cy) at the times t for the solve rows ``solve`` [..., 8] (broadcast against t)."""
    solve = np.asarray(solve, dtype=np.float64)
    p = (solve[..., 0], solve[..., 1], solve[..., 2])
    w, T, axis = solve[..., 3], solve[..., 4], solve[..., 5] != 0
    if variant == "swap_axis":
        axis = ~axis
    if variant == "drop_w":
        w = np.ones_like(w)
    t_c = T / 2 * np.ones_like(t) if variant == "centre_T" else t / 2
    env = envelope_value(envelope, p, t, t_c, variant)
    phase_on = variant != "ry_phase"
    if mode == "rwa":
        c = 0.5 * env * w
        cx, cy = np.where(axis, 0.0, c), np.where(axis, c, 0.0)
    elif mode == "lab":
        carrier = np.where(axis & phase_on, np.cos(omega_c * t + np.pi / 2), np.cos(omega_c * t))
        cx = env * carrier * np.cos(omega_q * t) * w
        cy = -env * carrier * np.sin(omega_q * t) * w
    elif mode == "drive":
        od, os_ = omega_c - omega_q, omega_c + omega_q
        y = axis & phase_on
        sd = -np.sin(od * t) if variant == "drive_sd_sign" else np.sin(od * t)
        mx = np.where(y, -0.5 * (np.sin(os_ * t) + sd), 0.5 * (np.cos(od * t) + np.cos(os_ * t)))
        my = np.where(y, -0.5 * (np.cos(os_ * t) - np.cos(od * t)), -0.5 * (np.sin(os_ * t) - sd))
        cx, cy = env * mx * w, env * my * w
    else:
        raise ValueError(mode)
    if variant == "y_sign":
        cy = -cy
    return cx, cy


def support(envelope: str, solves, variant=None) -> np.ndarray:
    """[n]: the end of the grid -- min(T, width) for square / cosine, T otherwise."""
    solves = np.atleast_2d(np.asarray(solves, dtype=np.float64))
    if envelope in ("square", "cosine") and variant != "full_span":
        return np.minimum(solves[:, 4], solves[:, 1])
    return solves[:, 4].copy()


def scheme(envelope: str, mode: str, solves, order: int, n_steps: int, lanes: int = 1, variant=None,
           omega_c=OMEGA, omega_q=OMEGA) -> np.ndarray:
    """The fixed-grid Magnus scheme on the support grid -> U [n, 2, 2] complex128."""
    solves = np.atleast_2d(np.asarray(solves, dtype=np.float64))
    h = support(envelope, solves, variant) / n_steps
    t = ER.node_times(np.zeros(len(solves)), h, n_steps, order)
    cx, cy = coefficients(envelope, mode, solves[:, None, :], t, omega_c, omega_q, variant)
    coef = np.stack([np.broadcast_to(cx, t.shape), np.broadcast_to(cy, t.shape)], axis=-1)
    return ER.magnus(np.stack([ER.X, ER.Y]), coef, h, order, lanes=lanes)


def doubling(envelope: str, mode: str, solves, tol: float, max_steps: int = 2 ** 13, first: int = 32):
    """Step doubling over ALL solves together: order-4 grids of 16, 32, 64, ... steps, accepted when
    max |U_N - U_{N/2}| / 15 <= tol for every solve -> (U, N, worst distance of the last round)."""
    prev, n = scheme(envelope, mode, solves, 4, first // 2), first
    while True:
        cur = scheme(envelope, mode, solves, 4, n)
        err = np.max(np.abs(cur - prev), axis=(1, 2))
        if (err / 15.0 <= tol).all() or 2 * n > max_steps:
            return cur, n, err
        prev, n = cur, 2 * n


def truth(envelope: str, mode: str, solve, omega_c=OMEGA, omega_q=OMEGA) -> np.ndarray:
    """U of one solve.  rwa: H(t) commutes with itself, U = exp(-i (w / 2) int env dt sigma) with the integral over
    the support by ``scipy.integrate.quad``; otherwise DOP853 at 1e-12 on the support."""
    solve = np.asarray(solve, dtype=np.float64)
    S = float(support(envelope, solve)[0])
    if mode == "rwa":
        area, _ = quad(lambda t: float(envelope_value(envelope, tuple(solve[:3]), t, t / 2)), 0.0, S,
                       epsabs=1e-14, epsrel=1e-14, limit=200)
        return expm(-1j * 0.5 * solve[3] * area * (ER.Y if solve[5] else ER.X))

    def fx(t, r):
        return coefficients(envelope, mode, solve, t, omega_c, omega_q)[0]

    def fy(t, r):
        return coefficients(envelope, mode, solve, t, omega_c, omega_q)[1]

    return ER.truth(np.stack([ER.X, ER.Y]), [fx, fy], 0.0, S)


def solve_row(p, w, T, axis) -> np.ndarray:
    row = np.zeros(8)
    row[:len(p)] = p
    row[3], row[4], row[5] = w, T, axis
    return row


def default_solve(envelope: str, axis: int, w: float) -> np.ndarray:
    """The solve of ``PulseGates.RX / RY (w)`` with the optimised default parameters of the envelope."""
    from qml_essentials_amd.pulses import PulseEnvelope

    pp = np.asarray(PulseEnvelope.get(envelope)["defaults"]["RY" if axis else "RX"], dtype=np.float64)
    return solve_row(pp[:-1], w, pp[-1], axis)


def seeded_solves(envelope: str, seed: int, n: int) -> np.ndarray:
    """n solves with differing p, w, T and alternating axis; for square / cosine the width is below T in rows
    0, 3, 6, ..., equal to T in rows 1, 4, ... and above it in the others."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n):
        T = rng.uniform(1.0, 3.2)
        w = rng.uniform(0.4, 2.5) * (-1.0 if k % 5 == 4 else 1.0)
        A = rng.uniform(0.3, 1.2)
        if envelope == "drag":
            p = [A, rng.uniform(0.2, 0.6), rng.uniform(0.8, 3.0)]
        elif envelope in ("square", "cosine"):
            p = [A, (rng.uniform(0.4, 0.9) * T, T, rng.uniform(1.1, 1.6) * T)[k % 3]]
        else:
            p = [A, rng.uniform(0.8, 3.0)]
        rows.append(solve_row(p, w, T, k % 2))
    return np.stack(rows)


# ---- whole tapes ------------------------------------------------------------------------------------------------------
def oracle_tape(tape, order: int, n_steps: int, row: int = 0):
    """A recorded pulse tape as the oracle's ``(name, wires, params)`` list of explicit matrices: every pulse leaf by
    :func:`scheme` on the grid of ``n_steps`` steps (row ``row`` of a batched request), every other gate by its own
    host matrix (row ``row`` of a batched one).  Nothing here touches the GPU."""
    from qml_essentials_amd.operations import Barrier
    from qml_essentials_amd.pulses import PulseRotation

    out = []
    for o in tape:
        if isinstance(o, Barrier):
            continue
        if isinstance(o, PulseRotation):
            solves = o.solves()
            m = scheme(o.envelope, o.mode, solves[row if len(solves) > 1 else 0][None], order, n_steps,
                       omega_c=o.omega_c, omega_q=o.omega_q)[0]
        else:
            m = np.asarray(o.matrix, dtype=np.complex128)
            if m.ndim == 3:
                m = m[row]
        out.append(("Matrix", list(o.wires), (m,)))
    return out
