"""An independent reference for ``qmle_pulse_unitaries`` and ``qmle_pulse_unitaries_jac``: the fixed-grid result of one
pulse solve in ``mpmath`` at 40 digits, from the definitions alone, and its derivatives by ``p0, p1, p2, w, T`` as
central differences of that same function with a step of 1e-12 (at 40 digits the quotient is exact far beyond
float64: truncation ~ step^2 x third derivative ~ 1e-24 x 1e6, rounding ~ 1e-40 / 1e-12).

It shares no closed-form derivative, no series and no threshold with the kernel or with ``tests/pulse_jac_reference.py``:

* the five envelopes as ``include/qmle_sv.h`` states them, the centre at t / 2 of the running time;
* ``lab`` as the product ``env cos(omega_c t + phi) cos(omega_q t) w`` and ``-env cos(omega_c t + phi) sin(omega_q t) w``,
  phi = pi / 2 for the Y axis.  ``drive`` is the same function (product-to-sum is an identity), so both modes are
  compared with this product form;
* ``rwa`` as ``env w / 2`` on the pulse's axis;
* ``E = cos r I - i (sin r / r)(gx X + gy Y)`` by division, ``E = I`` at r = 0;
* the order-2 midpoint grid and the order-4 two-node grid over S = min(T, width) for square and cosine, over T otherwise.

The side that ends the grid (width or T) is read off the base point and held while differencing: that is the header's
convention (dS/dwidth = 1, dS/dT = 0 for width < T; otherwise, the tie included, dS/dwidth = 0, dS/dT = 1).  The NaN
rule of the kernels (a step beyond 2^15) is not modelled.
"""
import functools

import mpmath
import numpy as np

ENVELOPES = ("gaussian", "square", "cosine", "drag", "sech")
DIGITS = 40

mp = mpmath.mp.clone()  # (a context of its own: the precision of the global one is not touched)
mp.dps = DIGITS
STEP = mp.mpf(10) ** -12

# One step of order 2 of a square pulse in rwa with p0 = 2, width = 2, T = 1: the exponent's norm r is |w| exactly.
# Both sides of the kernel's series switch r < 0.05, zeros of sinc (pi, 2 pi), large exponents, the norm bound 2^15.
SINGLE_STEP_W = (0.0, 1e-9, 1e-4, 0.049, float(np.nextafter(0.05, 0.0)), 0.05, float(np.nextafter(0.05, 1.0)), 0.051,
                 1.0, float(np.pi), float(2 * np.pi), 100.0, 3e4, 32768.0)


def single_step_rows(ws=SINGLE_STEP_W) -> np.ndarray:
    """[len(ws), 8] solve rows ``p0, p1, p2, w, T, axis, 0, 0`` of those single steps, RX and RY alternating."""
    rows = np.zeros((len(ws), 8))
    rows[:, 0], rows[:, 1], rows[:, 3], rows[:, 4] = 2.0, 2.0, ws, 1.0
    rows[:, 5] = np.arange(len(ws)) % 2
    return rows


def _envelope(envelope, p0, p1, p2, t):
    d = t / 2  # t - t_c with t_c = t / 2
    if envelope == "gaussian":
        return p0 * mp.exp(-((d / p1) ** 2) / 2)
    if envelope == "square":
        return p0 if abs(d) <= p1 / 2 else mp.mpf(0)
    if envelope == "cosine":
        x = d / p1
        x = min(max(x, -mp.mpf(1) / 2), mp.mpf(1) / 2)
        return p0 * mp.cos(mp.pi * x)
    if envelope == "drag":
        g = p0 * mp.exp(-((d / p2) ** 2) / 2)
        return g * (1 - p1 * d / p2 ** 2)
    if envelope == "sech":
        return p0 / mp.cosh(d / p1)
    raise ValueError(envelope)


def _coefficients(envelope, rwa, axis_y, p0, p1, p2, w, t, omega_c, omega_q):
    env = _envelope(envelope, p0, p1, p2, t)
    if rwa:
        c = env * w / 2
        return (mp.mpf(0), c) if axis_y else (c, mp.mpf(0))
    carrier = mp.cos(omega_c * t + (mp.pi / 2 if axis_y else 0))
    return env * carrier * mp.cos(omega_q * t) * w, -env * carrier * mp.sin(omega_q * t) * w


def _unitary(envelope, rwa, axis_y, width_side, order, n_steps, omega_c, omega_q, p0, p1, p2, w, T):
    """[[u00, u01], [u10, u11]] of the grid's ordered product."""
    S = p1 if width_side else T
    h = S / n_steps
    if order == 2:
        offsets, weights = [mp.mpf(1) / 2], [[mp.mpf(1)]]
    elif order == 4:
        q = mp.sqrt(3) / 6
        offsets = [mp.mpf(1) / 2 - q, mp.mpf(1) / 2 + q]
        a1, a2 = mp.mpf(1) / 4 + q, mp.mpf(1) / 4 - q
        weights = [[a1, a2], [a2, a1]]  # Omega_a first, then Omega_b
    else:
        raise ValueError(order)
    u00, u01, u10, u11 = mp.mpc(1), mp.mpc(0), mp.mpc(0), mp.mpc(1)
    for s in range(n_steps):
        c = [_coefficients(envelope, rwa, axis_y, p0, p1, p2, w, (s + off) * h, omega_c, omega_q) for off in offsets]
        for row in weights:
            gx = h * sum(a * cj[0] for a, cj in zip(row, c))
            gy = h * sum(a * cj[1] for a, cj in zip(row, c))
            r = mp.sqrt(gx * gx + gy * gy)
            if r == 0:
                continue  # E = I
            cs, sn = mp.cos(r), mp.sin(r) / r
            e01, e10 = -1j * sn * mp.mpc(gx, -gy), -1j * sn * mp.mpc(gx, gy)  # -i sinc (gx X + gy Y)
            u00, u01, u10, u11 = (cs * u00 + e01 * u10, cs * u01 + e01 * u11,
                                  e10 * u00 + cs * u10, e10 * u01 + cs * u11)
    return u00, u01, u10, u11


@functools.lru_cache(maxsize=None)
def _row(envelope, rwa, row, order, n_steps, omega_c, omega_q):
    """[6, 2, 2] complex128 of one solve; ``row`` = (p0, p1, p2, w, T, axis) as floats (exact in mpmath)."""
    base = [mp.mpf(v) for v in row[:5]]
    axis_y = row[5] != 0
    width_side = envelope in ("square", "cosine") and row[1] < row[4]  # (the tie is the T side)
    oc, oq = (None, None) if rwa else (mp.mpf(omega_c), mp.mpf(omega_q))

    def f(args):
        return _unitary(envelope, rwa, axis_y, width_side, order, n_steps, oc, oq, *args)

    out = np.zeros((6, 2, 2), dtype=np.complex128)
    out[0] = np.array([complex(v) for v in f(base)]).reshape(2, 2)
    for k in range(5):
        if k == 2 and envelope != "drag":
            continue  # (nothing above reads p2)
        up, down = list(base), list(base)
        up[k], down[k] = base[k] + STEP, base[k] - STEP
        out[k + 1] = np.array([complex((a - b) / (2 * STEP)) for a, b in zip(f(up), f(down))]).reshape(2, 2)
    return out


def reference(envelope: str, mode: str, solves, order: int, n_steps: int, omega_c: float, omega_q: float) -> np.ndarray:
    """[rows, 6, 2, 2] complex128: slot 0 the grid's U, slots 1..5 its derivatives by p0, p1, p2, w, T.  ``mode`` is
    "rwa", "lab" or "drive"; the last two are one function here.  Results are kept per row, so that tests which name
    the same row twice pay once."""
    if mode not in ("rwa", "lab", "drive"):
        raise ValueError(mode)
    rwa = mode == "rwa"
    solves = np.atleast_2d(np.asarray(solves, dtype=np.float64))
    freq = (None, None) if rwa else (float(omega_c), float(omega_q))
    return np.stack([_row(envelope, rwa, tuple(float(v) for v in r[:6]), int(order), int(n_steps), *freq)
                     for r in solves])
