"""NumPy forward-mode restatement of ``qmle_pulse_unitaries_jac``: the fixed-grid Magnus result of a pulse solve AND its
exact derivative by the five arguments ``p0, p1, p2, w, T`` (discretise, then differentiate), built on
``tests/pulse_reference.py`` (the grid, the support rule, the seeded solves) and ``tests/evolution_reference.py`` (the
node constants and the lane split).  Every formula is written out in closed form, so the same code runs in float64 and
in ``np.longdouble`` -- the distance between the two is the reference's own rounding error.

    g = h sum_j a_j c(t_j),  h = S / n_steps,  t_j = (s + c_j) h,  c = env(t) k(t) w
    dg/dtheta = h sum_j a_j dc/dtheta (t_j) + dh/dtheta sum_j a_j (c(t_j) + t_j dc/dt (t_j))
    E = cos r I - i sinc r (gx X + gy Y),  dE = -sinc rho I - i ((kappa rho gx + sinc dgx) X + (kappa rho gy + sinc dgy) Y)
    rho = gx dgx + gy dgy,  kappa = (cos r - sinc r) / r^2
    U <- E U,  dU_k <- dE_k U + E dU_k

Conventions (``include/qmle_sv.h``): S = min(T, width) for square / cosine with dS/dwidth = 1, dS/dT = 0 for
width < T and dS/dwidth = 0, dS/dT = 1 otherwise (the tie is the T side); square's amplitude has derivative zero by
its width (almost everywhere).
"""
import numpy as np

import evolution_reference as ER
import pulse_reference as PR

SLOTS = ("U", "p0", "p1", "p2", "w", "T")

VARIANTS = {
    "no_node_shift": "d/dT without the moving-node term t dc/dt",
    "no_span_width": "the width derivative of square / cosine without the grid term",
    "one_term_product": "dU <- dE U alone, without E dU",
    "w_ratio": "d/dw as c / w (wrong, and not finite, at w = 0)",
    "drag_dsigma_sign": "the sign of drag's sigma derivative",
    "lab_kt_swapped": "omega_c and omega_q exchanged in the time derivative of lab's carrier",
    "drive_no_difference_term": "the (omega_c - omega_q) terms of the time derivative of drive's carrier dropped",
    "drive_sd_sign": "the sign of sin((omega_c - omega_q) t) in drive's carrier",
}
# These three differ from the right scheme at omega_c != omega_q alone (on resonance the term they get wrong is
# multiplied by an exact zero, or the exchange is of two equal numbers): tests/test_pulse_mp_reference_cpu.py.
DETUNED_VARIANTS = ("lab_kt_swapped", "drive_no_difference_term", "drive_sd_sign")


def variant_applies(name: str, envelope: str, mode: str) -> bool:
    if name == "no_node_shift":
        return not (envelope == "square" and mode == "rwa")  # (there c does not depend on t)
    if name == "no_span_width":
        # (cosine: the grid term is the integrand at the end of the support, where the cosine vanishes -- what is
        # left of it on a grid is of the size of the quadrature error)
        return envelope == "square"
    if name == "drag_dsigma_sign":
        return envelope == "drag"
    if name == "lab_kt_swapped":
        return mode == "lab"
    if name in ("drive_no_difference_term", "drive_sd_sign"):
        return mode == "drive"
    return True


def column_scale(ref):
    """[6]: what a slot's distance is divided by -- 1 for U, max(1, max |column|) for the derivative slots."""
    s = np.maximum(1.0, np.abs(ref).max(axis=(0, 2, 3)))
    s[0] = 1.0
    return s


def envelope_jac(envelope: str, p0, p1, p2, t, variant=None):
    """(env, d/dp0, d/dp1, d/dp2, d/dt) at the times t, the centre at t / 2."""
    d = t / 2
    zero = np.zeros_like(t)
    pi = t.dtype.type(np.pi)
    if envelope == "gaussian":
        x = d / p1
        f = np.exp(-(x * x) / 2)
        g = p0 * f
        return g, f, g * x * x / p1, zero, -g * x / p1 / 2
    if envelope == "square":
        on = (np.abs(d) <= p1 / 2).astype(t.dtype)
        return p0 * on, on, zero, zero, zero
    if envelope == "cosine":
        x = d / p1
        inside = (np.abs(x) <= 0.5).astype(t.dtype)
        xc = np.clip(x, -0.5, 0.5)
        dx = -pi * p0 * np.sin(pi * xc) * inside
        return p0 * np.cos(pi * xc), np.cos(pi * xc), dx * (-x / p1), zero, dx / p1 / 2
    if envelope == "drag":
        x = d / p2
        f = np.exp(-(x * x) / 2)
        g = p0 * f
        u = d / (p2 * p2)
        k = 1 - p1 * u
        ds = g * x * x / p2 * k + 2 * g * p1 * u / p2
        if variant == "drag_dsigma_sign":
            ds = -ds
        return g * k, f * k, -g * u, ds, (-g * u * k - g * p1 / (p2 * p2)) / 2
    if envelope == "sech":
        u = d / p1
        sech = 1 / np.cosh(u)
        th = np.tanh(u)
        return p0 * sech, sech, p0 * sech * th * u / p1, zero, -p0 * sech * th / p1 / 2
    raise ValueError(envelope)


def carrier_jac(mode: str, axis, t, omega_c, omega_q, variant=None):
    """(kx, ky, dkx/dt, dky/dt): c = env k w.  axis: bool [n, 1]."""
    ty = t.dtype.type
    pi, oc, oq = ty(np.pi), ty(omega_c), ty(omega_q)
    half, zero = np.full_like(t, 0.5), np.zeros_like(t)
    if mode == "rwa":
        return np.where(axis, zero, half), np.where(axis, half, zero), zero, zero
    if mode == "lab":
        a = oc * t + np.where(axis, pi / 2, ty(0))
        cc, sc, cq, sq = np.cos(a), np.sin(a), np.cos(oq * t), np.sin(oq * t)
        dc, dq = (oq, oc) if variant == "lab_kt_swapped" else (oc, oq)
        return cc * cq, -cc * sq, -dc * sc * cq - dq * cc * sq, dc * sc * sq - dq * cc * cq
    if mode == "drive":
        od, os_ = oc - oq, oc + oq
        sd, cd, ss, cs = np.sin(od * t), np.cos(od * t), np.sin(os_ * t), np.cos(os_ * t)
        sk = -sd if variant == "drive_sd_sign" else sd
        kx = np.where(axis, -(ss + sk) / 2, (cd + cs) / 2)
        ky = np.where(axis, -(cs - cd) / 2, -(ss - sk) / 2)
        if variant == "drive_no_difference_term":
            od = ty(0)
        kxt = np.where(axis, -(os_ * cs + od * cd) / 2, -(od * sd + os_ * ss) / 2)
        kyt = np.where(axis, (os_ * ss - od * sd) / 2, -(os_ * cs - od * cd) / 2)
        return kx, ky, kxt, kyt
    raise ValueError(mode)


def _mat(re_diag, off_x, off_y):
    """[n, 2, 2]: re_diag I - i (off_x X + off_y Y)."""
    ctype = np.result_type(re_diag.dtype, np.complex64)
    M = np.zeros(re_diag.shape + (2, 2), dtype=ctype)
    M[..., 0, 0] = M[..., 1, 1] = re_diag
    M[..., 0, 1] = -1j * off_x - off_y
    M[..., 1, 0] = -1j * off_x + off_y
    return M


def _kappa(r, c, sinc):
    r2 = r * r
    series = -1 / r.dtype.type(3) + r2 * (1 / r.dtype.type(30) - r2 * (1 / r.dtype.type(840) - r2 * (
        1 / r.dtype.type(45360) - r2 / r.dtype.type(3991680))))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r < 0.05, series, (c - sinc) / np.where(r2 == 0, 1, r2))


def scheme_jac(envelope: str, mode: str, solves, order: int, n_steps: int, lanes: int = 1, variant=None,
               omega_c=PR.OMEGA, omega_q=PR.OMEGA, dtype=np.float64) -> np.ndarray:
    """[n, 6, 2, 2] complex: slot 0 the scheme's U, slots 1..5 its derivatives by p0, p1, p2, w, T."""
    ty = np.dtype(dtype).type
    solves = np.atleast_2d(np.asarray(solves, dtype=np.float64)).astype(dtype)
    n = len(solves)
    p0, p1, p2, w, T = (solves[:, k:k + 1] for k in range(5))
    axis = solves[:, 5:6] != 0
    sup = envelope in ("square", "cosine")
    width_ends = (p1 < T) if sup else np.zeros_like(T, dtype=bool)
    S = np.where(width_ends, p1, T)  # (= PR.support: min(T, width), the tie on the T side)
    assert np.array_equal(S[:, 0].astype(np.float64), PR.support(envelope, solves.astype(np.float64)))
    h = S / ty(n_steps)
    dh = np.ones_like(h) / ty(n_steps)
    dh_p1 = np.where(width_ends, dh, 0) if variant != "no_span_width" else np.zeros_like(h)
    dh_T = np.where(width_ends, 0, dh)
    steps = np.arange(n_steps).astype(dtype)[None, :]
    sq3 = np.sqrt(ty(3)) / 6
    if order == 2:
        offs, alpha = [ty(0.5)], [[ty(1)]]
    else:
        offs = [ty(0.5) - sq3, ty(0.5) + sq3]
        a1, a2 = ty(0.25) + sq3, ty(0.25) - sq3
        alpha = [[a1, a2], [a2, a1]]  # Omega_a, Omega_b
    node = []
    for off in offs:
        t = (steps + off) * h  # [n, steps]
        e0, e1, e2, e3, e4 = envelope_jac(envelope, p0, p1, p2, t, variant)
        kx, ky, kxt, kyt = carrier_jac(mode, axis, t, omega_c, omega_q, variant)
        v = {}
        for a, (k, kt) in enumerate(((kx, kxt), (ky, kyt))):
            m = e0 * k
            c = m * w
            if variant == "w_ratio":
                with np.errstate(divide="ignore", invalid="ignore"):
                    dw = c / w
            else:
                dw = m
            cdot = (e4 * k + e0 * kt) * w
            v[a] = dict(c=c, p0=e1 * k * w, p1=e2 * k * w, p2=e3 * k * w, w=dw, mv=c + t * cdot,
                        mvT=c if variant == "no_node_shift" else c + t * cdot)
        node.append(v)

    def summed(half, a, key):
        return sum(alpha[half][j] * node[j][a][key] for j in range(len(offs)))

    ctype = np.result_type(dtype, np.complex64)
    halves = []
    for half in range(len(alpha)):
        g = [h * summed(half, a, "c") for a in range(2)]
        dg = [[h * summed(half, a, "p0"), h * summed(half, a, "p1") + dh_p1 * summed(half, a, "mv"),
               h * summed(half, a, "p2"), h * summed(half, a, "w"), dh_T * summed(half, a, "mvT")] for a in range(2)]
        r = np.sqrt(g[0] * g[0] + g[1] * g[1])
        c_, s_ = np.cos(r), np.sin(r)
        sinc = np.where(r < 0.05, 1 - r * r / 6 * (1 - r * r / 20 * (1 - r * r / 42)), s_ / np.where(r == 0, 1, r))
        kap = _kappa(r, c_, sinc)
        E = _mat(c_, sinc * g[0], sinc * g[1])  # [n, steps, 2, 2]
        dE = []
        for k in range(5):
            rho = g[0] * dg[0][k] + g[1] * dg[1][k]
            dE.append(_mat(-sinc * rho, kap * rho * g[0] + sinc * dg[0][k], kap * rho * g[1] + sinc * dg[1][k]))
        bad = ~(np.abs(g[0]) + np.abs(g[1]) <= 32768.0)
        halves.append((E, dE, bad))
    eye = np.broadcast_to(np.eye(2, dtype=ctype), (n, 2, 2))
    partial = []
    for lo, hi in ER._split(n_steps, lanes):
        U, dU = eye.copy(), [np.zeros((n, 2, 2), dtype=ctype) for _ in range(5)]
        for s in range(lo, hi):
            for E, dE, _ in halves:
                for k in range(5):
                    dU[k] = dE[k][:, s] @ U if variant == "one_term_product" else dE[k][:, s] @ U + E[:, s] @ dU[k]
                U = E[:, s] @ U
        partial.append((U, dU))
    U, dU = partial[0]
    for L, dL in partial[1:]:
        dU = [dL[k] @ U + L @ dU[k] for k in range(5)]
        U = L @ U
    out = np.stack([U] + dU, axis=1)
    failed = np.zeros(n, dtype=bool)
    for _, _, bad in halves:
        failed |= bad.any(axis=1)
    out[failed] = np.nan
    return out


def solve_with_jacobian(table, envelope: str, mode: str, omega_c: float, omega_q: float, order: int = 4,
                        n_steps: int = 64):
    """The signature of ``pulses.solve_with_jacobian`` on the CPU (the solver that tests inject into ``qoc``):
    (U [n, 2, 2], J [n, 5, 2, 2], steps)."""
    out = scheme_jac(envelope, mode, table, order, n_steps, omega_c=omega_c, omega_q=omega_q)
    return out[:, 0].copy(), out[:, 1:].copy(), n_steps
