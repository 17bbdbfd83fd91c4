"""NumPy forward-mode restatement of ``qmle_evolve_magnus_jac``: the fixed-grid Magnus solve of
``tests/evolution_reference.py`` with the EXACT derivative of the grid's result in given directions -- discretise,
then differentiate.  A direction k is a derivative ``dcoef[row, k, node, term]`` of the coefficient table and ``dh[row,
k]`` of the step.  Per exponential factor ``Omega = h sum_j a_j A(t_j)``, ``A = -i sum_i c_i H_i``:

    dOmega = dh sum_j a_j A(t_j) + h sum_j a_j dA(t_j),     U <- E U,   dU <- dE U + E dU

``dim = 2``: ``E = exp(-i (g0 I + a . sigma))`` and ``dE`` in closed form, in any real dtype (``np.longdouble`` too).
``dim = 4``: the column series of the kernel with its derivative term by term, ``v_{k+1} = Omega v_k / (k + 1)``,
``dv_{k+1} = (dOmega v_k + Omega dv_k) / (k + 1)``, the exponent cut into ``ceil(nu / 0.5)`` parts that chain through
``(v, dv)`` and the term count taken from ``nu``, the largest absolute row sum of ``h sum c_i H_i``.  The lanes of a row
combine as ``P = P_b P_a``, ``dP = dP_b P_a + P_b dP_a``.

``VARIANTS`` names what an implementation can get wrong; ``seeded_cases`` holds inputs on which every applicable
variant lies at least 1e-6 x ``column_scale`` from the right result (``tests/test_evolve_jac_reference_cpu.py``
asserts it).
"""
import numpy as np

import evolution_reference as ER
from pulse_jac_reference import column_scale  # noqa: F401  (the scale of the 1e-12 bar, per slot)

THETA, MAX_NORM = 0.5, 32768.0

VARIANTS = {
    "drop_dh": "the dh term of dOmega dropped",
    "no_E_dU": "dU <- dE U without E dU",
    "combine_no_dPb": "the lane combine dP = P_b dP_a without dP_b P_a (lanes > 1)",
    "weights_b": "the second factor of an order-4 step with the first factor's weights in dOmega (order 4)",
    "series_first": "the derivative series stops at dOmega v: no dOmega in the terms behind the first (dim 4)",
    "parts_no_product": "only the first part of a cut exponent is differentiated (dim 4, nu > 0.5)",
}


def variant_applies(name: str, dim: int, order: int, lanes: int, cut: bool) -> bool:
    if name == "combine_no_dPb":
        return lanes > 1
    if name == "weights_b":
        return order == 4
    if name == "series_first":
        return dim == 4
    if name == "parts_no_product":
        return dim == 4 and cut
    return True


def _pauli_parts(G):
    """g0, ax, ay, az of the 2x2 Hermitian G = g0 I + a . sigma (real scalars of G's precision)."""
    return ((G[0, 0].real + G[1, 1].real) / 2, G[0, 1].real, -G[0, 1].imag, (G[0, 0].real - G[1, 1].real) / 2)


def exp_su2_jac(G, dG):
    """(E, dE): exp(-i G) and its derivative in the direction dG, G and dG Hermitian 2x2, in their own precision."""
    ct = G.dtype.type
    rt = G.real.dtype.type
    g0, ax, ay, az = _pauli_parts(G)
    d0, dx, dy, dz = _pauli_parts(dG)
    r2 = ax * ax + ay * ay + az * az
    r = np.sqrt(r2)
    if r < 0.05:  # the series of sinc and of (cos r - sinc r) / r^2
        sinc = rt(1) - r2 / 6 * (1 - r2 / 20 * (1 - r2 / 42 * (1 - r2 / 72)))
        kappa = -rt(1) / 3 + r2 * (rt(1) / 30 - r2 * (rt(1) / 840 - r2 * (rt(1) / 45360 - r2 * (rt(1) / 3991680))))
    else:
        sinc = np.sin(r) / r
        kappa = (np.cos(r) - sinc) / r2
    c = np.cos(r)
    rho = ax * dx + ay * dy + az * dz
    eye = np.eye(2, dtype=G.dtype)
    sx = np.array([[0, 1], [1, 0]], dtype=G.dtype)
    sy = np.array([[0, -1j], [1j, 0]], dtype=G.dtype)
    sz = np.array([[1, 0], [0, -1]], dtype=G.dtype)
    a_s = ax * sx + ay * sy + az * sz
    da_s = dx * sx + dy * sy + dz * sz
    M = c * eye - ct(1j) * sinc * a_s
    dM = -sinc * rho * eye - ct(1j) * (kappa * rho * a_s + sinc * da_s)
    ph = np.cos(g0) - ct(1j) * np.sin(g0)
    return ph * M, ph * (dM - ct(1j) * d0 * M)


def series_counts(G):
    """(nu, parts, terms) of the kernel's column series for the Hermitian exponent G."""
    nu = float(np.max(np.sum(np.abs(G.real) + np.abs(G.imag) * (1 - np.eye(G.shape[0])), axis=1)))
    parts = int(np.ceil(nu / THETA)) if nu > THETA else 1
    nu_part = nu / parts
    n, bound = 1, nu_part
    while n < 24 and bound >= 1e-19:
        bound *= nu_part / (n + 1)
        n += 1
    return nu, parts, n


def apply_series_jac(G, dG, U, dU, variant=None):
    """(exp(-i G) U, d exp(-i G) U + exp(-i G) dU) by the column series (every column at once)."""
    nu, parts, n_series = series_counts(G)
    if not nu <= MAX_NORM:
        return np.full_like(U, np.nan), np.full_like(dU, np.nan)
    V, dV = U.copy(), dU.copy()
    for p in range(parts):
        T, dT = V.copy(), dV.copy()
        with_d = not (variant == "parts_no_product" and p > 0)
        for k in range(1, n_series + 1):
            f = 1.0 / (parts * k)
            Z = G @ dT
            if with_d and not (variant == "series_first" and k > 1):
                Z = Z + dG @ T
            T, dT = -1j * f * (G @ T), -1j * f * Z
            V, dV = V + T, dV + dT
    return V, dV


def _factor(H, c_nodes, dc_nodes, w, dw, h, dh, variant):
    """The Hermitian exponent G = h sum_j w_j sum_i c_i(t_j) H_i and its derivative (with the weights dw = w)."""
    G = h * sum(a * np.tensordot(c, H, axes=1) for a, c in zip(w, c_nodes))
    dG = h * sum(a * np.tensordot(dc, H, axes=1) for a, dc in zip(dw, dc_nodes))
    if variant != "drop_dh":
        dG = dG + dh * sum(a * np.tensordot(c, H, axes=1) for a, c in zip(dw, c_nodes))
    return G, dG


def magnus_jac(H, coef, h, dcoef, dh, order: int, lanes: int = 1, variant: str = None, dtype=np.float64):
    """H [n_terms, d, d], coef [rows, nodes, n_terms], h [rows], dcoef [rows, n_dirs, nodes, n_terms], dh [rows,
    n_dirs] -> [rows, 1 + n_dirs, d, d]: U and its exact grid derivatives.  ``dtype``: the real type of the
    arithmetic (``np.longdouble`` at dim 2 only)."""
    rt = np.dtype(dtype).type
    ct = np.result_type(rt, np.complex64).type
    H = np.asarray(H).astype(ct)
    coef, dcoef = np.asarray(coef).astype(rt), np.asarray(dcoef).astype(rt)
    rows, nodes, _ = coef.shape
    n_dirs, d = dcoef.shape[1], H.shape[-1]
    h = np.broadcast_to(np.asarray(h).astype(rt), (rows,))
    dh = np.asarray(dh).astype(rt)
    per = 2 if order == 4 else 1
    n_steps = nodes // per
    a1, a2 = rt(ER.A1), rt(ER.A2)
    if rt is not np.float64:  # the weights in the arithmetic's own precision
        s3 = np.sqrt(rt(3))
        a1, a2 = rt(1) / 4 + s3 / 6, rt(1) / 4 - s3 / 6
    out = np.empty((rows, 1 + n_dirs, d, d), dtype=ct)
    for r in range(rows):
        for k in range(n_dirs):
            partial = []
            for lo, hi in ER._split(n_steps, lanes):
                U, dU = np.eye(d, dtype=ct), np.zeros((d, d), dtype=ct)
                for s in range(lo, hi):
                    cn = [coef[r, per * s + j] for j in range(per)]
                    dn = [dcoef[r, k, per * s + j] for j in range(per)]
                    if order == 2:
                        factors = [((rt(1),), (rt(1),))]
                    else:
                        wb = (a1, a2) if variant == "weights_b" else (a2, a1)
                        factors = [((a1, a2), (a1, a2)), ((a2, a1), wb)]
                    for w, dw in factors:
                        G, dG = _factor(H, cn, dn, w, dw, h[r], dh[r, k], variant)
                        if d == 2:
                            E, dE = exp_su2_jac(G, dG)
                            U, dU = E @ U, dE @ U + (0 if variant == "no_E_dU" else E @ dU)
                        else:
                            V, dV = apply_series_jac(G, dG, U, np.zeros_like(dU) if variant == "no_E_dU" else dU,
                                                     variant)
                            U, dU = V, dV
                partial.append((U, dU))
            P, dP = partial[0]
            for Pb, dPb in partial[1:]:
                dP = Pb @ dP + (0 if variant == "combine_no_dPb" else dPb @ P)
                P = Pb @ P
            if not np.isfinite(P).all():
                P = np.full_like(P, np.nan)
            if not (np.isfinite(P).all() and np.isfinite(dP).all()):
                dP = np.full_like(P, np.nan)
            if k == 0:
                out[r, 0] = P
            out[r, 1 + k] = dP
    return out


def is_cut(H, coef, h, order: int) -> bool:
    """Does any factor of the solve have nu > 0.5 (a cut exponent)?"""
    return any(series_counts(G)[1] > 1 for G in _exponents(H, coef, h, order))


def _exponents(H, coef, h, order: int):
    per = 2 if order == 4 else 1
    for r in range(coef.shape[0]):
        for s in range(coef.shape[1] // per):
            cn = [coef[r, per * s + j] for j in range(per)]
            for w in ([(1.0,)] if order == 2 else [(ER.A1, ER.A2), (ER.A2, ER.A1)]):
                yield _factor(np.asarray(H), cn, cn, w, w, h[r], 0.0, None)[0]


# ---- seeded cases ----------------------------------------------------------------------------------------------------
# The Hamiltonians of evolution_reference on a short grid (a few steps: at dim 4 the exponents are cut into parts), the
# table differentiated in random directions.  Per case the seed of the directions (0 unless the CPU test needed another).
SEEDS = {}


def seeded_case(dim: int, order: int, seed: int, rows: int = 2, n_steps: int = 6, n_dirs: int = 2):
    name = f"dim{dim}-order{order}-seed{seed}"
    case = (ER.case_dim2 if dim == 2 else ER.case_dim4)(seed, rows)
    t0 = np.full(rows, case["t0"]) + 0.01 * np.arange(rows)
    h = (case["t1"] - t0) / n_steps * (1.0 + 0.03 * np.arange(rows))
    coef = ER.coef_table(case["fns"], ER.node_times(t0, h, n_steps, order))
    rng = np.random.default_rng([SEEDS.get(name, 0), dim, order, seed])
    dcoef = rng.normal(size=(rows, n_dirs) + coef.shape[1:])
    dh = rng.normal(size=(rows, n_dirs)) * 0.5
    return dict(name=name, H=case["H"], coef=coef, h=h, dcoef=dcoef, dh=dh, order=order, dim=dim)


def seeded_cases():
    return [seeded_case(dim, order, seed) for dim in (2, 4) for order in (2, 4) for seed in ER.SEEDS[:2]]
