"""NumPy reference of ``qmle_density_apply_wide``: ``rho -> sum_m K_m rho K_m^+`` on arbitrary wires of a
``[2^n, 2^n]`` array in complex128, the complex64 evaluation of either form that sets the GPU tests' floor, seeded
cases, and named WRONG variants of the reference that the tests' metric has to tell apart from it.

Inputs are generic complex arrays, not Hermitian ones: on a Hermitian rho an exchanged ket and bra half shows only
as a conjugate."""
import functools
import itertools

import numpy as np

FACTOR = 16          # complex64: rel_err <= FACTOR * c64_floor (tests/test_gpu_noise_routes.py)
X64_RTOL = 1e-12     # complex128: rel_err below this
MARGIN = 100         # a wrong variant differs from the truth by at least MARGIN times the complex64 bound


def _blocks(rho, n, wires):
    """rho [2^n, 2^n] -> X[d, d, rest] (ket bits of ``wires``, bra bits of ``wires``, everything else) and the
    function that undoes it."""
    k = len(wires)
    t = np.asarray(rho).reshape((2,) * (2 * n))
    src = list(wires) + [n + w for w in wires]
    moved = np.moveaxis(t, src, list(range(2 * k)))
    shape = moved.shape

    def back(x):
        return np.moveaxis(x.reshape(shape), list(range(2 * k)), src).reshape(2 ** n, 2 ** n)

    return moved.reshape(2 ** k, 2 ** k, -1), back


def apply_wide(rho, n, wires, ops):
    """sum_m K_m rho K_m^+ with K_m on ``wires`` (the first wire the most significant bit of its index), complex128."""
    ops = np.asarray(ops, dtype=np.complex128).reshape(-1, 2 ** len(wires), 2 ** len(wires))
    x, back = _blocks(np.asarray(rho, dtype=np.complex128), n, wires)
    return back(np.einsum("mab,bcr,mdc->adr", ops, x, np.conj(ops), optimize=True))


def superoperator(ops):
    """S[(a, b), (c, e)] = sum_m K_m[a, c] conj(K_m[b, e]), the index order of ``KrausChannel.superoperator``."""
    ops = np.asarray(ops, dtype=np.complex128)
    d = ops.shape[-1]
    return np.einsum("mac,mbe->abce", ops, np.conj(ops)).reshape(d * d, d * d)


def apply_wide_c64(rho, n, wires, ops, form):
    """The same form evaluated by NumPy in complex64: inputs and operators rounded to complex64, the products taken in
    complex64 (the superoperator itself summed in complex128 and rounded once, as the library builds it)."""
    d = 2 ** len(wires)
    ops = np.asarray(ops, dtype=np.complex128).reshape(-1, d, d)
    x, back = _blocks(np.asarray(rho).astype(np.complex64), n, wires)
    if form == "superoperator":
        s = superoperator(ops).astype(np.complex64)
        return back((s @ x.reshape(d * d, -1)).astype(np.complex64))
    o = ops.astype(np.complex64)
    acc = np.zeros_like(x)
    for km in o:
        t = np.einsum("ab,bcr->acr", km, x)
        acc = acc + np.einsum("acr,dc->adr", t, np.conj(km))
    return back(acc.astype(np.complex64))


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.complex128), np.asarray(want, dtype=np.complex128)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def auto_form(k, n_ops, per_sample=False):
    """The automatic rule of the library: where the measured times of the two forms cross (profiles/density_wide.md),
    not where their arithmetic does (n_ops = d / 2)."""
    return "sandwich" if per_sample or n_ops <= (1 if k == 3 else 4) else "superoperator"


def c64_floor(rho, n, wires, ops, form, want=None):
    want = apply_wide(rho, n, wires, ops) if want is None else want
    return rel_err(apply_wide_c64(rho, n, wires, ops, form), want)


# ---- wrong variants ------------------------------------------------------------------------------------------------
def _no_conj(rho, n, wires, ops):  # the bra side without conjugation: sum K rho K^T
    ops = np.asarray(ops, dtype=np.complex128)
    x, back = _blocks(np.asarray(rho, dtype=np.complex128), n, wires)
    return back(np.einsum("mab,bcr,mdc->adr", ops, x, ops, optimize=True))


def _halves_exchanged(rho, n, wires, ops):  # K on the bra wires, conj K on the ket wires
    return apply_wide(np.asarray(rho).T, n, wires, ops).T


def _dagger(rho, n, wires, ops):  # K^+ for K
    return apply_wide(rho, n, wires, np.conj(np.swapaxes(np.asarray(ops), -1, -2)))


def _wires_reversed(rho, n, wires, ops):
    return apply_wide(rho, n, list(wires)[::-1], ops)


def _first_only(rho, n, wires, ops):
    return apply_wide(rho, n, wires, np.asarray(ops)[:1])


def _super_transposed(rho, n, wires, ops):  # S^T for S: (row pair) <-> (column pair)
    d = 2 ** len(wires)
    x, back = _blocks(np.asarray(rho, dtype=np.complex128), n, wires)
    return back(superoperator(ops).T @ x.reshape(d * d, -1))


WRONG = {"no_conj": _no_conj, "halves_exchanged": _halves_exchanged, "dagger": _dagger,
         "wires_reversed": _wires_reversed, "first_only": _first_only, "super_transposed": _super_transposed}


def applicable(kind, n_ops):
    """The variants that differ from the truth for operators of this kind: Pauli words are Hermitian and real or
    imaginary, so the depolarizing channel is blind to everything but a dropped operator."""
    if kind == "depol":
        return ["first_only"]
    return [v for v in WRONG if v != "first_only" or n_ops > 1]


# ---- seeded cases ----------------------------------------------------------------------------------------------------
KINDS = ("unitary", "nonunitary", "half", "half1", "depol", "per_sample")
DEPOL_P = 0.1


def depolarizing_kraus(p, k):
    """The 4^k operators of ``NQubitDepolarizingChannel`` (identity first, Pauli words in product order)."""
    paulis = [np.eye(2), np.array([[0, 1], [1, 0]]), np.array([[0, -1j], [1j, 0]]), np.diag([1.0, -1.0])]
    out = []
    for i, word in enumerate(itertools.product(range(4), repeat=k)):
        m = np.eye(1, dtype=np.complex128)
        for j in word:
            m = np.kron(m, paulis[j])
        out.append((np.sqrt(1 - p * (4 ** k - 1) / 4 ** k) if i == 0 else np.sqrt(p / 4 ** k)) * m)
    return np.stack(out)


def _ginibre(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def operators(kind, k, batch, rng):
    """-> complex128 ``[n_ops, d, d]`` (``per_sample``: ``[batch, d, d]`` unitaries)."""
    d = 2 ** k
    if kind == "unitary":
        return np.linalg.qr(_ginibre(rng, d, d))[0][None]
    if kind == "nonunitary":
        return _ginibre(rng, 1, d, d) / np.sqrt(2 * d)
    if kind in ("half", "half1"):
        m = d // 2 + (kind == "half1")
        return _ginibre(rng, m, d, d) / np.sqrt(2 * d * m)
    if kind == "depol":
        return depolarizing_kraus(DEPOL_P, k)
    if kind == "per_sample":
        return np.stack([np.linalg.qr(_ginibre(rng, d, d))[0] for _ in range(batch)])
    raise ValueError(kind)


def wire_sets(n, k):
    """The lowest wires in order; a set with wire n - 1 and wire 0 out of order (a bra target on position 0); a
    descending set.  Registers too small for three different sets return fewer."""
    sets = [list(range(k)),
            [n - 1, 0, n // 2] if k == 3 else [1, n - 2, 0, n - 1],
            list(range(n - 1, n - 1 - k, -1))]
    out = []
    for s in sets:
        if len(set(s)) == k and s not in out:
            out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def case(n, k, wires, kind, batch=1, seed=0):
    """-> ``(rho [batch, 2^n, 2^n] generic complex128, ops, want [batch, 2^n, 2^n])``; computed once per argument set
    and shared (callers must not write into the arrays)."""
    rng = np.random.default_rng([seed, n, k, KINDS.index(kind), batch] + list(wires))
    rho = _ginibre(rng, batch, 2 ** n, 2 ** n) / 2 ** n
    ops = operators(kind, k, batch, rng)
    want = np.stack([apply_wide(rho[b], n, list(wires), ops[b:b + 1] if kind == "per_sample" else ops)
                     for b in range(batch)])
    for a in (rho, ops, want):
        a.setflags(write=False)
    return rho, ops, want
