"""NumPy complex128 reference for dense matrices on three and four wires (``qmle_apply_matrix``, the segmented
execution of ``simulation.simulate_and_measure``) with named wrong variants of itself, the cases the GPU tests use,
and seeded Hamiltonians of dimension 8 and 16 for ``qmle_evolve_magnus_wide``.

Convention (``operations.embed_matrix``): the first wire of ``wires`` is the most significant bit of the matrix index,
wire ``w`` is axis ``w`` of the state reshaped to ``(2,) * n`` -- bit position ``n - 1 - w`` of the flat index.
"""
import itertools

import numpy as np

import evolution_reference as R

# what an implementation of the apply pass can get wrong
VARIANTS = {
    "lsb_first": "the wires read least-significant first (the last wire as the top bit of the matrix index)",
    "transpose": "U^T instead of U (row and column index exchanged)",
    "conjugate": "conj(U) instead of U",
    "sample0": "the matrix of sample 0 for every sample (per-sample matrices, batch > 1)",
    "position": "wire w taken as bit position w (axis n - 1 - w)",
}


def variant_applies(name: str, per_sample: bool, batch: int, wires, n: int) -> bool:
    if name == "sample0":
        return per_sample and batch > 1
    if name == "position":  # the same axes in the same order: nothing to tell apart
        return [n - 1 - w for w in wires] != list(wires)
    if name == "lsb_first":
        return list(wires)[::-1] != list(wires)
    return True


def apply(states, U, wires, n: int, variant: str = None) -> np.ndarray:
    """``U`` ([d, d], or [B, d, d]: one per state) on ``wires`` of ``states`` [B, 2^n] -> [B, 2^n], complex128,
    by tensordot over the wire axes.  ``variant``: one of VARIANTS."""
    psi = np.asarray(states, dtype=np.complex128)
    B, k = psi.shape[0], len(wires)
    U = np.asarray(U, dtype=np.complex128)
    per_sample = U.ndim == 3
    wires = list(wires)
    if variant == "lsb_first":
        wires = wires[::-1]
    if variant == "position":
        wires = [n - 1 - w for w in wires]
    if variant == "transpose":
        U = np.swapaxes(U, -1, -2)
    if variant == "conjugate":
        U = np.conj(U)
    out = np.empty_like(psi)
    for b in range(B):
        M = U[0 if variant == "sample0" else b] if per_sample else U
        t = M.reshape((2,) * (2 * k))
        v = np.tensordot(t, psi[b].reshape((2,) * n), axes=(list(range(k, 2 * k)), wires))
        out[b] = np.moveaxis(v, list(range(k)), wires).reshape(-1)
    return out


def random_unitaries(rng, d: int, count: int = None) -> np.ndarray:
    """Haar-like unitaries from the QR decomposition of Gaussian matrices: [d, d], or [count, d, d]."""
    m = count or 1
    g = rng.normal(size=(m, d, d)) + 1j * rng.normal(size=(m, d, d))
    q = np.stack([np.linalg.qr(x)[0] for x in g])
    return q if count else q[0]


def random_states(rng, batch: int, n: int) -> np.ndarray:
    psi = rng.normal(size=(batch, 1 << n)) + 1j * rng.normal(size=(batch, 1 << n))
    return psi / np.linalg.norm(psi, axis=1, keepdims=True)


def wire_sets(k: int, n: int):
    """The four wire sets of one register size: the top positions, the bottom positions (position 0 among them), a
    scattered set (position 0 among them) and a permuted order of another scattered set -- as wires (wire w = position n - 1 - w).  Where the register is the gate
    (n == k) all four are orders of the same wires."""
    pos_top = list(range(n - 1, n - 1 - k, -1))
    pos_bottom = list(range(k - 1, -1, -1))
    step = max(1, (n - 1) // (k - 1))
    pos_scattered = sorted({min(n - 1, i * step) for i in range(k)}, reverse=True)
    if len(pos_scattered) < k:
        pos_scattered = pos_top
    step2 = max(1, (n - 2) // (k - 1))  # the permuted order: a scattered set that leaves position 0 alone where it can
    base = sorted({min(n - 1, 1 + i * step2) for i in range(k)}, reverse=True)
    if len(base) < k:
        base = pos_scattered
    permuted = base[1:] + base[:1]
    if k == 4:
        permuted = [permuted[1], permuted[0]] + permuted[2:]
    return {"top": [n - 1 - p for p in pos_top], "bottom": [n - 1 - p for p in pos_bottom],
            "scattered": [n - 1 - p for p in pos_scattered], "permuted": [n - 1 - p for p in permuted]}


# register sizes of the GPU sweep: the register as the gate; one thread / one wave / one block of 256 groups and the
# sizes beside those edges (groups = 2^(n - k): 64 at n = k + 6, 256 at n = k + 8)
SIZES = {3: (3, 4, 9, 10, 11, 12), 4: (4, 5, 11, 12, 13)}


def apply_cases():
    """(id, k, n, wires, batch, per_sample) of every GPU case of the apply pass but the long batch."""
    out = []
    for k in (3, 4):
        for wires in itertools.permutations(range(5), k):
            for per_sample in (False, True):
                out.append((f"k{k}-n5-{''.join(map(str, wires))}-{'rows' if per_sample else 'const'}", k, 5,
                            list(wires), 3, per_sample))
        for n in SIZES[k]:
            for name, wires in wire_sets(k, n).items():
                for per_sample in (False, True):
                    out.append((f"k{k}-n{n}-{name}-{'rows' if per_sample else 'const'}", k, n, wires, 2, per_sample))
    return out


def case_data(k: int, n: int, batch: int, per_sample: bool, seed: int = 0):
    """Seeded unitaries and normalised states of one case."""
    rng = np.random.default_rng(1000 * k + 10 * n + batch + (7 if per_sample else 0) + seed)
    U = random_unitaries(rng, 1 << k, batch if per_sample else None)
    return U, random_states(rng, batch, n)


# ---- Hamiltonians of dimension 8 and 16 from Pauli strings ----------------------------------------------------------
PAULI = {"I": R.I2, "X": R.X, "Y": R.Y, "Z": R.Z}


def pauli_string(word: str) -> np.ndarray:
    m = np.ones((1, 1), dtype=np.complex128)
    for c in word:
        m = np.kron(m, PAULI[c])
    return m


def solver_case(dim: int, n_terms: int, rows: int, n_steps: int, order: int, seed: int = 0, norm: float = 12.0):
    """A seeded Hamiltonian of ``n_terms`` distinct non-identity Pauli strings on log2(dim) wires with per-row
    coefficients and steps: H [n_terms, dim, dim], coef [rows, nodes, n_terms], h [rows].  Every string has 2-norm
    1, so ``h sum_i |c_i| <= norm`` bounds ``h |sum_i c_i H_i|``; the table is scaled to spend ``norm`` (12, below
    the 15 that tests/test_gpu_evolution.py sizes for) on one step whatever the number of steps: with more steps
    the exponent of a step shrinks and the product of them keeps a norm of that order."""
    k = dim.bit_length() - 1
    rng = np.random.default_rng(100000 * dim + 1000 * n_terms + 100 * rows + 10 * n_steps + order + seed)
    words = ["".join(w) for w in itertools.product("IXYZ", repeat=k)][1:]
    words = [words[i] for i in rng.permutation(len(words))[:n_terms]]
    H = np.stack([pauli_string(w) for w in words])
    nodes = n_steps * (2 if order == 4 else 1)
    h = rng.uniform(0.6, 1.0, size=rows) / n_steps
    coef = rng.uniform(-1.0, 1.0, size=(rows, nodes, n_terms))
    coef *= (norm * rng.uniform(0.5, 1.0, size=(rows, 1, 1))) / (n_steps * h[:, None, None] * np.abs(coef).sum(-1, keepdims=True))
    return dict(H=H, coef=coef, h=h, words=words)


SOLVER_LANES = {8: (0, 1, 4, 8), 16: (0, 1, 4)}


def solver_cases():
    """(id, dim, n_terms, rows, n_steps, order) of every GPU case of the solver (each runs at every lane count)."""
    out = []
    for dim in (8, 16):
        for order in (2, 4):
            for rows, n_steps, n_terms in ((1, 1, 1), (1, 64, 16), (3, 5, 16), (3, 64, 1), (70, 5, 1), (70, 1, 16)):
                out.append((f"dim{dim}-o{order}-r{rows}-s{n_steps}-t{n_terms}", dim, n_terms, rows, n_steps, order))
    return out


def solver_variant_applies(name: str, order: int, rows: int, lanes: int, n_steps: int, n_terms: int) -> bool:
    """``evolution_reference.variant_applies`` narrowed to what a case can show.  With ONE term every exponential
    of a row is a function of the same matrix: they commute, and exchanging factors, weights, nodes or the side of
    the multiplication changes nothing -- only a wrong ``h`` shows.  A run of one step of order 2 is one factor,
    and with one step there is no second run to combine in another order."""
    if not R.variant_applies(name, order, rows, lanes):
        return False
    if name == "h_row0":
        return True
    if n_terms == 1:
        return False
    if name == "right_multiply":  # (the factors of ONE run are multiplied on the wrong side: a run needs two of them)
        return -(-n_steps // lanes) > 1 or order == 4
    if name == "reverse_combine":
        return n_steps > 1
    return True
