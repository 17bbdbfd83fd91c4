"""Pauli-word observables on the GPU: ``qmle_expval_pauli`` / ``_f64`` / ``qmle_density_expval_pauli``
(csrc/qmle_pauli.hip) against a NumPy complex128 reference that applies a word by flipping and signing axes
of the ``(2,) * n`` view of the state -- no index arithmetic in common with the kernels -- and the routes of
``Script.execute`` / ``Script.gradient`` / compiled calls that use them, against the oracle.

Tolerances: 1e-6 absolute for complex64 states (``test_expval_parity_groups_of_eight``), 1e-12 for complex128,
with unit-norm states and weights of at most 1 in magnitude.  Inputs are complex64 values (held in complex128
for the reference and for the complex128 kernels)."""
import os
import re

import numpy as np
import pytest

from oracle import einsum_sim as OE
from test_gpu_analysis_kernels import _states

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"c64": 1e-6, "c128": 1e-12}


def _N():
    from qml_essentials_amd import _native as N

    return N


def _tile_bits():
    """Registers of up to this many qubits stay in one workgroup's LDS (csrc/qmle_pauli.hip)."""
    src = open(os.path.join(ROOT, "qml-essentials_amd", "csrc", "qmle_pauli.hip")).read()
    return int(re.search(r"constexpr int kPauliTileBits = (\d+);", src).group(1))


def _dev(st, dtype):
    t = torch.from_numpy(np.ascontiguousarray(st))
    return (t.to(torch.complex64) if dtype == "c64" else t).cuda()


def ref_word(st, n, x_wires, z_wires):
    """<psi|P|psi> per state, P = i^ny X^x Z^z (Z first, then the flips), in complex128."""
    B = st.shape[0]
    psi = st.reshape((B,) + (2,) * n)
    phi = psi
    for w in range(n):
        if (z_wires >> w) & 1:
            shape = [1] * (n + 1)
            shape[1 + w] = 2
            phi = phi * np.array([1.0, -1.0]).reshape(shape)
    flips = [1 + w for w in range(n) if (x_wires >> w) & 1]
    if flips:
        phi = np.flip(phi, axis=flips)
    ny = bin(x_wires & z_wires).count("1")
    return np.real((1j ** ny) * np.sum(np.conj(psi) * phi, axis=tuple(range(1, n + 1))))


def ref_terms(st, n, terms, n_obs):
    out = np.zeros((st.shape[0], n_obs))
    cache = {}
    for coef, x, z, col in terms:
        if (x, z) not in cache:
            cache[(x, z)] = ref_word(st, n, x, z)
        out[:, col] += coef * cache[(x, z)]
    return out


def _wires(n, positions):
    m = 0
    for p in positions:
        if 0 <= p < n:
            m |= 1 << (n - 1 - p)
    return m


def single_words(n):
    """(x wires, z wires) of the single-word cases, by bit position (wire w = position n - 1 - w)."""
    top = n - 1
    words = [
        ([], []),                                   # identity
        ([0], []),                                  # X on wire n-1
        ([min(2, top)], []),                        # a position in 1..3
        ([min(4, top)], []),                        # position 4
        ([top], []),                                # X on wire 0: tile-id bits choose the partner tile
        ([top], [top]),                             # Y on wire 0
        ([0, top], [top // 2]),                     # low and high positions, Z in between
        ([top], list(range(n))),                    # Y on top, Z on every other position (tile-id bits too)
        ([], list(range(max(0, n - 4), n))),        # Z on the four highest positions
        ([], [0, top]),
        ([1 % n, top], [0, top // 2, top]),
        ([0, top], [0, top]),                       # 2 Y's
        ([0, 1 % n, top], [0, 1 % n, top]),         # 3 Y's (fewer on tiny registers)
        ([0, 1 % n, 2 % n, top], [0, 1 % n, 2 % n, top]),  # 4 Y's
        (list(range(n)), []),                       # X on every wire
        (list(range(min(n, 12))), [3 % n, top]),    # the widest word one tile holds
    ]
    return [(_wires(n, x), _wires(n, z)) for x, z in words]


def _run_and_check(n, B, terms, n_obs, dtype, seed=0):
    st = _states(np.random.default_rng(100 * n + B + seed), B, n)
    got = _N().expval_pauli(_dev(st, dtype), terms, n_obs).cpu().numpy()
    want = ref_terms(st, n, terms, n_obs)
    assert got.dtype == (np.float32 if dtype == "c64" else np.float64) and got.shape == want.shape
    err = np.abs(got - want).max()
    print(f"n={n} B={B} {dtype} terms={len(terms)} max err {err:.3e}")
    assert err <= TOL[dtype], (n, B, dtype, err)
    return got, want


@pytest.mark.parametrize("dtype", ["c64", "c128"])
def test_single_words_on_both_sides_of_the_tile_threshold(dtype):
    T = _tile_bits()
    sizes = [1, 2, 3, 5, T, T + 1, 16]
    N = _N()
    taken = set()
    for n in sizes:
        words = single_words(n)
        terms = [(1.0, x, z, k) for k, (x, z) in enumerate(words)]
        # the host code's rule: up to T qubits one workgroup holds the state (one read, whatever the word);
        # above, the word over all wires does not fit a tile and is streamed (two more reads)
        reads = N.pauli_reads(n, terms, f64=dtype == "c128")
        taken.add("whole" if n <= T else "tiled")
        assert (reads == 1) if n <= T else (reads >= 3), (n, reads)
        for B in (1, 3):
            got, want = _run_and_check(n, B, terms, len(words), dtype)
        assert np.abs(want[:, 0] - 1.0).max() < 1e-6   # the identity word: the norm
    assert taken == {"whole", "tiled"}


@pytest.mark.parametrize("dtype", ["c64", "c128"])
def test_four_phases_of_y_words(dtype):
    n = 6
    terms = []
    for k in range(1, 5):
        m = _wires(n, [0, 2, 4, 5][:k])
        terms.append((1.0, m, m, k - 1))
    got, want = _run_and_check(n, 3, terms, 4, dtype)
    assert np.abs(want).max() > 1e-3   # the words do not vanish on these states


@pytest.mark.parametrize("dtype", ["c64", "c128"])
def test_several_passes_add_into_one_column(dtype):
    N = _N()
    n = 14
    each = [(1.0, 1 << w, 0, w) for w in range(n)]
    assert N.pauli_reads(n, each) >= 2   # 10 positions above the lowest 4, 8 per pass
    _run_and_check(n, 3, each, n, dtype)
    # observables sharing an x mask; one observable with terms of both passes and a diagonal one;
    # columns 1 and 4 stay empty
    a, b = _wires(n, [4]), _wires(n, [13])
    terms = [(0.5, a, 0, 0), (-0.25, a, _wires(n, [4, 9]), 2), (0.75, a, _wires(n, [0]), 3),
             (0.3, b, 0, 0), (0.2, 0, _wires(n, [6, 13]), 0), (-0.6, b, b, 3), (1.0, b, 0, 5)]
    terms += [(0.1, 1 << w, 0, 0) for w in range(n)]
    assert N.pauli_reads(n, terms) >= 2
    got, _ = _run_and_check(n, 3, terms, 6, dtype, seed=1)
    assert np.all(got[:, [1, 4]] == 0.0)


@pytest.mark.parametrize("dtype", ["c64", "c128"])
def test_streamed_word_over_all_wires(dtype):
    N = _N()
    n = 14
    every = (1 << n) - 1
    terms = [(1.0, every, 0, 0)]
    assert N.pauli_reads(n, terms) == 2
    _run_and_check(n, 3, terms, 1, dtype)
    # the same x mask with nine sign patterns (more than one launch holds), mixed with tile terms
    rng = np.random.default_rng(2)
    terms = [(float(rng.uniform(-1, 1)), every, int(rng.integers(0, 1 << n)), k % 3) for k in range(9)]
    terms += [(0.5, 1, 0, 1), (0.5, 0, 5, 2)]
    assert N.pauli_reads(n, terms) == 3   # one launch for the nine, one tile pass
    _run_and_check(n, 2, terms, 3, dtype, seed=1)


@pytest.mark.parametrize("dtype", ["c64", "c128"])
@pytest.mark.parametrize("n_obs", [1, 9, 40])
def test_observable_counts_with_empty_columns(dtype, n_obs):
    n = 13
    rng = np.random.default_rng(n_obs)
    cols = sorted(set(range(0, n_obs, 3)) | {n_obs - 1})
    terms = [(float(rng.uniform(-1, 1)), int(rng.integers(0, 1 << n)) & _wires(n, range(12)),
              int(rng.integers(0, 1 << n)), c) for c in cols for _ in range(2)]
    got, _ = _run_and_check(n, 2, terms, n_obs, dtype)
    empty = [c for c in range(n_obs) if c not in cols]
    assert np.all(got[:, empty] == 0.0)


@pytest.mark.parametrize("dtype", ["c64", "c128"])
def test_batches_beyond_one_grid(dtype):
    n, B = 2, 70000
    terms = [(1.0, 1, 0, 0), (1.0, 2, 2, 1), (0.5, 3, 1, 2), (1.0, 0, 3, 2)]
    _run_and_check(n, B, terms, 3, dtype)


@pytest.mark.parametrize("dtype", ["c64", "c128"])
def test_two_calls_give_the_same_bits(dtype):
    N = _N()
    n = 14
    st = _dev(_states(np.random.default_rng(9), 3, n), dtype)
    terms = [(1.0, 1 << w, 0, w % 4) for w in range(n)] + [(0.5, (1 << n) - 1, 3, 1), (0.5, 0, 6, 2)]
    a = N.expval_pauli(st, terms, 4)
    b = N.expval_pauli(st, terms, 4)
    assert torch.equal(a, b)


def _index_mask(n, wire_mask):
    """Wire mask (bit w = wire w) -> mask of the basis index, whose most significant bit is wire 0."""
    return sum(((wire_mask >> w) & 1) << (n - 1 - w) for w in range(n))


def trace_of_word(rho, n, x, z):
    """Re Tr(P rho) per matrix, P = i^ny X^x Z^z: P[j ^ x, j] = i^ny (-1)^(j . z) are its only entries, so the trace
    gathers the 2^n elements rho[j, j ^ x] -- no 2^n x 2^n word matrix."""
    j = np.arange(1 << n)
    xi, zi = _index_mask(n, x), _index_mask(n, z)
    parity = np.zeros_like(j)
    for b in range(n):
        parity ^= ((j & zi) >> b) & 1
    sign = 1.0 - 2.0 * parity
    ny = bin(x & z).count("1")
    return np.real((1j ** ny) * (rho[:, j, j ^ xi].astype(np.complex128) * sign).sum(axis=1))


@pytest.mark.parametrize("n", [1, 2, 5, 9, 10])
def test_density_words_against_the_trace(n):
    """n = 9, 10: D = 2^n > 256 threads, so the kernel's loop over j makes two and four trips, with 200 random words
    whose x masks have high bits set."""
    from test_pauli_observables_cpu import word_matrix

    N = _N()
    rng = np.random.default_rng(n)
    D, B = 1 << n, 3
    rho = (rng.standard_normal((B, D, D)) + 1j * rng.standard_normal((B, D, D))).astype(np.complex64)
    rho /= np.abs(rho).sum(axis=(1, 2), keepdims=True)   # sum |rho_ij| = 1: every word is at most 1
    if n <= 5:
        words = [(x, z) for x, z in single_words(n)]
    else:
        # a random word of a random matrix is a sum of 2^n signed elements of size 4^-n: nothing to compare.  Most of
        # rho is therefore a product of 2 x 2 matrices, one per wire, each with one diagonal and one off-diagonal entry
        # of size 1/2 and a random phase: |Tr(P m)| = 1/2 for all four P, every word of the product has size 2^-n, and
        # an observable of 40 words comes to several 1e-3; sum |rho_ij| stays at most 1
        prod = np.ones((B, 1, 1), dtype=np.complex128)
        for _ in range(n):
            m = np.zeros((B, 2, 2), dtype=np.complex128)
            for b in range(B):
                d, r, c = rng.integers(0, 2, size=3)
                m[b, d, d], m[b, r, 1 - r] = 0.5 * np.exp(2j * np.pi * rng.random(2))
            prod = np.einsum("bij,bkl->bikjl", prod, m).reshape(B, 2 * prod.shape[1], 2 * prod.shape[2])
        rho = (0.1 * rho + 0.9 * prod).astype(np.complex64)
        words = [(int(x), int(z)) for x, z in rng.integers(0, 1 << n, size=(200, 2))]
        words[:3] = [(D - 1, 0), (D - 1, D - 1), (1 << (n - 1), 1)]  # X and Y on every wire; the index's low bit
    terms = [(1.0, x, z, k % 5) for k, (x, z) in enumerate(words)]   # every column's words straddle the launches
    terms += [(-0.125, x, z, 5) for x, z in words] * 4   # more terms than one launch takes
    want = np.zeros((B, 7))
    wires = list(range(n))
    for coef, x, z, col in terms:
        tr = trace_of_word(rho, n, x, z)
        if n <= 5:  # the gather is the trace with the word's matrix
            P = word_matrix(x, z, wires)
            full = np.real(np.trace(P[None] @ rho.astype(np.complex128), axis1=1, axis2=2))
            assert np.abs(tr - full).max() < 1e-14
        want[:, col] += coef * tr
    got = N.density_expval_pauli(torch.from_numpy(rho.reshape(B, D * D)).cuda(), n, terms, 7).cpu().numpy()
    err = np.abs(got - want).max()
    print(f"density n={n} max err {err:.3e}")
    assert err <= 1e-6 and np.all(got[:, 6] == 0.0)
    assert np.abs(want).max() > 1e-3


# ---- through the public interface --------------------------------------------------------------------
def _circuit_and_tape(n, theta):
    """A small entangling circuit on n wires and the oracle's tape of it."""
    from qml_essentials_amd import operations as op

    def circuit(th):
        for q in range(n):
            op.RY(th[q], wires=q)
        for q in range(n - 1):
            op.CX(wires=[q, q + 1])
        for q in range(n):
            op.RX(th[n + q], wires=q)
        op.CX(wires=[n - 1, 0])

    tape = ([("RY", [q], (theta[q],)) for q in range(n)] + [("CX", [q, q + 1], ()) for q in range(n - 1)]
            + [("RX", [q], (theta[n + q],)) for q in range(n)] + [("CX", [n - 1, 0], ())])
    return circuit, tape


def _observables(rng):
    from qml_essentials_amd import operations as op

    h = rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8))
    h = h + h.conj().T
    h /= np.linalg.norm(h, 2)   # spectral norm 1: an O(1) expectation value
    xyz = op.prod(op.PauliX(0, record=False), op.PauliY(1, record=False), op.PauliZ(2, record=False))
    obs = [op.PauliZ(0, record=False), op.PauliX(1, record=False), op.PauliY(2, record=False), xyz,
           op.Hermitian(h, wires=[3, 0, 2], record=False)]
    oracle = [("PauliZ", [0]), ("PauliX", [1]), ("PauliY", [2]),
              ("Matrix:", [0, 1, 2], np.asarray(xyz.matrix)), ("Matrix:", [3, 0, 2], h)]
    return obs, oracle


@pytest.mark.parametrize("n", [5, 14])
def test_execute_measures_pauli_and_three_wire_observables(n):
    from qml_essentials_amd.script import Script

    rng = np.random.default_rng(n)
    obs, oracle = _observables(rng)
    theta = rng.uniform(0, 2 * np.pi, 2 * n)
    circuit, tape = _circuit_and_tape(n, theta)
    got = Script(circuit, n_qubits=n).execute(type="expval", obs=obs, args=(theta,))
    want = OE.simulate_and_measure(tape, n, "expval", oracle, np.complex128)
    err = np.abs(got - want).max()
    print(f"execute n={n} max err {err:.3e}")
    assert got.dtype == np.float32 and err < 1e-6


@pytest.mark.parametrize("n", [5, 14])
def test_execute_in_x64(n):
    from qml_essentials_amd import utils
    from qml_essentials_amd.script import Script

    rng = np.random.default_rng(n)
    obs, oracle = _observables(rng)
    theta = rng.uniform(0, 2 * np.pi, (2, 2 * n))
    circuit, _ = _circuit_and_tape(n, theta[0])
    with utils.x64_scope(True):
        got = Script(circuit, n_qubits=n).execute(type="expval", obs=obs, args=(theta,), in_axes=(0,))
    want = np.stack([OE.simulate_and_measure(_circuit_and_tape(n, t)[1], n, "expval", oracle, np.complex128)
                     for t in theta])
    err = np.abs(got - want).max()
    print(f"x64 execute n={n} max err {err:.3e}")
    assert got.dtype == np.float64 and err < 1e-12


def test_noisy_circuit_measures_the_same_observables():
    from helpers import frontend_to_oracle
    from oracle import dense as OD
    from oracle import noise as ON
    from qml_essentials_amd import operations as op
    from qml_essentials_amd.script import Script
    from qml_essentials_amd.tape import shift_and_append
    from test_noise_cpu import _noisy_tape

    rng = np.random.default_rng(11)
    n = 3
    tape = _noisy_tape(rng)
    rho = ON.simulate_mixed(frontend_to_oracle(tape), n)
    h = rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8))
    h = h + h.conj().T
    h /= np.linalg.norm(h, 2)
    obs = [op.PauliZ(0, record=False), op.PauliX(1, record=False), op.PauliY(2, record=False),
           op.prod(op.PauliX(0, record=False), op.PauliY(1, record=False), op.PauliZ(2, record=False)),
           op.Hermitian(h, wires=[2, 0, 1], record=False)]
    dense = [OD.lift(np.asarray(o.matrix), o.wires, n) for o in obs]
    got = Script(f=lambda: shift_and_append(tape, 0), n_qubits=n).execute(type="expval", obs=obs)
    err = np.abs(got - ON.measure_density(rho, n, "expval", dense)).max()
    print(f"noisy max err {err:.3e}")
    assert err < 2e-6


def test_parameter_shift_gradient_of_x_and_y():
    from qml_essentials_amd import operations as op
    from qml_essentials_amd.script import Script

    n = 3
    rng = np.random.default_rng(4)
    theta = rng.uniform(0, 2 * np.pi, 2 * n)
    circuit, _ = _circuit_and_tape(n, theta)
    obs = [op.PauliX(0, record=False), op.PauliY(1, record=False)]
    (g,) = Script(circuit, n_qubits=n).gradient(obs, args=(theta,))

    def f(t):
        return OE.simulate_and_measure(_circuit_and_tape(n, t)[1], n, "expval", [("PauliX", [0]), ("PauliY", [1])],
                                       np.complex128)

    eps = 1e-6
    fd = np.stack([(f(theta + eps * e) - f(theta - eps * e)) / (2 * eps) for e in np.eye(2 * n)], axis=1)
    got = np.asarray(g)
    assert got.shape == fd.shape
    err = np.abs(got - fd).max()
    print(f"gradient max err {err:.3e}")
    assert err < 2e-5


def test_compiled_call_equals_the_recorded_path():
    from qml_essentials_amd.script import Script

    n = 5
    rng = np.random.default_rng(6)
    obs, _ = _observables(rng)
    theta = rng.uniform(0, 2 * np.pi, (3, 2 * n)).astype(np.float32)
    circuit, _ = _circuit_and_tape(n, theta[0])
    script = Script(circuit, n_qubits=n)
    cc = script.compiled("pauli", "expval", obs, (theta[0],), (0,))
    assert cc._measure()[0] == "pauli"
    got = cc.run([torch.from_numpy(theta).cuda()], [1], [3], 3)
    want = script.execute(type="expval", obs=obs, args=(theta,), in_axes=(0,))
    assert got.is_cuda and np.abs(got.cpu().numpy() - want).max() < 1e-6
