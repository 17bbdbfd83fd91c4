"""CPU-only: observables as weighted Pauli words (``operations.pauli_decompose`` / ``pauli_terms``), the
host planner of ``qmle_expval_pauli`` (how many times a term set streams the state) and the argument
checks of the new entry points, which are decided before any device work."""
import ctypes as C
from functools import reduce

import numpy as np
import pytest

from qml_essentials_amd import _native as N
from qml_essentials_amd import jaqsi
from qml_essentials_amd import operations as op

I2 = np.eye(2, dtype=np.complex128)
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)
Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)

ERR_INVALID_ARG, ERR_WIRE_RANGE = -1, -4


def word_matrix(x_mask, z_mask, wires):
    """i^ny X^x Z^z on ``wires`` (first wire = most significant factor), factor by factor."""
    facs = []
    for w in wires:
        f = I2
        if (x_mask >> w) & 1:
            f = f @ X
        if (z_mask >> w) & 1:
            f = f @ Z
        if (x_mask >> w) & (z_mask >> w) & 1:
            f = 1j * f
        facs.append(f)
    return reduce(np.kron, facs)


@pytest.mark.parametrize("wires", [[0], [3], [2, 0], [1, 4], [3, 0, 2], [5, 1, 2], [2, 7, 0, 4], [3, 2, 1, 0]])
def test_decomposition_rebuilds_a_random_hermitian_matrix(wires):
    rng = np.random.default_rng(17 + len(wires) + wires[0])
    d = 2 ** len(wires)
    a = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    m = (a + a.conj().T) / 2
    terms = op.pauli_decompose(m, wires)
    assert all(not ((x | z) & ~sum(1 << w for w in wires)) for _, x, z in terms)
    rebuilt = sum(c * word_matrix(x, z, wires) for c, x, z in terms)
    assert np.max(np.abs(rebuilt - m)) < 1e-12


def test_real_part_of_the_coefficients_is_the_hermitian_part():
    rng = np.random.default_rng(5)
    m = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
    rebuilt = sum(c * word_matrix(x, z, [1, 0]) for c, x, z in op.pauli_decompose(m, [1, 0]))
    assert np.max(np.abs(rebuilt - (m + m.conj().T) / 2)) < 1e-12


@pytest.mark.parametrize("n_y", [1, 2, 3, 4])
def test_y_is_i_x_z_on_every_wire_of_a_word(n_y):
    wires = list(range(n_y))
    mask = (1 << n_y) - 1
    assert np.array_equal(word_matrix(mask, mask, wires), reduce(np.kron, [Y] * n_y))
    terms = op.pauli_decompose(reduce(np.kron, [Y] * n_y), wires)
    assert terms == [(1.0, mask, mask)]
    # Y on wire 0 (x) X on wire 1 (x) Z on wire 2
    assert op.pauli_decompose(reduce(np.kron, [Y, X, Z]), [0, 1, 2]) == [(1.0, 0b011, 0b101)]


def test_pauli_terms_of_named_and_composed_observables():
    assert op.pauli_terms(op.PauliX(wires=2, record=False)) == [(1.0, 4, 0)]
    assert op.pauli_terms(op.PauliY(wires=1, record=False)) == [(1.0, 2, 2)]
    assert op.pauli_terms(op.PauliZ(wires=0, record=False)) == [(1.0, 0, 1)]
    assert op.pauli_terms(op.Id(wires=3, record=False)) == [(1.0, 0, 0)]
    assert op.pauli_terms(jaqsi.build_parity_observable([0, 3, 1])) == [(1.0, 0, 0b1011)]
    prod = op.prod(op.PauliX(wires=0, record=False), op.PauliY(wires=1, record=False),
                   op.PauliZ(wires=2, record=False))
    assert op.pauli_terms(prod) == [(1.0, 0b011, 0b110)]
    assert op.pauli_terms(0.5 * op.PauliX(wires=1, record=False)) == [(0.5, 2, 0)]
    # X0 X1 + Z0 Z1 through Operation.__add__
    both = (op.prod(op.PauliX(wires=0, record=False), op.PauliX(wires=1, record=False))
            + op.prod(op.PauliZ(wires=0, record=False), op.PauliZ(wires=1, record=False)))
    assert sorted(op.pauli_terms(both)) == [(1.0, 0, 3), (1.0, 3, 0)]


def test_observables_without_pauli_terms():
    batched = op.Operation(wires=0, matrix=np.stack([X, Z]), record=False)
    assert op.pauli_terms(batched) is None
    assert op.pauli_terms(op.RX(0.3, wires=0, record=False)) is None
    seven = op.Operation(wires=list(range(7)), matrix=np.eye(128), record=False)
    assert op.pauli_terms(seven) is None
    assert op.pauli_terms(op.BitFlip(0.1, wires=0)) is None


# ---- host planner: reads of the state ----------------------------------------------------------------
def _pos_mask(n, positions):
    """wire mask of a set of bit positions (wire w is position n - 1 - w)"""
    return sum(1 << (n - 1 - p) for p in positions)


def test_diagonal_terms_take_one_read():
    n = 24
    terms = [(1.0, 0, 1 << w, w) for w in range(n)] + [(0.5, 0, 3 << w, n + w) for w in range(n - 1)]
    assert N.pauli_reads(n, terms) == 1
    assert N.pauli_reads(n, terms, f64=True) == 1


@pytest.mark.parametrize("others", [[4, 5, 6, 7, 8, 9, 10, 11], [23, 22, 21, 20, 19, 18, 17, 16],
                                    [5, 9, 12, 13, 17, 20, 22, 23]])
def test_terms_inside_the_low_four_and_eight_other_positions_take_one_read(others):
    n = 24
    inside = [0, 1, 2, 3] + others
    terms = [(1.0, _pos_mask(n, [p]), 0, k) for k, p in enumerate(inside)]                    # X on each
    terms += [(1.0, _pos_mask(n, inside[k:k + 3]), _pos_mask(n, [inside[k], 14]), 12 + k) for k in range(9)]
    terms += [(1.0, _pos_mask(n, inside), _pos_mask(n, inside), 30)]                           # Y on all twelve
    terms += [(1.0, 0, _pos_mask(n, [15, 3]), 31)]
    assert N.pauli_reads(n, terms) == 1


@pytest.mark.parametrize("n", [1, 2, 5, 12])
def test_small_registers_always_take_one_read(n):
    every = (1 << n) - 1
    terms = [(1.0, every, 0, 0), (1.0, every, every, 1), (1.0, 1, 0, 2), (1.0, 0, every, 3)]
    terms += [(1.0, 1 << w, 0, 4 + w) for w in range(n)]
    assert N.pauli_reads(n, terms) == 1


def _ising(n):
    return ([(1.0, 1 << w, 0, w) for w in range(n)]
            + [(1.0, 0, 3 << w, n + w) for w in range(n - 1)])


def test_transverse_field_ising_at_24_qubits_takes_at_most_three_reads():
    assert 1 <= N.pauli_reads(24, _ising(24)) <= 3   # 20 positions above the lowest 4, 8 per pass


def test_a_word_wider_than_a_tile_is_streamed():
    r = N.pauli_reads(14, [(1.0, (1 << 14) - 1, 0, 0)])
    assert 1 <= r <= 2


def test_every_term_of_a_wide_x_mask_shares_its_two_reads():
    n = 14
    every = (1 << n) - 1
    rng = np.random.default_rng(8)
    for k in (9, 64, 300):   # more terms than any fixed group of registers holds
        terms = [(1.0, every, int(rng.integers(0, 1 << n)), j % 7) for j in range(k)]
        assert N.pauli_reads(n, terms) == 2
        assert N.pauli_reads(n, terms + [(1.0, 0, 3, 0), (1.0, 1, 0, 1)]) == 3
    two = [(1.0, every, j, 0) for j in range(20)] + [(1.0, every ^ 1, j, 1) for j in range(20)]
    assert N.pauli_reads(n, two) == 4


def test_reads_are_bounded_by_the_distinct_x_masks():
    rng = np.random.default_rng(3)
    for n in (13, 18, 24, 30):
        for _ in range(20):
            k = int(rng.integers(1, 40))
            masks = [int(rng.integers(0, 1 << n)) for _ in range(4)]   # few masks, many terms on each
            terms = [(float(rng.uniform(-1, 1)), masks[int(rng.integers(0, 4))] if rng.random() < 0.8 else 0,
                      int(rng.integers(0, 1 << n)), int(rng.integers(0, 5))) for _ in range(k)]
            distinct = len({x for _, x, _, _ in terms if x})
            assert 1 <= N.pauli_reads(n, terms) <= 2 * distinct + 1


def test_masks_beyond_32_wires_are_refused_not_truncated():
    with pytest.raises(ValueError):
        N.pauli_term_array([(1.0, 1 << 32, 0, 0)])
    with pytest.raises(ValueError):
        N.pauli_term_array([(1.0, 0, 1 << 40, 0)])
    assert not N.pauli_terms_supported(30, [(1.0, 1 << 33, 0, 0)])
    assert N.pauli_terms_supported(30, [(1.0, 1 << 29, 1, 0)])
    assert not N.pauli_terms_supported(31, [(1.0, 1, 1, 0)])                       # qubits
    assert not N.pauli_terms_supported(4, [(1.0, 1, 1, 4096)])                     # observables
    assert not N.pauli_terms_supported(4, [(1.0, 1, 1, 0)] * 65537)                # terms


# ---- argument checks, decided on the host ------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_touching_a_device():
    lib = N.lib()
    good = N.pauli_term_array([(1.0, 1, 2, 0)])
    buf = C.c_void_p(256)  # never dereferenced: every call below is refused on the host
    big = 1 << 40

    def call(fn, states=buf, n=4, batch=1, terms=good, n_terms=1, n_obs=1, out=buf, ws=buf, wsb=big):
        return fn(states, n, batch, terms, n_terms, n_obs, out, ws, wsb, None)

    for fn in (lib.qmle_expval_pauli, lib.qmle_expval_pauli_f64):
        assert call(fn, states=None) == ERR_INVALID_ARG
        assert call(fn, out=None) == ERR_INVALID_ARG
        assert call(fn, ws=None) == ERR_INVALID_ARG
        assert call(fn, terms=None) == ERR_INVALID_ARG
        assert call(fn, batch=0) == ERR_INVALID_ARG
        for n_terms in (0, -1, 65537):
            assert call(fn, n_terms=n_terms) == ERR_INVALID_ARG
        for n_obs in (0, 4097):
            assert call(fn, n_obs=n_obs) == ERR_INVALID_ARG
        for n in (0, 31):
            assert call(fn, n=n) == ERR_INVALID_ARG
        assert call(fn, terms=N.pauli_term_array([(1.0, 1, 0, 1)])) == ERR_INVALID_ARG     # obs == n_obs
        assert call(fn, terms=N.pauli_term_array([(1.0, 1, 0, -1)])) == ERR_INVALID_ARG
        assert call(fn, terms=N.pauli_term_array([(1.0, 1 << 4, 0, 0)])) == ERR_WIRE_RANGE  # wire 4 of 4 qubits
        assert call(fn, terms=N.pauli_term_array([(1.0, 0, 1 << 31, 0)])) == ERR_WIRE_RANGE
    need = lib.qmle_expval_pauli_workspace_bytes(4, 1, 1, 1)
    need64 = lib.qmle_expval_pauli_workspace_bytes_f64(4, 1, 1, 1)
    assert need > 0 and need64 > 0
    assert call(lib.qmle_expval_pauli, wsb=need - 1) == ERR_INVALID_ARG
    assert call(lib.qmle_expval_pauli_f64, wsb=need64 - 1) == ERR_INVALID_ARG

    def dens(rho=buf, n=2, batch=1, terms=good, n_terms=1, n_obs=1, out=buf):
        return lib.qmle_density_expval_pauli(rho, n, batch, terms, n_terms, n_obs, out, None)

    assert dens(rho=None) == ERR_INVALID_ARG and dens(out=None) == ERR_INVALID_ARG
    assert dens(terms=None) == ERR_INVALID_ARG and dens(batch=0) == ERR_INVALID_ARG
    assert dens(n_terms=0) == ERR_INVALID_ARG and dens(n_terms=65537) == ERR_INVALID_ARG
    assert dens(n_obs=0) == ERR_INVALID_ARG and dens(n_obs=4097) == ERR_INVALID_ARG
    assert dens(n=0) == ERR_INVALID_ARG and dens(n=17) == ERR_INVALID_ARG
    assert dens(terms=N.pauli_term_array([(1.0, 1, 0, 1)])) == ERR_INVALID_ARG
    assert dens(terms=N.pauli_term_array([(1.0, 4, 0, 0)])) == ERR_WIRE_RANGE

    assert lib.qmle_expval_pauli_reads(4, None, 1, 0) == ERR_INVALID_ARG
    assert lib.qmle_expval_pauli_reads(31, good, 1, 0) == ERR_INVALID_ARG
    assert lib.qmle_expval_pauli_reads(1, good, 1, 0) == ERR_WIRE_RANGE
