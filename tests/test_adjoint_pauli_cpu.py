"""CPU-only: the entry points of the Pauli-word adjoint seed (``qmle_apply_pauli_sum``,
``qmle_adjoint_gradient_pauli`` and their complex128 twins) are exported, refuse bad arguments before any
device work, plan their reads on the host, and ``Script.vjp`` routes observable lists to the right seed."""
import ctypes as C

import numpy as np
import pytest

from qml_essentials_amd import _native as N
from qml_essentials_amd import adjoint, jaqsi
from qml_essentials_amd import operations as op
from qml_essentials_amd.script import Script

ERR_INVALID_ARG, ERR_WIRE_RANGE = -1, -4

NEW_SYMBOLS = ["qmle_apply_pauli_sum", "qmle_apply_pauli_sum_f64", "qmle_apply_pauli_sum_workspace_bytes",
               "qmle_apply_pauli_sum_workspace_bytes_f64", "qmle_apply_pauli_sum_reads",
               "qmle_adjoint_gradient_pauli", "qmle_adjoint_gradient_pauli_f64",
               "qmle_adjoint_pauli_workspace_bytes", "qmle_adjoint_pauli_workspace_bytes_f64"]


def test_the_nine_new_symbols_resolve():
    lib = N.lib()
    bound = {name for name, _, _ in N.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in bound and hasattr(lib, name), name


def test_y_is_i_x_z_in_the_apply_formula():
    """(P psi)[i] = i^ny (-1)^popc((i ^ x) & z) psi[i ^ x] on one qubit, x = z = 1:
    (Y psi)[1] = i psi[0], (Y psi)[0] = -i psi[1]."""
    psi = np.array([0.3 + 0.1j, -0.2 + 0.7j])
    out = np.array([1j * (-1) ** bin((i ^ 1) & 1).count("1") * psi[i ^ 1] for i in range(2)])
    assert np.allclose(out, np.array([[0, -1j], [1j, 0]]) @ psi)


# ---- argument checks, decided on the host ------------------------------------------------------------
def test_apply_refuses_bad_arguments_before_touching_a_device():
    lib = N.lib()
    good = N.pauli_term_array([(1.0, 1, 2, 0)])
    buf, other = C.c_void_p(256), C.c_void_p(1 << 20)  # never dereferenced: every call is refused on the host
    big = 1 << 40

    def call(fn, states=buf, n=4, batch=1, terms=good, n_terms=1, n_obs=1, weights=buf, out=other, ws=buf, wsb=big):
        return fn(states, n, batch, terms, n_terms, n_obs, weights, out, ws, wsb, None)

    for fn, wsq in ((lib.qmle_apply_pauli_sum, lib.qmle_apply_pauli_sum_workspace_bytes),
                    (lib.qmle_apply_pauli_sum_f64, lib.qmle_apply_pauli_sum_workspace_bytes_f64)):
        for name in ("states", "out", "ws", "weights", "terms"):
            assert call(fn, **{name: None}) == ERR_INVALID_ARG, name
        assert call(fn, batch=0) == ERR_INVALID_ARG
        for n_terms in (0, 65537):
            assert call(fn, n_terms=n_terms) == ERR_INVALID_ARG
        for n_obs in (0, 4097):
            assert call(fn, n_obs=n_obs) == ERR_INVALID_ARG
        for n in (0, 31):
            assert call(fn, n=n) == ERR_INVALID_ARG
        assert call(fn, terms=N.pauli_term_array([(1.0, 1, 0, 1)])) == ERR_INVALID_ARG      # obs == n_obs
        assert call(fn, terms=N.pauli_term_array([(1.0, 1 << 4, 0, 0)])) == ERR_WIRE_RANGE  # a mask bit at n_qubits
        assert call(fn, terms=N.pauli_term_array([(1.0, 0, 1 << 4, 0)])) == ERR_WIRE_RANGE
        assert call(fn, out=buf) == ERR_INVALID_ARG                                          # d_out == d_states
        need = wsq(4, 1, 1, 1)
        assert need > 0
        assert call(fn, wsb=need - 1) == ERR_INVALID_ARG
    assert lib.qmle_apply_pauli_sum_reads(4, None, 1, 0) == ERR_INVALID_ARG
    assert lib.qmle_apply_pauli_sum_reads(31, good, 1, 0) == ERR_INVALID_ARG
    assert lib.qmle_apply_pauli_sum_reads(4, N.pauli_term_array([(1.0, 16, 0, 0)]), 1, 0) == ERR_WIRE_RANGE


def test_adjoint_entry_points_refuse_bad_observable_terms_before_touching_a_device():
    lib = N.lib()
    plan = N.Plan([("RX", [0], [0], -1)], 4, 1)
    good = N.pauli_term_array([(1.0, 1, 2, 0)])
    gterm = N._adjoint_term_array([(0, 1, 0, 0, 0, 1.0, -1)])
    buf = C.c_void_p(256)
    big = 1 << 40

    def call(fn, terms=good, n_terms=1, n_obs=1, ws=buf, wsb=big):
        return fn(plan._h, plan._h, buf, buf, 1, buf, terms, n_terms, n_obs, gterm, 1, buf, 1, ws, wsb, None)

    for fn, wsq in ((lib.qmle_adjoint_gradient_pauli, lib.qmle_adjoint_pauli_workspace_bytes),
                    (lib.qmle_adjoint_gradient_pauli_f64, lib.qmle_adjoint_pauli_workspace_bytes_f64)):
        assert call(fn, terms=None) == ERR_INVALID_ARG and call(fn, ws=None) == ERR_INVALID_ARG
        for n_terms in (0, 65537):
            assert call(fn, n_terms=n_terms) == ERR_INVALID_ARG
        for n_obs in (0, 4097):
            assert call(fn, n_obs=n_obs) == ERR_INVALID_ARG
        assert call(fn, terms=N.pauli_term_array([(1.0, 1, 0, 1)])) == ERR_INVALID_ARG
        assert call(fn, terms=N.pauli_term_array([(1.0, 1 << 4, 0, 0)])) == ERR_WIRE_RANGE
        need = wsq(plan._h, plan._h, 1, 1, 1)
        assert need > 0
        assert call(fn, wsb=need - 1) == ERR_INVALID_ARG
    # the seed's tables come on top of the Z sweep's workspace
    assert (lib.qmle_adjoint_pauli_workspace_bytes(plan._h, plan._h, 1, 1, 1)
            > lib.qmle_adjoint_workspace_bytes(plan._h, plan._h, 1))


# ---- host planner: reads of the state ----------------------------------------------------------------
def _pos_mask(n, positions):
    """wire mask of a set of bit positions (wire w is position n - 1 - w)"""
    return sum(1 << (n - 1 - p) for p in positions)


def test_reads_follow_the_planner():
    """The planner's rule (csrc/qmle_pauli.hip): up to 12 qubits the tile is the state -- 1 read; diagonal words
    join the first pass -- 1; a pass holds the lowest 4 positions and at most 8 further positions of X/Y support,
    so ten single-X words on positions 4..13 are cut after the eighth -- 2 passes; a word whose own support needs
    10 > 8 positions above the lowest 4 is streamed, psi[i] and psi[i ^ x] -- 2 reads for its x mask."""
    every12 = (1 << 12) - 1
    any12 = [(1.0, every12, 0, 0), (0.5, every12, every12, 1), (1.0, 1, 0, 2), (1.0, 0, every12, 0)]
    any12 += [(1.0, 1 << w, 1 << (11 - w), 3) for w in range(12)]
    assert N.apply_pauli_reads(12, any12) == 1 and N.apply_pauli_reads(12, any12, f64=True) == 1
    diag = [(1.0, 0, 1 << w, w) for w in range(20)] + [(0.5, 0, 3 << w, 20 + w) for w in range(19)]
    assert N.apply_pauli_reads(20, diag) == 1
    ten = [(1.0, _pos_mask(14, [p]), 0, k) for k, p in enumerate(range(4, 14))]
    assert N.apply_pauli_reads(14, ten) == 2
    assert N.apply_pauli_reads(14, [(1.0, (1 << 14) - 1, 0, 0)]) == 2
    # terms with equal (x, z) are one word, whatever their observables
    assert N.apply_pauli_reads(14, [(1.0, (1 << 14) - 1, 5, k) for k in range(7)]) == 2


# ---- Script.vjp: which seed an observable list takes ---------------------------------------------------
def _circuit(th):
    for q in range(6):
        op.RY(th[q], wires=q)
    op.CX(wires=[0, 1])


@pytest.fixture
def seen(monkeypatch):
    calls = []

    def fake(low, n_qubits, batch, obs_groups, weights, want, x64=False, obs_terms=None):
        calls.append((obs_groups, obs_terms))
        return np.zeros((np.shape(weights)[0], low.n_slots))

    monkeypatch.setattr(adjoint, "adjoint_slot_gradient", fake)
    return calls


def _parities(k):
    groups = [[q] for q in range(6)] + [[a, b] for a in range(6) for b in range(a + 1, 6)] \
        + [[a, b, c] for a in range(6) for b in range(a + 1, 6) for c in range(b + 1, 6)]
    return [op.PauliZ(wires=g[0], record=False) if len(g) == 1 else jaqsi.build_parity_observable(g)
            for g in groups[:k]]


def test_vjp_keeps_the_z_seed_for_at_most_32_parities(seen):
    s = Script(_circuit, n_qubits=6)
    th = np.linspace(0.1, 1.0, 6)
    for k in (1, 32):
        s.vjp(_parities(k), np.ones(k), args=(th,))
        groups, terms = seen[-1]
        assert terms is None and len(groups) == k


def test_vjp_takes_the_term_list_for_everything_else(seen):
    s = Script(_circuit, n_qubits=6)
    th = np.linspace(0.1, 1.0, 6)
    s.vjp(_parities(33), np.ones(33), args=(th,))
    groups, terms = seen[-1]
    assert groups is None and len(terms) == 33 and all(x == 0 for _, x, _, _ in terms)
    rng = np.random.default_rng(2)
    a = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
    for obs in ([op.PauliX(wires=0, record=False)], [op.PauliY(wires=3, record=False)],
                [op.Hermitian(matrix=(a + a.conj().T) / 2, wires=[1, 4], record=False)],
                [op.PauliZ(wires=0, record=False), op.PauliX(wires=5, record=False)]):
        s.vjp(obs, np.ones(len(obs)), args=(th,), pauli_seed=True)
        groups, terms = seen[-1]
        assert groups is None and terms, obs
        assert {col for _, _, _, col in terms} == set(range(len(obs)))


def test_vjp_still_refuses_observables_without_pauli_terms(seen):
    s = Script(_circuit, n_qubits=6)
    th = np.linspace(0.1, 1.0, 6)
    with pytest.raises(adjoint.AdjointUnsupported, match="RX"):
        s.vjp([op.PauliZ(wires=0, record=False), op.RX(0.3, wires=0, record=False)], np.ones(2), args=(th,),
              pauli_seed=True)
    assert not seen


def test_vjp_keeps_its_refusal_of_non_z_observables_without_the_flag(seen):
    """The Pauli seed is asked for (``pauli_seed=True``): callers that rely on ``AdjointUnsupported`` for an
    X / Y / Hermitian observable to fall back to the parameter-shift Jacobian keep getting it."""
    s = Script(_circuit, n_qubits=6)
    th = np.linspace(0.1, 1.0, 6)
    with pytest.raises(adjoint.AdjointUnsupported, match="pauli_seed"):
        s.vjp([op.PauliX(wires=0, record=False)], np.ones(1), args=(th,))
    assert not seen
