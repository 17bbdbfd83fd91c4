"""CPU-only checks for dense matrices and Hamiltonian evolution on three and four wires: the NumPy references the
GPU tests compare against (tests/wide_gate_reference.py, tests/evolution_reference.py at dim 8 and 16) are right and
tell their own wrong variants apart on every GPU case; the argument errors of ``qmle_apply_matrix`` and
``qmle_evolve_magnus_wide`` are statuses without a device; the tape splitter; the refusals that stay; and the
resource figures of the two kernels."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import evolution_reference as R
import wide_gate_reference as W
from qml_essentials_amd import _native as N
from qml_essentials_amd import operations as op
from qml_essentials_amd import simulation
from qml_essentials_amd.operations import embed_matrix, is_wide_matrix_gate
from qml_essentials_amd.tape import recording

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z, X = R.Z, R.X


# ---- the reference of the apply pass -----------------------------------------------------------------------------
@pytest.mark.parametrize("k,n,wires", [(3, 3, [2, 0, 1]), (3, 5, [4, 0, 2]), (3, 6, [1, 5, 3]), (4, 4, [3, 1, 0, 2]),
                                       (4, 6, [5, 0, 3, 2]), (4, 7, [2, 6, 4, 1])])
def test_reference_apply_is_the_embedded_matrix(k, n, wires):
    rng = np.random.default_rng(k * 100 + n)
    U, psi = W.random_unitaries(rng, 1 << k, 2), W.random_states(rng, 2, n)
    full = [embed_matrix(U[b], wires, range(n)) for b in range(2)]
    want = np.stack([full[b] @ psi[b] for b in range(2)])
    assert np.abs(W.apply(psi, U, wires, n) - want).max() <= 1e-14
    assert np.abs(W.apply(psi, U[0], wires, n) - np.stack([full[0] @ psi[b] for b in range(2)])).max() <= 1e-14


def test_every_gpu_case_of_the_apply_pass_tells_every_wrong_variant_apart():
    """The rule of tests/test_x64_reference_cpu.py: a GPU result within 2e-6 (complex64) or 1e-12 (complex128) of the
    reference rules a variant out only if the variant is at least 1e-6 of the largest amplitude away on that case."""
    closest = {v: np.inf for v in W.VARIANTS}
    for name, k, n, wires, batch, per_sample in W.apply_cases():
        U, psi = W.case_data(k, n, batch, per_sample)
        want = W.apply(psi, U, wires, n)
        scale = np.abs(want).max()
        for v in W.VARIANTS:
            if not W.variant_applies(v, per_sample, batch, wires, n):
                continue
            gap = np.abs(W.apply(psi, U, wires, n, variant=v) - want).max() / scale
            closest[v] = min(closest[v], gap)
            assert gap >= 1e-6, (name, v, gap)
    print(closest)
    assert all(np.isfinite(g) for g in closest.values())  # every variant applied somewhere


def test_wire_sets_cover_the_top_the_bottom_and_an_order_that_is_not_sorted():
    for k in (3, 4):
        for n in W.SIZES[k]:
            sets = W.wire_sets(k, n)
            for wires in sets.values():
                assert len(set(wires)) == k and all(0 <= w < n for w in wires)
            assert n - 1 in sets["bottom"] and 0 in sets["top"]  # position 0 / the top position
            assert sets["permuted"] != sorted(sets["permuted"])


# ---- the reference of the solver at dim 8 and 16 -------------------------------------------------------------------
def _lanes_of_case(dim, rows, n_steps):
    auto = N.lib().qmle_evolve_wide_lanes(rows, n_steps, dim)
    return [auto if lanes == 0 else lanes for lanes in W.SOLVER_LANES[dim]]


@pytest.mark.parametrize("name,dim,n_terms,rows,n_steps,order", W.solver_cases(), ids=[c[0] for c in W.solver_cases()])
def test_every_gpu_case_of_the_solver_is_sized_and_discriminating(name, dim, n_terms, rows, n_steps, order):
    c = W.solver_case(dim, n_terms, rows, n_steps, order)
    assert c["H"].shape == (n_terms, dim, dim) and len(set(c["words"])) == n_terms
    assert np.abs(c["H"] - np.conj(np.swapaxes(c["H"], -1, -2))).max() == 0.0
    # the sizing rule of tests/test_gpu_evolution.py: h |sum c_i H_i| below about 15 even with one step
    A = np.einsum("rnt,tij->rnij", c["coef"], c["H"])
    norms = n_steps * c["h"][:, None] * np.linalg.norm(A, ord=2, axis=(-2, -1))
    assert norms.max() <= 15.0 and norms.max() >= 1.0, norms.max()
    shown = set()
    for lanes in sorted(set(_lanes_of_case(dim, rows, n_steps))):
        want = R.magnus(c["H"], c["coef"], c["h"], order, lanes=lanes)
        assert np.abs(np.einsum("rji,rjk->rik", want.conj(), want) - np.eye(dim)).max() <= 1e-13
        for v in R.VARIANTS:
            if not W.solver_variant_applies(v, order, rows, lanes, n_steps, n_terms):
                continue
            gap = np.abs(R.magnus(c["H"], c["coef"], c["h"], order, lanes=lanes, variant=v) - want).max()
            shown.add(v)
            assert gap >= 1e-6, (name, lanes, v, gap)
    assert shown or (rows == 1 and n_terms == 1)  # (one row of one term: a single commuting family, nothing to mix up)


def test_every_variant_of_the_scheme_is_shown_by_some_gpu_case():
    shown = set()
    for _name, dim, n_terms, rows, n_steps, order in W.solver_cases():
        for lanes in _lanes_of_case(dim, rows, n_steps):
            shown |= {v for v in R.VARIANTS if W.solver_variant_applies(v, order, rows, lanes, n_steps, n_terms)}
    assert shown == set(R.VARIANTS)


def test_the_numpy_scheme_agrees_with_mpmath_at_dim_16():
    """The yardstick of the 1e-12 bar: ``evolution_reference.magnus`` (float64, scipy's expm) against the same grid in
    40-digit arithmetic with ``mpmath.expm``, on the dim-16, order-4 case with the most steps, one row.  1e-13 here
    leaves the GPU comparison a margin of 10."""
    import mpmath as mp

    cases = [c for c in W.solver_cases() if c[1] == 16 and c[5] == 4 and c[2] == 16]
    _name, dim, n_terms, rows, n_steps, order = max(cases, key=lambda c: c[4])
    assert n_steps == 64
    c = W.solver_case(dim, n_terms, rows, n_steps, order)
    want = R.magnus(c["H"], c["coef"][:1], c["h"][:1], order)[0]
    mp.mp.dps = 40
    s3 = mp.sqrt(3)
    a1, a2 = mp.mpf(1) / 4 + s3 / 6, mp.mpf(1) / 4 - s3 / 6
    H = [mp.matrix(h.tolist()) for h in c["H"]]
    hh = mp.mpf(float(c["h"][0]))
    U = mp.eye(dim)
    for s in range(n_steps):
        A = []
        for node in (2 * s, 2 * s + 1):
            m = mp.zeros(dim)
            for t in range(n_terms):
                m += mp.mpf(float(c["coef"][0, node, t])) * H[t]
            A.append(-1j * m)
        U = mp.expm(hh * (a1 * A[0] + a2 * A[1])) * U
        U = mp.expm(hh * (a2 * A[0] + a1 * A[1])) * U
    got = np.array([[complex(U[i, j]) for j in range(dim)] for i in range(dim)])
    err = np.abs(got - want).max()
    print("mpmath vs numpy scheme", err)
    assert err <= 1e-13


# ---- status codes without a device -----------------------------------------------------------------------------------
def test_apply_matrix_argument_errors_are_statuses_without_a_device():
    lib = N.lib()
    null = C.c_void_p(None)
    one = C.c_void_p(16)  # a non-NULL pointer that is never followed: every call below is refused first

    def call(states=one, n=5, batch=1, f64=0, wires=(0, 1, 2), k=None, mats=one, per_sample=0):
        k = len(wires) if k is None else k
        w = None if wires is None else (C.c_int32 * max(1, len(wires)))(*wires)
        return lib.qmle_apply_matrix(states, n, batch, f64, w, k, mats, per_sample, null)

    assert call(wires=(0, 1)) == -10 and call(wires=(0, 1, 2, 3, 4)) == -10 and call(wires=(0,)) == -10  # UNSUPPORTED
    assert call(wires=(), k=0) == -10 and call(wires=(0, 1, 2), k=-3) == -10
    assert call(wires=(0, 1, 5)) == -4 and call(wires=(0, -1, 2)) == -4 and call(wires=(0, 1, 2, 7)) == -4  # WIRE_RANGE
    assert call(wires=(0, 1, 1)) == -3 and call(wires=(3, 1, 2, 3)) == -3                                  # DUPLICATE
    assert call(states=null) == -1 and call(mats=null) == -1 and call(wires=None, k=3) == -1               # INVALID_ARG
    assert call(batch=0) == -1 and call(batch=-2) == -1
    assert call(n=2) == -1 and call(n=3, wires=(0, 1, 2, 3)) == -1 and call(n=33) == -1
    assert call(f64=2) == -1 and call(per_sample=2) == -1
    # the wider refusal comes first: five wires are unsupported whatever else is wrong with the call
    assert call(states=null, wires=(0, 1, 2, 3, 4)) == -10
    with pytest.raises(ValueError):
        N.check(-4, "qmle_apply_matrix")


def test_evolve_magnus_wide_argument_errors_are_statuses_without_a_device():
    lib = N.lib()
    null = C.c_void_p(None)
    one = C.c_void_p(16)

    def call(terms=one, n_terms=1, dim=8, coef=one, hh=one, rows=1, order=4, n_steps=1, lanes=0, out=one):
        return lib.qmle_evolve_magnus_wide(terms, n_terms, dim, coef, hh, rows, order, n_steps, lanes, out, null)

    assert call(dim=2) == -10 and call(dim=4) == -10 and call(dim=32) == -10 and call(dim=12) == -10  # UNSUPPORTED
    assert call(order=3) == -10 and call(dim=16, order=1) == -10
    assert call(n_steps=0) == -1 and call(rows=0) == -1 and call(n_terms=0) == -1 and call(n_terms=17) == -1
    assert call(terms=null) == -1 and call(coef=null) == -1 and call(hh=null) == -1 and call(out=null) == -1
    # lanes * dim <= 64: {1, 4, 8} at dim 8, {1, 4} at dim 16
    assert call(lanes=2) == -1 and call(lanes=16) == -1 and call(dim=16, lanes=8) == -1 and call(lanes=-1) == -1
    assert call(rows=2 ** 30, lanes=8) == -1 and call(dim=16, rows=2 ** 30, lanes=4) == -1
    # lanes_per_row = 0: the widest allowed split that fills the card and leaves every run a step
    assert lib.qmle_evolve_wide_lanes(1, 8192, 8) == 8 and lib.qmle_evolve_wide_lanes(1, 8192, 16) == 4
    assert lib.qmle_evolve_wide_lanes(1, 5, 8) == 4 and lib.qmle_evolve_wide_lanes(1, 3, 16) == 1
    assert lib.qmle_evolve_wide_lanes(102400, 256, 8) == 1 and lib.qmle_evolve_wide_lanes(1024, 256, 16) == 4
    assert lib.qmle_evolve_wide_lanes(0, 1, 8) == -1 and lib.qmle_evolve_wide_lanes(1, 1, 4) == -10


def test_evolve_magnus_keeps_refusing_dim_8():
    H = np.zeros((1, 8, 8), dtype=np.complex128)
    one = C.c_void_p(16)
    assert N.lib().qmle_evolve_magnus(C.c_void_p(H.ctypes.data), 1, 8, one, one, 1, 4, 1, 0, 1, one, C.c_void_p(None)) == -10


# ---- the predicate and the tape splitter -----------------------------------------------------------------------------
def _u(k, seed=0, batch=None):
    return W.random_unitaries(np.random.default_rng(seed), 1 << k, batch)


def test_the_predicate_names_explicit_matrices_on_three_and_four_wires_only():
    with recording() as tape:
        op.RX(0.3, wires=0)
        op.CCX(wires=[0, 1, 2])
        op.CSWAP(wires=[2, 0, 1])
        op.Operation(wires=[0, 1], matrix=W.random_unitaries(np.random.default_rng(1), 4))
        op.Operation(wires=[0, 1, 2], matrix=_u(3))
        op.Operation(wires=[3, 1, 2, 0], matrix=_u(4, batch=5))
        op.Operation(wires=[0, 1, 2, 3, 4], matrix=np.eye(32))
        op.Barrier(wires=[0, 1, 2])
        op.BitFlip(0.1, wires=0)
    assert [is_wide_matrix_gate(o) for o in tape] == [False, False, False, False, True, True, False, False, False]
    P = op.prod(op.CX(wires=[0, 1], record=False), op.CX(wires=[1, 2], record=False))
    assert is_wide_matrix_gate(P) and is_wide_matrix_gate(P.dagger()) and is_wide_matrix_gate(P.power(2))
    assert simulation._tape_batch(tape[:6]) == 5
    for o in (tape[4], tape[5], P):  # no plan holds such a gate: lowering keeps refusing it
        with pytest.raises(NotImplementedError, match="not supported"):
            o.lower(5)


def test_the_tape_splitter_cuts_at_wide_gates():
    def tape_of(pattern):  # g: an ordinary gate, W: a wide one
        with recording() as tape:
            for c in pattern:
                if c == "g":
                    op.RY(0.1, wires=1)
                else:
                    op.Operation(wires=[0, 1, 2], matrix=_u(3))
        return tape

    for pattern, lengths, positions in (("ggg", [3], []), ("Wgg", [0, 2], [0]), ("ggW", [2, 0], [2]),
                                        ("gWWg", [1, 0, 1], [1, 2]), ("W", [0, 0], [0]), ("", [0], []),
                                        ("gWgWg", [1, 1, 1], [1, 3])):
        tape = tape_of(pattern)
        segments, pos = simulation.split_at_wide_gates(tape)
        assert [len(s) for s in segments] == lengths and pos == positions, pattern
        assert len(segments) == len(pos) + 1
        rebuilt = []
        for i, seg in enumerate(segments):  # segments and gates interleave to the tape again
            rebuilt += seg + ([tape[pos[i]]] if i < len(pos) else [])
        assert all(a is b for a, b in zip(rebuilt, tape)) and len(rebuilt) == len(tape)


# ---- refusals that stay (all raised on the host, before any device work) -----------------------------------------------
def test_five_wires_noisy_tapes_and_gradients_stay_refused():
    from qml_essentials_amd.script import Script

    H3 = np.kron(np.kron(Z, Z), X)
    obs = [op.PauliZ(wires=0, record=False)]

    def five():
        op.Operation(wires=[0, 1, 2, 3, 4], matrix=np.eye(32))

    with recording() as tape:
        five()
    with pytest.raises(NotImplementedError, match="generic 5-qubit"):
        simulation.LoweredTape(tape, 5)
    assert simulation.split_at_wide_gates(tape)[1] == []

    def wide(th):
        op.RX(th, wires=0)
        op.Operation(wires=[0, 1, 2], matrix=_u(3))

    with pytest.raises(NotImplementedError, match="generic 3-qubit"):
        Script(f=wide, n_qubits=3).vjp(obs, np.ones(1), args=(np.array(0.3),))
    with pytest.raises(NotImplementedError, match="generic 3-qubit"):
        Script(f=wide, n_qubits=3).gradient(obs, args=(np.array(0.3),))
    with pytest.raises(NotImplementedError, match="generic 3-qubit"):
        Script(f=wide, n_qubits=3).compiled("k", "expval", obs, (np.array(0.3),), (0,))

    def three_wires(s):
        op.Hermitian(H3, [0, 1, 2]).evolve()(t=s, wires=[0, 1, 2])

    with pytest.raises(NotImplementedError, match="1 or 2 wires"):
        Script(f=three_wires, n_qubits=3).vjp(obs, np.ones(1), args=(np.array(0.4),), pauli_seed=True,
                                              through_evolve=True)
    # 32x32 and up: the solver's own refusal names the limit
    from qml_essentials_amd.evolution import Evolution

    with pytest.raises(NotImplementedError, match="at most 4 wires"):
        Evolution._solve(np.zeros((1, 32, 32), dtype=np.complex128), np.ones((1, 1, 1)), np.ones(1), 2)


def test_a_noisy_tape_with_a_wide_gate_is_refused_before_any_device_work(monkeypatch):
    with recording() as tape:
        op.RX(0.3, wires=0)
        op.BitFlip(0.1, wires=0)
        op.Operation(wires=[0, 1, 2], matrix=_u(3))
    monkeypatch.setattr(N, "require_gpu", lambda: __import__("torch"))
    with pytest.raises(NotImplementedError, match="noisy tapes"):
        simulation.simulate_and_measure(tape, 3, "probs")


# ---- resource figures --------------------------------------------------------------------------------------------------
def test_the_two_kernels_are_built_without_scratch_and_at_their_occupancy():
    import __graft_entry__ as G

    res = json.load(open(G.RESOURCES))
    solver = {k: v for k, v in res.items() if "k_evolve_wide" in k}
    apply = {k: v for k, v in res.items() if "k_apply_matrix" in k}
    assert len(solver) == 4   # <DIM 8 / 16> x <ORDER 2 / 4>
    # <K 3 / 4> x (<complex64, complex128> x <NT> + complex64 in pairs: position 0 is a target, never streamed)
    assert len(apply) == 10
    for name, r in {**solver, **apply}.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
    for name, r in solver.items():  # the bar tests/test_evolve_jac_reference_cpu.py sets for its kin
        assert r["Occupancy"] >= 2 and r["VGPRs"] + r["AGPRs"] <= 256, (name, r)
        assert r["LDS Size"] <= 40960, (name, r)  # four workgroups of 128 threads per CU
    reported = {}  # what the build reports, per <K, complex128, pairs>: waves per SIMD
    for name, r in apply.items():
        k4, f64, pair = (a == b for a, b in zip(re.search(r"ILi(\d)ELb(\d)ELb(\d)ELb\dE", name).groups(), "411"))
        reported.setdefault((4 if k4 else 3, f64, pair), set()).add(r["Occupancy"])
        assert r["LDS Size"] == (1 << (2 * (4 if k4 else 3))) * (16 if f64 else 8), (name, r)
    assert reported == {(3, False, False): {8}, (3, False, True): {8}, (3, True, False): {8},
                        (4, False, False): {6}, (4, False, True): {7}, (4, True, False): {4}}, reported
