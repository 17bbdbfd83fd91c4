"""GPU: ``qmle_evolve_magnus`` against the NumPy scheme of ``tests/evolution_reference.py``, the ``evolve`` API
against known answers, and per-sample matrix gates (``MAT1_ROW`` / ``MAT2_ROW``) inside circuits against a per-row
NumPy simulation with the truth unitaries.

Bars.  complex128 output of the kernel: 1e-12 (the project's complex128 bar; the arithmetic is float64 end to end).
complex64 output: 2e-7 (one float32 rounding of entries of modulus <= 1 is 6e-8).  Unitarity of the complex128
output: 1e-12.  Circuits: 2e-6 on complex64 states, the bar of the explicit-matrix cases of
tests/test_gpu_kernels.py; 1e-12 with x64."""
import numpy as np
import pytest
from scipy.linalg import expm

import evolution_reference as R
from oracle import einsum_sim as OE
from qml_essentials_amd import _native as N
from qml_essentials_amd import operations as op
from qml_essentials_amd import utils
from qml_essentials_amd.script import NotAffine, Script

pytestmark = pytest.mark.gpu

LANES = (0, 1, 4, 16, 64)


def check_kernel(H, coef, h, order, label):
    """Every lanes_per_row, both output types, against one NumPy reference."""
    want = R.magnus(H, coef, h, order)
    d = H.shape[-1]
    for lanes in LANES:
        got = N.evolve_magnus(H, coef, h, order, lanes_per_row=lanes).cpu().numpy()
        err = np.abs(got - want).max()
        uni = np.abs(np.einsum("rji,rjk->rik", got.conj(), got) - np.eye(d)).max()
        got32 = N.evolve_magnus(H, coef, h, order, lanes_per_row=lanes, complex64=True).cpu().numpy()
        err32 = np.abs(got32 - want).max()
        print(label, "lanes", lanes, "err", err, "unitarity", uni, "complex64 err", err32)
        assert got.dtype == np.complex128 and got32.dtype == np.complex64
        assert err <= 1e-12, (label, lanes, err)
        assert uni <= 1e-12, (label, lanes, uni)
        assert err32 <= 2e-7, (label, lanes, err32)


# n_steps around the lane counts (fewer steps than lanes included) x rows around the wave and block sizes
GRID = [(1, 1000), (2, 65), (3, 64), (63, 5), (64, 1), (65, 64), (257, 5), (1024, 1)]


@pytest.mark.parametrize("n_steps,rows", GRID)
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("dim", [2, 4])
def test_kernel_matches_the_numpy_scheme(dim, order, n_steps, rows):
    """Per-row t0 != 0 and per-row h; 1, 2 and 3 terms.  The rows' windows and pulse scales vary within a factor
    of 1.4, so that h |sum c_i H_i| stays below ~15 even with ONE step: the 1e-12 bar is that of float64 products of
    matrices of moderate norm (an exponential's rounding error grows with the norm of its exponent)."""
    c = (R.case_dim2 if dim == 2 else R.case_dim4)(11, rows)
    t0 = c["t0"] + 0.003 * (np.arange(rows) % 50)
    t1 = c["t1"] + 0.02 * (np.arange(rows) % 31)
    h = (t1 - t0) / n_steps
    t = R.node_times(t0, h, n_steps, order)
    for n_terms in (1, 2, 3):
        # (one term alone: take the time-dependent one, not the constant)
        pick = [1] if n_terms == 1 else list(range(n_terms))
        H = c["H"][pick]
        coef = R.coef_table([c["fns"][k] for k in pick], t)
        check_kernel(H, coef, h, order, f"dim{dim} order{order} terms{n_terms} steps{n_steps} rows{rows}")


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name,case", R.seeded_cases(), ids=[n for n, _ in R.seeded_cases()])
def test_kernel_on_the_seeded_hamiltonians_that_tell_the_wrong_variants_apart(name, case, order):
    """The cases (3 rows that differ in pulse, start and step; 64 steps) on which tests/test_evolution_cpu.py shows
    every wrong variant of the scheme at least 1e-6 away: agreeing to 1e-12 here rules each of them out."""
    seed = int(name.split("seed")[1])
    c = (R.case_dim2 if case["dim"] == 2 else R.case_dim4)(seed, 3)
    t0 = c["t0"] + 0.01 * np.arange(3)
    t1 = c["t1"] + 0.3 * np.arange(3)
    h = (t1 - t0) / 64
    coef = R.coef_table(c["fns"], R.node_times(t0, h, 64, order))
    check_kernel(c["H"], coef, h, order, f"{name} order{order}")


def test_kernel_static_exponentials_of_large_norm_and_zero():
    """One step of order 2 with a constant term is exp(-i t H): t far beyond the series' radius (the exponent is
    cut into parts), negative, and zero."""
    rng = np.random.default_rng(5)
    a = rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4))
    for H in ((a + a.conj().T) / 2, R.X + 0.5 * R.Z + 0.25 * np.eye(2)):
        t = np.array([0.0, 1e-9, 0.3, -2.0, 7.3, 40.0])
        got = N.evolve_magnus(H[None], np.ones((6, 1, 1)), t, 2).cpu().numpy()
        want = np.stack([expm(-1j * x * H) for x in t])
        assert np.abs(got - want).max() <= 1e-12


# ---- the API ---------------------------------------------------------------------------------------------------------
def test_known_answers_of_static_evolution():
    """Reference tests/test_jaqsi.py:146-158: exp(-i t Z)|0> leaves <X> = 0; from |+>, |<X>| = cos(2 t)."""
    def from_zero(t):
        op.Hermitian(matrix=R.Z, wires=0).evolve()(t=t, wires=0)

    def from_plus(t):
        op.H(wires=0)
        op.Hermitian(matrix=R.Z, wires=0).evolve()(t=t, wires=0)

    t = 0.3
    res = Script(f=from_zero).execute(type="expval", obs=[op.PauliX(0)], args=(t,))
    assert np.allclose(res, [0.0], atol=1e-6)
    res = Script(f=from_plus).execute(type="expval", obs=[op.PauliX(0)], args=(t,))
    assert np.allclose(res, [np.cos(2 * t)], atol=1e-6)  # (the Hamiltonian itself is not on the tape: no sign flip)
    ts = np.linspace(-1.0, 2.0, 7)
    res = Script(f=from_plus).execute(type="expval", obs=[op.PauliX(0)], args=(ts,), in_axes=(0,))
    assert np.allclose(np.asarray(res)[:, 0], np.cos(2 * ts), atol=1e-6)


def herm(m, wires=0):
    return op.Hermitian(matrix=m, wires=wires, record=False)


@pytest.mark.parametrize("solver", ["dopri8", "dopri5", "magnus2", "magnus4"])
def test_constant_coefficients_equal_the_static_gate_and_expm(solver):
    T = 0.5
    ph = (lambda p, t: 1.0) * herm(R.Z)
    U = ph.evolve(solver=solver)([None], T).matrix
    static = herm(R.Z).evolve()(T).matrix
    assert U.shape == (2, 2) and np.abs(U - static).max() <= 1e-6
    assert np.abs(static - expm(-1j * T * R.Z)).max() <= 1e-12
    # reference tests/test_jaqsi.py:1077-1098: H = X + Y, two constant terms
    ph = (lambda p, t: 1.0) * herm(R.X) + (lambda p, t: 1.0) * herm(R.Y)
    U = ph.evolve(solver=solver)([np.array([]), np.array([])], T).matrix
    assert np.abs(U - expm(-1j * T * (R.X + R.Y))).max() <= 1e-6
    # a window [t0, t1] and parameters: H = p0 X + p1 ZZ-like 4x4
    H4 = np.kron(R.X, R.Z)
    ph = (lambda p, t: p[0]) * herm(H4, [0, 1]) + (lambda p, t: p * np.ones_like(t)) * herm(np.kron(R.Z, R.Z), [0, 1])
    U = ph.evolve(solver=solver)([np.array([0.7]), 0.4], [0.2, 1.1]).matrix
    assert np.abs(U - expm(-1j * 0.9 * (0.7 * H4 + 0.4 * np.kron(R.Z, R.Z)))).max() <= 1e-6


def test_time_dependent_solve_is_unitary_and_matches_the_truth():
    case = R.case_dim2(12)
    wrap = [lambda p, t, f=f: p * f(np.atleast_2d(t), np.zeros((1, 1), dtype=int))[0] for f in case["fns"]]
    ph = wrap[0] * herm(R.X) + wrap[1] * herm(R.Y) + wrap[2] * herm(R.Z)
    U = ph.evolve()([1.0, 1.0, 1.0], [case["t0"], case["t1"]]).matrix
    assert np.abs(U.conj().T @ U - np.eye(2)).max() <= 1e-12
    assert np.abs(U - R.truth(case["H"], case["fns"], case["t0"], case["t1"])).max() <= 2.8e-8  # atol + rtol


def test_step_budget_failures():
    ph = (lambda p, t: p * np.cos(1e3 * t)) * herm(R.X)
    with pytest.raises(RuntimeError, match="max_steps"):
        ph.evolve(max_steps=4)([2.0], 1.0)
    U = ph.evolve(max_steps=4, throw=False)([2.0], 1.0).matrix
    assert U.shape == (2, 2) and np.isnan(U).all()
    with pytest.raises(RuntimeError, match="max_steps"):
        ph.evolve(max_steps=64)([2.0], 1.0)       # 64 steps do not resolve cos(1e3 t) to 2.8e-8 either
    easy = (lambda p, t: 1.0) * herm(R.X)
    U = easy.evolve(throw=False)([None], 0.5).matrix
    assert np.isfinite(U).all() and np.abs(U - expm(-0.5j * R.X)).max() <= 1e-6


@pytest.mark.parametrize("name,case", R.seeded_cases()[:2], ids=["dim2", "dim4"])
def test_dopri8_takes_the_grid_of_the_numpy_rule(name, case):
    wrap = [lambda p, t, f=f: f(np.atleast_2d(t), np.zeros((1, 1), dtype=int))[0] for f in case["fns"]]
    wires = [0] if case["dim"] == 2 else [0, 1]
    ph = wrap[0] * herm(case["H"][0], wires)
    for f, H in zip(wrap[1:], case["H"][1:]):
        ph = ph + f * herm(H, wires)
    gate = ph.evolve(solver="dopri8")([None] * len(wrap), [case["t0"], case["t1"]])
    want, n, ok = R.doubling(case["H"], case["fns"], case["t0"], case["t1"], atol=1.4e-8, rtol=1.4e-8)
    assert ok.all() and gate.evolve_steps == n
    assert np.abs(gate.matrix - want[0]).max() <= 1e-12


# ---- row gates in circuits -----------------------------------------------------------------------------------------------
RNG = np.random.default_rng(77)
A4 = RNG.normal(size=(4, 4)) + 1j * RNG.normal(size=(4, 4))
H1 = 0.8 * R.X - 0.6 * R.Y + 0.3 * R.Z + 0.2 * np.eye(2)
H2 = (A4 + A4.conj().T) / 2


def one_qubit_circuit(n, w):
    """RY on every wire; RX, the row gate, RX on wire w (one merged 2x2); a CX from w; the row gate again."""
    def f(t):
        gate = op.Hermitian(matrix=H1, wires=w).evolve()
        for q in range(n):
            op.RY(0.3 + 0.1 * q, wires=q)
        op.RX(0.4, wires=w)
        gate(t, wires=w)
        op.RX(-0.7, wires=w)
        if n > 1:
            op.CX(wires=[w, (w + 1) % n])
        gate(0.5 * t, wires=w)

    def oracle(t):
        tape = [("RY", [q], (0.3 + 0.1 * q,)) for q in range(n)]
        tape += [("RX", [w], (0.4,)), ("Matrix", [w], (expm(-1j * t * H1),)), ("RX", [w], (-0.7,))]
        if n > 1:
            tape.append(("CX", [w, (w + 1) % n], ()))
        tape.append(("Matrix", [w], (expm(-0.5j * t * H1),)))
        return tape

    return f, oracle


def two_qubit_circuit(n, wires):
    """RY on every wire; RZ on the first wire, the 4x4 row gate, RX on the second wire; a CX; a time-dependent
    two-term 4x4 row gate whose amplitude is the batched argument."""
    a, b = wires
    ZZ, XI = np.kron(R.Z, R.Z), np.kron(R.X, np.eye(2))

    def f(t):
        for q in range(n):
            op.RY(0.3 + 0.1 * q, wires=q)
        op.RZ(0.9, wires=a)
        op.Hermitian(matrix=H2, wires=wires).evolve()(t, wires=wires)
        op.RX(0.35, wires=b)
        op.CX(wires=[b, a])
        ph = (lambda p, s: p * np.ones_like(s)) * herm(ZZ, wires) + (lambda p, s: 1.0) * herm(XI, wires)
        ph.evolve(solver="magnus4", magnus_steps=8)([t, None], 0.6)   # constant in time: exact on any grid

    def oracle(t):
        tape = [("RY", [q], (0.3 + 0.1 * q,)) for q in range(n)]
        tape += [("RZ", [a], (0.9,)), ("Matrix", [a, b], (expm(-1j * t * H2),)), ("RX", [b], (0.35,)),
                 ("CX", [b, a], ()), ("Matrix", [a, b], (expm(-0.6j * (t * ZZ + XI)),))]
        return tape

    return f, oracle


def run_rows(f, oracle, n, B, x64=False, type="state", obs=()):
    ts = np.linspace(0.2, 1.9, B) + 0.01 * np.arange(B) ** 2  # every row different
    got = np.asarray(Script(f=f, n_qubits=n).execute(type=type, obs=list(obs), args=(ts,), in_axes=(0,)))
    want = np.stack([OE.simulate_and_measure(oracle(t), n, type, [("PauliZ", [q]) for q in obs_wires(obs)],
                                             np.complex128) for t in ts])
    assert got.shape == want.shape
    if type == "state":
        assert got.dtype == (np.complex128 if x64 else np.complex64)
    return np.abs(got - want).max()


def obs_wires(obs):
    return [o.wires[0] for o in obs]


SIZES = [(1, 17), (3, 3), (5, 17), (14, 3), (16, 3)]  # whole state in LDS up to 5, tile passes at 14 and 16


@pytest.mark.parametrize("n,B", SIZES)
def test_one_qubit_row_gates_in_circuits(n, B):
    for w in sorted({0, n // 2, n - 1}):  # highest, middle and lowest wire
        err = run_rows(*one_qubit_circuit(n, w), n, B)
        print("n", n, "B", B, "wire", w, "err", err)
        assert err <= 2e-6, (n, B, w, err)


@pytest.mark.parametrize("n,B", SIZES[1:])
def test_two_qubit_row_gates_in_circuits(n, B):
    for wires in ([0, 1], [n - 2, n - 1], [0, n - 1], [n - 1, 0], [n // 2 + 1, n // 2 - 1 if n > 3 else 0]):
        if wires[0] == wires[1]:
            continue
        err = run_rows(*two_qubit_circuit(n, wires), n, B)
        print("n", n, "B", B, "wires", wires, "err", err)
        assert err <= 2e-6, (n, B, wires, err)


def test_expval_of_a_circuit_with_row_gates():
    n, B = 5, 17
    obs = [op.PauliZ(wires=q, record=False) for q in (0, 2, 4)]
    f, oracle = two_qubit_circuit(n, [3, 1])
    assert run_rows(f, oracle, n, B, type="expval", obs=obs) <= 2e-6
    f, oracle = one_qubit_circuit(n, 2)
    assert run_rows(f, oracle, n, B, type="expval", obs=obs) <= 2e-6


@pytest.mark.parametrize("B", [3, 70])
def test_row_gates_beside_every_other_source_of_the_matrix_builder(B):
    """The builder forms the row gates' matrices and those of every other gate in one kernel: controlled rotations,
    the controlled phase, Rot, fixed gates and two-qubit rotations beside both row opcodes, below and above the 64
    samples from which a wave builds one group."""
    n = 3

    def f(t):
        op.H(wires=0)
        op.Rot(0.3, 0.5, -0.4, wires=1)
        op.CRX(0.7, wires=[0, 1])
        op.Hermitian(matrix=H1, wires=1).evolve()(t, wires=1)
        op.CRZ(t, wires=[1, 2])
        op.ControlledPhaseShift(0.9, wires=[2, 0])
        op.Hermitian(matrix=H2, wires=[2, 0]).evolve()(t, wires=[2, 0])
        op.CRY(-1.1, wires=[2, 1])
        op.RXX(0.6, wires=[0, 1])
        op.S(wires=2)
        op.PauliY(wires=0)

    def oracle(t):
        return [("H", [0], ()), ("Rot", [1], (0.3, 0.5, -0.4)), ("CRX", [0, 1], (0.7,)),
                ("Matrix", [1], (expm(-1j * t * H1),)), ("CRZ", [1, 2], (t,)), ("CPhase", [2, 0], (0.9,)),
                ("Matrix", [2, 0], (expm(-1j * t * H2),)), ("CRY", [2, 1], (-1.1,)), ("RXX", [0, 1], (0.6,)),
                ("S", [2], ()), ("PauliY", [0], ())]

    err = run_rows(f, oracle, n, B)
    print("B", B, "err", err)
    assert err <= 2e-6


@pytest.mark.parametrize("n", [3, 14])
def test_row_gates_in_x64_mode(n):
    utils.enable_x64(True)
    try:
        for w in (0, n - 1):
            err = run_rows(*one_qubit_circuit(n, w), n, 3, x64=True)
            assert err <= 1e-12, (n, w, err)
        for wires in ([0, n - 1], [n - 1, 1]):
            err = run_rows(*two_qubit_circuit(n, wires), n, 3, x64=True)
            assert err <= 1e-12, (n, wires, err)
    finally:
        utils.enable_x64(False)


# ---- what is deliberately not served -------------------------------------------------------------------------------------
def test_the_three_refusals():
    from qml_essentials_amd import adjoint

    def circuit(theta, t):
        op.RX(theta, wires=0)
        op.Hermitian(matrix=H1, wires=0).evolve()(t, wires=0)

    def noisy(theta, t):
        circuit(theta, t)
        op.BitFlip(0.1, wires=0)

    ts, th = np.linspace(0.1, 0.5, 3), np.linspace(0.3, 0.9, 3)
    s = Script(f=circuit, n_qubits=1)
    # the angle-map path: an evolved gate is no affine function of the device-resident arguments
    with pytest.raises(NotAffine):
        s.compiled("k", "state", [], (th[0], ts[0]), (0, 1))
    # a noisy tape
    with pytest.raises(NotImplementedError, match="density-matrix mode"):
        Script(f=noisy, n_qubits=1).execute(type="probs", args=(th, ts), in_axes=(0, 0))
    # the adjoint sweep: no rule for the gate; and no derivative through the solver
    z = [op.PauliZ(wires=0, record=False)]
    with pytest.raises(adjoint.AdjointUnsupported, match="MAT1_ROW"):
        s.vjp(z, np.ones((3, 1)), args=(th, ts), in_axes=(0, 0), argnums=(0,))
    with pytest.raises(NotImplementedError, match="non-linear"):
        s.gradient(z, args=(th, ts), in_axes=(0, 0), argnums=(1,))
