"""GPU: ``qmle_apply_matrix`` and the segmented execution of tapes that hold explicit matrices on three and four
wires, against the NumPy reference of tests/wide_gate_reference.py (which tests/test_wide_gates_cpu.py checks against
``embed_matrix`` and against its own wrong variants on every case used here).

Bars: 2e-6 relative to the state's largest amplitude on complex64, 1e-12 on complex128 -- the bars of the
explicit-matrix cases of tests/test_gpu_kernels.py and tests/test_gpu_x64_routes.py.

Register sizes of the sweep (``wide_gate_reference.SIZES``): a thread takes one group of 2^k amplitudes and a block
256 groups, so n - k = 0 is the register as the gate, n - k = 1 two threads, n - k = 6 one wave, 7 two waves, 8 one
block and 9 two blocks: n in {3, 4, 9, 10, 11, 12} at k = 3 and {4, 5, 11, 12, 13} at k = 4 cover those edges."""
import itertools

import numpy as np
import pytest
from scipy.linalg import expm

import evolution_reference as R
import wide_gate_reference as W
from qml_essentials_amd import _native as N
from qml_essentials_amd import jaqsi as js
from qml_essentials_amd import operations as op
from qml_essentials_amd import simulation, utils
from qml_essentials_amd.script import Script

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

X, Y, Z, I2 = R.X, R.Y, R.Z, R.I2
BAR = {False: 2e-6, True: 1e-12}


def run_apply(k, n, wires, batch, per_sample, f64):
    U, psi = W.case_data(k, n, batch, per_sample)
    want = W.apply(psi, U, wires, n)
    states = torch.from_numpy(psi).to(torch.complex128 if f64 else torch.complex64).cuda()
    start = states.clone()
    out = N.apply_matrix(states, wires, U)
    assert out is states and out.dtype == start.dtype
    got = states.cpu().numpy().astype(np.complex128)
    return np.abs(got - want).max() / np.abs(want).max()


@pytest.mark.parametrize("per_sample", [False, True], ids=["const", "rows"])
@pytest.mark.parametrize("f64", [False, True], ids=["c64", "c128"])
@pytest.mark.parametrize("k", [3, 4])
def test_every_ordered_wire_tuple_at_five_qubits(k, f64, per_sample):
    worst = 0.0
    tuples = list(itertools.permutations(range(5), k))
    assert len(tuples) == (60 if k == 3 else 120)
    for wires in tuples:
        err = run_apply(k, 5, list(wires), 3, per_sample, f64)
        worst = max(worst, err)
        assert err <= BAR[f64], (wires, err)
    print("k", k, "c128" if f64 else "c64", "rows" if per_sample else "const", "worst", worst)


@pytest.mark.parametrize("f64", [False, True], ids=["c64", "c128"])
@pytest.mark.parametrize("k,n", [(k, n) for k in (3, 4) for n in W.SIZES[k]])
def test_register_sizes_around_the_thread_wave_and_block_edges(k, n, f64):
    for name, wires in W.wire_sets(k, n).items():
        for per_sample in (False, True):
            err = run_apply(k, n, wires, 2, per_sample, f64)
            print("k", k, "n", n, name, wires, "rows" if per_sample else "const", err)
            assert err <= BAR[f64], (name, wires, per_sample, err)


@pytest.mark.parametrize("f64", [False, True], ids=["c64", "c128"])
def test_a_batch_beyond_65535(f64):
    """65537 states of three qubits, one matrix per state: the first, the last and the states around 65535 by the
    reference, every state by torch's batched product."""
    B, rng = 65537, np.random.default_rng(3)
    psi = W.random_states(rng, B, 3)
    few = W.random_unitaries(rng, 8, 16)
    U = few[np.arange(B) % 16] * np.exp(1j * 0.001 * np.arange(B))[:, None, None]
    wires = [2, 0, 1]
    dtype = torch.complex128 if f64 else torch.complex64
    states = torch.from_numpy(psi).to(dtype).cuda()
    mats = torch.from_numpy(U).cuda()
    N.apply_matrix(states, wires, mats)
    got = states.cpu().numpy().astype(np.complex128)
    pick = [0, 1, 65534, 65535, 65536]
    want = W.apply(psi[pick], U[pick], wires, 3)
    assert np.abs(got[pick] - want).max() / np.abs(want).max() <= BAR[f64]
    # every state: the matrix index is (wire 2, wire 0, wire 1), the state's axes are (wire 0, wire 1, wire 2)
    every = np.einsum("bxyzXYZ,bYZX->byzx", U.reshape((B,) + (2,) * 6), psi.reshape(B, 2, 2, 2)).reshape(B, 8)
    assert np.abs(every[pick] - want).max() <= 1e-14
    assert np.abs(every - got).max() <= (1e-12 if f64 else 2e-6)


@pytest.mark.parametrize("k,n,f64,positions", [(4, 27, False, [4, 13, 20, 26]), (3, 26, True, [3, 12, 25])])
def test_states_of_one_gib_take_the_streaming_route(k, n, f64, positions):
    """From 1 GiB of state on, a gate whose lowest position leaves every load whole 128-byte lines runs with
    non-temporal accesses -- other instantiations of the kernel than every smaller case above, and a fault in them
    can show at no smaller size: one case per precision, each with its lowest target on the lowest position that
    still streams.  The reference is torch's contraction in complex128 on the device."""
    wires = [n - 1 - p for p in positions][::-1]
    wires = wires[1:] + wires[:1]  # (a permuted order)
    g = torch.Generator(device="cuda").manual_seed(n + k)
    psi = torch.randn((1 << n, 2), generator=g, device="cuda", dtype=torch.float64 if f64 else torch.float32)
    psi = torch.view_as_complex(psi).reshape(1, -1)
    psi /= torch.linalg.vector_norm(psi)
    U = torch.from_numpy(W.random_unitaries(np.random.default_rng(k), 1 << k)).cuda()
    ref = psi.to(torch.complex128).reshape((2,) * n)
    want = torch.tensordot(U.reshape((2,) * (2 * k)), ref, dims=(list(range(k, 2 * k)), wires))
    want = torch.movedim(want, list(range(k)), wires).reshape(-1)
    del ref
    N.apply_matrix(psi, wires, U)
    err = float((psi.reshape(-1).to(torch.complex128) - want).abs().max() / want.abs().max())
    print("k", k, "n", n, "c128" if f64 else "c64", positions, err)
    assert err <= BAR[f64]


def test_wrapper_refusals():
    states = torch.zeros((2, 32), dtype=torch.complex64, device="cuda")
    with pytest.raises(NotImplementedError):
        N.apply_matrix(states, [0, 1], np.eye(4))
    with pytest.raises(ValueError, match="range"):
        N.apply_matrix(states, [0, 1, 5], np.eye(8))
    with pytest.raises(ValueError, match="do not fit"):
        N.apply_matrix(states, [0, 1, 2], np.zeros((3, 8, 8)))


# ---- front end ------------------------------------------------------------------------------------------------------------
def gate_matrix(name, *params):
    return np.asarray(getattr(op, name)(*params, wires=list(range(2 if name in ("CX", "CZ") else 1)), record=False).matrix)


def gate_matrix_rows(name, thetas):
    return np.stack([gate_matrix(name, float(t)) for t in thetas])


def reference_state(n, steps, B=1):
    """steps: [(matrix [d, d] or [B, d, d], wires)] applied to |0..0> of B samples."""
    psi = np.zeros((B, 1 << n), dtype=np.complex128)
    psi[:, 0] = 1.0
    for m, wires in steps:
        psi = W.apply(psi, m, wires, n)
    return psi


def measure(psi, n, type, obs_mats=()):
    if type == "state":
        return psi
    if type == "probs":
        return np.abs(psi) ** 2
    if type == "density":
        return psi[:, :, None] * psi.conj()[:, None, :]
    return np.stack([np.real(np.einsum("bi,bi->b", psi.conj(), W.apply(psi, m, wires, n))) for m, wires in obs_mats], axis=1)


def check_all_types(f, n, steps, B, args=(), in_axes=None, bar64=2e-6):
    """state, probs, density and expval (a Z, a Z-parity, a PauliX) in both precisions against the reference."""
    psi = reference_state(n, steps, B)
    obs = [op.PauliZ(wires=1, record=False), js.build_parity_observable([0, 2]), op.PauliX(wires=n - 1, record=False)]
    obs_mats = [(Z, [1]), (np.kron(Z, Z), [0, 2]), (X, [n - 1])]
    for x64 in (False, True):
        utils.enable_x64(x64)
        try:
            for type, ob, om in (("state", [], ()), ("probs", [], ()), ("density", [], ()), ("expval", obs, obs_mats),
                                 ("expval", obs[:1], obs_mats[:1]), ("expval", obs[:2], obs_mats[:2])):
                got = np.asarray(Script(f=f, n_qubits=n).execute(type=type, obs=list(ob), args=args, in_axes=in_axes))
                want = measure(psi, n, type, om)
                if in_axes is None:
                    want = want[0]
                assert got.shape == want.shape, (type, got.shape, want.shape)
                if x64:
                    assert got.dtype in (np.complex128, np.float64), (type, got.dtype)
                err = np.abs(got - want).max()
                print("x64" if x64 else "c64", type, len(ob), "err", err)
                assert err <= (1e-12 if x64 else bar64), (x64, type, err)
        finally:
            utils.enable_x64(False)


H3 = np.kron(np.kron(Z, Z), X)


def test_static_three_body_evolution_between_ordinary_gates():
    t = 0.37

    def f():
        op.RY(0.3, wires=0)
        op.RX(0.5, wires=3)
        op.CX(wires=[0, 1])
        op.H(wires=2)
        op.Hermitian(H3, [0, 1, 2]).evolve()(t, wires=[2, 0, 1])
        op.CX(wires=[2, 3])
        op.RY(-0.4, wires=1)

    steps = [(gate_matrix("RY", 0.3), [0]), (gate_matrix("RX", 0.5), [3]), (gate_matrix("CX"), [0, 1]),
             (gate_matrix("H"), [2]), (expm(-1j * t * H3), [2, 0, 1]), (gate_matrix("CX"), [2, 3]),
             (gate_matrix("RY", -0.4), [1])]
    check_all_types(f, 4, steps, 1)


def three_term_hamiltonian():
    mats = [np.kron(np.kron(Z, Z), X), np.kron(np.kron(X, I2), Y), np.kron(np.kron(I2, Y), Z)]

    def herm(m):
        return op.Hermitian(matrix=m, wires=[0, 1, 2], record=False)

    fns = [lambda p, t: p * np.cos(1.3 * t), lambda p, t: p * np.ones_like(t), lambda p, t: p * t]
    ph = fns[0] * herm(mats[0]) + fns[1] * herm(mats[1]) + fns[2] * herm(mats[2])
    return ph, np.stack(mats)


@pytest.mark.parametrize("solver", ["magnus4", "dopri8"])
def test_parametrized_hamiltonian_with_one_matrix_per_sample(solver):
    """Batched parameters and a batched T through in_axes, batch 5: one 8x8 matrix per sample."""
    B = 5
    rng = np.random.default_rng(9)
    p = rng.uniform(0.4, 1.2, size=(B, 3))
    T = rng.uniform(0.8, 1.4, size=B)
    ph, mats = three_term_hamiltonian()

    def f(p, T):
        op.RY(0.3, wires=0)
        op.H(wires=1)
        op.CX(wires=[1, 3])
        ph.evolve(solver=solver, magnus_steps=24)([p[0], p[1], p[2]], T)
        op.RX(0.2, wires=2)

    ref_fns = [lambda t, r: p[r, 0] * np.cos(1.3 * t), lambda t, r: p[r, 1] * np.ones_like(t), lambda t, r: p[r, 2] * t]
    if solver == "magnus4":
        U = R.solve_fixed(mats, ref_fns, np.zeros(B), T, 24, 4)
    else:  # the rule behind the adaptive names, at the default tolerances of each mode
        U = None
    for x64 in (False, True):
        tol = 1.0e-10 if x64 else 1.4e-8
        if solver == "dopri8":
            U, _n, ok = R.doubling(mats, ref_fns, np.zeros(B), T, atol=tol, rtol=tol)
            assert ok.all()
        steps = [(gate_matrix("RY", 0.3), [0]), (gate_matrix("H"), [1]), (gate_matrix("CX"), [1, 3]), (U, [0, 1, 2]),
                 (gate_matrix("RX", 0.2), [2])]
        psi = reference_state(4, steps, B)
        utils.enable_x64(x64)
        try:
            for type in ("state", "probs"):
                got = np.asarray(Script(f=f, n_qubits=4).execute(type=type, args=(p, T), in_axes=(0, 0)))
                err = np.abs(got - measure(psi, 4, type)).max()
                print(solver, "x64" if x64 else "c64", type, err)
                assert got.shape[0] == B and err <= (1e-12 if x64 else 2e-6), (solver, x64, type, err)
        finally:
            utils.enable_x64(False)


def test_four_wire_hamiltonian_two_wide_gates_in_a_row_and_a_tape_of_one_wide_gate():
    rng = np.random.default_rng(21)
    a = rng.normal(size=(16, 16)) + 1j * rng.normal(size=(16, 16))
    H4 = (a + a.conj().T) / 4.0
    t = 0.21

    def four():  # a four-wire Hamiltonian on a permuted order, then a three-wire one, nothing between them
        op.RY(0.7, wires=2)
        op.Hermitian(H4, [0, 1, 2, 3]).evolve()(t, wires=[3, 1, 0, 2])
        op.Hermitian(H3, [0, 1, 2]).evolve()(2 * t, wires=[1, 3, 2])
        op.RX(0.1, wires=0)

    steps = [(gate_matrix("RY", 0.7), [2]), (expm(-1j * t * H4), [3, 1, 0, 2]), (expm(-2j * t * H3), [1, 3, 2]),
             (gate_matrix("RX", 0.1), [0])]
    check_all_types(four, 4, steps, 1)

    def alone():
        op.Hermitian(H4, [0, 1, 2, 3]).evolve()(t, wires=[1, 0, 3, 2])

    check_all_types(alone, 4, [(expm(-1j * t * H4), [1, 0, 3, 2])], 1)


def test_a_product_of_gates_runs_and_equals_its_factors():
    """``A.prod(B)`` is the matrix product A B on the union of the wires -- B acts first --; its dagger and its
    square run too."""
    P = op.prod(op.CX(wires=[0, 1], record=False), op.CX(wires=[1, 2], record=False))

    def product():
        op.H(wires=0)
        op.RY(0.9, wires=1)
        op.Operation(wires=P.wires, matrix=P.matrix, name=P.name)
        op.RX(0.3, wires=2)

    def factors():
        op.H(wires=0)
        op.RY(0.9, wires=1)
        op.CX(wires=[1, 2])
        op.CX(wires=[0, 1])
        op.RX(0.3, wires=2)

    def dagger_and_power():
        op.H(wires=0)
        op.RY(0.9, wires=1)
        op.prod(op.CX(wires=[0, 1], record=False), op.CX(wires=[1, 2], record=False)).dagger()
        op.prod(op.CX(wires=[0, 1], record=False), op.CX(wires=[1, 2], record=False)).power(2)

    for x64 in (False, True):
        utils.enable_x64(x64)
        try:
            a = np.asarray(Script(f=product, n_qubits=3).execute(type="state"))
            b = np.asarray(Script(f=factors, n_qubits=3).execute(type="state"))
            c = np.asarray(Script(f=dagger_and_power, n_qubits=3).execute(type="state"))
        finally:
            utils.enable_x64(False)
        bar = 1e-12 if x64 else 2e-6
        assert np.abs(a - b).max() <= bar
        M = np.asarray(P.matrix)
        want = reference_state(3, [(gate_matrix("H"), [0]), (gate_matrix("RY", 0.9), [1]), (M.conj().T, P.wires),
                                   (M @ M, P.wires)])[0]
        assert np.abs(c - want).max() <= bar


def test_shots_sample_the_exact_probabilities_with_the_given_key():
    from qml_essentials_amd.utils import PRNGKey

    t = 0.37

    def f():
        op.RY(0.3, wires=0)
        op.H(wires=2)
        op.Hermitian(H3, [0, 1, 2]).evolve()(t, wires=[2, 0, 1])
        op.RY(-0.4, wires=1)

    s = Script(f=f, n_qubits=3)
    key = PRNGKey(5)
    exact = s.execute(type="probs", as_tensor=True)
    got = np.asarray(s.execute(type="probs", shots=500, key=key))
    want = simulation.sample_shots(exact.reshape(1, -1), 3, "probs", [], 500, key).cpu().numpy()[0]
    assert np.array_equal(got, want) and abs(got.sum() - 1.0) < 1e-6
    z = [op.PauliZ(wires=0, record=False)]
    got = np.asarray(s.execute(type="expval", obs=z, shots=500, key=key))
    want = simulation.sample_shots(exact.reshape(1, -1), 3, "expval", z, 500, key).cpu().numpy()[0]
    assert np.array_equal(got, want)


def test_a_batch_cut_inside_the_call_equals_the_whole_batch(monkeypatch):
    """Per-sample angles and one 8x8 matrix per sample, five samples in chunks of two: the angle tables and the
    matrices are sliced by rows, and a sampled row keeps its own random stream."""
    from qml_essentials_amd import memory
    from qml_essentials_amd.batching import Batched
    from qml_essentials_amd.tape import recording
    from qml_essentials_amd.utils import PRNGKey

    rng = np.random.default_rng(17)
    U, th = W.random_unitaries(rng, 8, 5), rng.uniform(0, 3, size=5)
    with recording() as tape:
        op.RY(Batched(th), wires=0)
        op.H(wires=2)
        op.Operation(wires=[2, 0, 1], matrix=U)
        op.RX(Batched(0.5 * th), wires=1)
    steps = [(gate_matrix_rows("RY", th), [0]), (gate_matrix("H"), [2]), (U, [2, 0, 1]), (gate_matrix_rows("RX", 0.5 * th), [1])]
    want = measure(reference_state(3, steps, 5), 3, "probs")
    z = [op.PauliZ(wires=1, record=False)]
    whole = simulation.simulate_and_measure(tape, 3, "probs")
    shots = simulation.simulate_and_measure(tape, 3, "expval", z, shots=200, key=PRNGKey(3))
    assert np.abs(whole - want).max() <= 2e-6
    monkeypatch.setattr(memory, "compute_chunk_size", lambda *a, **k: 2)
    assert np.array_equal(simulation.simulate_and_measure(tape, 3, "probs"), whole)
    assert np.array_equal(simulation.simulate_and_measure(tape, 3, "probs", as_tensor=True).cpu().numpy(), whole)
    assert np.array_equal(simulation.simulate_and_measure(tape, 3, "expval", z, shots=200, key=PRNGKey(3)), shots)


def test_what_stays_refused_on_the_gpu_too():
    def noisy():
        op.RX(0.3, wires=0)
        op.Hermitian(H3, [0, 1, 2]).evolve()(0.2, wires=[0, 1, 2])
        op.BitFlip(0.1, wires=0)

    with pytest.raises(NotImplementedError, match="noisy tapes"):
        Script(f=noisy, n_qubits=3).execute(type="probs")

    def five():
        op.Operation(wires=[0, 1, 2, 3, 4], matrix=np.eye(32))

    with pytest.raises(NotImplementedError, match="generic 5-qubit"):
        Script(f=five, n_qubits=5).execute(type="probs")
    with pytest.raises(NotImplementedError, match="at most 4 wires"):
        op.Hermitian(np.eye(32), [0, 1, 2, 3, 4], record=False).evolve()(0.1, wires=[0, 1, 2, 3, 4])
