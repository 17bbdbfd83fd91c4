"""GPU: adjoint gradients through explicit matrices on three and four wires -- ``qmle_wide_moment`` alone,
``qmle_adjoint_segment`` on states the test prepares, and ``Script.vjp(wide_gates=True)`` end to end -- against the
NumPy complex128 reference of tests/wide_adjoint_reference.py (which tests/test_wide_adjoint_cpu.py holds to central
differences of its own cost and to its own wrong variants).

Bars: ``tolerance(n, x64)`` of tests/test_gpu_adjoint_routes.py -- 1e-12 in complex128, 4e-6 up to n = 13 and 1e-5 up to
n = 16 in complex64 --, for the moment kernel on unit-norm states as absolute errors of the cotangent's entries (each
is at most 1), for gradients relative to max(1, sum |w|).  The measured worst case is printed, as there.

The moment at n = 20 (batch 2, the many-block reduction: 128 and 64 blocks per state) has a complex64 bar of its own,
set as ``BOUND_19_20`` was: four times the error measured against the reference, rounded to one digit.  Measured on an
MI355X: 2.8e-10 (k = 3, scattered wires; an entry of the moment of two random unit vectors of 2^20 amplitudes is itself
about 1e-3), so ``BOUND_20 = 1e-9``; the complex128 bar stays 1e-12.

Register sizes of the moment sweep: a lane takes four groups of 2^k amplitudes per step and a wave 16 (k = 4) or 32
(k = 3), so n = k, k + 1 and k + 2 have fewer groups than one step, and ``wide_gate_reference.SIZES`` pass the wave,
block and two-block edges."""
import itertools

import numpy as np
import pytest

import wide_adjoint_reference as A
import wide_gate_reference as W
from qml_essentials_amd import _native as N
from qml_essentials_amd import adjoint, simulation
from qml_essentials_amd import jaqsi as js
from qml_essentials_amd import operations as op
from qml_essentials_amd.script import Script
from qml_essentials_amd.simulation import LoweredTape, get_plan
from qml_essentials_amd.tape import recording
from qml_essentials_amd.utils import x64_scope
from tests.test_gpu_adjoint_routes import tolerance

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BOUND_20 = 1e-9  # 4 x the measured 2.8e-10, one digit (see the module docstring)


# ---- the moment kernel alone --------------------------------------------------------------------------------------------
def moment_data(k, n, batch, seed=0):
    """Independent unit-norm psi and lambda (lambda is NOT derived from psi) and one unitary per sample."""
    rng = np.random.default_rng(7000 * k + 10 * n + batch + seed)
    return W.random_states(rng, batch, n), W.random_states(rng, batch, n), W.random_unitaries(rng, 1 << k, batch)


def run_moment(k, n, wires, batch, mode, f64, seed=0):
    """mode: "none" (d_mats = NULL: the moment itself), "const" (one matrix), "rows" (one per sample) -> max |error|"""
    psi, lam, U = moment_data(k, n, batch, seed)
    mats = None if mode == "none" else U[0] if mode == "const" else U
    want = A.moment_reference(psi, lam, wires, n, mats)
    dtype = torch.complex128 if f64 else torch.complex64
    p, l = torch.from_numpy(psi).to(dtype).cuda(), torch.from_numpy(lam).to(dtype).cuda()
    p0, l0 = p.clone(), l.clone()
    got = N.wide_moment(p, l, wires, mats)
    assert got.dtype == dtype and tuple(got.shape) == (batch, 1 << k, 1 << k)
    assert torch.equal(p, p0) and torch.equal(l, l0)  # read, never written
    return np.abs(got.cpu().numpy().astype(np.complex128) - want).max()


@pytest.mark.parametrize("mode", ["none", "const", "rows"])
@pytest.mark.parametrize("f64", [False, True], ids=["c64", "c128"])
@pytest.mark.parametrize("k", [3, 4])
def test_moment_of_every_ordered_wire_tuple_at_five_qubits(k, f64, mode):
    """batch 3, distinct matrices per sample in the "rows" mode"""
    tuples = list(itertools.permutations(range(5), k))
    assert len(tuples) == (60 if k == 3 else 120)
    worst = 0.0
    for wires in tuples:
        err = run_moment(k, 5, list(wires), 3, mode, f64)
        worst = max(worst, err)
        assert err <= tolerance(5, f64), (wires, err)
    print("moment k", k, "c128" if f64 else "c64", mode, "worst", worst)


@pytest.mark.parametrize("f64", [False, True], ids=["c64", "c128"])
@pytest.mark.parametrize("k,n", sorted({(k, n) for k in (3, 4) for n in (k, k + 1, k + 2) + W.SIZES[k]}))
def test_moment_at_register_sizes_around_the_step_wave_and_block_edges(k, n, f64):
    for name, wires in W.wire_sets(k, n).items():
        for mode in ("none", "rows"):
            err = run_moment(k, n, wires, 2, mode, f64)
            print("moment k", k, "n", n, name, wires, mode, err)
            assert err <= tolerance(n, f64), (name, wires, mode, err)


@pytest.mark.parametrize("f64", [False, True], ids=["c64", "c128"])
@pytest.mark.parametrize("k", [3, 4])
def test_moment_many_block_reduction_at_twenty_qubits(k, f64):
    worst = 0.0
    for name, wires in W.wire_sets(k, 20).items():
        err = run_moment(k, 20, wires, 2, "rows", f64)
        print("moment k", k, "n 20", name, wires, "c128" if f64 else "c64", err)
        worst = max(worst, err)
    print("moment k", k, "n 20 worst", worst)
    assert worst <= (1e-12 if f64 else BOUND_20)


@pytest.mark.parametrize("f64", [False, True], ids=["c64", "c128"])
def test_two_moment_calls_give_identical_bits(f64):
    for k, n, wires in ((4, 13, [12, 3, 0, 7]), (3, 12, [0, 1, 2]), (4, 20, [19, 18, 2, 5])):
        psi, lam, U = moment_data(k, n, 2)
        dtype = torch.complex128 if f64 else torch.complex64
        p, l = torch.from_numpy(psi).to(dtype).cuda(), torch.from_numpy(lam).to(dtype).cuda()
        a = N.wide_moment(p, l, wires, U)
        b = N.wide_moment(p, l, wires, U)
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def test_moment_wrapper_refusals():
    p = torch.zeros((2, 32), dtype=torch.complex64, device="cuda")
    with pytest.raises(NotImplementedError):
        N.wide_moment(p, p.clone(), [0, 1])
    with pytest.raises(ValueError, match="range"):
        N.wide_moment(p, p.clone(), [0, 1, 5])
    with pytest.raises(ValueError, match="do not fit"):
        N.wide_moment(p, p.clone(), [0, 1, 2], np.zeros((3, 8, 8)))
    with pytest.raises(ValueError, match="agree"):
        N.wide_moment(p, p.to(torch.complex128), [0, 1, 2])


# ---- one segment on resident states ------------------------------------------------------------------------------------
def segment_tape(n, B, rng):
    """RX / CRZ layers around a one-wire and a two-wire explicit matrix, per-sample angles; no wide gate."""
    th = rng.uniform(-np.pi, np.pi, size=(B, 4 * n))
    from qml_essentials_amd.batching import Batched

    with recording() as tape:
        for q in range(n):
            op.RX(Batched(th[:, q]), wires=q)
        for q in range(n - 1):
            op.CRZ(Batched(th[:, n + q]), wires=[q, q + 1])
        op.Operation(wires=[1], matrix=W.random_unitaries(rng, 2))
        op.Operation(wires=[n - 1, 0], matrix=W.random_unitaries(rng, 4))
        for q in range(n):
            op.RY(Batched(th[:, 2 * n + q]), wires=q)
        op.CX(wires=[0, n - 1])
        for q in range(n):
            op.RZ(Batched(th[:, 3 * n + q]), wires=q)
    return tape


@pytest.mark.parametrize("x64", [False, True], ids=["c64", "c128"])
@pytest.mark.parametrize("n", [6, 14])
def test_forward_run_seed_and_one_segment_call_give_the_sweeps_gradient(n, x64):
    B, rng = 2, np.random.default_rng(n)
    tape = segment_tape(n, B, rng)
    groups = [[0], [1, n - 1], [2]]
    w = rng.uniform(-1, 1, size=(B, 3))
    with x64_scope(x64):
        low = LoweredTape(tape, n)
        want = [s % 3 != 1 for s in range(low.n_slots)]  # every third column is asked of nobody
        mat_entry = [getattr(o, "_native", None) is None and o._matrix is not None for o in tape]
        mat_low = [name in ("MAT1", "MAT2") for name, _w, _s, _o in low.ops]
        assert sum(mat_entry) == sum(mat_low) == 2
        g_ref, cots_ref = adjoint.adjoint_slot_and_matrices_gradient(low, n, B, groups, w, want, mat_low, x64=x64)
        ft, ct = (torch.float64, torch.complex128) if x64 else (torch.float32, torch.complex64)
        sw = adjoint.plan_segments(tape, n, want, mat_entry, x64)
        (sg,) = sw.segments
        pair = torch.empty((2 * B, 1 << n), dtype=ct, device="cuda")
        a_f = torch.from_numpy(low.angle_table(B, dtype=np.float64 if x64 else np.float32)).cuda()
        plan = get_plan(low, (simulation.PLAN_FLAGS or 0) | N.PLAN_NO_MERGE) if x64 else get_plan(low)
        if x64:
            plan.run64(a_f, "state", out=pair[:B])
        else:
            plan.run(a_f, "state", out=pair[:B])
        N.apply_pauli_sum(pair[:B], adjoint._z_seed_terms(groups), torch.from_numpy(w).to(ft).cuda(), out=pair[B:])
        a_r = (a_f.index_select(1, torch.from_numpy(sg.perm).cuda()) * torch.from_numpy(sg.sign).to(ft).cuda()).contiguous()
        grad = torch.full((B, low.n_slots), 7.0, dtype=ft, device="cuda")
        cot = torch.zeros((B, sw.cot_stride), dtype=ft, device="cuda")
        N.adjoint_segment(get_plan(sg.rev, adjoint.REV_FLAGS), a_r, pair, list(sg.terms), grad, cot_off=list(sg.cot_off),
                          cot=cot, two_wire=sg.two_wire)
    grad, cot = grad.cpu().numpy(), cot.cpu().numpy()
    scale = np.maximum(1.0, np.abs(w).sum(axis=1))[:, None]
    cols = np.array(want)
    err = (np.abs(grad[:, cols] - g_ref[:, cols]) / scale).max()
    blocks = [cot[:, :8].reshape(B, 2, 2, 2), cot[:, 8:40].reshape(B, 4, 4, 2)]
    err_c = max((np.abs(b[..., 0] + 1j * b[..., 1] - c) / scale[:, :, None]).max() for b, c in zip(blocks, cots_ref))
    back = pair[:B].cpu().numpy()
    back[:, 0] -= 1.0
    print("segment n", n, "c128" if x64 else "c64", "gradient", err, "cotangents", err_c, "psi - |0>", np.abs(back).max())
    assert err <= tolerance(n, x64) and err_c <= tolerance(n, x64)
    assert np.abs(back).max() <= tolerance(n, x64)           # psi is back at |0..0>
    assert np.all(grad[:, ~cols] == 7.0)                     # a column no term names is untouched


# ---- end to end -----------------------------------------------------------------------------------------------------------
def mixed_case(n, B=2, seed=3, pauli=False):
    """A two-wire evolved gate and a three-wire one on the same tape, both with a time that is a leaf."""
    rng = np.random.default_rng(seed + n)
    base = A.make_case("middle", n, B, seed, pauli)
    k = next(i for i, st in enumerate(base.steps) if st.kind == "WIDE")
    two = A.Step("WIDE", (n - 1, 1), 1, A.random_hermitian(rng, 4))
    steps = base.steps[:k] + (two,) + base.steps[k:]
    return base._replace(name="mixed", steps=steps, t=rng.uniform(0.2, 0.9, size=(B, 2)))


def case_of(name, n, B=2, pauli=False):
    return mixed_case(n, B, pauli=pauli) if name == "mixed" else A.make_case(name, n, B, pauli=pauli)


def circuit_of(case):
    def f(theta, t):
        for st in case.steps:
            if st.kind == "WIDE":
                k = len(st.wires)
                op.Hermitian(st.H, list(range(k)), record=False).evolve()(t[st.angle], wires=list(st.wires))
            elif st.kind in ("CX", "H"):
                getattr(op, st.kind)(wires=list(st.wires))
            else:
                getattr(op, st.kind)(theta[st.angle], wires=list(st.wires))

    return f


def observables_of(case, pauli):
    n = case.n
    if pauli:
        return [op.PauliX(wires=0, record=False), op.Hermitian(matrix=np.kron(A.Z, A.Y), wires=[1, n - 1], record=False),
                op.PauliZ(wires=2, record=False)]
    return [op.PauliZ(wires=0, record=False), js.build_parity_observable([1, n - 1]), op.PauliZ(wires=2, record=False)]


def check_vjp(case, pauli, x64, leaves="both", K=1, shared_t=False):
    """``leaves``: "both" (angles and times), "theta" (the wide gates are constants of the gradient: one matrix per
    sample through in_axes, or -- ``shared_t`` -- one for all samples)."""
    B, n = case.theta.shape[0], case.n
    if shared_t:
        case = case._replace(t=np.repeat(case.t[:1], B, axis=0))
    rng = np.random.default_rng(11)
    weights = [case.weights] + [rng.uniform(-1, 1, size=case.weights.shape) for _ in range(K - 1)]
    s = Script(f=circuit_of(case), n_qubits=n)
    cot = np.stack(weights) if K > 1 else weights[0]
    kw = dict(args=(case.theta, case.t[0] if shared_t else case.t), in_axes=(0, None if shared_t else 0),
              pauli_seed=pauli, wide_gates=True)
    with x64_scope(x64):
        if leaves == "both":
            got = s.vjp(observables_of(case, pauli), cot, argnums=(0, 1), through_evolve=True, **kw)
        else:
            got = s.vjp(observables_of(case, pauli), cot, argnums=(0,), **kw)
    worst = 0.0
    for k, w in enumerate(weights):
        g_theta, g_t, _cots = A.gradients(case._replace(weights=w))
        scale = np.maximum(1.0, np.abs(w).sum(axis=1))[:, None]
        mine = [g[k] for g in got] if K > 1 else list(got)
        assert mine[0].shape == g_theta.shape
        worst = max(worst, (np.abs(mine[0] - g_theta) / scale).max())
        if leaves == "both":
            assert mine[1].shape == g_t.shape
            worst = max(worst, (np.abs(mine[1] - g_t) / scale).max())
    print(case.name, "n", n, "pauli" if pauli else "z", "c128" if x64 else "c64", leaves, "K", K, "worst", worst)
    assert worst <= tolerance(n, x64), worst


@pytest.mark.parametrize("x64", [False, True], ids=["c64", "c128"])
@pytest.mark.parametrize("name,n,pauli", [("middle", 4, False), ("first", 5, True), ("last", 6, False), ("two", 5, True),
                                          ("unsorted", 4, True), ("mixed", 5, False)])
def test_vjp_by_the_times_and_the_angles_at_once(name, n, pauli, x64):
    check_vjp(case_of(name, n, pauli=pauli), pauli, x64)


@pytest.mark.parametrize("x64", [False, True], ids=["c64", "c128"])
@pytest.mark.parametrize("name,n,pauli,shared", [("middle", 5, False, True), ("two", 6, False, False),
                                                 ("first", 4, True, False), ("last", 5, True, True)])
def test_vjp_with_wide_gates_that_are_constants_of_the_gradient(name, n, pauli, shared, x64):
    """one matrix for all samples (``shared``) or one per sample through in_axes: the sweep just inverts them"""
    check_vjp(case_of(name, n, B=3, pauli=pauli), pauli, x64, leaves="theta", shared_t=shared)


@pytest.mark.parametrize("x64", [False, True], ids=["c64", "c128"])
def test_vjp_with_k_stacked_cotangents(x64):
    check_vjp(case_of("two", 5, pauli=False), False, x64, K=3)
    check_vjp(case_of("mixed", 4, pauli=True), True, x64, K=2)


def test_vjp_at_fourteen_qubits():
    check_vjp(case_of("middle", 14, B=1, pauli=False), False, False)


def test_a_batch_cut_inside_the_call_equals_the_whole_batch(monkeypatch):
    from qml_essentials_amd import memory

    case = case_of("two", 5, B=5)
    s = Script(f=circuit_of(case), n_qubits=5)
    kw = dict(args=(case.theta, case.t), in_axes=(0, 0), argnums=(0, 1), through_evolve=True, wide_gates=True)
    whole = s.vjp(observables_of(case, False), case.weights, **kw)
    calls = []

    def small(*a, **k):
        calls.append(a)
        return 4  # two states per sample: chunks of two samples

    monkeypatch.setattr(memory, "compute_chunk_size", small)
    cut = s.vjp(observables_of(case, False), case.weights, **kw)
    assert calls
    for a, b in zip(whole, cut):
        assert np.array_equal(a, b)
    g_theta, g_t, _ = A.gradients(case)
    scale = np.maximum(1.0, np.abs(case.weights).sum(axis=1))[:, None]
    assert (np.abs(cut[0] - g_theta) / scale).max() <= tolerance(5, False)
    assert (np.abs(cut[1] - g_t) / scale).max() <= tolerance(5, False)


def test_what_stays_refused_with_the_keyword():
    def noisy(s):
        op.RX(s, wires=0)
        op.Hermitian(np.kron(np.kron(A.Z, A.Z), A.X), [0, 1, 2]).evolve()(0.2, wires=[0, 1, 2])
        op.BitFlip(0.1, wires=0)

    obs = [op.PauliZ(wires=0, record=False)]
    with pytest.raises(NotImplementedError, match="noisy"):
        Script(f=noisy, n_qubits=3).vjp(obs, np.ones(1), args=(np.array(0.3),), wide_gates=True)

    def wide(s):
        op.RX(s, wires=0)
        op.Hermitian(np.kron(np.kron(A.Z, A.Z), A.X), [0, 1, 2]).evolve()(0.2, wires=[0, 1, 2])

    with pytest.raises(NotImplementedError, match="generic 3-qubit"):  # the parameter shift lowers the whole tape
        Script(f=wide, n_qubits=3).gradient(obs, args=(np.array(0.3),))


@pytest.mark.parametrize("x64", [False, True], ids=["c64", "c128"])
def test_pulse_leaves_beside_a_wide_gate_equal_the_tape_with_the_gate_in_factors(x64):
    """Pulse leaves go through their segment's matrix cotangents.  The reference is the sweep that existed, on the
    same tape with the wide gate -- the product CX(0, 1) CX(1, 2) as one 8x8 matrix -- written as its two factors;
    each route is held to ``tolerance`` elsewhere, so they are within twice that of each other."""
    from qml_essentials_amd.gates import PulseGates, PulseInformation

    PulseInformation.reset_defaults()
    P = op.prod(op.CX(wires=[0, 1], record=False), op.CX(wires=[1, 2], record=False))

    def circuit(as_matrix):
        def f(w):
            PulseGates.RX(w[0], wires=0)
            PulseGates.RY(w[1], wires=1)
            op.H(wires=2)
            op.RZ(w[2], wires=2)
            if as_matrix:
                op.Operation(wires=P.wires, matrix=P.matrix, name=P.name)
            else:
                op.CX(wires=[1, 2])
                op.CX(wires=[0, 1])
            PulseGates.RX(0.5 * w[0], wires=2)
            op.RY(w[3], wires=0)

        return f

    w = np.array([0.7, 1.3, -0.4, 2.1])
    obs = [op.PauliZ(wires=q, record=False) for q in range(3)]
    cot = np.array([0.8, -1.1, 0.6])
    try:
        with x64_scope(x64):
            (got,) = Script(f=circuit(True), n_qubits=3).vjp(obs, cot, args=(w,), wide_gates=True)
            (want,) = Script(f=circuit(False), n_qubits=3).vjp(obs, cot, args=(w,))
    finally:
        PulseInformation.reset_defaults()
    err = np.abs(got - want).max() / max(1.0, np.abs(cot).sum())
    print("pulse leaves beside a wide gate", "c128" if x64 else "c64", err, want)
    assert np.abs(want).min() > 1e-3  # (every element is fed)
    assert err <= 2 * tolerance(3, x64)
