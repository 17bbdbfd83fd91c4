"""Every route of the adjoint sweep against the exact complex128 gradient of tests/adjoint_reference.py.

Each test goes through ``adjoint.adjoint_slot_gradient`` -- the function ``Model.gradient(method="adjoint")``,
``Script.vjp`` and the torch bridge end in -- forces one route of ``adjoint_run`` / ``f64_adjoint_run`` and proves
that it ran:

* LDS (``k_adjoint_lds``): what the host tests, from ``get_plan(low).describe()`` -- ``whole_state_lds``, one
  stage, ``n <= 13`` -- and no 4-wire operator on the tape; for the ``DENSE4`` instantiations a group of kind 2 / 3
  among the stage's groups; for the slots-in-global-memory variant more operators than fit beside psi and lambda.
* fused (``k_tile_adj`` / ``k_adj_tile_final``): ``adjoint.REV_FLAGS = REV_FLAGS_FUSED``, so that the fallback of
  ``run_sweep`` compiles the fused plan again and a refusal arrives as ``N.Unsupported``; and every stage of the
  reverse plan is a tile stage, so no gate of the tape is left to the per-gate kernels.
* streaming (``k_adj_overlap`` / ``k_adj_final``): ``adjoint.REV_FLAGS_FUSED = REV_FLAGS``; below 14 qubits a 4-wire
  operator on the tape (asserted) keeps the sweep out of the LDS kernel.
* complex128 (``k64_*``): ``x64_scope(True)``; it has one route.

A 4-wire operator has no ``op.Operation`` form (``Operation.lower`` refuses matrices on more than 2 wires), so the
tapes carry it as ``Dense4``, an Operation that lowers to the engine's ``MAT4`` as noise channels do.  The Golomb
encoding exists on the whole register only (``DIAG_ALL``); "on three wires" at n = 14 is that operator with the marks
of the three wires repeated over the others.  Under complex128 the n = 14 tape keeps its Golomb gate but does not
differentiate it (the difference quotient is good to 1e-9, not 1e-12), so that one reference serves both precisions.

The two-round complex128 case runs at n = 13 with 16385 samples, not at n = 3: a round is ``4 GiB / (32 << n)``
samples capped at 65535, and ``N.adjoint_gradient`` cuts batches into 32767 rows before the library sees them, so no
batch reaches a second round below 13 qubits (16384 per round).  Its rows repeat three angle rows with a weight row
each of their own, so every row has an exact reference.

Tolerances (times ``max(1, sum_k |w_k|)`` of the row): 4e-6 up to 13 qubits and 1e-5 at 14-16 (the figures of
test_gpu_gradients.py and test_gpu_adjoint_pauli.py), 1e-12 in complex128.  At 19 and 20 qubits the largest error
measured on the MI355X was 1.4e-7 (n = 19, Z seed; 4.1e-8 at n = 20); the tests assert four times that, rounded up
to one digit: 6e-7.  The largest errors elsewhere: 2.5e-7 in the LDS kernel (1.3e-6 on the Golomb angle), 1.5e-7 in
the small streaming runs, 1.4e-7 fused, 1.7e-6 streaming at n = 14 (the Golomb angle; 2.9e-7 without), 6.4e-16 in
complex128.
"""
import numpy as np
import pytest

from qml_essentials_amd import adjoint, simulation
from qml_essentials_amd import operations as op
from qml_essentials_amd.script import Script
from qml_essentials_amd.simulation import get_plan
from qml_essentials_amd.utils import x64_scope
from tests import adjoint_reference as R
from tests.test_gpu_adjoint_pauli import observables

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BOUND_19_20 = 6e-7  # 4 x the measured 1.4e-7, one digit (see the module docstring)


class Dense4(op.Operation):
    """a 16x16 matrix on 4 wires as the engine's MAT4 operator"""

    def lower(self, n_qubits):
        m = np.asarray(self.matrix)
        return "MAT4", self.wires, [], np.stack([m.real, m.imag], axis=-1).astype(np.float64).reshape(-1)


GATES = {"CPhase": op.ControlledPhaseShift}


def spread_marks(wires, n):
    """the Golomb marks of ``wires`` as a diagonal of the whole register (wire w = bit n - 1 - w of the index)"""
    marks = np.asarray(R.G.golomb_ruler(2 ** len(wires)), dtype=np.float64)
    idx = np.arange(2 ** n)
    sub = np.zeros_like(idx)
    for w in wires:
        sub = (sub << 1) | ((idx >> (n - 1 - w)) & 1)
    return marks[sub]


def script_of(spec, n):
    """the spec with the package's operations; the angles arrive as one array, in tape order"""
    def circuit(th):
        for name, wires, idx, const in spec:
            if name == "Matrix":
                (Dense4 if len(wires) == 4 else op.Operation)(wires=wires, matrix=const)
            elif name == "Golomb":
                op.DiagonalQubitUnitary.from_phases(spread_marks(wires, n), th[idx[0]], wires=list(range(n)))
            else:
                GATES.get(name, getattr(op, name, None))(*[th[i] for i in idx],
                                                        wires=wires if len(wires) > 1 else wires[0])
    return Script(circuit, n_qubits=n)


def lowered(case, theta=None):
    theta = case.theta if theta is None else theta
    s = script_of(case.spec, case.n)
    _tape, low, n, B, slots, _shapes, _batched = s._trace_for_gradient([], (theta,), None, (0,), (0,))
    assert n == case.n and B == theta.shape[0] and low.n_slots == case.spec.n_theta == len(slots)
    for k in (0, low.n_slots // 2, low.n_slots - 1):  # slot k is angle k of the spec
        assert np.array_equal(np.broadcast_to(low.values[k], (B,)), theta[:, k])
    return low


def pauli_terms_of(case):
    _groups, mats, _wz, _wp = R.case_observables(case)
    obs = observables(case.n, np.random.default_rng([case.seed, case.n, 78]))
    for o, (m, wires) in zip(obs, mats):  # the observables the reference differentiated
        assert list(o.wires) == list(wires) and np.array_equal(np.asarray(o.matrix), m)
    terms = simulation.pauli_term_list(obs, case.n)
    assert terms is not None and len(obs) == len(mats)
    return terms


def tolerance(n, x64):
    return 1e-12 if x64 else 4e-6 if n <= 13 else 1e-5 if n <= 16 else BOUND_19_20


def sweep(case, low, seed, x64=False, wanted=None, weights=None):
    """-> (gradient [B, n_theta] from the sweep, weights)"""
    groups, _mats, wz, wp = R.case_observables(case)
    wanted = case.wanted if wanted is None else wanted
    want = [k in set(wanted) for k in range(low.n_slots)]
    w = weights if weights is not None else (wz if seed == "z" else wp)
    B = w.shape[0]
    with x64_scope(x64):
        if seed == "z":
            return adjoint.adjoint_slot_gradient(low, case.n, B, groups, w, want, x64=x64), w
        return adjoint.adjoint_slot_gradient(low, case.n, B, None, w, want, x64=x64, obs_terms=pauli_terms_of(case)), w


def compare(case, got, seed, x64=False, wanted=None):
    """every row against the reference; columns that were not asked for are exactly zero"""
    wanted = case.wanted if wanted is None else wanted
    ref = R.case_gradients(case.name)[0 if seed == "z" else 1]
    _groups, _mats, wz, wp = R.case_observables(case)
    w = wz if seed == "z" else wp
    tol = tolerance(case.n, x64)
    rest = [k for k in range(case.spec.n_theta) if k not in set(wanted)]
    assert got.shape == ref.shape and not got[:, rest].any()
    worst = 0.0
    for b in range(ref.shape[0]):
        err = np.abs(got[b, wanted] - ref[b, wanted]).max() / max(1.0, np.abs(w[b]).sum())
        worst = max(worst, err)
        assert err <= tol, (case.name, seed, "row", b, "angle", wanted[int(np.abs(got[b, wanted] - ref[b, wanted]).argmax())],
                            err, tol)
    print(case.name, seed, "x64" if x64 else "c64", "max |sweep - reference| / max(1, sum|w|)", worst, "tolerance", tol)
    return worst


@pytest.fixture(autouse=True)
def fresh_reverse_tapes():
    adjoint._REV_CACHE.clear()
    yield
    adjoint._REV_CACHE.clear()


def force(monkeypatch, route):
    if route == "fused":
        monkeypatch.setattr(adjoint, "REV_FLAGS", adjoint.REV_FLAGS_FUSED)
    elif route == "streaming":
        monkeypatch.setattr(adjoint, "REV_FLAGS_FUSED", adjoint.REV_FLAGS)


def reverse_plan_stages(flags):
    """the stage kinds of the reverse plan the last sweep ran"""
    (rev, _terms, _perm), = list(adjoint._REV_CACHE.values())[-1:]
    return [st["kind"] for st in get_plan(rev, flags).describe()["stages"]]


def assert_lds(low, n, dense4=None, more_ops_than=None):
    names = [o[0] for o in low.ops]
    d = get_plan(low).describe()
    assert d["whole_state_lds"] and len(d["stages"]) == 1 and n <= 13 and "MAT4" not in names
    kinds = {g["kind"] for g in d["stages"][0]["groups"]}
    if dense4 is not None:
        assert bool(kinds & {2, 3}) == dense4, kinds
    if more_ops_than is not None:
        assert d["stages"][0]["n_lowered"] > more_ops_than, d["stages"][0]["n_lowered"]
    return d


SEEDS = ["z", "pauli"]


# ---- the LDS kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 13])
def test_lds_sweep_every_gate_kind(n, seed):
    """k_adjoint_lds<false, *> up to 3 qubits; from 7 qubits on the plan compiler forms a group of kind 3 from the
    tape's 2-wire gates, so these run k_adjoint_lds<true, *> (the 13-qubit run of
    test_lds_sweep_operator_slots_in_global_memory is the <false, *> one at full size).  n = 7 / 8 straddle the
    switch to 256 threads."""
    case = R.cases()[f"lds_all_n{n}"]
    low = lowered(case)
    assert_lds(low, n, dense4=n > 3)
    compare(case, sweep(case, low, seed)[0], seed)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", [4, 13])
def test_lds_sweep_with_a_dense_forward_group(n, seed):
    """k_adjoint_lds<true, *>: an explicit 2-wire matrix gives the forward plan a dense group"""
    case = R.cases()[f"lds_dense_n{n}"]
    low = lowered(case)
    assert_lds(low, n, dense4=True)
    compare(case, sweep(case, low, seed)[0], seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_lds_sweep_golomb_marks(seed):
    """the marks table in the LDS kernel: the Golomb encoding on 5 wires, differentiated with respect to its input"""
    case = R.cases()["lds_golomb_n5"]
    low = lowered(case)
    assert_lds(low, 5) and "DIAG_ALL" in [o[0] for o in low.ops]
    compare(case, sweep(case, low, seed)[0], seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_lds_sweep_operator_slots_in_global_memory(seed):
    """slots_in_lds = 0: n_ops * 48 > 160 KiB - (16 << 13) - 288 * 4, i.e. more than 658 forward operators"""
    case = R.cases()["lds_deep_n13"]
    low = lowered(case)
    assert_lds(low, 13, dense4=False, more_ops_than=658)
    compare(case, sweep(case, low, seed)[0], seed)


def test_lds_sweep_32_z_parities():
    """the kernel's zmask array full"""
    case = R.cases()["lds_32_parities_n6"]
    low = lowered(case)
    assert_lds(low, 6) and len(R.case_observables(case)[0]) == 32
    compare(case, sweep(case, low, "z")[0], "z")


# ---- the streaming kernels on a handful of chunks ---------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", [4, 6])
def test_streaming_sweep_below_14_qubits(n, seed, monkeypatch):
    """a 4-wire operator on the tape: k_adj_overlap on 8 and 32 float4 chunks per state, generators on position 0
    (swap01) and controlled from it (pmask & 1)"""
    case = R.cases()[f"mat4_n{n}"]
    low = lowered(case)
    assert "MAT4" in [o[0] for o in low.ops] and get_plan(low).describe()["whole_state_lds"]
    force(monkeypatch, "streaming")
    compare(case, sweep(case, low, seed)[0], seed)


# ---- the fused tile passes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("third", [False, True], ids=["every_angle", "every_third_angle"])
@pytest.mark.parametrize("n", [14, 16])
def test_fused_sweep_every_control_target_class(n, third, seed, monkeypatch):
    """k_tile_adj: X / Y / Z / P1 generators with and without a control, controls and targets on positions 0-3,
    4-11 and >= 12; every third angle only: slots without a term and stages without terms"""
    case = R.cases()[f"tile_third_n{n}" if third else f"tile_n{n}"]
    low = lowered(case)
    force(monkeypatch, "fused")
    got = sweep(case, low, seed)[0]  # (a refusal of the fused plan raises N.Unsupported here)
    kinds = reverse_plan_stages(adjoint.REV_FLAGS_FUSED)
    assert kinds and set(kinds) == {"tile"}, kinds
    compare(case, got, seed)


# ---- the streaming kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", ["wide_golomb_n14", "wide_n15"])
def test_streaming_sweep_from_14_qubits(name, seed, monkeypatch):
    """k_adj_overlap / k_adj_final: the fused tape plus RXX, RYY, RZZ, RZX on pairs with position 0 and a position
    >= 12, a SWAP, a CCX, a 2-wire matrix and (n = 14) the Golomb marks"""
    case = R.cases()[name]
    low = lowered(case)
    force(monkeypatch, "streaming")
    compare(case, sweep(case, low, seed)[0], seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_fused_and_streaming_sweeps_agree(seed, monkeypatch):
    """one tape on both routes: within twice the route tolerance of each other (each is held to the reference above)"""
    case = R.cases()["tile_n14"]
    low = lowered(case)
    force(monkeypatch, "fused")
    fused, w = sweep(case, low, seed)
    monkeypatch.undo()
    adjoint._REV_CACHE.clear()
    force(monkeypatch, "streaming")
    streamed, _ = sweep(case, low, seed)
    err = (np.abs(fused - streamed).max(axis=1) / np.maximum(1.0, np.abs(w).sum(axis=1))).max()
    print("n 14", seed, "max |fused - streaming| / max(1, sum|w|)", err)
    assert err <= 2 * tolerance(14, False)
    compare(case, streamed, seed)


# ---- the reduction kernels' thresholds -------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", [19, 20])
def test_streaming_sweep_reduction_thresholds(n, seed, monkeypatch):
    """adj_blocks = 128 (k_adj_final with 64 threads, two strides) and 256 (the 256-thread launch)"""
    case = R.cases()[f"threshold_n{n}"]
    gz, gp = R.case_gradients(case.name)
    assert min(np.abs(gz[:, case.wanted]).min(), np.abs(gp[:, case.wanted]).min()) >= 1e-3  # (not checked on the CPU)
    low = lowered(case)
    force(monkeypatch, "streaming")
    compare(case, sweep(case, low, seed)[0], seed)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", [18, 19])
def test_complex128_sweep_reduction_thresholds(n, seed):
    """f64_adj_blocks = 128 / 256: k_adj_final<double2, double> with 64 and with 256 threads"""
    case = R.cases()[f"threshold_n{n}"]
    compare(case, sweep(case, lowered(case), seed, x64=True)[0], seed, x64=True)


# ---- the complex128 sweep ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", ["lds_all_n3", "lds_all_n8", "mat4_n4", "wide_golomb_n14"])
def test_complex128_sweep(name, seed):
    case = R.cases()[name]
    wanted = [k for k in case.wanted if k not in R.golomb_angles(case.spec)]
    compare(case, sweep(case, lowered(case), seed, x64=True, wanted=wanted)[0], seed, x64=True, wanted=wanted)


@pytest.mark.parametrize("seed", SEEDS)
def test_complex128_sweep_in_two_rounds(seed):
    """16385 samples at n = 13: a round of 16384 and a ragged one of 1; every row against its reference"""
    case = R.cases()["lds_all_n13"]
    B, rows = 16385, case.theta.shape[0]
    assert (4 << 30) // (32 << 13) == B - 1 and B <= 32767
    rng = np.random.default_rng(14)
    groups, mats, _wz, _wp = R.case_observables(case)
    nz = len(groups)
    w = rng.uniform(0.5, 1.5, (B, nz if seed == "z" else len(mats))) * rng.choice([-1.0, 1.0], (B, 1))
    pick = np.arange(B) % rows
    low = lowered(case, case.theta[pick])
    got, _ = sweep(case, low, seed, x64=True, weights=w)
    jac = R.case_jacobians(case.name)
    cols = slice(0, nz) if seed == "z" else slice(nz, None)
    ref = np.einsum("bk,btk->bt", w, jac[pick][:, :, cols])
    err = np.abs(got - ref).max(axis=1) / np.maximum(1.0, np.abs(w).sum(axis=1))
    print("two rounds", seed, "max |sweep - reference| / max(1, sum|w|)", err.max(), "last row", err[-1])
    assert got.shape == ref.shape and err.max() <= 1e-12


# ---- angles that reach their gates through arithmetic ------------------------------------------------------------
def test_vjp_folds_the_sweep_onto_arguments_by_the_chain_rule():
    """Script.vjp on angles th[0] * x, th[1] + x and th[0] once more: the reference gradient per gate occurrence,
    folded by the chain rule"""
    spec, x, th, angles, tangents = R.chain_case()
    mats = R.pauli_mats(3, np.random.default_rng(9))
    obs = observables(3, np.random.default_rng(9))
    cot = np.array([0.8, -1.1, 0.6, 1.3, -0.7])
    ref = R.chain_rule(R.reference_gradient(lambda t: R.oracle_tape(spec, t), angles(th), 3,
                                            lambda psi: float(cot @ R.expectations(psi, 3, mats))), tangents, 2)

    def circuit(a):
        given = [a[0] * x, a[1] + x, a[0]]
        for name, wires, idx, const in spec:
            if name == "Matrix":
                op.Operation(wires=wires, matrix=const)
            else:
                getattr(op, name)(*[given[i] for i in idx], wires=wires if len(wires) > 1 else wires[0])

    s = Script(circuit, n_qubits=3)
    (g32,) = s.vjp(obs, cot, args=(th,), pauli_seed=True)
    with x64_scope(True):
        (g64,) = s.vjp(obs, cot, args=(th,), pauli_seed=True)
    e32, e64 = np.abs(g32 - ref).max(), np.abs(g64 - ref).max()
    print("chain rule: float32 err", e32, "complex128 err", e64)
    assert min(np.abs(ref)) >= 1e-3 and e32 <= 4e-6 * np.abs(cot).sum() and e64 <= 1e-12
