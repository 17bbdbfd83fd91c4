"""Host side of wide gates and wide channels on noisy tapes: the NumPy reference of tests/density_wide_reference.py
against the oracle's ``apply_to_density`` and against its own wrong variants; the automatic rule and the status codes of
``qmle_density_apply_wide`` without a device; what ``simulation.doubled_tape`` emits for an explicit matrix on three or
four wires; the refusals that stay, with and without ``wide_gates=True``; the new kernels' resources."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import density_wide_reference as R
from oracle import noise as ON
from qml_essentials_amd import _native as N
from qml_essentials_amd import adjoint, simulation
from qml_essentials_amd import operations as op
from qml_essentials_amd.script import NotAffine, Script
from qml_essentials_amd.tape import recording
from qml_essentials_amd.unitary import UnitaryGates

CASES = [(3, 4, (3, 0, 2)), (4, 5, (1, 3, 0, 4)), (3, 5, (0, 1, 2)), (4, 4, (3, 2, 1, 0))]


def _density(n, rng):
    a = rng.normal(size=(2 ** n, 2 ** n)) + 1j * rng.normal(size=(2 ** n, 2 ** n))
    rho = a @ a.conj().T
    return rho / np.trace(rho)


# ---- the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n,wires", CASES)
@pytest.mark.parametrize("kind", ["unitary", "half1", "depol"])
def test_the_reference_equals_the_oracle_on_density_matrices(k, n, wires, kind):
    rng = np.random.default_rng([7, k, n])
    rho, ops = _density(n, rng), R.operators(kind, k, 1, rng)
    want = ON.apply_to_density(rho, n, "QubitChannel", list(wires), (list(ops),))
    got = R.apply_wide(rho, n, list(wires), ops)
    assert np.abs(got - want).max() <= 1e-14
    # the superoperator in the front end's index order says the same
    d = 2 ** k
    x, back = R._blocks(rho, n, list(wires))
    assert np.abs(back(R.superoperator(ops) @ x.reshape(d * d, -1)) - want).max() <= 1e-14


def test_the_superoperator_has_the_front_ends_index_order():
    with recording():
        ch = UnitaryGates.NQubitDepolarizingChannel(0.3, [0, 1])
    assert np.allclose(R.superoperator(np.stack(ch.kraus_matrices())), ch.superoperator(), atol=1e-15)


@pytest.mark.parametrize("k,n,wires", CASES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_every_case_tells_every_applicable_wrong_variant_apart(k, n, wires, kind):
    """Each wrong variant misses the truth by at least 100 times the bound the GPU tests use for that case."""
    rho, ops, want = R.case(n, k, wires, kind, 3 if kind == "per_sample" else 1)
    for b in range(rho.shape[0]):
        o = ops[b:b + 1] if kind == "per_sample" else ops
        floors = [R.c64_floor(rho[b], n, list(wires), o, form, want[b]) for form in ("sandwich", "superoperator")]
        bound = R.FACTOR * max(floors)
        assert 1e-8 < min(floors) and bound < 1e-4, floors
        variants = R.applicable(kind, len(o))
        assert "first_only" in variants or len(o) == 1
        for name in variants:
            miss = R.rel_err(R.WRONG[name](rho[b], n, list(wires), o), want[b])
            assert miss >= R.MARGIN * bound, (name, miss, bound)


def test_on_a_real_symmetric_input_exchanged_halves_show_only_as_a_conjugate():
    """Why the cases are generic complex arrays: sum conj(K) rho K^T = conj(sum K conj(rho) K^+)."""
    rng = np.random.default_rng(3)
    rho, ops = _density(4, rng).real, R.operators("half", 3, 1, rng)
    wrong = R.WRONG["halves_exchanged"](rho, 4, [3, 0, 2], ops)
    assert np.allclose(wrong, np.conj(R.apply_wide(rho, 4, [3, 0, 2], ops)), atol=1e-14)


# ---- the library without a device ----------------------------------------------------------------------------------------
def test_the_automatic_rule():
    lib = N.lib()
    for k in (3, 4):
        d = 2 ** k
        assert lib.qmle_density_apply_wide_form(k, 1, 0) == 1
        # at n_ops = d / 2, where the arithmetic of the two forms is level, and beyond: the superoperator -- the measured
        # times cross earlier (profiles/density_wide.md): after one operator at k = 3, after four at k = 4
        assert lib.qmle_density_apply_wide_form(k, d // 2, 0) == 2
        assert lib.qmle_density_apply_wide_form(k, d // 2 + 1, 0) == 2
        last = 1 if k == 3 else 4
        assert lib.qmle_density_apply_wide_form(k, last, 0) == 1 and lib.qmle_density_apply_wide_form(k, last + 1, 0) == 2
        assert lib.qmle_density_apply_wide_form(k, d * d, 0) == 2
        assert lib.qmle_density_apply_wide_form(k, 1, 1) == 1
        assert lib.qmle_density_apply_wide_form(k, 2, 1) == -1 and lib.qmle_density_apply_wide_form(k, 0, 0) == -1
        assert lib.qmle_density_apply_wide_form(k, 1, 2) == -1
        for n_ops in (1, 2, 4, 5, d // 2, d // 2 + 1, d * d):
            assert {1: "sandwich", 2: "superoperator"}[lib.qmle_density_apply_wide_form(k, n_ops, 0)] == R.auto_form(k, n_ops)
    assert lib.qmle_density_apply_wide_form(2, 1, 0) == -10 and lib.qmle_density_apply_wide_form(5, 1, 0) == -10


def test_argument_errors_are_statuses_without_a_device():
    lib = N.lib()
    null, one = C.c_void_p(None), C.c_void_p(256)  # (never followed: every call below is refused first)
    big = 1 << 40

    def call(rho=one, n=5, batch=1, f64=0, wires=(0, 1, 2), k=None, ops=one, n_ops=1, per_sample=0, form=0, ws=one,
             ws_bytes=big):
        k = len(wires) if k is None else k
        w = None if wires is None else (C.c_int32 * max(1, len(wires)))(*wires)
        return lib.qmle_density_apply_wide(rho, n, batch, f64, w, k, ops, n_ops, per_sample, form, ws, ws_bytes, null)

    def query(n=5, batch=1, k=3, n_ops=1, f64=0, form=0):
        return lib.qmle_density_apply_wide_workspace_bytes(n, batch, k, n_ops, f64, form)

    assert call(wires=(0, 1)) == -10 and call(wires=(0, 1, 2, 3, 4)) == -10 and call(wires=(), k=0) == -10  # UNSUPPORTED
    assert call(rho=null, wires=(0, 1, 2, 3, 4)) == -10  # the wider refusal first
    assert query(k=2) == 0 and query(k=5) == 0
    assert call(rho=null) == -1 and call(ops=null) == -1 and call(ws=null) == -1 and call(wires=None, k=3) == -1  # INVALID_ARG
    assert call(batch=0) == -1 and query(batch=0) == 0
    assert call(n=2) == -1 and query(n=2) == 0
    assert call(n=17) == -1 and query(n=17) == 0 and query(n=16) > 0  # 2n <= QMLE_MAX_QUBITS = 32
    assert call(f64=2) == -1 and query(f64=2) == 0 and call(f64=-1) == -1
    assert call(per_sample=2) == -1 and call(per_sample=-1) == -1
    assert call(form=3) == -1 and call(form=-1) == -1 and query(form=3) == 0 and query(form=-1) == 0
    assert call(n_ops=0) == -1 and query(n_ops=0) == 0
    assert call(per_sample=1, n_ops=2) == -1 and call(per_sample=1, form=2) == -1
    assert call(form=1, n_ops=65) == -1 and query(form=1, n_ops=65) == 0 and query(form=1, n_ops=64) > 0
    assert call(form=1, n_ops=257, wires=(0, 1, 2, 3)) == -1 and query(k=4, form=1, n_ops=257) == 0
    assert call(wires=(0, 1, 5)) == -4 and call(wires=(0, -1, 2)) == -4                                      # WIRE_RANGE
    assert call(wires=(0, 1, 1)) == -3 and call(wires=(3, 1, 2, 3)) == -3                                    # DUPLICATE
    # the workspace: the superoperator in the run's precision (and 256 bytes for aligning it); the sandwich keeps nothing
    assert query(k=3, n_ops=5, f64=0) == 64 * 64 * 8 + 256 and query(k=4, n_ops=9, f64=1) == 256 * 256 * 16 + 256
    assert query(k=3, n_ops=1) == 256 and query(k=4, n_ops=4) == 256 and query(k=4, n_ops=1, form=2) == 256 * 256 * 8 + 256
    assert query(k=3, n_ops=4, form=1) == 256 and query(k=3, n_ops=2) == 64 * 64 * 8 + 256
    for kw in (dict(n_ops=5), dict(n_ops=1), dict(n_ops=1, form=2), dict(n_ops=64, form=1)):
        need = query(**kw)
        assert need > 0 and call(ws_bytes=need - 1, **kw) == -7                                             # WORKSPACE


def test_the_abi_version_is_still_150_and_the_new_symbols_are_declared():
    assert N.lib().qmle_sv_version() == 150
    names = {s[0] for s in N.SYMBOLS}
    new = {"qmle_density_apply_wide", "qmle_density_apply_wide_workspace_bytes", "qmle_density_apply_wide_form"}
    assert new <= names
    header = open(os.path.join(os.path.dirname(N.LIB_PATH), "..", "include", "qmle_sv.h")).read()
    for name in new:
        assert name + "(" in header
    assert callable(N.density_apply_wide)


def test_the_kernels_are_built_without_scratch_or_spills():
    import __graft_entry__ as G

    assert "qmle_density_wide.hip" in G.UNITS
    if not os.path.exists(G.RESOURCES):
        G.build(force=True)
    res = json.load(open(G.RESOURCES))
    family = {k: v for k, v in res.items() if "k_dwide_" in k}
    # two forms x k = 3 / 4 x two precisions, and the builder of S per k and precision
    for stem, count in (("k_dwide_sandwich", 4), ("k_dwide_super", 4), ("k_dwide_build_super", 4)):
        assert len([k for k in family if stem + "I" in k]) == count, stem
    for name, r in family.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["Dynamic Stack"] == "False", name
    for name, r in family.items():  # one 4096-amplitude tile per workgroup: at least two workgroups per CU
        if "build" not in name:
            assert r["LDS Size"] in (32768, 65536) and r["Occupancy"] >= 2, (name, r)


# ---- the front end -------------------------------------------------------------------------------------------------------
def _u(k, seed=0):
    return R.operators("unitary", k, 1, np.random.default_rng(seed))[0]


def test_doubled_tape_emits_a_wide_gate_behind_the_products_that_touch_it():
    n = 5
    with recording() as tape:
        op.RX(0.3, wires=0)
        op.BitFlip(0.1, wires=0)          # pending on (0,)
        op.PhaseFlip(0.2, wires=0)        # ... multiplied into it
        op.AmplitudeDamping(0.1, wires=4)  # pending on (4,): no wire of the gate
        op.Operation(wires=[2, 0, 1], matrix=_u(3))
        op.BitFlip(0.1, wires=1)
        op.Operation(wires=[1, 2, 3, 4], matrix=np.stack([_u(4, 1), _u(4, 2)]))
    items = simulation.doubled_tape(tape, n)
    kinds = [type(it).__name__ if not isinstance(it, simulation._Lowered) else (it.name, list(it.lower(2 * n)[1])) for it in items]
    assert kinds == [("RX", [0]), ("RX", [5]), ("MAT2", [0, 5]), "_WideGate", ("MAT2", [4, 9]), ("MAT2", [1, 6]), "_WideGate"]
    g3, g4 = items[3], items[6]
    assert g3.wires == [2, 0, 1] and g3.matrix.shape == (8, 8) and g3.matrix.dtype == np.complex128
    assert g4.wires == [1, 2, 3, 4] and g4.matrix.shape == (2, 16, 16)
    # the product that was flushed before the gate is the two channels' superoperator
    with recording():
        flip, phase = op.BitFlip(0.1, wires=0), op.PhaseFlip(0.2, wires=0)
    blob = items[2].lower(2 * n)[3].reshape(4, 4, 2)
    assert np.allclose(blob[..., 0] + 1j * blob[..., 1], phase.superoperator() @ flip.superoperator(), atol=1e-15)
    # a wide channel directly behind a wide gate on overlapping wires: the two items, in tape order
    with recording() as tape2:
        op.Operation(wires=[0, 1, 2], matrix=_u(3))
        UnitaryGates.NQubitDepolarizingChannel(0.1, [2, 3, 1])
    items2 = simulation.doubled_tape(tape2, 4)
    assert [type(it).__name__ for it in items2] == ["_WideGate", "_WideChannel"]
    assert len(items2[1].kraus) == 64 and len(list(items2[1].kraus_plans(4))) == 64  # (the route the bench measures against)
    with pytest.raises(ValueError, match="does not match 3 wire"):
        simulation.doubled_tape([op.Operation(wires=[0, 1, 2], matrix=np.eye(4), record=False)], 3)


def _noisy_wide_tape():
    with recording() as tape:
        op.RX(0.3, wires=0)
        op.BitFlip(0.1, wires=0)
        op.Operation(wires=[0, 1, 2], matrix=_u(3))
    return tape


def test_without_the_keyword_the_refusal_is_unchanged(monkeypatch):
    monkeypatch.setattr(N, "require_gpu", lambda: __import__("torch"))
    with pytest.raises(NotImplementedError) as err:
        simulation.simulate_and_measure(_noisy_wide_tape(), 3, "probs")
    assert str(err.value) == ("explicit matrices on 3 or 4 wires (products of gates, evolved unitaries of three- and "
                              "four-wire Hamiltonians) are not available on noisy tapes: the density-matrix path has no "
                              "pass for them")
    with pytest.raises(NotImplementedError, match="noisy tapes"):
        simulation.simulate_and_measure(_noisy_wide_tape(), 3, "probs", wide_gates=False)

    import inspect

    assert inspect.signature(Script.execute).parameters["wide_gates"].default is False
    assert inspect.signature(simulation.simulate_and_measure).parameters["wide_gates"].default is False


def test_refusals_that_stay_with_the_keyword(monkeypatch):
    monkeypatch.setattr(N, "require_gpu", lambda: __import__("torch"))
    # five wires: a matrix (refused where it is lowered) and a channel
    with recording() as five:
        op.BitFlip(0.1, wires=0)
        op.Operation(wires=[0, 1, 2, 3, 4], matrix=np.eye(32))
    with pytest.raises(NotImplementedError, match="5-qubit"):
        simulation.simulate_and_measure(five, 5, "probs", wide_gates=True)
    with recording() as five_ch:
        op.Operation(wires=[0, 1, 2], matrix=_u(3))
        UnitaryGates.NQubitDepolarizingChannel(0.1, [0, 1, 2, 3, 4])
    with pytest.raises(NotImplementedError, match="more than 4 wires"):
        simulation.simulate_and_measure(five_ch, 5, "probs", wide_gates=True)
    # "state" of a noisy tape
    with pytest.raises(ValueError, match="not defined for mixed"):
        simulation.simulate_and_measure(_noisy_wide_tape(), 3, "state", wide_gates=True)
    # the adjoint sweep over vec(rho): wide gates and wide channels, each named
    with pytest.raises(adjoint.AdjointUnsupported, match="explicit matrix on 3 wires"):
        adjoint.plan_density(_noisy_wide_tape(), 3, [True])
    with recording() as wide_ch:
        op.RX(0.3, wires=0)
        UnitaryGates.NQubitDepolarizingChannel(0.1, [0, 1, 2])
    with pytest.raises(adjoint.AdjointUnsupported, match="channel on 3 wires"):
        adjoint.plan_density(wide_ch, 3, [True])


def test_a_compiled_call_records_a_tape_with_a_wide_gate_or_a_wide_channel():
    from qml_essentials_amd.script import CompiledCall

    def gate(x):
        op.RX(x, wires=0)
        op.BitFlip(0.1, wires=0)
        op.Operation(wires=[0, 1, 2], matrix=_u(3))

    def channel(x):
        op.RX(x, wires=0)
        UnitaryGates.NQubitDepolarizingChannel(0.1, [0, 1, 2])

    obs = [op.PauliZ(wires=0, record=False)]
    for f in (gate, channel):
        with pytest.raises(NotAffine, match="wide channel"):
            CompiledCall(Script(f, n_qubits=3), "expval", obs, (np.array(0.3),), (0,), {}, upload=False)


def test_gradient_and_the_noisy_sweep_refuse_the_tape_through_the_public_calls():
    def f(x):
        op.RX(x, wires=0)
        op.BitFlip(0.1, wires=0)
        op.Operation(wires=[0, 1, 2], matrix=_u(3))

    obs = [op.PauliZ(wires=0, record=False)]
    # the parameter shift lowers the whole tape as a pure state: the channel's own refusal, as on every noisy tape
    with pytest.raises(TypeError, match="BitFlip is a noise channel and cannot be applied to a pure statevector"):
        Script(f, n_qubits=3).gradient(obs, args=(np.array(0.3),))
    # the sweep over vec(rho) meets the wide gate where the tape is lowered, before any device work
    with pytest.raises(NotImplementedError, match="generic 3-qubit matrices are not supported"):
        Script(f, n_qubits=3).vjp(obs, np.ones(1), args=(np.array(0.3),), noisy=True)
    # (a wide CHANNEL under vjp(noisy=True) is refused by adjoint.plan_density, above; through the public call the
    # refusal needs a device and is in tests/test_gpu_density_wide_tapes.py)
