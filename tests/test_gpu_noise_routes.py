"""Noisy circuits past eight doubled wires, on every route the engine has for them, against the oracle's complex128
``simulate_mixed`` (``noise_reference.simulate_mixed_fast``).  tests/test_noise_reference_cpu.py asserts, without a
GPU, which routes the plans below take -- the whole-state tile of 10, 12 and 14 wires, and 12- / 13-wire tiles over
arbitrary bit sets whose later stages load their tiles, with 16 x 16 groups (GK_DENSE4, GK_REG4X) in them -- and that
the metric below sees a dropped channel, exchanged wires and a missing conjugation with a margin of 100.

Tolerances.  complex64 rho: ``rel_err = ||got - want||_F / ||want||_F <= 16 * c64_floor``, where ``c64_floor`` is the
same ``rel_err`` of the oracle's own complex64 run of that tape against its complex128 run (1e-7 .. 8e-7 here, so the
bound is 2e-6 .. 1.3e-5 of the norm: the project's 2e-6 read relatively).  The factor is reasoned: the oracle's
complex64 run rounds the stored rho once per operation and computes in complex128; the engine also takes a 16-term
complex dot product per element of a 16 x 16 operator in float32 and builds products of up to six 4 x 4 matrices in
float32.  Every test prints ``rel_err / c64_floor``; profiles/noise_parity.md records them.
complex128 rho: ``rel_err < 1e-12``.  Probabilities and expectation values: the absolute 2e-6 of tests/test_gpu_noise.py,
1e-5 with a ``Hermitian`` among the observables."""
import numpy as np
import pytest

from oracle import dense as OD
from oracle import noise as ON

import noise_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FACTOR = 16
X64_RTOL = 1e-12
ATOL, ATOL_HERMITIAN = 2e-6, 1e-5


def _N():
    from qml_essentials_amd import _native as N

    return N


def _flag_sets():
    N = _N()
    return {"default": 0, "no_sparse": N.PLAN_NO_SPARSE, "no_regtile": N.PLAN_NO_REGTILE, "no_fusion": N.PLAN_NO_FUSION,
            "tile10_low4": N.plan_flags(force_global=True, force_tile=True, tile_bits=10, low_bits=4),
            "tile10_low7": N.plan_flags(force_global=True, force_tile=True, tile_bits=10, low_bits=7),
            "tile11": N.plan_flags(tile_bits=11)}


FLAG_NAMES = ["default", "no_sparse", "no_regtile", "no_fusion", "tile10_low4", "tile10_low7", "tile11"]


def _check_rho(label, got, tape, row=0, floor_row=0):
    """One complex64 sample against the reference of that row; the floor is the tape's (its rows share the structure)."""
    want, floor = R.reference_rho(tape, row), R.tape_floor(tape, floor_row)
    err = R.rel_err(np.asarray(got).reshape(want.shape), want)
    print(f"{label} row {row}: rel_err {err:.3e} = {err / floor:.2f} x c64_floor {floor:.3e}")
    assert err <= FACTOR * floor, (label, row, err, floor)


def _replay(tape):
    from qml_essentials_amd.script import Script
    from qml_essentials_amd.tape import shift_and_append

    return Script(f=lambda: shift_and_append(tape.ops, 0), n_qubits=tape.n)


# ---- a. the engine, every geometry -------------------------------------------------------------------------
def _run_state(tape, flags):
    low, plan = R.lowered(tape, flags)
    batch = max(int(np.shape(v)[0]) for v in low.values if np.ndim(v))
    angles = torch.from_numpy(low.angle_table(batch)).cuda()
    return plan.run(angles, "state").cpu().numpy()


@pytest.mark.parametrize("flags", FLAG_NAMES)
@pytest.mark.parametrize("case", R.ENGINE_CASES, ids=["-".join(map(str, c)) for c in R.ENGINE_CASES])
def test_engine_evolves_vec_rho_on_every_geometry(case, flags):
    tape = R.route_tape(*case)
    got = _run_state(tape, _flag_sets()[flags])
    assert got.shape == (R.BATCH, 4 ** tape.n)
    for row in range(R.BATCH):
        _check_rho(f"{'-'.join(map(str, case))} {flags}", got[row], tape, row)


def test_a_batch_with_a_ragged_last_chunk():
    tape = R.route_tape(*R.RAGGED_CASE)
    got = _run_state(tape, 0)
    assert got.shape == (33, 4 ** tape.n)
    for row in (0, 32):
        _check_rho("spread-8 batch 33", got[row], tape, row)
    assert np.abs(got[32] - got[0]).max() > 1e-4


# ---- b. wide channels: operators applied in place on a resident vec(rho) ------------------------------------------
@pytest.mark.parametrize("case", R.WIDE_CASES, ids=["-".join(map(str, c)) for c in R.WIDE_CASES])
def test_wide_channels_on_a_resident_state(case):
    tape = R.route_tape(*case)
    assert sorted(len(o.wires) for o in tape.ops if id(o) in tape.depol)[-2:] == [3, 4]
    rho = _replay(tape).execute(type="density")
    assert rho.dtype == np.complex64
    _check_rho("-".join(map(str, case)), rho, tape)


@pytest.mark.parametrize("case", [R.WIDE_CASES[0], R.WIDE_CASES[2]], ids=["n7", "n9"])
def test_wide_channels_on_a_resident_state_in_x64(case):
    from qml_essentials_amd.utils import x64_scope

    tape = R.route_tape(*case)
    with x64_scope(True):
        rho = _replay(tape).execute(type="density")
    err = R.rel_err(rho, R.reference_rho(tape))
    print(f"{'-'.join(map(str, case))} x64: rel_err {err:.3e}")
    assert rho.dtype == np.complex128 and err < X64_RTOL


# ---- c. the noisy model, compiled and recorded -----------------------------------------------------------------
def _check_model(label, got, execution_type, ansatz, n, layers, state_prep=True):
    _model, params, inputs, _noise = R.model_case(ansatz, n, layers, state_prep)
    floor_tape = R.model_sample_tape(ansatz, n, layers, state_prep, 0, 0)
    assert got.shape[:2] == (len(inputs), len(params))
    zs = [OD.lift(ON.Z, [q], n) for q in range(n)]
    for i in range(len(inputs)):
        for p in range(len(params)):
            tape = R.model_sample_tape(ansatz, n, layers, state_prep, i, p)
            rho = R.reference_rho(tape)
            if execution_type == "density":
                floor = R.tape_floor(floor_tape)
                err = R.rel_err(got[i, p], rho)
                print(f"{label} sample ({i}, {p}): rel_err {err:.3e} = {err / floor:.2f} x c64_floor {floor:.3e}")
                assert err <= FACTOR * floor, (label, i, p, err, floor)
            elif execution_type == "probs":
                err = np.abs(got[i, p].reshape(-1) - np.real(np.diag(rho))).max()
                print(f"{label} sample ({i}, {p}): probs max err {err:.3e}")
                assert err <= ATOL
            else:
                err = np.abs(got[i, p] - ON.measure_density(rho, n, "expval", zs)).max()
                print(f"{label} sample ({i}, {p}): expval max err {err:.3e}")
                assert err <= ATOL


@pytest.mark.parametrize("execution_type", ["density", "probs", "expval"])
@pytest.mark.parametrize("ansatz,n,layers", R.MODEL_CASES, ids=[f"{a}-{n}" for a, n, _ in R.MODEL_CASES])
def test_noisy_model_compiled(ansatz, n, layers, execution_type):
    model, params, inputs, noise = R.model_case(ansatz, n, layers)
    model.host_arrays_via_device = True
    got = model(params=params, inputs=inputs, noise_params=dict(noise), execution_type=execution_type)
    assert any(cc.density for cc in model.script._compiled.values())
    _check_model(f"{ansatz}-{n} compiled {execution_type}", np.asarray(got), execution_type, ansatz, n, layers)


@pytest.mark.parametrize("execution_type", ["density", "probs", "expval"])
@pytest.mark.parametrize("ansatz,n,layers", R.MODEL_CASES, ids=[f"{a}-{n}" for a, n, _ in R.MODEL_CASES])
def test_noisy_model_recorded(ansatz, n, layers, execution_type):
    from qml_essentials_amd.model import Model

    _model, params, inputs, noise = R.model_case(ansatz, n, layers)
    slow = Model(n_qubits=n, n_layers=layers, circuit_type=ansatz, output_qubit=-1)
    slow.host_arrays_via_device = False  # -> script.execute records the tape per call
    got = slow(params=params, inputs=inputs, noise_params=dict(noise), execution_type=execution_type)
    assert not slow.script._compiled
    _check_model(f"{ansatz}-{n} recorded {execution_type}", np.asarray(got), execution_type, ansatz, n, layers)


def test_noisy_model_without_state_preparation():
    """The first stages of its plan carry known zeros (tests/test_noise_reference_cpu.py)."""
    ansatz, n, layers = R.NO_STATE_PREP
    model, params, inputs, noise = R.model_case(ansatz, n, layers, False)
    assert "StatePreparation" not in noise
    got = model(params=params, inputs=inputs, noise_params=dict(noise), execution_type="density")
    assert any(cc.density for cc in model.script._compiled.values())
    _check_model(f"{ansatz}-{n} bare", np.asarray(got), "density", ansatz, n, layers, False)


# ---- d. observables on the evolved state --------------------------------------------------------------------
def test_observables_of_the_evolved_state_at_eight_qubits():
    from qml_essentials_amd import jaqsi as js
    from qml_essentials_amd import operations as op

    n = 8
    tape = R.route_tape("spread", n, 0, R.BATCH)
    rng = np.random.default_rng(8)
    h = rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8))
    h = h + h.conj().T
    h /= np.linalg.norm(h, 2)  # spectral norm 1: an O(1) expectation value
    xyz = op.prod(op.PauliX(7, record=False), op.PauliY(0, record=False), op.PauliZ(3, record=False))
    obs = [op.PauliZ(wires=0, record=False), op.PauliZ(wires=7, record=False), js.build_parity_observable([0, 3, 7]),
           op.PauliX(wires=4, record=False), op.PauliY(wires=7, record=False), xyz,
           op.Hermitian(h, wires=[6, 0, 3], record=False)]
    dense = [OD.lift(np.asarray(o.matrix), o.wires, n) for o in obs]
    want = np.stack([ON.measure_density(R.reference_rho(tape, row), n, "expval", dense) for row in range(R.BATCH)])
    assert np.abs(want).max(axis=0).min() > 1e-3, "no observable vanishes on these states"
    script = _replay(tape)
    for what, sel, atol in (("Z", slice(0, 2), ATOL), ("Pauli words", slice(0, 6), ATOL),
                            ("with the Hermitian", slice(0, 7), ATOL_HERMITIAN)):
        got = script.execute(type="expval", obs=obs[sel])
        err = np.abs(got - want[:, sel]).max()
        print(f"observables at n = 8, {what}: max err {err:.3e}")
        assert got.shape == want[:, sel].shape and err <= atol, (what, err)
    probs = script.execute(type="probs")
    err = max(np.abs(probs[row].reshape(-1) - np.real(np.diag(R.reference_rho(tape, row)))).max()
              for row in range(R.BATCH))
    print(f"probabilities at n = 8: max err {err:.3e}")
    assert err <= ATOL
