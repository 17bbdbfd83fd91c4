"""CPU side of the noisy adjoint (tests/test_gpu_density_adjoint.py): the reference gradient against a central
difference, the wrong variants it has to tell from the truth on every case the GPU runs, the host-side plan
(``adjoint.plan_density``) against the library's own count of transfers, and the argument checks of
``qmle_adjoint_density`` that return before any device work."""
import ctypes as C

import numpy as np
import pytest

from qml_essentials_amd import _native as N
from qml_essentials_amd import adjoint
from qml_essentials_amd import operations as op

import density_adjoint_reference as DR
import noise_reference as NR
import test_gpu_density_adjoint as G


# ---- the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
def test_shift_rule_equals_central_difference(n):
    tape = NR.random_noisy_tape(n, np.random.default_rng(70 + n), 20).without_wide_channels() if n == 3 \
        else G.step_tape("CRX", (0, 1), "amp", 2)
    ot = NR.reference_tape(tape)
    for L in (DR.cost_matrix(n, [0.7, -1.2, 0.4], groups=G.z_groups(n)),
              DR.cost_matrix(n, [0.3, -0.8, 0.5, 1.1], terms=G.pauli_terms(n))):
        g = DR.shift_gradient(ot, n, L)
        assert np.abs(g).max() > 1e-2
        assert np.abs(g - DR.central_difference(ot, n, L)).max() <= 1e-7
        assert np.abs(g - DR.adjoint_gradient(ot, n, L)).max() <= 1e-12  # the rule of the sweep, on dense matrices
        # the plain form of the rule, every shifted circuit run to its end: the same numbers, the same complex64 floor
        assert np.abs(g - DR.shift_jacobian_forward(ot, n, [L])[0]).max() <= 1e-12
        f32 = np.abs(DR.shift_jacobian(ot, n, [L], dtype=np.complex64)[0] - g).max()
        p32 = np.abs(DR.shift_jacobian_forward(ot, n, [L], dtype=np.complex64)[0] - g).max()
        assert 1e-9 < f32 < 1e-6 and 1e-9 < p32 < 1e-6


def _gpu_cases():
    """(name, tape, wanted angles, seed of the weights, rows of them): the weights each GPU test draws"""
    for case in G.STEP_CASES:
        tape = G.step_tape(*case)
        yield "step " + str(case), tape, tuple(range(G.n_slots(tape))), 11, G.B
    for n in (5, 7, 8):
        tape = G.random_tape(n)
        yield f"random {n}", tape, G.wanted_of(tape, G.WANTED[n]), 12 + n, G.B
    tape = G.random_tape(5)
    yield "stacked", tape, G.wanted_of(tape, 12), 21, 2 * G.B
    yield "subset", tape, G.wanted_of(tape, 12)[1::3], 22, G.B
    tape = G.model_noisy_tape()
    yield "model", tape, G.wanted_of(tape, 10), 23, G.B


@pytest.mark.parametrize("name,tape,wanted,wseed,rows", list(_gpu_cases()), ids=lambda v: v if isinstance(v, str) else None)
def test_every_gpu_case_tells_the_wrong_variants_apart(name, tape, wanted, wseed, rows):
    """by at least 100 x the tolerance the case is held to (the routes figure; the 4 x floor figure is smaller on every
    tape here, which the GPU test prints), for both seeds and every row of weights the GPU test uses: the gradient is
    linear in the weights, so the variants' Jacobians per observable serve all rows"""
    n = tape.n
    ot = NR.reference_tape(tape, 0)
    need = 100 * G.routes_tolerance(2 * n, False)
    for seed in (("z",) if name == "subset" else ("z", "pauli")):
        Ls = G.observables(n, seed)[2]
        jac = {v: j[:, list(wanted)] for v, j in DR.adjoint_jacobians(ot, n, Ls, (None,) + DR.VARIANTS).items()}
        for w in G.weights(len(Ls), rows, wseed):
            for variant in DR.VARIANTS:
                moved = DR.metric(w @ jac[variant], w @ jac[None], w)
                assert moved >= need, (name, seed, variant, moved, need)


# ---- the plan ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_plan():
    from qml_essentials_amd.model import Model

    model = Model(n_qubits=3, n_layers=2, circuit_type="Circuit_19", output_qubit=-1)
    rng = np.random.default_rng(5)
    tape = NR.model_tape("Circuit_19", 3, 2, NR.NOISE, rng.uniform(0, 2 * np.pi, size=model.params.shape[1:]),
                         rng.uniform(0, 2 * np.pi, size=(1,)), model=model)
    return tape, adjoint.plan_density(tape.ops, 3, [True] * G.n_slots(tape))


def test_plan_has_one_step_per_parametrised_gate_and_five_transfers_each(model_plan):
    tape, sw = model_plan
    assert len(sw.steps) == G.n_slots(tape) == sw.n_slots > 0
    assert sorted(s[8][0] for s in sw.steps) == list(range(sw.n_slots))  # every source slot is reported once
    assert adjoint.STEP_TRANSFERS_FWD + adjoint.STEP_TRANSFERS_BWD == 5
    free = 2 + adjoint.FREE_TRANSFERS * (sw.n_free_fwd + sw.n_free_bwd)  # checkpoint 0, the seed, the term-free runs
    assert sw.transfers(1) == free + 5 * len(sw.steps)
    # every op of the doubled tape is in exactly one step or outside all of them
    covered = sorted(k for s in sw.steps for k in range(s[4], s[4] + s[5]))
    assert len(covered) == len(set(covered)) and len(sw.fwd.ops) == len(covered) + sw.n_free_fwd
    # leaving an angle out turns its step into term-free operators
    fewer = adjoint.plan_density(tape.ops, 3, [k != 0 for k in range(sw.n_slots)])
    assert len(fewer.steps) == len(sw.steps) - 1


def test_checkpoints_are_counted_once_per_sample(model_plan):
    _tape, sw = model_plan
    state = 8 << 6
    assert sw.checkpoints == len(sw.steps) + 1
    assert sw.sample_bytes(1) == (sw.checkpoints + 1) * state
    assert sw.sample_bytes(3) == (sw.checkpoints + 3) * state  # K = 3: two more rows of lambda, no more checkpoints
    assert sw.sample_bytes(3, x64=True) == 2 * sw.sample_bytes(3)
    assert sw.transfers(3) - sw.transfers(1) == 2 * (sw.transfers(2) - sw.transfers(1))  # forward once, backward K times


def test_rounds(model_plan):
    _tape, sw = model_plan
    need = sw.sample_bytes(3)
    assert adjoint.density_rounds(5, need, 2 * need) == [2, 2, 1]
    assert adjoint.density_rounds(5, need, 100 * need) == [5]
    assert adjoint.density_rounds(5, need, 100 * need, max_samples=3) == [3, 2]
    with pytest.raises(adjoint.AdjointUnsupported, match=str(need)):
        adjoint.density_rounds(5, need, need - 1)
    # the need of a call as the library states it (host only): checkpoints, lambda, matrix rows, partial sums, tables
    fwd, rev = _plans(sw)
    call = lambda bc: adjoint.density_call_bytes(sw, fwd, rev, bc, 3, 3)  # noqa: E731
    assert call(1) > sw.sample_bytes(3) and call(2) - call(1) >= sw.sample_bytes(3)
    assert adjoint.density_rounds(5, call, call(2)) == [2, 2, 1]
    assert adjoint.density_rounds(5, call, call(3) - 1) == [2, 2, 1]
    assert adjoint.density_rounds(5, call, call(5)) == [5]
    with pytest.raises(adjoint.AdjointUnsupported, match=str(call(1))):
        adjoint.density_rounds(5, call, call(1) - 1)


def test_refusals_name_the_operation():
    from qml_essentials_amd.unitary import UnitaryGates

    with NR.recording_depolarizing() as (ops, _d):
        op.RX(0.3, wires=0)
        UnitaryGates.NQubitDepolarizingChannel(0.1, [0, 1, 2])
    with pytest.raises(adjoint.AdjointUnsupported, match="3 wires"):
        adjoint.plan_density(ops, 3, [True])


def _plans(sw):
    mk = lambda low: N.Plan(low.ops, low.n_qubits, low.n_slots, low.consts if len(low.consts) else None,  # noqa: E731
                            adjoint.DENSITY_FLAGS)
    return mk(sw.fwd), mk(sw.rev)


def test_library_counts_the_transfers_of_the_plan(model_plan):
    _tape, sw = model_plan
    fwd, rev = _plans(sw)
    for k in (1, 3):
        assert N.adjoint_density_transfers(fwd, rev, list(sw.steps), n_cot=k) == sw.transfers(k)
    tape = G.random_tape(5)
    sw5 = adjoint.plan_density(tape.ops, 5, [k % 2 == 0 for k in range(G.n_slots(tape))])
    assert N.adjoint_density_transfers(*_plans(sw5), list(sw5.steps), n_cot=2, f64=True) == sw5.transfers(2)


# ---- argument checks, all before device work (no GPU here) -----------------------------------------------------------
def _call(sw, fwd, rev, masks, terms, n_terms, ws_bytes=None, batch=2):
    lib = N.lib()
    fake = C.c_void_p(1 << 20)  # device pointers that a refused call never reads
    need = lib.qmle_adjoint_density_workspace_bytes(fwd._h, rev._h, batch, 1, len(sw.steps))
    return need, lib.qmle_adjoint_density(
        fwd._h, rev._h, fake, fake, batch, 1, fake, masks, terms, n_terms, 2, N.density_step_array(list(sw.steps)),
        len(sw.steps), fake, int(sw.chan.size), fake, max(1, sw.n_slots), fake,
        C.c_size_t(need if ws_bytes is None else ws_bytes), None)


def test_bad_arguments_come_back_with_their_codes(model_plan):
    _tape, sw = model_plan
    fwd, rev = _plans(sw)
    masks = (C.c_uint32 * 2)(1, 2)
    terms = N.pauli_term_array([(1.0, 1, 0, 0), (1.0, 2, 2, 1)])
    assert _call(sw, fwd, rev, None, None, 0)[1] == -1            # both seeds NULL
    assert _call(sw, fwd, rev, masks, terms, 2)[1] == -1          # both seeds set
    need, _ = _call(sw, fwd, rev, None, None, 0)
    assert need > (sw.checkpoints + 1) * 2 * (8 << 6)
    assert _call(sw, fwd, rev, masks, None, 0, ws_bytes=need - 512)[1] == -7   # QMLE_ERR_WORKSPACE
    bad = (C.c_uint32 * 2)(1, 1 << 3)                             # a Z on a wire the system does not have
    assert _call(sw, fwd, rev, bad, None, 0)[1] == -4
    # 2n < 4: one system wire
    with NR.recording_depolarizing() as (ops, _d):
        op.RX(0.3, wires=0)
        op.BitFlip(0.1, wires=0)
    one = adjoint.plan_density(ops, 1, [True])
    f1, r1 = _plans(one)
    assert N.lib().qmle_adjoint_density_workspace_bytes(f1._h, r1._h, 2, 1, 1) > 0
    assert _call(one, f1, r1, (C.c_uint32 * 2)(1, 1), None, 0)[1] == -1
