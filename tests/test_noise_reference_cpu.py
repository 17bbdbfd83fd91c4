"""The reference side of tests/test_gpu_noise_routes.py, and the routes those tests name, without a GPU.

* ``noise_reference.simulate_mixed_fast`` -- the oracle's ``simulate_mixed`` with the n-qubit depolarizing channel in
  closed form -- equals the oracle's Kraus sum.
* The metric of the GPU comparisons, ``rel_err <= 16 * c64_floor``, sees a wrong tape: for every tape the GPU tests run,
  a dropped one-wire channel, a two-wire channel with its wires exchanged and a bra side without its conjugation move
  rho by more than 100 times that tolerance.  This is a condition on the tapes.  The dropped channel is an
  AmplitudeDamping; dropping one of the weakest channels of the noisy model instead -- BitFlip(0.01), PhaseFlip(0.015),
  DepolarizingChannel(0.02) behind one gate -- moves rho by 7e-4 .. 3e-3, which is 60 to 250 times the tolerance of
  these tapes (their 300 to 450 operations put the reference's complex64 error at 4e-7 .. 8e-7).  The model's only
  two-wire channel is the depolarizing one, which is the same channel with its wires exchanged: the exchange is
  asserted on the tapes that hold ``noise_reference.pair_channel``.
* The plans of the doubled tapes take the routes the GPU tests are there for, read from ``Plan.describe()`` and
  ``Plan.tile_route``: a retune cannot silently move the tests off them."""
import numpy as np
import pytest

from oracle import noise as ON
from qml_essentials_amd import _native as N

import noise_reference as R
from helpers import frontend_to_oracle

GK_REG4, GK_DENSE4, GK_REG4X = 1, 2, 3  # group kinds of describe() (csrc/qmle_internal.h)
MARGIN = 100 * 16


# ---- closed form == Kraus sum ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 7])
@pytest.mark.parametrize("make", ["spread", "random"])
def test_closed_form_equals_the_kraus_sum(make, n):
    """spread_tape: k = 2 in both wire orders, k = 3 and k = 4 in mixed order; the oracle gets the front end's Kraus
    matrices (16, 64, 256 of them)."""
    rng = np.random.default_rng(40 + n)
    tape = R.spread_tape(n, rng) if make == "spread" else R.random_noisy_tape(n, rng, 30)
    assert tape.depol and all(type(o).__name__ == "QubitChannel" for o in tape.ops if id(o) in tape.depol)
    ref = R.reference_tape(tape)
    assert sum(name == "NQubitDepolarizing" for name, _, _ in ref) == len(tape.depol)
    got = R.simulate_mixed_fast(ref, n)
    want = ON.simulate_mixed(frontend_to_oracle(tape.ops), n)
    assert np.abs(got - want).max() < 1e-14
    assert abs(np.trace(got) - 1) < 1e-13


@pytest.mark.parametrize("wires", [[0, 1], [3, 1], [0, 2, 3], [4, 2, 0], [1, 4, 0], [0, 1, 3, 4], [4, 3, 1, 0],
                                   [2, 0, 4, 1]])
def test_closed_form_on_every_width_and_wire_order(wires):
    from qml_essentials_amd.unitary import UnitaryGates

    n, p = 5, 0.37
    head = R.reference_tape(R.random_noisy_tape(n, np.random.default_rng(len(wires) + wires[0]), 20))
    kraus = UnitaryGates.NQubitDepolarizingChannel(p, wires).kraus_matrices()
    got = R.simulate_mixed_fast(head + [("NQubitDepolarizing", wires, (p, len(wires)))], n)
    want = ON.simulate_mixed(head + [("QubitChannel", wires, (kraus,))], n)
    assert np.abs(got - want).max() < 1e-14
    assert np.abs(got - R.simulate_mixed_fast(head, n)).max() > 1e-3


def test_the_model_tape_carries_its_depolarizing_channels():
    ansatz, n, layers = R.MODEL_CASES[0]
    tape = R.model_sample_tape(ansatz, n, layers)
    two_wire = [o for o in tape.ops if type(o).__name__ == "QubitChannel"]
    assert two_wire and all(tape.depol[id(o)] == R.NOISE["MultiQubitDepolarizing"] for o in two_wire)
    bare = R.model_sample_tape(ansatz, n, layers, False)
    assert len(bare.ops) == len(tape.ops) - n, "StatePreparation is one BitFlip per wire"
    got = R.simulate_mixed_fast(R.reference_tape(tape), n)
    assert np.abs(got - ON.simulate_mixed(frontend_to_oracle(tape.ops), n)).max() < 1e-14


# ---- the metric discriminates ----------------------------------------------------------------------------------
def _route_tapes():
    out = [("-".join(map(str, c)), c, None) for c in R.ENGINE_CASES + [R.RAGGED_CASE] + R.WIDE_CASES]
    out += [("-".join(map(str, m)), None, m + (True,)) for m in R.MODEL_CASES]
    out.append(("-".join(map(str, R.NO_STATE_PREP)) + "-bare", None, R.NO_STATE_PREP + (False,)))
    return out


def _tape_of(case, model):
    return R.route_tape(*case) if case else R.model_sample_tape(*model)


@pytest.mark.parametrize("label,case,model", _route_tapes(), ids=[t[0] for t in _route_tapes()])
def test_the_metric_sees_a_wrong_tape(label, case, model):
    tape = _tape_of(case, model)
    n, ref = tape.n, R.reference_tape(tape)
    want, floor = R.reference_rho(tape), R.tape_floor(tape)
    assert 2e-8 < floor < 1e-6, floor  # a complex64 rounding per operation
    moved = {"dropped channel": R.rel_err(R.simulate_mixed_fast(R.drop_one_wire_channel(ref), n), want)}
    swapped = R.swap_two_wire_channel(ref)
    if model is None:
        moved["exchanged wires"] = R.rel_err(R.simulate_mixed_fast(swapped, n), want)
    else:
        assert swapped is None and tape.depol, "the model's two-wire channels are depolarizing channels"
    if case is None or case[0] != "spread_wide":  # (its gates are those of the "spread" tape of the same n)
        moved["no conjugation"] = R.rel_err(R.rho_without_bra_conjugation(tape), want)
    print(label, f"floor {floor:.2e} tolerance {16 * floor:.2e}", {k: f"{v:.2e}" for k, v in moved.items()})
    for what, err in moved.items():
        assert err > MARGIN * floor, (label, what, err, MARGIN * floor)


# ---- routes -----------------------------------------------------------------------------------------------------
def _stages(tape, flags=0):
    _low, plan = R.lowered(tape.without_wide_channels(), flags)
    return plan, plan.describe()


def _kinds(stage):
    return {g["kind"] for g in stage["groups"]}


@pytest.mark.parametrize("label,case,model", _route_tapes(), ids=[t[0] for t in _route_tapes()])
def test_default_plans_take_the_routes_the_gpu_tests_name(label, case, model):
    tape = _tape_of(case, model)
    n = tape.n
    plan, desc = _stages(tape)
    stages = desc["stages"]
    assert desc["n_qubits"] == 2 * n and all(s["kind"] == "tile" and not s["fast"] for s in stages)
    for si in range(len(stages)):  # the 16 x 16 instantiation of k_tile, every stage
        r = plan.tile_route(si, 3, N.Plan.TM_STORE, 0, N.Plan.ROUTE_INIT_ZERO if si == 0 else 0)
        assert r["status"] == 0 and r["family"] == "k_tile" and r["dense4"], (label, si, r)
    if n <= 7:
        assert desc["whole_state_lds"] and len(stages) == 1 and stages[0]["T"] == 2 * n
        assert {GK_DENSE4, GK_REG4X} <= _kinds(stages[0])
        if n == 7:
            assert plan.tile_route(0, 3, N.Plan.TM_STORE, 0, N.Plan.ROUTE_INIT_ZERO)["lds_bytes"] >= 128 * 1024
    else:
        assert not desc["whole_state_lds"] and len(stages) >= 2
        assert all(s["T"] in (12, 13) for s in stages)
        later = stages[1:]  # they load their tiles
        assert any(GK_DENSE4 in _kinds(s) for s in later) and any(GK_REG4X in _kinds(s) for s in later), label
        assert any(s["bits"] != list(range(s["T"])) for s in later), "tiles over arbitrary bit sets"


@pytest.mark.parametrize("n,lo,hi", [(8, 5, 9), (9, 2, 13)])
def test_the_noisy_model_takes_several_tile_stages(n, lo, hi):
    """The benchmarked model (Hardware_Efficient, 3 layers at n = 8), its neighbours, and the same at n = 9."""
    seen = set()
    for ansatz, layers in (("Hardware_Efficient", 3), ("Circuit_19", 1), ("Strongly_Entangling", 1)):
        model, params, inputs, noise = R.model_case(ansatz, n, layers)
        tape = R.model_tape(ansatz, n, layers, noise, params[0], inputs[0], model=model)
        _plan, desc = _stages(tape)
        seen.add(len(desc["stages"]))
        assert not desc["whole_state_lds"] and all(s["T"] in (12, 13) and not s["fast"] for s in desc["stages"])
    assert lo <= min(seen) and max(seen) <= hi, seen


def test_known_zeros_reach_a_loading_stage_and_no_sparse_ignores_them():
    """Without StatePreparation -- and with it -- the second stage of the n = 8 model loads tiles with known-zero bits
    (describe() reports Stage::zero_in whatever the flags); PLAN_NO_SPARSE makes the launches ignore them: the first
    pass then runs every tile instead of the one that can be non-zero."""
    P = N.Plan
    for state_prep in (False, True):
        tape = R.model_sample_tape(*R.NO_STATE_PREP, state_prep)
        plan, desc = _stages(tape)
        assert any(s["zero_in"] != 0 for s in desc["stages"][1:])
        first = plan.tile_route(0, 6, P.TM_STORE, 0, P.ROUTE_FROM_ZERO | P.ROUTE_INIT_ZERO)
        assert first["compact"] and first["grid"] == [1, 6]
        plan, desc = _stages(tape, N.PLAN_NO_SPARSE)
        tiles = [1 << (desc["n_qubits"] - s["T"]) for s in desc["stages"]]
        for si, t in enumerate(tiles):
            r = plan.tile_route(si, 6, P.TM_STORE, 0, P.ROUTE_FROM_ZERO | (P.ROUTE_INIT_ZERO if si == 0 else 0))
            assert r["status"] == 0 and not r["compact"] and r["grid"] == [t, 6], (si, r)


@pytest.mark.parametrize("case", R.ENGINE_CASES, ids=["-".join(map(str, c)) for c in R.ENGINE_CASES])
def test_forced_geometries_are_what_they_say(case):
    tape = R.route_tape(*case)
    n2 = 2 * tape.n
    for tile_bits, low_bits in ((10, 4), (10, 7)):
        _plan, desc = _stages(tape, N.plan_flags(force_global=True, force_tile=True, tile_bits=tile_bits,
                                                 low_bits=low_bits))
        tiled = [s for s in desc["stages"] if s["kind"] == "tile"]
        assert tiled and all(s["T"] <= min(tile_bits, n2) for s in tiled), [(s["kind"], s.get("T")) for s in desc["stages"]]
        if n2 > tile_bits:
            assert not desc["whole_state_lds"] and len(tiled) >= 2
    _plan, desc = _stages(tape, N.plan_flags(tile_bits=11))
    if n2 > 14:
        assert all(s["T"] <= 11 for s in desc["stages"] if s["kind"] == "tile") and len(desc["stages"]) >= 2
