"""Matrix cotangents from every route of the adjoint sweep against the exact reference of
tests/matrix_cotangent_reference.py.

Each test goes through ``adjoint.adjoint_slot_and_matrix_gradient`` -- the function ``Script.vjp`` ends in when a tape
holds pulse leaves -- forces one route with the idioms of tests/test_gpu_adjoint_routes.py and proves it from
``describe()`` as that file does:

* LDS (``k_adjoint_lds``): ``whole_state_lds``, one stage, n <= 13, no 4-wire operator; for the slots-in-global
  variant more than 658 forward operators.
* streaming complex64 (``k_adj_moment`` / ``k_adj_cot_final``): ``adjoint.REV_FLAGS_FUSED = REV_FLAGS``; at n = 5 a
  ``Dense4`` on the tape keeps the sweep out of LDS; at n = 14 the matrix gates sit on wires 0, 7 and 13 -- bit
  positions 13, 6 and 0, the last one inside a float4.
* fused refusal: with ``adjoint.REV_FLAGS = REV_FLAGS_FUSED`` both attempts of ``run_sweep`` compile the fused plan
  and the request raises ``N.Unsupported``; unforced, ``run_sweep`` returns the streaming result.
* complex128 (``k64_adj_moment`` / ``k_adj_cot_final<double2, double>``): ``x64_scope(True)``.

Every entry of every ``G`` and every angle column of the same sweep is compared, row by row, under both seeds.
Tolerances are ``tests/test_gpu_adjoint_routes.tolerance(n, x64)`` times ``max(1, sum_k |w_k|)`` of the row: 4e-6 up to
13 qubits, 1e-5 at 14, 1e-12 in complex128 (each entry of ``G`` is bounded by ``|lambda| |psi| <= sum |w|``, the scale
those figures were set for).

Largest errors measured on the MI355X, as fractions of ``max(1, sum |w|)`` (``G`` / angle columns of the same sweep):
2.2e-7 / 3.0e-7 in the LDS kernel (1.4e-7 / 4.6e-8 with the operator slots in global memory), 6.8e-8 / 1.0e-7 streaming
at n = 5, 5.1e-8 / 7.9e-8 streaming at n = 14, 6.7e-16 / 6.2e-16 in complex128 (profiles/pulse_gradient.md).
"""
import numpy as np
import pytest

from qml_essentials_amd import _native as N
from qml_essentials_amd import adjoint
from qml_essentials_amd.simulation import get_plan
from qml_essentials_amd.utils import x64_scope
from tests import matrix_cotangent_reference as M
from tests.test_gpu_adjoint_routes import assert_lds, force, script_of, tolerance

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEEDS = ["z", "pauli"]


@pytest.fixture(autouse=True)
def fresh_reverse_tapes():
    adjoint._REV_CACHE.clear()
    yield
    adjoint._REV_CACHE.clear()


def lowered(case):
    """-> (lowered tape, slot of every angle of the spec, matrix-cotangent flag per lowered op)"""
    s = script_of(case.spec, case.n)
    _tape, low, n, B, _slots, _shapes, _batched = s._trace_for_gradient([], (case.theta,), None, (0,), (0,))
    assert n == case.n and B == case.theta.shape[0] and len(low.ops) == len(case.spec)
    slot_of, at = {}, 0
    for (name, _w, slots, _off), (sname, _sw, idx, const) in zip(low.ops, case.spec):
        if name == "MAT1_ROW":
            assert sname == "Matrix" and np.asarray(const).ndim == 3 and len(slots) == 8
        else:
            assert len(slots) == len(idx), (name, sname)
            for s_, k in zip(slots, idx):
                slot_of[k] = s_
        at += len(slots)
    assert at == low.n_slots and len(slot_of) == case.spec.n_theta
    for k in (0, case.spec.n_theta - 1):
        assert np.array_equal(np.broadcast_to(low.values[slot_of[k]], (B,)), case.theta[:, k])
    want_mat = [i in case.mats for i in range(len(low.ops))]
    kinds = {low.ops[i][0] for i in case.mats}
    assert kinds == {"MAT1", "MAT1_ROW"}  # constant and per-sample matrices on one tape
    return low, slot_of, want_mat


def pauli_terms_of(case):
    from qml_essentials_amd import simulation
    from tests.test_gpu_adjoint_pauli import observables

    mats = M.case_observables(case)[1]
    obs = observables(case.n, np.random.default_rng([case.seed, case.n, 78]))
    for o, (m, wires) in zip(obs, mats):
        assert list(o.wires) == list(wires) and np.array_equal(np.asarray(o.matrix), m)
    terms = simulation.pauli_term_list(obs, case.n)
    assert terms is not None and len(obs) == len(mats)
    return terms


def sweep(case, low, slot_of, want_mat, seed, x64=False):
    groups, _mats, wz, wp = M.case_observables(case)
    want = [False] * low.n_slots
    for k in case.wanted:
        want[slot_of[k]] = True
    w = wz if seed == "z" else wp
    B = w.shape[0]
    with x64_scope(x64):
        if seed == "z":
            return adjoint.adjoint_slot_and_matrix_gradient(low, case.n, B, groups, w, want, want_mat, x64=x64)
        return adjoint.adjoint_slot_and_matrix_gradient(low, case.n, B, None, w, want, want_mat, x64=x64,
                                                        obs_terms=pauli_terms_of(case))


def compare(case, slot_of, got, seed, x64=False):
    """every entry of every G and every angle column, row by row; columns that were not asked for are exactly zero"""
    grad, cot = got
    ref_grad, ref_cot = M.case_reference(case.name, seed)
    _g, _m, wz, wp = M.case_observables(case)
    w = wz if seed == "z" else wp
    tol = tolerance(case.n, x64)
    assert cot.shape == ref_cot.shape and cot.dtype == (np.complex128 if x64 else np.complex64)
    cols = [slot_of[k] for k in case.wanted]
    rest = sorted(set(range(grad.shape[1])) - set(cols))
    assert not grad[:, rest].any()
    worst_g = worst_a = 0.0
    for b in range(ref_cot.shape[0]):
        scale = max(1.0, np.abs(w[b]).sum())
        err_g = np.abs(cot[b] - ref_cot[b]).max() / scale
        err_a = np.abs(grad[b, cols] - ref_grad[b, case.wanted]).max() / scale
        worst_g, worst_a = max(worst_g, err_g), max(worst_a, err_a)
    print(case.name, seed, "x64" if x64 else "c64", "max |G - G_ref| / max(1, sum|w|)", worst_g,
          "max |angle gradient - reference| / max(1, sum|w|)", worst_a, "tolerance", tol)
    for b in range(ref_cot.shape[0]):
        scale = max(1.0, np.abs(w[b]).sum())
        assert np.abs(cot[b] - ref_cot[b]).max() / scale <= tol, (case.name, seed, "row", b, "G")
        assert np.abs(grad[b, cols] - ref_grad[b, case.wanted]).max() / scale <= tol, (case.name, seed, "row", b)
    return worst_g, worst_a


# ---- the LDS kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [2, 3, 13])
def test_lds_sweep_matrix_cotangents(n, B, seed):
    """fewer amplitudes than threads (n = 2), the gate on each wire (n = 3), several strided iterations at the
    largest LDS state (n = 13)"""
    case = M.cases()[f"lds_n{n}_b{B}"]
    low, slot_of, want_mat = lowered(case)
    assert_lds(low, n)
    compare(case, slot_of, sweep(case, low, slot_of, want_mat, seed), seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_lds_sweep_matrix_cotangents_operator_slots_in_global_memory(seed):
    """slots_in_lds = 0: more than 658 forward operators beside psi and lambda at 13 qubits"""
    case = M.cases()["lds_deep_n13"]
    low, slot_of, want_mat = lowered(case)
    assert_lds(low, 13, more_ops_than=658)
    compare(case, slot_of, sweep(case, low, slot_of, want_mat, seed), seed)


# ---- the streaming kernels -----------------------------------------------------------------------------------------
def reverse_plan_stages(flags):
    """(kind, lowered operators) of every stage of the reverse plan the last sweep ran"""
    (rev, _terms, _tab), = list(adjoint._REV_CACHE.values())[-1:]
    return [(st["kind"], st["n_lowered"]) for st in get_plan(rev, flags).describe()["stages"]]


@pytest.mark.parametrize("seed", SEEDS)
def test_streaming_sweep_matrix_cotangents_below_14_qubits(seed, monkeypatch):
    """a 4-wire operator on the tape: k_adj_moment on 16 float4 per state, gates on positions 4, 0, 2, 0"""
    case = M.cases()["stream_n5"]
    low, slot_of, want_mat = lowered(case)
    assert "MAT4" in [o[0] for o in low.ops] and get_plan(low).describe()["whole_state_lds"]
    force(monkeypatch, "streaming")
    compare(case, slot_of, sweep(case, low, slot_of, want_mat, seed), seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_streaming_sweep_matrix_cotangents_at_14_qubits(seed, monkeypatch):
    """matrix gates on wires 0, 7, 13, 7: positions 13 and 6 across two float4, position 0 inside one"""
    case = M.cases()["stream_n14"]
    assert [case.spec[g][1] for g in case.mats] == [[0], [7], [13], [7]]
    low, slot_of, want_mat = lowered(case)
    force(monkeypatch, "streaming")
    got = sweep(case, low, slot_of, want_mat, seed)
    stages = reverse_plan_stages(adjoint.REV_FLAGS)  # one streaming pass per gate: no stage holds two operators
    assert len(stages) == len(case.spec) and {k for _kind, k in stages} == {1}, stages
    compare(case, slot_of, got, seed)


def test_fused_tile_route_refuses_a_cotangent_request(monkeypatch):
    """k_tile_adj takes generator overlaps only: forced, the request raises; through run_sweep's own fallback the
    same request returns the streaming result"""
    case = M.cases()["stream_n14"]
    low, slot_of, want_mat = lowered(case)
    force(monkeypatch, "fused")
    with pytest.raises(N.Unsupported):
        sweep(case, low, slot_of, want_mat, "z")
    monkeypatch.undo()
    adjoint._REV_CACHE.clear()
    compare(case, slot_of, sweep(case, low, slot_of, want_mat, "z"), "z")


# ---- complex128 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", ["lds_n2_b3", "lds_n3_b3", "stream_n14"])
def test_complex128_sweep_matrix_cotangents(name, seed):
    case = M.cases()[name]
    low, slot_of, want_mat = lowered(case)
    compare(case, slot_of, sweep(case, low, slot_of, want_mat, seed, x64=True), seed, x64=True)


def test_a_request_on_anything_but_a_one_wire_matrix_is_unsupported():
    """mat_out >= 0 on a rotation: QMLE_ERR_UNSUPPORTED from the library itself"""
    case = M.cases()["lds_n3_b1"]
    low, slot_of, want_mat = lowered(case)
    sweep(case, low, slot_of, want_mat, "z")
    (rev, terms, tab), = list(adjoint._REV_CACHE.values())[-1:]
    bad = [0 if name == "RX" else -1 for name, _w, _s, _o in rev.ops]
    assert 0 in bad
    groups, _mats, wz, _wp = M.case_observables(case)
    a_f = torch.from_numpy(low.angle_table(1)).cuda()
    a_r = (a_f.index_select(1, tab.perm) * tab.sign.float()).contiguous()
    w = torch.from_numpy(wz.astype(np.float32)).cuda()
    with pytest.raises(N.Unsupported):
        N.adjoint_cotangent(get_plan(low), get_plan(rev, adjoint.REV_FLAGS), a_f, a_r, w, groups, terms,
                            low.n_slots, bad, 1)
