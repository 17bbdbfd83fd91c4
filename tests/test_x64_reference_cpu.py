"""No GPU: the reference of tests/test_gpu_x64_routes.py (tests/x64_reference.py) against the oracle, the resolving
power of every case that module runs, and the plan shapes its merge cases are named after.

Discrimination is a condition on the inputs, not a measurement of the engine: for every case and every wrong variant
of the reference that changes what the case computes (``x64_reference.applies``: decided from the gates' symmetries),
the compared quantity moves by at least 1e-6 in the norm the GPU test asserts (max |difference| over every row) --
10^6 times the 1e-12 bar.  One exception, reasoned and not measured (``x64_reference.see_bar``): constants rounded
to float32 move an amplitude by 3e-8 (matrices) to 2e-6 (marks) of itself, whatever the inputs; that variant's
condition is 1e-9, the figure the constants test asks of the same difference on the GPU."""
import numpy as np
import pytest

from oracle import einsum_sim as OE
from tests.helpers import random_tape

import x64_reference as R


@pytest.mark.parametrize("n", range(1, 9))
def test_apply_tape_equals_the_oracle_from_the_zero_state(n):
    rng = np.random.default_rng(6400 + n)
    tape = random_tape(n, 40 if n > 1 else 10, rng)
    want = OE.simulate_pure(tape, n, np.complex128)
    got = R.apply_tape(R.zero_states(2, n), tape, n)
    assert got.dtype == np.complex128 and np.abs(got - want[None, :]).max() < 1e-14


def test_apply_tape_explicit_matrices_golomb_diagonal_and_per_row_angles():
    """What the oracle's simulate_pure cannot start from or does not take: a given start state, 1-, 2- and 4-wire
    matrices in any wire order, the diagonal over the whole register, one angle per row -- against dense matrices."""
    from oracle.dense import lift

    n, rng = 5, np.random.default_rng(3)
    psi0 = R.haar_states(rng, 2, n)
    U1, U2, U4 = (R.random_unitary(rng, d) for d in (2, 4, 16))
    marks, x, th = R.random_marks(rng, n), np.array([0.3, 1.9]), np.array([0.7, 2.2])
    tape = [("Matrix", [3], (U1,)), ("CRX", [4, 1], (th,)), ("Matrix", [4, 0], (U2,)), ("DiagAll", [], (x, marks)),
            ("Matrix", [2, 4, 0, 3], (U4,))]
    got = R.apply_tape(psi0, tape, n)
    from oracle import gates as G
    for b in range(2):
        want = lift(U1, [3], n) @ psi0[b]
        want = lift(G.matrix("CRX", (th[b],)), [4, 1], n) @ want
        want = lift(U2, [4, 0], n) @ want
        want = np.exp(-1j * marks * x[b]) * want
        want = lift(U4, [2, 4, 0, 3], n) @ want
        assert np.abs(got[b] - want).max() < 1e-14


# ---- discrimination ----------------------------------------------------------------------------------------
def _discriminates(case):
    """Assert the condition for one case; -> the variants that applied."""
    base, applied = R.compared(case), set()
    for wrong in R.WRONG:
        moved = None
        for q, want in base.items():
            if not R.applies(case, wrong, q):
                continue
            if moved is None:
                moved = R.compared(case, wrong)
            d = float(np.abs(moved[q] - want).max())
            assert d >= R.see_bar(case, wrong), (case.label, wrong, q, d)
            applied.add(wrong)
    return applied


_APPLY_AT_5 = {
    "RY": {"transpose", "bit_order", "angles_prev"},
    "MAT1": {"transpose", "conjugate", "bit_order", "consts_f32"},
    "CRX": {"control_target", "conjugate", "bit_order", "angles_prev"},
    "CPhase": {"conjugate", "bit_order", "angles_prev"},
    "CCX": {"control_target", "bit_order"},
    "RZX": {"targets", "conjugate", "bit_order", "angles_prev"},
    "MAT2": {"targets", "transpose", "conjugate", "bit_order", "consts_f32"},
    "CSWAP": {"control_target", "bit_order"},
    "MAT4": {"transpose", "conjugate", "bit_order", "mat4_order", "consts_f32"},
    "DIAG_ALL": {"conjugate", "angles_prev", "golomb_sign", "golomb_bitrev", "consts_f32"},
}


@pytest.mark.parametrize("n,kind", R.RESIDENT, ids=[f"{k}-{n}" for n, k in R.RESIDENT])
def test_every_resident_case_sees_every_wrong_variant(n, kind):
    applied = set()
    for case in R.resident_cases(n, kind):
        applied |= _discriminates(case)
    if n == 5:  # (and the table of which mistakes a kind can make at all is what this module says it is)
        assert applied == _APPLY_AT_5[kind], (kind, applied)
    assert applied


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_lds_kind_case_sees_every_wrong_variant(kind):
    for case in R.lds_kind_cases(10, kind):
        assert _discriminates(case) >= _APPLY_AT_5[kind] - {"bit_order"}, case.label


@pytest.mark.parametrize("n", [10, 14])
@pytest.mark.parametrize("merge", R.MERGES)
def test_every_merge_case_sees_every_wrong_variant(merge, n):
    for case in R.merge_cases(n, merge):
        applied = _discriminates(case)
        assert {"control_target", "transpose", "conjugate", "bit_order", "angles_prev"} <= applied, case.label
        if merge not in ("1q_onto_1q", "1q_onto_RXX"):
            assert "targets" in applied, case.label


def test_constants_rows_measurement_and_schedule_cases_see_every_wrong_variant():
    for n, resident in R.CONSTANTS:
        applied = _discriminates(R.constants_case(n, resident))
        assert {"transpose", "conjugate", "bit_order", "mat4_order", "golomb_sign", "golomb_bitrev", "consts_f32",
                "targets", "control_target", "angles_prev"} <= applied
    for n, B, resident in R.ROWS:
        applied = _discriminates(R.rows_case(n, B, resident))
        assert ("angles_prev" in applied) == (B > 1) and ("angles_mod64" in applied) == (B > 64), (n, B, applied)
    for n, B in [(n, R.BATCH) for n in R.MEASURE_N] + list(R.DENSITY):
        applied = _discriminates(R.measure_case(n, B))
        assert {"bit_order", "golomb_sign", "conjugate"} <= applied or n == 1, (n, B, applied)
    for n in (9, 14):
        case = R.observables_case(n)
        assert len(case.groups) == 32 and len(set(case.groups)) == 32
        assert "bit_order" in _discriminates(case)
    assert "angles_prev" in _discriminates(R.schedule_case())


def test_two_round_case_sees_every_wrong_variant_and_the_second_round():
    """(h): row 16384 is the first of the second round; evaluated with the rows of the first it is row 0.  The batch
    cycles through three angle rows and 16384 % 3 = 1, so the two differ."""
    case = R.two_round_case()
    applied = _discriminates(case)
    assert {"control_target", "targets", "conjugate", "bit_order", "angles_prev", "golomb_sign", "golomb_bitrev"} <= applied
    first_of_second_round = (4 << 30) // (16 << R.TWO_ROUND_N)
    assert first_of_second_round == R.TWO_ROUND_B - 1 and first_of_second_round % 3 == 1
    ref = R.compared(case)
    for q in ("state", "expval"):
        assert np.abs(ref[q][first_of_second_round % 3] - ref[q][0]).max() >= R.SEE, q
        assert np.abs(ref[q][(R.TWO_ROUND_B - 2) % 3] - ref[q][first_of_second_round % 3]).max() >= R.SEE, q


def test_all_cases_lists_every_family():
    labels = [c.label for c in R.all_cases()]
    assert len(labels) == len(set(labels))
    for family in "abcdefg":
        assert any(lb.startswith(family + " ") for lb in labels), family


# ---- plan shapes, host only ----------------------------------------------------------------------------------
# per merge case: (operators, plain matrix floats) its gates add behind the prefix -- merged (default flags,
# PLAN_TAPE_ORDER) and one operator per gate (PLAN_NO_MERGE, PLAN_NO_FUSION).  A 2x2 record is 8 floats, a 4x4 one 32;
# the 2x2 records of gates that a later 4x4 took with it (take_pending) stay allocated.
_MERGED = {"1q_onto_1q": (2, 16), "1q_onto_RXX": (1, 32), "1q_onto_MAT2": (1, 32), "4x4_same_pair": (1, 32),
           "4x4_reversed_pair": (2, 64), "4x4_takes_pending": (1, 48)}
_PER_GATE = {"1q_onto_1q": (4, 32), "1q_onto_RXX": (3, 48), "1q_onto_MAT2": (3, 48), "4x4_same_pair": (2, 64),
             "4x4_reversed_pair": (2, 64), "4x4_takes_pending": (4, 56)}


@pytest.mark.parametrize("n", [10, 14])
@pytest.mark.parametrize("merge", R.MERGES)
def test_merge_cases_are_what_their_names_say(merge, n):
    """Default flags: RY.RZ of the prefix is one 2x2 per wire, the CX chain one operator each, and the case's gates
    merge as named -- a one-qubit gate on the first / second wire of a 4x4 (BuildOp::pad 1 / 2) leaves neither an
    operator nor a matrix record of its own.  describe() has no list of a group's members, so the count of operators
    and of plain matrix floats (``mat_floats_old``, inside the row stride ``stats()["mat_floats"]``) is asserted
    against the hand count."""
    from qml_essentials_amd import _native as N

    for case in R.merge_cases(n, merge)[:6]:
        ops, angles, consts = case.native()
        n_gates = len(case.tape)
        for flags in (0, N.PLAN_TAPE_ORDER, N.PLAN_NO_MERGE, N.PLAN_NO_FUSION):
            plan = N.Plan(ops, n, angles.shape[1], consts.astype(np.float32), flags)
            d, st = plan.describe(), plan.stats()
            merged = not flags & (N.PLAN_NO_MERGE | N.PLAN_NO_FUSION)
            pre_ops, pre_floats = (n + n - 1, 8 * (2 * n - 1)) if merged else (3 * n - 1, 8 * (3 * n - 1))
            add_ops, add_floats = (_MERGED if merged else _PER_GATE)[merge]
            assert d["n_ops"] == 3 * n - 1 + n_gates
            assert d["n_lowered"] == pre_ops + add_ops, (case.label, flags, d["n_lowered"])
            assert d["mat_floats_old"] == pre_floats + add_floats, (case.label, flags, d["mat_floats_old"])
            assert st["mat_floats"] == d["mat_row_floats"] >= d["mat_floats_old"]
            if not merged:
                assert d["n_lowered"] == d["n_ops"]
            else:
                assert d["n_lowered"] < d["n_ops"] and d["mat_floats_old"] < 8 * (3 * n - 1) + _PER_GATE[merge][1]
