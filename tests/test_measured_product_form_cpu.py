"""Product-form groups without closing diagonals, host side only: the measured mode of the matrix builder's
record through `qmle_group_product_form_measured` -- the rotation as three shears, no closing diagonal, a flag word --,
the phase-exact mode held bit for bit to the values of the commit before (tests/golden/product_form), and which groups
the plan compiler marks (`closing_free_groups` of `qmle_plan_describe`) while every earlier field keeps its value."""
import ctypes as C
import functools
import os

import numpy as np

from qml_essentials_amd import _native as N
from tests.test_abi_cpu import he_layer_ops
from tests.test_group_product_form_cpu import (BIT_SETS, CLOSE, FORMS, REC, STEPS, TOL, check_product_plan, kron_on_bits,
                                               product_record)
from tests.test_lane_swap_group_cpu import PARENT
from tests.test_measure_in_registers_cpu import ALL_LIVE, N_PARAMS
from tests.test_unit_form_gates_cpu import _fused, _ry, _rz

NO_CLOSE = 44   # the record's flag word, in floats (qmle_sv.h)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "product_form")


def measured_record(mats, bits):
    n = len(mats)
    u = np.ascontiguousarray(np.stack([np.asarray(m, dtype=np.complex128).reshape(4) for m in mats]).view(np.float64).reshape(n, 8))
    rec, forms = np.full(REC, np.nan), (C.c_int * n)()
    rc = N.lib().qmle_group_product_form_measured(u.ctypes.data_as(C.POINTER(C.c_double)), (C.c_int * n)(*bits), n,
                                                   rec.ctypes.data_as(C.POINTER(C.c_double)), forms)
    assert rc == 0
    return rec, list(forms)


def measured_operator(rec):
    """The 16 x 16 operator the kernel applies from a measured-mode record: opening diagonal, then per marked bit the
    three shears a0 += w0 a1; a1 += w1 a0; a0 += w0 a1 -- and nothing else."""
    cplx = lambda a: a.reshape(-1, 2) @ np.array([1, 1j])
    op = np.diag(cplx(rec[:32]))
    for b in range(4):
        form, w0, w1 = rec[FORMS + b], rec[STEPS + 2 * b], rec[STEPS + 2 * b + 1]
        assert form in (0.0, 3.0)
        if form == 0.0:
            assert w0 == 0.0 and w1 == 0.0
            continue
        up, low = np.array([[1, w0], [0, 1]]), np.array([[1, 0], [w1, 1]])
        step = up @ low @ up
        full = np.eye(1)
        for j in (3, 2, 1, 0):
            full = np.kron(full, step if j == b else np.eye(2))
        op = full @ op
    return op


def check_measured(mats, bits, tol=TOL):
    rec, forms = measured_record(mats, bits)
    assert rec[0] == 1.0 and rec[1] == 0.0, "opening entry 0 is a literal 1"
    assert forms == [3] * len(bits) and all(rec[FORMS + b] == 3.0 for b in bits)
    assert all(rec[FORMS + b] == 0.0 for b in set(range(4)) - set(bits))
    assert rec[NO_CLOSE] == 1.0 and rec[NO_CLOSE + 1:CLOSE].tolist() == [0.0] * 3, "the flag word"
    assert np.array_equal(rec[CLOSE:].reshape(16, 2), np.tile([1.0, 0.0], (16, 1))), "closing entries are exact ones"
    for m, b in zip(mats, bits):
        g = np.hypot(abs(m[0, 0]), abs(m[1, 0]))
        c, s = abs(m[0, 0]) / g, abs(m[1, 0]) / g
        w0, w1 = rec[STEPS + 2 * b], rec[STEPS + 2 * b + 1]
        assert 0.0 <= -w0 <= 1.0 and abs(-w0 - s / (1 + c)) <= 1e-15 and abs(w1 - s) <= 1e-15, (w0, w1, c, s)
    # the phase-exact record of the same group: same opening diagonal, bit for bit
    old, _forms = product_record(mats, bits)
    assert np.array_equal(old[:32], rec[:32])
    A = measured_operator(rec)
    B = kron_on_bits([m / np.hypot(abs(m[0, 0]), abs(m[1, 0])) for m in mats], bits)
    err = np.abs(np.abs(A) - np.abs(B)).max()
    assert err <= tol, (err, bits)
    D = B @ np.linalg.inv(A)     # A is unitary up to rounding
    off = np.abs(D - np.diag(np.diag(D))).max()
    assert off <= tol and np.abs(np.abs(np.diag(D)) - 1.0).max() <= tol, (off, bits)
    return rec


def test_random_fused_gates_give_the_group_up_to_unit_phases():
    rng = np.random.default_rng(191)
    for k in range(400):
        bits = BIT_SETS[k % len(BIT_SETS)]
        check_measured([_fused(*rng.uniform(0, 2 * np.pi, 3)) for _ in bits], bits)


def test_scaled_matrices_as_the_chain_leaves_them():
    """U / pivot and P U: the measured mode drops each member's modulus |g|."""
    rng = np.random.default_rng(193)
    for k in range(200):
        us = [_fused(*rng.uniform(0, 2 * np.pi, 3)) for _ in range(4)]
        piv = [u[0, 0] if abs(u[0, 0]) >= abs(u[0, 1]) else u[0, 1] for u in us]
        P = np.prod(piv[:3]) * (rng.uniform(0.5, 1.0) * np.exp(1j * rng.uniform(0, 6.28))) ** (k % 33)
        mats = [us[0] / piv[0], us[1] / piv[1], us[2] / piv[2], P * us[3]]
        check_measured(mats, [0, 1, 2, 3])
        check_measured(mats[2:], [2, 3])


def test_identity_ry_pi_diagonals_and_c_equal_s():
    eye = np.eye(2, dtype=np.complex128)
    r = np.sqrt(0.5)
    h = np.array([[r, -r], [r, r]], dtype=np.complex128)   # |m00| == |m10| bit for bit
    for bits in BIT_SETS:
        rec = check_measured([eye] * len(bits), bits)
        assert all(rec[STEPS + 2 * b] == 0.0 and rec[STEPS + 2 * b + 1] == 0.0 for b in bits)
        # RY(pi): m00 = 6e-17; and c = 0 exactly: tau = 1, s = 1
        check_measured([_ry(np.pi)] * len(bits), bits)
        rec = check_measured([np.array([[0, -1], [1, 0]], dtype=np.complex128)] * len(bits), bits)
        assert all(rec[STEPS + 2 * b] == -1.0 and rec[STEPS + 2 * b + 1] == 1.0 for b in bits)
        rec = check_measured([h] * len(bits), bits)
        assert all(rec[STEPS + 2 * b] == -r / (1 + r) and rec[STEPS + 2 * b + 1] == r for b in bits)
        check_measured([_ry(np.pi / 2)] * len(bits), bits)
    rng = np.random.default_rng(192)
    for _ in range(50):
        rec = check_measured([_rz(t) for t in rng.uniform(0, 2 * np.pi, 4)], BIT_SETS[0])
        assert all(rec[STEPS + 2 * b] == 0.0 and rec[STEPS + 2 * b + 1] == 0.0 for b in range(4)), "s = 0: tau = 0"


def test_the_phase_exact_entry_returns_what_it_returned_before():
    """`qmle_group_product_form` against the records the library of the commit before this mode gave for the same inputs
    (tests/golden/make_product_form_fixtures.py): bit for bit, the unused words still zero."""
    u, want = np.load(os.path.join(GOLDEN, "inputs.npy")), np.load(os.path.join(GOLDEN, "records.npy"))
    assert len(u) == len(want) == 56
    for i in range(len(u)):
        bits = BIT_SETS[i % len(BIT_SETS)]
        mats = [u[i, k].view(np.complex128).reshape(2, 2) for k in range(len(bits))]
        rec, forms = product_record(mats, bits)
        assert np.array_equal(rec.view(np.uint64), want[i].view(np.uint64)), i
        assert set(forms) <= {1, 2} and rec[FORMS + 4:CLOSE].tolist() == [0.0] * 4


def test_invalid_arguments_are_refused():
    u = np.ascontiguousarray(np.stack([np.eye(2, dtype=np.complex128).reshape(4)] * 2).view(np.float64))
    rec = np.zeros(REC)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    f = N.lib().qmle_group_product_form_measured
    assert f(dp(u), (C.c_int * 2)(1, 1), 2, dp(rec), None) != 0, "two members on one bit"
    assert f(dp(u), (C.c_int * 2)(0, 4), 2, dp(rec), None) != 0
    assert f(dp(u), (C.c_int * 2)(0, 1), 5, dp(rec), None) != 0
    assert f(dp(u), (C.c_int * 2)(0, 1), 2, dp(rec), None) == 0, "forms may be NULL"


# ---- which groups the plan compiler marks ----------------------------------------------------------------------------

N_Q = 16
# name: (front-group gates in front of its four RY, last-group gates, gates behind the closing CX pair; what the last
#        stage reports: product_form_groups, closing_free_groups, lane swap, crossed)
VARIANTS = {
    # the rotation layer and the CX ring: every group capable
    "all": ("cx", [("Rot", 8), ("Rot", 9)], [], [True, True], [True, True], True, False),
    # a one-op last group that runs gate by gate behind a capable group (a diagonal behind the carrier stays plain, so
    # the chain is whole in the front group): straight, and the crossed swaps
    "one_op_last": ("cx", [("RZ", 9)], [], [True, False], [True, False], True, False),
    "one_op_last_crossed": ("cx", [("RZ", 8)], [], [True, False], [True, False], True, True),
    # only the last group capable: the front group holds controlled rotations, which no chain takes
    "only_last": ("crx3", [("Rot", 8), ("Rot", 9)], [], [False, True], [False, True], True, False),
}


def tape(name, tile_bits, n=N_Q, variants=VARIANTS):
    """struct of a hand-built tape, entries (gate, wires), wire = n - 1 - position, after `tape` of
    tests/test_gpu_group_product_form.py: the top positions first, so that they fill the earlier stages; then the group
    {4, 5, 6, 7}, two CX inside it, the last group's gates on positions 8 and / or 9, the CX pair that closes the ring,
    and whatever the variant puts behind it."""
    def P(pos):
        return n - 1 - pos

    front, last, behind = variants[name][:3]
    top = list(range(15, 9 if tile_bits == 10 else 10, -1))
    t = [("Rot", [P(p)]) for p in top + [0, 1, 2, 3, 4, 5, 6]]
    t += [("CZ", [P(p), P(i % 4)]) for i, p in enumerate(top)] + [("CX", [P(3), P(4)]), ("CX", [P(2), P(5)])]
    if front == "cx":
        t += [("CX", [P(7), P(4)]), ("CX", [P(7), P(5)]), ("CX", [P(7), P(6)])]
    elif front == "rot_cx":
        t += [("Rot", [P(7)]), ("CX", [P(7), P(4)]), ("CX", [P(7), P(5)]), ("CX", [P(7), P(6)])]
    else:
        assert front == "crx3"
        t += [("CRX", [P(7), P(4)]), ("CRX", [P(7), P(5)]), ("CRX", [P(7), P(6)])]
    if front != "crx3":
        t += [("RY", [P(p)]) for p in (4, 5, 6, 7)]
    t += [("CX", [P(5), P(4)]), ("CX", [P(7), P(6)])]
    t += [(g, [P(pos)]) for g, pos in last]
    t += [("CX", [P(9), P(8)]), ("CX", [P(8), P(7)])]
    t += [(g, [P(pos) for pos in poss]) for g, poss in behind]
    return t


def to_ops(struct):
    ops, k = [], 0
    for g, wires in struct:
        npar = N_PARAMS.get(g, 0)
        ops.append((g, list(wires), list(range(k, k + npar)), -1))
        k += npar
    return ops, k


def plan_of(struct, tile_bits, flags=ALL_LIVE):
    ops, slots = to_ops(struct)
    return N.Plan(ops, N_Q, slots, flags=flags | N.PLAN_TAPE_ORDER | N.plan_flags(tile_bits=tile_bits))


def check_closing_free(desc):
    """closing_free_groups is parallel to product_form_groups, marks product-form groups only, and nothing has run."""
    check_product_plan(desc)
    for st in desc["stages"]:
        if st["kind"] != "tile" or not st["fast"]:
            assert not any(st.get("closing_free_groups", []))
            continue
        free, marks = st["closing_free_groups"], st["product_form_groups"]
        assert len(free) == len(marks) and all(m or not f for f, m in zip(free, marks))
        assert st["measured_form_last_run"] is False


@functools.lru_cache(maxsize=None)
def _headline(n):
    ops, slots = he_layer_ops(n)
    return N.Plan(ops, n, slots, flags=ALL_LIVE).executed("expval").describe()


def test_headline_stage_marks_all_three_groups_and_keeps_every_earlier_field():
    d = _headline(24)
    last = d["stages"][-1]
    assert last["product_form_groups"] == [True, True, True] and last["closing_free_groups"] == [True, True, True]
    # the literals of tests/test_group_product_form_cpu.py, tests/test_unit_form_gates_cpu.py, tests/test_lane_swap_group_cpu.py
    assert [g["n_ops"] for g in last["fast_groups"]] == [4, 4, 2]
    assert last["unit_form_ops"] == list(range(9)) and last["scale_carriers"] == [9]
    assert d["mat_floats_old"] == 8 * 48 and d["mat_floats"] == 8 * 58 == PARENT[24]["mat_floats"]
    assert d["mat_row_floats"] == 8 * 58 + 3 * REC
    assert last["product_form_records"] == [8 * 58, 8 * 58 + REC, 8 * 58 + 2 * REC]
    for key in ("fast_ops", "fast_groups", "measure_records"):
        assert last[key] == PARENT[24][key], key
    check_closing_free(d)
    # the plan's own stages (live states): the mark is a property of a stage of a plan, whatever later runs it
    ops, slots = he_layer_ops(24)
    check_closing_free(N.Plan(ops, 24, slots, flags=ALL_LIVE).describe())


def test_23_qubit_layer_has_its_carrier_in_the_one_op_group_and_stays_unmarked():
    """Its two product-form groups pass rule 1, but the chain's carrier is the one op of the last group, which runs gate
    by gate and applies P U with |P| the product of the pivots' moduli: measured records in front of it would leave the
    state scaled by |P|.  Rule 2 keeps the chain whole, so the layer runs the phase-exact records, as before."""
    d = _headline(23)
    last = d["stages"][-1]
    assert [g["n_ops"] for g in last["fast_groups"]] == [4, 4, 1]
    assert last["product_form_groups"] == [True, True, False]
    # the one-op last group holds the carrier of the chain: the chain is split between the marked groups and it
    assert last["scale_carriers"] == [8]
    assert last["closing_free_groups"] == [False, False, False]
    assert d["mat_floats"] == PARENT[23]["mat_floats"]
    for key in ("fast_ops", "fast_groups", "measure_records"):
        assert last[key] == PARENT[23][key], key
    check_closing_free(d)


def _last(name, tile_bits, variants=VARIANTS):
    d = plan_of(tape(name, tile_bits, variants=variants), tile_bits).executed("expval").describe()
    check_closing_free(d)
    last = d["stages"][-1]
    assert last["T"] == tile_bits
    return last


def test_the_variants_are_what_their_names_say():
    for tile_bits in (10, 12):
        for name, (_f, _l, _b, marks, free, swap, crossed) in VARIANTS.items():
            last = _last(name, tile_bits)
            assert len(last["fast_groups"]) == 2, name
            assert last["product_form_groups"] == marks and last["closing_free_groups"] == free, (name, last["closing_free_groups"])
            assert last["last_group_lane_swap"] is swap, name
            if swap:
                assert last["lane_swap_crossed"] is crossed, name
    assert [g["n_ops"] for g in _last("one_op_last", 10)["fast_groups"]] == [4, 1]
    assert _last("one_op_last", 10)["scale_carriers"] == [3], "the carrier sits in the front group"
    codes = [c for c, _o in _last("only_last", 10)["fast_ops"]]
    assert len(codes) == 5 and all(4 <= c < 16 for c in codes[:3]), "controlled dense gates in the front group"


UNMARKED = {
    # a rotation in front of the CX fan on a wire that an RY of the next group follows: two gathers, both groups in
    # product form (`three_and_four` of tests/test_gpu_group_product_form.py), the first fails rule 1, the chain is split
    "rot_then_ry": ("rot_cx", [("Rot", 8), ("Rot", 9)], []),
    # an RY on a member's wire behind the CX ring
    "ry_behind": ("cx", [("Rot", 8), ("Rot", 9)], [("RY", [4])]),
    # a CRX on wires the ring has spread both groups to
    "crx_behind": ("cx", [("Rot", 8), ("Rot", 9)], [("CRX", [9, 8])]),
    # a diagonal on the last group's wire: that group fails rule 1, the front group passes it (position 9 is reached
    # from 8 before 8 is reached from 7) -- and the chain, units in front and carrier behind, is split
    "split_chain": ("cx", [("Rot", 8), ("Rot", 9)], [("RZ", [9])]),
}


def test_a_gate_behind_the_ring_or_a_split_chain_leaves_the_groups_unmarked():
    for tile_bits in (10, 12):
        for name in UNMARKED:
            last = _last(name, tile_bits, variants=UNMARKED)
            assert any(last["product_form_groups"]), name
            assert not any(last["closing_free_groups"]), (name, last["closing_free_groups"])
            # every record is still there, where it was
            assert all((o >= 0) == m for o, m in zip(last["product_form_records"], last["product_form_groups"]))
