"""Product form of a fast-kernel gate group, host side only: the matrix builder's decomposition
M = g diag(1, l) [[c, -s], [s, c]] diag(1, r), its two real-step forms and the two diagonals of a group through
`qmle_group_product_form`, and which groups the plan compiler marks (`product_form_groups`, `product_form_records`,
`mat_row_floats` of `qmle_plan_describe`) while every earlier field of the report keeps its value."""
import ctypes as C
import functools

import numpy as np
import pytest

from qml_essentials_amd import _native as N
from tests.test_abi_cpu import he_layer_ops
from tests.test_lane_swap_group_cpu import PARENT
from tests.test_measure_in_registers_cpu import ALL_LIVE, FUZZ_SEEDS, fuzz_struct, to_native
from tests.test_unit_form_gates_cpu import _check_stage, _fused, _ry, _rz

REC, STEPS, FORMS, CLOSE = 80, 32, 40, 48   # the record's layout, in floats (qmle_sv.h)
TOL = 1e-12


def product_record(mats, bits):
    n = len(mats)
    u = np.ascontiguousarray(np.stack([np.asarray(m, dtype=np.complex128).reshape(4) for m in mats]).view(np.float64).reshape(n, 8))
    rec, forms = np.full(REC, np.nan), (C.c_int * n)()
    rc = N.lib().qmle_group_product_form(u.ctypes.data_as(C.POINTER(C.c_double)), (C.c_int * n)(*bits), n,
                                          rec.ctypes.data_as(C.POINTER(C.c_double)), forms)
    assert rc == 0
    return rec, list(forms)


def record_operator(rec):
    """The 16 x 16 operator the kernel applies from a record: opening diagonal, one real step per marked bit in the
    form its word names (the direct one as its two in-place FMAs), closing diagonal."""
    cplx = lambda a: a.reshape(-1, 2) @ np.array([1, 1j])
    op = np.diag(cplx(rec[:32]))
    for b in range(4):
        form, w0, w1 = rec[FORMS + b], rec[STEPS + 2 * b], rec[STEPS + 2 * b + 1]
        assert form in (0.0, 1.0, 2.0)
        if form == 0.0:
            assert w0 == 0.0 and w1 == 0.0
            continue
        if form == 1.0:   # a0 += w0 a1 (w0 = -t), then a1 += w1 a0
            step = np.array([[1, 0], [w1, 1]]) @ np.array([[1, w0], [0, 1]])
        else:             # (a0, a1) <- (t' a0 - a1, a0 + t' a1)
            assert w1 == 0.0
            step = np.array([[w0, -1], [1, w0]])
        full = np.eye(1)
        for j in (3, 2, 1, 0):   # index bit 3 is the leftmost factor
            full = np.kron(full, step if j == b else np.eye(2))
        op = full @ op
    assert rec[FORMS + 4:CLOSE].tolist() == [0.0] * 4
    return np.diag(cplx(rec[CLOSE:])) @ op


def kron_on_bits(mats, bits):
    full = np.eye(1)
    for j in (3, 2, 1, 0):
        full = np.kron(full, mats[bits.index(j)] if j in bits else np.eye(2))
    return full


def check_group(mats, bits, tol=TOL):
    rec, forms = product_record(mats, bits)
    assert rec[0] == 1.0 and rec[1] == 0.0, "opening entry 0 is a literal 1"
    want = kron_on_bits(mats, bits)
    scale = max(1.0, np.abs(want).max())
    err = np.abs(record_operator(rec) - want).max() / scale
    assert err <= tol, (err, bits)
    for m, b, f in zip(mats, bits, forms):
        c, s = abs(m[0, 0]), abs(m[1, 0])
        assert f == (1 if c >= s else 2) and rec[FORMS + b] == f
        w0, w1 = rec[STEPS + 2 * b], rec[STEPS + 2 * b + 1]
        if f == 1:
            t = -w0
            assert 0.0 <= t <= 1.0 and abs(t - s / c) <= 1e-15 and abs(w1 - t / (1 + t * t)) <= 1e-15
        else:
            assert 0.0 <= w0 < 1.0 and abs(w0 - c / s) <= 1e-15 and w1 == 0.0
    for b in set(range(4)) - set(bits):
        assert rec[FORMS + b] == 0.0
    return rec, forms


BIT_SETS = [[0, 1, 2, 3], [3, 1, 0, 2], [2, 3], [0, 3], [1, 2, 3], [0, 1, 2], [1]]


def test_random_fused_gates_reconstruct():
    rng = np.random.default_rng(91)
    seen = set()
    for k in range(400):
        bits = BIT_SETS[k % len(BIT_SETS)]
        mats = [_fused(*rng.uniform(0, 2 * np.pi, 3)) for _ in bits]
        _rec, forms = check_group(mats, bits)
        seen |= set(forms)
    assert seen == {1, 2}


def test_identity_ry_pi_diagonals_and_antidiagonals():
    eye = np.eye(2, dtype=np.complex128)
    for bits in BIT_SETS:
        rec, forms = check_group([eye] * len(bits), bits)
        assert forms == [1] * len(bits)
        assert np.array_equal(rec[:32].reshape(16, 2), np.tile([1.0, 0.0], (16, 1))), "r = 1 where s = 0"
        # RY(pi) on every member: m00 = cos(pi / 2) = 6e-17, the mirrored form with t' of that size
        _rec, forms = check_group([_ry(np.pi)] * len(bits), bits)
        assert forms == [2] * len(bits)
        # ... and with m00 = 0 exactly (c = 0: l = 1)
        rec, forms = check_group([np.array([[0, -1], [1, 0]], dtype=np.complex128)] * len(bits), bits)
        assert forms == [2] * len(bits) and all(rec[STEPS + 2 * b] == 0.0 for b in bits)
    rng = np.random.default_rng(92)
    for _ in range(50):
        bits = BIT_SETS[0]
        diags = [_rz(t) for t in rng.uniform(0, 2 * np.pi, 4)]
        rec, forms = check_group(diags, bits)
        assert forms == [1, 1, 1, 1] and all(rec[STEPS + 2 * b] == 0.0 and rec[STEPS + 2 * b + 1] == 0.0 for b in bits)
        anti = [np.array([[0, np.exp(1j * a)], [np.exp(1j * b), 0]]) for a, b in rng.uniform(0, 2 * np.pi, (4, 2))]
        _rec, forms = check_group(anti, bits)
        assert forms == [2, 2, 2, 2]
        check_group([diags[0], anti[1], _fused(0.3, 1.1, 2.5)], [2, 0, 3])


def test_c_equal_s_takes_the_direct_form():
    r = np.sqrt(0.5)
    h = np.array([[r, -r], [r, r]], dtype=np.complex128)   # |m00| == |m10| bit for bit
    ph = np.exp(0.7j)
    rec, forms = check_group([h, ph * h, np.diag([1, 1j]) @ h @ np.diag([1, -1j])], [0, 1, 3])
    assert forms == [1, 1, 1]
    assert all(rec[STEPS + 2 * b] == -1.0 and rec[STEPS + 2 * b + 1] == 0.5 for b in (0, 1, 3))
    # RY(pi / 2) as the builder's fp64 cos and sin give it: whichever way they round, the rule is c >= s
    check_group([_ry(np.pi / 2)] * 4, [0, 1, 2, 3])


def test_scaled_matrices_as_the_chain_leaves_them():
    """U / pivot (unit-form members) and P U (the carrier): a scalar times a unitary, moduli from 1 / sqrt 2 up to the
    2^16 a full chain can reach."""
    rng = np.random.default_rng(93)
    for k in range(200):
        us = [_fused(*rng.uniform(0, 2 * np.pi, 3)) for _ in range(4)]
        piv = [u[0, 0] if abs(u[0, 0]) >= abs(u[0, 1]) else u[0, 1] for u in us]
        P = np.prod(piv[:3]) * (rng.uniform(0.5, 1.0) * np.exp(1j * rng.uniform(0, 6.28))) ** (k % 33)
        mats = [us[0] / piv[0], us[1] / piv[1], us[2] / piv[2], P * us[3]]
        check_group(mats, [0, 1, 2, 3])
        check_group(mats[2:], [2, 3])


def test_invalid_arguments_are_refused():
    eye = np.eye(2, dtype=np.complex128)
    u = np.ascontiguousarray(np.stack([eye.reshape(4)] * 2).view(np.float64))
    rec = np.zeros(REC)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    f = N.lib().qmle_group_product_form
    assert f(dp(u), (C.c_int * 2)(1, 1), 2, dp(rec), None) != 0, "two members on one bit"
    assert f(dp(u), (C.c_int * 2)(0, 4), 2, dp(rec), None) != 0
    assert f(dp(u), (C.c_int * 2)(0, 1), 5, dp(rec), None) != 0
    assert f(dp(u), (C.c_int * 2)(0, 1), 2, dp(rec), None) == 0, "forms may be NULL"


# ---- which groups the plan compiler marks ----------------------------------------------------------------------------

def check_product_stage(desc, st):
    """Per tile stage: a marked group holds >= 2 uncontrolled dense / diagonal / unit-form ops on distinct bits, its
    record sits behind the unit-form records, records do not overlap and stay inside the row."""
    if st["kind"] != "tile":
        assert "product_form_groups" not in st
        return []
    _check_stage(desc, st)   # every earlier field as tests/test_unit_form_gates_cpu.py checks it
    if not st["fast"]:
        assert "product_form_groups" not in st or not any(st["product_form_groups"])
        return []
    marks, recs = st["product_form_groups"], st["product_form_records"]
    assert len(marks) == len(recs) == len(st["fast_groups"])
    k, out = 0, []
    for g, mark, off in zip(st["fast_groups"], marks, recs):
        codes = [c for c, _o in st["fast_ops"][k:k + g["n_ops"]]]
        k += g["n_ops"]
        plain = all(c < 4 or 16 <= c < 20 or 48 <= c < 56 for c in codes)
        distinct = len({c & 3 for c in codes}) == len(codes)
        if mark:
            assert g["n_ops"] >= 2 and plain and distinct, codes
            assert off % 8 == 0 and desc["mat_floats"] <= off and off + REC <= desc["mat_row_floats"]
            out.append(off)
        else:
            assert off == -1
            if g["n_ops"] >= 2 and plain and distinct:
                # eligible by its codes, yet unmarked: some op's matrix holds a caller's constant
                assert any(st["fast_ops"][i][1] < desc["mat_floats_old"] and i not in st["scale_carriers"]
                           for i in range(k - g["n_ops"], k))
    assert st["group_product_form_last_run"] is False, "nothing has run"
    return out


def check_product_plan(desc):
    offs = sorted(o for st in desc["stages"] for o in check_product_stage(desc, st))
    assert offs == list(range(desc["mat_floats"], desc["mat_floats"] + REC * len(offs), REC))
    assert desc["mat_row_floats"] == desc["mat_floats"] + REC * len(offs)
    return offs


@functools.lru_cache(maxsize=None)
def _headline(n):
    ops, slots = he_layer_ops(n)
    return N.Plan(ops, n, slots, flags=ALL_LIVE).executed("expval").describe()


def test_headline_stage_marks_all_three_groups_and_keeps_every_earlier_field():
    d = _headline(24)
    last = d["stages"][-1]
    assert [g["n_ops"] for g in last["fast_groups"]] == [4, 4, 2]
    assert last["product_form_groups"] == [True, True, True]
    # the literals of tests/test_unit_form_gates_cpu.py and tests/test_lane_swap_group_cpu.py
    assert last["unit_form_ops"] == list(range(9)) and last["scale_carriers"] == [9]
    assert d["mat_floats_old"] == 8 * 48 and d["mat_floats"] == 8 * 58 == PARENT[24]["mat_floats"]
    for key in ("fast_ops", "fast_groups", "measure_records"):
        assert last[key] == PARENT[24][key], key
    assert last["last_group_lane_swap"] is True and last["lane_swap_crossed"] is False
    assert last["staging"] == "dma" and last["wave_private_walk"] is True
    offs = check_product_plan(d)
    assert last["product_form_records"] == offs[-3:]
    own = N.Plan(*_args(24), flags=ALL_LIVE).describe()
    assert [len(s["unit_form_ops"]) for s in own["stages"]] == [11, 7, 3]
    assert own["mat_floats_old"] == d["mat_floats_old"]
    check_product_plan(own)


def _args(n):
    ops, slots = he_layer_ops(n)
    return ops, n, slots


def test_23_qubit_layer_marks_its_two_four_op_groups():
    d = _headline(23)
    last = d["stages"][-1]
    assert [g["n_ops"] for g in last["fast_groups"]] == [4, 4, 1]
    assert last["product_form_groups"] == [True, True, False] and last["product_form_records"][2] == -1
    assert d["mat_floats"] == PARENT[23]["mat_floats"]
    for key in ("fast_ops", "fast_groups", "measure_records"):
        assert last[key] == PARENT[23][key], key
    assert last["last_group_lane_swap"] is True and last["lane_swap_crossed"] is True
    check_product_plan(d)


def test_controlled_constant_and_same_bit_ops_leave_a_group_unmarked():
    n = 16
    h = np.array([1, 0, 1, 0, 1, 0, -1, 0], dtype=np.float32) / np.sqrt(2.0).astype(np.float32)
    flags = ALL_LIVE | N.PLAN_FORCE_TILE | N.PLAN_TAPE_ORDER

    def fast_stage(ops, slots, consts=None):
        d = N.Plan(ops, n, slots, consts=consts, flags=flags).describe()
        stages = [s for s in d["stages"] if s["fast"]]
        assert len(stages) == 1
        check_product_plan(d)
        return d, stages[0]

    def groups_of(st, wires):
        """marks of the groups that hold a position of `wires`"""
        pos = {n - 1 - w for w in wires}
        return [m for g, m in zip(st["fast_groups"], st["product_form_groups"]) if pos & set(g["bits"]) and g["n_ops"]]

    # four rotations on one group's positions: marked
    ops = [("RX", [n - 1 - p], [p], -1) for p in range(4)]
    _d, st = fast_stage(ops, 4)
    assert groups_of(st, [n - 1 - p for p in range(4)]) == [True]
    # ... with a CRX among them: unmarked
    _d, st = fast_stage(ops + [("CRX", [n - 1, n - 2], [4], -1)], 5)
    assert groups_of(st, [n - 1]) == [False]
    # ... with a caller's constant matrix (it need not be unitary): unmarked
    _d, st = fast_stage(ops[:3] + [("MAT1", [n - 4], [], 0)], 3, consts=h)
    assert groups_of(st, [n - 1]) == [False]
    # ... two ops on one bit that a controlled gate keeps from merging: unmarked
    two = [("RX", [n - 1], [0], -1), ("RY", [n - 2], [1], -1), ("CRX", [n - 3, n - 4], [2], -1), ("RZ", [n - 1], [3], -1)]
    d, st = fast_stage(two, 4)
    assert not any(st["product_form_groups"])
    assert d["mat_row_floats"] == d["mat_floats"]


@pytest.mark.parametrize("seed", FUZZ_SEEDS[:8])
def test_fuzz_tapes_keep_every_old_record(seed):
    ops, slots = to_native(fuzz_struct(seed, 16))
    for flags in (0, ALL_LIVE, ALL_LIVE | N.plan_flags(tile_bits=10)):
        plan = N.Plan(ops, 16, slots, flags=flags)
        for d in (plan.describe(), plan.executed("expval").describe()):
            check_product_plan(d)
            assert d["mat_floats_old"] <= d["mat_floats"] <= d["mat_row_floats"]
