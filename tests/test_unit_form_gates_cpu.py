"""Unit-pivot form of the fast tile kernel's gates, host side only: which ops of a stage the plan compiler marks
(`unit_form_ops`, `scale_carriers` and `fast_ops` of `qmle_plan_describe`), where their records go in the matrix row,
and the matrix builder's pivot rule and chain product through `qmle_unit_form_chain`."""
import ctypes as C

import numpy as np
import pytest

from qml_essentials_amd import _native as N
from tests.test_abi_cpu import he_layer_ops
from tests.test_measure_in_registers_cpu import ALL_LIVE, FUZZ_SEEDS, fuzz_struct, to_native

FC_DENSE, FC_CDENSE, FC_DIAG, FC_CDIAG, FC_X, FC_UDENSE, FC_UDIAG, FC_COUNT = 0, 4, 16, 20, 32, 48, 52, 56
MAX_CHAIN = 32


def _chains(stage):
    """The stage's chains as (unit-form ops, carrier): a carrier closes the chain of the unit-form ops since the
    carrier before it."""
    units, carriers = stage["unit_form_ops"], stage["scale_carriers"]
    assert units == sorted(units) and carriers == sorted(carriers) and not set(units) & set(carriers)
    out, lo = [], -1
    for c in carriers:
        out.append(([u for u in units if lo < u < c], c))
        lo = c
    assert sum(len(u) for u, _c in out) == len(units), "a unit-form op behind the last carrier keeps its pivot"
    return out


def _check_stage(desc, stage):
    """What holds for every tile stage: chain lengths, codes, and where the records sit."""
    old, row = desc["mat_floats_old"], desc["mat_floats"]
    ops = stage["fast_ops"]
    if not stage["fast"]:
        assert not stage["unit_form_ops"] and not stage["scale_carriers"] and not ops
        return
    assert len(ops) == sum(g["n_ops"] for g in stage["fast_groups"])
    for units, carrier in _chains(stage):
        assert 1 <= len(units) <= MAX_CHAIN
        assert FC_DENSE <= ops[carrier][0] < FC_CDENSE, "a carrier is a plain dense gate"
    marked = set(stage["unit_form_ops"]) | set(stage["scale_carriers"])
    for i, (code, off) in enumerate(ops):
        assert 0 <= code < FC_COUNT and off % 8 == 0
        assert (FC_UDENSE <= code < FC_COUNT) == (i in stage["unit_form_ops"])
        # new records behind the old row; every other op reads the record it always read
        assert (old <= off < row) if i in marked else (off < old), (i, code, off)


def _executed(ops, n, slots, flags=ALL_LIVE, meas="expval"):
    return N.Plan(ops, n, slots, flags=flags).executed(meas).describe()


def test_headline_measuring_stage_has_nine_unit_form_ops_and_one_carrier():
    ops, slots = he_layer_ops(24)
    d = _executed(ops, 24, slots)
    last = d["stages"][-1]
    assert [g["n_ops"] for g in last["fast_groups"]] == [4, 4, 2]
    assert last["unit_form_ops"] == list(range(9)) and last["scale_carriers"] == [9]
    assert all(FC_UDENSE <= c < FC_UDIAG for c, _o in last["fast_ops"][:9])
    for st in d["stages"]:
        _check_stage(d, st)
    # the plain records: one per lowered operator (24 fused RY.RZ.RY + 24 CX), as before; 10 new ones behind them
    assert d["mat_floats_old"] == 8 * 48 and d["mat_floats"] == 8 * 58
    new = sorted(o for st in d["stages"] for i, (_c, o) in enumerate(st["fast_ops"])
                 if i in st["unit_form_ops"] or i in st["scale_carriers"])
    assert new == list(range(8 * 48, 8 * 58, 8))
    # the plan's own schedule (live states: apply_inplace, the adjoint sweep) gets its chains per stage too
    own = N.Plan(ops, 24, slots, flags=ALL_LIVE).describe()
    assert [len(s["unit_form_ops"]) for s in own["stages"]] == [11, 7, 3]
    assert [len(s["scale_carriers"]) for s in own["stages"]] == [1, 1, 1]
    assert own["mat_floats_old"] == d["mat_floats_old"]
    for st in own["stages"]:
        _check_stage(own, st)


def test_a_stage_with_one_eligible_op_reports_none():
    n = 16
    struct = [("RX", [0])] + [("CRX", [w, w + 1]) for w in range(n - 1)]
    ops, slots = to_native(struct)
    d = N.Plan(ops, n, slots, flags=ALL_LIVE | N.PLAN_FORCE_TILE).describe()
    fast = [s for s in d["stages"] if s["fast"]]
    assert fast
    for s in d["stages"]:
        assert not s["unit_form_ops"] and not s["scale_carriers"]
    assert d["mat_floats"] == d["mat_floats_old"]
    # two eligible ops, the second one diagonal (tape order kept): no dense op behind it to carry the pivot
    ops, slots = to_native([("RX", [0]), ("RZ", [1])] + [("CRX", [w, w + 1]) for w in range(n - 1)])
    d = N.Plan(ops, n, slots, flags=ALL_LIVE | N.PLAN_FORCE_TILE | N.PLAN_TAPE_ORDER).describe()
    assert all(not s["unit_form_ops"] and not s["scale_carriers"] for s in d["stages"])
    # ... a diagonal op in front of a dense one takes the unit form, the dense one carries
    ops, slots = to_native([("RZ", [1]), ("RX", [0])] + [("CRX", [w, w + 1]) for w in range(2, n - 1)])
    d = N.Plan(ops, n, slots, flags=ALL_LIVE | N.PLAN_FORCE_TILE | N.PLAN_TAPE_ORDER).describe()
    marked = [s for s in d["stages"] if s["unit_form_ops"]]
    assert len(marked) == 1 and len(marked[0]["unit_form_ops"]) == 1 and len(marked[0]["scale_carriers"]) == 1
    u, c = marked[0]["unit_form_ops"][0], marked[0]["scale_carriers"][0]
    assert FC_UDIAG <= marked[0]["fast_ops"][u][0] < FC_COUNT and u < c


def test_controlled_and_constant_matrix_gates_are_not_eligible():
    n = 16
    h = np.array([1, 0, 1, 0, 1, 0, -1, 0], dtype=np.float32) / np.sqrt(2.0).astype(np.float32)
    ops = [("RX", [0], [0], -1), ("RY", [1], [1], -1),
           ("CRX", [2, 3], [2], -1), ("CRZ", [3, 4], [3], -1),
           ("MAT1", [5], [], 0), ("RY", [6], [4], -1), ("MAT1", [6], [], 0),   # a product with a constant in it
           ("RX", [7], [5], -1)]
    d = N.Plan(ops, n, 6, consts=h, flags=ALL_LIVE | N.PLAN_FORCE_TILE).describe()
    stages = [s for s in d["stages"] if s["fast"]]
    assert len(stages) == 1
    st = stages[0]
    _check_stage(d, st)
    codes = [c for c, _o in st["fast_ops"]]
    assert len(codes) == 7
    plain_dense = [i for i, c in enumerate(codes) if FC_DENSE <= c < FC_CDENSE]
    ctl = [i for i, c in enumerate(codes) if FC_CDENSE <= c < FC_DIAG or FC_CDIAG <= c < FC_X]
    assert len(ctl) == 2 and not set(ctl) & (set(st["unit_form_ops"]) | set(st["scale_carriers"]))
    # RX[0], RY[1], RX[7] are eligible: two unit-form ops and the carrier; the two constant-matrix ops stay plain
    assert len(st["unit_form_ops"]) == 2 and len(st["scale_carriers"]) == 1
    assert len(plain_dense) == 3 and sum(i not in st["scale_carriers"] for i in plain_dense) == 2
    assert d["mat_floats"] - d["mat_floats_old"] == 8 * 3


@pytest.mark.parametrize("seed", FUZZ_SEEDS[:8])
def test_fuzz_tapes_keep_the_old_records_and_bound_their_chains(seed):
    ops, slots = to_native(fuzz_struct(seed, 16))
    for flags in (ALL_LIVE, 0, ALL_LIVE | N.plan_flags(tile_bits=10)):
        plan = N.Plan(ops, 16, slots, flags=flags)
        d = plan.executed("expval").describe()
        if flags & N.PLAN_NO_ABSORB:  # (else the executed plan runs a shorter tape: the folded tail is gone)
            assert d["mat_floats_old"] == plan.describe()["mat_floats_old"]
        for st in d["stages"]:
            _check_stage(d, st)


def test_a_chain_longer_than_32_is_split():
    n = 20
    ops, slots = [], 0
    for _layer in range(4):
        layer, k = he_layer_ops(n)
        ops += [(name, w, [s + slots for s in sl], c) for name, w, sl, c in layer]
        slots += k
    # (the plan's own schedule, 13-bit tiles: its second stage holds 35 eligible ops; the from-zero variant that a
    # batch run executes spreads them differently and stays at 31 + 1 -- tests/test_gpu_unit_form_gates.py forces this one)
    d = N.Plan(ops, n, slots, flags=ALL_LIVE).describe()
    for st in d["stages"]:
        _check_stage(d, st)
    assert max(len(st["scale_carriers"]) for st in d["stages"]) >= 2
    assert max(len(u) for st in d["stages"] for u, _c in _chains(st)) == MAX_CHAIN
    for st in _executed(ops, n, slots)["stages"]:
        assert len(st["unit_form_ops"]) <= MAX_CHAIN


# ---- the matrix builder's chain, on the host -------------------------------------------------------------------------

def _ry(t):
    c, s = np.cos(t / 2), np.sin(t / 2)
    return np.array([[c, -s], [s, c]], dtype=np.complex128)


def _rz(t):
    return np.diag([np.exp(-0.5j * t), np.exp(0.5j * t)])


def _fused(a, b, c):
    return _ry(c) @ _rz(b) @ _ry(a)   # tape order RY, RZ, RY: the later gate on the left


def _chain(mats, diag=None):
    n = len(mats)
    u = np.ascontiguousarray(np.stack([m.reshape(4) for m in mats]).view(np.float64).reshape(n, 8))
    rec, piv, car = np.zeros((max(n - 1, 1), 8)), np.zeros((max(n - 1, 1), 2)), np.zeros(8)
    dg = None if diag is None else (C.c_int * n)(*diag)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert N.lib().qmle_unit_form_chain(dp(u), dg, n, dp(rec), dp(piv), dp(car)) == 0
    cplx = lambda a: a.reshape(-1, 2) @ np.array([1, 1j])
    return rec[:n - 1], cplx(piv[:n - 1]), cplx(car).reshape(2, 2)


def _unit_matrix(rec):
    x, y, z = rec[0] + 1j * rec[1], rec[2] + 1j * rec[3], rec[4] + 1j * rec[5]
    form = rec[6]
    assert rec[7] == 0 and form in (1.0, 2.0)
    return (np.array([[1, x], [y, z]]) if form == 1.0 else np.array([[x, 1], [y, z]])), int(form)


ANGLE_SETS = [(0, 0, 0), (np.pi, 0, 0), (np.pi / 2, 0, 0), (np.pi, np.pi, np.pi), (2 * np.pi, 0, 0)]


def test_pivot_rule_and_chain_product():
    rng = np.random.default_rng(77)
    angles = ANGLE_SETS + [tuple(a) for a in rng.uniform(0, 2 * np.pi, (1000, 3))]
    mats = [_fused(*a) for a in angles]
    # chains of 32 unit-form ops + a carrier, as the plan compiler cuts them
    for lo in range(0, len(mats), MAX_CHAIN):
        members = mats[lo:lo + MAX_CHAIN]
        last = mats[(lo + 7) % len(mats)]
        rec, piv, car = _chain(members + [last])
        P = 1.0 + 0j
        for U, r, p in zip(members, rec, piv):
            Up, form = _unit_matrix(r)
            assert np.abs(p * Up - U).max() <= 1e-15
            assert (form == 1) == (abs(U[0, 0]) >= abs(U[0, 1]))
            assert p == (U[0, 0] if form == 1 else U[0, 1])
            assert abs(p) >= 0.7071 - 1e-12
            P *= p
        assert np.abs(car - P * last).max() <= 1e-14 * max(1.0, abs(P))
        assert 2.0 ** -16 * (1 - 1e-12) <= abs(P) <= 1.0 + 1e-12
    # the named angle sets: the identity is form 1; RY(pi) has m00 = 0 up to the rounding of cos(pi / 2), form 2;
    # RY(pi) RZ(pi) RY(pi) = diag(-i, i) up to rounding and RY(2 pi) = -1 are form 1 (RY(pi / 2), the tie, goes by
    # the rule above, whichever way cos and sin of pi / 4 round)
    forms = [_unit_matrix(r)[1] for r in _chain(mats[:5] + [mats[5]])[0]]
    assert [forms[i] for i in (0, 1, 3, 4)] == [1, 2, 1, 1]
    exact_zero = np.array([[0, -1], [1, 0]], dtype=np.complex128)   # m00 = 0 exactly
    rec, piv, car = _chain([exact_zero, mats[5]])
    Up, form = _unit_matrix(rec[0])
    assert form == 2 and piv[0] == -1 and np.array_equal(piv[0] * Up, exact_zero)
    assert np.abs(car - piv[0] * mats[5]).max() <= 1e-15
    # a lone carrier is the matrix itself
    _rec, _piv, car = _chain([mats[9]])
    assert np.array_equal(car, mats[9])


def test_diagonal_members_use_pivot_m00():
    rng = np.random.default_rng(78)
    ds = [_rz(t) for t in rng.uniform(0, 2 * np.pi, 8)]
    last = _fused(0.3, 1.1, 2.5)
    rec, piv, car = _chain(ds + [last], diag=[1] * 8 + [0])
    P = 1.0 + 0j
    for D, r, p in zip(ds, rec, piv):
        assert p == D[0, 0] and abs(abs(p) - 1) <= 1e-15
        assert list(r[:6]) == [1, 0, 0, 0, 0, 0]
        assert abs(p * (r[6] + 1j * r[7]) - D[1, 1]) <= 1e-15
        P *= p
    assert np.abs(car - P * last).max() <= 1e-15
