"""The matrix builder's angle-map instantiations (k_build_matrices_map, k_build_matrices_product_map: angles formed on
the fly from the leaves, qmle_run_batch_map from 64 samples on) against the table instantiations and against the
complex128 oracle, for every gate kind, every form of a build item and every row rule.

  (a) k_build_angles alone against tests/angle_map_reference.py: unreduced entries bit for bit, reduced entries within
      one float32 ulp (the compiler may fuse the multiply-subtract of the reduction); 1, 3 and 8 leaves, a NULL leaf,
      slots of 0, 1 and 5 terms, divisors and moduli that are no powers of two, a zipped pair, batch offsets below, at,
      across and beyond 2^32, slots exactly at +-period (not reduced).
  (b) every gate kind through the map with the state in the LDS (5 qubits): fused 2x2 items of several gates, 4x4 items
      with 2x2 sources on the first and on the second wire, Rot, constant matrices; a Golomb tape on the table route.
  (c) chains of unit-pivot records and product-form groups through the map (16 qubits, at most 130 states).
  (d) the ansatz zoo through Model.__call__.

In (b) and (c) three results must be the same bits, states and <Z> of every wire: plan.run_map, plan.run on the table of
N.build_angles, and plan.run on the first 63 rows of that table (the table instantiation below one wave per item).
Sampled rows also match the oracle fed the reference table.  Every case asserts `matrices_from_map_last_run` from the
report of the plan that ran: true on the map route, false on every table route -- a silent fall-back to the table
would otherwise let the whole file pass.

What (c) cannot hold: the measuring walk from the last group's registers (_assert_product_walk of
tests/test_gpu_group_product_form.py) needs 5120 workgroups, 160 states at 10-bit tiles; at 130 states and fewer the
same product-form groups run in k_tile2 one tile per workgroup.  (c) therefore asserts what the matrix builder is
about: the groups marked, `group_product_form_last_run`, the unit-form ops and their carriers, per stage.

Gate kinds the planner never admits to a chain or a product-form group: CRX, CRY, CRZ, CPhase (assign_unit_forms takes
uncontrolled one-qubit operators only).  The report of the `controlled` variant shows it: their fast ops carry
controlled dispatch codes (4..15 dense, 20..31 diagonal), none of them is listed in `unit_form_ops`, and the group that
holds them is not marked in `product_form_groups`.  They reach the map instantiation as ordinary 2x2 items, in (b), in
(c) and in (d)."""
import functools
import warnings

import numpy as np
import pytest

from oracle import circuits as OC
from oracle import einsum_sim as OE
from tests import angle_map_reference as R
from tests.helpers import N_PARAMS, ONE_Q, THREE_Q, TWO_Q, oracle_tape, tape_to_native
from tests.test_angle_map_reference_cpu import make_model, zoo, zoo_arguments
from tests.test_gpu_group_product_form import N_Q, SPECIAL, VARIANTS
from tests.test_gpu_group_product_form import tape as product_tape
from tests.test_gpu_measure_in_registers import TOL, _rows
from tests.test_measure_in_registers_cpu import ALL_LIVE, fuzz_struct

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FOUR_PI = R.FOUR_PI
BATCHES = (64, 65, 130)
B_MAX = 130


class _NullLeaf:
    """A leaf without elements (the parameters of an ansatz that has none): a NULL pointer, stride 0."""

    @staticmethod
    def data_ptr():
        return 0


def _dev(leaves):
    return [_NullLeaf() if l is None else torch.from_numpy(np.ascontiguousarray(l, dtype=np.float32)).cuda()
            for l in leaves]


def _from_map(plan, meas):
    return plan.executed(meas).describe()["stages"][-1]["matrices_from_map_last_run"]


def _assert_table(got, want, mask, what):
    """Unreduced entries bit for bit, reduced entries within one float32 ulp; -> number of entries an ulp off."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    same = got.view(np.int32) == want.view(np.int32)
    assert same[~mask].all(), (what, "an unreduced entry differs", np.argwhere(~same & ~mask)[:4])
    ulps = R.ulp_distance(got, want)
    assert ulps.max(initial=0) <= 1, (what, "a reduced entry is off by", int(ulps.max()))
    off = int((ulps > 0).sum())
    print(what, "entries", got.size, "reduced", int(mask.sum()), "an ulp off the reference", off)
    return off


# ---------------------------------------------------------------------------------------------------------------
# (a) the table kernel alone
# ---------------------------------------------------------------------------------------------------------------
def _split_exact(v):
    """Three float32 whose float64 sum, taken in order, is the double v exactly."""
    hi = np.float32(v)
    mid = np.float32(np.float64(v) - np.float64(hi))
    lo = np.float32(np.float64(v) - np.float64(hi) - np.float64(mid))
    assert np.float64(hi) + np.float64(mid) + np.float64(lo) == np.float64(v)
    return hi, mid, lo


@functools.lru_cache(maxsize=None)
def _case_a(n_leaves):
    """-> (map, leaves, strides, divs, mods, slots at +per and -per).  Coefficients +-3^k, k = 0..7, leaves in +-5.
    3 leaves: moduli 7, 5, 3 under divisors 1, 7, 35.  8 leaves: those, a NULL leaf with stride 0, a zipped pair
    (divisor 1, equal moduli), a broadcast leaf that holds the boundary terms and one more broadcast leaf.
    1 leaf: one row per sample."""
    rng = np.random.default_rng(5100 + n_leaves)
    if n_leaves == 1:
        widths, divs, mods = [6], [1], [B_MAX]
    else:
        widths, divs, mods = [4, 3, 2], [1, 7, 35], [7, 5, 3]
    if n_leaves == 8:
        widths, divs, mods = widths + [0, 2, 2, 2, 1], divs + [1, 1, 1, 1, 1], mods + [1, B_MAX, B_MAX, 1, 1]
    usable = [k for k, w in enumerate(widths) if w and not (n_leaves == 8 and k == 6)]
    leaves = [None if w == 0 else rng.uniform(-5.0, 5.0, (mods[k], w)).astype(np.float32)
              for k, w in enumerate(widths)]
    ptr, arg, idx, coef, const = [0], [], [], [], []

    def slot(n_terms, c):
        for j in range(n_terms):
            k = usable[(len(ptr) + j) % len(usable)]
            arg.append(k)
            idx.append(int(rng.integers(widths[k])))
            coef.append(float(3 ** int(rng.integers(0, 8))) * (1.0 if rng.random() < 0.5 else -1.0))
        const.append(c)
        ptr.append(len(arg))

    for n_terms in (0, 1, 5, 1, 2, 3, 1, 2, 3, 2, 1, 3):
        slot(n_terms, float(rng.uniform(-1.0, 1.0)))
    n_slots = len(const)
    period = np.full(n_slots, FOUR_PI)
    period[[1, 5]] = 0.0
    edge = ()
    if n_leaves == 8:  # two slots exactly at +per and -per on every row: const = hi, two terms of coefficient +-1
        hi, mid, lo = _split_exact(FOUR_PI)
        leaves[6] = np.array([[mid, lo]], dtype=np.float32)
        for sign in (1.0, -1.0):
            arg.extend([6, 6]); idx.extend([0, 1]); coef.extend([sign, sign])
            const.append(sign * float(hi))
            ptr.append(len(arg))
        period = np.concatenate([period, [FOUR_PI, FOUR_PI]])
        edge = (n_slots, n_slots + 1)
    m = R.MapArrays(ptr, arg, idx, coef, const, period)
    for l in leaves:
        if l is not None:
            l.setflags(write=False)
    return m, leaves, widths, divs, mods, edge


OFFSETS_A = {"zero": 0, "last_32_bit": 2 ** 32 - B_MAX - 1, "across_2_32": 2 ** 32 - B_MAX // 2, "beyond": 2 ** 33 + 3}


@pytest.mark.parametrize("with_period", [True, False], ids=["periods", "no_periods"])
@pytest.mark.parametrize("offset", sorted(OFFSETS_A), ids=sorted(OFFSETS_A))
@pytest.mark.parametrize("n_leaves", [1, 3, 8])
def test_table_kernel_against_the_reference(n_leaves, offset, with_period):
    from qml_essentials_amd import _native as N

    m, leaves, strides, divs, mods, edge = _case_a(n_leaves)
    off = OFFSETS_A[offset]
    period = m.period if with_period else None
    want, mask = R.table(leaves, strides, divs, mods, m.ptr, m.arg, m.idx, m.coef, m.const, period, B_MAX, off)
    d = m.device()
    got = N.build_angles(_dev(leaves), strides, divs, mods, *d[:5], m.n_slots, B_MAX, off,
                         d_period=d[5] if with_period else None).cpu().numpy()
    _assert_table(got, want, mask, f"(a) leaves={n_leaves} offset={offset} periods={with_period}")
    if with_period:
        periodic = m.period > 0
        assert not mask[:, ~periodic].any()
        share = mask[:, periodic].mean()
        print("(a) reduced share of the periodic slots", share)
        assert share > 0.5, share
        for s, sign in zip(edge, (1.0, -1.0)):  # exactly at +-per: stays
            assert not mask[:, s].any() and (got[:, s] == np.float32(sign * FOUR_PI)).all(), (s, got[:3, s])
    else:
        assert not mask.any() and np.abs(got).max() > 1e3


def test_a_negative_batch_offset_is_refused():
    """It would wrap as an unsigned row: QMLE_ERR_INVALID_ARG from every entry point, before any launch."""
    from qml_essentials_amd import _native as N

    m, leaves, strides, divs, mods, _edge = _case_a(3)
    d, dl = m.device(), _dev(leaves)
    with pytest.raises(ValueError, match="invalid argument"):
        N.build_angles(dl, strides, divs, mods, *d[:5], m.n_slots, B_MAX, -1, d_period=d[5])
    ops, angles, consts = tape_to_native([("RX", [q % 2], (0.0,)) for q in range(m.n_slots)], 2)
    plan = N.Plan(ops, 2, len(angles), consts)
    args = m.args(3).set(dl, strides, divs, mods, -1)
    with pytest.raises(ValueError, match="invalid argument"):
        plan.run_map(args, B_MAX, "state")
    with pytest.raises(ValueError, match="invalid argument"):
        plan.run_map(args, B_MAX, "state", token=0)
    assert plan.run_map(args.set(dl, strides, divs, mods, 0), B_MAX, "state").shape == (B_MAX, 4)


# ---------------------------------------------------------------------------------------------------------------
# the three routes of (b) and (c)
# ---------------------------------------------------------------------------------------------------------------
def _three_routes(plan, m, leaves, strides, divs, mods, batch, offset, meas, wires, want_table, mask, what,
                  expect_map=True):
    """run_map, run on the built table, run on its first 63 rows: the same bits.  -> (result, table)."""
    from qml_essentials_amd import _native as N

    d, dl = m.device(), _dev(leaves)
    args = m.args(len(leaves)).set(dl, strides, divs, mods, offset)
    one = plan.run_map(args, batch, meas, wires)
    assert _from_map(plan, meas) is expect_map, (what, "run_map of", batch)
    table = N.build_angles(dl, strides, divs, mods, *d[:5], m.n_slots, batch, offset, d_period=d[5])
    _assert_table(table.cpu().numpy(), want_table[:batch], mask[:batch], what + " table")
    two = plan.run(table, meas, wires)
    assert _from_map(plan, meas) is False, (what, "run of a table")
    few = plan.run(table[:63].contiguous(), meas, wires)
    assert _from_map(plan, meas) is False
    assert torch.equal(one, two), (what, meas, "map and table differ", int((one != two).sum()))
    assert torch.equal(few, two[:63]), (what, meas, "63 rows alone differ")
    short = plan.run_map(args, 63, meas, wires)  # fewer than 64 samples: the call itself takes the table route
    assert _from_map(plan, meas) is False and torch.equal(short, few)
    return one, table


# ---------------------------------------------------------------------------------------------------------------
# (b) every gate kind, state in the LDS
# ---------------------------------------------------------------------------------------------------------------
N_B = 5


def _unitary(d, seed):
    rng = np.random.default_rng(seed)
    return np.linalg.qr(rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d)))[0].astype(np.complex64)


def _g(name, *wires):
    return (name, list(wires), (0.0,) * N_PARAMS.get(name, 0))


def _layer(name, n=N_B):
    return [_g(name, q) for q in range(n)]


TAPES_B = {
    # fused 2x2 items of two and three gates, a constant 2x2 among them; Rot alone and fused
    "one_qubit": [_g("H", 0), _g("RX", 0), _g("S", 0), _g("PauliX", 1), _g("RY", 1), _g("PauliZ", 1),
                  _g("PauliY", 2), _g("RZ", 2), ("Matrix", [2], (_unitary(2, 51),)), _g("Rot", 3), _g("S", 3), _g("H", 3),
                  _g("RX", 4), _g("RY", 4), _g("RZ", 4)]
                 + [_g("CX", q, (q + 1) % N_B) for q in range(N_B)] + _layer("Rot")
                 + [_g("CZ", 0, 2), _g("CY", 1, 3)] + _layer("RY"),
    # uncontrolled 4x4 gates take the one-qubit gates in front of them (take_pending) and behind them
    # (multiply_onto) as U (x) I / I (x) U sources: BuildOp::pad 1 (first wire) and 2 (second wire)
    "two_qubit": _layer("RY")
                 + [_g("RXX", 0, 1), _g("Rot", 0), _g("H", 1), _g("RYY", 2, 3), _g("S", 3), _g("RX", 2),
                    _g("CRX", 0, 2), _g("CRY", 1, 3), _g("CRZ", 2, 4), _g("CPhase", 3, 0),
                    _g("RZ", 1), _g("RZZ", 1, 2), _g("PauliY", 2), _g("RZX", 3, 4), _g("RX", 4), _g("Rot", 3),
                    _g("CX", 4, 0), _g("CY", 0, 1), _g("CZ", 1, 2),
                    _g("RX", 1), ("Matrix", [1, 3], (_unitary(4, 52),)), _g("RY", 3), _g("SWAP", 0, 4), _g("RZ", 0)]
                 + _layer("RY"),
    "three_qubit": _layer("H") + _layer("RX")
                   + [_g("CCX", 0, 1, 2), _g("RY", 2), _g("CSWAP", 3, 4, 0), _g("Rot", 0), _g("CCX", 4, 2, 1), _g("RZ", 1),
                      _g("CSWAP", 1, 0, 3)] + _layer("RX"),
    # the Golomb diagonal reads its angle in the pass itself: the call keeps the table route
    "golomb": _layer("RY") + [("Golomb", [], (0.0,))] + _layer("RX") + [_g("CX", q, (q + 1) % N_B) for q in range(N_B)],
}
# (batch, batch offset): the 32-bit row arithmetic of AngleMapSrc::small, its last case, a batch that crosses 2^32, 64 bits
SHAPES_B = [(64, 0), (65, 2 ** 32 - 65 - 1), (130, 2 ** 32 - 65), (130, 2 ** 33 + 3)]


def test_the_tapes_of_b_hold_every_gate_kind():
    from qml_essentials_amd import _native as N

    names = {name for t in TAPES_B.values() for name, _w, _p in t}
    assert names >= set(ONE_Q) | set(TWO_Q) | set(THREE_Q) | {"Matrix", "Golomb"}, sorted(names)
    dims = {np.asarray(p[0]).shape[0] for t in TAPES_B.values() for name, _w, p in t if name == "Matrix"}
    assert dims == {2, 4}, "a constant 2x2 (MAT1) and a constant 4x4 (MAT2)"

    def n_lowered(t):
        ops, angles, consts = tape_to_native(t, N_B)
        return N.Plan(ops, N_B, len(angles), consts).describe()["n_lowered"]

    # one build item each: three gates fused into a 2x2; a 4x4 with 2x2 sources in front of it and behind it, on
    # its first and on its second wire
    assert n_lowered([_g("H", 0), _g("RX", 0), _g("S", 0)]) == 1
    assert n_lowered([_g("RY", 0), _g("RY", 1), _g("RXX", 0, 1), _g("Rot", 0), _g("H", 1)]) == 1
    assert n_lowered([_g("RZX", 3, 4), _g("RX", 4), _g("Rot", 3)]) == 1


@functools.lru_cache(maxsize=None)
def _case_b(name):
    """The tape's plan arguments, an affine map with 3^7 on every third slot, leaves (one row per sample; moduli 7
    and 5 under divisors 1 and 7)."""
    template = TAPES_B[name]
    ops, angles, consts = tape_to_native(template, N_B)
    n_slots = len(angles)
    rng = np.random.default_rng(5200 + len(template))
    golomb = [sl[0] for op_name, _w, sl, _o in ops if op_name == "DIAG_ALL"]
    period = np.full(n_slots, FOUR_PI)
    period[golomb] = 0.0
    m = R.affine_map(n_slots, [6, 4, 3], rng, period, big=set(range(0, n_slots, 3)) - set(golomb))
    for s in golomb:
        # the pass evaluates marks * x in float32 like the reference (marks up to 1522 at 5 qubits): |x| <= 0.0045
        # keeps the phase below 7 rad and its rounding below 2.4e-7, so that the 1e-6 bar judges the route
        m.coef[m.ptr[s]:m.ptr[s + 1]] = 5e-4 / max(1, m.ptr[s + 1] - m.ptr[s])
        m.const[s] = 2e-3
    leaves = [rng.uniform(-5.0, 5.0, (rows, w)).astype(np.float32) for rows, w in ((B_MAX, 6), (7, 4), (5, 3))]
    return template, ops, n_slots, consts, m, leaves, [6, 4, 3], [1, 1, 7], [B_MAX, 7, 5]


def _fill(template, row):
    out, k = [], 0
    for name, wires, params in template:
        if name == "Matrix":
            out.append((name, wires, params))
            continue
        out.append((name, wires, tuple(float(x) for x in row[k:k + len(params)])))
        k += len(params)
    return out


@pytest.mark.parametrize("batch,offset", SHAPES_B, ids=[f"{b}-{i}" for i, (b, _o) in enumerate(SHAPES_B)])
@pytest.mark.parametrize("name", sorted(TAPES_B))
def test_every_gate_kind_through_the_map(name, batch, offset):
    from qml_essentials_amd import _native as N

    template, ops, n_slots, consts, m, leaves, strides, divs, mods = _case_b(name)
    plan = N.Plan(ops, N_B, n_slots, consts)
    assert plan.describe()["whole_state_lds"]
    want_table, mask = m.table(leaves, strides, divs, mods, batch, offset)
    assert mask.any() and np.abs(want_table).max() <= 4.0 * np.pi
    wires = list(range(N_B))
    expect_map = name != "golomb"
    state, _t = _three_routes(plan, m, leaves, strides, divs, mods, batch, offset, "state", (), want_table, mask,
                              f"(b) {name} {batch}", expect_map)
    z, _t = _three_routes(plan, m, leaves, strides, divs, mods, batch, offset, "expval", wires, want_table, mask,
                          f"(b) {name} {batch}", expect_map)
    state, z = state.cpu().numpy().astype(np.complex128), z.cpu().numpy().astype(np.float64)
    worst_s = worst_z = 0.0
    for r in _rows(batch):
        t = oracle_tape(_fill(template, want_table[r].astype(np.float64)), N_B)
        ws = np.asarray(OE.simulate_and_measure(t, N_B, "state", (), np.complex128)).reshape(-1)
        wz = np.asarray(OE.simulate_and_measure(t, N_B, "expval", [("PauliZ", [q]) for q in wires], np.complex128))
        worst_s, worst_z = max(worst_s, np.abs(state[r] - ws).max()), max(worst_z, np.abs(z[r] - wz).max())
    print(f"(b) {name} {batch} offset {offset}: worst |amplitude err| {worst_s:.3e}, worst |<Z> err| {worst_z:.3e}")
    assert worst_s <= 1e-6 and worst_z <= TOL, (worst_s, worst_z)


# ---------------------------------------------------------------------------------------------------------------
# (c) chains and product-form groups, 16 qubits
# ---------------------------------------------------------------------------------------------------------------
THETA_C = {"RY": 0, "RX": 0, "Rot": 1, "CRX": 0, "CRY": 0}  # the angle that sets c and s (the product form's cases)


def _P(pos):
    return N_Q - 1 - pos


def _kinds_tape():
    """`both` with its four RY (the front product-form group, positions 4..7) replaced by H RX | S RY | Y RZ RY | RX:
    each a fused 2x2 item, so the group stays four ops and stays in product form."""
    new = {4: ["H", "RX"], 5: ["S", "RY"], 6: ["PauliY", "RZ", "RY"], 7: ["RX"]}
    out = []
    for g, w in product_tape("both", 10):
        out += [(h, list(w)) for h in new[_P(w[0])]] if g == "RY" else [(g, w)]
    return out


def _controlled_tape():
    """`last` with the three CZ of position 7 replaced by CRY, CRZ and CPhase."""
    it = iter(["CRY", "CRZ", "CPhase"])
    return [(next(it), w) if g == "CZ" and w[0] == _P(7) else (g, w) for g, w in product_tape("last", 10)]


# name: (struct, plan flags, marks of the last stage's groups or None, last group by lane swaps, crossed)
def _cases_c():
    from qml_essentials_amd import _native as N

    hand = ALL_LIVE | N.PLAN_TAPE_ORDER | N.plan_flags(tile_bits=10)
    cases = {name: (product_tape(name, 10), hand, *VARIANTS[name][2:]) for name in VARIANTS}
    cases["kinds"] = (_kinds_tape(), hand, [True, True], True, False)
    cases["controlled"] = (_controlled_tape(), hand, [False, True], True, False)
    cases["four_waves"] = (product_tape("three_and_four", 12), ALL_LIVE | N.PLAN_TAPE_ORDER | N.plan_flags(tile_bits=12),
                           *VARIANTS["three_and_four"][2:])
    # the chain tapes of tests/test_gpu_unit_form_gates.py: storing stages with chains (10-bit tiles), and the default
    # geometry's group that mixes unit forms with every other kind of gate
    for seed in (3, 13):
        cases[f"fuzz{seed}"] = (fuzz_struct(seed, N_Q), ALL_LIVE | N.plan_flags(tile_bits=10), None, None, None)
    cases["fuzz42"] = (fuzz_struct(42, N_Q), ALL_LIVE, None, None, None)
    return cases


CASES_C = ("both", "front", "front_crossed", "last", "last_diagonal", "crx", "three_and_four", "kinds", "controlled",
           "four_waves", "fuzz3", "fuzz13", "fuzz42")


def _to_ops(struct):
    ops, k = [], 0
    for g, wires in struct:
        npar = N_PARAMS.get(g, 0)
        ops.append((g, list(wires), list(range(k, k + npar)), -1))
        k += npar
    return ops, k


@functools.lru_cache(maxsize=None)
def _case_c(name):
    """Leaf 0 holds one row of angles per sample (rows 1..4: all angles 0, then pi, 2.2, pi / 2 on every rotation angle)
    and enters with coefficient 1; leaf 1 (modulus 7) is zero on its rows 1..4 and enters every third slot with +-3^7:
    the samples b with b % 7 in {0, 5, 6} have sums of about 1e4 rad there, the special rows keep their angles exactly."""
    struct, flags, marks, swap, crossed = _cases_c()[name]
    ops, n_slots = _to_ops(struct)
    rng = np.random.default_rng(5300 + len(struct) + n_slots)
    ang = rng.uniform(0, 2 * np.pi, (B_MAX, n_slots)).astype(np.float32)
    for row, theta in SPECIAL:
        ang[row] = 0.0
        k = 0
        for g, _w in struct:
            if g in THETA_C:
                ang[row, k + THETA_C[g]] = theta
            k += N_PARAMS.get(g, 0)
    shared = rng.uniform(-5.0, 5.0, (7, 4)).astype(np.float32)
    shared[1:5] = 0.0
    ptr, arg, idx, coef = [0], [], [], []
    for s in range(n_slots):
        arg.append(0); idx.append(s); coef.append(1.0)
        if s % 3 == 0:
            arg.append(1); idx.append(s % 4); coef.append(float(3 ** 7) * (1.0 if s % 2 else -1.0))
        ptr.append(len(arg))
    m = R.MapArrays(ptr, arg, idx, coef, np.zeros(n_slots), np.full(n_slots, FOUR_PI))
    leaves, strides, divs, mods = [ang, shared], [n_slots, 4], [1, 1], [B_MAX, 7]
    want_table, mask = m.table(leaves, strides, divs, mods, B_MAX, 0)
    for row, _theta in SPECIAL:
        assert np.array_equal(want_table[row], ang[row])
    assert np.abs(R.sums(leaves, strides, divs, mods, m.ptr, m.arg, m.idx, m.coef, m.const, B_MAX, 0)).max() > 5e3
    return struct, flags, marks, swap, crossed, ops, n_slots, m, leaves, strides, divs, mods, want_table, mask


@functools.lru_cache(maxsize=None)
def _oracle_c(name, row):
    struct, want_table = _case_c(name)[0], _case_c(name)[12]
    t, k = [], 0
    for g, wires in struct:
        p = N_PARAMS.get(g, 0)
        t.append((g, list(wires), tuple(float(x) for x in want_table[row, k:k + p])))
        k += p
    state = np.asarray(OE.simulate_and_measure(t, N_Q, "state", (), np.complex128)).reshape(-1)
    z = np.asarray(OE.simulate_and_measure(t, N_Q, "expval", [("PauliZ", [q]) for q in range(N_Q)], np.complex128))
    return state, z


def _assert_forms_ran(name, desc, marks, swap, crossed):
    """From the report of the plan that ran: unit-form chains with their carriers, the groups marked for the product
    form, and that the stage's last launch took that form."""
    stages = [s for s in desc["stages"] if s["kind"] == "tile" and s["fast"]]
    assert stages and any(s["unit_form_ops"] and s["scale_carriers"] for s in stages), name
    marked = [s for s in stages if any(s["product_form_groups"])]
    assert marked, name
    for s in marked:
        assert s["group_product_form_last_run"] is True, name
    last = desc["stages"][-1]
    if marks is not None:
        assert last["kind"] == "tile" and last["fast"] and last["T"] in (10, 12)
        assert last["product_form_groups"] == marks, last["product_form_groups"]
        assert last["group_product_form_last_run"] is True
        assert last["last_group_lane_swap"] is swap
        if swap:
            assert last["lane_swap_crossed"] is crossed
    if name == "kinds":
        assert [g["n_ops"] for g in last["fast_groups"]] == [4, 2] and last["unit_form_ops"] == [0, 1, 2, 3, 4]
    if name == "controlled":  # the report that shows CRY / CRZ / CPhase outside every chain and product-form group
        codes = [c for c, _o in last["fast_ops"]]
        ctrl = [i for i, c in enumerate(codes) if 4 <= c < 16 or 20 <= c < 32]
        assert len(ctrl) == 3 and not set(ctrl) & (set(last["unit_form_ops"]) | set(last["scale_carriers"]))
        assert all(i < last["fast_groups"][0]["n_ops"] for i in ctrl) and last["product_form_groups"][0] is False


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", CASES_C)
def test_chains_and_product_form_groups_through_the_map(name, batch):
    from qml_essentials_amd import _native as N

    struct, flags, marks, swap, crossed, ops, n_slots, m, leaves, strides, divs, mods, want_table, mask = _case_c(name)
    plan = N.Plan(ops, N_Q, n_slots, flags=flags)
    wires = list(range(N_Q))
    rows = sorted(set(_rows(batch)) | {3, 4})
    what = f"(c) {name} {batch}"
    z, _t = _three_routes(plan, m, leaves, strides, divs, mods, batch, 0, "expval", wires, want_table, mask, what)
    z_rows = z[rows].cpu().numpy().astype(np.float64)
    del z
    plan.run_map(m.args(2).set(_dev(leaves), strides, divs, mods, 0), batch, "expval", wires)
    assert _from_map(plan, "expval") is True
    _assert_forms_ran(name, plan.executed("expval").describe(), marks, swap, crossed)
    state, _t = _three_routes(plan, m, leaves, strides, divs, mods, batch, 0, "state", (), want_table, mask, what)
    s_rows = state[rows].cpu().numpy().astype(np.complex128)
    del state
    plan.run_map(m.args(2).set(_dev(leaves), strides, divs, mods, 0), batch, "state")
    assert _from_map(plan, "state") is True
    _assert_forms_ran(name, plan.executed("state").describe(), marks, swap, crossed)
    worst_s = worst_z = 0.0
    for i, r in enumerate(rows):
        ws, wz = _oracle_c(name, r)
        worst_s, worst_z = max(worst_s, np.abs(s_rows[i] - ws).max()), max(worst_z, np.abs(z_rows[i] - wz).max())
    print(f"{what}: worst |amplitude err| {worst_s:.3e}, worst |<Z> err| {worst_z:.3e}")
    assert worst_s <= 1e-6 and worst_z <= TOL, (worst_s, worst_z)


# ---------------------------------------------------------------------------------------------------------------
# (d) the ansatz zoo through Model.__call__
# ---------------------------------------------------------------------------------------------------------------
ZOO_TOL = 2e-6  # the bar of tests/test_gpu_model.py::test_large_encoding_angles_keep_float32_accuracy


def _zoo_spec(kw):
    if "encoding" in kw:
        strategy, gates = kw["encoding"]
        return OC.ModelSpec(4, 1, kw["circuit_type"], encoding=gates, strategy=strategy)
    return OC.ModelSpec(4, 1, kw["circuit_type"])


def _zoo_case(model, spec, p, x, zipped):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert model.host_arrays_via_device is True
        dev = np.asarray(model(params=p, inputs=x))
        calls = list(model.script._compiled.values())
        assert len(calls) == 1
        plan = calls[0].plan
        assert _from_map(plan, "expval") is True, "the default route of 72 samples builds its matrices from the map"
        model.host_arrays_via_device = False
        host = np.asarray(model(params=p, inputs=x))
        assert _from_map(plan, "expval") is False, "the host's angle table"
    assert dev.shape == host.shape
    d = np.abs(dev - host).max()
    n_p = 1 if 0 in model.params.shape else p.shape[0]
    dev = dev.reshape(72, 4)
    worst = 0.0
    for b in (0, 1, 35, 36, 70, 71):
        i, j = (b, b) if zipped else (b // n_p, b % n_p)
        t = OC.model_tape(spec, np.asarray(p[min(j, p.shape[0] - 1)], dtype=np.float64), x[i].astype(np.float64),
                          zero_inputs_batch1=False)
        want = OE.simulate_and_measure(t, 4, "expval", [("PauliZ", [q]) for q in range(4)], np.complex128)
        worst = max(worst, np.abs(dev[b] - np.asarray(want)).max())
    print(f"(d) {spec.ansatz} {spec.strategy}: map route vs host table {d:.3e}, worst |<Z> err| vs oracle {worst:.3e}")
    assert d <= ZOO_TOL and worst <= ZOO_TOL, (d, worst)


@pytest.mark.parametrize("name,kw", zoo(), ids=[n for n, _ in zoo()])
def test_the_ansatz_zoo_on_the_map_route(name, kw):
    model = make_model(kw)
    p, x = zoo_arguments(model, 8, 9, seed=7100)
    _zoo_case(model, _zoo_spec(kw), p, x, zipped=False)


def test_zipped_batch_axes_on_the_map_route():
    kw = dict(circuit_type="Circuit_19")
    model = make_model(kw, repeat_batch_axis=[False, True, True])
    p, x = zoo_arguments(model, 72, 72, seed=7200)
    _zoo_case(model, _zoo_spec(kw), p, x, zipped=True)
