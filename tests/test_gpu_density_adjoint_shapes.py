"""The adjoint sweep over vec(rho) (``adjoint.density_gradient``: ``k_dens_fwd``, ``k_dens_bwd``, the two seed kernels
and ``k_adj_final`` behind them) at every launch shape, wire position and seed, against the factorised exact gradient of
tests/density_factorised_reference.py -- the full 4^n reference of tests/test_gpu_density_adjoint.py stops at n = 8.

Launch shapes of a step on n system wires (``dens_blocks``: 4^n / 2^NB work items, 1024 per workgroup, at most 1024
workgroups; NB = 2 for a one-wire step, 4 for a two-wire step):

    n = 6   one-wire: one workgroup, four grid-stride rounds
    n = 7   one-wire: 4 partial sums per row;  two-wire: one workgroup, four rounds
    n = 8   two-wire: 4 partials (one-wire: 16)
    n = 10  one-wire: 256 partials, the 256-thread finish;  two-wire: 64
    n = 11  one-wire: exactly 1024 workgroups;  two-wire: 256 partials
    n = 12  one-wire: 4096 wanted, the grid capped at 1024: the grid-stride loop

At each size steps sit on wire n - 1 (bit position 0: the float4 loads in complex64), on wire 0 (the highest positions)
and on a middle wire; two-wire steps on (n - 2, n - 1) and (n - 1, 0) in both orders and on (0, n / 2).

Bounds, in the metric max |sweep - reference| / max(1, sum |w|) per row: complex128 1e-12; complex64
max(``routes_tolerance(2 n)``, 4 x the factorised complex64 floor) -- ``routes_tolerance`` is 1e-5 from 14 doubled wires
on, and that figure is carried upward to n = 10, 11, 12.  Every case prints the error it reached per step width, with
the partial count of that width (``-s``); profiles/density_adjoint.md keeps the table.

tests/test_density_factorised_reference_cpu.py checks, without a GPU, for every tape and observable set used here that no
wire sits in a basis state, that every differentiated entry is visible and that the wrong adjoint rules are 100 bars
away.  Not covered: channels on three or four wires (refused by the sweep), per-sample matrices, and the
``Script.vjp`` / ``Model.gradient`` front ends at these sizes (checked at small n; they add no kernel route)."""
import functools

import numpy as np
import pytest

from qml_essentials_amd import _native as N
from qml_essentials_amd import adjoint

import density_adjoint_reference as DR
import density_factorised_reference as F
import noise_reference as NR
import test_gpu_density_adjoint as G

pytestmark = pytest.mark.gpu

SHAPE_SIZES = (6, 7, 8, 10, 11, 12)
KINDS = ("CRZ", "CPhase", "RZZ", "CRX", "CRY", "RXX", "RYY", "RZX")  # diagonal kinds first: a later gate turns their
CHANNELS = ("amp", "pair", "phase", None, "bitflip", "depol", "phaseflip")  # angle into something a Z seed sees


def batch_of(key):
    return 1 if key[0] == "shape" and key[1] >= 11 else 2


def blocks(n, nb):
    """``dens_blocks`` of csrc/qmle_density_dev.h: workgroups per state = partial sums per row."""
    return int(min(1024, max(1, (4**n >> nb) + 1023 >> 10)))


# ---- tapes: key -> (steps, clusters, wires the observables sit on) ---------------------------------------------------
def layout(key):
    kind, n = key[0], key[1]
    if kind == "shape":
        a, b, m = n - 2, n - 1, n // 2
        if key[2] == "ends":
            steps = [("RX", (b,), "amp"), ("RY", (0,), "depol"), ("RY", (m,), "phase")]
            if n < 12:
                steps += [("CRX", (a, b), "amp"), ("RXX", (b, a), "pair"), ("CRY", (b, 0), "bitflip"), ("RZX", (0, b), None)]
            return steps, [[0, a, b], [m - 1, m]], [b, 0, m, a]
        return [("RYY", (0, m), "amp"), ("RX", (b,), None)], [[0, m], [a, b]], [0, m, b]
    if kind == "kinds":
        # shallow groups: the gradient of a group's first angle passes through every later channel of the group
        clusters = {7: [[0, 6], [1, 5], [2, 4], [3]], 8: [[0, 7], [1, 6], [2, 5], [3, 4]]}[n]
        pairs = [tuple(c) for c in clusters if len(c) == 2]
        steps = [("RZ", (3,), "amp"), ("RX", (n - 1,), "phase"), ("RY", (0,), "bitflip"), ("Rot", (1,), "depol"),
                 ("RX", (2,), None), ("RY", (clusters[-1][-1],), "phaseflip")]
        for i in range(2 * len(KINDS)):  # every kind once with its first wire the lower one, once the higher one
            lo, hi = sorted(pairs[i % len(pairs)])
            steps.append((KINDS[i // 2], (hi, lo) if i % 2 else (lo, hi), CHANNELS[i % len(CHANNELS)]))
        return steps, clusters, list(range(n))
    if kind == "terms":  # n = 4: the full reference is at hand
        return ([("CRX", (3, 0), "amp"), ("RYY", (1, 2), "pair"), ("Rot", (2,), "depol"), ("RZX", (0, 3), None)],
                [[0, 3], [1, 2]], [0, 1, 2, 3])
    if kind == "small":  # the CPU comparison with the full reference
        return {(4, 0): ([("CRY", (0, 1), "phase"), ("RXX", (3, 2), "amp"), ("RZ", (1,), "bitflip"), ("RX", (2,), None)],
                         [[0, 1], [2, 3]]),
                (5, 0): ([("CRX", (0, 1), "amp"), ("RZX", (4, 2), "pair"), ("Rot", (3,), "depol"), ("RYY", (2, 3), None)],
                         [[0, 1], [2, 3, 4]]),
                (5, 1): ([("CRY", (4, 0), "phase"), ("RXX", (1, 3), "amp"), ("RZ", (2,), "bitflip"),
                          ("CPhase", (3, 2), "pair"), ("CRZ", (0, 4), None), ("RX", (4,), "depol")],
                         [[0, 4], [1, 2, 3]])}[key[1:]] + (list(range(n)),)
    raise KeyError(key)


# Seeds of the tapes' angles, as ``PYTHONPATH=. python tests/test_density_factorised_reference_cpu.py`` finds and prints
# them under the three conditions of that file, for every observable set and row of weights used with the tape here.
# An int (``find_seed``): the first of 0, 1, 2, .. that serves when every group takes it.  A tuple (``find_seeds``, the
# kinds tapes, whose groups carry too many angles for one seed to serve them all): one seed per group -- a group's
# angles depend on its own seed alone -- group by group the first that serves.  A tape without an entry takes 0.
SEEDS = {("shape", 6, "ends"): 37, ("shape", 6, "mid"): 0, ("shape", 7, "ends"): 78, ("shape", 7, "mid"): 73,
         ("shape", 8, "ends"): 69, ("shape", 8, "mid"): 58, ("shape", 10, "ends"): 102, ("shape", 10, "mid"): 9,
         ("shape", 11, "ends"): 5, ("shape", 11, "mid"): 2, ("shape", 12, "ends"): 10, ("terms", 4): 9,
         ("kinds", 7, "all"): (20, 551, 61, 0), ("kinds", 8, "all"): (1, 2, 2, 3), ("kinds", 7, "z32"): (10, 12, 2, 0),
         ("kinds", 7, "rows"): (635, 34, 9, 0), ("kinds", 7, "words"): (14, 1, 0, 1)}


class Built:
    def __init__(self, key, seed):
        steps, clusters, self.obs_wires = layout(key)
        self.key, self.n, self.B = key, key[1], batch_of(key)
        self.groups = F.fill_groups(self.n, clusters)
        self.seeds = tuple(seed) if isinstance(seed, tuple) else (int(seed or 0),) * len(self.groups)
        assert len(self.seeds) == len(self.groups)
        rngs = [np.random.default_rng([s, k, self.n, sum(map(ord, key[0] + str(key[2:])))]) for k, s in enumerate(self.seeds)]
        self.tape, self.wanted = F.factorised_tape(self.n, self.groups, steps, rngs, self.B)
        # per wanted slot: the amplitudes its step holds in registers (4: a one-wire step, 16: a two-wire step)
        self.width = [w for g, wires, _c in steps for w in [4 if len(wires) == 1 else 16] * (3 if g == "Rot" else 1)]


@functools.lru_cache(maxsize=None)
def built(key):
    return Built(key, SEEDS.get(key))


# ---- observable sets -------------------------------------------------------------------------------------------------
def _m(*wires):
    return sum(1 << w for w in wires)


def observable_set(name, bt):
    """-> (Z groups | None, Pauli terms | None): what ``adjoint.density_gradient`` takes"""
    W, n = bt.obs_wires, bt.n
    if name == "z":  # every wire of interest alone, two of them, all of them
        return [[w] for w in W] + [[W[0], W[1]], list(W)], None
    if name == "pauli":  # X and Y on every wire of interest, and a Hermitian on two of them
        a, b = _m(W[0]), _m(W[1])
        terms = [t for i, w in enumerate(W) for t in ((1.0, _m(w), 0, 2 * i), (1.0, _m(w), _m(w), 2 * i + 1))]
        col = 2 * len(W)
        return None, terms + [(0.4, a, 0, col), (-0.7, b, 0, col), (0.5, a | b, a | b, col), (0.3, 0, a | b, col)]
    if name == "z32":  # n = 7: a middle wire, a parity across three groups, the whole register, QMLE_MAX_QUBITS groups
        assert n == 7
        groups = ([[3], [0, 1, 2], list(range(7))] + [[w] for w in range(7)] + [[w, (w + 3) % 7] for w in range(7)]
                  + [[w, (w + 1) % 7, (w + 2) % 7] for w in range(7)] + [[v for v in range(7) if v != w] for w in range(7)]
                  + [[1, 5]])
        assert len(groups) == N.MAX_QUBITS
        return groups, None
    if name == "words":  # n = 7
        assert n == 7
        return None, [(1.0, _m(1, 3, 5), _m(1, 3, 5), 0),                       # Y Y Y: the phase i^3
                      (1.0, _m(0, 6), _m(0, 6), 1),                             # Y Y: i^2
                      (0.8, 0, 0, 2), (0.9, _m(4), _m(2), 2),                   # the identity (gradient exactly 0), Z_2 X_4
                      (1.0, _m(2, 3), _m(3, 4), 3),                             # X_2 Y_3 Z_4 on the middle wires
                      (0.6, _m(2), 0, 4), (-0.4, _m(2), _m(4), 4), (0.7, _m(2), _m(2), 4),  # X_2, X_2 Z_4, Y_2: ONE entry
                      (0.3, _m(2), _m(0, 6), 4),                                             # per row of Lambda, and X_2 Z_0 Z_6
                      (0.9, _m(1), 0, 5), (-0.6, 0, _m(5), 5), (0.5, _m(6), 0, 5), (0.7, _m(3), 0, 5), (0.4, 0, _m(0), 5)]  # (X_3: the last RY on wire 3 commutes with Y_3)
    if name in ("terms96", "terms97"):  # n = 4: kDensMaxSeedTerms distinct words over four columns, and one more
        rng = np.random.default_rng(96)
        words = rng.permutation(256)[:int(name[5:])]
        return None, [(float(c), int(v) >> 4, int(v) & 15, t % 4) for t, (v, c) in
                      enumerate(zip(words, rng.uniform(-1.0, 1.0, size=len(words))))]
    raise KeyError(name)


def reference_observables(name, bt):
    groups, terms = observable_set(name, bt)
    return F.z_observables(groups) if terms is None else F.pauli_observables(terms)


def reference_for(bt, obs_name, row, full=False):
    """-> (Jacobian in complex128, the same evaluation in complex64), factorised, or (``full``) on the 4^n matrix"""
    obs = reference_observables(obs_name, bt)
    if full:
        ot, Ls = NR.reference_tape(bt.tape, row), F.full_cost_matrices(bt.n, obs)
        ref = DR.shift_jacobian(ot, bt.n, Ls, set(bt.wanted))
        c64 = DR.shift_jacobian(ot, bt.n, Ls, set(bt.wanted), dtype=np.complex64)
    else:
        ref = F.jacobian(bt.tape, bt.groups, row, obs, bt.wanted)[1]
        c64 = F.jacobian(bt.tape, bt.groups, row, obs, bt.wanted, dtype=np.complex64)[1]
    ref.flags.writeable = c64.flags.writeable = False
    return ref, c64


@functools.lru_cache(maxsize=None)
def reference(key, obs_name, row):
    return reference_for(built(key), obs_name, row, full=key[0] == "terms")


def bar(n, x64, floor=0.0):
    """complex64 from n = 10 on: max(1e-5, 4 x floor) -- ``routes_tolerance`` past 13 doubled wires, carried upward"""
    return 1e-12 if x64 else max(G.routes_tolerance(2 * n, False), 4.0 * floor)


def n_columns(obs_name, bt):
    return len(reference_observables(obs_name, bt))


# (name, tape key, observable set, cotangents per sample, seed of the weights): what the GPU tests below run, each in
# both precisions unless it says otherwise; tests/test_density_factorised_reference_cpu.py walks the same list
def _cases():
    for n in SHAPE_SIZES:
        for which in ("ends", "mid") if n < 12 else ("ends",):
            for obs in ("z", "pauli"):
                yield f"shape n={n} {which}", ("shape", n, which), obs, 1, 100 + n
    for n in (7, 8):
        for obs in ("z", "pauli"):
            yield f"kinds n={n}", ("kinds", n, "all"), obs, 1, 200 + n
    # (the same steps with angles of their own: a tape then has to meet the conditions for its own rows of weights only)
    yield "seed z32", ("kinds", 7, "z32"), "z32", 1, 301
    yield "seed words", ("kinds", 7, "words"), "words", 1, 302
    yield "seed terms96", ("terms", 4), "terms96", 1, 303
    yield "rows K=3", ("kinds", 7, "rows"), "z", 3, 304


CASES = list(_cases())


def case_weights(obs_name, bt, K, wseed):
    return G.weights(n_columns(obs_name, bt), K * bt.B, wseed)


# ---- the sweep and the comparison --------------------------------------------------------------------------------------
def sweep(bt, obs_name, w, x64):
    groups, terms = observable_set(obs_name, bt)
    want = [k in set(bt.wanted) for k in range(G.n_slots(bt.tape))]
    sw = adjoint.plan_density(bt.tape.ops, bt.n, want)
    assert len(sw.steps) == len(bt.wanted) and sw.checkpoints == len(bt.wanted) + 1
    assert [4 if s[1][1] < 0 else 16 for s in sw.steps] == bt.width
    with G.x64_scope(x64):
        return adjoint.density_gradient(bt.tape.ops, bt.n, bt.B, groups, w, want, x64=x64, obs_terms=terms)


def compare(name, bt, obs_name, got, w, x64):
    """Row r of ``got`` / ``w`` is sample r % B.  Prints, per step width, the partial count and the largest error with
    its bar; -> the largest error."""
    wanted, width = list(bt.wanted), np.array(bt.width)
    assert got.shape == (w.shape[0], G.n_slots(bt.tape))
    worst = {}
    for r in range(got.shape[0]):
        ref, c64 = reference(bt.key, obs_name, r % bt.B)
        scale = max(1.0, float(np.abs(w[r]).sum()))
        tol = bar(bt.n, x64, float(np.abs(w[r] @ c64 - w[r] @ ref).max()) / scale)
        err = np.abs(got[r] - w[r] @ ref)[wanted] / scale
        for nb in sorted(set(bt.width)):
            e = float(err[width == nb].max())
            worst[nb] = max(worst.get(nb, (0.0, 0.0)), (e, tol))
        assert err.max() <= tol, (name, obs_name, r, float(err.max()), tol)
        unwanted = [k for k in range(got.shape[1]) if k not in set(wanted)]
        assert not np.any(got[r, unwanted]), (name, "columns that are not wanted must be exactly zero")
    for nb, (e, tol) in worst.items():
        print(f"{name} | {obs_name} | {'x64' if x64 else 'c64'} | n {bt.n} | {'one' if nb == 4 else 'two'}-wire step | "
              f"partials {blocks(bt.n, 2 if nb == 4 else 4)} | error {e:.2e} | bar {tol:.1e}")
    return max(e for e, _t in worst.values())


def run_case(name, key, obs_name, K, wseed, x64):
    bt = built(key)
    w = case_weights(obs_name, bt, K, wseed)
    got = sweep(bt, obs_name, w, x64)
    assert got.shape[0] == K * bt.B
    return compare(name, bt, obs_name, got, w, x64)


def _named(prefix):
    return [c for c in CASES if c[0].startswith(prefix)]


# n = 12: complex64 and one-wire steps only (128 MiB per state)
SHAPE_RUNS = [(n, which, x64) for n in SHAPE_SIZES for which in ("ends", "mid") for x64 in (False, True)
              if n < 12 or (which == "ends" and not x64)]


@pytest.mark.parametrize("n,which,x64", SHAPE_RUNS, ids=lambda v: {False: "c64", True: "x64"}.get(v, str(v)))
def test_launch_shapes(n, which, x64):
    """one row of the table above per size; steps on wires n - 1, 0 and a middle one, both seeds"""
    ran = [run_case(*c, x64) for c in CASES if c[1] == ("shape", n, which)]
    assert len(ran) == 2


@pytest.mark.parametrize("x64", [False, True], ids=["c64", "x64"])
@pytest.mark.parametrize("n", [7, 8])
def test_every_gate_kind_on_the_multi_block_routes(n, x64):
    """every kind of ONE_WIRE, TWO_WIRE and Rot, the two-wire kinds in both wire orders, behind them a one-wire channel
    on each wire, the pair channel or nothing; every angle wanted.  n = 7: the one-wire steps leave 4 partials per row;
    n = 8: the two-wire steps do."""
    bt = built(("kinds", n, "all"))
    gates = {s[0] for s in layout(bt.key)[0]}
    assert gates == set(F.ONE_WIRE) | set(F.TWO_WIRE) | {"Rot"}
    assert blocks(n, 2) > 1 and (n == 7 or blocks(n, 4) > 1) and len(bt.wanted) == 24
    ran = [run_case(*c, x64) for c in _named(f"kinds n={n}")]
    assert len(ran) == 2


@pytest.mark.parametrize("x64", [False, True], ids=["c64", "x64"])
@pytest.mark.parametrize("obs_name", ["z32", "words"])
def test_seeds(obs_name, x64):
    """z32: Z on a middle wire, a parity across three groups, the full-register parity, QMLE_MAX_QUBITS groups in one
    call.  words: three Y factors (``q == 3`` of ``k_dens_seed_pauli``), two, an identity term, middle wires, and one
    Hermitian whose terms land on the same entry of Lambda and must add."""
    (case,) = [c for c in CASES if c[2] == obs_name]
    run_case(*case, x64)


@pytest.mark.parametrize("x64", [False, True], ids=["c64", "x64"])
def test_identity_term_alone_has_no_gradient(x64):
    bt = built(("kinds", 7, "words"))
    want = [k in set(bt.wanted) for k in range(G.n_slots(bt.tape))]
    with G.x64_scope(x64):
        got = adjoint.density_gradient(bt.tape.ops, 7, bt.B, None, np.ones((bt.B, 1)), want, x64=x64,
                                       obs_terms=[(0.8, 0, 0, 0)])
    print("identity term: largest |gradient|", float(np.abs(got).max()))
    assert float(np.abs(got).max()) <= bar(7, x64)  # Tr(rho) does not move: exactly 0 up to the rounding of the sweep


@pytest.mark.parametrize("x64", [False, True], ids=["c64", "x64"])
def test_seed_term_limit_from_below(x64):
    """96 terms (``kDensMaxSeedTerms``) at n = 4 against the full 4^n reference"""
    (case,) = _named("seed terms96")
    assert len(observable_set("terms96", built(case[1]))[1]) == 96
    run_case(*case, x64)


@pytest.mark.parametrize("x64", [False, True], ids=["c64", "x64"])
def test_seed_term_limit_from_above(x64):
    """97 terms: the library answers QMLE_ERR_UNSUPPORTED before any device work, the wrapper raises ``Unsupported``"""
    bt = built(("terms", 4))
    terms = observable_set("terms97", bt)[1]
    assert len(terms) == 97 and terms[:96] == observable_set("terms96", bt)[1]
    want = [k in set(bt.wanted) for k in range(G.n_slots(bt.tape))]
    with G.x64_scope(x64), pytest.raises(N.Unsupported, match="qmle status -10"):
        adjoint.density_gradient(bt.tape.ops, 4, bt.B, None, G.weights(4, bt.B, 303), want, x64=x64, obs_terms=terms)


@pytest.mark.parametrize("x64", [False, True], ids=["c64", "x64"])
def test_rows_read_their_own_checkpoint(x64):
    """K = 3 cotangents x B = 2 samples at n = 7: row r of lambda reads checkpoint r % B, and the samples' angles differ"""
    (case,) = _named("rows K=3")
    bt = built(case[1])
    assert bt.B == 2 and case[3] == 3
    a, b = (reference(case[1], "z", r)[0] for r in range(2))
    assert float(np.abs(a - b).max()) > 1e-2  # a wrong modulus would show
    run_case(*case, x64)
