"""CPU side of tests/test_gpu_density_adjoint_shapes.py: the factorised reference (tests/density_factorised_reference.py)
against the full 4^n reference where that one can go, and the conditions that keep a GPU comparison from passing for the
wrong reason, for every tape, observable set and row of weights the GPU file uses -- all from the reference alone."""
import functools

import numpy as np
import pytest

from qml_essentials_amd import adjoint

import density_adjoint_reference as DR
import density_factorised_reference as F
import noise_reference as NR
import test_gpu_density_adjoint_shapes as S

G = S.G


# ---- the factorised reference against the full one ---------------------------------------------------------------------
@pytest.mark.parametrize("obs_name", ["z", "pauli"])
@pytest.mark.parametrize("key", [("small", 4, 0), ("small", 5, 0), ("small", 5, 1), ("terms", 4)], ids=str)
def test_factorised_equals_full_reference(key, obs_name):
    """n = 4 (groups 2 + 2), n = 5 (2 + 3 and {0, 4} + {1, 2, 3}): within 1e-12 in ``DR.metric``, values included"""
    bt = S.built(key)
    assert sorted(map(sorted, bt.groups)) == {("small", 4, 0): [[0, 1], [2, 3]], ("small", 5, 0): [[0, 1], [2, 3, 4]],
                                              ("small", 5, 1): [[0, 4], [1, 2, 3]], ("terms", 4): [[0, 3], [1, 2]]}[key]
    obs = S.reference_observables(obs_name, bt)
    Ls = F.full_cost_matrices(bt.n, obs)
    if obs_name == "z":  # the words of the Z seed are the cost matrices of the existing reference
        groups = S.observable_set("z", bt)[0]
        for k, L in enumerate(Ls):
            assert np.array_equal(L, DR.cost_matrix(bt.n, np.eye(len(groups))[k], groups=groups))
    else:
        terms = S.observable_set("pauli", bt)[1]
        for k, L in enumerate(Ls):
            assert np.abs(L - DR.cost_matrix(bt.n, np.eye(len(Ls))[k], terms=terms)).max() <= 1e-15
    w = G.weights(len(obs), 3, 7)
    for row in range(bt.B):
        ot = NR.reference_tape(bt.tape, row)
        full = DR.shift_jacobian(ot, bt.n, Ls, set(bt.wanted))
        values, fact = F.jacobian(bt.tape, bt.groups, row, obs, bt.wanted)
        assert np.abs(full[:, list(bt.wanted)]).max() > 1e-2
        assert DR.metric(fact, full, np.ones(1)) <= 1e-12
        assert max(DR.metric(w[r] @ fact, w[r] @ full, w[r]) for r in range(3)) <= 1e-12
        assert np.abs(values - [DR.cost(ot, bt.n, L) for L in Ls]).max() <= 1e-12
        # the complex64 evaluation sits at single precision, not at zero and not beyond
        f32 = np.abs(F.jacobian(bt.tape, bt.groups, row, obs, bt.wanted, dtype=np.complex64)[1] - fact).max()
        assert 1e-10 < f32 < 1e-6
        # a wrong rule in the groups is that wrong rule on the register ("drop_channels" on the register also drops the
        # channels of the OTHER groups from the pull-back, whose factors then depend on the tape order: not compared)
        for v in ("overlap_behind", "halved"):
            wrong = F.jacobian(bt.tape, bt.groups, row, obs, bt.wanted, variant=v)[1]
            assert DR.metric(wrong, DR.adjoint_jacobian(ot, bt.n, Ls, v) * np.isin(np.arange(full.shape[1]), bt.wanted),
                             np.ones(1)) <= 1e-12


def test_a_gate_across_groups_is_refused():
    bt = S.built(("small", 4, 0))
    with pytest.raises(ValueError, match="acts across"):
        F.split(bt.tape, [[0, 2], [1, 3]])


def test_only_the_steps_angles_are_differentiated():
    """the RY layer runs through the one-operator passes: checkpoints = steps + 1"""
    bt = S.built(("kinds", 7, "words"))
    want = [k in set(bt.wanted) for k in range(G.n_slots(bt.tape))]
    sw = adjoint.plan_density(bt.tape.ops, bt.n, want)
    assert bt.wanted == tuple(range(7, 7 + 24)) and sw.checkpoints == 25
    assert sum(1 for s in sw.steps if s[3] < 0) >= 2  # steps with no channel behind them: chan_off = -1
    one = S.built(("shape", 11, "ends"))  # B = 1
    assert one.B == 1 and one.tape.n == 11 and len(one.wanted) == 7


def test_partial_counts_of_the_launch_table():
    """``dens_blocks`` restated: the routes the sizes of the GPU file were chosen for"""
    assert [S.blocks(n, 2) for n in S.SHAPE_SIZES] == [1, 4, 16, 256, 1024, 1024]
    assert [S.blocks(n, 4) for n in S.SHAPE_SIZES] == [1, 1, 4, 64, 256, 1024]
    assert 4**6 >> 2 == 4 * 256 and 4**7 >> 4 == 4 * 256      # one workgroup, four rounds
    assert 4**12 >> 2 == 4 * 1024 * 1024                      # four times what 1024 workgroups cover in one round


# ---- the conditions ----------------------------------------------------------------------------------------------------
def condition_failures(bt, cases, wires_only=False):
    """What the tape ``bt`` misses of the three conditions, for the ``cases`` that use it (S.CASES entries)."""
    out = []
    for row in range(bt.B):  # 1. no wire in a basis state
        z = np.abs(F.wire_z(bt.tape, bt.groups, row))
        out += [("wire <Z>", row, wire, float(z[wire])) for wire in range(bt.n) if not 0.1 <= z[wire] <= 0.9]
    if out or wires_only:
        return out
    wanted = list(bt.wanted)
    for name, _key, obs_name, K, wseed in cases:
        w = S.case_weights(obs_name, bt, K, wseed)
        obs = S.reference_observables(obs_name, bt)
        refs = [S.reference_for(bt, obs_name, row) for row in range(bt.B)]
        wrong = [{v: F.jacobian(bt.tape, bt.groups, row, obs, bt.wanted, variant=v)[1] for v in DR.VARIANTS}
                 for row in range(bt.B)]
        for r in range(w.shape[0]):
            ref, c64 = refs[r % bt.B]
            scale = max(1.0, float(np.abs(w[r]).sum()))
            entries = np.abs(w[r] @ ref)[wanted] / scale
            # 2. every differentiated entry is visible
            out += [("entry", name, obs_name, r, wanted[k], float(entries[k])) for k in np.flatnonzero(entries < 1e-3)]
            need = 100 * S.bar(bt.n, False, float(np.abs(w[r] @ c64 - w[r] @ ref).max()) / scale)
            for v in DR.VARIANTS:  # 3. the wrong rules are 100 complex64 bars away
                moved = DR.metric(w[r] @ wrong[r % bt.B][v], w[r] @ ref, w[r])
                if moved < need:
                    out.append(("variant", name, obs_name, r, v, moved, need))
    return out


TAPE_KEYS = sorted({c[1] for c in S.CASES}, key=str)


def find_seeds(key, limit=4000):
    """How ``S.SEEDS`` was found: group by group the first seed under which nothing that belongs to the group -- the <Z>
    of its wires, the entries of its angles -- misses a condition, the other groups kept; then the whole tape again
    (the variants' distance belongs to no group).  -> the seeds, or None."""
    cases = [c for c in S.CASES if c[1] == key]
    bt = S.Built(key, None)
    home = {w: k for k, g in enumerate(bt.groups) for w in g}
    where = F.split(bt.tape, bt.groups)[1]
    owner = lambda x: home[x[2]] if x[0] == "wire <Z>" else where[x[4]][0] if x[0] == "entry" else -1  # noqa: E731
    seeds = [0] * len(bt.groups)
    for sweep in range(10):  # first every wire's <Z> (cheap, and it hides the rest), then the entries, again as long as
        for g in range(len(bt.groups)):  # another group's new factors move an entry below the line
            for s in range(seeds[g], seeds[g] + limit):
                seeds[g] = s
                missed = condition_failures(S.Built(key, tuple(seeds)), cases, wires_only=sweep == 0)
                if not any(owner(x) == g for x in missed):
                    break
            else:
                return None
        if sweep and not condition_failures(S.Built(key, tuple(seeds)), cases):
            return tuple(seeds)
    return None


def find_seed(key, limit=4000):
    """The int seeds of ``S.SEEDS`` (the shape and terms tapes): the first of 0, 1, 2, .. that, taken for every group,
    meets the conditions.  -> the seed, or None."""
    cases = [c for c in S.CASES if c[1] == key]
    return next((s for s in range(limit) if not condition_failures(S.Built(key, s), cases)), None)


@pytest.mark.parametrize("key", TAPE_KEYS, ids=str)
def test_every_gpu_tape_meets_the_conditions(key):
    """every wire's |<Z>| in [0.1, 0.9]; every differentiated entry of every reference row at least 1e-3 of
    max(1, sum |w|); every wrong variant of ``DR.adjoint_jacobians`` in the groups at least 100 complex64 bars away"""
    assert condition_failures(S.built(key), [c for c in S.CASES if c[1] == key]) == []


def test_the_case_list_covers_the_table():
    keys = {c[1] for c in S.CASES}
    assert {k[1] for k in keys if k[0] == "shape"} == {6, 7, 8, 10, 11, 12}
    assert ("shape", 12, "mid") not in keys
    assert [c[2:4] for c in S.CASES if c[1] == ("kinds", 8, "all")] == [("z", 1), ("pauli", 1)]
    assert [c[2:4] for c in S.CASES if c[1] == ("kinds", 7, "all")] == [("z", 1), ("pauli", 1)]
    assert {(c[1], c[2], c[3]) for c in S.CASES if c[1][:2] == ("kinds", 7) and c[1][2] != "all"} == {
        (("kinds", 7, "z32"), "z32", 1), (("kinds", 7, "words"), "words", 1), (("kinds", 7, "rows"), "z", 3)}
    for n in (6, 7, 8, 10, 11):  # wires n - 1, 0 and a middle one; (n - 2, n - 1) and (n - 1, 0) both ways, (0, n / 2)
        steps = S.layout(("shape", n, "ends"))[0] + S.layout(("shape", n, "mid"))[0]
        wires = [s[1] for s in steps]
        for need in [(n - 1,), (0,), (n // 2,), (n - 2, n - 1), (n - 1, n - 2), (n - 1, 0), (0, n - 1), (0, n // 2)]:
            assert need in wires, (n, need)
    assert [s[1] for s in S.layout(("shape", 12, "ends"))[0]] == [(11,), (0,), (6,)]
    two = [s for s in S.layout(("kinds", 8, "all"))[0] if len(s[1]) == 2]
    for kind in G.TWO_WIRE:  # both wire orders, and among the channels behind them every variant
        assert sorted(s[1][0] < s[1][1] for s in two if s[0] == kind) == [False, True]
    assert {s[2] for s in S.layout(("kinds", 8, "all"))[0]} == {"amp", "phase", "bitflip", "depol", "phaseflip", "pair", None}


@functools.lru_cache(maxsize=None)
def _words():
    return S.observable_set("words", S.built(("kinds", 7, "words")))[1]


def test_the_word_seed_holds_what_it_names():
    ny = [bin(x & z).count("1") for _c, x, z, _col in _words()]
    assert 3 in ny and 2 in ny and any(x == 0 and z == 0 and c != 0 for c, x, z, _col in _words())
    same = [(x, col) for _c, x, _z, col in _words() if col == 4]
    assert len(same) == 4 and len(set(same)) == 1  # four terms on ONE entry (i, i ^ x) of every row of Lambda
    groups = S.observable_set("z32", S.built(("kinds", 7, "z32")))[0]
    assert len(groups) == 32 and [3] in groups and list(range(7)) in groups
    bt = S.built(("kinds", 7, "words"))
    home = {w: k for k, g in enumerate(bt.groups) for w in g}
    assert len({home[w] for w in groups[1]}) == 3


if __name__ == "__main__":  # PYTHONPATH=. python tests/test_density_factorised_reference_cpu.py [kind ..]: S.SEEDS, printed
    import sys

    for key_ in [k for k in TAPE_KEYS if len(sys.argv) < 2 or k[0] in sys.argv[1:]]:
        print(f"    {key_!r}: {(find_seeds if key_[0] == 'kinds' else find_seed)(key_)!r},", flush=True)
