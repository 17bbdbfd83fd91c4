"""Chunks of one qmle_run_batch call that share a workspace slot: a two-pass all-live plan fills a slot with zeros
once per call and leaves the fill out for every later chunk in it.  Results must not know about it."""
import functools

import numpy as np
import pytest

from oracle import einsum_sim as OE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = 23            # with 1, 3 or 4 states per chunk: many reuses of a slot, and a short last chunk
IN_FLIGHT = (1, 3, 4)
SIZES = (16, 18, 20)
PARITY = ((0, 1), (2, 5, 9), (0, 7, 8, 15), (3,))  # multi-wire Z parities: the general-mask epilogue


def _layers(n, layers):
    from tests.test_abi_cpu import he_layer_ops

    ops, slots = [], 0
    for _ in range(layers):
        o, s_ = he_layer_ops(n)
        ops += [(g, w, [x + slots for x in sl], m) for g, w, sl, m in o]
        slots += s_
    return ops, slots


def _flags():
    from qml_essentials_amd import _native as N

    return N.PLAN_NO_SPARSE | N.PLAN_NO_ABSORB


def _two_stage_plan(n, top_first, monkeypatch):
    """One Hardware-Efficient layer, all-live: two tile passes.  The cost model puts the first tile on the low
    positions at these sizes; candidate 48 puts it on the top 14 (shift = n - 14), as at n = 24."""
    from qml_essentials_amd import _native as N

    ops, slots = _layers(n, 1)
    if top_first:
        monkeypatch.setenv("QMLE_FORCE_CAND", "48")
    plan = N.Plan(ops, n, slots, flags=_flags())
    monkeypatch.delenv("QMLE_FORCE_CAND", raising=False)
    for meas in ("expval", "probs"):
        st = plan.executed(meas).describe()["stages"]
        assert len(st) == 2 and all(s["kind"] == "tile" for s in st), st
        assert (st[0]["shift"] == n - 14) if top_first else (st[0]["shift"] == 0 and st[0]["T"] < n), st[0]
    return plan, slots


def _three_stage_plan(n):
    from qml_essentials_amd import _native as N

    for layers in (3, 4, 5, 6):
        ops, slots = _layers(n, layers)
        plan = N.Plan(ops, n, slots, flags=_flags())
        if len(plan.executed("expval").describe()["stages"]) >= 3:
            return plan, slots
    raise AssertionError(f"no all-live plan of three passes at n = {n}")


def _angles(n, slots, seed=0):
    return np.random.default_rng(7 * n + seed).uniform(0, 2 * np.pi, (B, slots)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _oracle_probs(n):
    """|psi|^2 of the B states of the one-layer circuit, complex128 (qubit q = bit n - 1 - q of the index)."""
    ops, slots = _layers(n, 1)
    ang = _angles(n, slots)
    out = np.empty((B, 1 << n))
    for b in range(B):
        tape = [(g, w, [float(ang[b, s]) for s in sl]) for g, w, sl, _ in ops]
        out[b] = np.abs(OE.simulate_pure(tape, n, np.complex128)) ** 2
    return out


def _oracle(n, meas):
    pr = _oracle_probs(n)
    if meas == "probs":
        return pr
    idx = np.arange(1 << n)
    groups = [(q,) for q in range(n)] if meas == "expval" else PARITY
    cols = []
    for grp in groups:
        sign = np.ones(1 << n)
        for q in grp:
            sign *= 1 - 2 * ((idx >> (n - 1 - q)) & 1)
        cols.append(pr @ sign)
    return np.stack(cols, axis=1)


def _run(plan, ang, meas, n, **kw):
    if meas == "parity":
        return plan.run_parity(ang, PARITY, **kw).clone()
    return plan.run(ang, meas, list(range(n)) if meas == "expval" else (), **kw).clone()


@pytest.mark.parametrize("top_first", [True, False], ids=["top_first", "low_first"])
@pytest.mark.parametrize("n", SIZES)
def test_chunks_that_reuse_a_filled_slot_give_the_single_chunk_results(n, top_first, monkeypatch):
    """<Z> of every wire, Z parities and probabilities of 23 states in chunks of 1, 3 and 4 (two slots on two
    streams, and one slot on the caller's stream): equal to each other within 2e-7, to the single-chunk run within
    1e-6 (sums arrive in another order), and to the complex128 oracle within 1e-6.  The <Z> runs leave fills out
    (asserted on the describe figure, so that they cannot pass on a path that never does); probabilities of a
    two-pass plan store the state in the second pass and must keep every fill (asserted too)."""
    plan, slots = _two_stage_plan(n, top_first, monkeypatch)
    ang = torch.from_numpy(_angles(n, slots)).cuda()
    full = 8 << n
    for meas in ("expval", "parity", "probs"):
        whole = _run(plan, ang, meas, n)
        err = float(np.abs(whole.cpu().numpy().astype(np.float64) - _oracle(n, meas)).max())
        print(f"n={n} top_first={top_first} {meas}: whole batch vs oracle {err:.3g}")
        assert err < 1e-6, (meas, err)
        for k in IN_FLIGHT:
            piped = _run(plan, ang, meas, n, states_in_flight=k)
            monkeypatch.setenv("QMLE_NO_CHUNK_OVERLAP", "1")
            serial = _run(plan, ang, meas, n, states_in_flight=k)
            monkeypatch.delenv("QMLE_NO_CHUNK_OVERLAP")
            wrote = plan.executed("probs" if meas == "probs" else "expval").describe()["stages"][0]["write_bytes_from_zero"]
            assert (wrote == full) if meas == "probs" else (wrote < full), (meas, k, wrote)
            d_forms = (piped - serial).abs().max().item()
            d_whole = max((piped - whole).abs().max().item(), (serial - whole).abs().max().item())
            d_oracle = float(np.abs(piped.cpu().numpy().astype(np.float64) - _oracle(n, meas)).max())
            print(f"  chunks of {k}: two streams vs one {d_forms:.3g}, vs whole batch {d_whole:.3g}, vs oracle {d_oracle:.3g}")
            assert d_forms < 2e-7, (meas, k, d_forms)
            assert d_whole < 1e-6, (meas, k, d_whole)
            assert d_oracle < 1e-6, (meas, k, d_oracle)
        assert (whole[0] - whole[1]).abs().max().item() > 1e-7  # rows are distinct parameter sets


@pytest.mark.parametrize("n", SIZES)
def test_first_chunk_in_a_slot_is_filled_whatever_the_workspace_held(n, monkeypatch):
    """A caller's workspace full of 0x7f bytes (3.4e38 as float32): the same rows as with a fresh one (<Z>: the
    runs that leave fills out; probabilities: a run that keeps them, beside it)."""
    plan, slots = _two_stage_plan(n, True, monkeypatch)
    ang = torch.from_numpy(_angles(n, slots)).cuda()
    for meas in ("expval", "probs"):
        whole = _run(plan, ang, meas, n)
        for k in IN_FLIGHT:
            for one_stream in (False, True):
                if one_stream:
                    monkeypatch.setenv("QMLE_NO_CHUNK_OVERLAP", "1")
                need = plan.workspace_bytes(B, meas, n if meas == "expval" else 0, k)
                ws = torch.full((need,), 0x7F, dtype=torch.uint8, device="cuda")
                got = _run(plan, ang, meas, n, states_in_flight=k, workspace=ws)
                monkeypatch.delenv("QMLE_NO_CHUNK_OVERLAP", raising=False)
                assert (got - whole).abs().max().item() < 1e-6, (meas, k, one_stream)


@pytest.mark.parametrize("n", SIZES)
def test_no_slot_stays_clean_across_calls(n, monkeypatch):
    """One workspace for a sequence of calls: the two-pass plan, a three-pass all-live plan (which leaves the slots
    full of amplitudes), "state" and Meyer-Wallach runs, and the two-pass plan again -- every result equals the
    single-chunk run of the same plan."""
    two, slots2 = _two_stage_plan(n, True, monkeypatch)
    three, slots3 = _three_stage_plan(n)
    ang2 = torch.from_numpy(_angles(n, slots2)).cuda()
    ang3 = torch.from_numpy(_angles(n, slots3, seed=1)).cuda()
    k = 3
    need = max(p.workspace_bytes(B, m, n if m == "expval" else 0, k)
               for p in (two, three) for m in ("expval", "probs", "state", "mw"))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    want = {(id(p), m): _run(p, a, m, n) for p, a in ((two, ang2), (three, ang3)) for m in ("expval", "probs", "state", "mw")}
    seq = [(two, ang2, "expval"), (three, ang3, "expval"), (two, ang2, "expval"), (two, ang2, "state"),
           (two, ang2, "probs"), (three, ang3, "probs"), (two, ang2, "probs"), (two, ang2, "mw"),
           (two, ang2, "expval"), (three, ang3, "mw"), (two, ang2, "expval")]
    for one_stream in (False, True):
        if one_stream:
            monkeypatch.setenv("QMLE_NO_CHUNK_OVERLAP", "1")
        for i, (p, a, m) in enumerate(seq):
            got = _run(p, a, m, n, states_in_flight=k, workspace=ws)
            d = (got - want[(id(p), m)]).abs().max().item()
            assert d < 1e-6, (i, m, one_stream, d)
            if p is two and m == "expval":  # (the sequence does exercise the reuse: fills were left out)
                assert p.executed(m).describe()["stages"][0]["write_bytes_from_zero"] < 8 << n
    monkeypatch.delenv("QMLE_NO_CHUNK_OVERLAP", raising=False)


@pytest.mark.parametrize("n", SIZES)
def test_describe_reports_what_stage_0_of_the_last_run_wrote(n, monkeypatch):
    """Plans that must keep their fills keep them (three passes; a "state" run): 8 * 2^n bytes per state.  The
    two-pass <Z> run with c chunks in s slots wrote s fills of a chunk and one first tile per state."""
    from qml_essentials_amd import _native as N

    full = 8 << n
    three, slots3 = _three_stage_plan(n)
    ang3 = torch.from_numpy(_angles(n, slots3, seed=1)).cuda()
    assert three.executed("expval").describe()["stages"][0]["write_bytes_from_zero"] == full
    three.run(ang3, "expval", list(range(n)), states_in_flight=3)
    assert three.executed("expval").describe()["stages"][0]["write_bytes_from_zero"] == full

    for top_first in (True, False):
        for k in IN_FLIGHT:
            for s in (2, 1):
                if s == 1:
                    monkeypatch.setenv("QMLE_NO_CHUNK_OVERLAP", "1")
                two, slots2 = _two_stage_plan(n, top_first, monkeypatch)  # (a fresh plan: workspace sizes are memoised)
                ang2 = torch.from_numpy(_angles(n, slots2)).cuda()
                ex = two.executed("expval")
                T = ex.describe()["stages"][0]["T"]
                assert ex.describe()["stages"][0]["write_bytes_from_zero"] == full        # before any run
                two.run(ang2, "expval", list(range(n)), states_in_flight=k)
                assert B > s * k  # every slot's first chunk is a whole one
                assert ex.describe()["stages"][0]["write_bytes_from_zero"] == (s * k * full + B * (8 << T)) // B, (k, s)
                two.run(ang2, "expval", list(range(n)))                                      # one chunk: it is filled
                assert ex.describe()["stages"][0]["write_bytes_from_zero"] == full
                two.run(ang2, "expval", list(range(n)), states_in_flight=k)
                two.run(ang2, "state", states_in_flight=k)
                assert two.executed("state").describe()["stages"][0]["write_bytes_from_zero"] == full
                monkeypatch.delenv("QMLE_NO_CHUNK_OVERLAP", raising=False)
    assert N.lib().qmle_sv_version() == 150
