"""The finishes of a fused Meyer-Wallach call (`plan.run(angles, "mw")`, csrc/qmle_mw.hip) on states whose purities
have a large population part AND a large cross part on every wire.

a. `test_per_position_finish_forced`: the per-position finish (k_mw_purity_fused, k_mw_purity_final, k_mw_pack) is
   the one every circuit on 29 or more qubits gets, and the columns finish hides it below that.
   QMLE_MW_FINISH_PER_POSITION=1 selects it for any tiled state, so it runs here at n = 15..26: last tiles of 10, 12, 13
   and 14 positions, one and two later reads, with and without the lean split, one slice and many, blocks of 64, 256
   and 1024 threads, one state, three, and a batch run in chunks.  Every case then runs again without the switch: the
   two finishes sum the same float32 rows in float64 and round once, so they agree to one float32 ulp.
b. `test_fused_route_at_its_natural_sizes`: n = 25..29 without any switch -- the columns finish at 128 and 256 slices,
   the non-temporal later reads from n = 27 on, exactly 64 columns of k_mw_colsum at n = 28, and at n = 29 the
   per-position finish where it is the call's own.

Reference: up to 22 qubits (the cases: up to 21) the oracle's C port of the same tape (oracle/c_port.py, purities by oracle/analysis.py);
above, the float64 sums of tests/mw_device_reference.py over the state that the same plan stores.  n = 20 takes both.
Tolerance 1e-6 on every purity and on Q, as in test_gpu_kernels.py::test_meyer_wallach_out_of_the_producing_pass.
Every case asserts `mw_finish_last_run`, so none passes on another finish than the one it names.

Not reached: the `oi < lg` branches of the finish kernels (a row of the producing pass covering several tiles).
route_tile keeps one tile per workgroup for Meyer-Wallach passes, so row_shift is 0 in every run."""
import functools
import time

import numpy as np
import pytest

from oracle import analysis as OA
from tests.mw_device_reference import purities_and_q

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-6
ULP = 2.0 ** -23     # one float32 ulp at 1.0: two roundings of float64 sums that agree to ~1e-16
PART_MIN = 1e-3      # a condition on the inputs: both parts of every purity a thousand times the tolerance
NORM_MAX = 1.25e-7  # of the C port's |norm^2 - 1|: its Q is then within 4 * 1.25e-7 = TOL / 2 of the exact one
CPORT_MAX_N = 22     # the C port up to here (the cases stop at 21: the oracle's purities take seconds per state)


def circuit(n):
    """RY and RZ on every wire, a ring of CRX(q, q + 1 mod n), a closing RY on every wire; slot = 4 groups of n"""
    ops = [("RY", [q], [q], -1) for q in range(n)] + [("RZ", [q], [n + q], -1) for q in range(n)]
    ops += [("CRX", [q, (q + 1) % n], [2 * n + q], -1) for q in range(n)]
    ops += [("RY", [q], [3 * n + q], -1) for q in range(n)]
    return ops, 4 * n


def angles(n, seeds):
    """one row per seed: angles that leave every wire with unequal populations and a large coherence (after one or
    two Hardware-Efficient layers |a - d| is ~1e-4 and a wrong sign of a signed total would pass)"""
    groups = [(0.5, 1.0), (0.3, 1.2), (0.5, 1.1), (0.1, 0.35)]
    rows = []
    for seed in seeds:
        rng = np.random.default_rng(seed)
        rows.append(np.concatenate([rng.uniform(lo, hi, n) for lo, hi in groups]))
    return np.stack(rows).astype(np.float32)


def oracle_tape(n, row):
    tape = [("RY", [q], (float(row[q]),)) for q in range(n)] + [("RZ", [q], (float(row[n + q]),)) for q in range(n)]
    tape += [("CRX", [q, (q + 1) % n], (float(row[2 * n + q]),)) for q in range(n)]
    return tape + [("RY", [q], (float(row[3 * n + q]),)) for q in range(n)]


def check_is_a_probe(pop, cross, what):
    """before anything of the library is looked at: the reference says that both parts of every purity are large"""
    assert float(pop.min()) >= PART_MIN and float(cross.min()) >= PART_MIN, \
        "%s: population part %.3g, cross part %.3g: choose another seed" % (what, float(pop.min()), float(cross.min()))


@functools.lru_cache(maxsize=None)
def cport_reference(n, seeds):
    """(purities by wire [batch, n], Q [batch]) of the C port's states of the tapes of angles(n, seeds).

    The C port's state is a float32 one: its gate matrices are rounded, so its norm drifts (|norm^2 - 1| up to 5e-7
    on these tapes), and a purity is quadratic in norm^2: a state with norm^2 = 1 + e has purities off by 2 e and Q by
    4 e, whatever computes them.  So that the reference's own error stays below half the tolerance, the seeds are
    chosen (on the host, from the C port alone) with |norm^2 - 1| <= NORM_MAX, and that is asserted here like the
    condition on the parts."""
    from oracle import c_port

    ang = angles(n, seeds)
    states = np.stack([c_port.simulate(oracle_tape(n, row), n) for row in ang])
    _, _, pop, cross = purities_and_q(torch.from_numpy(states), return_parts=True)
    check_is_a_probe(pop, cross, "C port, n = %d, seeds %s" % (n, seeds))
    norms = np.array([np.vdot(v, v).real for v in states.astype(np.complex128)])
    assert np.abs(norms - 1).max() <= NORM_MAX, "C port, n = %d, seeds %s: norm^2 - 1 = %s" % (n, seeds, norms - 1)
    pur = np.stack([OA.qubit_purities_pure(v.astype(np.complex128), n) for v in states])
    pur.setflags(write=False)
    return pur, 2 * (1 - pur.mean(axis=1))


def device_reference(plan, ang, what):
    """the same of the states that `plan` stores, summed in float64 on the device"""
    st = plan.run(ang, "state")
    pur, q, pop, cross = purities_and_q(st, return_parts=True)
    del st
    check_is_a_probe(pop, cross, what)
    return pur.cpu().numpy(), q.cpu().numpy()


def run_mw(plan, ang, want_finish, in_flight=0):
    got = plan.run(ang, "mw", states_in_flight=in_flight).cpu().numpy()
    torch.cuda.synchronize()
    last = plan.executed("mw").describe()["stages"][-1]
    assert last["mw_finish_last_run"] == want_finish, last["mw_finish_last_run"]
    return got


def max_err(got, pur, q):
    return float(np.abs(got[:, 1:] - pur).max()), float(np.abs(got[:, 0] - q).max())


# n, seeds (one per state), plan's tile_bits, no_sparse, lean, states in flight (0: all) -> last tile, later reads,
# slices, threads of the forced finish -- read from qmle_meyer_wallach_describe on the host, asserted below.  The
# seeds up to n = 21 were searched on the host for cport_reference's two conditions; above that the condition on the
# parts is asserted on the device reference.
FORCED = [
    (15, (1507, 1508, 1512), 10, False, True, 0, dict(T=10, reads=1, slices=1, threads=64)),
    (16, (1602,), 0, True, False, 0, dict(T=12, reads=1, slices=1, threads=64)),
    (17, (1702, 1711, 1714), 0, False, True, 0, dict(T=13, reads=1, slices=1, threads=64)),
    (18, (1803,), 14, False, False, 0, dict(T=14, reads=1, slices=1, threads=64)),
    (18, (1850, 1852, 1854, 1856, 1858), 10, False, True, 2, dict(T=10, reads=1, slices=1, threads=256)),  # chunks: 2, 2, 1
    (20, (2006,), 0, False, True, 0, dict(T=13, reads=1, slices=1, threads=256)),    # both references
    (21, (2108,), 10, False, False, 0, dict(T=10, reads=2, slices=8, threads=256)),
    (23, (2300, 2301, 2302), 0, False, False, 0, dict(T=12, reads=2, slices=8, threads=256)),
    # (slices of the producing pass's rows and of a later read's have their own lengths: 128 and 256 rows here ...
    (24, (2400,), 14, False, True, 0, dict(T=14, reads=2, slices=8, threads=256)),
    # ... 256 and 128 here)
    (24, (2400,), 0, True, False, 0, dict(T=12, reads=2, slices=16, threads=256)),
    (26, (2600,), 10, False, True, 0, dict(T=10, reads=2, slices=64, threads=1024)),  # 65536 rows in 64 slices
]


def test_forced_cases_cover_what_they_are_for():
    shapes = [c[6] for c in FORCED]
    assert {s["T"] for s in shapes} == {10, 12, 13, 14} and {s["reads"] for s in shapes} == {1, 2}
    assert {s["threads"] for s in shapes} == {64, 256, 1024} and {c[4] for c in FORCED} == {True, False}
    assert 1 in {s["slices"] for s in shapes} and max(s["slices"] for s in shapes) > 1
    assert {1, 3} <= {len(c[1]) for c in FORCED} and any(c[5] and c[5] < len(c[1]) for c in FORCED)


@pytest.mark.parametrize("n,seeds,tile_bits,no_sparse,lean,in_flight,shape", FORCED,
                         ids=["n%d_b%d_T%d_%s%s" % (c[0], len(c[1]), c[6]["T"], "lean" if c[4] else "nolean",
                                                    "_chunks" if c[5] else "") for c in FORCED])
def test_per_position_finish_forced(n, seeds, tile_bits, no_sparse, lean, in_flight, shape, monkeypatch):
    from qml_essentials_amd import _native as N

    batch = len(seeds)
    for name in ("QMLE_MW_FUSE_TILED", "QMLE_MW_NO_LEAN", "QMLE_MW_FINISH_PER_POSITION"):
        monkeypatch.delenv(name, raising=False)
    ops, slots = circuit(n)
    plan = N.Plan(ops, n, slots, flags=N.plan_flags(tile_bits=tile_bits, no_sparse=no_sparse))
    stage = plan.executed("mw").describe()["stages"][-1]
    route_flags = 0 if lean else N.Plan.ROUTE_NO_MW_LEAN
    chunk = in_flight or batch
    d = N.mw_describe(0, chunk, plan=plan, flags=route_flags | N.Plan.ROUTE_MW_PER_POSITION)
    cols = N.mw_describe(0, chunk, plan=plan, flags=route_flags)
    assert d["route"] == "fused" and d["finish"] == "per-position" and cols["finish"] == "columns"
    assert (stage["T"], len(d["reads"]), d["slices"], d["finish_threads"], d["lean"]) == \
        (shape["T"], shape["reads"], shape["slices"], shape["threads"], lean), (stage["T"], d)
    if in_flight:
        assert plan.workspace_bytes(batch, "mw", 0, in_flight) < plan.workspace_bytes(batch, "mw", 0, 0)
    ang = torch.from_numpy(angles(n, seeds)).cuda()
    refs = []
    if n <= CPORT_MAX_N:
        refs.append(("C port",) + cport_reference(n, seeds))
    if n > CPORT_MAX_N or n == 20:
        refs.append(("device",) + device_reference(plan, ang, "stored state, n = %d" % n))
    if not lean:
        monkeypatch.setenv("QMLE_MW_NO_LEAN", "1")
    monkeypatch.setenv("QMLE_MW_FINISH_PER_POSITION", "1")
    forced = run_mw(plan, ang, "per-position", in_flight)
    monkeypatch.delenv("QMLE_MW_FINISH_PER_POSITION")
    columns = run_mw(plan, ang, "columns", in_flight)
    again = run_mw(plan, ang, "columns", in_flight)
    assert forced.shape == (batch, n + 1)
    errs = [(name,) + max_err(forced, pur, q) + (float((forced[:, 1:] - pur).mean()),) for name, pur, q in refs]
    d_pur, d_q = max_err(forced, columns[:, 1:], columns[:, 0])
    print("\nforced per-position n %d batch %d T %d reads %d lean %s slices %d threads %d: " % (
        n, batch, stage["T"], len(d["reads"]), lean, d["slices"], d["finish_threads"])
        + ", ".join("max error against %s: purities %.3g Q %.3g (mean signed, purities: %.3g)" % e for e in errs)
        + "; against the columns finish: purities %.3g Q %.3g; two columns runs equal: %s" % (
            d_pur, d_q, np.array_equal(columns, again)))
    for name, e_pur, e_q, _ in errs:
        assert e_pur < TOL and e_q < TOL, (name, e_pur, e_q)
    if len(refs) == 2:  # the two references of one tape: the C port's state and the stored one are float32 both
        assert np.abs(refs[0][1] - refs[1][1]).max() < TOL and np.abs(refs[0][2] - refs[1][2]).max() < TOL
    assert np.array_equal(columns, again)  # (the rows are reproducible: no atomics anywhere on the route)
    assert d_pur <= ULP and d_q <= 2 * ULP, (d_pur, d_q)


# n, plan flags (tile_bits, no_sparse) -> finish, slices, last tile, later reads
NATURAL = [
    (25, 0, False, dict(finish="columns", slices=128, T=12, reads=2)),
    (25, 0, True, dict(finish="columns", slices=64, T=13, reads=2)),
    (26, 0, False, dict(finish="columns", slices=256, T=12, reads=2)),
    (26, 0, True, dict(finish="columns", slices=256, T=12, reads=2)),
    (27, 0, False, dict(finish="columns", slices=256, T=12, reads=2)),
    (27, 0, True, dict(finish="columns", slices=256, T=12, reads=2)),
    (28, 12, False, dict(finish="columns", slices=256, T=12, reads=2)),
    (28, 0, True, dict(finish="columns", slices=256, T=12, reads=2)),
    (29, 0, False, dict(finish="per-position", slices=64, T=12, reads=3)),
    (29, 0, True, dict(finish="per-position", slices=64, T=12, reads=3)),
]


@pytest.mark.parametrize("n,tile_bits,no_sparse,shape", NATURAL,
                         ids=["n%d_%s" % (c[0], "nosparse" if c[2] else "default") for c in NATURAL])
def test_fused_route_at_its_natural_sizes(n, tile_bits, no_sparse, shape, monkeypatch):
    from qml_essentials_amd import _native as N

    for name in ("QMLE_MW_FUSE_TILED", "QMLE_MW_NO_LEAN", "QMLE_MW_FINISH_PER_POSITION"):
        monkeypatch.delenv(name, raising=False)
    if torch.cuda.mem_get_info()[0] < 3 * (8 << n):
        pytest.skip("needs three times the state (%d GiB) of free device memory" % ((3 * (8 << n)) >> 30))
    t0 = time.perf_counter()
    ops, slots = circuit(n)
    plan = N.Plan(ops, n, slots, flags=N.plan_flags(tile_bits=tile_bits, no_sparse=no_sparse))
    stage = plan.executed("mw").describe()["stages"][-1]
    d = N.mw_describe(0, 1, plan=plan)
    assert d["route"] == "fused" and d["lean"] and stage["bits"] != list(range(stage["T"]))
    assert (d["finish"], d["slices"], stage["T"], len(d["reads"])) == \
        (shape["finish"], shape["slices"], shape["T"], shape["reads"]), (stage["T"], d)
    assert all(r["nt"] == (n >= 27) for r in d["reads"]) and d["reads"][0]["kind"] == "later_low"
    if n == 28:  # 48 columns of a row + 16 signed totals: the last column of k_mw_colsum's thread = column map
        first = [g for g in d["regions"] if g["name"] == "colsum0"][0]
        assert first["bytes"] == d["slices"] * 64 * 8, first
    ang = torch.from_numpy(angles(n, (100 * n,))).cuda()
    pur, q = device_reference(plan, ang, "stored state, n = %d" % n)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    got = run_mw(plan, ang, shape["finish"])
    t2 = time.perf_counter()
    e_pur, e_q = max_err(got, pur, q)
    line = "\nfused n %d T %d reads %d slices %d threads %d finish %s: max error against the device reference: " \
           "purities %.3g Q %.3g; plan, state and reference %.2f s, fused call %.2f s" % (
               n, stage["T"], len(d["reads"]), d["slices"], d["finish_threads"], d["finish"], e_pur, e_q, t1 - t0, t2 - t1)
    if n == 29:  # the stand-alone reads of the stored state
        monkeypatch.setenv("QMLE_MW_FUSE_TILED", "0")
        alone = run_mw(plan, ang, "")
        monkeypatch.delenv("QMLE_MW_FUSE_TILED")
        a_pur, a_q = max_err(alone, got[:, 1:], got[:, 0])
        line += "; against the stand-alone reads: purities %.3g Q %.3g (%.2f s)" % (a_pur, a_q, time.perf_counter() - t2)
    print(line)
    assert e_pur < TOL and e_q < TOL, (e_pur, e_q)
    if n == 29:
        assert a_pur < TOL and a_q < TOL, (a_pur, a_q)
