"""Chunks of one qmle_run_batch call whose workspace slots stay zeroed (two tile passes with a fused <Z> epilogue,
DESIGN 4.12) run free on the two internal streams: no event orders one stream's measuring pass behind the other's
(ChunkPipeline).  Every row must be what the one-stream loop gives and what the complex128 oracle gives,
and every run says, in the executed plan's report of its last run, which loop form it took.

Bounds: 1e-6 against the oracle (the bound of tests/test_gpu_fill_reuse.py, whose plans, angles and oracle rows these
tests share); against the one-stream rows one unit in the last place of a float32 at the scale of the values,
|<Z>| <= 1: 2^-23.  (No kernel of these runs adds in arrival order, so the rows are expected to be equal.)"""
import numpy as np
import pytest

from tests.test_gpu_fill_reuse import B, IN_FLIGHT, SIZES, _angles, _oracle, _three_stage_plan, _two_stage_plan

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-6
ULP = float(np.spacing(np.float32(1.0)))  # 2^-23
BATCHES = (7, B)


def _form(plan, meas="expval"):
    return plan.executed(meas).describe()["stages"][-1]["chunk_loop_last_run"]


def _expval(plan, ang, n, k, monkeypatch, one_stream=False, workspace=None):
    """<Z> of every wire with a workspace cut for two slots of k states -> (rows, loop form of the run)."""
    # (asked with the switch off: the size is memoised per plan, and a query under the switch reserves one slot)
    plan.workspace_bytes(int(ang.shape[0]), "expval", n, k)
    if one_stream:
        monkeypatch.setenv("QMLE_NO_CHUNK_OVERLAP", "1")
    try:
        out = plan.run(ang, "expval", list(range(n)), states_in_flight=k, workspace=workspace).clone()
    finally:
        monkeypatch.delenv("QMLE_NO_CHUNK_OVERLAP", raising=False)
    return out, _form(plan)


def _check(got, serial, want, what):
    d_oracle = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    d_serial = (got - serial).abs().max().item()
    print(f"  {what}: vs oracle {d_oracle:.3g}, two streams vs one {d_serial:.3g}")
    assert d_oracle < TOL, (what, d_oracle)
    assert d_serial <= ULP, (what, d_serial)


@pytest.mark.parametrize("top_first", [True, False], ids=["top_first", "low_first"])
@pytest.mark.parametrize("n", SIZES)
def test_free_running_chunks_give_the_one_stream_rows(n, top_first, monkeypatch):
    """7 and 23 states in chunks of 1, 3 and 4 (7 / 3 / 2 and 23 / 8 / 6 chunks, the last one short): the two-stream
    run is free, the QMLE_NO_CHUNK_OVERLAP=1 run one stream.  (7 states with room for two chunks of 4 fit the
    workspace whole: batch_layout runs them as one chunk on the caller's stream.)"""
    plan, slots = _two_stage_plan(n, top_first, monkeypatch)
    assert _form(plan) == "none"  # before any run
    all_ang = _angles(n, slots)
    for batch in BATCHES:
        ang = torch.from_numpy(all_ang[:batch]).cuda()
        want = _oracle(n, "expval")[:batch]
        for k in IN_FLIGHT:
            piped, form = _expval(plan, ang, n, k, monkeypatch)
            serial, form_serial = _expval(plan, ang, n, k, monkeypatch, one_stream=True)
            assert form == ("free" if 2 * k < batch else "one_stream"), (batch, k, form)
            assert form_serial == "one_stream", (batch, k, form_serial)
            _check(piped, serial, want, f"n={n} batch={batch} chunks of {k} ({form})")
    assert (piped[0] - piped[1]).abs().max().item() > 1e-7  # rows are distinct parameter sets


@pytest.mark.parametrize("n", SIZES)
def test_a_workspace_full_of_0x7f_bytes(n, monkeypatch):
    """The caller's workspace holds 3.4e38 everywhere: each slot's first chunk is filled, on either stream, before
    anything of that slot is read."""
    plan, slots = _two_stage_plan(n, True, monkeypatch)
    all_ang = _angles(n, slots)
    for batch in BATCHES:
        ang = torch.from_numpy(all_ang[:batch]).cuda()
        want = _oracle(n, "expval")[:batch]
        for k in IN_FLIGHT:
            need = plan.workspace_bytes(batch, "expval", n, k)
            serial, _ = _expval(plan, ang, n, k, monkeypatch, one_stream=True)
            ws = torch.full((need,), 0x7F, dtype=torch.uint8, device="cuda")
            piped, form = _expval(plan, ang, n, k, monkeypatch, workspace=ws)
            assert form == ("free" if 2 * k < batch else "one_stream"), (batch, k, form)
            _check(piped, serial, want, f"n={n} batch={batch} chunks of {k}, 0x7f workspace")


@pytest.mark.parametrize("n", SIZES)
def test_two_calls_in_a_row_on_one_workspace(n, monkeypatch):
    """The second call is queued while the first one's chunks may still run on the internal streams: it forks from the
    caller's stream, which the first call joined.  Its rows are those of its own angles (the batch reversed)."""
    plan, slots = _two_stage_plan(n, True, monkeypatch)
    ang = torch.from_numpy(_angles(n, slots)).cuda()
    back = torch.flip(ang, dims=(0,)).contiguous()
    want = _oracle(n, "expval")
    for k in IN_FLIGHT:
        ws = torch.empty(plan.workspace_bytes(B, "expval", n, k), dtype=torch.uint8, device="cuda")
        first = plan.run(ang, "expval", list(range(n)), states_in_flight=k, workspace=ws)
        second = plan.run(back, "expval", list(range(n)), states_in_flight=k, workspace=ws)
        assert _form(plan) == "free"
        first, second = first.clone(), second.clone()
        serial, _ = _expval(plan, ang, n, k, monkeypatch, one_stream=True)
        _check(first, serial, want, f"n={n} chunks of {k}, first call")
        _check(second, torch.flip(serial, dims=(0,)), want[::-1], f"n={n} chunks of {k}, second call")


@pytest.mark.parametrize("n", SIZES)
def test_work_on_the_callers_stream_before_and_after(n, monkeypatch):
    """A side stream of the caller's: the angles are produced by a kernel queued on it in front of the call and the
    rows consumed by one queued behind it, without a synchronise in between -- the internal streams fork behind the
    first and the caller's stream waits for both of them in front of the second."""
    plan, slots = _two_stage_plan(n, True, monkeypatch)
    host = torch.from_numpy(_angles(n, slots))
    want = _oracle(n, "expval")
    serial, _ = _expval(plan, host.cuda(), n, 3, monkeypatch, one_stream=True)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        half = host.cuda() * 0.5
        pad = torch.zeros(1 << 24, device="cuda")
        for _ in range(4):
            pad += 1.0           # (keeps the stream busy while the call is queued)
        ang = half + half        # the angles exist only once this has run
        out = plan.run(ang, "expval", list(range(n)), states_in_flight=3)
        after = out * 2.0        # reads every row on the caller's stream
        pad *= 2.0
    stream.synchronize()
    assert _form(plan) == "free"
    assert float(pad[0]) == 8.0 and float(pad[-1]) == 8.0
    _check(after * 0.5, serial, want, f"n={n} on a side stream of the caller's")


def _headline_rows(n, batch, per_chunk, rows, monkeypatch):
    """The headline's layer at n qubits in chunks of per_chunk states: free against one stream on every row, and
    against oracle.c_port on `rows`.  -> the last stage's report of the free run."""
    from oracle import c_port
    from qml_essentials_amd import _native as N
    from tests.test_abi_cpu import he_layer_ops

    ops, slots = he_layer_ops(n)
    ang = np.random.default_rng(9000 + n + batch).uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)
    plan = N.Plan(ops, n, slots, flags=N.PLAN_NO_SPARSE | N.PLAN_NO_ABSORB)
    dev = torch.from_numpy(ang).cuda()
    piped, form = _expval(plan, dev, n, per_chunk, monkeypatch)
    last = plan.executed("expval").describe()["stages"][-1]
    # (the one-stream loop takes a workspace cut for two slots as one slot of twice the states, and a launch of
    # twice the states may walk twice the tiles per workgroup, which adds a row's tiles in another order: cut for half)
    assert per_chunk % 2 == 0
    serial, _ = _expval(plan, dev, n, per_chunk // 2, monkeypatch, one_stream=True)
    assert form == "free", form
    assert plan.executed("expval").describe()["stages"][-1]["measure_tiles_per_workgroup_last_run"] == \
        last["measure_tiles_per_workgroup_last_run"]
    d_serial = (piped - serial).abs().max().item()
    print(f"n={n} batch={batch} chunks of {per_chunk}: two streams vs one {d_serial:.3g}")
    assert d_serial <= ULP, d_serial
    got = piped.cpu().numpy()
    for b in rows:
        tape = [(name, wires, tuple(float(ang[b, s]) for s in sl)) for name, wires, sl, _ in ops]
        err = np.abs(got[b] - c_port.expval_z(c_port.simulate(tape, n), n, list(range(n)))).max()
        print(f"  row {b}: max |err| vs oracle {err:.3g}")
        assert err <= TOL, (b, err)
    return last


def test_23_qubits_six_states_in_chunks_of_two(monkeypatch):
    """Three chunks of 2^23-amplitude states, two of them in slot 0.  (Two states are 2048 workgroups of one tile each:
    below the 5120 at which launch_tile lets a workgroup walk two tiles, so this run measures a tile per workgroup;
    the case below walks.)"""
    last = _headline_rows(23, 6, 2, (0, 5), monkeypatch)
    assert last["staging"] == "dma"


def test_the_dma_walk_in_free_running_chunks(monkeypatch):
    """Chunks of six 23-qubit states walk two tiles per workgroup, staged by LDS DMA (tests/test_gpu_dma_staging.py):
    three such chunks on the two streams, two walks sharing the card."""
    last = _headline_rows(23, 18, 6, (0, 17), monkeypatch)
    assert last["measure_tiles_per_workgroup_last_run"] == 2 and last["measured_from_registers_last_run"] is True
    assert last["staging"] == "dma" and last["staging_dma_last_run"] is True


def test_every_other_run_keeps_the_staged_pipeline(monkeypatch):
    """Three tile passes store into the state buffer behind stage 0, and so does the second pass of a two-pass plan
    asked for probabilities: their chunks are filled one by one and stay one stage apart."""
    n = 16
    three, slots3 = _three_stage_plan(n)
    ang3 = torch.from_numpy(_angles(n, slots3, seed=1)).cuda()
    whole = three.run(ang3, "expval", list(range(n))).clone()
    assert _form(three) == "one_stream"  # one chunk
    piped, form = _expval(three, ang3, n, 3, monkeypatch)
    assert form == "staged", form
    serial, form_serial = _expval(three, ang3, n, 3, monkeypatch, one_stream=True)
    assert form_serial == "one_stream", form_serial
    assert (piped - serial).abs().max().item() <= ULP
    assert (piped - whole).abs().max().item() < TOL

    two, slots2 = _two_stage_plan(n, True, monkeypatch)
    ang2 = torch.from_numpy(_angles(n, slots2)).cuda()
    probs = two.run(ang2, "probs", states_in_flight=3)
    assert _form(two, "probs") == "staged"
    assert float(np.abs(probs.cpu().numpy().astype(np.float64) - _oracle(n, "probs")).max()) < TOL
    two.run(ang2, "expval", list(range(n)), states_in_flight=3)
    assert _form(two) == "free"
