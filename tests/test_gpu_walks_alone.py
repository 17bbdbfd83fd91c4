"""Runs whose measuring pass streams at least 1 GiB per chunk, in at least four chunks, take the `alone` form
(ChunkPipeline): one internal stream carries the measuring passes back to back and nothing else,
the other every chunk's first pass and epilogue, one chunk ahead with the first passes.  Every row must be what the
one-stream loop gives and what the complex128 oracle gives, whatever the workspace held, call after call.

The shape: the headline's layer at 20 qubits, all-live, in chunks of 128 states -- exactly 1 GiB per launch, a
workspace of 2 GiB.  Bounds, as in tests/test_gpu_free_running_chunks.py: 1e-6 against oracle.c_port; against the
one-stream rows one unit in the last place of a float32 at the scale of the values, |<Z>| <= 1: 2^-23.  (The same
kernels run with the same arguments, so the rows are expected to be equal.)"""
import functools

import numpy as np
import pytest

from tests.test_gpu_free_running_chunks import TOL, ULP, _expval, _form

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_Q = 20
K = 128   # states per chunk: 128 * 8 * 2^20 = 1 GiB
MOST = 520


@functools.lru_cache(maxsize=None)
def _layer(n):
    from qml_essentials_amd import _native as N
    from tests.test_abi_cpu import he_layer_ops

    ops, slots = he_layer_ops(n)
    plan = N.Plan(ops, n, slots, flags=N.PLAN_NO_SPARSE | N.PLAN_NO_ABSORB)
    assert len(plan.executed("expval").describe()["stages"]) == 2
    return plan, ops, slots


@functools.lru_cache(maxsize=None)
def _angles(n=N_Q, batch=MOST):
    return np.random.default_rng(9100 + n).uniform(0, 2 * np.pi, (batch, _layer(n)[2])).astype(np.float32)


def _serial(n, ang, k, monkeypatch):
    """The one-stream rows.  (The one-stream loop takes a workspace cut for two slots as one slot of twice the states,
    and a launch of twice the states may walk twice the tiles per workgroup, which adds a row's tiles in another order:
    cut for half the chunk.)"""
    assert k % 2 == 0
    rows, form = _expval(_layer(n)[0], ang, n, k // 2, monkeypatch, one_stream=True)
    assert form == "one_stream", form
    return rows, _layer(n)[0].executed("expval").describe()["stages"][-1]["measure_tiles_per_workgroup_last_run"]


def _oracle_row(n, host, b):
    from oracle import c_port

    tape = [(name, wires, tuple(float(host[b, s]) for s in sl)) for name, wires, sl, _ in _layer(n)[1]]
    return c_port.expval_z(c_port.simulate(tape, n), n, list(range(n)))


def _check(got, serial, what):
    d = (got - serial).abs().max().item()
    print(f"  {what}: alone vs one stream {d:.3g}")
    assert d <= ULP, (what, d)


def _check_oracle(n, got, host, rows):
    got = got.cpu().numpy()
    for b in rows:
        err = float(np.abs(got[b] - _oracle_row(n, host, b)).max())
        print(f"  row {b}: max |err| vs oracle {err:.3g}")
        assert err <= TOL, (b, err)


@pytest.mark.parametrize("batch", [512, MOST], ids=["four_chunks", "short_last_chunk"])
def test_walks_alone_give_the_one_stream_rows(batch, monkeypatch):
    """512 states are four chunks of 128; 520 end in a chunk of 8."""
    plan = _layer(N_Q)[0]
    host = _angles()[:batch]
    ang = torch.from_numpy(host).cuda()
    got, form = _expval(plan, ang, N_Q, K, monkeypatch)
    assert form == "alone", form
    tpw = plan.executed("expval").describe()["stages"][-1]["measure_tiles_per_workgroup_last_run"]
    serial, tpw_serial = _serial(N_Q, ang, K, monkeypatch)
    assert tpw == tpw_serial, (tpw, tpw_serial)
    _check(got, serial, f"batch {batch}")
    _check_oracle(N_Q, got, host, (0, batch - 1))
    assert (got[0] - got[1]).abs().max().item() > 1e-7  # rows are distinct parameter sets


def test_a_workspace_full_of_0x7f_bytes(monkeypatch):
    """Each slot's first chunk is filled on the stream of the first passes before the other stream reads the slot."""
    plan = _layer(N_Q)[0]
    ang = torch.from_numpy(_angles()).cuda()
    serial, _ = _serial(N_Q, ang, K, monkeypatch)
    ws = torch.full((plan.workspace_bytes(MOST, "expval", N_Q, K),), 0x7F, dtype=torch.uint8, device="cuda")
    got, form = _expval(plan, ang, N_Q, K, monkeypatch, workspace=ws)
    assert form == "alone", form
    _check(got, serial, "0x7f workspace")


def test_a_second_call_on_the_returned_token_fills_nothing(monkeypatch):
    plan = _layer(N_Q)[0]
    ang = torch.from_numpy(_angles()).cuda()
    back = torch.flip(ang, dims=(0,)).contiguous()
    serial, _ = _serial(N_Q, ang, K, monkeypatch)
    ws = torch.full((plan.workspace_bytes(MOST, "expval", N_Q, K),), 0x7F, dtype=torch.uint8, device="cuda")
    wires = list(range(N_Q))
    first, used, token = plan.run(ang, "expval", wires, states_in_flight=K, workspace=ws, token=0)
    first = first.clone()
    st = plan.executed("expval").describe()["stages"]
    assert used is ws and token != 0 and st[-1]["chunk_loop_last_run"] == "alone"
    assert st[0]["write_bytes_from_zero"] == (2 * K * (8 << N_Q) + MOST * (8 << st[0]["T"])) // MOST
    second, used, token2 = plan.run(back, "expval", wires, states_in_flight=K, workspace=ws, token=token)
    second = second.clone()
    st = plan.executed("expval").describe()["stages"]
    assert used is ws and token2 == token and st[-1]["chunk_loop_last_run"] == "alone"
    assert st[0]["write_bytes_from_zero"] == 8 << st[0]["T"], st[0]["write_bytes_from_zero"]
    _check(first, serial, "first call")
    _check(second, torch.flip(serial, dims=(0,)), "second call, on the token")


def test_two_calls_in_a_row_without_a_synchronise(monkeypatch):
    """The second call forks from the caller's stream, which the first call's two streams joined."""
    plan = _layer(N_Q)[0]
    ang = torch.from_numpy(_angles()).cuda()
    back = torch.flip(ang, dims=(0,)).contiguous()
    ws = torch.empty(plan.workspace_bytes(MOST, "expval", N_Q, K), dtype=torch.uint8, device="cuda")
    wires = list(range(N_Q))
    first = plan.run(ang, "expval", wires, states_in_flight=K, workspace=ws)
    second = plan.run(back, "expval", wires, states_in_flight=K, workspace=ws)
    assert _form(plan) == "alone"
    first, second = first.clone(), second.clone()
    serial, _ = _serial(N_Q, ang, K, monkeypatch)
    _check(first, serial, "first call")
    _check(second, torch.flip(serial, dims=(0,)), "second call")


def test_three_chunks_stay_free(monkeypatch):
    plan = _layer(N_Q)[0]
    ang = torch.from_numpy(_angles()[:384]).cuda()
    got, form = _expval(plan, ang, N_Q, K, monkeypatch)
    assert form == "free", form
    serial, _ = _serial(N_Q, ang, K, monkeypatch)
    _check(got, serial, "three chunks")


def test_work_on_the_callers_stream_before_and_after(monkeypatch):
    """A side stream of the caller's: the angles are produced by a kernel queued on it in front of the call and the
    rows consumed by one queued behind it, without a synchronise in between."""
    plan = _layer(N_Q)[0]
    host = torch.from_numpy(_angles()[:512])
    serial, _ = _serial(N_Q, host.cuda(), K, monkeypatch)
    plan.workspace_bytes(512, "expval", N_Q, K)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        half = host.cuda() * 0.5
        pad = torch.zeros(1 << 24, device="cuda")
        for _ in range(4):
            pad += 1.0           # (keeps the stream busy while the call is queued)
        ang = half + half        # the angles exist only once this has run
        out = plan.run(ang, "expval", list(range(N_Q)), states_in_flight=K)
        after = out * 2.0        # reads every row on the caller's stream
        pad *= 2.0
    stream.synchronize()
    assert _form(plan) == "alone"
    assert float(pad[0]) == 8.0 and float(pad[-1]) == 8.0
    _check(after * 0.5, serial, "on a side stream of the caller's")


def test_the_dma_walk_of_several_tiles_runs_alone(monkeypatch):
    """23 qubits, 64 states in chunks of 16 (1 GiB): a workgroup walks several tiles, staged by LDS DMA."""
    n, batch, k = 23, 64, 16
    plan = _layer(n)[0]
    host = _angles(n, batch)
    ang = torch.from_numpy(host).cuda()
    got, form = _expval(plan, ang, n, k, monkeypatch)
    last = plan.executed("expval").describe()["stages"][-1]
    assert form == "alone", form
    assert last["measure_tiles_per_workgroup_last_run"] > 1 and last["staging_dma_last_run"] is True, last
    serial, tpw_serial = _serial(n, ang, k, monkeypatch)
    assert last["measure_tiles_per_workgroup_last_run"] == tpw_serial
    _check(got, serial, "23 qubits")
    _check_oracle(n, got, host, (0, batch - 1))


def test_a_model_keeps_its_workspace_in_the_alone_form(monkeypatch):
    """Through Model -> CompiledCall: 20 qubits, all-live, 2048 states (four chunks of 512).  The second call runs on
    the kept pair and fills nothing; its rows are those of the first call bit for bit."""
    from qml_essentials_amd import _native as N
    from qml_essentials_amd import simulation
    from qml_essentials_amd.model import Model

    n, batch = 20, 2048
    monkeypatch.setattr(simulation, "PLAN_FLAGS", N.PLAN_NO_SPARSE | N.PLAN_NO_ABSORB)
    model = Model(n, 1, "Hardware_Efficient", data_reupload=False)
    params = np.random.default_rng(6).uniform(0, 2 * np.pi, (batch, *model.params.shape[1:])).astype(np.float32)
    dev = torch.from_numpy(params).cuda()
    first = model(params=dev).clone()
    calls = [cc for cc in model.script._compiled.values() if cc._kept is not None]
    assert len(calls) == 1
    cc = calls[0]
    key, ws, token, kept = cc._kept
    ex = cc.plan.executed("expval")
    st = ex.describe()["stages"]
    assert len(st) == 2 and st[-1]["chunk_loop_last_run"] == "alone" and kept and token
    assert st[0]["write_bytes_from_zero"] > 8 << st[0]["T"]
    second = model(params=dev).clone()
    assert cc._kept[1] is ws and cc._kept[2] == token
    st = ex.describe()["stages"]
    assert st[-1]["chunk_loop_last_run"] == "alone" and st[0]["write_bytes_from_zero"] == 8 << st[0]["T"]
    assert torch.equal(first, second)
    from oracle import c_port, circuits as OC

    spec = OC.ModelSpec(n, 1, "Hardware_Efficient", data_reupload=False)
    got = second.reshape(batch, -1).cpu().numpy()
    for b in (0, batch - 1):
        want = c_port.expval_z(c_port.simulate(OC.model_tape(spec, params[b], [0.0]), n), n, list(range(n)))
        assert float(np.abs(want - got[b]).max()) < TOL, b
