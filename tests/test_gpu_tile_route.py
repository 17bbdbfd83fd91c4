"""`route_tile` predicts, `launch_tile` issues: for a handful of small runs the route asked for BEFORE the run
(`Plan.tile_route`, host only) equals what the run then reports in the `*_last_run` keys of `describe()`, and the
numbers agree with the oracle at the 1e-6 each case holds in its own test (tests/test_gpu_dma_staging.py,
tests/test_gpu_measure_in_registers.py, tests/test_gpu_kernels.py).

The request is the engine's for the last stage of the run: a fused <Z> pass of single-wire observables asks
TM_EXPVAL_PARTIAL with rows per walk, a whole state in the LDS asks TM_EXPVAL from |0..0>, a Meyer-Wallach run asks
TM_STORE_MW.  `measure_tiles_per_workgroup_last_run` counts the tile kernels' fused <Z> pass only: 0 when
k_reg_measure* took the pass, when the whole state sat in the LDS and for Meyer-Wallach."""
import numpy as np
import pytest

from tests.test_gpu_measure_in_registers import TOL, _reference
from tests.test_measure_in_registers_cpu import ALL_LIVE, N_PARAMS, fuzz_struct, to_native

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _tape(struct, ang_row):
    tape, k = [], 0
    for name, wires in struct:
        p = N_PARAMS.get(name, 0)
        tape.append((name, list(wires), tuple(float(x) for x in ang_row[k:k + p])))
        k += p
    return tape


def _he_struct(n):
    from tests.test_abi_cpu import he_layer_ops

    return [(name, list(wires)) for name, wires, _s, _c in he_layer_ops(n)[0]]


def _route_then_run(struct, n, ang, meas, flags, route_meas, route_flags, fused_walk):
    """The route of the executed plan's last stage, the run, and the run's report against the route."""
    from qml_essentials_amd import _native as N

    ops, slots = to_native(struct)
    plan = N.Plan(ops, n, slots, flags=flags)
    ex = plan.executed(meas)
    last_i = len(ex.describe()["stages"]) - 1
    batch = ang.shape[0]
    route = ex.tile_route(last_i, batch, route_meas, n if meas == "expval" else 0, route_flags)
    assert route["status"] == 0 and route["grid"][1] == batch, route
    dev = torch.from_numpy(np.array(ang, dtype=np.float32)).cuda()
    got = (plan.run(dev, "expval", list(range(n))) if meas == "expval" else plan.run(dev, meas)).cpu().numpy()
    torch.cuda.synchronize()
    last = ex.describe()["stages"][-1]
    walk = fused_walk and not route["family"].startswith("k_reg_measure")
    assert last["measure_tiles_per_workgroup_last_run"] == ((1 << route["row_shift"]) if walk else 0)
    assert last["measured_from_registers_last_run"] is (walk and route["from_registers"])
    assert last["wave_private_walk_last_run"] is (walk and route["wave_private"])
    assert last["staging_dma_last_run"] is (walk and route["staging_dma"])
    assert last["last_group_lane_swap_last_run"] is (walk and route["lane_swap"])
    assert last["group_product_form_last_run"] is route["product_form"]
    return got, route, last


def _c_port_expval(struct, ang, n, rows):
    from oracle import c_port

    return np.asarray([c_port.expval_z(c_port.simulate(_tape(struct, ang[b]), n), n, list(range(n))) for b in rows])


@pytest.mark.parametrize("batch,tpw", [(160, 2), (640, 8)])
def test_the_16_qubit_walks(batch, tpw):
    from qml_essentials_amd import _native as N

    P = N.Plan
    struct, ang, rows, want = _reference(13, 16, batch)
    got, route, last = _route_then_run(struct, 16, ang, "expval", ALL_LIVE | N.plan_flags(tile_bits=10),
                                       P.TM_EXPVAL_PARTIAL, P.ROUTE_FROM_ZERO | P.ROUTE_MULTI_ROWS, True)
    assert route["tiles_per_workgroup"] == tpw and route["staging_dma"] and route["wave_private"]
    assert rows[0] == 0 and rows[-1] == batch - 1
    err = np.abs(got[rows] - want).max()
    print(batch, tpw, "max |err| vs oracle", err)
    assert err <= TOL, err


def test_the_20_qubit_dma_walk():
    from qml_essentials_amd import _native as N

    P = N.Plan
    n, batch = 20, 20
    struct = fuzz_struct(10, n)
    slots = sum(N_PARAMS.get(name, 0) for name, _w in struct)
    ang = np.random.default_rng(8100).uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)
    got, route, last = _route_then_run(struct, n, ang, "expval", ALL_LIVE | N.plan_flags(tile_bits=11),
                                       P.TM_EXPVAL_PARTIAL, P.ROUTE_FROM_ZERO | P.ROUTE_MULTI_ROWS, True)
    assert route["tiles_per_workgroup"] == 2 and route["staging_dma"] and route["wave_private"]
    err = np.abs(got[[0, batch - 1]] - _c_port_expval(struct, ang, n, (0, batch - 1))).max()
    print("max |err| vs oracle", err)
    assert err <= TOL, err


def test_a_sparse_k2_shaped_plan():
    """One Hardware-Efficient layer at 16 qubits under default flags: the folded plan's last pass goes to
    k_reg_measure*, which is no tile walk."""
    from qml_essentials_amd import _native as N

    P = N.Plan
    n, batch = 16, 64
    struct = _he_struct(n)
    slots = sum(N_PARAMS.get(name, 0) for name, _w in struct)
    ang = np.random.default_rng(8200).uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)
    got, route, last = _route_then_run(struct, n, ang, "expval", 0, P.TM_EXPVAL_MASKS,
                                       P.ROUTE_FROM_ZERO | P.ROUTE_MULTI_ROWS | P.ROUTE_FOLD_COLS, True)
    assert route["family"] == last["expval_kernel"] and route["family"].startswith("k_reg_measure")
    err = np.abs(got[[0, batch - 1]] - _c_port_expval(struct, ang, n, (0, batch - 1))).max()
    print(route["family"], "max |err| vs oracle", err)
    assert err <= TOL, err


def test_a_12_qubit_whole_state_plan():
    from qml_essentials_amd import _native as N

    P = N.Plan
    n, batch = 12, 8
    struct = _he_struct(n)
    slots = sum(N_PARAMS.get(name, 0) for name, _w in struct)
    ang = np.random.default_rng(8300).uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)
    got, route, last = _route_then_run(struct, n, ang, "expval", ALL_LIVE, P.TM_EXPVAL, P.ROUTE_INIT_ZERO, False)
    assert route["family"] == "k_tile2" and route["ws"] and route["measure"] and not route["multi"]
    err = np.abs(got[[0, batch - 1]] - _c_port_expval(struct, ang, n, (0, batch - 1))).max()
    print("max |err| vs oracle", err)
    assert err <= TOL, err


def test_a_meyer_wallach_run():
    """The producing pass reports its tile's sums (TM_STORE_MW): every wire's purity of rows 0 and last against the
    oracle's purities of the oracle's state."""
    from oracle import analysis as OA, einsum_sim as OE
    from qml_essentials_amd import _native as N

    P = N.Plan
    n, batch = 16, 3
    struct = _he_struct(n)
    slots = sum(N_PARAMS.get(name, 0) for name, _w in struct)
    ang = np.random.default_rng(8400).uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)
    got, route, last = _route_then_run(struct, n, ang, "mw", ALL_LIVE, P.TM_STORE_MW,
                                       P.ROUTE_FROM_ZERO | P.ROUTE_MULTI_ROWS, False)
    assert route["family"] == "k_tile2" and route["mw"] and route["tiles_per_workgroup"] == 1
    for b in (0, batch - 1):
        psi = np.asarray(OE.simulate_and_measure(_tape(struct, ang[b]), n, "state", (), np.complex128)).reshape(-1)
        pur = OA.qubit_purities_pure(psi, n)
        err = max(np.abs(got[b, 1:] - pur).max(), abs(got[b, 0] - 2 * (1 - pur.mean())))
        print(b, "max |err| vs oracle", err)
        assert err <= 1e-6, err
