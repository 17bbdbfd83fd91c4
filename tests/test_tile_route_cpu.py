"""The launch policy of the tile passes as a value (`route_tile`), through `Plan.tile_route`, no GPU.

The expected values are the ones the GPU tests assert from the `*_last_run` report of a run -- walk lengths of
tests/test_gpu_dma_staging.py, the kernel choice of tests/test_abi_cpu.py's K2 plan -- not the output of the function
under test.  A request is what the engine knows when it launches the stage: `measuring` below is the fused <Z> pass
of a batch run with single-wire observables (TM_EXPVAL_PARTIAL, the run started from |0..0>, the engine takes rows
that cover several tiles)."""
import functools

import pytest

from qml_essentials_amd import _native as N
from tests.test_abi_cpu import he_layer_ops
from tests.test_measure_in_registers_cpu import ALL_LIVE, fuzz_struct, to_native

P = N.Plan
FZ, MR, IZ, FC = P.ROUTE_FROM_ZERO, P.ROUTE_MULTI_ROWS, P.ROUTE_INIT_ZERO, P.ROUTE_FOLD_COLS
ERR_UNSUPPORTED, ERR_INVALID_ARG = -10, -1
K_MASK_MULTI_OBS = 24  # kMaskMultiObs, qmle_tile.hip


@functools.lru_cache(maxsize=None)
def _plan(kind, n, flags=0, meas="expval"):
    """(plan, executed view, its description); `kind`: "he" (one Hardware-Efficient layer), a fuzz seed, or
    "rx_cx_ry" (tests/test_gpu_measure_in_registers.py: known zeros inside the measuring tile under default flags)."""
    if kind == "he":
        ops, slots = he_layer_ops(n)
    elif kind == "rx_cx_ry":
        ops, slots = to_native([("RX", [w]) for w in range(n)] + [("CX", [w, w + 1]) for w in range(0, n - 1, 2)]
                               + [("RY", [w]) for w in range(n)])
    else:
        ops, slots = to_native(fuzz_struct(kind, n))
    top = P(ops, n, slots, flags=flags)
    ex = top.executed(meas)
    return top, ex, ex.describe()


def measuring(ex, desc, batch, flags=0):
    n = desc["n_qubits"]
    return ex.tile_route(len(desc["stages"]) - 1, batch, P.TM_EXPVAL_PARTIAL, n, FZ | MR | flags)


def kernel_of(r):
    """The instantiation a route names, as the template arguments of its kernel."""
    if r["family"] == "k_tile2":
        return ("k_tile2", r["nt"], r["measure"], r["multi"], r["ws"], r["mw"], r["masks"])
    if r["family"] == "k_tile":
        return ("k_tile", r["dense4"], r["mw"])
    return (r["family"],)


TILE2_INSTANCES = {("k_tile2",) + t for t in [
    (False, False, False, False, False, False), (True, False, False, False, False, False),
    (False, True, False, False, False, False), (True, True, False, False, False, False),
    (False, False, True, False, False, False), (True, False, True, False, False, False),
    (False, True, True, False, False, False), (True, True, True, False, False, False),
    (False, True, True, False, False, True), (True, True, True, False, False, True),
    (False, False, False, True, False, False), (False, True, False, True, False, False),
    (False, True, False, False, True, False), (True, True, False, False, True, False),
    (False, True, False, True, True, False)]}
TILE_INSTANCES = {("k_tile", d4, mw) for d4 in (False, True) for mw in (False, True)}


def assert_agrees_with_describe(r, last):
    """Staging, wave-private walk, lane swap and <Z> from registers of a measuring walk are the batch-independent
    fields of describe()."""
    assert r["status"] == 0 and r["family"] == "k_tile2" and r["measure"] and r["multi"]
    assert r["from_registers"] is last["register_measure_qualifies"] is True
    assert r["staging_dma"] is (last["staging"] == "dma")
    assert r["wave_private"] is last["wave_private_walk"]
    assert r["lane_swap"] is last["last_group_lane_swap"]
    assert r["lane_swap_crossed"] is last.get("lane_swap_crossed", False)
    assert r["walk_slab"] is (last["load_map"] == "slab")
    assert r["row_shift"] == r["tiles_per_workgroup"].bit_length() - 1
    assert r["grid"][0] * r["tiles_per_workgroup"] == 1 << (last["_n"] - last["T"])


def _last(desc):
    last = dict(desc["stages"][-1])
    last["_n"] = desc["n_qubits"]
    return last


@pytest.mark.parametrize("batch,tpw,nt", [(6, 2, False), (16, 4, True)])
def test_walk_lengths_of_the_23_qubit_layer(batch, tpw, nt):
    """tests/test_gpu_dma_staging.py: 2 tiles per workgroup at a batch of 6, 4 at 16, where 16 states of 2^23
    amplitudes are the 1 GiB that turns the streaming instantiation on."""
    _top, ex, desc = _plan("he", 23, ALL_LIVE)
    r = measuring(ex, desc, batch)
    assert r["tiles_per_workgroup"] == tpw and r["nt"] is nt and r["grid"][1] == batch
    last = _last(desc)
    assert_agrees_with_describe(r, last)
    assert r["staging_dma"] and r["wave_private"] and r["lane_swap"] and r["product_form"]


@pytest.mark.parametrize("batch,tpw", [(160, 2), (320, 4), (640, 8)])
def test_walk_lengths_of_the_16_qubit_case(batch, tpw):
    """Fuzz tape 13 in 10-bit tiles (test_short_and_long_walks)."""
    _top, ex, desc = _plan(13, 16, ALL_LIVE | N.plan_flags(tile_bits=10))
    r = measuring(ex, desc, batch)
    assert r["tiles_per_workgroup"] == tpw and r["threads"] == 64
    assert_agrees_with_describe(r, _last(desc))
    assert r["staging_dma"] and r["wave_private"]


def test_the_20_qubit_case_walks_two_wave_private_by_dma():
    """Fuzz tape 10 in 11-bit tiles at a batch of 20 (test_lane_offsets_read_from_the_table)."""
    _top, ex, desc = _plan(10, 20, ALL_LIVE | N.plan_flags(tile_bits=11))
    r = measuring(ex, desc, 20)
    assert r["tiles_per_workgroup"] == 2 and r["wave_private"] and r["staging_dma"]
    assert_agrees_with_describe(r, _last(desc))


def test_register_staged_walks_agree_with_describe():
    """Fuzz tape 13 in 12-bit tiles keeps a barrier per group and stages through registers; fuzz tape 3 stages by DMA
    without being wave-private (tests/test_gpu_dma_staging.py)."""
    _top, ex, desc = _plan(13, 16, ALL_LIVE)
    r = measuring(ex, desc, 640)
    assert r["tiles_per_workgroup"] == 2 and not r["staging_dma"] and not r["wave_private"]
    assert_agrees_with_describe(r, _last(desc))
    _top, ex, desc = _plan(3, 16, ALL_LIVE | N.plan_flags(tile_bits=11))
    r = measuring(ex, desc, 320)
    assert r["tiles_per_workgroup"] == 2 and r["staging_dma"] and not r["wave_private"]
    assert_agrees_with_describe(r, _last(desc))


def test_the_known_zero_k2_plan():
    """Default (sparse) flags, one layer at 24 qubits: one tile per workgroup and the compact grid in the storing
    passes, the product kernels in the middle, k_reg_measure_mono last
    (test_known_zero_tracking_and_kernel_choice_of_the_k2_plan)."""
    _top, ex, desc = _plan("he", 24)
    st = desc["stages"]
    assert len(st) == 3 and st[2]["expval_kernel"] == "k_reg_measure_mono" and st[1]["product"]
    first = ex.tile_route(0, 32, P.TM_STORE, 0, FZ | FC | IZ)
    assert first["status"] == 0 and first["compact"] and first["tiles_per_workgroup"] == 1 and first["grid"] == [1, 32]
    assert not first["fill"] and not first["fill_elided"], "known-zero tracking: nothing to fill"
    mid = ex.tile_route(1, 32, P.TM_STORE, 0, FZ | FC)
    assert mid["family"] == "k_product_stream" and mid["compact"] and mid["tiles_per_workgroup"] == 1
    assert mid["grid"] == [256 // 32, 32], "32 states: 256 workgroups of 512 live amplitudes"
    assert ex.tile_route(1, 1, P.TM_STORE, 0, FZ | FC)["family"] == "k_tile_product", "fewer than 128 workgroups"
    no_cols = ex.tile_route(1, 32, P.TM_STORE, 0, FZ)
    assert no_cols["family"] == "k_tile2" and no_cols["compact"] and no_cols["tiles_per_workgroup"] == 1
    assert no_cols["grid"][0] == 1 << bin(no_cols["tile_free"]).count("1")
    for flags in (0, P.ROUTE_SEMI_SINGLE):  # (the veto is k_reg_measure<false>'s alone)
        last = ex.tile_route(2, 32, P.TM_EXPVAL_MASKS, 24, FZ | FC | MR | flags)
        assert last["family"] == st[2]["expval_kernel"] and last["mono_q"] == 4 and last["pair"] and not last["nt"]
        assert last["row_shift"] == 4 and last["tiles_per_workgroup"] == 16 and last["grid"] == [4096 >> 4, 32]
        assert not last["from_registers"] and not last["staging_dma"]
    assert ex.tile_route(2, 256, P.TM_EXPVAL_MASKS, 24, FZ | FC | MR)["nt"], "256 x 2^20 live amplitudes = 2 GiB"


def test_whole_state_plans_take_ws():
    _top, ex, desc = _plan("he", 12)
    assert desc["whole_state_lds"]
    want = {P.TM_STORE: (False, False), P.TM_PROBS: (False, False), P.TM_EXPVAL: (True, False),
            P.TM_MW_ONLY: (True, True)}
    for meas, (measure, mw) in want.items():
        r = ex.tile_route(0, 8, meas, 12 if meas == P.TM_EXPVAL else 0, IZ)
        assert kernel_of(r) == ("k_tile2", False, measure, False, True, mw, False), (meas, r)
        assert r["grid"] == [1, 8] and r["tiles_per_workgroup"] == 1 and not r["fill"]


def test_meyer_wallach_requests_take_mw():
    _top, ex, desc = _plan("he", 20, ALL_LIVE, "mw")
    last = len(desc["stages"]) - 1
    r = ex.tile_route(last, 4, P.TM_STORE_MW, 0, FZ | MR)
    assert kernel_of(r) == ("k_tile2", False, True, False, False, True, False)
    assert r["tiles_per_workgroup"] == 1 and r["row_shift"] == 0, "Meyer-Wallach rows keep one tile per workgroup"
    assert kernel_of(ex.tile_route(last, 128, P.TM_STORE_MW, 0, FZ | MR))[1] is True, "128 x 2^20 x 8 B = 1 GiB"
    lean = r["mw_lean"]
    assert lean is (desc["stages"][last]["bits"][:4] == [0, 1, 2, 3])
    assert not ex.tile_route(last, 4, P.TM_STORE_MW, 0, FZ | MR | P.ROUTE_NO_MW_LEAN)["mw_lean"]


def test_z_parity_requests_take_masks_up_to_the_accumulator_count():
    _top, ex, desc = _plan(13, 16, ALL_LIVE | N.plan_flags(tile_bits=10))
    last = len(desc["stages"]) - 1
    r = ex.tile_route(last, 640, P.TM_EXPVAL_MASKS, K_MASK_MULTI_OBS, FZ | MR)
    assert kernel_of(r) == ("k_tile2", False, True, True, False, False, True)
    assert r["tiles_per_workgroup"] == 8 and r["row_shift"] == 3 and not r["from_registers"]
    more = ex.tile_route(last, 640, P.TM_EXPVAL_MASKS, K_MASK_MULTI_OBS + 1, FZ | MR)
    assert kernel_of(more) == ("k_tile2", False, True, False, False, False, False) and more["row_shift"] == 0
    rows_per_tile = ex.tile_route(last, 640, P.TM_EXPVAL_MASKS, 4, FZ)
    assert not rows_per_tile["masks"] and rows_per_tile["tiles_per_workgroup"] == 1, "the caller takes no walk rows"


def test_no_multi_zin_turns_the_walk_off_for_known_zero_local_bits_only():
    """18 qubits under default flags: known zeros inside the measuring tile, none among the tiles
    (test_known_zeros_inside_the_tile_keep_register_staging walks 2 at a batch of 160)."""
    _top, ex, desc = _plan("rx_cx_ry", 18)
    last = _last(desc)
    assert any((last["zero_in"] >> p) & 1 for p in last["bits"])
    r = measuring(ex, desc, 160)
    assert r["tiles_per_workgroup"] == 2 and not r["staging_dma"] and r["from_registers"]
    assert_agrees_with_describe(r, last)
    off = measuring(ex, desc, 160, P.ROUTE_NO_MULTI_ZIN)
    assert off["tiles_per_workgroup"] == 1 and not off["multi"] and not off["from_registers"]
    assert off["grid"][0] == 2 * r["grid"][0]
    _top, ex, desc = _plan(13, 16, ALL_LIVE | N.plan_flags(tile_bits=10))  # no known zeros: the switch changes nothing
    assert measuring(ex, desc, 160, P.ROUTE_NO_MULTI_ZIN) == measuring(ex, desc, 160)


def test_a_filled_first_pass_fills_or_elides():
    _top, ex, desc = _plan("he", 23, ALL_LIVE)
    assert desc["stages"][0]["shift"] > 0, "the top-first tile of the schedule for runs from |0..0>"
    r = ex.tile_route(0, 6, P.TM_STORE, 0, FZ | IZ)
    assert r["status"] == 0 and r["fill"] and not r["fill_elided"] and r["compact"] and r["grid"] == [1, 6]
    e = ex.tile_route(0, 6, P.TM_STORE, 0, FZ | IZ | P.ROUTE_ZEROS_IN_PLACE)
    assert e["fill_elided"] and not e["fill"]
    assert {k: v for k, v in e.items() if not k.startswith("fill")} == {k: v for k, v in r.items() if not k.startswith("fill")}


def test_refused_requests_return_their_status():
    _top, ex, desc = _plan("he", 23, ALL_LIVE)
    assert ex.tile_route(0, 6, P.TM_STORE, 0, FZ)["status"] == ERR_UNSUPPORTED, "a shifted tile outside a filled first pass"
    # Meyer-Wallach rows out of a tile of fewer than 10 qubits (callers check mw_fusable)
    _top, ex, desc = _plan("he", 12, N.plan_flags(tile_bits=8, force_tile=True))
    small = [i for i, s in enumerate(desc["stages"]) if s["kind"] == "tile" and s["T"] < 10]
    assert small
    assert ex.tile_route(small[-1], 4, P.TM_STORE_MW, 0, FZ)["status"] == ERR_UNSUPPORTED
    assert ex.tile_route(small[-1], 4, P.TM_STORE, 0, FZ)["status"] == 0
    # (QMLE_ERR_INTERNAL, a measuring walk without the register records: build_fast_groups writes them for every
    # k_tile2 stage below the whole state, so no plan that compiles reaches it)
    with pytest.raises(Exception):
        ex.tile_route(len(desc["stages"]), 4)
    with pytest.raises(Exception):
        ex.tile_route(0, 0)


@functools.lru_cache(maxsize=None)
def _density_plan():
    """vec(rho) of five noisy qubits: one whole-state tile of ten with a 16 x 16 superoperator group (GK_DENSE4)."""
    from qml_essentials_amd import operations as op, simulation
    from qml_essentials_amd.unitary import UnitaryGates

    n = 5
    with op.recording() as tape:
        for w in range(n):
            op.RX(0.3, wires=w)
        op.CX(wires=[0, 1])
        UnitaryGates.NQubitDepolarizingChannel(0.2, [0, 1])
    low = simulation.LoweredTape(simulation.doubled_tape(tape, n), 2 * n)
    plan = P(low.ops, 2 * n, low.n_slots, consts=low.consts if len(low.consts) else None)
    stages = plan.describe()["stages"]
    assert len(stages) == 1 and stages[0]["T"] == 10 and not stages[0]["fast"]
    return plan, 0


def test_every_instantiation_is_reached():
    """All 15 k_tile2 and 4 k_tile instantiations, from requests a run can make."""
    seen = set()

    def go(ex, stage, batch, meas, n_obs, flags):
        r = ex.tile_route(stage, batch, meas, n_obs, flags)
        assert r["status"] == 0, r
        seen.add(kernel_of(r))
        return r

    _t, ws, _d = _plan("he", 12)
    for meas in (P.TM_STORE, P.TM_EXPVAL, P.TM_MW_ONLY):  # WS, WS + MEASURE, WS + MW
        go(ws, 0, 8, meas, 12 if meas == P.TM_EXPVAL else 0, IZ)
    _t, ex, d = _plan(13, 16, ALL_LIVE | N.plan_flags(tile_bits=10))
    last = len(d["stages"]) - 1
    big = 1 << (30 - 3 - 16)  # states of 2^16 amplitudes in 1 GiB
    for batch in (8, big):  # plain and streaming
        go(ex, last, batch, P.TM_STORE, 0, 0)                      # one tile (8 states) / a storing walk
        go(ex, last, batch, P.TM_EXPVAL_PARTIAL, 16, FZ)           # measuring, rows per tile
        go(ex, last, batch, P.TM_STORE_MW, 0, FZ | MR)             # MW
    for batch in (640, big):
        go(ex, last, batch, P.TM_STORE, 0, 0)                      # storing walk
        go(ex, last, batch, P.TM_EXPVAL_PARTIAL, 16, FZ | MR)      # measuring walk
        go(ex, last, batch, P.TM_EXPVAL_MASKS, 8, FZ | MR)         # MASKS
    # streaming stores without a walk: the last storing pass of a run, known zeros inside its tile, the walk off
    _t, kz, d = _plan("rx_cx_ry", 18)
    go(kz, len(d["stages"]) - 1, 1 << (30 - 3 - 18), P.TM_STORE, 0, FZ | P.ROUTE_NO_MULTI_ZIN)
    assert TILE2_INSTANCES <= seen, sorted(TILE2_INSTANCES - seen)
    # k_tile: tiles outside k_tile2's 10..13 qubits
    _t, wide, d = _plan("he", 16, N.plan_flags(tile_bits=14, no_sparse=True), "mw")
    s14 = [i for i, s in enumerate(d["stages"]) if s["kind"] == "tile" and s["T"] == 14 and not s["fast"]]
    assert s14
    go(wide, s14[-1], 4, P.TM_STORE, 0, 0)
    go(wide, s14[-1], 4, P.TM_STORE_MW, 0, FZ)
    rho, stage = _density_plan()
    go(rho, stage, 4, P.TM_STORE, 0, IZ)
    go(rho, stage, 4, P.TM_MW_ONLY, 0, IZ)  # (no caller asks Meyer-Wallach rows of vec(rho); the instantiation exists)
    assert TILE_INSTANCES <= seen, sorted(TILE_INSTANCES - seen)
