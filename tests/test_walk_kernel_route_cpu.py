"""Which tile stages `route_tile` sends to k_measure_walk, host side only: through `qmle_plan_tile_route`
(`Plan.tile_route`, the field `walk_kernel`) and `describe` (`walk_kernel_last_run`, false before any run).

The kernel takes the register-measuring DMA walk with the last group through lane swaps when every group of the stage
runs in product form: the headline layer's last stage, the `all` tapes of tests/test_measured_product_form_cpu.py and
a variant of `all` whose swaps are the crossed ones, and nothing else.  Every other field of the route keeps the value the commit before gave it (PARENT_ROUTE: the
headline's route as that library answered it).

Batches: the headline request is the bench's chunk of 32 states.  A 16-qubit tape at 32 states runs one tile per
workgroup, which is no walk at all, so the hand-built tapes are asked at the batches of their GPU tests: 160 rows (10-bit
tiles, 2 tiles per workgroup), 640 rows (10-bit: 8; 12-bit: 2)."""
import functools

from qml_essentials_amd import _native as N
from tests.test_abi_cpu import he_layer_ops
from tests.test_measure_in_registers_cpu import ALL_LIVE
from tests.test_measured_product_form_cpu import VARIANTS, plan_of, tape

P = N.Plan
PARTIAL = (P.TM_EXPVAL_PARTIAL, P.ROUTE_MULTI_ROWS)

# route of the 24-qubit headline layer's last stage, 32 states, TM_EXPVAL_PARTIAL, ROUTE_MULTI_ROWS, before the field
PARENT_ROUTE = {
    "status": 0, "family": "k_tile2", "dense4": False, "mw": False, "nt": True, "measure": True, "multi": True,
    "ws": False, "masks": False, "mono_q": 0, "pair": False, "grid": [512, 32], "threads": 256, "lds_bytes": 32768,
    "compact": False, "tile_free": 0, "mw_lean": False, "slots_in_lds": True, "fill": False, "fill_elided": False,
    "tiles_per_workgroup": 8, "row_shift": 3, "walk_slab": True, "walk_sync_staged": False,
    "walk_sync_tile_end": False, "staging_dma": True, "lane_swap": True, "lane_swap_crossed": False,
    "from_registers": True, "wave_private": True, "product_form": True,
}


@functools.lru_cache(maxsize=None)
def _layer(n, flags=ALL_LIVE):
    ops, slots = he_layer_ops(n)
    return N.Plan(ops, n, slots, flags=flags).executed("expval")


def _last_route(ex, batch, meas, route_flags, n_obs):
    stages = ex.describe()["stages"]
    route = ex.tile_route(len(stages) - 1, batch, meas, n_obs, route_flags)
    assert route["status"] == 0, route
    return route, stages[-1]


def test_headline_takes_the_kernel_and_every_earlier_field_keeps_its_value():
    route, last = _last_route(_layer(24), 32, *PARTIAL, 24)
    assert route["walk_kernel"] is True
    assert list(route)[-1] == "walk_kernel" and list(route)[-2] == "product_form", "appended behind product_form"
    for key in ("grid", "threads", "lds_bytes", "tiles_per_workgroup", "row_shift"):
        assert route[key] == PARENT_ROUTE[key], key
    assert {k: v for k, v in route.items() if k != "walk_kernel"} == PARENT_ROUTE
    # the report: `expval_kernel` stays what it was (the tile kernels, as opposed to k_reg_measure*), and nothing has run
    assert last["expval_kernel"] == "k_tile" and last["product_form_groups"] == [True, True, True]
    assert last["walk_kernel_last_run"] is False
    # the plain-load twin (5 states: below 1 GiB) takes it too
    route, _ = _last_route(_layer(24), 5, *PARTIAL, 24)
    assert route["walk_kernel"] is True and route["nt"] is False


def test_23_qubit_layer_keeps_k_tile2():
    """Its last group holds one op that runs gate by gate."""
    route, last = _last_route(_layer(23), 32, *PARTIAL, 23)
    assert last["product_form_groups"] == [True, True, False]
    assert route["family"] == "k_tile2" and route["lane_swap"] and route["staging_dma"] and route["from_registers"]
    assert route["walk_kernel"] is False


def _variant_route(name, tile_bits, batch):
    return _last_route(plan_of(tape(name, tile_bits), tile_bits).executed("expval"), batch, *PARTIAL, 16)


def test_the_hand_built_tapes():
    for tile_bits, batch, tpw in ((10, 160, 2), (10, 640, 8), (12, 640, 2)):
        for name, (_f, _l, _b, marks, _free, swap, crossed) in VARIANTS.items():
            route, last = _variant_route(name, tile_bits, batch)
            assert last["product_form_groups"] == marks
            # every variant takes the walk the kernel serves ...
            assert route["family"] == "k_tile2" and route["tiles_per_workgroup"] == tpw and route["from_registers"]
            assert route["staging_dma"] and route["lane_swap"] is swap and route["lane_swap_crossed"] is crossed
            # ... and only the one whose groups all run in product form takes the kernel
            assert route["walk_kernel"] is (name == "all"), (name, tile_bits, batch)
            assert all(marks) is (name == "all")


def crossed_tape(tile_bits, n=16):
    """`all` with CX(9,8), CX(4,8), CX(6,8), CX(8,6) (positions) in front of the front group's CX block: the front group
    then holds position 9 on lane bit 4 and 8 on lane bit 5 (the bank-conflict ordering of its lane bits), the last
    group 8 and 9 at in-thread indices 2 and 3 -- an all-product-form stage with the crossed swaps."""
    def P(pos):
        return n - 1 - pos

    top = list(range(15, 9 if tile_bits == 10 else 10, -1))
    t = [("Rot", [P(p)]) for p in top + [0, 1, 2, 3, 4, 5, 6]]
    t += [("CZ", [P(p), P(i % 4)]) for i, p in enumerate(top)] + [("CX", [P(3), P(4)]), ("CX", [P(2), P(5)])]
    t += [("CX", [P(9), P(8)]), ("CX", [P(4), P(8)]), ("CX", [P(6), P(8)]), ("CX", [P(8), P(6)])]
    t += [("CX", [P(7), P(4)]), ("CX", [P(7), P(5)]), ("CX", [P(7), P(6)])]
    t += [("RY", [P(p)]) for p in (4, 5, 6, 7)] + [("CX", [P(5), P(4)]), ("CX", [P(7), P(6)])]
    t += [("Rot", [P(8)]), ("Rot", [P(9)]), ("CX", [P(9), P(8)]), ("CX", [P(8), P(7)])]
    return t


def test_a_crossed_all_product_form_stage_takes_the_kernel():
    for tile_bits, batch, tpw in ((10, 160, 2), (10, 640, 8), (12, 640, 2)):
        route, last = _last_route(plan_of(crossed_tape(tile_bits), tile_bits).executed("expval"), batch, *PARTIAL, 16)
        assert [g["bits"] for g in last["fast_groups"]] == [[4, 5, 6, 7], [5, 6, 8, 9]]
        assert last["fast_groups"][0]["thread_bits"][4:6] == [9, 8], "lane bits 4 and 5 of the front group"
        assert last["product_form_groups"] == [True, True]
        assert route["tiles_per_workgroup"] == tpw and route["staging_dma"] and route["lane_swap"]
        assert route["lane_swap_crossed"] is True and route["walk_kernel"] is True, (tile_bits, batch)


def test_one_tile_per_workgroup_is_no_walk():
    route, _ = _variant_route("all", 10, 32)
    assert route["tiles_per_workgroup"] == 1 and route["from_registers"] is False and route["walk_kernel"] is False


def test_other_requests_of_the_headline_stage_keep_k_tile2():
    ex = _layer(24)
    route, _ = _last_route(ex, 32, P.TM_STORE, P.ROUTE_MULTI_ROWS, 0)
    assert route["family"] == "k_tile2" and not route["measure"] and route["walk_kernel"] is False
    route, _ = _last_route(ex, 32, P.TM_EXPVAL_MASKS, P.ROUTE_MULTI_ROWS, 5)
    assert route["family"] == "k_tile2" and route["masks"] and route["walk_kernel"] is False
    # rows per tile (the caller does not take rows per walk): one tile per workgroup
    route, _ = _last_route(ex, 32, P.TM_EXPVAL_PARTIAL, 0, 24)
    assert route["tiles_per_workgroup"] == 1 and route["walk_kernel"] is False


def test_a_known_zero_plan_keeps_its_route():
    """Default flags: known-zero tracking and observable folding on; whatever takes the folded plan's last pass, it is
    not the walk kernel."""
    ex = _layer(24, 0)
    for meas, flags in ((P.TM_EXPVAL_PARTIAL, P.ROUTE_FROM_ZERO | P.ROUTE_MULTI_ROWS),
                        (P.TM_EXPVAL_MASKS, P.ROUTE_FROM_ZERO | P.ROUTE_MULTI_ROWS | P.ROUTE_FOLD_COLS)):
        route, _ = _last_route(ex, 32, meas, flags, 24)
        assert route["walk_kernel"] is False, route
    # ... and every tile stage of the plan, asked as a storing pass from |0..0>
    stages = ex.describe()["stages"]
    for i, st in enumerate(stages[:-1]):
        if st["kind"] == "tile":
            r = ex.tile_route(i, 32, P.TM_STORE, 0, P.ROUTE_FROM_ZERO | (P.ROUTE_INIT_ZERO if i == 0 else 0))
            assert r["walk_kernel"] is False
