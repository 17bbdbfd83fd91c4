"""`chunk_loop_last_run` of `qmle_plan_describe` before any run (host only; the forms themselves need a GPU:
tests/test_gpu_free_running_chunks.py)."""
from tests.test_abi_cpu import he_layer_ops


def test_a_plan_that_has_not_run_reports_no_loop_form():
    from qml_essentials_amd import _native as N

    n = 16
    ops, slots = he_layer_ops(n)
    plan = N.Plan(ops, n, slots, flags=N.PLAN_NO_SPARSE | N.PLAN_NO_ABSORB)
    for meas in ("expval", "probs", "state"):
        stages = plan.executed(meas).describe()["stages"]
        assert stages[-1]["chunk_loop_last_run"] == "none", meas
        assert all("chunk_loop_last_run" not in st for st in stages[:-1])  # reported once, beside staging_dma_last_run
