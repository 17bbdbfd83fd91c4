"""Which loop form a batch run takes, asked of the host entry `qmle_chunk_loop_form` (no GPU): `alone`
-- the measuring passes back to back on one stream, everything else of a chunk on the other -- for runs whose slots
stay zeroed, whose chunk holds at least 1 GiB of states and whose batch has at least four chunks; every other run the
form it took before.  The forms themselves run in tests/test_gpu_walks_alone.py."""
import pytest

from tests.test_abi_cpu import he_layer_ops
from tests.test_gpu_fill_reuse import B, IN_FLIGHT, _three_stage_plan, _two_stage_plan


def _he_plan(n, extra=0):
    from qml_essentials_amd import _native as N

    ops, slots = he_layer_ops(n)
    return N.Plan(ops, n, slots, flags=N.PLAN_NO_SPARSE | N.PLAN_NO_ABSORB | extra)


def test_the_headline_run_takes_its_measuring_passes_alone():
    """24 qubits, all-live: chunks of 32 states are 4 GiB.  1024 states are 32 chunks; 96 are three, and 128 four."""
    plan = _he_plan(24)
    assert len(plan.executed("expval").describe()["stages"]) == 2
    assert plan.chunk_loop_form(1024, "expval") == "alone"
    assert plan.chunk_loop_form(128, "expval") == "alone"
    assert plan.chunk_loop_form(96, "expval") == "free"
    assert plan.chunk_loop_form(32, "expval") == "one_stream"  # one chunk


def test_the_threshold_is_one_gib_per_chunk_and_four_chunks():
    """20 qubits: a state is 8 MiB, so 128 states are exactly 1 GiB."""
    plan = _he_plan(20)
    assert plan.chunk_loop_form(512, "expval", 128) == "alone"
    assert plan.chunk_loop_form(520, "expval", 128) == "alone"   # five chunks, the last one of 8 states
    assert plan.chunk_loop_form(385, "expval", 128) == "alone"   # four chunks, the last one of 1 state
    assert plan.chunk_loop_form(384, "expval", 128) == "free"    # three chunks
    assert plan.chunk_loop_form(512, "expval", 127) == "free"    # 8 MiB short of 1 GiB
    assert plan.chunk_loop_form(512, "expval", 64) == "free"
    assert plan.chunk_loop_form(2048, "expval") == "alone"       # the default: chunks of 512
    assert plan.chunk_loop_form(1100, "expval") == "free"        # ... three of them


@pytest.mark.parametrize("top_first", [True, False], ids=["top_first", "low_first"])
def test_small_two_stage_runs_stay_free(top_first, monkeypatch):
    """The shapes of tests/test_gpu_free_running_chunks.py and tests/test_gpu_kept_slots.py: 16 qubits, 7 and 23
    states in chunks of 1, 3 and 4."""
    plan, _ = _two_stage_plan(16, top_first, monkeypatch)
    for batch in (7, B):
        for k in IN_FLIGHT:
            assert plan.chunk_loop_form(batch, "expval", k) == ("free" if 2 * k < batch else "one_stream"), (batch, k)


def test_23_qubit_runs_of_a_few_states_stay_free():
    plan = _he_plan(23)
    assert plan.chunk_loop_form(6, "expval", 2) == "free"    # three chunks of 128 MiB
    assert plan.chunk_loop_form(18, "expval", 6) == "free"   # three chunks of 384 MiB
    assert plan.chunk_loop_form(64, "expval", 16) == "alone"  # four chunks of 1 GiB


def test_runs_that_fill_every_chunk_stay_staged(monkeypatch):
    three, _ = _three_stage_plan(16)
    assert three.chunk_loop_form(B, "expval", 3) == "staged"
    two, _ = _two_stage_plan(16, True, monkeypatch)
    assert two.chunk_loop_form(B, "probs", 3) == "staged"
    assert two.chunk_loop_form(B, "expval", 3) == "free"
    # ... at the headline's size too: probabilities store the state in the second pass
    assert _he_plan(24).chunk_loop_form(1024, "probs") == "staged"


def test_one_stream_runs_stay_on_one_stream(monkeypatch):
    from qml_essentials_amd import _native as N

    assert _he_plan(24, N.plan_flags(no_fusion=True)).chunk_loop_form(1024, "expval") == "one_stream"
    plan = _he_plan(24)
    monkeypatch.setenv("QMLE_NO_CHUNK_OVERLAP", "1")
    assert plan.chunk_loop_form(1024, "expval") == "one_stream"
    monkeypatch.delenv("QMLE_NO_CHUNK_OVERLAP")
    assert plan.chunk_loop_form(1024, "expval") == "alone"


def test_arguments_no_run_would_accept():
    from qml_essentials_amd import _native as N

    plan = _he_plan(16)
    assert N.lib().qmle_chunk_loop_form(None, 8, 2, 0) == b"none"
    assert N.lib().qmle_chunk_loop_form(plan._h, 0, 2, 0) == b"none"
    assert N.lib().qmle_chunk_loop_form(plan._h, 8, 9, 0) == b"none"
