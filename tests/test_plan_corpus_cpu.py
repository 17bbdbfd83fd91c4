"""The corpus of tools/plan_corpus.py -- the tapes whose plans a change to the plan compiler is compared on -- keeps
reaching every branch of the compiler it names, and a compile is a function of the tape, the flags and the tuning
switches alone: compiled twice, a case gives the same text.  No GPU."""
import functools

import pytest

from tools import plan_corpus as PC


@functools.lru_cache(maxsize=None)
def _corpus():
    """{case name: (status, texts)} of the whole corpus, compiled once."""
    return {case.name: PC.compile_text(case) for case in PC.cases()}


def test_case_names_are_unique_and_every_valid_case_compiles():
    cases = PC.cases()
    assert len({c.name for c in cases}) == len(cases)
    for name, (status, texts) in _corpus().items():
        assert (status != 0) == name.startswith("invalid-"), (name, status)
        assert bool(texts) == (status == 0), name


def test_the_corpus_reaches_every_branch_it_names():
    seen = [d for _status, texts in _corpus().values() for d in PC.descriptions(texts)]
    assert PC.missing_branches(seen) == []
    assert PC.missing_branches(seen[:1]) != [], "one plan does not show every branch: the check can fail"


def test_every_validation_error_is_reported_and_the_first_failing_op_decides():
    status = {name: s for name, (s, _t) in _corpus().items() if name.startswith("invalid-")}
    want = {"unknown_op": -5, "wire_count": -2, "wire_range": -4, "duplicate_wires": -3, "slot_range": -11,
            "const_range": -1, "diag_all_range": -1}
    for kind, code in want.items():
        assert status["invalid-" + kind] == code, kind
    for name, got in status.items():
        if "-then-" in name:
            first = name[len("invalid-"):].split("-then-")[0]
            assert got == want[first], name


def test_every_forced_candidate_that_may_run_is_the_one_described():
    """QMLE_FORCE_CAND = k on the all-live layers: the executed <Z> plan runs candidate k wherever the compiler may
    take it, and one of each of the five variants is among them."""
    import json

    variants = set()
    for name, (status, texts) in _corpus().items():
        if not name.startswith("cand-") or not name.split("-")[-1].isdigit() or "-all_live-" not in name:
            continue
        k, ran = int(name.split("-")[-1]), json.loads(texts[1 + list(PC.N.MEAS).index("expval")])["candidate"]
        if ran == k:
            variants.add(k // PC.CANDIDATES_PER_VARIANT)
    assert variants == set(range(PC.N_VARIANTS))


@pytest.mark.parametrize("prefix", ["he-24-", "fuzz-16-", "random-14-", "noisy-spread-9", "cand-20-all_live-5", "edge-"])
def test_compiling_a_case_twice_gives_the_same_text(prefix):
    cases = [c for c in PC.cases() if c.name.startswith(prefix)]
    assert cases
    for case in cases:
        assert PC.compile_text(case) == _corpus()[case.name], case.name
