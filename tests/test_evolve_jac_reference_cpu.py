"""CPU: the NumPy restatement of ``qmle_evolve_magnus_jac`` (``tests/evolve_jac_reference.py``) is right -- its
derivative slots equal central differences of ``evolution_reference.magnus`` -- and its seeded cases tell every
named wrong variant apart; the entry point's argument refusals need no device.

Figures (printed by the tests).  Central differences with the step 1e-5 / max(1, max |dh_k / h|) per direction agree
with the restatement to 1.9e-8 at worst over the seeded cases (truncation of the difference quotient, h^2 f''' / 6 with
third derivatives of order 100); the bar is 2e-7.  The nearest wrong variant lies 0.034 x column_scale away."""
import ctypes as C

import numpy as np
import pytest

import evolution_reference as ER
import evolve_jac_reference as J
from qml_essentials_amd import _native as N

CASES = J.seeded_cases()
IDS = [c["name"] for c in CASES]


def _args(c):
    return c["H"], c["coef"], c["h"], c["dcoef"], c["dh"], c["order"]


@pytest.fixture(scope="module")
def right():
    """The restatement on every seeded case, lanes 1 and 4: computed once."""
    return {(c["name"], lanes): J.magnus_jac(*_args(c), lanes=lanes) for c in CASES for lanes in (1, 4)}


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_slot_zero_is_the_forward_scheme_and_the_slots_are_its_derivatives(c, right):
    ref = right[c["name"], 1]
    U = ER.magnus(c["H"], c["coef"], c["h"], c["order"])
    e_u = np.abs(ref[:, 0] - U).max()
    worst = 0.0
    for k in range(c["dcoef"].shape[1]):
        eps = 1e-5 / max(1.0, np.abs(c["dh"][:, k] / c["h"]).max())
        up = ER.magnus(c["H"], c["coef"] + eps * c["dcoef"][:, k], c["h"] + eps * c["dh"][:, k], c["order"])
        dn = ER.magnus(c["H"], c["coef"] - eps * c["dcoef"][:, k], c["h"] - eps * c["dh"][:, k], c["order"])
        worst = max(worst, np.abs((up - dn) / (2 * eps) - ref[:, 1 + k]).max())
    print(c["name"], "U against expm:", e_u, "slots against central differences:", worst)
    assert e_u <= 1e-12
    assert worst <= 2e-7


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_lane_split_changes_the_result_through_rounding_only(c, right):
    a, b = right[c["name"], 1], right[c["name"], 4]
    assert (np.abs(a - b).max(axis=(0, 2, 3)) <= 1e-13 * J.column_scale(a)).all()


@pytest.mark.parametrize("c", [c for c in CASES if c["dim"] == 2], ids=[n for n in IDS if n.startswith("dim2")])
def test_dim_2_in_long_double_agrees_with_float64(c, right):
    hi = J.magnus_jac(*_args(c), dtype=np.longdouble)
    assert hi.dtype == np.clongdouble
    err = np.abs(hi - right[c["name"], 1]).max(axis=(0, 2, 3)) / J.column_scale(right[c["name"], 1])
    print(c["name"], "float64 against long double:", err.max())
    assert (err <= 1e-13).all()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_every_wrong_variant_is_told_apart(c, right):
    """Every applicable variant, in every derivative slot, at least 1e-6 x column_scale away (the project's
    separation bar); slot 0 (U itself) is the same for all of them."""
    cut = J.is_cut(c["H"], c["coef"], c["h"], c["order"])
    assert cut or c["dim"] == 2  # (the seeded 4x4 cases do cut their exponents)
    seen = set()
    for lanes in (1, 4):
        ref = right[c["name"], lanes]
        scale = J.column_scale(ref)
        for v in J.VARIANTS:
            if not J.variant_applies(v, c["dim"], c["order"], lanes, cut):
                continue
            wrong = J.magnus_jac(*_args(c), lanes=lanes, variant=v)
            sep = (np.abs(wrong - ref).max(axis=(0, 2, 3)) / scale)[1:].min()
            print(c["name"], "lanes", lanes, v, "separation", sep)
            assert sep >= 1e-6, (v, lanes, sep)
            seen.add(v)
    want = {v for v in J.VARIANTS if any(J.variant_applies(v, c["dim"], c["order"], lanes, cut) for lanes in (1, 4))}
    assert seen == want


def test_series_counts_follow_the_norm_alone():
    assert J.series_counts(np.zeros((4, 4), dtype=complex)) == (0.0, 1, 1)
    nu, parts, n = J.series_counts(np.diag([0.5, 0, 0, 0]).astype(complex))
    assert (nu, parts) == (0.5, 1) and 14 <= n <= 24
    nu, parts, n = J.series_counts(np.diag([7.3, 0, 0, 0]).astype(complex))
    assert parts == 15 and nu / parts <= 0.5


def test_the_entry_point_refuses_bad_arguments_before_touching_a_device():
    """Status codes decided on the host: the device pointers below point nowhere and are never read."""
    fn = N.lib().qmle_evolve_magnus_jac
    H = np.ascontiguousarray(np.stack([ER.X, ER.Z]))
    hp, p, null = C.c_void_p(H.ctypes.data), C.c_void_p(0x1000), C.c_void_p(None)

    def call(h_terms=hp, n_terms=2, dim=2, coef=p, h=p, dcoef=p, dh=p, rows=3, n_dirs=2, order=4, n_steps=8, lanes=0,
             out=p):
        return fn(h_terms, n_terms, dim, coef, h, dcoef, dh, rows, n_dirs, order, n_steps, lanes, out, null)

    UNSUPPORTED, INVALID = -10, -1
    assert call(dim=3) == UNSUPPORTED and call(dim=8) == UNSUPPORTED
    assert call(order=3) == UNSUPPORTED
    for kw in (dict(h_terms=null), dict(coef=null), dict(h=null), dict(dcoef=null), dict(dh=null), dict(out=null),
               dict(n_terms=0), dict(n_terms=17), dict(rows=0), dict(n_steps=0), dict(n_dirs=0), dict(n_dirs=65),
               dict(lanes=2), dict(lanes=128), dict(dim=4, lanes=64),
               dict(rows=1 << 27, n_dirs=64), dict(rows=1 << 26, n_dirs=2, lanes=16)):
        assert call(**kw) == INVALID, kw
    assert N.lib().qmle_sv_version() == 150


def test_the_new_kernels_use_no_scratch_and_spill_nothing():
    """``kernel_resources.json`` (written by the build): the four instantiations of ``k_evolve_magnus_jac`` are there,
    without scratch or spills, at two waves per SIMD or more; the sweep's LDS kernel keeps its occupancy."""
    import json
    import os

    with open(os.path.join(os.path.dirname(N.__file__), "kernel_resources.json")) as f:
        res = json.load(f)
    jac = {k: v for k, v in res.items() if "k_evolve_magnus_jac" in k}
    assert len(jac) == 4
    for name, v in jac.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, name
        assert v["Occupancy"] >= 2 and v["VGPRs"] + v["AGPRs"] <= 256, (name, v)
    lds = {k: v for k, v in res.items() if "k_adjoint_lds" in k}
    assert len(lds) == 4 and all(v["Occupancy"] >= 4 and v["ScratchSize"] == 0 for v in lds.values())
