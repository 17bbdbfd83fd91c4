"""GPU: the launch shapes, the automatic lane choice, the step regimes and the non-finite-derivative edge of the pulse
kernels -- what ``tests/test_gpu_qoc.py`` (7 solves x 37 steps) and ``tests/test_gpu_pulse.py`` leave open.

* ``qmle_pulse_unitaries_jac`` at every shape of ``tests/test_gpu_pulse.py`` (one solve and one step, fewer steps than
  lanes, 18 blocks, 256 steps), lanes = 0 included: its own combine, its own fold of the norm check and its own idle
  lanes see them all.
* lanes = 0 of ``qmle_evolve_magnus``, ``qmle_pulse_unitaries`` and ``qmle_pulse_unitaries_jac`` on both sides of every
  row count at which ``qmle_evolve_lanes`` changes its answer, bit for bit against the explicit count, and rows across
  the whole table against NumPy.
* single steps with r = |w| on both sides of the series switch r < 0.05, at zeros of sinc and up to the norm bound
  2^15, against the 40-digit reference of ``tests/pulse_mp_reference.py``; one ulp beyond the bound is NaN.
* sigma = 0, T = 0 and width = 0.

Bars.  1e-12, the project's complex128 bar, for U; 1e-12 x ``column_scale`` for the derivative slots
(``tests/test_gpu_qoc.py``).  ``tests/test_pulse_mp_reference_cpu.py`` holds the NumPy schemes within a quarter of that of
the 40-digit reference at these regimes."""
import numpy as np
import pytest

import evolution_reference as ER
import pulse_jac_reference as PJ
import pulse_mp_reference as MP
import pulse_reference as P
from pulse_jac_reference import column_scale
from qml_essentials_amd import _native as N
from test_gpu_pulse import SHAPES

pytestmark = pytest.mark.gpu

BAR = 1e-12


def plain(solves, envelope, mode, order, steps, lanes=0):
    return N.pulse_unitaries(solves, envelope, mode, P.OMEGA, P.OMEGA, order, steps, lanes_per_solve=lanes).cpu().numpy()


def jac(solves, envelope, mode, order, steps, lanes=0):
    return N.pulse_unitaries_jac(solves, envelope, mode, P.OMEGA, P.OMEGA, order, steps,
                                 lanes_per_solve=lanes).cpu().numpy()


# ---- the sensitivity kernel at the plain kernel's shapes ----------------------------------------------------------------
@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("envelope", P.ENVELOPES)
def test_sensitivity_kernel_at_every_shape_of_the_plain_kernel(envelope, mode):
    worst = np.zeros(6)
    for n, steps, lanes_list in SHAPES:
        solves = P.seeded_solves(envelope, 31, n)
        for order in (2, 4):
            want = PJ.scheme_jac(envelope, mode, solves, order, steps)  # (shared by every lane count)
            scale = column_scale(want)
            for lanes in lanes_list:
                got = jac(solves, envelope, mode, order, steps, lanes)
                assert got.shape == (n, 6, 2, 2) and got.dtype == np.complex128
                err = np.abs(got - want).max(axis=(0, 2, 3)) / scale
                worst = np.maximum(worst, err)
                assert (err <= BAR).all(), (n, steps, order, lanes, err)
                d0 = np.abs(got[:, 0] - plain(solves, envelope, mode, order, steps, lanes)).max()
                assert d0 <= BAR, (n, steps, order, lanes, d0)
                if envelope != "drag":
                    assert not got[:, 3].any()  # the p2 slot of a two-parameter envelope
    print(envelope, mode, "worst distance / scale per slot", worst)


# ---- the automatic lane choice --------------------------------------------------------------------------------------------
# (rows, steps, lanes): both sides of every row count at which the choice changes, and steps between two widths
LANE_CASES = [(2048, 64, 64), (2049, 64, 16), (8192, 16, 16), (8193, 16, 4), (32768, 4, 4), (32769, 4, 1), (3, 63, 16)]


def documented_lanes(rows, steps):
    """include/qmle_sv.h: the widest of 4, 16 and 64 lanes with rows x lanes within 256 CUs x 4 SIMDs x 2 waves x 64
    work items and no more lanes than steps; else 1."""
    fits = [c for c in (4, 16, 64) if rows * c <= 256 * 4 * 2 * 64 and c <= steps]
    return max(fits) if fits else 1


def picked_rows(rows):
    """Rows 0, 255, 256 (the first block edge at one lane per row), rows - 1 and 50 seeded others."""
    pick = {0, 255, 256, rows - 1} | set(np.random.default_rng(rows).integers(0, rows, 50).tolist())
    return np.array(sorted(r for r in pick if r < rows))


_TABLE = {}


def drag_table(rows):
    """(A prefix of the longest table: ``seeded_solves`` draws row after row.)"""
    if "drag" not in _TABLE:
        _TABLE["drag"] = P.seeded_solves("drag", 41, max(c[0] for c in LANE_CASES))
    return _TABLE["drag"][:rows]


@pytest.mark.parametrize("rows,steps,lanes", LANE_CASES)
def test_automatic_lanes_of_the_pulse_kernels(rows, steps, lanes):
    assert N.lib().qmle_evolve_lanes(rows, steps) == lanes == documented_lanes(rows, steps)
    solves, pick = drag_table(rows), picked_rows(rows)
    auto, explicit = plain(solves, "drag", "lab", 4, steps, 0), plain(solves, "drag", "lab", 4, steps, lanes)
    assert np.array_equal(auto, explicit)
    d = np.abs(auto[pick] - P.scheme("drag", "lab", solves[pick], 4, steps)).max()
    assert d <= BAR, d
    auto_j, explicit_j = jac(solves, "drag", "lab", 4, steps, 0), jac(solves, "drag", "lab", 4, steps, lanes)
    assert np.array_equal(auto_j, explicit_j)
    want = PJ.scheme_jac("drag", "lab", solves[pick], 4, steps)
    err = np.abs(auto_j[pick] - want).max(axis=(0, 2, 3)) / column_scale(want)
    print(rows, "x", steps, "->", lanes, "lanes; pulse_unitaries", d, "pulse_unitaries_jac / scale", err)
    assert (err <= BAR).all(), err
    assert np.isfinite(auto).all() and np.isfinite(auto_j).all()
    if lanes != 1:  # another count is another order of the products: the comparison above can tell counts apart
        other = plain(solves, "drag", "lab", 4, steps, 1)
        assert not np.array_equal(other, auto) and np.abs(other - auto).max() <= BAR


@pytest.mark.parametrize("rows,steps,lanes", LANE_CASES)
def test_automatic_lanes_of_evolve_magnus(rows, steps, lanes):
    assert N.lib().qmle_evolve_lanes(rows, steps) == lanes == documented_lanes(rows, steps)
    case = ER.case_dim4(12, rows)
    # (5 step lengths beside the 8 scales of the case: 40 different rows before one repeats)
    h = (case["t1"] - case["t0"]) / steps * (1.0 - 0.01 * (np.arange(rows) % 5))
    coef = ER.coef_table(case["fns"], ER.node_times(np.full(rows, case["t0"]), h, steps, 4))
    auto = N.evolve_magnus(case["H"], coef, h, 4, lanes_per_row=0).cpu().numpy()
    explicit = N.evolve_magnus(case["H"], coef, h, 4, lanes_per_row=lanes).cpu().numpy()
    assert auto.shape == (rows, 4, 4) and np.array_equal(auto, explicit)
    pick = picked_rows(rows)
    d = np.abs(auto[pick] - ER.magnus(case["H"], coef[pick], h[pick], 4)).max()
    print(rows, "x", steps, "->", lanes, "lanes; evolve_magnus", d)
    assert d <= BAR, d


# ---- step regimes ---------------------------------------------------------------------------------------------------------
def test_single_steps_across_the_series_switch_and_the_norm_bound():
    """r = |w| exactly (``pulse_mp_reference.single_step_rows``), each row against the 40-digit reference with the
    scale of its own row; one row one ulp beyond 2^15 among them is NaN in all six slots and leaves the others alone."""
    ws = list(MP.SINGLE_STEP_W)
    beyond = 5
    ws.insert(beyond, float(np.nextafter(32768.0, np.inf)))
    solves = MP.single_step_rows(ws)
    keep = np.arange(len(ws)) != beyond
    want = MP.reference("square", "rwa", solves[keep], 2, 1, P.OMEGA, P.OMEGA)
    row_scale = np.stack([column_scale(want[k:k + 1]) for k in range(len(want))])[:, :, None, None]
    worst = 0.0
    for lanes in (1, 4, 0):
        got, U = jac(solves, "square", "rwa", 2, 1, lanes), plain(solves, "square", "rwa", 2, 1, lanes)
        assert np.isnan(got[beyond].real).all() and np.isnan(got[beyond].imag).all() and np.isnan(U[beyond]).all()
        assert np.isfinite(got[keep]).all() and np.isfinite(U[keep]).all()
        err = (np.abs(got[keep] - want) / row_scale).max(axis=(1, 2, 3))
        err_U = np.abs(U[keep] - want[:, 0]).max(axis=(1, 2))
        worst = max(worst, err.max(), err_U.max())
        assert (err <= BAR).all() and (err_U <= BAR).all(), (lanes, err, err_U)
        assert np.array_equal(got[0, 0], np.eye(2))  # w = 0
    print("single steps, worst distance / own scale", worst, "largest scale", row_scale.max())


@pytest.mark.parametrize("factor", (1e-6, 30.0))
def test_every_step_in_the_series_branch_and_steps_in_the_division_branch(factor):
    """The gaussian ``lab`` solves with w scaled (tests/test_pulse_mp_reference_cpu.py has the step sizes): all seven
    rows against NumPy, rows 0, 1 and 4 against the 40-digit reference."""
    solves = P.seeded_solves("gaussian", 5, 7)
    solves[:, 3] *= factor
    rows = [0, 1, 4]
    for order in (2, 4):
        want = PJ.scheme_jac("gaussian", "lab", solves, order, 37)
        exact = MP.reference("gaussian", "lab", solves[rows], order, 37, P.OMEGA, P.OMEGA)
        for lanes in (1, 16):
            got, U = jac(solves, "gaussian", "lab", order, 37, lanes), plain(solves, "gaussian", "lab", order, 37, lanes)
            err = np.abs(got - want).max(axis=(0, 2, 3)) / column_scale(want)
            err_mp = np.abs(got[rows] - exact).max(axis=(0, 2, 3)) / column_scale(exact)
            err_U = np.abs(U[rows] - exact[:, 0]).max()
            print("w x", factor, "order", order, "lanes", lanes, "against NumPy", err.max(), "against mpmath",
                  err_mp.max(), "U", err_U)
            assert (err <= BAR).all() and (err_mp <= BAR).all() and err_U <= BAR, (order, lanes, err, err_mp, err_U)


# ---- non-finite derivatives of a finite solve ------------------------------------------------------------------------------
@pytest.mark.parametrize("envelope,column", [("gaussian", 1), ("sech", 1), ("drag", 2)])
def test_a_zero_sigma_is_non_finite_where_the_numpy_scheme_is(envelope, column):
    """gaussian and sech with sigma = 0: the envelope is 0 at every node, U = I is kept, and the envelope's derivatives
    by sigma and by t are 0 x inf -- the sigma slot and the T slot are not finite, the others are.  drag with
    sigma = 0: the envelope itself is 0 x inf, so the solve fails the norm check and all six slots are NaN."""
    clean = P.seeded_solves(envelope, 5, 3)
    solves = clean.copy()
    solves[1, column] = 0.0
    for mode in ("lab", "rwa"):
        with np.errstate(all="ignore"):
            want = PJ.scheme_jac(envelope, mode, solves, 4, 37)
        finite = np.isfinite(want)
        if envelope == "drag":
            assert not finite[1].any()
        else:
            assert finite[1].all(axis=(1, 2)).tolist() == [True, True, False, True, True, False]
            assert np.array_equal(want[1, 0], np.eye(2))
        scale = column_scale(np.where(finite, want, 0.0))[None, :, None, None]
        for lanes in (1, 16):
            got = jac(solves, envelope, mode, 4, 37, lanes)
            assert np.array_equal(np.isfinite(got), finite), (mode, lanes)
            err = np.abs(np.where(finite, got - np.where(finite, want, 0.0), 0.0)) / scale
            print(envelope, "sigma = 0,", mode, "lanes", lanes, "finite slots of the row",
                  finite[1].all(axis=(1, 2)).tolist(), "worst finite distance / scale", err.max())
            assert err.max() <= BAR, (mode, lanes, err.max())  # U and every finite slot
            assert np.array_equal(got[[0, 2]], jac(clean, envelope, mode, 4, 37, lanes)[[0, 2]])
            U = plain(solves, envelope, mode, 4, 37, lanes)
            assert np.array_equal(np.isfinite(U), finite[:, 0])
            if envelope != "drag":
                assert np.array_equal(U[1], np.eye(2)) and np.array_equal(got[1, 0], np.eye(2))


def test_zero_duration_and_zero_width_are_finite_with_the_identity():
    for envelope, column in (("gaussian", 4), ("square", 1)):
        clean = P.seeded_solves(envelope, 5, 3)
        clean[1, 5] = 0.0  # (an RX: lab's RY carrier vanishes at t = 0, and dU/dT at T = 0 with it)
        solves = clean.copy()
        solves[1, column] = 0.0  # T = 0; width = 0 (the grid ends at the width)
        want = PJ.scheme_jac(envelope, "lab", solves, 4, 37)
        assert np.isfinite(want).all()
        for lanes in (1, 16):
            got = jac(solves, envelope, "lab", 4, 37, lanes)
            assert np.isfinite(got).all() and np.array_equal(got[1, 0], np.eye(2))
            assert np.array_equal(plain(solves, envelope, "lab", 4, 37, lanes)[1], np.eye(2))
            err = np.abs(got - want).max(axis=(0, 2, 3)) / column_scale(want)
            print(envelope, "T = 0" if column == 4 else "width = 0", "lanes", lanes, "against NumPy / scale", err.max())
            assert (err <= BAR).all(), (envelope, lanes, err)
            assert np.array_equal(got[[0, 2]], jac(clean, envelope, "lab", 4, 37, lanes)[[0, 2]])
            if envelope == "gaussian":
                exact = MP.reference("gaussian", "lab", solves[1:2], 4, 37, P.OMEGA, P.OMEGA)
                d = np.abs(got[1:2] - exact).max(axis=(0, 2, 3)) / column_scale(exact)
                print("T = 0, lanes", lanes, "against mpmath per slot", d, "|dU/dT|", np.abs(exact[0, 5]).max())
                assert (d <= BAR).all(), d
                assert np.abs(exact[0, 5]).max() > 1e-2  # (the T slot is not trivially zero)
