"""CPU: the NumPy schemes that the GPU tests compare the pulse kernels with (``tests/pulse_reference.py``,
``tests/pulse_jac_reference.py``) against the independent 40-digit reference of ``tests/pulse_mp_reference.py`` -- on and
off resonance, at steps on both sides of the series switch, at zeros of sinc and at the 2^15 norm bound -- and the
three wrong variants that only a run with omega_c != omega_q can see.  Nothing here touches the GPU.

Bar.  Every slot's distance over its column scale (``pulse_jac_reference.column_scale``: 1 for U, max(1, max |column|)
for a derivative slot) stays under 2.5e-13, a quarter of the GPU tests' 1e-12: the NumPy schemes then serve as the
kernels' reference at that bar.  Worst measured: 9.6e-14 on resonance (order 2; 4.8e-14 at order 4), 5.0e-14 detuned,
7.9e-14 at w x 30, 2.4e-16 for the single steps (``profiles/qoc.md``).
"""
import numpy as np
import pytest

import pulse_jac_reference as PJ
import pulse_mp_reference as MP
import pulse_reference as P

SEED, N_SOLVES, N_STEPS = 5, 7, 37  # (the cases of tests/test_qoc_cpu.py)
ROWS = (0, 1, 4)  # an RX, an RY, and w < 0; for square / cosine rows 1 and 4 are the ties width == T
QUARTER_BAR = 2.5e-13
RESONANT = (P.OMEGA, P.OMEGA)
DETUNED = ((10 * np.pi, 9 * np.pi), (9 * np.pi, 10 * np.pi), (10 * np.pi, 0.0), (7.3, 31.0))

SINGLE_STEP_W = MP.SINGLE_STEP_W  # one step with r = |w| exactly: both sides of the series switch, up to 2^15


def scaled_distance(got, want):
    """[6]: max |got - want| per slot over the column scale of ``want``."""
    return np.abs(got - want).max(axis=(0, 2, 3)) / PJ.column_scale(want)


def test_the_picked_rows_are_what_the_cases_need():
    for envelope in P.ENVELOPES:
        solves = P.seeded_solves(envelope, SEED, N_SOLVES)
        assert [int(solves[r, 5]) for r in ROWS] == [0, 1, 0] and solves[4, 3] < 0 < solves[0, 3]
        if envelope in ("square", "cosine"):
            assert solves[0, 1] < solves[0, 4] and solves[1, 1] == solves[1, 4] and solves[4, 1] == solves[4, 4]


@pytest.mark.parametrize("order", (2, 4))
@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("envelope", P.ENVELOPES)
def test_numpy_schemes_against_mpmath_on_and_off_resonance(envelope, mode, order):
    """``drive`` is compared with the product form too: the two are one function."""
    solves = P.seeded_solves(envelope, SEED, N_SOLVES)[list(ROWS)]
    for oc, oq in (RESONANT,) + DETUNED:
        want = MP.reference(envelope, mode, solves, order, N_STEPS, oc, oq)
        J = PJ.scheme_jac(envelope, mode, solves, order, N_STEPS, omega_c=oc, omega_q=oq)
        U = P.scheme(envelope, mode, solves, order, N_STEPS, omega_c=oc, omega_q=oq)
        d, dU = scaled_distance(J, want), np.abs(U - want[:, 0]).max()
        print(envelope, mode, order, "omega_c, omega_q = %.4g, %.4g:" % (oc, oq), "scheme_jac worst slot", d.max(),
              "scheme", dU)
        assert (d <= QUARTER_BAR).all(), (oc, oq, d)
        assert dU <= QUARTER_BAR, (oc, oq, dU)
        if envelope != "drag":
            assert not want[:, 3].any() and not J[:, 3].any()


def test_single_steps_on_both_sides_of_the_series_switch_and_up_to_the_norm_bound():
    solves = MP.single_step_rows()
    J = PJ.scheme_jac("square", "rwa", solves, 2, 1)
    U = P.scheme("square", "rwa", solves, 2, 1)
    want = MP.reference("square", "rwa", solves, 2, 1, *RESONANT)
    assert np.isfinite(J).all()  # (32768 is within the bound)
    for k, w in enumerate(SINGLE_STEP_W):
        d = scaled_distance(J[k:k + 1], want[k:k + 1])
        print("w = %.17g:" % w, "worst slot", d.max(), "scale", PJ.column_scale(want[k:k + 1]).max())
        assert (d <= QUARTER_BAR).all(), (w, d)
    assert PJ.column_scale(want).max() >= 3e4  # (dU/dT of the largest steps)
    # The plain scheme goes through scipy's scaling-and-squaring expm, whose rounding grows with the exponent's norm
    # (about norm x 2^-52: 1.3e-12 at 3e4).  It is held to the bar where the GPU tests use it, at norms of a few
    # radians; the device test of these single steps compares with mpmath directly.
    dU = np.abs(U - want[:, 0]).max(axis=(1, 2))
    print("plain scheme (scipy expm) per w:", dU)
    small = np.abs(SINGLE_STEP_W) <= 2 * np.pi
    assert dU[small].max() <= QUARTER_BAR
    assert np.array_equal(J[0, 0], np.eye(2))  # w = 0


@pytest.mark.parametrize("factor", (1e-6, 30.0))
def test_every_step_in_the_series_branch_and_steps_in_the_division_branch(factor):
    """The gaussian ``lab`` rows with w scaled: x 1e-6 leaves every step's r below 0.05, x 30 takes steps far above it
    (x 300 would exceed the bar by the scheme's own rounding, 6.6e-13: it is not a case)."""
    solves = P.seeded_solves("gaussian", SEED, N_SOLVES)[list(ROWS)]
    solves[:, 3] *= factor
    for order in (2, 4):
        h = P.support("gaussian", solves) / N_STEPS
        cx, cy = P.coefficients("gaussian", "lab", solves[:, None, :], P.ER.node_times(np.zeros(3), h, N_STEPS, order))
        r = np.hypot(cx, cy) * h[:, None]  # (order 4: an exponent is a weighted sum of two nodes, |a1| + |a2| < 1)
        if factor < 1:
            assert r.max() < 0.05 / 2
        else:
            assert (r.max(axis=1) > 10 * 0.05).all()
        want = MP.reference("gaussian", "lab", solves, order, N_STEPS, *RESONANT)
        d = scaled_distance(PJ.scheme_jac("gaussian", "lab", solves, order, N_STEPS), want)
        print("gaussian lab, w x", factor, "order", order, "largest node |c| h", r.max(), "worst slot", d.max())
        assert (d <= QUARTER_BAR).all(), d
        assert np.abs(P.scheme("gaussian", "lab", solves, order, N_STEPS) - want[:, 0]).max() <= QUARTER_BAR


@pytest.mark.parametrize("variant", PJ.DETUNED_VARIANTS)
def test_detuned_wrong_variants_are_invisible_on_resonance_and_told_apart_off_it(variant):
    """On resonance the three variants ARE the right scheme, bit for bit: the term they get wrong is multiplied by
    omega_c - omega_q = 0 or by sin(0 t) = 0, or exchanges two equal numbers.  That is the gap that the suite had while
    every test ran at omega_c = omega_q.  At (10 pi, 9 pi) every row is at least 1e-6 away in some slot (the margin of
    ``test_every_wrong_variant_is_told_apart`` in tests/test_qoc_cpu.py)."""
    mode = "lab" if variant == "lab_kt_swapped" else "drive"
    oc, oq = DETUNED[0]
    least = np.inf
    for envelope in P.ENVELOPES:
        assert PJ.variant_applies(variant, envelope, mode)
        solves = P.seeded_solves(envelope, SEED, N_SOLVES)
        for order in (2, 4):
            right = PJ.scheme_jac(envelope, mode, solves, order, N_STEPS)
            wrong = PJ.scheme_jac(envelope, mode, solves, order, N_STEPS, variant=variant)
            assert np.abs(wrong - right).max() == 0.0, (envelope, order)
            right = PJ.scheme_jac(envelope, mode, solves, order, N_STEPS, omega_c=oc, omega_q=oq)
            wrong = PJ.scheme_jac(envelope, mode, solves, order, N_STEPS, variant=variant, omega_c=oc, omega_q=oq)
            apart = np.abs(wrong - right).max(axis=(1, 2, 3))  # per row, the slot that differs most
            least = min(least, apart.min())
            assert (apart >= 1e-6).all(), (envelope, order, apart)
            if variant != "drive_sd_sign":
                assert np.array_equal(wrong[:, 0], right[:, 0])  # (the time derivative of the carrier is not in U)
            else:  # the plain scheme has the same hook
                U = P.scheme(envelope, mode, solves, order, N_STEPS)
                assert np.array_equal(P.scheme(envelope, mode, solves, order, N_STEPS, variant=variant), U)
                U = P.scheme(envelope, mode, solves, order, N_STEPS, omega_c=oc, omega_q=oq)
                Uw = P.scheme(envelope, mode, solves, order, N_STEPS, variant=variant, omega_c=oc, omega_q=oq)
                assert (np.abs(Uw - U).max(axis=(1, 2)) >= 1e-6).all(), (envelope, order)
    print(variant, "least distance of a row at (10 pi, 9 pi):", least)


def test_mpmath_reference_holds_the_side_of_the_base_point():
    """At the tie width == T the T slot carries the grid term and the width slot does not; one ulp below, the
    reverse -- as ``include/qmle_sv.h`` states it."""
    tie = P.seeded_solves("square", SEED, N_SOLVES)[1:2]
    assert tie[0, 1] == tie[0, 4]
    at = MP.reference("square", "lab", tie, 4, 8, *DETUNED[0])
    below = tie.copy()
    below[0, 1] = np.nextafter(below[0, 1], 0.0)
    under = MP.reference("square", "lab", below, 4, 8, *DETUNED[0])
    assert not at[0, 2].any() and np.abs(at[0, 5]).max() > 1e-3
    assert not under[0, 5].any() and np.abs(under[0, 2] - at[0, 5]).max() <= 1e-9
