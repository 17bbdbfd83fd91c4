"""GPU: ``qmle_evolve_magnus_jac`` -- the table-driven Magnus solve with the exact derivative of the grid's result in
given directions -- against the NumPy restatement of ``tests/evolve_jac_reference.py``.

Bars (the project's): 1e-12 for ``U`` and 1e-12 x ``max(1, max |column|)`` per derivative slot
(``pulse_jac_reference.column_scale``)."""
import numpy as np
import pytest
from scipy.linalg import expm

import evolution_reference as R
import evolve_jac_reference as J
from qml_essentials_amd import _native as N

pytestmark = pytest.mark.gpu


def lanes_of(dim):
    """Every lanes_per_row the entry point takes at this dim (a 4x4 run of steps takes four lanes: no 64)."""
    return (0, 1, 4, 16, 64) if dim == 2 else (0, 1, 4, 16)


def check(H, coef, h, dcoef, dh, order, label, want=None):
    want = J.magnus_jac(H, coef, h, dcoef, dh, order) if want is None else want
    scale = J.column_scale(want)
    for lanes in lanes_of(H.shape[-1]):
        got = N.evolve_magnus_jac(H, coef, h, dcoef, dh, order, lanes_per_row=lanes).cpu().numpy()
        assert got.shape == want.shape and got.dtype == np.complex128
        err = np.abs(got - want).max(axis=(0, 2, 3)) / scale
        print(label, "lanes", lanes, "U", err[0], "slots", err[1:].max(), "scale", scale.max())
        assert (err <= 1e-12).all(), (label, lanes, err)
    return want


def table(dim, order, n_steps, rows, n_dirs, seed=11):
    """Per-row t0 and h as tests/test_gpu_evolution.py; directions: random derivatives of the table and the step."""
    c = (R.case_dim2 if dim == 2 else R.case_dim4)(seed, rows)
    t0 = c["t0"] + 0.003 * (np.arange(rows) % 50)
    t1 = c["t1"] + 0.02 * (np.arange(rows) % 31)
    h = (t1 - t0) / n_steps
    coef = R.coef_table(c["fns"], R.node_times(t0, h, n_steps, order))
    rng = np.random.default_rng([dim, order, n_steps, rows, n_dirs])
    dcoef = rng.normal(size=(rows, n_dirs) + coef.shape[1:])
    dh = rng.normal(size=(rows, n_dirs)) / n_steps
    return c["H"], coef, h, dcoef, dh


@pytest.mark.parametrize("n_dirs", [1, 3])
@pytest.mark.parametrize("n_steps,rows", [(1, 70), (3, 64), (63, 5), (65, 3), (257, 2)])
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("dim", [2, 4])
def test_kernel_matches_the_restatement(dim, order, n_steps, rows, n_dirs):
    """Steps around the lane counts (fewer steps than lanes included), rows around the wave, 1 to 3 terms."""
    H, coef, h, dcoef, dh = table(dim, order, n_steps, rows, n_dirs)
    for n_terms in (1, 2, 3):
        pick = [1] if n_terms == 1 else list(range(n_terms))  # (one term alone: the time-dependent one)
        check(H[pick], coef[..., pick], h, dcoef[..., pick], dh, order,
              f"dim{dim} order{order} terms{n_terms} steps{n_steps} rows{rows} dirs{n_dirs}")


def test_lanes_the_entry_point_refuses_at_dim_4():
    H, coef, h, dcoef, dh = table(4, 2, 70, 2, 1)
    with pytest.raises(ValueError):
        N.evolve_magnus_jac(H, coef, h, dcoef, dh, 2, lanes_per_row=64)
    with pytest.raises(ValueError):
        N.evolve_magnus_jac(H, coef, h, dcoef, dh, 2, lanes_per_row=2)


@pytest.mark.parametrize("dim", [2, 4])
def test_permuted_directions_give_bit_identical_permuted_slots(dim):
    """One (row, direction) is one unit of work: a slot does not depend on where it stands in the call."""
    H, coef, h, dcoef, dh = table(dim, 4, 37, 5, 4)
    perm = np.array([2, 0, 3, 1])
    for lanes in lanes_of(dim):
        a = N.evolve_magnus_jac(H, coef, h, dcoef, dh, 4, lanes_per_row=lanes).cpu().numpy()
        b = N.evolve_magnus_jac(H, coef, h, np.ascontiguousarray(dcoef[:, perm]), np.ascontiguousarray(dh[:, perm]), 4,
                                lanes_per_row=lanes).cpu().numpy()
        assert np.array_equal(a[:, 0], b[:, 0])
        assert np.array_equal(a[:, 1 + perm], b[:, 1:])


def test_static_exponential_and_its_time_derivative():
    """One step of order 2 with a constant term and dh = 1: U = exp(-i t H), dU = -i H exp(-i t H) -- t far beyond
    the series' radius (the exponent is cut into parts), negative, tiny and zero."""
    rng = np.random.default_rng(5)
    a = rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4))
    t = np.array([0.0, 1e-9, 0.3, -2.0, 7.3, 40.0])
    for H in ((a + a.conj().T) / 2, R.X + 0.5 * R.Z + 0.25 * np.eye(2)):
        got = N.evolve_magnus_jac(H[None], np.ones((6, 1, 1)), t, np.zeros((6, 1, 1, 1)), np.ones((6, 1)), 2)
        got = got.cpu().numpy()
        U = np.stack([expm(-1j * x * H) for x in t])
        dU = np.stack([-1j * H @ u for u in U])
        scale = max(1.0, np.abs(dU).max())
        print("dim", H.shape[0], "U", np.abs(got[:, 0] - U).max(), "dU", np.abs(got[:, 1] - dU).max() / scale)
        assert np.abs(got[:, 0] - U).max() <= 1e-12
        assert np.abs(got[:, 1] - dU).max() <= 1e-12 * scale


@pytest.mark.parametrize("dim", [2, 4])
def test_a_row_with_a_non_finite_coefficient_is_nan_and_its_neighbours_are_exact(dim):
    H, coef, h, dcoef, dh = table(dim, 4, 9, 6, 2)
    want = J.magnus_jac(H, coef, h, dcoef, dh, 4)
    for bad in (np.nan, np.inf):
        c = coef.copy()
        c[2, 5, 1] = bad
        for lanes in lanes_of(dim):
            got = N.evolve_magnus_jac(H, c, h, dcoef, dh, 4, lanes_per_row=lanes).cpu().numpy()
            assert np.isnan(got[2].real).all() and np.isnan(got[2].imag).all()
            keep = [0, 1, 3, 4, 5]
            assert (np.abs(got[keep] - want[keep]).max(axis=(0, 2, 3)) <= 1e-12 * J.column_scale(want)).all()


@pytest.mark.parametrize("case", J.seeded_cases(), ids=[c["name"] for c in J.seeded_cases()])
def test_kernel_on_the_seeded_cases_that_tell_the_wrong_variants_apart(case):
    """The cases on which tests/test_evolve_jac_reference_cpu.py shows every wrong variant at least 1e-6 x
    column_scale away: agreeing to 1e-12 here rules each of them out."""
    check(case["H"], case["coef"], case["h"], case["dcoef"], case["dh"], case["order"], case["name"])
