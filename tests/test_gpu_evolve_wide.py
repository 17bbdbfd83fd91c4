"""GPU: ``qmle_evolve_magnus_wide`` (dim 8 and 16) against the NumPy scheme of tests/evolution_reference.py.

Bars: ``max |U - reference| <= 1e-12`` and ``max |U^H U - I| <= 1e-12``, the project's complex128 bar;
tests/test_wide_gates_cpu.py shows the reference within 1e-13 of a 40-digit evaluation (a margin of 10) and every
case below at least 1e-6 away from every wrong variant of the scheme that the case can show."""
import numpy as np
import pytest

import evolution_reference as R
import wide_gate_reference as W
from qml_essentials_amd import _native as N

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = W.solver_cases()


@pytest.mark.parametrize("name,dim,n_terms,rows,n_steps,order", CASES, ids=[c[0] for c in CASES])
def test_kernel_matches_the_numpy_scheme_at_every_lane_count(name, dim, n_terms, rows, n_steps, order):
    c = W.solver_case(dim, n_terms, rows, n_steps, order)
    want = R.magnus(c["H"], c["coef"], c["h"], order)
    H = torch.from_numpy(c["H"]).cuda()  # (device terms: uploaded once for all lane counts)
    results = {}
    for lanes in W.SOLVER_LANES[dim]:
        got = N.evolve_magnus_wide(H, c["coef"], c["h"], order, lanes_per_row=lanes).cpu().numpy()
        err = np.abs(got - want).max()
        uni = np.abs(np.einsum("rji,rjk->rik", got.conj(), got) - np.eye(dim)).max()
        print(name, "lanes", lanes, "err", err, "unitarity", uni)
        assert got.dtype == np.complex128 and got.shape == (rows, dim, dim)
        assert err <= 1e-12, (name, lanes, err)
        assert uni <= 1e-12, (name, lanes, uni)
        results[lanes] = got
    first = results[W.SOLVER_LANES[dim][0]]
    for lanes, got in results.items():  # the split changes the result through rounding only
        assert np.abs(got - first).max() <= 1e-12, (name, lanes)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("dim", [8, 16])
def test_a_row_over_the_norm_limit_is_nan_and_its_neighbours_are_not(dim, order):
    c = W.solver_case(dim, 16, 3, 5, order)
    coef, h = c["coef"].copy(), c["h"].copy()
    coef[1] *= 1.0e6  # h |sum c_i H_i| (largest absolute row sum) far beyond 2^15 in every step of row 1
    bad = coef.copy()
    bad[2, 0, 0] = np.nan   # and a row whose table holds a NaN
    want = R.magnus(c["H"], c["coef"], c["h"], order)
    for lanes in W.SOLVER_LANES[dim]:
        got = N.evolve_magnus_wide(c["H"], coef, h, order, lanes_per_row=lanes).cpu().numpy()
        assert np.isnan(got[1]).all(), lanes
        assert np.abs(got[[0, 2]] - want[[0, 2]]).max() <= 1e-12, lanes
        got = N.evolve_magnus_wide(c["H"], bad, h, order, lanes_per_row=lanes).cpu().numpy()
        assert np.isnan(got[1]).all() and np.isnan(got[2]).all(), lanes
        assert np.abs(got[0] - want[0]).max() <= 1e-12, lanes


@pytest.mark.parametrize("dim", [8, 16])
def test_exponents_beyond_the_series_radius_are_cut_into_parts(dim):
    """One step of order 2 with a constant term is exp(-i t H): norms from 0 to ~40 (up to 80 parts)."""
    from scipy.linalg import expm

    rng = np.random.default_rng(dim)
    a = rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim))
    Hm = (a + a.conj().T) / (2.0 * np.linalg.norm(a, 2))
    t = np.array([0.0, 1e-9, 0.3, -2.0, 7.3, 40.0])
    got = N.evolve_magnus_wide(Hm[None], np.ones((6, 1, 1)), t, 2).cpu().numpy()
    want = np.stack([expm(-1j * x * Hm) for x in t])
    assert np.abs(got - want).max() <= 1e-12


def test_only_the_diagonal_and_what_lies_above_it_is_read():
    """The terms are taken as Hermitian, as by qmle_evolve_magnus: garbage below the diagonal and in the
    imaginary part of the diagonal changes nothing."""
    c = W.solver_case(8, 16, 3, 5, 4)
    want = N.evolve_magnus_wide(c["H"], c["coef"], c["h"], 4).cpu().numpy()
    H = c["H"].copy()
    low = np.tril_indices(8, -1)
    H[:, low[0], low[1]] = 7.0 - 3.0j
    H[:, np.arange(8), np.arange(8)] += 5.0j
    got = N.evolve_magnus_wide(H, c["coef"], c["h"], 4).cpu().numpy()
    assert np.array_equal(got, want)
