"""The reference gradient of tests/adjoint_reference.py on its own: its simulation against the oracle's, every
shift rule against a difference quotient of the same complex128 cost, the difference quotient against itself at
twice the step (it is the reference where a gate has no shift rule), and -- for every case the GPU route tests
run below 19 qubits -- that no differentiated angle has a gradient a wrong kernel could hide in."""
import numpy as np
import pytest

from oracle import einsum_sim as OE
from tests import adjoint_reference as R


def four_qubit_tape():
    """every gate kind of the reference on 4 wires, the Golomb encoding and a 2-wire matrix included"""
    rng = np.random.default_rng(5)
    spec = R.everything(4, rng, dense2=True, golomb=True)
    theta = rng.uniform(0.4, 5.9, spec.n_theta)
    theta[R.golomb_angles(spec)] *= 0.005  # (as the cases do: see adjoint_reference._case)
    mats = R.z_mats(R.z_groups(4)) + R.pauli_mats(4, rng)
    w = rng.uniform(0.5, 1.5, len(mats)) * rng.choice([-1.0, 1.0], len(mats))
    return spec, theta, (lambda psi: float(w @ R.expectations(psi, 4, mats)))


def test_the_sliced_gate_product_is_the_oracles_einsum():
    spec, theta, _ = four_qubit_tape()
    tape = R.oracle_tape(spec, theta)
    mine = R.run_from(R.zero_state(4), tape, 4)
    assert np.abs(mine - OE.simulate_pure(tape, 4, np.complex128)).max() <= 1e-15
    rng = np.random.default_rng(6)
    for n in (3, 6):  # every gate of a larger tape, one at a time, on a random state
        spec = R.everything(n, rng, dense2=True, dense4=[4, 1, 5, 2] if n == 6 else None)
        psi = rng.standard_normal(2 ** n) + 1j * rng.standard_normal(2 ** n)
        for name, wires, params in R.oracle_tape(spec, rng.uniform(0, 6, spec.n_theta)):
            k = len(wires)
            want = np.einsum(OE.einsum_subscript(n, k, tuple(wires)),
                             R.G.matrix(name, params).reshape((2,) * (2 * k)), psi.reshape((2,) * n)).reshape(-1)
            assert np.abs(R.apply_gate(psi, (name, wires, params), n) - want).max() <= 1e-14, (name, wires)


def test_every_shift_rule_equals_the_difference_quotient():
    """|rule - D(1e-3)| <= 1e-9 and |D(2e-3) - D(1e-3)| <= 1e-9 for every angle with a rule (frequencies <= 1: the
    quotient's error is |C^(5)| h^4 / 30 ~ 1e-13); for the Golomb angle the same two steps divided by its highest
    frequency -- D at that step IS the reference there, so only its agreement with the doubled step is checked."""
    spec, theta, cost = four_qubit_tape()
    tape_fn = lambda t: R.oracle_tape(spec, t)  # noqa: E731
    steps = {k: R.golomb_step(spec, k) for k in R.golomb_angles(spec)}
    grad = R.reference_gradient(tape_fn, theta, 4, cost, steps=steps)
    kinds = set()
    for name, _w, idx, _c in spec:
        for k in idx:
            h = steps.get(k, 1e-3)
            d1 = R.difference_gradient(tape_fn, theta, 4, cost, k, h)
            d2 = R.difference_gradient(tape_fn, theta, 4, cost, k, 2 * h)
            print(name, "angle", k, "rule", grad[k], "|rule - D(h)|", abs(grad[k] - d1), "|D(2h) - D(h)|", abs(d2 - d1))
            assert abs(grad[k] - d1) <= 1e-9 and abs(d2 - d1) <= 1e-9, (name, k)
            assert abs(grad[k]) >= 1e-3, (name, k)
            kinds.add(name)
    assert kinds == set(R.RULES) | {"Golomb"}


def test_the_golomb_steps_of_the_gpu_cases_agree_with_their_double():
    """the difference quotient as the GPU tests use it: 3 of 5 and 3 of 14 wires (marks up to 44)"""
    for name in ("lds_golomb_n5", "wide_golomb_n14"):
        case = R.cases()[name]
        groups, mats, wz, wp = R.case_observables(case)
        every = R.z_mats(groups) + mats
        w = np.concatenate([wz[0], wp[0]])
        cost = lambda psi: float(w @ R.expectations(psi, case.n, every))  # noqa: E731
        (k,) = R.golomb_angles(case.spec)
        h = R.golomb_step(case.spec, k)
        tape_fn = lambda t: R.oracle_tape(case.spec, t)  # noqa: E731
        d1 = R.difference_gradient(tape_fn, case.theta[0], case.n, cost, k, h)
        d2 = R.difference_gradient(tape_fn, case.theta[0], case.n, cost, k, 2 * h)
        print(name, "step", h, "D(h)", d1, "|D(2h) - D(h)|", abs(d2 - d1))
        assert abs(d2 - d1) <= 1e-9


def test_chain_rule_folds_gate_angles_onto_arguments():
    """angles th[0] * x and th[1] + x on two gates, and th[0] once more on a third: against the difference quotient
    of the cost as a function of the arguments"""
    spec, x, th, angles, tangents = R.chain_case()
    mats = R.pauli_mats(3, np.random.default_rng(9))
    cost = lambda psi: float(R.expectations(psi, 3, mats).sum())  # noqa: E731
    tape_fn = lambda t: R.oracle_tape(spec, t)  # noqa: E731
    g = R.chain_rule(R.reference_gradient(tape_fn, angles(th), 3, cost), tangents, 2)
    for a in range(2):
        def f(s, a=a):
            t = th.copy()
            t[a] += s
            return cost(R.run_from(R.zero_state(3), tape_fn(angles(t)), 3))
        assert abs(g[a] - R.central_difference(f, 1e-3)) <= 1e-9


CPU_CASES = [name for name, c in R.cases().items() if c.n < 19]


@pytest.mark.parametrize("name", CPU_CASES)
def test_no_gpu_case_is_vacuous(name):
    """|dC/dtheta| >= 1e-3 for every differentiated angle, every batch row and both seeds: a wrong sign, a wrong
    coefficient or a dropped block then moves the entry by more than any tolerance of the route tests"""
    case = R.cases()[name]
    gz, gp = R.case_gradients(name)
    assert gz.shape == gp.shape == case.theta.shape and len(case.wanted) >= 1
    lo_z, lo_p = np.abs(gz[:, case.wanted]).min(), np.abs(gp[:, case.wanted]).min()
    print(name, "angles", len(case.wanted), "of", case.spec.n_theta, "gates", len(case.spec),
          "min |dC/dtheta| Z seed", lo_z, "Pauli seed", lo_p)
    assert lo_z >= 1e-3 and lo_p >= 1e-3
    rest = [k for k in range(case.spec.n_theta) if k not in case.wanted]
    assert not gz[:, rest].any() and not gp[:, rest].any()
