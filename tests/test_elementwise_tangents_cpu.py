"""CPU: the elementwise tangent rules of ``batching.elementwise_tangents()`` against central differences on a
``Batched.leaf``, and their absence outside the context.

Bar.  Central differences with step 1e-6 on functions whose third derivatives stay below ~100 on the sampled range
carry 1e-12 x f''' / 6 of truncation and 1e-16 / 1e-6 of rounding: 1e-8 covers both with a factor of ten."""
import numpy as np
import pytest

from qml_essentials_amd.batching import Batched, elementwise_tangents, param_tangent

UFUNCS = [np.sin, np.cos, np.tan, np.exp, np.expm1, np.log, np.log1p, np.sqrt, np.square, np.reciprocal, np.sinh,
          np.cosh, np.tanh, np.arctan]
X = np.array([[0.3, 0.7, 1.1], [0.45, 0.9, 1.3]])  # [B = 2, 3]: inside every function's domain, away from tan's pole
EPS = 1e-6


def tangent_of(fn):
    """(value, d value[b, e] / d leaf[b, e]) of an elementwise ``fn`` from the tangent terms of its result."""
    with elementwise_tangents():
        y = fn(Batched.leaf(X.copy(), 0))
    assert isinstance(y, Batched) and y.tan is not None and y.shape == (3,)
    d = np.zeros_like(X)
    for lid, idx, coef in y.tan:
        assert lid == 0 and np.array_equal(idx, np.arange(3))  # element e depends on leaf element e
        d += coef
    return y.data, d


def central(fn):
    return (fn(X + EPS) - fn(X - EPS)) / (2 * EPS)


@pytest.mark.parametrize("ufunc", UFUNCS, ids=[u.__name__ for u in UFUNCS])
def test_every_listed_ufunc(ufunc):
    val, d = tangent_of(ufunc)
    assert np.array_equal(val, ufunc(X))
    err = np.abs(d - central(ufunc)).max()
    print(ufunc.__name__, err)
    assert err <= 1e-8


@pytest.mark.parametrize("name,fn", [
    ("x ** 3", lambda x: x ** 3),
    ("x ** -0.5", lambda x: x ** -0.5),
    ("np.power(x, 2.5)", lambda x: np.power(x, 2.5)),
    ("2 / x", lambda x: 2.0 / x),
    ("x / (1 + x * x)", lambda x: x / (1.0 + x * x)),
    ("sin(x) / x", lambda x: np.sin(x) / x),
    ("p0 * cos(p1 * t)", lambda x: x * np.cos(1.7 * x)),
    ("exp(-x ** 2 / 2) * tanh(x)", lambda x: np.exp(-x ** 2 / 2.0) * np.tanh(x)),
])
def test_constant_powers_quotients_and_compositions(name, fn):
    val, d = tangent_of(fn)
    assert np.allclose(val, fn(X), rtol=0, atol=1e-15)
    err = np.abs(d - central(fn)).max()
    print(name, err)
    assert err <= 1e-8


def test_two_leaves_and_constants():
    with elementwise_tangents():
        p, t = Batched.leaf(X.copy(), 0), Batched.leaf(X[:, ::-1].copy(), 1)
        y = p[0] * np.cos(p[1] * t[2])
        const = np.sin(Batched(X.copy(), []))
    grads = {0: np.zeros_like(X), 1: np.zeros_like(X)}
    for lid, idx, coef in y.tan:
        grads[lid][:, int(idx)] += coef
    p0, p1, t2 = X[:, 0], X[:, 1], X[:, 0]  # (t[2] is X[:, ::-1][:, 2] = X[:, 0])
    assert np.allclose(grads[0][:, 0], np.cos(p1 * t2), atol=1e-15)
    assert np.allclose(grads[0][:, 1], -p0 * np.sin(p1 * t2) * t2, atol=1e-15)
    assert np.allclose(grads[1][:, 2], -p0 * np.sin(p1 * t2) * p1, atol=1e-15)
    assert const.tan == []


def test_what_stays_unknown_inside_the_context():
    with elementwise_tangents():
        x, y = Batched.leaf(X.copy(), 0), Batched.leaf(X.copy(), 1)
        assert np.arctan2(x, y).tan is None      # more than one tracked input
        assert np.abs(x).tan is None             # a ufunc outside the list
        assert (x ** y).tan is None              # a tracked exponent
        assert np.floor(x).tan is None


def test_outside_the_context_nothing_changed():
    x = Batched.leaf(X[:, :1].copy().reshape(2), 0)
    assert param_tangent(np.sin(x)) is None
    assert param_tangent(x ** 2) is None
    assert param_tangent(1.0 / x) is None
    assert param_tangent(x / x) is None
    assert param_tangent(np.power(x, 2)) is None
    assert param_tangent(np.sin(Batched(X[:, 0].copy(), []))) == []
    assert param_tangent(np.power(Batched(X[:, 0].copy(), []), 2)) == []
    with elementwise_tangents():
        assert param_tangent(np.sin(x)) is not None
    assert param_tangent(np.sin(x)) is None  # (the context restores the state when it ends)
