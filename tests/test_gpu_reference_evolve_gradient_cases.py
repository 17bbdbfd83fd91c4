"""GPU: the reference's ``TestEvolve.test_evolve_parametrized_differentiable`` (``tests/test_jaqsi.py``) with its
inputs and its assertion: the gradient of ``<X>`` through ``ph.evolve()([p], 1.0)``, ``f(p, t) = p`` on Z after a
Hadamard, is ``-2 sin 2p`` at ``atol = 1e-4``.  Where the reference takes ``jax.grad`` through ``Script.execute``, this
project takes ``Script.vjp(pauli_seed=True, through_evolve=True)`` with the cotangent 1."""
import numpy as np
import pytest

from qml_essentials_amd import operations as op
from qml_essentials_amd import utils
from qml_essentials_amd.script import Script

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("x64", [False, True])
def test_evolve_parametrized_differentiable(x64):
    def coeff(p, t):
        return p

    Z = op.PauliZ._matrix

    def circuit(p_val):
        op.H(wires=0)  # prepare |+>
        ph = coeff * op.Hermitian(matrix=Z, wires=0, record=False)
        ph.evolve()([p_val], 1.0)

    p_val = np.array(0.5)
    with utils.x64_scope(x64):
        (grad,) = Script(f=circuit).vjp([op.PauliX(0)], np.array([1.0]), args=(p_val,), pauli_seed=True,
                                        through_evolve=True)
    # <X> = cos(2p) for H exp(-ipZ)|0>, so d<X>/dp = -2 sin(2p)
    expected_grad = -2.0 * np.sin(2.0 * p_val)
    assert np.shape(grad) == ()
    assert np.allclose(grad, expected_grad, atol=1e-4), f"Grad: {grad}, expected: {expected_grad}"
