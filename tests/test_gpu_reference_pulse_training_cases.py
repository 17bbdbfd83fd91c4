"""The reference's two pulse-training tests (``tests/test_model.py``: ``test_pulse_model``,
``test_pulse_mode_training``) restated on this package: where the reference takes ``jax.grad`` of a cost through
``model(..., gate_mode="pulse")`` with respect to ``params`` and ``pulse_params``, this package returns the
vector-Jacobian product of the outputs with the cost's derivative (``Model.gradient(cotangent=...)``) from one trace
and one backward sweep; the Adam step is written out in NumPy (first step of optax.adam: ``m / (1 - b1) = g``,
``v / (1 - b2) = g^2``, and so on)."""
import time

import numpy as np
import pytest

from qml_essentials_amd.coefficients import Datasets
from qml_essentials_amd.gates import PulseInformation
from qml_essentials_amd.model import Model

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_state():
    PulseInformation.reset_defaults()
    yield
    PulseInformation.reset_defaults()


class Adam:
    """optax.adam(lr): b1 = 0.9, b2 = 0.999, eps = 1e-8, bias-corrected moments"""

    def __init__(self, lr, shapes):
        self.lr, self.t = lr, 0
        self.m = [np.zeros(s) for s in shapes]
        self.v = [np.zeros(s) for s in shapes]

    def step(self, values, grads):
        self.t += 1
        out = []
        for k, (x, g) in enumerate(zip(values, grads)):
            self.m[k] = 0.9 * self.m[k] + 0.1 * g
            self.v[k] = 0.999 * self.v[k] + 0.001 * g * g
            m_hat, v_hat = self.m[k] / (1 - 0.9 ** self.t), self.v[k] / (1 - 0.999 ** self.t)
            out.append(x - self.lr * m_hat / (np.sqrt(v_hat) + 1e-8))
        return out


def mse_gradient(model, params, pulse_params, x, y):
    """d mean((y_hat - y)^2) / d(params, pulse_params), y_hat = the mean over the model's outputs"""
    y_hat = np.asarray(model(params=params, pulse_params=pulse_params, inputs=x, force_mean=True, gate_mode="pulse"),
                       dtype=np.float64).reshape(-1)
    n_out = model.n_qubits
    cot = np.repeat((2.0 * (y_hat - y) / y.size / n_out)[:, None], n_out, axis=1)
    g_p, g_s = model.gradient(params=params, pulse_params=pulse_params, inputs=x, gate_mode="pulse", method="adjoint",
                              wrt=("params", "pulse_params"), cotangent=cot)
    return g_p.sum(axis=0).reshape(np.shape(params)), g_s.sum(axis=0).reshape(np.shape(pulse_params))


def test_pulse_model():
    model = Model(n_qubits=2, n_layers=1, circuit_type="Hardware_Efficient")
    domain = np.array([-np.pi, np.pi])
    omegas = np.array([1, 2, 3, 4])
    coefficients = np.array([1, 1, 1, 1])
    n_d = int(np.ceil(2 * np.max(np.abs(domain)) * np.max(omegas)))
    x = np.linspace(domain[0], domain[1], num=n_d)
    y = np.stack([1 / np.linalg.norm(omegas) * np.sum(coefficients * np.cos(omegas.T * s)) for s in x])

    pulse_params_before = np.array(model.pulse_params, dtype=np.float64)
    params = np.array(model.params, dtype=np.float64)
    grads = mse_gradient(model, params, pulse_params_before, x, y)
    opt = Adam(0.01, [params.shape, pulse_params_before.shape])
    model.params, model.pulse_params = opt.step([params, pulse_params_before], grads)
    pulse_params_after = np.array(model.pulse_params)

    assert not np.allclose(pulse_params_before, pulse_params_after), "pulse_params did not update during training"
    assert np.any(np.abs(grads[1]) > 1e-6), "Gradient wrt pulse_params is too small"


def test_pulse_mode_training():
    PulseInformation.set_rwa(True)
    model = Model(n_qubits=2, n_layers=1, circuit_type="Circuit_1")
    domain_samples, fourier_samples, _coefficients = Datasets.generate_fourier_series(
        random_key=model.random_key, model=model)
    x = np.asarray(domain_samples, dtype=np.float64)
    y = np.asarray(fourier_samples, dtype=np.float64).reshape(-1)
    values = [np.array(model.params, dtype=np.float64), np.array(model.pulse_params, dtype=np.float64)]
    opt = Adam(0.001, [v.shape for v in values])
    first = [v.copy() for v in values]
    start = time.time()
    for _epoch in range(1, 5):
        grads = mse_gradient(model, values[0], values[1], x, y)
        values = opt.step(values, grads)
        model.params, model.pulse_params = values
    end = time.time()
    print(f"Time taken: {end - start}")
    assert end - start < 60, "Time limit of 60 seconds exceeded"
    assert not np.allclose(first[0], values[0]) and not np.allclose(first[1], values[1])
