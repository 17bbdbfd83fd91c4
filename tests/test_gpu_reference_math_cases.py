"""The reference's tests/test_math.py:36-163 cases through qml_essentials_amd.math (x64, the reference
runs them with jax_enable_x64), with their inputs and tolerances.  The Model and Script cases must take
the GPU route (math.last_path), not the finite-difference fallback."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from qml_essentials_amd import math as qm  # noqa: E402
from qml_essentials_amd.math import fubini_study_metric, quantum_fisher_information  # noqa: E402
from qml_essentials_amd.model import Model  # noqa: E402
from qml_essentials_amd.operations import CX, RX, RY  # noqa: E402
from qml_essentials_amd.script import Script  # noqa: E402
from qml_essentials_amd.utils import x64_scope  # noqa: E402


@pytest.fixture(autouse=True)
def _x64():
    with x64_scope(True):
        yield


def test_qfi_model_state():
    model = Model(n_qubits=2, n_layers=1, circuit_type="Hardware_Efficient")
    model.execution_type = "state"
    F = quantum_fisher_information(lambda p: model(params=p), model.params)
    assert qm.last_path == "gpu"
    P = model.params.size
    assert F.shape == (P, P)
    assert np.allclose(F, F.T, atol=1e-7)
    assert np.min(np.linalg.eigvalsh(F)) >= -1e-6


def test_fubini_study_model_state():
    model = Model(n_qubits=2, n_layers=1, circuit_type="Hardware_Efficient")
    model.execution_type = "state"
    params = model.params
    g = fubini_study_metric(lambda p: model(params=p), params)
    assert qm.last_path == "gpu"
    F = quantum_fisher_information(lambda p: model(params=p), params)
    assert qm.last_path == "gpu"
    P = params.size
    assert g.shape == (P, P)
    assert np.allclose(F, 4.0 * g, atol=1e-7)


def test_qfi_model_density():
    model = Model(n_qubits=2, n_layers=1, circuit_type="Hardware_Efficient")
    model.execution_type = "density"
    F = quantum_fisher_information(lambda p: model(params=p, noise_params={"BitFlip": 0.1}), model.params)
    assert qm.last_path == "gpu"
    P = model.params.size
    assert F.shape == (P, P)
    assert np.allclose(F, F.T, atol=1e-7)
    assert np.min(np.linalg.eigvalsh(F)) >= -1e-6
    # the same number through the fallback (a wrapper the capture does not accept)
    F_fd = quantum_fisher_information(lambda p: np.array(model(params=p, noise_params={"BitFlip": 0.1})),
                                      model.params)
    assert qm.last_path == "fallback"
    np.testing.assert_allclose(F, F_fd, atol=1e-6)


def test_qfi_jaqsi_circuit():
    def state_fn(theta):
        def circuit(t):
            RX(t[0], wires=0)
            RY(t[1], wires=1)
            CX(wires=[0, 1])

        return Script(circuit, n_qubits=2).execute(type="state", args=(theta,))

    theta = np.array([0.7, 1.3])
    F = quantum_fisher_information(state_fn, theta)
    assert qm.last_path == "gpu"
    g = fubini_study_metric(state_fn, theta)
    assert qm.last_path == "gpu"
    assert np.allclose(F, np.eye(2), atol=1e-10)
    assert np.allclose(F, 4.0 * g, atol=1e-10)


def test_fubini_study_rejects_density_model():
    model = Model(n_qubits=2, n_layers=1, circuit_type="Hardware_Efficient")
    model.execution_type = "density"
    with pytest.raises(ValueError):
        fubini_study_metric(lambda p: model(params=p, noise_params={"BitFlip": 0.1}), model.params)
