"""GPU: ``coefficients.FourierTree`` on the device route against its host route, batches against single calls, and the
analytic spectrum of a circuit with 4 x 10^20 leaves against the complex128 engine.

Device and host walk the same tables in float64 and differ by rounding only; their difference is held to
``8 P 2^-53 A(omega)`` (``tests/test_fourier_tree_cpu.py``).  A comes from the node-by-node interpreter, which is run for the three shallow
models; the four deep ones are held to 1e-12 (``fourier_tree_models.DEEP``), tighter than the formula there.
"""
import numpy as np
import pytest

import fourier_dag_reference as R
from fourier_tree_models import DEEP, SEVEN, SEVEN_IDS, make
from qml_essentials_amd import coefficients as CO
from qml_essentials_amd.coefficients import FourierTree
from qml_essentials_amd.model import Model

pytestmark = pytest.mark.gpu

EPS = 2.0**-53


@pytest.mark.parametrize("ansatz, n_qubits, n_layers", SEVEN, ids=SEVEN_IDS)
def test_device_coefficients_equal_host_coefficients(ansatz, n_qubits, n_layers):
    model = make(ansatz, n_qubits, n_layers)
    tree = FourierTree(model)
    assert tree._resolve_evaluate(None) == "device"
    dev, freqs = tree.get_spectrum()
    host, freqs_host = tree.get_spectrum(evaluate="host")
    assert np.array_equal(freqs[0], freqs_host[0]) and dev[0].shape == freqs[0].shape
    err = np.abs(dev[0] - host[0])
    if (ansatz, n_qubits, n_layers) in DEEP:
        bound = np.full(err.shape, 1e-12)
    else:
        dag = tree._ensure_dag()
        angles, _, _ = tree._canonical_angles(tree._params, np.ones(1))
        A = R.interpret(dag.nodes, tree._levels(True), dag.roots, dag.root_phase, dag.dims, angles, absolute=True)
        flat = [i for i in range(dag.masks[0].bit_length()) if (dag.masks[0] >> i) & 1]
        bound = 8 * tree.n_params * EPS * A[0, 0, flat]
    print(f"{ansatz}-{n_qubits}q-{n_layers}l: {tree._dag.n_nodes} nodes, {len(freqs[0])} frequencies, "
          f"max |device - host| {err.max():.2e}")
    assert np.all(err <= bound), (err.max(), bound.min())
    assert abs(np.sum(dev[0]).imag) < 1e-12


def test_a_batch_equals_single_calls_in_one_launch():
    model = make("Hardware_Efficient", 4, 2, output_qubit=-1)
    tree = FourierTree(model)
    model.initialize_params(repeat=5)
    params = np.array(model.params)
    before = CO.TREE_LAUNCHES
    coeffs, freqs = tree.get_spectrum(params=params)
    assert CO.TREE_LAUNCHES == before + 1  # five parameter sets, four roots: one call of the entry point
    assert len(coeffs) == 4 and all(c.shape == (5, len(f)) for c, f in zip(coeffs, freqs))
    for b in range(5):
        single, _ = tree.get_spectrum(params=params[b:b + 1])
        assert all(np.array_equal(c[b], s[0]) for c, s in zip(coeffs, single))
    assert CO.TREE_LAUNCHES == before + 6
    host, _ = tree.get_spectrum(params=params, evaluate="host")
    assert CO.TREE_LAUNCHES == before + 6
    assert all(np.max(np.abs(c - h)) < 1e-13 for c, h in zip(coeffs, host))
    # values: a batch of inputs times a batch of parameter sets, laid out like the model's result
    xs = np.array([[0.3], [-2.0]])
    before = CO.TREE_LAUNCHES
    values = tree(params=params, inputs=xs)
    assert CO.TREE_LAUNCHES == before + 1 and values.shape == (2, 5, 4)
    want = np.asarray(model(params=params, inputs=xs))
    assert want.shape == values.shape and np.allclose(values, want, atol=1e-5)


def test_analytic_spectrum_of_a_deep_circuit_equals_the_complex128_engine():
    """Strongly_Entangling, 4 qubits, 4 layers: 4 x 10^20 leaves, ~1.3 x 10^4 merged nodes.  ``sum c_w e^{iwx}`` of the
    device coefficients against ``Model(..., x64=True)`` at 4 inputs: both are 1e-12-class against the dense value."""
    model = Model(n_qubits=4, n_layers=4, circuit_type="Strongly_Entangling", output_qubit=0, x64=True)
    tree = FourierTree(model, evaluate="device", max_leaves=1000)
    with pytest.raises(CO.FourierTreeTooLarge, match='method="dp"'):
        tree.leaf_arrays  # (the explicit tree is out of reach; nothing numeric needs it)
    coeffs, freqs = tree.get_spectrum()
    c, f = coeffs[0], np.asarray(freqs[0])
    assert 10000 < tree._dag.n_nodes < 20000
    xs = np.random.default_rng(3).uniform(-np.pi, np.pi, size=4)
    series = np.array([np.sum(c * np.exp(1j * f * x)) for x in xs])
    want = np.asarray(model(params=model.params, inputs=xs.reshape(-1, 1)), dtype=np.float64).reshape(-1)
    print("max |series - x64 model|", np.abs(series.real - want).max())
    assert np.max(np.abs(series.imag)) < 1e-11
    assert np.max(np.abs(series.real - want)) < 1e-11
    assert np.max(np.abs(tree(params=model.params, inputs=xs.reshape(-1, 1)) - want)) < 1e-11
