"""The reference's ``tests/test_coefficients.py`` analytic cases (TestFourierTree) with its own models and assertions.
The FFT coefficients they are compared with come from the complex64 engine: ``atol=1e-5``, as there."""
import numpy as np
import pytest

from fourier_tree_models import scaled_model, two_feature_rotation_model
from qml_essentials_amd.coefficients import Coefficients, FourierTree
from qml_essentials_amd.model import Model

pytestmark = pytest.mark.gpu


def _compare_with_fft(model, tree, fft_coeffs, fft_freqs, analytical_coeffs, analytical_freqs, force_mean):
    """The assertions of test_coefficients.py:430-468.  The reference keeps the FFT coefficients that ``isclose`` does
    not call zero (atol 1e-8) and compares those with the analytic list; the complex64 engine leaves 1e-8-sized noise
    on the coefficients that vanish, so here the analytic coefficients are placed on the FFT's frequency axis and
    EVERY FFT coefficient is compared, at the case's own atol=1e-5: the vanishing ones must be within 1e-5 of 0."""
    fft_coeffs, fft_freqs = np.asarray(fft_coeffs), np.asarray(fft_freqs)
    placed = np.zeros(fft_coeffs.shape, dtype=np.complex128).reshape(len(fft_freqs), -1)
    assert placed.shape[1] == len(analytical_coeffs)
    for r, (c, f) in enumerate(zip(analytical_coeffs, analytical_freqs)):
        for value, w in zip(c, np.asarray(f)):
            (at,) = np.flatnonzero(fft_freqs == w)
            placed[at, r] = value
    assert np.isclose(sum(np.sum(c) for c in analytical_coeffs).imag, 0.0, atol=1.0e-5), "Imaginary part is not zero"
    assert np.isclose(fft_coeffs.reshape(placed.shape), placed, atol=1.0e-5).all(), \
        "FFT and analytical coefficients are not equal."
    analytical_coeffs = np.stack(analytical_coeffs).T
    for ref_input in np.linspace(-np.pi, np.pi, 10):
        exp_fft = Coefficients.evaluate_Fourier_series(coefficients=fft_coeffs, frequencies=fft_freqs, inputs=ref_input)
        exp_fourier = Coefficients.evaluate_Fourier_series(coefficients=analytical_coeffs,
                                                           frequencies=analytical_freqs[0], inputs=ref_input)
        exp_tree = tree(inputs=ref_input, force_mean=force_mean)
        assert np.isclose(exp_fft, exp_fourier, atol=1.0e-5).all(), "FFT and analytical Fourier series do not match"
        assert np.isclose(exp_tree, exp_fourier, atol=1.0e-5).all(), "Analytic Fourier series evaluation not working"


@pytest.mark.parametrize("circuit_type, n_qubits, n_layers, output_qubit",
                         [("Circuit_1", 3, 1, [0, 1]), ("Circuit_9", 4, 1, 0), ("Circuit_19", 3, 1, 0)],
                         ids=["Circuit_1-3q", "Circuit_9-4q", "Circuit_19-3q"])
def test_coefficients_tree(circuit_type, n_qubits, n_layers, output_qubit):
    """test_coefficients.py:402-468."""
    model = Model(n_qubits=n_qubits, n_layers=n_layers, circuit_type=circuit_type, output_qubit=output_qubit)
    fft_coeffs, fft_freqs = Coefficients.get_spectrum(model, shift=True, force_mean=False)
    tree = FourierTree(model)
    coeffs, freqs = tree.get_spectrum()
    _compare_with_fft(model, tree, fft_coeffs, fft_freqs, coeffs, freqs, force_mean=False)


def test_coefficients_tree_mq():
    """test_coefficients.py:470-523: every qubit measured, mean over the roots."""
    model = Model(n_qubits=3, n_layers=1, circuit_type="Hardware_Efficient", output_qubit=-1)
    fft_coeffs, fft_freqs = Coefficients.get_spectrum(model, shift=True)
    tree = FourierTree(model)
    coeffs, freqs = tree.get_spectrum(force_mean=True)
    assert len(coeffs) == len(freqs) == 1
    _compare_with_fft(model, tree, fft_coeffs, fft_freqs, coeffs, freqs, force_mean=True)


def test_coefficients_tree_multi_feature():
    """test_coefficients.py:525-561."""
    model = Model(n_qubits=3, n_layers=1, circuit_type="Circuit_19", output_qubit=0, encoding=["RX", "RY"])
    assert model.n_input_feat == 2
    tree = FourierTree(model)
    coeffs, freqs = tree.get_spectrum(force_mean=True)
    coeffs, freqs = coeffs[0], np.asarray(freqs[0])
    assert freqs.ndim == 2 and freqs.shape[1] == 2
    assert np.isclose(np.sum(coeffs).imag, 0.0, atol=1.0e-5)
    rng = np.random.default_rng(0)
    for _ in range(8):
        x = rng.uniform(-np.pi, np.pi, size=2)
        series = np.sum(coeffs * np.exp(1j * (freqs @ x)))
        tree_val = tree(inputs=x, force_mean=True)
        model_val = np.mean(model(model.params, inputs=np.array([x])))
        assert np.isclose(np.real(series), model_val, atol=1.0e-5)
        assert np.isclose(tree_val, model_val, atol=1.0e-5)


def test_coefficients_tree_input_scaling():
    """test_coefficients.py:563-620: per-gate scalings 1, 3, 9, found from the tape."""
    model = scaled_model()
    expected = {-13, -11, -7, -5, 5, 7, 11, 13}
    tree = FourierTree(model)
    assert tree.input_scaling[tree.all_input_indices].tolist() == [1, 3, 9]
    coeffs, freqs = tree.get_spectrum()
    coeffs, freqs = np.asarray(coeffs[0]), np.asarray(freqs[0])
    nz = np.abs(coeffs) > 1e-8
    assert set(freqs[nz].astype(int).tolist()) == expected
    assert np.isclose(np.sum(coeffs).imag, 0.0, atol=1.0e-5)
    assert set(np.asarray(model.exact_spectrum()[0]).tolist()) == expected
    fft_coeffs, fft_freqs = Coefficients.get_spectrum(scaled_model(), shift=True)
    # (the reference cuts the FFT at 1e-8 too; the complex64 engine leaves 1e-7 on vanishing coefficients, so the
    # FFT is cut at this file's tolerance -- the eight true coefficients are four orders above it)
    fft_nz = np.abs(np.asarray(fft_coeffs)) > 1e-5
    assert np.min(np.abs(coeffs[nz])) > 1e-3
    assert set(np.asarray(fft_freqs)[fft_nz].astype(int).tolist()) == expected
    with pytest.raises(NotImplementedError, match="scaling"):
        tree.get_exact_support(method="dp")
    rng = np.random.default_rng(0)
    for _ in range(6):
        x = float(rng.uniform(-np.pi, np.pi))
        series = np.real(np.sum(coeffs * np.exp(1j * freqs * x)))
        circ = np.asarray(model(model.params, inputs=np.array([[x]])))
        assert np.isclose(series, circ.reshape(-1)[0], atol=1.0e-5)


def test_coefficients_tree_multi_feature_per_gate_rejected():
    """test_coefficients.py:622-641."""
    with pytest.raises(NotImplementedError, match="single feature"):
        FourierTree(two_feature_rotation_model())


def test_fourier_tree_batched_params():
    """test_coefficients.py:643-667: batched model parameters fall back to the first set, with a warning each time."""
    model = Model(n_qubits=2, n_layers=1, circuit_type="Circuit_19", output_qubit=0)
    model.initialize_params(model.random_key, repeat=4)
    assert model.params.ndim == 3 and model.params.shape[0] == 4
    first_params = np.array(model.params[0])
    with pytest.warns(UserWarning, match="batched"):
        tree = FourierTree(model)
    coeffs, freqs = tree.get_spectrum()
    assert set(np.asarray(freqs[0]).tolist()).issubset(set(int(v) for v in model.frequencies[0]))
    with pytest.warns(UserWarning, match="batched"):
        val_tree = tree(inputs=0.5)
    val_model = model(first_params, inputs=np.array([[0.5]]))
    assert np.isclose(val_tree, val_model, atol=1.0e-5).all()


def test_exact_support_dp_matches_tree():
    """test_coefficients.py:669-685."""
    for circuit_type in ["Circuit_19", "Hardware_Efficient"]:
        model = Model(n_qubits=3, n_layers=1, circuit_type=circuit_type, output_qubit=0)
        tree = FourierTree(model)
        for st, sd in zip(tree.get_exact_support(method="tree"), tree.get_exact_support(method="dp")):
            assert set(np.asarray(st).tolist()) == set(np.asarray(sd).tolist()), circuit_type


def test_exact_support_dp_upper_bound():
    """test_coefficients.py:687-707."""
    model = Model(n_qubits=1, n_layers=2, circuit_type="No_Ansatz", data_reupload=True, encoding="RX", output_qubit=0)
    tree = FourierTree(model)
    sup_tree = set(np.asarray(tree.get_exact_support("tree")[0]).tolist())
    sup_dp = set(np.asarray(tree.get_exact_support("dp")[0]).tolist())
    assert sup_tree == {-2, 2}
    assert sup_dp == {-2, 0, 2}
    assert sup_tree.issubset(sup_dp)


def test_exact_support_dp_deep_circuit():
    """test_coefficients.py:709-740: 4 x 10^20 leaves; the merged walk contains every FFT-significant frequency."""
    model = Model(n_qubits=4, n_layers=4, circuit_type="Strongly_Entangling", output_qubit=0)
    tree = FourierTree(model)
    union = set()
    for sup in tree.get_exact_support(method="dp"):
        union |= set(np.asarray(sup).tolist())
    naive = set(int(v) for v in model.frequencies[0])
    assert union.issubset(naive)
    fft_coeffs, fft_freqs = Coefficients.get_spectrum(model, shift=True, force_mean=True)
    significant = {int(f) for f, c in zip(np.asarray(fft_freqs).ravel(), np.asarray(fft_coeffs).ravel())
                   if abs(c) > 1e-4}
    assert significant.issubset(union)
