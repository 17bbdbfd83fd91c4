"""Models shared by the Fourier-tree tests: seven ansatz circuits from 42 to 204 Pauli rotations, whose merged DAGs run
from 6 x 10^2 to 8 x 10^5 nodes, and the two hand-written scripts of the reference's ``TestFourierTree``."""
import warnings

import numpy as np

import qml_essentials_amd.jaqsi as js
from qml_essentials_amd.model import Model
from qml_essentials_amd.operations import PauliRot

# (ansatz, qubits, layers): Pauli rotations 42 .. 204, merged nodes 6 x 10^2 .. 8 x 10^5, leaves up to 4 x 10^20
SEVEN = [("Circuit_19", 3, 2), ("Circuit_19", 4, 2), ("Hardware_Efficient", 4, 2), ("Strongly_Entangling", 4, 4),
         ("Hardware_Efficient", 6, 3), ("Strongly_Entangling", 6, 4), ("Hardware_Efficient", 8, 3)]
# The rounding bound 8 P 2^-53 A needs A = sum over paths of |weight|.  It is below 30 for the first three; the other
# four have A between 10^3 and 10^6 at random parameters (4 x 10^20 leaves cancel down to a number below 1), where the
# formula allows 10^-7 and says little: they are held to 1e-12 instead, which is tighter.  A is computed for the
# smallest of them only (``test_fourier_tree_cpu.py`` asserts that it exceeds 30 there).
DEEP = SEVEN[3:]
SEVEN_IDS = [f"{a}-{q}q-{l}l" for a, q, l in SEVEN]


def make(ansatz, n_qubits, n_layers, **kw):
    kw.setdefault("output_qubit", 0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return Model(n_qubits=n_qubits, n_layers=n_layers, circuit_type=ansatz, **kw)


def scaled_model():
    """Three encoding rotations with the data scalings 1, 3, 9 between two variational ones, no tags: feature and
    scaling must come out of the tape.  Its spectrum is {+-5, +-7, +-11, +-13}."""
    def variational(params, inputs, *args, **kwargs):
        params = params.squeeze()
        PauliRot(1 * inputs, "Y", wires=[0])
        PauliRot(params[0], "XZX", wires=[0, 1, 2])
        PauliRot(3 * inputs, "XZ", wires=[0, 1])
        PauliRot(params[1], "YY", wires=[0, 1])
        PauliRot(9 * inputs, "XY", wires=[0, 1])

    model = Model(n_qubits=3, n_layers=1, output_qubit=0)
    model._params_shape = (2, 1)
    model.initialize_params()
    model.degree = (27,)  # 2 * 13 + 1: the FFT route's sampling grid
    model.script = js.Script(f=variational, n_qubits=3)
    return model


def two_feature_rotation_model():
    """One rotation whose angle mixes two features: the tree must refuse it."""
    def variational(params, inputs, *args, **kwargs):
        params = params.squeeze()
        PauliRot(inputs[..., 0] + inputs[..., 1], "X", wires=[0])
        PauliRot(params[0], "Z", wires=[0])
        PauliRot(params[1], "Z", wires=[1])

    model = Model(n_qubits=2, n_layers=1, output_qubit=0, encoding=["RX", "RY"])
    model._params_shape = (2, 1)
    model.initialize_params()
    model.script = js.Script(f=variational, n_qubits=2)
    return model


def dense_values(model, xs, params=None):
    """Dense complex128 expectation values ``[len(xs), n_obs]`` of the model's own script at the inputs ``xs``
    (``[n, d]``), gate by gate from ``Operation.matrix``."""
    from fourier_dag_reference import dense_expectations
    from qml_essentials_amd.tape import recording

    params = np.asarray(model.params if params is None else params, dtype=np.float64)
    _, obs = model._build_obs()
    out = []
    for x in np.asarray(xs, dtype=np.float64).reshape(len(xs), -1):
        inputs = model._inputs_validation(x)
        model._zero_inputs = False
        with recording() as tape:
            model.script.f(params.reshape(1, *params.shape[-2:]), inputs, None, None, model._enc_params_validation(None))
        out.append(dense_expectations(tape, obs, model.n_qubits).real)
    return np.array(out)
