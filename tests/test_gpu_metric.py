"""qmle_gram against NumPy, and the quantum geometric tensor / QFI of Script and Model against fp64
oracle differences (oracle/einsum_sim, oracle/noise, oracle/c_port)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import c_port as OCP  # noqa: E402
from oracle import circuits as OC  # noqa: E402
from oracle import einsum_sim as OE  # noqa: E402
from oracle import noise as ON  # noqa: E402
from qml_essentials_amd import _native as N  # noqa: E402
from qml_essentials_amd.ansaetze import Ansaetze  # noqa: E402
from qml_essentials_amd.model import Model  # noqa: E402
from qml_essentials_amd.utils import x64_scope  # noqa: E402


def _rand_states(rng, shape, dtype):
    s = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    s /= np.linalg.norm(s, axis=-1, keepdims=True)
    return s.astype(dtype)


def _check_gram(a, b=None, f64=False):
    ta = torch.from_numpy(a).cuda()
    tb = None if b is None else torch.from_numpy(b).cuda()
    got = N.gram(ta, tb).cpu().numpy()
    a64 = a.astype(np.complex128)
    b64 = a64 if b is None else b.astype(np.complex128)
    want = np.conj(a64) @ np.swapaxes(b64, 1, 2)
    if f64:
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    else:
        bound = np.abs(a64) @ np.swapaxes(np.abs(b64), 1, 2)  # sum |a||b|
        assert np.all(np.abs(got - want) <= 1e-6 * bound + 1e-30)
    if b is None:
        np.testing.assert_array_equal(got, np.conj(np.swapaxes(got, 1, 2)))
    return got


@pytest.mark.parametrize("n", list(range(1, 13)))
def test_gram_small_registers_many_groups(n):
    rng = np.random.default_rng(n)
    groups = 300 if n < 10 else 20
    for rows in (1, 5, 37, 70):
        _check_gram(_rand_states(rng, (groups, rows, 2**n), np.complex64))
        _check_gram(_rand_states(rng, (groups, rows, 2**n), np.complex128), f64=True)


@pytest.mark.parametrize("n,rows_list", [(16, (1, 31, 64, 97, 241)), (20, (1, 31, 64, 97)), (24, (1, 9))])
def test_gram_large_registers(n, rows_list):
    rng = np.random.default_rng(100 + n)
    for rows in rows_list:
        _check_gram(_rand_states(rng, (1, rows, 2**n), np.complex64))
    if n <= 20:
        _check_gram(_rand_states(rng, (1, 31, 2**n), np.complex128), f64=True)


def test_gram_general_form_and_bitwise_repeatability():
    rng = np.random.default_rng(7)
    for n, ra, rb in ((5, 7, 3), (14, 33, 70), (18, 65, 2)):
        a = _rand_states(rng, (2, ra, 2**n), np.complex64)
        b = _rand_states(rng, (2, rb, 2**n), np.complex64)
        g1 = _check_gram(a, b)
        g2 = _check_gram(a, b)
        np.testing.assert_array_equal(g1, g2)
        _check_gram(a.astype(np.complex128), b.astype(np.complex128), f64=True)
    a = torch.from_numpy(_rand_states(rng, (1, 241, 2**20), np.complex64)).cuda()
    np.testing.assert_array_equal(N.gram(a).cpu().numpy(), N.gram(a).cpu().numpy())


def test_gram_n24_entries_against_numpy():
    """n = 24, 73 rows (4.9 GB): 8 rows pulled back to the host and checked entry by entry."""
    rows, D = 73, 2**24
    g = torch.Generator(device="cuda").manual_seed(5)
    s = torch.randn((1, rows, D), dtype=torch.complex64, device="cuda", generator=g)
    got = N.gram(s).cpu().numpy()[0]
    pick = [0, 1, 17, 31, 32, 63, 64, 72]
    host = s[0, pick].cpu().numpy().astype(np.complex128)
    want = np.conj(host) @ host.T
    bound = np.abs(host) @ np.abs(host).T
    sub = got[np.ix_(pick, pick)]
    assert np.all(np.abs(sub - want) <= 1e-6 * bound)
    del s


# ---- model QFI against oracle differences ----
def _oracle_state(spec, params, inputs, dtype=np.complex128):
    return OE.simulate_pure(OC.model_tape(spec, params, inputs), spec.n_qubits, dtype=dtype).reshape(-1)


def _oracle_qfi(state_fn, p0, h=1e-3):
    flat = p0.reshape(-1)
    psi = state_fn(p0)
    cols = []
    for i in range(flat.size):
        f = []
        for k in (2, 1, -1, -2):
            q = flat.copy()
            q[i] += k * h
            f.append(state_fn(q.reshape(p0.shape)))
        cols.append((-f[0] + 8 * f[1] - 8 * f[2] + f[3]) / (12 * h))
    J = np.stack(cols, axis=-1)
    A = np.conj(J.T) @ J
    v = np.conj(J.T) @ psi
    return 4 * np.real(A - np.outer(v, np.conj(v)))


ANSAETZE = [a.__name__ for a in Ansaetze.get_available()]


@pytest.mark.parametrize("name", ANSAETZE)
def test_model_qfi_every_ansatz_against_oracle(name):
    rng = np.random.default_rng(abs(hash(name)) % 1000)
    for n in (4, 5):
        model = Model(n_qubits=n, n_layers=1, circuit_type=name)
        if model.params.size == 0:
            continue
        spec = OC.ModelSpec(n, 1, name)
        p = rng.uniform(0, 2 * np.pi, model.params.shape[1:])
        x = np.array([0.37])
        want = _oracle_qfi(lambda q: _oracle_state(spec, q, x), p)
        got = model.quantum_fisher_information(params=p.astype(np.float32), inputs=x)
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, atol=2e-5)
        with x64_scope(True):
            got64 = model.quantum_fisher_information(params=p, inputs=x)
        np.testing.assert_allclose(got64, want, atol=1e-9)
        np.testing.assert_allclose(model.fubini_study_metric(params=p, inputs=x), got / 4, atol=1e-6)


def test_model_qfi_n6_strongly_entangling_x64():
    rng = np.random.default_rng(6)
    model = Model(n_qubits=6, n_layers=2, circuit_type="Strongly_Entangling")
    spec = OC.ModelSpec(6, 2, "Strongly_Entangling")
    p = rng.uniform(0, 2 * np.pi, model.params.shape[1:])
    x = np.array([0.1])
    want = _oracle_qfi(lambda q: _oracle_state(spec, q, x), p)
    with x64_scope(True):
        got = model.quantum_fisher_information(params=p, inputs=x)
    np.testing.assert_allclose(got, want, atol=1e-10)


def test_batched_params_and_inputs_match_per_point_calls():
    rng = np.random.default_rng(11)
    model = Model(n_qubits=4, n_layers=2, circuit_type="Hardware_Efficient")
    P = rng.uniform(0, 2 * np.pi, (3,) + model.params.shape[1:]).astype(np.float32)
    X = rng.uniform(0, 1, (3, 1)).astype(np.float32)
    got = model.quantum_fisher_information(params=P, inputs=X[0])  # params batched only
    assert got.shape == (3, P[0].size, P[0].size)
    for b in range(3):
        one = model.quantum_fisher_information(params=P[b], inputs=X[0])
        np.testing.assert_allclose(got[b], one, atol=1e-5)
    got_x = model.quantum_fisher_information(params=P[0], inputs=X)  # inputs batched only
    for b in range(3):
        np.testing.assert_allclose(got_x[b], model.quantum_fisher_information(params=P[0], inputs=X[b]),
                                   atol=1e-5)


def test_model_20_qubits_against_c_port():
    rng = np.random.default_rng(20)
    n = 20
    model = Model(n_qubits=n, n_layers=2, circuit_type="Hardware_Efficient")
    spec = OC.ModelSpec(n, 2, "Hardware_Efficient")
    p = rng.uniform(0, 2 * np.pi, model.params.shape[1:])
    x = np.array([0.5])
    got = model.quantum_fisher_information(params=p.astype(np.float32), inputs=x)
    # the same fold on rows computed by the C port: d_i psi by the state rule psi(theta + pi e_i) / 2
    # (every parameter of Hardware_Efficient drives one RY / RZ)
    flat = p.reshape(-1)
    psi = OCP.simulate(OC.model_tape(spec, p, x), n)
    cols = []
    for i in range(flat.size):
        q = flat.copy()
        q[i] += np.pi
        cols.append(OCP.simulate(OC.model_tape(spec, q.reshape(p.shape), x), n) / 2)
    J = np.stack(cols, axis=-1).astype(np.complex128)
    psi = psi.astype(np.complex128)
    v = np.conj(J.T) @ psi
    want = 4 * np.real(np.conj(J.T) @ J - np.outer(v, np.conj(v)))
    np.testing.assert_allclose(got, want, atol=2e-5)


def test_forced_column_block_split_matches_unsplit():
    rng = np.random.default_rng(12)
    model = Model(n_qubits=8, n_layers=2, circuit_type="Strongly_Entangling")
    p = rng.uniform(0, 2 * np.pi, model.params.shape[1:])
    x = np.array([0.2])
    whole = model.quantum_geometric_tensor(params=p.astype(np.float32), inputs=x)
    split = model.quantum_geometric_tensor(params=p.astype(np.float32), inputs=x, row_block=7)
    np.testing.assert_allclose(split, whole, atol=1e-6)
    with x64_scope(True):
        w64 = model.quantum_geometric_tensor(params=p, inputs=x)
        s64 = model.quantum_geometric_tensor(params=p, inputs=x, row_block=5)
    np.testing.assert_allclose(s64, w64, atol=1e-12)


def test_noisy_model_qfi_against_oracle_noise():
    rng = np.random.default_rng(3)
    noise = {"BitFlip": 0.05, "Depolarizing": 0.02}
    model = Model(n_qubits=3, n_layers=1, circuit_type="Hardware_Efficient")
    model.noise_params = noise
    spec = OC.ModelSpec(3, 1, "Hardware_Efficient")
    p = rng.uniform(0, 2 * np.pi, model.params.shape[1:])
    x = np.array([0.3])

    def rho_fn(q):
        return ON.simulate_mixed(ON.with_gate_noise(OC.model_tape(spec, q, x), noise), 3)

    h = 1e-3
    flat = p.reshape(-1)
    cols = []
    for i in range(flat.size):
        f = []
        for k in (2, 1, -1, -2):
            q = flat.copy()
            q[i] += k * h
            f.append(rho_fn(q.reshape(p.shape)))
        cols.append((-f[0] + 8 * f[1] - 8 * f[2] + f[3]) / (12 * h))
    from qml_essentials_amd import math as qm

    want = qm._qfi_density(np.stack(cols, axis=-1), rho_fn(p))
    with x64_scope(True):
        got = model.quantum_fisher_information(params=p, inputs=x)
    np.testing.assert_allclose(got, want, atol=1e-7)
    got32 = model.quantum_fisher_information(params=p.astype(np.float32), inputs=x)
    np.testing.assert_allclose(got32, want, atol=2e-4)
