"""Adjoint gradients for Pauli-word and Hermitian observables: the seed ``lambda = H psi``
(``qmle_apply_pauli_sum``) against NumPy, ``Script.vjp`` against the parameter-shift Jacobian of the same
engine and against an independent oracle, the cotangent / observable forms, and the term-list sweep against
the Z sweep on all-Z lists."""
import numpy as np
import pytest

from oracle import einsum_sim as OE
from qml_essentials_amd import _native as N
from qml_essentials_amd import adjoint, jaqsi
from qml_essentials_amd import operations as op
from qml_essentials_amd.script import Script
from qml_essentials_amd.utils import x64_scope

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


# ---- the seed against NumPy ----------------------------------------------------------------------------
def word(s):
    """'XIYZ' (wire 0 first) -> (x_wire_mask, z_wire_mask)"""
    x = sum(1 << w for w, p in enumerate(s) if p in "XY")
    z = sum(1 << w for w, p in enumerate(s) if p in "ZY")
    return x, z


def terms_of(entries):
    return [(c, *word(s), o) for c, s, o in entries]


def pos(mask, n):
    return sum(1 << (n - 1 - w) for w in range(n) if (mask >> w) & 1)


def apply_numpy(psi, terms, weights, n):
    """out[b][i] = sum_t w[b][obs_t] coef_t i^ny (-1)^popc((i ^ x) & z) psi[b][i ^ x] by index permutation"""
    idx = np.arange(1 << n)
    out = np.zeros_like(psi, dtype=np.complex128)
    for coef, xw, zw, o in terms:
        x, z = pos(xw, n), pos(zw, n)
        ny = bin(x & z).count("1")
        par = np.zeros(1 << n, dtype=np.int64)
        v = (idx ^ x) & z
        while v.any():
            par ^= v & 1
            v >>= 1
        out += (weights[:, o, None] * coef * (1j ** ny)) * (1.0 - 2.0 * par) * psi[:, idx ^ x]
    return out


def pad(s, n, at=0):
    return "I" * at + s + "I" * (n - at - len(s))


def seed_cases():
    """(id, n, [(coef, word, observable)]); 3 observables everywhere: 0 and 1 share a word, 2 has no term"""
    cases = [
        ("n1", 1, [(0.7, "X", 0), (-0.4, "X", 1), (1.1, "Y", 0), (0.3, "Z", 1), (0.25, "I", 1)]),
        ("n2", 2, [(0.7, "XX", 0), (-0.4, "XX", 1), (1.1, "YY", 0), (0.3, "YZ", 1), (-0.6, "ZX", 0),
                   (0.2, "IY", 1), (0.9, "ZI", 0)]),
        ("n3", 3, [(0.7, "YYY", 0), (-0.4, "YYY", 1), (1.1, "XYZ", 0), (0.3, "YYI", 1), (-0.6, "IIX", 0),
                   (0.2, "ZZZ", 1), (0.9, "YIZ", 0), (0.5, "IXY", 1)]),
    ]
    for n in (12, 13):
        cases.append((f"n{n}", n, [
            (0.7, pad("XYZ", n, 2), 0), (-0.4, pad("XYZ", n, 2), 1),                     # shared, ny = 1
            (1.1, pad("YXY", n, n - 3), 0),                                              # ny = 2, Y on the last wire
            (0.3, pad("YYZY", n, 5), 1),                                                 # ny = 3
            (-0.6, pad("X", n, n - 1), 0),                                               # X on the last wire
            (0.2, pad("ZIZ", n, 0), 1), (0.9, "I" * n, 0),                               # diagonal
            (0.5, "X" + "I" * (n - 2) + "X", 1), (-0.8, "Y" * n, 0), (0.35, "X" * n, 1),  # widest supports
        ]))
    n = 14
    ten = [(0.3 + 0.1 * k, pad("X", n, n - 1 - p), k % 2) for k, p in enumerate(range(4, 14))]  # positions 4..13
    cases.append(("n14_two_passes", n, ten + [(0.7, pad("X", n, n - 1 - 4), 1), (0.4, pad("ZYZ", n, 9), 0),
                                              (-0.2, pad("ZZ", n, 0), 1)]))
    cases.append(("n14_streamed", n, [(0.7, "X" * n, 0), (-0.4, "X" * n, 1), (1.1, "Y" * n, 0)]))
    cases.append(("n14_tile_then_streamed", n, [(0.7, "X" * n, 0), (-0.4, "X" * n, 1), (1.1, "Y" * n, 0),
                                                (0.6, "XZ" + "Y" * (n - 3) + "X", 1), (0.3, pad("ZZ", n, 3), 0),
                                                (0.5, pad("Y", n, n - 1), 1)]))
    return cases


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128], ids=["c64", "c128"])
@pytest.mark.parametrize("case", seed_cases(), ids=lambda c: c[0])
def test_seed_equals_the_index_permutation_formula(case, dtype):
    """|err| <= 4 n_words eps sum_t |w coef| max|psi| per sample (eps = 2^-24 / 2^-53): an output element is a
    sum of at most n_words products of a rounded coefficient and an amplitude.  Two calls give the same bits."""
    _, n, entries = case
    terms = terms_of(entries)
    B, n_obs = 3, 3
    rng = np.random.default_rng(100 + n)
    psi = rng.standard_normal((B, 1 << n)) + 1j * rng.standard_normal((B, 1 << n))
    psi = (psi / np.linalg.norm(psi, axis=1, keepdims=True)).astype(dtype)
    rtype = np.float32 if dtype == np.complex64 else np.float64
    w = rng.uniform(-1.5, 1.5, (B, n_obs)).astype(rtype)           # a different weight row per sample
    want = apply_numpy(psi.astype(np.complex128), terms, w.astype(np.float64), n)
    st = torch.from_numpy(psi).cuda()
    got_t = N.apply_pauli_sum(st, terms, torch.from_numpy(w).cuda())
    again = N.apply_pauli_sum(st, terms, torch.from_numpy(w).cuda())
    assert got_t.dtype == st.dtype and torch.equal(got_t, again)
    assert torch.equal(st.cpu(), torch.from_numpy(psi))            # the states are read only
    got = got_t.cpu().numpy().astype(np.complex128)
    eps = 2.0 ** -24 if dtype == np.complex64 else 2.0 ** -53
    n_words = len({(x, z) for _, x, z, _ in terms})
    assert N.apply_pauli_reads(n, terms) >= 1
    for b in range(B):
        bound = 4 * n_words * eps * sum(abs(w[b, o] * c) for c, _, _, o in terms) * np.abs(psi[b]).max()
        err = np.abs(got[b] - want[b]).max()
        print(case[0], dtype.__name__, "sample", b, "err", err, "bound", bound)
        assert err <= bound, (case[0], b, err, bound)


# ---- Script.vjp against the parameter-shift Jacobian of the same engine -----------------------------------
def hermitian(rng, k):
    a = rng.standard_normal((2 ** k, 2 ** k)) + 1j * rng.standard_normal((2 ** k, 2 ** k))
    return (a + a.conj().T) / 2


def observables(n, rng):
    """[X(0), Y(n // 2), Hermitian on wires [n // 5, 3 n // 5], Z(n - 1)] and the product word X0 Y1 Z2 (as far as
    the register has the wires): at n = 15 these are X0, Y7, Hermitian[3, 9], Z14."""
    hw = sorted({n // 5, (3 * n) // 5})
    obs = [op.PauliX(wires=0, record=False), op.PauliY(wires=n // 2, record=False),
           op.Hermitian(matrix=hermitian(rng, len(hw)), wires=hw, record=False),
           op.PauliZ(wires=n - 1, record=False)]
    if n >= 3:
        obs.append(op.prod(op.PauliX(wires=0, record=False), op.PauliY(wires=1, record=False),
                           op.PauliZ(wires=2, record=False)))
    elif n == 2:
        obs.append(op.prod(op.PauliX(wires=0, record=False), op.PauliY(wires=1, record=False)))
    return obs


def big15(th):  # the circuit of test_gpu_gradients.test_adjoint_tiny_registers_and_streaming_path
    for q in range(15):
        op.RY(th[q], wires=q)
    for q in range(14):
        op.CRX(th[15 + q], wires=[q, q + 1])
    op.ControlledPhaseShift(th[29], wires=[14, 0]); op.RXX(th[30], wires=[3, 9])
    op.Rot(th[31], th[32], th[33], wires=7)


def layered(n):
    """RX / RY / RZ / CX / CRX only (what the fused k_tile_adj sweep takes); 3 n + (n - 1) angles"""
    def circuit(th):
        for q in range(n):
            op.RX(th[q], wires=q); op.RY(th[n + q], wires=q)
        for q in range(n - 1):
            op.CX(wires=[q, q + 1])
        for q in range(n):
            op.RZ(th[2 * n + q], wires=q)
        for q in range(n - 1):
            op.CRX(th[3 * n + q], wires=[q + 1, q])
    return circuit, 4 * n - 1


def watch_sweeps(monkeypatch):
    """Wrap ``N.adjoint_gradient``: the returned list gets, per call, the ``N.Unsupported`` it raised or None.
    ``adjoint.run_sweep`` hides a refusal of the fused plan behind the streaming sweep; this shows it."""
    calls, inner = [], N.adjoint_gradient

    def wrapped(*args, **kwargs):
        try:
            out = inner(*args, **kwargs)
        except N.Unsupported as e:
            calls.append(e)
            raise
        calls.append(None)
        return out

    monkeypatch.setattr(N, "adjoint_gradient", wrapped)
    return calls


@pytest.mark.parametrize("n", [1, 2, 4, 13, 14, 15])
def test_vjp_equals_parameter_shift_jacobian(n, monkeypatch):
    """The comparison of tests/test_gpu_gradients.py for Z, with its tolerances: 4e-6 max(1, sum|cot|) where
    the whole sweep runs in LDS (n <= 13), 1e-5 max(1, sum|cot|) from 14 qubits on (n = 14: fused k_tile_adj
    passes -- the sweep's first call is not refused; n = 15: the per-gate streaming sweep, the tape has gates the
    fused passes do not take)."""
    calls = watch_sweeps(monkeypatch)
    rng = np.random.default_rng(40 + n)
    circuit, n_th = (big15, 34) if n == 15 else layered(n)
    s = Script(circuit, n_qubits=n)
    obs = observables(n, rng)
    th = rng.uniform(0, 6.28, n_th)
    cot = rng.normal(size=len(obs))
    (jac,) = s.gradient(obs, args=(th,))
    (g,) = s.vjp(obs, cot, args=(th,), pauli_seed=True)
    atol = (4e-6 if n <= 13 else 1e-5) * max(1.0, np.abs(cot).sum())
    err = np.abs(g - cot @ jac).max()
    print("n", n, "max |vjp - cot @ jacobian|", err, "atol", atol)
    assert g.shape == (n_th,) and err <= atol
    assert calls and (n != 14 or calls[0] is None), calls


# ---- Script.vjp against an independent oracle --------------------------------------------------------------
def oracle_tape(n, th):
    """RX / RY / RZ / CX only: the same gates for Script and for the einsum oracle"""
    tape, k = [], 0
    for layer in range(2):
        for q in range(n):
            for g in ("RX", "RY", "RZ"):
                tape.append((g, [q], (th[k],)))
                k += 1
        for q in range(layer, n - 1, 2):
            tape.append(("CX", [q, q + 1], ()))
        tape.append(("CX", [n - 1, 0], ()))
    return tape


def oracle_cost(n, th, mats, cot):
    """sum_o cot_o <psi| M_o |psi> with psi from the einsum oracle (complex128) and <M> by NumPy"""
    return state_cost(OE.simulate_and_measure(oracle_tape(n, th), n, "state", (), np.complex128), n, mats, cot)


def state_cost(psi, n, mats, cot):
    """sum_o cot_o <psi| M_o |psi> of a complex128 state of 2^n amplitudes (tests/adjoint_reference.py shares it)"""
    t = psi.reshape((2,) * n)
    c = 0.0
    for (m, wires), w in zip(mats, cot):
        k = len(wires)
        r = np.tensordot(m.reshape((2,) * (2 * k)), t, axes=(list(range(k, 2 * k)), wires))
        r = np.moveaxis(r, list(range(k)), wires)
        c += w * np.vdot(psi, r.reshape(-1)).real
    return c


_ORACLE = {}


def oracle_gradient(n):
    """(th, observables, cot, exact gradient): every gate is exp(-i theta P / 2), so the two-term shift
    dC/dtheta = (C(theta + pi/2) - C(theta - pi/2)) / 2 is exact.  Computed once per size."""
    if n not in _ORACLE:
        rng = np.random.default_rng(70 + n)
        th = rng.uniform(0, 6.28, 6 * n)
        obs = observables(n, rng)
        mats = [(np.asarray(o.matrix, dtype=np.complex128), list(o.wires)) for o in obs]
        cot = rng.normal(size=len(obs))
        grad = np.zeros_like(th)
        for k in range(th.size):
            d = np.zeros_like(th)
            d[k] = np.pi / 2
            grad[k] = (oracle_cost(n, th + d, mats, cot) - oracle_cost(n, th - d, mats, cot)) / 2
        _ORACLE[n] = (th, obs, cot, grad)
    return _ORACLE[n]


def script_of_oracle_tape(n):
    def circuit(th):
        for name, wires, params in oracle_tape(n, th):
            getattr(op, name)(*params, wires=wires if len(wires) > 1 else wires[0])
    return Script(circuit, n_qubits=n)


@pytest.mark.parametrize("n", [4, 10])
def test_vjp_equals_the_oracle_gradient(n):
    th, obs, cot, want = oracle_gradient(n)
    s = script_of_oracle_tape(n)
    (g32,) = s.vjp(obs, cot, args=(th,), pauli_seed=True)
    with x64_scope(True):
        (g64,) = s.vjp(obs, cot, args=(th,), pauli_seed=True)
        if n == 4:
            (jac64,) = s.gradient(obs, args=(th,))
    e32, e64 = np.abs(g32 - want).max(), np.abs(g64 - want).max()
    print("n", n, "float32 sweep err", e32, "x64 sweep err", e64)
    assert e32 <= 4e-6 * max(1.0, np.abs(cot).sum())
    assert e64 <= 1e-12
    if n == 4:  # the x64 parameter-shift Jacobian contracted by hand, as tests/test_gpu_x64.py does for Z
        assert np.abs(g64 - cot @ jac64).max() <= 1e-13


# ---- cotangent and observable forms ----------------------------------------------------------------------
def test_stacked_cotangents_and_batching_equal_separate_calls():
    n = 4
    rng = np.random.default_rng(9)
    circuit, n_th = layered(n)
    s = Script(circuit, n_qubits=n)
    obs = observables(n, rng)
    TH = rng.uniform(0, 6.28, (5, n_th))
    WK = rng.normal(size=(3, 5, len(obs)))
    (gk,) = s.vjp(obs, WK, args=(TH,), in_axes=(0,), pauli_seed=True)
    assert gk.shape == (3, 5, n_th)
    (jac,) = s.gradient(obs, args=(TH,), in_axes=(0,))
    for k in range(3):
        (g1,) = s.vjp(obs, WK[k], args=(TH,), in_axes=(0,), pauli_seed=True)
        assert np.allclose(gk[k], g1, atol=1e-6)
        assert np.allclose(g1, np.einsum("bk,bkp->bp", WK[k], jac), atol=4e-6 * max(1.0, np.abs(WK[k]).sum(axis=1).max()))
        for b in (0, 4):
            (gb,) = s.vjp(obs, WK[k, b], args=(TH[b],), pauli_seed=True)
            assert np.allclose(g1[b], gb, atol=1e-6)


def test_33_z_parities_equal_two_calls_of_the_z_seed():
    n = 6
    circuit, n_th = layered(n)
    s = Script(circuit, n_qubits=n)
    groups = [[q] for q in range(n)] + [[a, b] for a in range(n) for b in range(a + 1, n)] \
        + [[a, b, c] for a in range(n) for b in range(a + 1, n) for c in range(b + 1, n)]
    obs = [op.PauliZ(wires=g[0], record=False) if len(g) == 1 else jaqsi.build_parity_observable(g)
           for g in groups[:33]]
    rng = np.random.default_rng(11)
    th, w = rng.uniform(0, 6.28, n_th), rng.normal(size=33)
    (g33,) = s.vjp(obs, w, args=(th,))
    (g32,) = s.vjp(obs[:32], w[:32], args=(th,))
    (g1,) = s.vjp(obs[32:], w[32:], args=(th,))
    assert np.abs(g33 - (g32 + g1)).max() <= 1e-6


# ---- the Z sweep and the term-list sweep on all-Z lists -------------------------------------------------------
@pytest.mark.parametrize("n", [10, 15])
def test_term_list_sweep_equals_the_z_sweep_on_z_observables(n):
    """Straight at the native layer (adjoint_slot_gradient hands both forms to N.adjoint_gradient): the seeds
    differ only in summation order -- 2e-6 sum|w|."""
    rng = np.random.default_rng(20 + n)
    circuit, n_th = (big15, 34) if n == 15 else layered(n)
    s = Script(circuit, n_qubits=n)
    groups = [[0], [n - 1], [1, n // 2], [0, 2, n - 2]]
    obs = [op.PauliZ(wires=g[0], record=False) if len(g) == 1 else jaqsi.build_parity_observable(g) for g in groups]
    th = rng.uniform(0, 6.28, n_th)
    _tape, low, _n, B, slots, _shapes, _batched = s._trace_for_gradient(obs, (th,), None, None, (0,))
    want = [False] * low.n_slots
    for slot, *_ in slots:
        want[slot] = True
    w = rng.normal(size=(2, len(groups))).astype(np.float32)
    terms = [(1.0, 0, sum(1 << q for q in g), k) for k, g in enumerate(groups)]
    for row in w:
        old = adjoint.adjoint_slot_gradient(low, n, B, groups, row[None], want)
        new = adjoint.adjoint_slot_gradient(low, n, B, None, row[None], want, obs_terms=terms)
        err = np.abs(old - new).max()
        print("n", n, "max |Z sweep - term-list sweep|", err)
        assert old.shape == new.shape and err <= 2e-6 * np.abs(row).sum()
