"""The adjoint sweep of noisy circuits over vec(rho) (``adjoint.density_gradient``, ``qmle_adjoint_density`` / ``_f64``,
``Script.vjp(noisy=True)``, ``Model.gradient(method="adjoint", noisy=True)``) against the exact complex128 gradient of
tests/density_adjoint_reference.py.

Every row is compared with the metric of tests/test_gpu_adjoint_routes.py, max |sweep - reference| / max(1, sum |w|).
x64: 1e-12.  complex64: the larger of that file's ``tolerance()`` at the DOUBLED wire count (4e-6 up to 13 wires, 1e-5 up
to 16) and four times the reference's own complex64 floor on the tape -- the same shift-rule gradient run with
``dtype=np.complex64`` against its complex128 run; the factor four is the margin for another summation order.  Every
comparison prints both figures and the error it reached."""
import functools
import zlib

import numpy as np
import pytest

from qml_essentials_amd import adjoint
from qml_essentials_amd import operations as op
from qml_essentials_amd.batching import Batched
from qml_essentials_amd.simulation import LoweredTape
from qml_essentials_amd.utils import x64_scope

import density_adjoint_reference as DR
from density_factorised_reference import ONE_WIRE, TWO_WIRE, one_wire_channel as _one_wire_channel
import noise_reference as NR

pytestmark = pytest.mark.gpu

B = 3
WANTED = {5: 12, 7: 12, 8: 12}  # angles differentiated per random tape


def routes_tolerance(n_wires, x64):  # tests/test_gpu_adjoint_routes.py::tolerance
    return 1e-12 if x64 else 4e-6 if n_wires <= 13 else 1e-5


# ---- observables -------------------------------------------------------------------------------------------------
def z_groups(n):
    return [[0], [n - 1], [0, n - 1]]


def pauli_terms(n):
    """X, Y, a product and a two-wire Hermitian as ``(coef, x, z, column)`` on wire masks."""
    a, b = 1 << 0, 1 << (n - 1)
    return [(1.0, a, 0, 0), (1.0, b, b, 1), (1.0, a | b, b, 2),            # X_0, Y_{n-1}, X_0 Y_{n-1}
            (0.4, a, 0, 3), (-0.7, b, 0, 3), (0.5, a | b, a | b, 3), (0.3, 0, a | b, 3)]  # a Hermitian on (0, n-1)


def observables(n, seed):
    if seed == "z":
        groups = z_groups(n)
        return groups, None, [DR.cost_matrix(n, np.eye(len(groups))[k], groups=groups) for k in range(len(groups))]
    terms = pauli_terms(n)
    return None, terms, [DR.cost_matrix(n, np.eye(4)[k], terms=terms) for k in range(4)]


def weights(n_obs, rows, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(rows, n_obs))


# ---- tapes ---------------------------------------------------------------------------------------------------------
def _angles(rng):
    return Batched(rng.uniform(0, 2 * np.pi, size=(B,)), [])


# (gate, wires, channel kind or "pair", n): every wire of n = 2 and n = 3 carries a one-wire step, so bit positions 0 / 1
# and the pair (q, q + n) at every distance occur; control and target in both orders, adjacent and at the ends
STEP_CASES = ([(g, (q,), ch, n) for n in (2, 3) for q in range(n)
               for g, ch in [(("RX", "RY", "RZ")[(q + n) % 3], ("amp", "phase", "bitflip")[q % 3])]]
              + [("Rot", (0,), "amp", 2), ("Rot", (2,), "depol", 3), ("RY", (1,), "phaseflip", 2),
                 ("CRX", (0, 1), "amp", 2), ("CRX", (1, 0), "phase", 2), ("CRY", (0, 2), "amp", 3),
                 ("CRY", (2, 0), "bitflip", 3), ("CRZ", (1, 2), "depol", 3), ("CRZ", (2, 1), "amp", 3),
                 ("CPhase", (0, 1), "phase", 3), ("CPhase", (2, 0), "amp", 3), ("RXX", (0, 2), "amp", 3),
                 ("RXX", (1, 0), "phase", 2), ("CRX", (2, 0), "pair", 3), ("CRZ", (0, 1), "pair", 2),
                 ("RYY", (0, 2), "amp", 3), ("RYY", (1, 0), "phase", 2), ("RZX", (0, 1), "amp", 2),
                 ("RZX", (2, 0), "amp", 3), ("RZX", (1, 2), "pair", 3), ("RZZ", (2, 1), "amp", 3)])


@functools.lru_cache(maxsize=None)
def step_tape(gate, wires, chan, n):
    """RY on every wire, the gate under test, then its channel: a one-wire channel on every wire of the gate, or
    ("pair") the two-wire channel of noise_reference.pair_channel -- a 16 x 16 superoperator -- behind the gate."""
    rng = np.random.default_rng(zlib.crc32(repr((gate, wires, chan, n)).encode()))
    with NR.recording_depolarizing() as (ops, depol):
        for w in range(n):
            op.RY(_angles(rng), wires=w)
            op.AmplitudeDamping(0.1 + 0.05 * w, wires=w)
        if gate == "Rot":
            op.Rot(_angles(rng), _angles(rng), _angles(rng), wires=wires[0])
        elif gate in ONE_WIRE:
            ONE_WIRE[gate](_angles(rng), wires=wires[0])
        else:
            TWO_WIRE[gate](_angles(rng), wires=list(wires))
        if chan == "pair":
            NR.pair_channel(0.1, 0.25, list(wires))
            op.PhaseDamping(0.2, wires=wires[1])
        else:
            for q in wires:
                _one_wire_channel(chan, q)
    return NR.NoisyTape(ops, depol, n)


@functools.lru_cache(maxsize=None)
def random_tape(n):
    # (seeds under which several steps, a two-wire one among them, carry a channel)
    return NR.random_noisy_tape(n, np.random.default_rng({5: 4007, 7: 4010, 8: 4014}[n]), 22, B).without_wide_channels()


@functools.lru_cache(maxsize=None)
def model_noisy_tape():
    """A noisy Circuit_19 model's tape at n = 5, one sample: the B rows differ in their weights."""
    return NR.model_sample_tape("Circuit_19", 5, 2)


def n_slots(tape):
    return LoweredTape([o for o in tape.ops if not isinstance(o, op.KrausChannel)], tape.n).n_slots


def wanted_of(tape, limit):
    """The angle slots a case differentiates: all of them up to ``limit``; of more, first those whose step carries a
    channel (the wrong variants of the reference differ there), then slots spread over the tape."""
    total = n_slots(tape)
    if total <= limit:
        return tuple(range(total))
    steps = adjoint.plan_density(tape.ops, tape.n, [True] * total).steps
    picked = [s[8][0] for s in steps if s[3] >= 0][:limit]
    for k in range(limit):
        s_ = int(round(k * (total - 1) / (limit - 1)))
        if len(picked) < limit and s_ not in picked:
            picked.append(s_)
    return tuple(sorted(picked))


# ---- the reference, once per (tape, row, seed) -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(tape, row, seed, wanted):
    """-> (Jacobian [n_obs, n_slots] in complex128, the reference's complex64 Jacobian), read-only, once per process"""
    Ls = observables(tape.n, seed)[2]
    ot = NR.reference_tape(tape, row)
    ref = DR.shift_jacobian(ot, tape.n, Ls, set(wanted))
    c64 = DR.shift_jacobian(ot, tape.n, Ls, set(wanted), dtype=np.complex64)
    ref.flags.writeable = c64.flags.writeable = False
    return ref, c64


def sweep(tape, seed, w, wanted, x64=False, rows=B, **kw):
    groups, terms, _Ls = observables(tape.n, seed)
    want = [k in set(wanted) for k in range(n_slots(tape))]
    with x64_scope(x64):
        return adjoint.density_gradient(tape.ops, tape.n, rows, groups, w, want, x64=x64, obs_terms=terms, **kw)


def compare(name, tape, seed, got, w, wanted, x64=False, same_rows=False, slack=1.0):
    """Row r of ``got`` / ``w`` ([K * rows]) is sample r % rows; -> the largest error"""
    rows = B
    worst = 0.0
    for r in range(got.shape[0]):
        ref, c64 = reference(tape, 0 if same_rows else r % rows, seed, tuple(wanted))
        scale = max(1.0, float(np.abs(w[r]).sum()))
        floor = float(np.abs(w[r] @ c64 - w[r] @ ref).max()) / scale
        tol = slack * (1e-12 if x64 else max(routes_tolerance(2 * tape.n, False), 4.0 * floor))
        err = float(np.abs(got[r] - w[r] @ ref).max()) / scale
        print(f"{name} {seed} {'x64' if x64 else 'c64'} row {r}: routes tolerance {routes_tolerance(2 * tape.n, x64):.1e} "
              f"4 x c64 floor {4 * floor:.2e} error {err:.2e}")
        assert err <= tol, (name, seed, r, err, tol)
        unwanted = [k for k in range(got.shape[1]) if k not in set(wanted)]
        assert not np.any(got[r, unwanted]), (name, "columns that are not wanted must be exactly zero")
        worst = max(worst, err)
    return worst


# ---- step level ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x64", [False, True], ids=["c64", "x64"])
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: f"{c[0]}{''.join(map(str, c[1]))}_{c[2]}_n{c[3]}")
def test_one_step_behind_its_channel(case, x64):
    """one parametrised gate and the channel behind it, both seeds"""
    tape = step_tape(*case)
    wanted = tuple(range(n_slots(tape)))
    assert any(len(s[1]) and s[3] >= 0 for s in adjoint.plan_density(tape.ops, tape.n, [True] * len(wanted)).steps)
    for seed in ("z", "pauli"):
        w = weights(3 if seed == "z" else 4, B, 11)
        compare("step", tape, seed, sweep(tape, seed, w, wanted, x64), w, wanted, x64)


# ---- tape level ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ["z", "pauli"])
@pytest.mark.parametrize("n", [5, 7, 8])
def test_random_noisy_tape(n, seed):
    """n = 7: 14 doubled wires, the first size past the single-launch regime of the engine"""
    tape = random_tape(n)
    wanted = wanted_of(tape, WANTED[n])
    w = weights(3 if seed == "z" else 4, B, 12 + n)
    compare(f"random n={n}", tape, seed, sweep(tape, seed, w, wanted), w, wanted)


@pytest.mark.parametrize("n", [5, 7])
def test_random_noisy_tape_x64(n):
    tape = random_tape(n)
    wanted = wanted_of(tape, WANTED[n])
    w = weights(3, B, 12 + n)
    compare(f"random n={n}", tape, "z", sweep(tape, "z", w, wanted, x64=True), w, wanted, x64=True)


@pytest.mark.parametrize("seed", ["z", "pauli"])
def test_stacked_cotangents_share_one_forward_run(seed):
    """K = 2 cotangents per sample: rows k * B + b"""
    tape = random_tape(5)
    wanted = wanted_of(tape, 12)
    w = weights(3 if seed == "z" else 4, 2 * B, 21)
    got = sweep(tape, seed, w, wanted)
    assert got.shape[0] == 2 * B
    compare("stacked", tape, seed, got, w, wanted)


def test_left_out_angles_stay_exactly_zero():
    tape = random_tape(5)
    wanted = wanted_of(tape, 12)[1::3]  # (a two-wire step with a channel among them)
    w = weights(3, B, 22)
    compare("subset", tape, "z", sweep(tape, "z", w, wanted), w, wanted)  # (compare checks the other columns)


@pytest.mark.parametrize("seed", ["z", "pauli"])
def test_noisy_model_tape(seed):
    tape = model_noisy_tape()
    wanted = wanted_of(tape, 10)
    w = weights(3 if seed == "z" else 4, B, 23)
    compare("model", tape, seed, sweep(tape, seed, w, wanted), w, wanted, same_rows=True)


def test_rounds_agree_with_the_uncut_call():
    """B = 5 cut into rounds 2, 2, 1 by ``max_bytes``"""
    rng = np.random.default_rng(31)
    with NR.recording_depolarizing() as (ops, depol):
        for q in range(3):
            op.RY(Batched(rng.uniform(0, 2 * np.pi, size=(5,)), []), wires=q)
            op.AmplitudeDamping(0.2, wires=q)
        op.CRX(Batched(rng.uniform(0, 2 * np.pi, size=(5,)), []), wires=[0, 2])
        op.DepolarizingChannel(0.05, wires=2)
    want = [True] * 4
    w = weights(3, 5, 32)
    sw = adjoint.plan_density(ops, 3, want)
    from qml_essentials_amd.simulation import get_plan

    plans = get_plan(sw.fwd, adjoint.DENSITY_FLAGS), get_plan(sw.rev, adjoint.DENSITY_FLAGS)
    need = lambda bc: adjoint.density_call_bytes(sw, *plans, bc, 1, 3)  # noqa: E731  (checkpoints, lambda, workspace, tables)
    assert need(2) > 2 * sw.sample_bytes(1) and need(3) > need(2)
    assert adjoint.density_rounds(5, need, need(2)) == [2, 2, 1]
    full = adjoint.density_gradient(ops, 3, 5, z_groups(3), w, want)
    cut = adjoint.density_gradient(ops, 3, 5, z_groups(3), w, want, max_bytes=need(2))
    with pytest.raises(adjoint.AdjointUnsupported, match=str(need(1))):
        adjoint.density_gradient(ops, 3, 5, z_groups(3), w, want, max_bytes=need(1) - 1)
    err = max(DR.metric(cut[r], full[r], w[r]) for r in range(5))
    print("rounds: max |cut - uncut| / max(1, sum|w|)", err)
    assert err <= 2 * routes_tolerance(6, False)
    tape = NR.NoisyTape(ops, depol, 3)
    for r in range(5):
        ref = DR.shift_gradient(NR.reference_tape(tape, r), 3, DR.cost_matrix(3, w[r], groups=z_groups(3)))
        assert DR.metric(cut[r], ref, w[r]) <= routes_tolerance(6, False)


# ---- front end -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noisy_model():
    from qml_essentials_amd.model import Model

    model = Model(n_qubits=3, n_layers=2, circuit_type="Circuit_19", output_qubit=-1)
    model.noise_params = {k: v for k, v in NR.NOISE.items()}
    rng = np.random.default_rng(41)
    return model, rng.uniform(0, 2 * np.pi, size=model.params.shape[1:]), rng.uniform(0, 2 * np.pi, size=(3, 1))


def forward(model, params, inputs):
    return np.asarray(model(params=params, inputs=inputs, execution_type="expval"), dtype=np.float64).reshape(3, -1)


def shift_rule(f, R):
    """f'(0) of a trigonometric polynomial of degree <= R / 2 in half-integer steps -- frequencies 0, 1/2, .., R / 2 --
    from 2 R evaluations: the general equidistant shift rule on the variable 2 x (degree R, shifts (2 mu - 1) pi / R in
    x).  -> (derivative, sum of |coefficients|).  R = 2 covers every single gate (controlled rotations have the
    frequencies 1/2 and 1); an input that feeds G encoding rotations needs R = 2 G."""
    total, norm = 0.0, 0.0
    for mu in range(1, 2 * R + 1):
        x = (2 * mu - 1) * np.pi / R        # shift in x; the polynomial has degree R in x / 2
        coef = (-1) ** (mu - 1) / (4 * R * np.sin(x / 4) ** 2) / 2.0
        total = total + coef * f(x)
        norm += abs(coef)
    return total, norm


def shift_jacobians(model, params, inputs):
    """The parameter-shift Jacobians of the model's outputs through its own forward pass (the complex64 density route):
    -> (d out / d params [B, n_out, *params.shape], d out / d inputs [B, n_out, 1], largest sum of |coefficients|).
    ``Model.gradient(method="parameter-shift")`` does not take a model with noise (it raises the channel's TypeError,
    with and without this feature), so the rule is formed here."""
    n_out = forward(model, params, inputs).shape[1]
    jp = np.zeros((3, n_out) + params.shape)
    norm = 0.0
    for idx in np.ndindex(*params.shape):
        def f(x, idx=idx):
            p = params.copy()
            p[idx] += x
            return forward(model, p, inputs)
        jp[(slice(None), slice(None)) + idx], c = shift_rule(f, 2)
        norm = max(norm, c)
    G = model.n_layers * model.n_qubits * 2  # (an input feeds at most one encoding rotation per layer and wire)
    ji, c = shift_rule(lambda x: np.stack([forward(model, params, inputs + x * (np.arange(3) == b)[:, None])[b]
                                           for b in range(3)]), G)
    return jp, ji[:, :, None], max(norm, c)


FRONT_END_BOUND = routes_tolerance(6, False)
"""The complex64 bound above at 6 doubled wires, with the metric max |adjoint - shift| / max(1, sum |w|): a one-hot
cotangent (the Jacobian) and the mean (weights 1 / n_out) have sum |w| = 1.  The 4 x floor figure could only widen it."""


@pytest.mark.parametrize("force_mean", [False, True], ids=["jacobian", "mean"])
def test_model_gradient_noisy_equals_parameter_shift(force_mean):
    model, params, inputs = noisy_model()
    jp, ji, _norm = shift_jacobians(model, params, inputs)
    got = model.gradient(params=params, inputs=inputs, wrt=("params", "inputs"), method="adjoint", noisy=True,
                         force_mean=force_mean)
    for one, g, ref in zip(("params", "inputs"), got, (jp, ji)):
        ref = ref.mean(axis=1) if force_mean else ref
        assert g.size == ref.size, (one, g.shape, ref.shape)
        err = float(np.abs(g.reshape(ref.shape) - ref).max())
        print("Model.gradient noisy", one, "mean" if force_mean else "jacobian", "max |adjoint - shift|", err, "bound",
              FRONT_END_BOUND, "largest entry", float(np.abs(ref).max()))
        assert float(np.abs(ref).max()) > 1e-2 and err <= FRONT_END_BOUND


def test_model_gradient_noisy_with_a_cotangent():
    model, params, inputs = noisy_model()
    jp, _ji, _norm = shift_jacobians(model, params, inputs)
    cot = weights(jp.shape[1], 3, 42)
    want = np.einsum("bk,bk...->b...", cot, jp)
    got = model.gradient(params=params, inputs=inputs, wrt="params", method="adjoint", noisy=True, cotangent=cot)
    got = got.reshape(want.shape)
    err = max(DR.metric(got[b], want[b], cot[b]) for b in range(3))
    print("Model.gradient noisy cotangent: max |adjoint - shift| / max(1, sum|w|)", err, "bound", FRONT_END_BOUND)
    assert err <= FRONT_END_BOUND


def _script_circuit(theta):
    op.RX(theta[0], wires=0)
    op.AmplitudeDamping(0.2, wires=0)
    op.CRY(theta[1], wires=[0, 1])
    op.DepolarizingChannel(0.05, wires=1)
    op.Rot(theta[2], theta[3], theta[4], wires=1)
    op.PhaseDamping(0.15, wires=1)
    op.RZZ(theta[0], wires=[1, 0])  # (theta[0] once more: the chain rule adds)
    op.BitFlip(0.1, wires=0)


@pytest.mark.parametrize("x64", [False, True], ids=["c64", "x64"])
@pytest.mark.parametrize("pauli", [False, True], ids=["z", "pauli"])
def test_script_vjp_noisy(pauli, x64):
    """Script.vjp(noisy=True) with in_axes, K = 2 stacked cotangents and both seeds against the complex128 reference"""
    from qml_essentials_amd.script import Script

    theta = np.random.default_rng(43).uniform(0, 2 * np.pi, size=(B, 5))
    obs = [op.PauliX(wires=0), op.PauliY(wires=1)] if pauli else [op.PauliZ(wires=0), op.PauliZ(wires=1)]
    terms = [(1.0, 1, 0, 0), (1.0, 2, 2, 1)]
    cot = weights(2, 2 * B, 44).reshape(2, B, 2)
    with x64_scope(x64):
        (got,) = Script(_script_circuit, n_qubits=2).vjp(obs, cot, args=(theta,), in_axes=(0,), pauli_seed=pauli, noisy=True)
    assert got.shape == (2, B, 5)
    for k in range(2):
        for b in range(B):
            with NR.recording_depolarizing() as (ops, depol):
                _script_circuit(theta[b])
            L = DR.cost_matrix(2, cot[k, b], terms=terms) if pauli else DR.cost_matrix(2, cot[k, b], groups=[[0], [1]])
            g = DR.shift_gradient(NR.reference_tape(NR.NoisyTape(ops, depol, 2)), 2, L)  # slots: RX, CRY, RZ, RY, RZ, RZZ
            ref = np.array([g[0] + g[5], g[1], g[2], g[3], g[4]])
            err = DR.metric(got[k, b], ref, cot[k, b])
            assert err <= routes_tolerance(4, x64), (k, b, err)


def test_without_the_keyword_nothing_changes():
    """a noisy model's adjoint gradient raises what it raised before: the channel's own refusal to be lowered"""
    model, params, inputs = noisy_model()
    with pytest.raises(TypeError, match="noise channel"):
        model.gradient(params=params, inputs=inputs, wrt="params", method="adjoint", force_mean=True)
    with pytest.raises(ValueError, match="noisy=True needs method='adjoint'"):
        model.gradient(params=params, inputs=inputs, wrt="params", noisy=True)


def test_script_vjp_without_the_keyword_and_the_keyword_without_noise():
    from qml_essentials_amd.script import Script

    theta = np.random.default_rng(45).uniform(0, 2 * np.pi, size=(B, 5))
    obs, cot = [op.PauliZ(wires=0), op.PauliZ(wires=1)], weights(2, B, 46)
    with pytest.raises(TypeError, match="noise channel"):  # (what a noisy tape raised before: the channel refuses to be lowered)
        Script(_script_circuit, n_qubits=2).vjp(obs, cot, args=(theta,), in_axes=(0,))

    def clean(th):  # no channel: noisy=True takes the pure-state sweep, bit for bit
        op.RX(th[0], wires=0)
        op.CRY(th[1], wires=[0, 1])
        op.Rot(th[2], th[3], th[4], wires=1)

    s = Script(clean, n_qubits=2)
    (plain,) = s.vjp(obs, cot, args=(theta,), in_axes=(0,))
    (keyed,) = s.vjp(obs, cot, args=(theta,), in_axes=(0,), noisy=True)
    assert np.abs(plain).max() > 1e-2 and np.array_equal(plain, keyed)


def test_three_wire_channel_is_refused():
    from qml_essentials_amd.script import Script
    from qml_essentials_amd.unitary import UnitaryGates

    def circuit(theta):
        op.RX(theta[0], wires=0)
        op.RY(theta[1], wires=1)
        UnitaryGates.NQubitDepolarizingChannel(0.1, [0, 1, 2])

    with pytest.raises(adjoint.AdjointUnsupported, match="3 wires"):
        Script(circuit, 3).vjp([op.PauliZ(wires=0)], np.ones(1), args=(np.array([0.3, 0.4]),), noisy=True)
