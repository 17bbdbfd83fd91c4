"""``qmle_density_apply_wide`` alone -- ``rho -> sum_m K_m rho K_m^+`` on 3 or 4 system wires of a resident vec(rho) --
against the complex128 einsum of tests/density_wide_reference.py (tests/test_density_wide_cpu.py shows, without a GPU,
that the metric below tells every wrong variant of that reference apart with a margin of 100).

Shapes: k = 3 at n = 3..8 and k = 4 at n = 4..8 -- the whole register being the targets, a register smaller than the
12-bit tile (2n < 12), equal to it (2n = 12), several tiles (2n = 14, 16) -- and one case at n = 10 with batch 2.
Wires: the lowest in order, a set with wire n - 1 and wire 0 out of order (a bra target on position 0), a descending
set.  Operators: one unitary, one non-unitary matrix, random sets of d / 2 and d / 2 + 1 (where the
arithmetic of the two forms is level, and one past it), the d^2 operators of NQubitDepolarizingChannel, one unitary per sample at batch 3.  Forms: automatic
and both forced wherever the arguments allow.

Bounds.  complex64: ``||got - want||_F / ||want||_F <= 16 * c64_floor`` (the rule of tests/test_gpu_noise_routes.py),
``c64_floor`` being the same error of a NumPy complex64 evaluation of the same form, per case; every case prints its
ratio (profiles/density_wide.md records them).  complex128: below 1e-12.  The two forced forms each meet the bound
against the reference, and their distance from one another is held to the same bound (with the larger of their two
floors)."""
import numpy as np
import pytest

import density_wide_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = [(3, n) for n in (3, 4, 5, 6, 7, 8)] + [(4, n) for n in (4, 5, 6, 7, 8)]
GEOMETRIES = [(k, n, tuple(w)) for k, n in SHAPES for w in R.wire_sets(n, k)]


def _N():
    from qml_essentials_amd import _native as N

    return N


def _forms(k, kind, n_ops):
    """The forms the arguments allow: a per-sample stack has no shared superoperator."""
    return ["auto", "sandwich"] if kind == "per_sample" else ["auto", "sandwich", "superoperator"]


def _run(rho, n, wires, ops, dtype, per_sample, form):
    N = _N()
    vec = torch.from_numpy(np.ascontiguousarray(rho.reshape(rho.shape[0], -1))).to(dtype).cuda()
    N.density_apply_wide(vec, n, list(wires), ops, per_sample=per_sample, form=form)
    return vec.cpu().numpy().reshape(rho.shape)


def _check(label, got, rho, want, n, wires, ops, kind, form, x64):
    """Every sample against its reference; returns the largest ratio (complex64) or error (complex128)."""
    worst, k = 0.0, len(wires)
    for b in range(rho.shape[0]):
        o = ops[b:b + 1] if kind == "per_sample" else ops
        err = R.rel_err(got[b], want[b])
        if x64:
            print(f"{label} sample {b} x64: rel_err {err:.3e}")
            assert err < R.X64_RTOL, (label, b, err)
            worst = max(worst, err)
            continue
        resolved = R.auto_form(k, len(o), kind == "per_sample") if form == "auto" else form
        floor = R.c64_floor(rho[b], n, list(wires), o, resolved, want[b])
        print(f"{label} sample {b}: rel_err {err:.3e} = {err / floor:.2f} x c64_floor {floor:.3e}")
        assert err <= R.FACTOR * floor, (label, b, err, floor)
        worst = max(worst, err / floor)
    return worst


@pytest.mark.parametrize("x64", [False, True], ids=["c64", "x64"])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=[f"k{k}-n{n}-{'_'.join(map(str, w))}" for k, n, w in GEOMETRIES])
def test_every_operator_set_and_form(geometry, x64):
    k, n, wires = geometry
    batch = 1 if list(wires) == list(range(k)) else 3  # (the lowest wires in order: batch 1; the other sets: batch 3)
    dtype = torch.complex128 if x64 else torch.complex64
    for kind in R.KINDS:
        b = 3 if kind == "per_sample" else batch
        rho, ops, want = R.case(n, k, wires, kind, b)
        got = {}
        for form in _forms(k, kind, len(ops)):
            label = f"k={k} n={n} wires={list(wires)} {kind} {form}"
            got[form] = _run(rho, n, wires, ops, dtype, kind == "per_sample", form)
            _check(label, got[form], rho, want, n, wires, ops, kind, form, x64)
        assert np.array_equal(got["auto"], got[R.auto_form(k, len(ops), kind == "per_sample")])  # the rule, and the same bits
        if "superoperator" in got:  # the two forced forms against each other, within the same bound
            for s in range(b):
                gap = R.rel_err(got["sandwich"][s], got["superoperator"][s])
                bound = R.X64_RTOL if x64 else R.FACTOR * max(
                    R.c64_floor(rho[s], n, list(wires), ops, f, want[s]) for f in ("sandwich", "superoperator"))
                assert gap <= bound, (kind, s, gap, bound)


@pytest.mark.parametrize("k,wires", [(3, (9, 0, 5)), (4, (1, 8, 0, 9))])
def test_ten_qubits_batch_two(k, wires):
    n = 10
    for kind in ("unitary", "half1"):
        rho, ops, want = R.case(n, k, wires, kind, 2)
        got = _run(rho, n, wires, ops, torch.complex64, False, "auto")
        _check(f"k={k} n=10 wires={list(wires)} {kind} auto", got, rho, want, n, wires, ops, kind, "auto", False)


@pytest.mark.parametrize("form,kind", [("sandwich", "unitary"), ("superoperator", "half1")])
def test_a_batch_past_one_launch(form, kind):
    """65537 samples at n = 3: the library splits the launch at 65535 grid rows."""
    N, n, k, wires, B = _N(), 3, 3, (2, 0, 1), 65537
    rho, ops, want = R.case(n, k, wires, kind, 3)
    rows = [0, 1, 2, 65534, 65535, 65536]
    vec = torch.zeros((B, 4 ** n), dtype=torch.complex64, device="cuda")
    src = torch.from_numpy(rho.reshape(3, -1)).to(torch.complex64).cuda()
    vec[:] = src[0]
    for i, r in enumerate(rows):
        vec[r] = src[i % 3]
    N.density_apply_wide(vec, n, list(wires), ops, form=form)
    got = vec[rows].cpu().numpy().reshape(len(rows), 2 ** n, 2 ** n)
    for i, r in enumerate(rows):
        err = R.rel_err(got[i], want[i % 3])
        floor = R.c64_floor(rho[i % 3], n, list(wires), ops, form, want[i % 3])
        print(f"batch 65537 {form} row {r}: rel_err {err:.3e} = {err / floor:.2f} x c64_floor {floor:.3e}")
        assert err <= R.FACTOR * floor, (r, err, floor)
    assert torch.equal(vec[3], vec[40000]) and torch.equal(vec[3], vec[65533])  # equal inputs, equal bits


def test_per_sample_operators_past_one_launch():
    """Sample b takes operator b on both sides of the launch split."""
    N, n, k, wires, B = _N(), 3, 3, (0, 1, 2), 65537
    rho, ops, want = R.case(n, k, wires, "per_sample", 3)
    vec = torch.from_numpy(rho.reshape(3, -1)).to(torch.complex64).cuda()[torch.arange(B, device="cuda") % 3].contiguous()
    mats = torch.from_numpy(np.ascontiguousarray(ops)).cuda()[torch.arange(B, device="cuda") % 3].contiguous()
    N.density_apply_wide(vec, n, list(wires), mats, per_sample=True)
    for r in (0, 1, 65534, 65535, 65536):
        err = R.rel_err(vec[r].cpu().numpy().reshape(2 ** n, 2 ** n), want[r % 3])
        floor = R.c64_floor(rho[r % 3], n, list(wires), ops[r % 3:r % 3 + 1], "sandwich", want[r % 3])
        print(f"per-sample batch 65537 row {r}: {err / floor:.2f} x c64_floor")
        assert err <= R.FACTOR * floor, (r, err, floor)


@pytest.mark.parametrize("x64", [False, True], ids=["c64", "x64"])
def test_a_slice_of_a_larger_tensor(x64):
    """Rows 2..4 of a 6-row tensor: a non-zero row offset; the other rows keep their bits."""
    N, n, k, wires = _N(), 6, 4, (1, 4, 0, 5)
    rho, ops, want = R.case(n, k, wires, "half", 3)
    dtype = torch.complex128 if x64 else torch.complex64
    big = torch.full((6, 4 ** n), 0.25 - 0.5j, dtype=dtype, device="cuda")
    big[2:5] = torch.from_numpy(rho.reshape(3, -1)).to(dtype).cuda()
    before = big.clone()
    N.density_apply_wide(big[2:5], n, list(wires), ops)
    got = big[2:5].cpu().numpy().reshape(3, 2 ** n, 2 ** n)
    _check("slice rows 2..4", got, rho, want, n, wires, ops, "half", "auto", x64)
    assert torch.equal(big[:2], before[:2]) and torch.equal(big[5:], before[5:])


def test_the_same_bits_from_call_to_call():
    n, k, wires = 7, 3, (6, 0, 3)
    rho, ops, _ = R.case(n, k, wires, "depol", 3)
    for form in ("sandwich", "superoperator"):
        a = _run(rho, n, wires, ops, torch.complex64, False, form)
        b = _run(rho, n, wires, ops, torch.complex64, False, form)
        assert np.array_equal(a, b)
