"""tests/matrix_cotangent2_reference.py against itself, ``adjoint.build_reverse(two_wire=True)``, the host-side
refusals of ``qmle_adjoint_cotangent_at`` / ``_f64`` and the resources of the kernels behind them; no GPU.

``G_ref`` (forward simulations alone) equals the adjoint-style computation ``M (U^+)^T`` to 1e-12, and each named
wrong variant -- wires exchanged, ``G`` transposed, ``(U^+)^T`` missing, ``U`` in place of ``U^+`` -- lies at least 1e-6
away from it on every two-wire gate of every case below 12 qubits (nearest seen: printed by the test).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from qml_essentials_amd import _native as N
from qml_essentials_amd import adjoint
from qml_essentials_amd.simulation import LoweredTape, _Lowered
from tests import matrix_cotangent2_reference as M2

SMALL = ["lds_n2", "lds_n6", "stream_n5", "x64_n3"]


@pytest.mark.parametrize("seed", ["z", "pauli"])
@pytest.mark.parametrize("name", SMALL)
def test_reference_equals_the_adjoint_style_computation_and_no_wrong_variant_does(name, seed):
    case = M2.cases()[name]
    mats, w = M2.seed_observables(case, seed)
    _grad, cots = M2.case_reference(name, seed)
    nearest = np.inf
    for b in range(case.theta.shape[0]):
        tape = M2.tape_of(case.spec, case.theta[b], b)
        for k, g in enumerate(case.mats):
            if len(case.spec[g][1]) != 2:
                continue
            forms = M2.adjoint_style2(tape, g, case.n, mats, w[b])
            assert np.abs(forms.pop("right") - cots[k][b]).max() <= 1e-12, (name, b, g)
            for variant, m in forms.items():
                dist = np.abs(m - cots[k][b]).max()
                nearest = min(nearest, dist)
                assert dist >= 1e-6, (name, b, g, variant, dist)
    print(name, seed, "nearest wrong variant", nearest)


def test_reference_cotangent_contracts_to_a_difference_quotient():
    """dC/dt of U(t) = exp(-i t K) U on the two-wire gate: 2 Re sum G dU/dt against central differences"""
    case = M2.cases()["x64_n3"]
    mats, w = M2.seed_observables(case, "pauli")
    tape = M2.tape_of(case.spec, case.theta[0], 0)
    g = next(g for g in case.mats if len(case.spec[g][1]) == 2)
    u = np.asarray(tape[g][2][0], dtype=np.complex128)
    rng = np.random.default_rng(5)
    k = rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4))
    k = k + k.conj().T
    du = -1j * k @ u
    G_ref = M2.reference_cotangent(tape, g, case.n, mats, w[0])
    from scipy.linalg import expm

    def cost(t):
        psi = M2.R.run_from(M2.R.zero_state(case.n), M2.M1.replaced(tape, g, expm(-1j * t * k) @ u), case.n)
        return M2.cost_of(psi, case.n, mats, w[0])

    h = 1e-5
    fd = (cost(h) - cost(-h)) / (2 * h)
    assert abs(2 * np.real(np.sum(G_ref * du)) - fd) <= 1e-7 * max(1.0, abs(fd))


def _tape(B=3):
    rng = np.random.default_rng(11)
    u2 = np.stack([M2.R.unitary(rng, 2) for _ in range(B)])
    u1 = np.stack([M2.R.unitary(rng, 1) for _ in range(B)])
    c2 = M2.R.unitary(rng, 2)
    ops = [_Lowered(("RX", [0], [np.full(B, 0.3)], None)),
           _Lowered(("MAT2_ROW", [2, 0], [np.stack([u2.real, u2.imag], -1).reshape(B, 32)[:, j] for j in range(32)], None)),
           _Lowered(("MAT1_ROW", [1], [np.stack([u1.real, u1.imag], -1).reshape(B, 8)[:, j] for j in range(8)], None)),
           _Lowered(("MAT2", [0, 1], [], np.stack([c2.real, c2.imag], -1).astype(np.float32).reshape(-1)))]
    return LoweredTape(ops, 3), u2, u1


def test_build_reverse_two_wire_daggers_a_mat2_row_through_src_and_sign():
    low, u2, _u1 = _tape()
    names = [o[0] for o in low.ops]
    assert names == ["RX", "MAT2_ROW", "MAT1_ROW", "MAT2"]
    flags = [False, True, True, True]
    rev_ops, terms, rev_src, rev_sign, mat_out, mat_dim = adjoint.build_reverse(
        low, adjoint._op_blobs(low), [True] + [False] * (low.n_slots - 1), flags, two_wire=True)
    assert mat_out == [2, 1, 0, -1] and mat_dim == [4, 2, 4]
    rev = LoweredTape(rev_ops, 3)
    assert [o[0] for o in rev.ops] == ["MAT2", "MAT1_ROW", "MAT2_ROW", "RX"]
    table = low.angle_table(3, dtype=np.float64)
    a_r = table[:, rev_src] * np.asarray(rev_sign)
    assert np.array_equal(a_r, rev.angle_table(3, dtype=np.float64))
    slots = rev.ops[2][2]
    assert len(slots) == 32 and len(rev_src) == 8 + 32 + 1
    m = a_r[:, slots].reshape(3, 4, 4, 2)
    assert np.array_equal(m[..., 0] + 1j * m[..., 1], np.conj(np.swapaxes(u2, 1, 2)))


def test_build_reverse_two_wire_flags_and_refusals():
    low, _u2, _u1 = _tape()
    blobs, want = adjoint._op_blobs(low), [False] * low.n_slots
    with pytest.raises(adjoint.AdjointUnsupported, match="matrix"):  # a flag on a rotation stays refused
        adjoint.build_reverse(low, blobs, want, [True, False, False, False], two_wire=True)
    with pytest.raises(adjoint.AdjointUnsupported, match="two-wire"):  # without two_wire nothing changed
        adjoint.build_reverse(low, blobs, want, [False] * 4)
    with pytest.raises(ValueError):
        adjoint.build_reverse(low, blobs, want, None, two_wire=True)


def test_the_cotangent_at_entry_points_refuse_bad_requests_before_touching_a_device():
    """Status codes decided on the host: the device pointers below point nowhere and are never read."""
    low, _u2, _u1 = _tape(1)
    rev_ops, terms, *_ = adjoint.build_reverse(low, adjoint._op_blobs(low), [False] * low.n_slots, [False] * 4,
                                               two_wire=True)
    rev = LoweredTape(rev_ops, 3)
    from qml_essentials_amd.simulation import get_plan

    fwd, rv = get_plan(low), get_plan(rev, adjoint.REV_FLAGS)
    arr = N._adjoint_term_array(terms)
    masks = N._wire_group_masks([[0]], 3)
    p, null = C.c_void_p(0x1000), C.c_void_p(None)
    INVALID, UNSUPPORTED, SLOT_RANGE = -1, -10, -11
    for fn, wsq in ((N.lib().qmle_adjoint_cotangent_at, N.lib().qmle_adjoint_cotangent_at_workspace_bytes),
                    (N.lib().qmle_adjoint_cotangent_at_f64, N.lib().qmle_adjoint_cotangent_at_workspace_bytes_f64)):
        assert wsq(fwd._h, rv._h, 1, 0, 1, 1) >= wsq(fwd._h, rv._h, 1, 0, 1, 0) > 0
        big = C.c_size_t(1 << 30)

        def call(off, stride=64, plan=rv, cot=p, n_terms=len(terms)):
            carr = (C.c_int32 * len(off))(*off) if off is not None else None
            return fn(fwd._h, plan._h, p, p, 1, p, masks, None, 0, 1, arr, n_terms, p, max(1, low.n_slots), carr,
                      stride, cot, p, big, null)

        # reverse tape: MAT2, MAT1_ROW, MAT2_ROW, RX
        assert call(None) == INVALID and call([0, -1, -1, -1], cot=null) == INVALID
        assert call([0, -1, -1, -1], stride=0) == INVALID and call([0, -1, -1, -1], n_terms=3) == INVALID
        assert call([-1, -1, -1, 0]) == UNSUPPORTED                      # a flag on a rotation
        assert call([0, -1, -1, -1], stride=31) == SLOT_RANGE            # a 32-scalar block in a row of 31
        assert call([-1, 57, -1, -1]) == SLOT_RANGE                      # an 8-scalar block that ends at 65
        assert call([0, 31, -1, -1]) == SLOT_RANGE                       # overlap
        assert call([0, 24, 32, -1]) == SLOT_RANGE                       # the 2x2 inside the first 4x4
    assert N.lib().qmle_sv_version() == 150


def test_the_two_wire_kernels_use_no_scratch_and_the_lds_kernel_keeps_its_occupancy():
    with open(os.path.join(os.path.dirname(N.__file__), "kernel_resources.json")) as f:
        res = json.load(f)
    new = {k: v for k, v in res.items() if "k_adj_moment2" in k or "k_adj_cot2_final" in k}
    assert len(new) == 4  # float2 and double2 of each
    for name, v in new.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
    lds = {k: v for k, v in res.items() if "k_adjoint_lds" in k}
    assert len(lds) == 4 and all(v["Occupancy"] >= 4 and v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0
                                 for v in lds.values())
