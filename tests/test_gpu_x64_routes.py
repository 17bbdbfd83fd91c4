"""Every branch of the complex128 engine's forward run (``qmle_run_batch_f64``: ``k64_lds`` up to 13 wires, one
``k64_op`` launch per operator above; ``qmle_apply_inplace_f64`` on resident states) against tests/x64_reference.py, a
plain NumPy complex128 evolution.  tests/test_x64_reference_cpu.py asserts without a GPU that every case below tells
every wrong variant of that reference (exchanged wires, transposed or conjugated matrices, the wrong bit order, a
neighbour's angle row, the first round's rows, float32 constants ...) apart by 1e-6, and that the merge cases
compile to the plan shapes they are named after.

Tolerance: the project's complex128 bar, ``max |got - want| < 1e-12`` for unit-norm states and for observables of
norm 1 (tests/test_gpu_x64.py, tests/test_gpu_noise_routes.py).  Every test prints its largest error;
profiles/x64_parity.md records the largest per family (a) to (g)."""
import ctypes as C

import numpy as np
import pytest

import x64_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = R.TOL
WORST = {}  # family -> largest error of this session


def _N():
    from qml_essentials_amd import _native as N

    return N


def _plan(case, flags=0, full_precision=True):
    """The case's plan (float32 blob, then the float64 constants unless ``full_precision`` is off) and its angles."""
    N = _N()
    ops, angles, consts = case.native()
    plan = N.Plan(ops, case.n, angles.shape[1], consts.astype(np.float32), flags)
    if full_precision and consts.size:
        plan.set_consts64(consts)
    return plan, torch.from_numpy(angles).cuda()


def _err(family, label, got, want):
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, got.dtype)
    err = float(np.abs(got - want).max())
    WORST[family] = max(WORST.get(family, 0.0), err)
    return err


def _resident(case, plan, angles):
    states = torch.from_numpy(case.psi0).cuda().contiguous()
    return _N().apply_inplace64(plan, angles, states).cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for family in sorted(WORST):
        print(f"\nx64 parity, family {family}: largest error {WORST[family]:.3e} (bar {TOL:.0e})", end="")
    print()


# ---- a. every operator kind at every position, on resident states ----------------------------------------------
@pytest.mark.parametrize("n,kind", R.RESIDENT, ids=[f"{k}-{n}" for n, k in R.RESIDENT])
def test_a_every_kind_at_every_position_on_resident_states(n, kind):
    """One-gate plans through ``apply_inplace64`` (``k64_op``), 3 rows with their own start state and angle: every
    ordered choice of wires at n = 5, of the wires {0, 1, 6, 7, 12, 13} at n = 14 (the strided loop of the streaming
    grid runs more than once there), and n = 1."""
    worst = 0.0
    for case in R.resident_cases(n, kind):
        plan, angles = _plan(case)
        err = _err("a", case.label, _resident(case, plan, angles), R.reference_state(case))
        assert err < TOL, (case.label, err)
        worst = max(worst, err)
    print(f"a {kind} n={n}: {len(R.resident_cases(n, kind))} positions, largest error {worst:.3e}")


# ---- b. the same kinds inside the LDS kernel, and what lower_tape merges ------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_b_every_kind_behind_an_entangling_prefix_in_the_lds_kernel(kind):
    """``run64`` at n = 10 (``k64_lds``): the gate behind RY, RZ on every wire and a CX chain, wires drawn from
    {0, 1, 4, 5, 8, 9}; default flags (the gate merges with its neighbours where it can) and PLAN_NO_MERGE (what
    the Python layer runs pure x64 calls on)."""
    N = _N()
    worst = 0.0
    for case in R.lds_kind_cases(10, kind):
        want = R.reference_state(case)
        for flags in (0, N.PLAN_NO_MERGE):
            plan, angles = _plan(case, flags)
            err = _err("b", case.label, plan.run64(angles, "state").cpu().numpy(), want)
            assert err < TOL, (case.label, flags, err)
            worst = max(worst, err)
    print(f"b {kind} n=10: {len(R.lds_kind_cases(10, kind))} positions x 2 flag settings, largest error {worst:.3e}")


@pytest.mark.parametrize("n", [10, 14])
@pytest.mark.parametrize("merge", R.MERGES)
def test_b_merged_operators_under_every_flag_setting(merge, n):
    """One-qubit gates multiplied onto one-qubit gates and onto either side of a 4x4 (BuildOp::pad 1 / 2), 4x4 onto
    4x4 on the same ordered pair, NOT on the reversed pair, a 4x4 that takes the pending gates of both wires: each
    flag setting within 1e-12 of the reference, the settings within 1e-13 of one another.  n = 14: the same
    through the streaming path."""
    N = _N()
    worst = spread = 0.0
    for case in R.merge_cases(n, merge):
        want = R.reference_state(case)
        got = {}
        for name, flags in (("default", 0), ("no_merge", N.PLAN_NO_MERGE), ("no_fusion", N.PLAN_NO_FUSION),
                            ("tape_order", N.PLAN_TAPE_ORDER)):
            plan, angles = _plan(case, flags)
            got[name] = plan.run64(angles, "state").cpu().numpy()
            err = _err("b", case.label, got[name], want)
            assert err < TOL, (case.label, name, err)
            worst = max(worst, err)
        for name in ("no_merge", "no_fusion", "tape_order"):
            d = float(np.abs(got[name] - got["default"]).max())
            assert d < 1e-13, (case.label, name, d)
            spread = max(spread, d)
    print(f"b {merge} n={n}: largest error {worst:.3e}, largest difference between flag settings {spread:.3e}")


# ---- c. constants at full precision ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,resident", R.CONSTANTS, ids=[f"n{n}{'-resident' if r else ''}" for n, r in R.CONSTANTS])
def test_c_constants_at_full_precision_and_the_float32_blob(n, resident):
    """MAT1, MAT2, MAT4 and DIAG_ALL with constants that are no float32 numbers.  After ``set_consts64`` the run
    is the full-precision reference; a plan with the float32 blob alone is the reference with float32-rounded
    constants (to 1e-12) and NOT the full-precision one (by more than 1e-9): each path is the one that ran."""
    N = _N()
    case = R.constants_case(n, resident)
    run = (lambda p, a: _resident(case, p, a)) if resident else (lambda p, a: p.run64(a, "state").cpu().numpy())
    want, want32 = R.reference_state(case), R.reference_state(case, "consts_f32")
    plan, angles = _plan(case)
    consts = case.native()[2]
    with pytest.raises(ValueError):
        plan.set_consts64(consts[:-1])
    err = _err("c", case.label, run(plan, angles), want)
    plan32, _ = _plan(case, full_precision=False)
    got32 = run(plan32, angles)
    err32, off = _err("c", case.label + " float32 blob", got32, want32), float(np.abs(got32 - want).max())
    print(f"{case.label}: float64 constants {err:.3e}; float32 blob {err32:.3e} from its own reference, "
          f"{off:.3e} from the full-precision one")
    assert err < TOL and err32 < TOL and off > 1e-9
    # the constants are part of the device image: fixed by the first complex128 run
    with pytest.raises(N.Unsupported):
        plan.set_consts64(consts)
    rc = N.lib().qmle_plan_set_consts_f64(plan32._h, consts.ctypes.data_as(C.POINTER(C.c_double)), int(consts.size))
    assert rc == -10  # QMLE_ERR_UNSUPPORTED
    assert _err("c", case.label + " again", run(plan32, angles), want32) < TOL


# ---- d. rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B,resident", R.ROWS, ids=[f"n{n}-B{B}{'-resident' if r else ''}" for n, B, r in R.ROWS])
def test_d_every_row_of_a_batch(n, B, resident):
    """About 25 gates of every kind, every row its own angles: both instantiations of the matrix builder (flat below
    64 rows, whole waves per group from 64 on), a ragged last wave, the row strides of angles, matrices and output."""
    N = _N()
    case = R.rows_case(n, B, resident)
    want = R.compared(case)
    for flags in ((0, N.PLAN_NO_MERGE) if n <= 5 else (0,)):
        plan, angles = _plan(case, flags)
        if resident:
            errs = {"state": _err("d", case.label, _resident(case, plan, angles), want["state"])}
        else:
            errs = {"state": _err("d", case.label, plan.run64(angles, "state").cpu().numpy(), want["state"]),
                    "probs": _err("d", case.label, plan.run64(angles, "probs").cpu().numpy(), want["probs"]),
                    "expval": _err("d", case.label, plan.run64(angles, "expval", case.groups).cpu().numpy(), want["expval"])}
        print(f"{case.label} flags {flags}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
        assert max(errs.values()) < TOL, (case.label, flags, errs)


def test_d_resident_rows_stop_at_the_grid_limit():
    """``apply_inplace64`` takes one grid row per sample: 65535 rows run, 65536 are QMLE_ERR_INVALID_ARG."""
    N = _N()
    plan = N.Plan([("RY", [0], [0], -1)], 1, 1)
    for B in (65535, 65536):
        th = np.linspace(0.1, 3.0, B)
        states = torch.zeros((B, 2), dtype=torch.complex128, device="cuda")
        states[:, 0] = 1.0
        angles = torch.from_numpy(th[:, None].copy()).cuda()
        if B == 65536:
            with pytest.raises(ValueError):
                N.apply_inplace64(plan, angles, states)
            ws = torch.empty(int(N.lib().qmle_apply_inplace_f64_workspace_bytes(plan._h, B)), dtype=torch.uint8, device="cuda")
            rc = N.lib().qmle_apply_inplace_f64(plan._h, C.c_void_p(angles.data_ptr()), B, C.c_void_p(states.data_ptr()),
                                                C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()), N._stream_ptr())
            assert rc == -1  # QMLE_ERR_INVALID_ARG
            assert float((states[:, 0] - 1.0).abs().max()) == 0.0  # nothing ran
        else:
            got = N.apply_inplace64(plan, angles, states).cpu().numpy()
            want = np.stack([np.cos(th / 2), np.sin(th / 2)], axis=1).astype(np.complex128)
            err = _err("d", "65535 rows", got, want)
            print(f"d 65535 resident rows at n=1: {err:.3e}")
            assert err < TOL


# ---- e. measurements -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.MEASURE_N)
def test_e_state_probs_and_expval_of_a_batch_of_three(n):
    case = R.measure_case(n, R.BATCH)
    want = R.compared(case)
    plan, angles = _plan(case)
    errs = {"state": _err("e", case.label, plan.run64(angles, "state").cpu().numpy(), want["state"]),
            "probs": _err("e", case.label, plan.run64(angles, "probs").cpu().numpy(), want["probs"]),
            "expval": _err("e", case.label, plan.run64(angles, "expval", case.groups).cpu().numpy(), want["expval"])}
    print(f"{case.label}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("n,B", R.DENSITY)
def test_e_density_of_every_row(n, B):
    """rho = |psi><psi| per row.  n = 1, 2, 3: a state is 32 to 128 bytes, less than the 256-byte alignment of the
    state buffer the LDS kernel writes for the outer product.  n = 12: 256 MiB per row, compared on the device."""
    case = R.measure_case(n, B)
    psi = R.reference_state(case)
    plan, angles = _plan(case)
    rho = plan.run64(angles, "density")
    assert rho.shape == (B, 1 << n, 1 << n) and rho.dtype == torch.complex128
    want = torch.from_numpy(psi).cuda()
    err = 0.0
    for b in range(B):
        err = max(err, float((rho[b] - torch.outer(want[b], want[b].conj())).abs().max()))
    WORST["e"] = max(WORST.get("e", 0.0), err)
    print(f"{case.label} density: {err:.3e}")
    assert err < TOL


def test_e_density_past_twelve_wires_and_bad_observables_are_refused():
    N = _N()
    case = R.measure_case(13, R.BATCH)
    plan, angles = _plan(case)
    with pytest.raises(N.Unsupported):
        plan.run64(angles[:1], "density")
    with pytest.raises(ValueError):
        plan.run64(angles, "expval", [[q % 13] for q in range(33)])
    with pytest.raises(ValueError):
        plan.run64(angles, "expval", [[0], [13]])
    with pytest.raises(ValueError):
        plan.run64(angles, "expval", [])


@pytest.mark.parametrize("n", [9, 14])
def test_e_thirty_two_observables(n):
    """The ABI's limit of <Z..Z> observables -- single wires, the parity of all wires, random subsets -- in the LDS
    kernel (n = 9) and in ``k64_expval`` (n = 14, one workgroup per row and observable)."""
    case = R.observables_case(n)
    plan, angles = _plan(case)
    got = plan.run64(angles, "expval", case.groups).cpu().numpy()
    err = _err("e", case.label, got, R.compared(case)["expval"])
    print(f"{case.label}: {err:.3e}")
    assert err < TOL


# ---- f. two rounds in the streaming regime -------------------------------------------------------------------------
def test_f_second_round_of_the_streaming_regime():
    """A round of the streaming regime is ``4 GiB / (16 << n)`` samples and 14 is its smallest n: 16384 samples, so a
    batch of 16385 is the smallest that starts a second round -- whose matrices, angles and output begin at row
    offset 16384 (about 4.1 GiB of workspace, and 4 GiB of output for ``state``).  The rows cycle through three
    angle rows; 16384 % 3 = 1, so the first row of the second round differs from row 0.  ``expval``: every row;
    ``state``: rows 0, 16383, 16384 against the reference and the norm of every row on the device.  The round
    offset of ``probs`` is exercised only through the code it shares with ``state`` (same state pointer, same
    ``b0 * D`` offset of the output)."""
    n, B = R.TWO_ROUND_N, R.TWO_ROUND_B
    assert (4 << 30) // (16 << 14) == B - 1 and n == 14
    case = R.two_round_case()
    want = R.compared(case)
    plan, angles3 = _plan(case)
    rows = torch.arange(B, device="cuda") % 3
    angles = angles3[rows].contiguous()
    ez = plan.run64(angles, "expval", case.groups).cpu().numpy()
    err_z = _err("f", case.label, ez, want["expval"][np.arange(B) % 3])
    state = plan.run64(angles, "state")
    assert state.shape == (B, 1 << n)
    errs = [_err("f", case.label, state[b].cpu().numpy(), want["state"][b % 3]) for b in (0, B - 2, B - 1)]
    norm_err = 0.0
    for b0 in range(0, B, 2048):
        norm2 = torch.view_as_real(state[b0:b0 + 2048]).pow(2).sum(dim=(1, 2))
        norm_err = max(norm_err, float((norm2.sqrt() - 1.0).abs().max()))
    WORST["f"] = max(WORST["f"], norm_err)
    print(f"f two rounds: expval of {B} rows {err_z:.3e}; state rows 0, {B - 2}, {B - 1}: "
          + ", ".join(f"{e:.3e}" for e in errs) + f"; | ||psi|| - 1 | over every row {norm_err:.3e}")
    assert err_z < TOL and max(errs) < TOL and norm_err < TOL


# ---- g. one plan object, both engines, a changed schedule ------------------------------------------------------------
def test_g_both_engines_on_one_plan_across_an_adopted_schedule():
    """``run64``, ``run`` (complex64), ``autotune``, ``run64`` again on ONE plan at n = 16: the two engines share the
    device image of the plan (``ensure_device_plan``, ``ensure_f64``), and adopting a schedule rebuilds it and may
    change the stride of the matrix row.  The two complex128 results are bit-identical."""
    case = R.schedule_case()
    want = R.reference_state(case)
    plan, angles = _plan(case)
    first = plan.run64(angles, "state").cpu().numpy()
    s32 = plan.run(angles.to(torch.float32), "state").cpu().numpy()
    rep = plan.autotune("state", 0, batch=case.B, top_k=4, reps=2)
    second = plan.run64(angles, "state").cpu().numpy()
    err = _err("g", case.label, first, want)
    print(f"{case.label}: {err:.3e}; autotune chose {rep}; complex64 differs by {np.abs(s32 - want).max():.3e}")
    assert err < TOL and np.array_equal(first, second)
    assert np.abs(s32 - want).max() < 2e-6
    z = plan.run64(angles, "expval", [[q] for q in range(case.n)]).cpu().numpy()
    assert _err("g", case.label + " expval", z, R.expval_z(want, [[q] for q in range(case.n)], case.n)) < TOL
