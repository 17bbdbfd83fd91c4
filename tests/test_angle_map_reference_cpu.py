"""The plain reference of the affine angle map (tests/angle_map_reference.py) against the host's own angle table.

The map of a Model's compiled call (script.CompiledCall, host half: no GPU) is fed to the reference; the same call
recorded with the whole batch gives LoweredTape.angle_table.  The host reduces a whole column when any row exceeds
4 pi, the device (and the reference) element by element, so the two tables are equal only modulo 4 pi: the bar is one
float32 ulp of 4 pi (2^-20 = 9.54e-7).  Both sides cast a value of at most 4 pi in modulus to float32, half an ulp of
4 pi each at the worst; what the float64 sums themselves differ by (1e-12 at 1e4 rad) does not count beside that.
tests/test_gpu_angle_map_builder.py holds the kernels to this reference."""
import warnings

import numpy as np
import pytest

from tests import angle_map_reference as R

ULP_4PI = float(np.spacing(np.float32(4.0 * np.pi)))  # 9.5367e-07


def zoo():
    """(name, Model arguments) of the ansatz zoo: every available ansatz at 4 qubits and one layer, Circuit_19 under a
    binary RX / RY and under a ternary RX encoding; tests/test_gpu_angle_map_builder.py runs the same list."""
    from qml_essentials_amd.ansaetze import Ansaetze

    out = [(c.__name__, dict(circuit_type=c.__name__)) for c in Ansaetze.get_available()]
    out.append(("Circuit_19-binary", dict(circuit_type="Circuit_19", encoding=("binary", ["RX", "RY"]))))
    out.append(("Circuit_19-ternary", dict(circuit_type="Circuit_19", encoding=("ternary", ["RX"]))))
    return out


def make_model(kw, n=4, **more):
    from qml_essentials_amd.ansaetze import Encoding
    from qml_essentials_amd.model import Model

    kw = dict(kw, **more)
    if "encoding" in kw:
        kw["encoding"] = Encoding(*kw["encoding"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return Model(n, 1, **kw)


def zoo_arguments(model, n_inputs, n_params, seed, x_hi=5.0):
    """float32 inputs in [1, x_hi] and parameter sets in [0, 2 pi): the same values on the host and the device path.
    An ansatz without parameters has one (empty) parameter set: it takes n_inputs * n_params inputs instead, so that
    every model of the zoo runs the same number of samples."""
    rng = np.random.default_rng(seed)
    if 0 in model.params.shape:
        n_inputs, n_params = n_inputs * n_params, 1
    x = rng.uniform(1.0, x_hi, (n_inputs, model.n_input_feat)).astype(np.float32)
    p = rng.uniform(0, 2 * np.pi, (n_params, *model.params.shape[1:])).astype(np.float32)
    return p, x


def host_map(model, p, x):
    """The compiled call of model(params=p, inputs=x), host half, with the leaves and row rules of
    Model._device_call: -> (cc, leaves, strides, divs, mods, B)."""
    from qml_essentials_amd.script import CompiledCall

    enc = model._enc_params_validation(None)
    pv, xv = model._params_validation(p), model._inputs_validation(x)
    B_P = 1 if 0 in pv.shape else int(pv.shape[0])
    B_I = int(xv.shape[0])
    model._batch_shape = (B_I, B_P, 1)
    B = int(np.prod(model.eff_batch_shape))
    cross = bool(B_I > 1 and B_P > 1 and model.repeat_batch_axis[0] and model.repeat_batch_axis[1])
    meas_type, obs = model._build_obs()
    args = (np.asarray(pv[0]) if pv.shape[0] else np.asarray(pv), np.asarray(xv[0]), None, None, enc)
    cc = CompiledCall(model.script, meas_type, obs, args, (0, 1), dict(noise_params=None, gate_mode="unitary"),
                      upload=False)
    leaves = [None if 0 in pv.shape else np.asarray(pv, dtype=np.float32).reshape(B_P, -1),
              np.asarray(xv, dtype=np.float32).reshape(B_I, -1)]
    strides = [0 if l is None else l.shape[1] for l in leaves]
    return cc, leaves, strides, [1, B_P if cross else 1], [max(B_P, 1), B_I], B


def host_table(model, p, x):
    """LoweredTape.angle_table of the same call recorded with the whole batch (the path of
    host_arrays_via_device = False)."""
    from qml_essentials_amd import simulation
    from qml_essentials_amd.batching import Batched
    from qml_essentials_amd.tape import batch_context

    enc = model._enc_params_validation(None)
    pv, xv = model._params_validation(p), model._inputs_validation(x)
    xb, pb = model._assimilate_batch(xv, pv)
    B = int(np.prod(model.eff_batch_shape))
    wrapped = [Batched(np.asarray(pb, dtype=np.float64)) if model.batch_shape[1] > 1 else pb,
               Batched(np.asarray(xb, dtype=np.float64)) if model.batch_shape[0] > 1 else xb, None, None, enc]
    with batch_context(B):
        tape = model.script._record_for_engine(*wrapped, noise_params=None, gate_mode="unitary")
    low = simulation.LoweredTape(tape, model.n_qubits)
    return low, low.angle_table(B)


def reference_table(cc, leaves, strides, divs, mods, B, offset=0):
    ptr, arg, idx, coef = cc._map
    return R.table(leaves, strides, divs, mods, ptr, arg, idx, coef, cc._const, cc._period, B, offset)


def _compare(model, p, x):
    cc, leaves, strides, divs, mods, B = host_map(model, p, x)
    want, mask = reference_table(cc, leaves, strides, divs, mods, B)
    low, host = host_table(model, p, x)
    assert host.shape == want.shape == (B, cc.n_slots) and low.n_slots == cc.n_slots
    periodic = np.asarray(cc._period) > 0
    if periodic.any():
        d = R.mod_distance(host[:, periodic], want[:, periodic])
        assert d.max() <= ULP_4PI, d.max()
    if (~periodic).any():  # never reduced on either side: the same float32
        assert np.array_equal(host[:, ~periodic], want[:, ~periodic])
    assert np.abs(want[:, periodic]).max(initial=0.0) <= np.float32(4.0 * np.pi)
    return want, mask, host


@pytest.mark.parametrize("name,kw", zoo(), ids=[n for n, _ in zoo()])
def test_zoo_maps_give_the_host_table_modulo_four_pi(name, kw):
    model = make_model(kw)
    p, x = zoo_arguments(model, 8, 9, seed=7100)
    want, mask, _host = _compare(model, p, x)
    assert want.shape[0] == 72
    if "ternary" in name or "binary" in name:
        assert mask.any(), "an encoding angle beyond 4 pi"


def test_zipped_batch_axes_share_their_row():
    model = make_model(dict(circuit_type="Circuit_19"), repeat_batch_axis=[False, True, True])
    p, x = zoo_arguments(model, 72, 72, seed=7200)
    cc, leaves, strides, divs, mods, B = host_map(model, p, x)
    assert B == 72 and divs == [1, 1] and mods == [72, 72]
    _compare(model, p, x)


def test_ternary_encoding_at_eight_qubits_reduces_most_of_its_angles():
    """3^7 x 5 = 1.1e4 rad: the encoding slots reduce on (almost) every row."""
    model = make_model(dict(circuit_type="Circuit_19", encoding=("ternary", ["RX"])), n=8)
    p, x = zoo_arguments(model, 8, 9, seed=7300)
    want, mask, host = _compare(model, p, x)
    enc = mask.any(axis=0)
    assert enc.sum() >= 6 and mask[:, enc].mean() > 0.5
    assert np.abs(host).max() <= np.float32(4.0 * np.pi)


def test_fused_and_unfused_reduction_round_to_the_same_float32():
    """acc - per * rint(acc / per) with and without a fused multiply-subtract, on this file's kind of sums
    (coefficients 3^0 .. 3^7, leaves in +-5, the range tests/test_gpu_angle_map_builder.py uses too): the float64
    results may differ in their last bits, their float32 casts do not."""
    rng = np.random.default_rng(7400)
    coef = (3.0 ** rng.integers(0, 8, 20000)).astype(np.float32)
    leaf = rng.uniform(-5.0, 5.0, 20000).astype(np.float32)
    acc = coef.astype(np.float64) * leaf.astype(np.float64) + rng.uniform(0, 2 * np.pi, 20000).astype(np.float32)
    acc = acc[np.abs(acc) > R.FOUR_PI]
    assert len(acc) > 10000
    differ64 = 0
    for a in acc:
        f, u = R.reduce_fused(float(a), R.FOUR_PI), R.reduce_unfused(float(a), R.FOUR_PI)
        differ64 += f != u
        assert np.float32(f) == np.float32(u), (a, f, u)
        assert abs(f) <= R.FOUR_PI / 2 * (1 + 1e-15)
    print("float64 results that differ between the two forms:", differ64, "of", len(acc))


def test_reference_rows_and_boundaries():
    """The row rule on Python integers across 2^32, and the reduction's strict bounds: +-per stay, the next float64
    beyond goes."""
    assert R.row_of(5, 2 ** 32 - 3, 7, 5) == ((2 ** 32 + 2) // 7) % 5
    assert R.row_of(0, 2 ** 33 + 3, 35, 3) == ((2 ** 33 + 3) // 35) % 3
    per = 12.5  # (a float32, so that a float32 leaf reaches it exactly)
    leaf = np.array([[per, -per, np.nextafter(np.float32(per), np.float32(99)), 2 * per]], dtype=np.float32)
    m = R.identity_map(4, period=[per] * 4)
    t, mask = m.table([leaf], [4], [1], [1], 1)
    assert mask.tolist() == [[False, False, True, True]]
    assert t[0, 0] == per and t[0, 1] == -per and t[0, 3] == 0.0 and abs(t[0, 2] - (leaf[0, 2] - per)) < 1e-6
    assert R.ulp_distance(np.float32([1.0, -0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), 0.0])).tolist() == [1, 0]


def test_a_negative_batch_offset_is_refused_before_any_launch():
    """qmle_build_angles and qmle_run_batch_map_w answer QMLE_ERR_INVALID_ARG (-1) to a negative batch offset, which
    would wrap as an unsigned row; the answer comes before any launch, so it needs no GPU (the addresses handed over
    are never read)."""
    import ctypes as C

    from qml_essentials_amd import _native as N

    L = N.lib()
    cell = (C.c_float * 4)()
    p = C.addressof(cell)
    lp, ls = (C.c_void_p * 1)(p), (C.c_int64 * 1)(1)
    ld, lm = (C.c_int32 * 1)(1), (C.c_int32 * 1)(1)
    assert L.qmle_build_angles(lp, ls, ld, lm, 1, p, p, p, p, p, None, 1, 4, -1, p, None) == -1
    plan = N.Plan([("RX", [0], [0], -1)], 1, 1)
    amap = N.QmleAngleMap(C.cast(lp, C.POINTER(C.c_void_p)), C.cast(ls, C.POINTER(C.c_int64)),
                          C.cast(ld, C.POINTER(C.c_int32)), C.cast(lm, C.POINTER(C.c_int32)), 1, p, p, p, p, p, None, -1)
    token = C.c_uint64(7)
    rc = L.qmle_run_batch_map_w(plan._h, C.byref(amap), p, 64, N.MEAS["state"], None, 0, p, p, 1 << 20, None,
                                C.byref(token))
    assert rc == -1 and token.value == 0
    assert L.qmle_run_batch_map(plan._h, C.byref(amap), p, 64, N.MEAS["state"], None, 0, p, p, 1 << 20, None) == -1
