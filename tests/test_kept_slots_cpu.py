"""The entries that take a workspace token (qmle_run_batch_w, qmle_run_batch_map_w, qmle_run_batch_parity_w; DESIGN
4.12), host side: they are exported, their argument errors are the status codes of the entries without a token, and
every error return writes 0 over the caller's token.  What a token does on the GPU: tests/test_gpu_kept_slots.py."""
import ctypes as C
import os
import re

from qml_essentials_amd import _native as N
from tests.test_abi_cpu import he_layer_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_ENTRIES = ("qmle_run_batch_w", "qmle_run_batch_map_w", "qmle_run_batch_parity_w")


def test_the_token_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "qmle_sv.h")).read()
    bound = {name: args for name, _res, args in N.SYMBOLS}
    lib = N.lib()
    for name in W_ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert hasattr(lib, name)
        # today's entry plus one trailing `uint64_t *ws_token`
        assert bound[name][:-1] == bound[name[:-2]] and bound[name][-1] is C.POINTER(C.c_uint64), name
    assert lib.qmle_sv_version() == 150
    assert "ws_token" in header and "nobody wrote the workspace" in header


def test_every_error_return_voids_the_token():
    lib = N.lib()
    ops, slots = he_layer_ops(6)
    plan = N.Plan(ops, 6, slots)
    null = C.c_void_p(None)
    one = C.c_void_p(256)  # (never dereferenced: every call below returns before its first HIP call)
    wires = (C.c_int32 * 1)(0)
    masks = (C.c_uint32 * 1)(1)

    def voided(call):
        tok = C.c_uint64(0x1234567890ABCDEF)
        rc = call(C.byref(tok))
        assert rc < 0 and tok.value == 0, (rc, tok.value)
        return rc

    # no plan; batch 0; a measurement type that does not exist; <Z> without wires; a wire out of range
    assert voided(lambda t: lib.qmle_run_batch_w(null, one, 1, 2, wires, 1, one, one, 1024, null, t)) == -1
    assert voided(lambda t: lib.qmle_run_batch_w(plan._h, one, 0, 2, wires, 1, one, one, 1024, null, t)) == -1
    assert voided(lambda t: lib.qmle_run_batch_w(plan._h, one, 1, 9, wires, 1, one, one, 1024, null, t)) < 0
    assert voided(lambda t: lib.qmle_run_batch_w(plan._h, one, 1, 2, None, 1, one, one, 1024, null, t)) == -1
    wires[0] = 6
    assert voided(lambda t: lib.qmle_run_batch_w(plan._h, one, 1, 2, wires, 1, one, one, 1024, null, t)) < 0
    # the map entry: no map; the parity entry: no masks, a mask beyond the register
    assert voided(lambda t: lib.qmle_run_batch_map_w(plan._h, null, one, 1, 2, None, 0, one, one, 1024, null, t)) == -1
    assert voided(lambda t: lib.qmle_run_batch_parity_w(plan._h, one, 1, None, 1, one, one, 1024, null, t)) == -1
    masks[0] = 1 << 6
    assert voided(lambda t: lib.qmle_run_batch_parity_w(plan._h, one, 1, masks, 1, one, one, 1024, null, t)) < 0
    # a NULL token is the entry without one
    assert lib.qmle_run_batch_w(null, one, 1, 2, wires, 1, one, one, 1024, null, None) == \
        lib.qmle_run_batch(null, one, 1, 2, wires, 1, one, one, 1024, null) == -1
