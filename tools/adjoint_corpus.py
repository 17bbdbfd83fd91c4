"""Bit-level record of the adjoint sweeps: ``python tools/adjoint_corpus.py [--lib PATH] [--out FILE]`` (needs a GPU).

One line per case -- route, case, seed, precision, then the SHA-256 of the gradient's bytes and, where the case asks
for matrix cotangents, of theirs -- and a last line with the digest over all lines.  The sweeps use no atomics, so
two runs of one library give the same file, and two libraries that compute the same thing give the same file:
``cmp`` the outputs of a build before and after a change that must not move a bit.

The cases are those of tests/test_gpu_adjoint_routes.py, test_gpu_matrix_cotangent.py and
test_gpu_matrix_cotangent2.py, through the same helpers, at the smallest shapes that reach each branch of
``adjoint_run`` / ``f64_adjoint_run``: the LDS kernel (Z and Pauli seeds, 1 and 3 samples, a dense forward group,
operator slots in global memory, a ``DIAG_ALL`` term, controlled rotations and a ``CPhase``, one-wire cotangents,
two-wire ones with t0 < t1 and t0 > t1), the streaming kernels below 14 qubits behind a 4-wire operator (one-wire
cotangents on bit position 0 and above, two-wire ones in both orders), streaming and fused at 14 qubits, the fused
route's refusal of a cotangent request with the fallback, complex128 at 3, 5 and 14 qubits, and the index form
``adjoint_cotangent`` beside ``adjoint_cotangent_at`` with offsets ``8 * index``.
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from qml_essentials_amd import _native as N  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main(argv):
    out = sys.stdout
    if "--lib" in argv:
        N.LIB_PATH = os.path.abspath(argv[argv.index("--lib") + 1])
    if "--out" in argv:
        out = open(argv[argv.index("--out") + 1], "w")
    import torch

    from qml_essentials_amd import adjoint
    from qml_essentials_amd.simulation import get_plan
    from tests import adjoint_reference as R
    from tests import matrix_cotangent2_reference as M2
    from tests import matrix_cotangent_reference as M1
    from tests import test_gpu_adjoint_routes as TR
    from tests import test_gpu_matrix_cotangent as T1
    from tests import test_gpu_matrix_cotangent2 as T2

    total = hashlib.sha256()
    flags = (adjoint.REV_FLAGS, adjoint.REV_FLAGS_FUSED)

    def emit(*words):
        line = " ".join(str(w) for w in words) + "\n"
        total.update(line.encode())
        out.write(line)
        out.flush()

    def routed(route, fn):
        """fn() with the reverse plans of `route` ("lds" and "any": as the package chooses)"""
        adjoint._REV_CACHE.clear()
        if route == "fused":
            adjoint.REV_FLAGS = flags[1]
        elif route == "streaming":
            adjoint.REV_FLAGS_FUSED = flags[0]
        try:
            return fn()
        finally:
            adjoint.REV_FLAGS, adjoint.REV_FLAGS_FUSED = flags
            adjoint._REV_CACHE.clear()

    def gradient(route, name, rows=None, x64=False):
        """a case of adjoint_reference.py, its first `rows` samples, under both seeds"""
        case = R.cases()[name]
        rows = case.theta.shape[0] if rows is None else rows
        low = TR.lowered(case, case.theta[:rows])
        _groups, _mats, wz, wp = R.case_observables(case)
        if route == "lds":
            TR.assert_lds(low, case.n)
        for seed, w in (("z", wz[:rows]), ("pauli", wp[:rows])):
            got, _w = routed(route, lambda: TR.sweep(case, low, seed, x64=x64, weights=w))
            emit(route, name, "rows", rows, seed, "x64" if x64 else "c64", sha(got))

    def cotangent(route, T, cases, name, x64=False, seeds=("z", "pauli")):
        """a case of matrix_cotangent_reference.py (T1: 2x2 blocks) or matrix_cotangent2_reference.py (T2: mixed)"""
        case = cases[name]
        low, slot_of, want_mat = T.lowered(case)
        if route == "lds":
            TR.assert_lds(low, case.n)
        for seed in seeds:
            grad, cot = routed(route, lambda: T.sweep(case, low, slot_of, want_mat, seed, x64=x64))
            cot = cot if isinstance(cot, np.ndarray) else np.concatenate([np.asarray(c).reshape(-1) for c in cot])
            emit(route, T.__name__.rsplit(".", 1)[-1], name, seed, "x64" if x64 else "c64", sha(grad), sha(cot))

    def both_forms(name):
        """adjoint_cotangent (one index per 2x2) and adjoint_cotangent_at (offsets 8 * index) on one call's arguments"""
        case = M1.cases()[name]
        low, slot_of, want_mat = T1.lowered(case)
        adjoint._REV_CACHE.clear()
        T1.sweep(case, low, slot_of, want_mat, "z")
        (rev, terms, tab), = list(adjoint._REV_CACHE.values())[-1:]
        idx, k = [], 0
        for opname, _w, _s, _o in rev.ops:
            idx.append(k if opname in ("MAT1", "MAT1_ROW") else -1)
            k += opname in ("MAT1", "MAT1_ROW")
        groups, _mats, wz, _wp = M1.case_observables(case)
        a_f = torch.from_numpy(low.angle_table(wz.shape[0])).cuda()
        a_r = (a_f.index_select(1, tab.perm) * tab.sign.float()).contiguous()
        w = torch.from_numpy(wz.astype(np.float32)).cuda()
        plans = get_plan(low), get_plan(rev, adjoint.REV_FLAGS)
        g0, c0 = N.adjoint_cotangent(*plans, a_f, a_r, w, groups, terms, low.n_slots, idx, k)
        g1, c1 = N.adjoint_cotangent_at(*plans, a_f, a_r, w, groups, terms, low.n_slots,
                                        [8 * i if i >= 0 else -1 for i in idx], 8 * k, False)
        c0 = torch.view_as_real(c0).cpu().numpy()
        emit("forms", name, "index", sha(g0.cpu().numpy()), sha(c0))
        emit("forms", name, "offset", sha(g1.cpu().numpy()), sha(c1.cpu().numpy()))
        adjoint._REV_CACHE.clear()

    one, two = M1.cases(), M2.cases()
    # ---- the LDS kernel
    gradient("lds", "lds_all_n3", rows=1)       # controlled rotations, a CPhase
    gradient("lds", "lds_all_n3", rows=3)
    gradient("lds", "lds_golomb_n5", rows=1)    # a DIAG_ALL term
    gradient("lds", "lds_golomb_n5", rows=3)
    gradient("lds", "lds_dense_n4")             # a dense forward group
    gradient("lds", "lds_deep_n13", rows=1)     # operator slots in global memory
    cotangent("lds", T1, one, "lds_n3_b1")
    cotangent("lds", T1, one, "lds_n3_b3")
    cotangent("lds", T2, two, "lds_n2")         # pairs (0, 1) and (1, 0)
    cotangent("lds", T2, two, "lds_n6")         # pairs (0, 5), (5, 0), (2, 3)
    # ---- streaming below 14 qubits: a 4-wire operator on the tape
    gradient("streaming", "mat4_n4")
    cotangent("streaming", T1, one, "stream_n5")  # bit positions 4, 0, 2, 0
    cotangent("streaming", T2, two, "stream_n5")  # pairs in both orders
    # ---- 14 qubits, two samples
    gradient("streaming", "tile_n14", rows=2)
    gradient("fused", "tile_n14", rows=2)
    cotangent("streaming", T1, one, "stream_n14")
    cotangent("streaming", T2, two, "stream_n14")
    try:
        cotangent("fused", T1, one, "stream_n14", seeds=("z",))
        emit("fused", "stream_n14", "accepted")
    except N.Unsupported:
        emit("fused", "stream_n14", "refused")
    cotangent("any", T1, one, "stream_n14", seeds=("z",))  # the fallback of run_sweep
    # ---- complex128
    gradient("x64", "lds_all_n3", x64=True)
    gradient("x64", "lds_golomb_n5", x64=True)
    gradient("x64", "tile_n14", rows=2, x64=True)
    cotangent("x64", T1, one, "lds_n3_b3", x64=True)
    cotangent("x64", T2, two, "x64_n3", x64=True)
    cotangent("x64", T1, one, "stream_n14", x64=True)
    cotangent("x64", T2, two, "stream_n14", x64=True)
    # ---- the two forms of a one-wire request
    both_forms("lds_n3_b1")
    out.write("digest %s\n" % total.hexdigest())
    if out is not sys.stdout:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
