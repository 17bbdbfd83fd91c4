"""Writes tests/golden/product_form/{inputs,records}.npy: what `qmle_group_product_form` of the library at LIB returns
for a fixed set of groups -- taken once from the library of the commit before the measured mode came in, so that
tests/test_measured_product_form_cpu.py can hold the phase-exact records to those values bit for bit.

    python tests/golden/make_product_form_fixtures.py LIB

inputs.npy   [K, 4, 8] float64   four 2x2 matrices per case (row-major re / im); a case on k bits uses the first k
records.npy  [K, 80] float64     the record of case i on BIT_SETS[i % 7] (tests/test_group_product_form_cpu.py)"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.test_group_product_form_cpu import BIT_SETS  # noqa: E402
from tests.test_unit_form_gates_cpu import _fused, _ry, _rz  # noqa: E402


def cases():
    rng = np.random.default_rng(95)
    out = []
    for k in range(42):
        us = [_fused(*rng.uniform(0, 2 * np.pi, 3)) for _ in range(4)]
        if k % 3 == 1:   # as a chain leaves them: U / pivot three times, then P U
            piv = [u[0, 0] if abs(u[0, 0]) >= abs(u[0, 1]) else u[0, 1] for u in us]
            us = [us[0] / piv[0], us[1] / piv[1], us[2] / piv[2], np.prod(piv[:3]) * us[3]]
        out.append(us)
    r = np.sqrt(0.5)
    for m in (np.eye(2), _ry(np.pi), _rz(0.9), np.array([[r, -r], [r, r]]), np.array([[0, -1], [1, 0]]), _ry(np.pi / 2),
              _ry(2.2)):
        out += [[np.asarray(m, dtype=np.complex128)] * 4] * 2
    return np.ascontiguousarray(np.asarray(out, dtype=np.complex128).reshape(len(out), 4, 4)).view(np.float64).reshape(len(out), 4, 8)


def main(lib_path):
    lib = C.CDLL(lib_path)
    u = cases()
    rec = np.zeros((len(u), 80))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for i in range(len(u)):
        bits = BIT_SETS[i % len(BIT_SETS)]
        ui = np.ascontiguousarray(u[i, :len(bits)])
        assert lib.qmle_group_product_form(dp(ui), (C.c_int * len(bits))(*bits), len(bits), dp(rec[i]), None) == 0
    os.makedirs(os.path.join(HERE, "product_form"), exist_ok=True)
    np.save(os.path.join(HERE, "product_form", "inputs.npy"), u)
    np.save(os.path.join(HERE, "product_form", "records.npy"), rec)
    print(u.shape, rec.shape)


if __name__ == "__main__":
    main(sys.argv[1])
