#!/usr/bin/env python3
"""Differential check of the three routes a batched Model call can take to its gate matrices: CUDA-tensor
arguments (qmle_run_batch_map: from 64 samples on the matrices are built straight from the affine angle
map) and host arrays (the angle table formed on the host in float64, then qmle_run_batch with the matrices
built from the table).  They must agree to 2e-6; every ansatz, random sizes / encodings / batch shapes with
64+ samples.  (The bit-for-bit comparison with qmle_build_angles + qmle_run_batch is
tests/test_gpu_kernels.py's.)"""
import os, sys, warnings
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qml_essentials_amd.ansaetze import Ansaetze
from qml_essentials_amd.model import Model

warnings.simplefilter("ignore")
rng = np.random.default_rng(int(os.environ.get("FUZZ_SEED", "7")))
names = [a.__name__ for a in Ansaetze.get_available()]
bad = ran = 0
for trial in range(int(os.environ.get("FUZZ_N", "120"))):
    n = int(rng.integers(2, 13))
    kw = dict(n_qubits=n, n_layers=int(rng.integers(1, 4)), circuit_type=str(rng.choice(names)),
              data_reupload=bool(rng.integers(2)))
    if rng.random() < 0.3:
        kw["encoding"] = str(rng.choice(["RX", "RY", "RZ"]))
    try:
        m = Model(**kw)
    except Exception as e:  # (ansatz needs more qubits etc.)
        continue
    B_I, B_P = int(rng.integers(1, 80)), int(rng.choice([1, 1, 2, 3]))
    if 0 in m.params.shape:  # an ansatz without parameters: nothing to batch (model.py:1444)
        B_P = 1
    if B_I * B_P < 64:
        B_I = 64 // B_P + 1
    x = rng.uniform(-3, 3, (B_I, m.n_input_feat)).astype(np.float32)
    p = rng.uniform(0, 6.28, (B_P, *m.params.shape[-2:])).astype(np.float32)
    et = str(rng.choice(["expval", "probs"])) if n <= 10 else "expval"
    xd, pd = torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()
    try:
        a = m(params=pd, inputs=xd, execution_type=et)
    except Exception as e:
        print("ERROR", kw, B_I, B_P, et, repr(e)[:200])
        bad += 1
        continue
    c = m(params=p, inputs=x, execution_type=et)
    a = a.cpu().numpy()
    ran += 1
    ok = a.shape == np.shape(c) and np.abs(a - np.asarray(c)).max() < 2e-6
    if not ok:
        bad += 1
        print("MISMATCH", kw, B_I, B_P, et, a.shape, np.shape(c),
              float(np.abs(a - np.asarray(c)).max()) if a.shape == np.shape(c) else None)
print(f"{ran} models run, mismatches: {bad}")
