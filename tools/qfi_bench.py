"""qmle_gram and end-to-end QFI timings; prints one JSON line.

  python tools/qfi_bench.py [--reps 5]

Gram cases: (n = 20, 241 rows) and (n = 24, 73 rows), one group each (Hermitian: the upper block triangle
is computed, the flop count below is the full product 8 d R^2 the roofline is quoted against); the
small-register case (n = 6, 37 rows, 10^4 groups); end-to-end QFI per point of
Model(20, 4, "Hardware_Efficient") (P = 240, 241 rows).  Peak: 157.3 TFLOP/s f32 MFMA."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 157.3


def _time(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    from qml_essentials_amd import _native as N
    from qml_essentials_amd.model import Model

    out = {"peak_tflops_f32_mfma": PEAK_TF}
    for n, rows, groups in ((20, 241, 1), (24, 73, 1), (6, 37, 10000)):
        d = 1 << n
        s = torch.randn((groups, rows, d), dtype=torch.complex64, device="cuda")
        ms = _time(lambda: N.gram(s), a.reps)
        flop = 8.0 * d * rows * rows * groups
        tf = flop / (ms * 1e-3) / 1e12
        out[f"gram_n{n}_r{rows}_g{groups}"] = {"ms": round(ms, 4), "tflops": round(tf, 2),
                                               "frac_peak": round(tf / PEAK_TF, 3),
                                               "hbm_gb": round(groups * rows * d * 8 / 1e9, 3)}
        del s
        torch.cuda.empty_cache()
    model = Model(n_qubits=20, n_layers=4, circuit_type="Hardware_Efficient")
    p = np.random.default_rng(0).uniform(0, 2 * np.pi, model.params.shape[1:]).astype(np.float32)
    ms = _time(lambda: model.quantum_fisher_information(params=p, inputs=np.array([0.5])), max(1, a.reps // 2))
    out["qfi_model20x4_he"] = {"P": int(p.size), "ms_per_point": round(ms, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
