"""Times ``qmle_evolve_magnus`` (Hamiltonian time evolution, csrc/qmle_evolve.hip) on the GPU:

  * rows = 102400 (1024 samples x 100 gates), order 4, 256 steps, dim 2 (3 terms) and dim 4 (4 terms), the library's
    choice of lanes per row;
  * rows = 1, 8192 steps, at every lanes_per_row;
  * the same scheme in NumPy / SciPy on the host beside it, timed on a sample of rows and scaled to all of them.

Method (profiles/evolution.md): device events around `reps` back-to-back launches after two warm-up launches, reps
chosen so that the timed window is at least 0.3 s; the median of 5 such windows.  The coefficient table is made on
the device.  fp64 multiply-adds per step are counted from the code (`fma_per_step`), the series length from the
norms of the benchmark's own exponents by the kernel's rule; the fp64 vector peak is the datasheet's 78.6 TFLOP/s
(half the 157.3 TFLOP/s fp32 vector rate): one multiply-add = 2 FLOP.

    python tools/evolve_bench.py [--rows 102400] [--steps 256] [--long-steps 8192] [--host-rows 16]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP64_VECTOR_PEAK = 78.6e12


def series_terms(nu: float) -> tuple:
    """(parts, terms per part) of the kernel's 4x4 exponential for an exponent of norm bound nu (qmle_evolve.hip)."""
    parts = max(1, math.ceil(nu / 0.5)) if nu > 0.5 else 1
    x, bound, n = nu / parts, nu / parts, 1
    while n < 24 and bound >= 1e-19:
        bound *= x / (n + 1)
        n += 1
    return parts, n


def mean_series_terms(H, coef, h) -> float:
    """parts x terms of the 4x4 series, averaged over the exponentials of an order-4 sample (coef [rows, 2 steps,
    terms], h [rows]): the kernel's norm bound -- |diagonal| plus |re| + |im| of the other entries, largest row."""
    import evolution_reference as R

    c1, c2 = coef[:, 0::2], coef[:, 1::2]
    out = []
    for wa, wb in ((R.A1, R.A2), (R.A2, R.A1)):
        G = np.einsum("rnt,tij->rnij", h[:, None, None] * (wa * c1 + wb * c2), H)
        mag = np.abs(G.real) + np.abs(G.imag)
        nu = mag.sum(axis=3).max(axis=2)
        out += [np.prod(series_terms(float(x))) for x in nu.reshape(-1)]
    return float(np.mean(out))


def fma_per_step(dim: int, order: int, n_terms: int, series: float) -> float:
    """fp64 multiplies and multiply-adds per step, from the code: the weighted sum of the terms, then per exponential
    dim 2: 16 (phase times the 2x2) + 32 (E U) + 12 (radius, sinc, entries); dim 4: 64 per series term and column
    (a packed Hermitian 4x4 times a complex column: 56, the term's scale: 8), `series` terms in all."""
    exps = 2 if order == 4 else 1
    weights = n_terms * (dim * dim + (2 if order == 4 else 1))
    if dim == 2:
        return exps * (weights + 16 + 32 + 12)
    return exps * (weights + series * 4 * 64)


def device_problem(torch, dim, rows, n_steps, order, seed=0):
    """Terms and a smooth coefficient table made on the device: a Gaussian pulse's two quadratures, a constant, and
    (dim 4) a ramp; per-row amplitudes."""
    import evolution_reference as R

    case = (R.case_dim2 if dim == 2 else R.case_dim4)(11)
    H = case["H"]
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    amp = 2.0 + torch.rand(rows, 1, generator=g, device=dev, dtype=torch.float64)
    T = 2.4
    h = torch.full((rows,), T / n_steps, dtype=torch.float64, device=dev)
    n = torch.arange(n_steps, device=dev, dtype=torch.float64)[None, :]
    if order == 2:
        t = (n + 0.5) * h[:, None]
    else:
        t = torch.stack([(n + R.C1) * h[:, None], (n + R.C2) * h[:, None]], dim=2).reshape(rows, 2 * n_steps)
    env = torch.exp(-0.5 * ((t - T / 2) / (T / 4)) ** 2)
    cols = [amp * env * torch.cos(5.0 * t), amp * env * torch.sin(5.0 * t), torch.ones_like(t)]
    if dim == 4:
        cols = [cols[2], cols[0], cols[1], t / T]
    coef = torch.stack(cols, dim=2).contiguous()
    return H, coef, h


def time_launches(torch, fn, min_seconds=0.3, windows=5):
    fn(); fn()
    torch.cuda.synchronize()
    t = time.perf_counter(); fn(); torch.cuda.synchronize()
    reps = max(1, int(min_seconds / max(time.perf_counter() - t, 1e-6)) + 1)
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out)), float(min(out)), float(max(out)), reps


def host_scheme_ms(H, coef, h, order, rows_total):
    import evolution_reference as R

    t = time.perf_counter()
    R.magnus(H, coef, h, order)
    return (time.perf_counter() - t) * 1e3 * rows_total / coef.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=102400)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--long-steps", type=int, default=8192)
    ap.add_argument("--host-rows", type=int, default=16)
    args = ap.parse_args()
    import torch

    from qml_essentials_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("evolve_bench needs a GPU: no timing is taken without one")
    for dim in (2, 4):
        H, coef, h = device_problem(torch, dim, args.rows, args.steps, 4)
        k = min(args.host_rows, args.rows)
        coef_host, h_host = coef[:k].cpu().numpy(), h[:k].cpu().numpy()
        series = mean_series_terms(H, coef_host, h_host) if dim == 4 else 0.0
        lanes = N.lib().qmle_evolve_lanes(args.rows, args.steps)
        med, lo, hi, reps = time_launches(torch, lambda: N.evolve_magnus(H, coef, h, 4))
        fma = fma_per_step(dim, 4, H.shape[0], series) * args.steps * args.rows
        host = host_scheme_ms(H, coef_host, h_host, 4, args.rows)
        print(json.dumps({"case": "batch", "dim": dim, "rows": args.rows, "order": 4, "n_steps": args.steps,
                          "n_terms": int(H.shape[0]), "lanes_per_row": lanes, "ms_median": med, "ms_min": lo,
                          "ms_max": hi, "reps": reps, "mean_series_terms": series,
                          "fma_per_step": fma_per_step(dim, 4, H.shape[0], series),
                          "tflops_fp64": 2 * fma / (med * 1e-3) / 1e12,
                          "fraction_of_fp64_vector_peak": 2 * fma / (med * 1e-3) / FP64_VECTOR_PEAK,
                          "table_gib": coef.numel() * 8 / 2 ** 30,
                          "table_gib_per_s": coef.numel() * 8 / 2 ** 30 / (med * 1e-3),
                          "host_numpy_scipy_ms_scaled": host, "host_rows_timed": k}), flush=True)
        del coef
    for dim in (2, 4):
        H, coef, h = device_problem(torch, dim, 1, args.long_steps, 4)
        k_host = host_scheme_ms(H, coef.cpu().numpy(), h.cpu().numpy(), 4, 1)
        for lanes in (1, 4, 16, 64, 0):
            med, lo, hi, reps = time_launches(torch, lambda: N.evolve_magnus(H, coef, h, 4, lanes_per_row=lanes),
                                              min_seconds=0.1)
            print(json.dumps({"case": "one_row", "dim": dim, "rows": 1, "order": 4, "n_steps": args.long_steps,
                              "lanes_per_row": lanes, "chosen": N.lib().qmle_evolve_lanes(1, args.long_steps),
                              "ms_median": med, "ms_min": lo, "ms_max": hi, "reps": reps,
                              "host_numpy_scipy_ms": k_host}), flush=True)


if __name__ == "__main__":
    main()
