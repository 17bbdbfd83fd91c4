"""Times the two kernels behind explicit matrices and Hamiltonian evolution on three and four wires:

  * ``qmle_apply_matrix`` (csrc/qmle_direct.hip) at n = 26 and 28, batch 1, k = 3 and 4, complex64 and complex128, on
    three wire sets -- the top positions, the bottom positions (0 .. k - 1) and a scattered set -- as bytes moved
    (one read and one write of the state) over time, beside the yardstick of the same session: the one-qubit
    streaming pass (``k_direct_1q`` through a ``PLAN_NO_FUSION`` plan and ``qmle_apply_inplace``; complex128: the same
    plan through ``qmle_apply_inplace_f64``), which moves the same bytes.  A k-wire pass replaces k of them.
  * ``qmle_evolve_magnus_wide`` (csrc/qmle_evolve.hip) at dim 8 and 16: 1024 rows x 256 steps of order 4 with the
    library's choice of lanes per row, and one row x 8192 steps at every lanes_per_row; the dim-4 kernel
    (``qmle_evolve_magnus``) on the same table shapes beside them.

Method (profiles/wide_gates.md): two warm-up launches, then device events around `reps` back-to-back launches, reps
chosen so that a window is at least 0.2 s; candidate and yardstick alternate, 5 windows each, the median is reported.

    python tools/wide_gate_bench.py [--qubits 26 28] [--rows 1024] [--steps 256] [--long-steps 8192] [--skip-solver]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12  # bytes / s, the datasheet's rate


def window(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def reps_for(torch, fn, min_seconds):
    fn(); fn()
    torch.cuda.synchronize()
    t = time.perf_counter(); fn(); torch.cuda.synchronize()
    return max(1, int(min_seconds / max(time.perf_counter() - t, 1e-6)) + 1)


def alternate(torch, fns, min_seconds=0.2, windows=5):
    """Median ms per launch of every function, their windows taken in turn."""
    reps = [reps_for(torch, f, min_seconds) for f in fns]
    out = [[] for _ in fns]
    for _ in range(windows):
        for i, f in enumerate(fns):
            out[i].append(window(torch, f, reps[i]))
    return [float(np.median(o)) for o in out], reps


def wire_sets(k, n):
    """As wires (wire w = position n - 1 - w): the top positions, positions 0 .. k - 1, and a scattered set."""
    step = (n - 1) // (k - 1)
    return {"top": list(range(k)), "bottom": list(range(n - k, n)),
            "scattered": [n - 1 - min(n - 2, 1 + i * step) for i in range(k)][::-1]}


def apply_leg(torch, N, n, f64):
    import wide_gate_reference as W

    dtype = torch.complex128 if f64 else torch.complex64
    states = torch.zeros((1, 1 << n), dtype=dtype, device="cuda")
    states[0, 0] = 1.0
    moved = 2 * states.numel() * states.element_size()
    # the yardstick: one dense one-qubit gate per pass on a middle wire (the plain pair-streaming mode of k_direct_1q)
    plan = N.Plan([("RX", [n // 2], [0], -1)], n, 1, flags=N.plan_flags(no_fusion=True))
    angle = torch.full((1, 1), 0.3, dtype=torch.float64 if f64 else torch.float32, device="cuda")
    if f64:
        yard = lambda: N.apply_inplace64(plan, angle, states)
    else:
        ws = torch.empty(max(1, plan.workspace_bytes(1, "state")), dtype=torch.uint8, device="cuda")
        yard = lambda: N.apply_inplace(plan, angle, states, workspace=ws)
    rng = np.random.default_rng(n)
    for k in (3, 4):
        U = torch.from_numpy(W.random_unitaries(rng, 1 << k)).cuda()
        for name, wires in wire_sets(k, n).items():
            (ms, yard_ms), reps = alternate(torch, [lambda: N.apply_matrix(states, wires, U), yard])
            flop_per_byte = 8 * (1 << k) / (2 * states.element_size())  # 8 flops per complex multiply-add
            print(json.dumps({"case": "apply", "n": n, "k": k, "dtype": "complex128" if f64 else "complex64",
                              "wires": name, "positions": sorted(n - 1 - w for w in wires), "ms": ms,
                              "GB_per_s": moved / ms / 1e6, "fraction_of_hbm_peak": moved / (ms * 1e-3) / HBM_PEAK,
                              "yardstick_ms": yard_ms, "yardstick_GB_per_s": moved / yard_ms / 1e6,
                              "ratio_to_yardstick": ms / yard_ms, "passes_replaced": k,
                              "flop_per_byte": flop_per_byte, "reps": reps}), flush=True)
    del states


def solver_problem(torch, dim, rows, n_steps, n_terms=4, seed=0):
    """Pauli-string terms and a smooth order-4 table made on the device: per-row amplitudes, h sum |c_i| = 2.4 / steps
    per node at most (a part or two of the series per factor on the long grid, a dozen on a coarse one)."""
    import wide_gate_reference as W

    k = dim.bit_length() - 1
    words = {1: ["X", "Y", "Z", "X"], 2: ["ZZ", "XI", "IY", "XZ"], 3: ["ZZX", "XIY", "IYZ", "YXI"],
             4: ["ZZXI", "XIYZ", "IYZX", "YXIZ"]}[k][:n_terms]
    H = np.stack([W.pauli_string(w) for w in words])
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    amp = 0.5 + 0.5 * torch.rand(rows, 1, generator=g, device=dev, dtype=torch.float64)
    T = 2.4
    h = torch.full((rows,), T / n_steps, dtype=torch.float64, device=dev)
    s = torch.arange(n_steps, device=dev, dtype=torch.float64)[None, :]
    c1, c2 = 0.5 - np.sqrt(3.0) / 6.0, 0.5 + np.sqrt(3.0) / 6.0
    t = torch.stack([(s + c1) * h[:, None], (s + c2) * h[:, None]], dim=2).reshape(rows, 2 * n_steps)
    env = torch.exp(-0.5 * ((t - T / 2) / (T / 4)) ** 2)
    cols = [amp * env * torch.cos(5.0 * t), amp * env * torch.sin(5.0 * t), 0.3 * torch.ones_like(t), 0.3 * t / T]
    return H, torch.stack(cols[:n_terms], dim=2).contiguous(), h


def solver_leg(torch, N, rows, steps, long_steps):
    for dim in (4, 8, 16):
        wide = dim > 4
        solve = (lambda H, c, h, lanes: N.evolve_magnus_wide(H, c, h, 4, lanes_per_row=lanes)) if wide else \
            (lambda H, c, h, lanes: N.evolve_magnus(H, c, h, 4, lanes_per_row=lanes))
        H, coef, h = solver_problem(torch, dim, rows, steps)
        Hd = torch.from_numpy(H).cuda() if wide else H
        chosen = N.lib().qmle_evolve_wide_lanes(rows, steps, dim) if wide else N.lib().qmle_evolve_lanes(rows, steps)
        (ms,), reps = alternate(torch, [lambda: solve(Hd, coef, h, 0)])
        print(json.dumps({"case": "solver_batch", "dim": dim, "rows": rows, "n_steps": steps, "order": 4,
                          "n_terms": int(H.shape[0]), "lanes_per_row": chosen, "ms": ms,
                          "us_per_row_step": ms * 1e3 / (rows * steps), "reps": reps}), flush=True)
        H, coef, h = solver_problem(torch, dim, 1, long_steps)
        Hd = torch.from_numpy(H).cuda() if wide else H
        for lanes in ((1, 4, 8) if dim == 8 else (1, 4) if dim == 16 else (1, 4, 16, 64)):
            (ms,), reps = alternate(torch, [lambda: solve(Hd, coef, h, lanes)], min_seconds=0.1)
            print(json.dumps({"case": "solver_one_row", "dim": dim, "rows": 1, "n_steps": long_steps, "order": 4,
                              "lanes_per_row": lanes, "ms": ms, "us_per_step": ms * 1e3 / long_steps,
                              "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, nargs="+", default=[26, 28])
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--long-steps", type=int, default=8192)
    ap.add_argument("--skip-solver", action="store_true")
    args = ap.parse_args()
    import torch

    from qml_essentials_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("wide_gate_bench needs a GPU: no timing is taken without one")
    for n in args.qubits:
        for f64 in (False, True):
            apply_leg(torch, N, n, f64)
    if not args.skip_solver:
        solver_leg(torch, N, args.rows, args.steps, args.long_steps)


if __name__ == "__main__":
    main()
