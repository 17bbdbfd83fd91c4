"""A/B of the two gradients of a NOISY model: the parameter-shift rule through the density-matrix forward pass against
``Model.gradient(method="adjoint", noisy=True)`` (``qmle_adjoint_density``), in ONE process, alternating runs.

    python3 tools/density_adjoint_bench.py [--qubits 8 10 12] [--reps 3] [--out profiles/density_adjoint_ab.json]

Noisy ``Model(n, 3, "Circuit_19")``, ``wrt="params"``, ``force_mean=True`` and the full Jacobian.
``Model.gradient(method="parameter-shift")`` does not take a model with noise, so the rule is formed here from the
model's own batched forward pass: every shifted parameter set is one row of ONE call (two shifts for the RX / RZ
angles, four for the CRX angles) -- the fastest form of that rule the front end offers, and it gives the whole Jacobian.
Times are wall-clock around calls that end in a device synchronise (host work included), best and median of ``reps``;
the share of the HBM peak is the sweep's modelled transfers (``adjoint.DensitySweep.transfers``) x state bytes over
that time -- an end-to-end figure, not a kernel's.

The step kernels' OWN time comes from a kernel trace in a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -o kt --output-format csv -- python3 tools/density_adjoint_bench.py --profile 12
    python3 tools/density_adjoint_bench.py --kernel-stats DIR/.../kt_kernel_stats.csv --profile 12

``--profile N`` runs only the ``force_mean`` sweep at ``N`` qubits (one sample, one cotangent: a forward step launch moves
two states, a backward one three); ``--kernel-stats`` reads the trace's per-kernel averages and prints, per step kernel,
its time per launch and the share of the HBM peak those modelled bytes reach in it."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HBM_PEAK = 8.0e12  # bytes / s (MI355X)
NOISE = {"BitFlip": 0.01, "PhaseFlip": 0.015, "Depolarizing": 0.02, "AmplitudeDamping": 0.05, "PhaseDamping": 0.06}


def shifted_params(params, n):
    """-> (stack [R, *params.shape], per row (flat index, coefficient)): the shift rule of every angle"""
    rows, how = [], []
    cp, cm = (np.sqrt(2) + 1) / (4 * np.sqrt(2)), (np.sqrt(2) - 1) / (4 * np.sqrt(2))
    flat = params.reshape(-1)
    per_layer = params.shape[-1]
    for i in range(flat.size):
        controlled = (i % per_layer) >= 2 * n  # Circuit_19: RX, RZ on every wire, then the ring of CRX
        rule = [(np.pi / 2, cp), (-np.pi / 2, -cp), (3 * np.pi / 2, -cm), (-3 * np.pi / 2, cm)] if controlled \
            else [(np.pi / 2, 0.5), (-np.pi / 2, -0.5)]
        for shift, coef in rule:
            p = flat.copy()
            p[i] += shift
            rows.append(p.reshape(params.shape))
            how.append((i, coef))
    return np.stack(rows), how


def kernel_stats(path, n, out=None):
    """Per step kernel of a ``--profile n`` trace: launches, mean time, modelled bytes per launch (two states forward,
    three backward, one sample and one cotangent) and the share of the HBM peak they reach in that time."""
    import csv

    state = 8 << (2 * n)
    rows = []
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        if "k_dens_fwd" not in name and "k_dens_bwd" not in name:
            continue
        avg_ns = float(r.get("AverageNs") or r.get("Average") or 0.0)
        moved = (2 if "k_dens_fwd" in name else 3) * state
        rows.append({"kernel": name, "launches": int(float(r.get("Calls") or 0)), "mean_us": avg_ns / 1e3,
                     "modelled_bytes_per_launch": moved, "share_of_hbm_peak": moved / (avg_ns * 1e-9) / HBM_PEAK if avg_ns else None})
    for row in rows:
        print(json.dumps(row), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, nargs="+", default=[8, 10, 12])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", type=int, default=None, help="only the force_mean sweep at this size (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a trace of --profile N: summarise the step kernels")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.profile or 12, a.out)
    import torch

    from qml_essentials_amd import adjoint
    from qml_essentials_amd.model import Model

    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    results = []
    for n in ([a.profile] if a.profile is not None else a.qubits):
        model = Model(n_qubits=n, n_layers=3, circuit_type="Circuit_19", output_qubit=-1)
        model.noise_params = dict(NOISE)
        rng = np.random.default_rng(n)
        params = rng.uniform(0, 2 * np.pi, size=model.params.shape[1:])
        inputs = rng.uniform(0, 2 * np.pi, size=(1,))
        stack, how = shifted_params(params, n)

        def shift():
            out = np.asarray(model(params=stack, inputs=inputs, execution_type="expval")).reshape(len(how), -1)
            jac = np.zeros((out.shape[1], params.size))
            for (i, coef), row in zip(how, out):
                jac[:, i] += coef * row
            torch.cuda.synchronize()
            return jac

        def sweep(force_mean):
            g = model.gradient(params=params, inputs=inputs, wrt="params", method="adjoint", noisy=True,
                               force_mean=force_mean)
            torch.cuda.synchronize()
            return np.asarray(g)

        state = 8 << (2 * n)
        if a.profile is not None:
            for _ in range(3):
                sweep(True)
            continue
        jac_shift, mean_sweep, jac_sweep = shift(), sweep(True), sweep(False)  # warm-up: plans, code objects
        plan = adjoint.last_density_sweep()  # what the sweep moves: the plan of the call just made
        diff = float(np.abs(jac_shift.reshape(jac_sweep.shape) - jac_sweep).max())
        times = {"shift": [], "sweep_mean": [], "sweep_jacobian": []}
        for _ in range(a.reps):  # alternating
            for name, f in (("shift", shift), ("sweep_mean", lambda: sweep(True)), ("sweep_jacobian", lambda: sweep(False))):
                t0 = time.perf_counter()
                f()
                times[name].append(time.perf_counter() - t0)
        row = {"n": n, "angles": int(params.size), "shifted_circuits": len(how), "steps": len(plan.steps),
               "checkpoints": plan.checkpoints, "checkpoint_bytes": plan.checkpoints * state,
               "max_abs_diff_shift_vs_sweep": diff, "mean_of_jacobian_vs_mean_sweep":
               float(np.abs(jac_sweep.mean(axis=0) - mean_sweep).max())}
        for name, ts in times.items():
            row[name + "_best_s"], row[name + "_median_s"] = min(ts), float(np.median(ts))
        for name, k in (("sweep_mean", 1), ("sweep_jacobian", n)):
            moved = plan.transfers(k) * state
            row[name + "_modelled_bytes"] = moved
            row[name + "_share_of_hbm_peak"] = moved / row[name + "_best_s"] / HBM_PEAK
        row["speedup_mean"] = row["shift_best_s"] / row["sweep_mean_best_s"]
        row["speedup_jacobian"] = row["shift_best_s"] / row["sweep_jacobian_best_s"]
        results.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
