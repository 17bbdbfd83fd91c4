"""Times the pulse solves with sensitivities behind ``qml_essentials_amd.qoc``:

  1. one launch of ``qmle_pulse_unitaries_jac`` on ``--solves`` drag / rwa solves (5e4: what one stage-0 scan step of
     the reference's defaults asks for), on the grid that the default solver settings resolve to (the step doubling
     of ``pulses`` run once on the same table);
  2. the same Jacobian by central differences through ``qmle_pulse_unitaries``: 11 launches (the table itself and
     two shifted copies per argument) -- what the code could do before the kernel existed; the two Jacobians are
     compared;
  3. one stage-0 scan step for CRX end to end (``--candidates`` candidates x ``--samples`` rotation angles: loss and
     gradient of the unitary cost for all candidates), split into the solve (table upload, launches, synchronise),
     the copy back and the host composition (recording, table building and the dense product rule in NumPy).

Method (profiles/qoc.md): host clock; every timed piece ends with a synchronisation or a device-to-host copy; ``--reps``
rounds after one warm-up round; median, min and max.

    python tools/qoc_bench.py [--solves 50000] [--candidates 256] [--samples 20] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    xs = sorted(xs)
    return dict(median_ms=1e3 * xs[len(xs) // 2], min_ms=1e3 * xs[0], max_ms=1e3 * xs[-1])


def solve_table(n: int) -> np.ndarray:
    """n drag solves around the optimised RX / RY defaults: parameters within +-50 %, w in [0, 2 pi), both axes."""
    from qml_essentials_amd.gates import PulseEnvelope

    rng = np.random.default_rng(11)
    table = np.zeros((n, 8))
    for axis, name in enumerate(("RX", "RY")):
        pp = np.asarray(PulseEnvelope.get("drag")["defaults"][name], dtype=np.float64)
        rows = slice(axis, n, 2)
        count = len(range(n)[rows])
        table[rows, :3] = pp[:3] * rng.uniform(0.5, 1.5, (count, 3))
        table[rows, 3] = rng.uniform(0, 2 * np.pi, count)
        table[rows, 4] = pp[3] * rng.uniform(0.5, 1.5, count)
        table[rows, 5] = axis
    return table


def bench_launch(args) -> dict:
    import torch

    from qml_essentials_amd import _native as N
    from qml_essentials_amd import pulses
    from qml_essentials_amd.gates import PulseGates

    table = solve_table(args.solves)
    oc, oq = float(PulseGates.omega_c), float(PulseGates.omega_q)
    _, _, steps = pulses.solve_with_jacobian(table, "drag", "rwa", oc, oq)  # the grid the defaults resolve to
    h = 1e-6
    t_jac, t_fd, t_kernel = [], [], []
    for rep in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        jac = N.pulse_unitaries_jac(table, "drag", "rwa", oc, oq, 4, steps).cpu().numpy()
        t1 = time.perf_counter()
        shifted = []
        for col in range(5):
            e = np.zeros(8)
            e[col] = h
            up = N.pulse_unitaries(table + e, "drag", "rwa", oc, oq, 4, steps).cpu().numpy()
            down = N.pulse_unitaries(table - e, "drag", "rwa", oc, oq, 4, steps).cpu().numpy()
            shifted.append((up - down) / (2 * h))
        base = N.pulse_unitaries(table, "drag", "rwa", oc, oq, 4, steps).cpu().numpy()
        t2 = time.perf_counter()
        dev = torch.from_numpy(table).to(N.current_device())
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        N.pulse_unitaries_jac(dev, "drag", "rwa", oc, oq, 4, steps)
        end.record()
        torch.cuda.synchronize()
        if rep:
            t_jac.append(t1 - t0), t_fd.append(t2 - t1), t_kernel.append(start.elapsed_time(end) * 1e-3)
    fd = np.stack(shifted, axis=1)
    return dict(case="launch", solves=args.solves, envelope="drag", mode="rwa", order=4, steps=int(steps),
                lanes=int(N.lib().qmle_evolve_lanes(args.solves, int(steps))),
                jac_one_launch=stats(t_jac), jac_launch_alone=stats(t_kernel), central_differences_11_launches=stats(t_fd),
                u_difference=float(np.abs(jac[:, 0] - base).max()),
                jacobian_difference=float(np.abs(jac[:, 1:] - fd).max()), difference_step=h)


def bench_scan_step(args) -> dict:
    import torch

    from qml_essentials_amd import _native as N
    from qml_essentials_amd import qoc
    from qml_essentials_amd.gates import PulseInformation
    from qml_essentials_amd.script import Script

    q = qoc.QOC(**{**qoc.default_qoc_params, "n_samples": args.samples})
    pulse_circuit, target_circuit = q.create_CRX()
    pp = np.asarray(PulseInformation.CRX.params, dtype=np.float64)
    cand = pp * np.random.default_rng(12).uniform(0.5, 1.5, (args.candidates, len(pp)))
    clock = dict(solve=0.0, copy=0.0, rows=0)
    steps = 32

    def solver(table, envelope, mode, omega_c, omega_q):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = N.pulse_unitaries_jac(table, envelope, mode, omega_c, omega_q, 4, steps)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = out.cpu().numpy()
        clock["solve"] += t1 - t0
        clock["copy"] += time.perf_counter() - t1
        clock["rows"] = len(table)
        return out[:, 0], out[:, 1:], steps

    basis = lambda fn: [Script(qoc._with_basis_prep(fn, k, 2), n_qubits=2) for k in range(4)]  # noqa: E731
    total = qoc.Cost(qoc.unitary_cost_fn, (0.5, 0.5), dict(
        pulse_basis_scripts=basis(pulse_circuit), target_basis_scripts=basis(target_circuit), n_samples=args.samples,
        n_qubits=2, solver=solver)) + None
    log_p = q._to_log_space(cand)
    t_all, t_solve, t_copy = [], [], []
    for rep in range(args.reps + 1):
        clock.update(solve=0.0, copy=0.0)
        t0 = time.perf_counter()
        loss, grads = q._value_and_grad_log(total, log_p)
        t1 = time.perf_counter()
        if rep:
            t_all.append(t1 - t0), t_solve.append(clock["solve"]), t_copy.append(clock["copy"])
    host = [a - s - c for a, s, c in zip(t_all, t_solve, t_copy)]
    return dict(case="stage-0 scan step, CRX", candidates=args.candidates, samples=args.samples, params=len(pp),
                steps=steps, requests=args.candidates * args.samples * 6, solves_launched=clock["rows"],
                whole_step=stats(t_all), solve=stats(t_solve), copy_back=stats(t_copy), host_composition=stats(host),
                finite_losses=int(np.isfinite(loss).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solves", type=int, default=50000)
    ap.add_argument("--candidates", type=int, default=256)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("qoc_bench.py needs a GPU")
    results = [bench_launch(args), bench_scan_step(args)]
    for r in results:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
