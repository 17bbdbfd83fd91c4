"""Times the pulse solves with sensitivities behind ``qml_essentials_amd.qoc``:

  1. one launch of ``qmle_pulse_unitaries_jac`` on ``--solves`` drag / rwa solves (5e4: what one stage-0 scan step of
     the reference's defaults asks for), on the grid that the default solver settings resolve to (the step doubling
     of ``pulses`` run once on the same table);
  2. the same Jacobian by central differences through ``qmle_pulse_unitaries``: 11 launches (the table itself and
     two shifted copies per argument) -- what the code could do before the kernel existed; the two Jacobians are
     compared;
  3. one stage-0 scan step for CRX end to end (``--candidates`` candidates x ``--samples`` rotation angles: loss and
     gradient of the unitary cost for all candidates), split into the solve (table upload, launches, synchronise),
     the copy back and the host composition (recording, table building and the dense product rule in NumPy);
  4. the same scan step with ``compose="host"`` and ``compose="device"`` alternating in one process, on the same fixed
     grid, split into the solve, the copy back, the composition (host: what is left of the evaluator; device: the call
     of ``qmle_compose_circuits`` with the upload of its tables and pools) and the rest (recording, table building,
     losses);
  5. one joint evaluation with gradient at the defaults -- 8 targets, ``--samples`` angles, the 256-candidate scan
     batch of the tied RX / RY leaf -- on both routes, alternating;
  6. the composition call of the joint evaluation alone, pools on the device, by HIP events.

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


class _Clock:
    """Host clocks around the solver, the composition call and the copies back of ``qoc``, every one closed by a
    synchronisation."""

    def __init__(self):
        import torch

        from qml_essentials_amd import _native as N
        from qml_essentials_amd import pulses

        self.torch, self.N, self.pulses = torch, N, pulses
        self.t = dict(solve=0.0, copy=0.0, compose=0.0)
        self.last_compose = None
        self._saved = (pulses.solve_with_jacobian, N.compose_circuits, N.to_host)

    def _timed(self, key, fn, keep=False):
        def wrapper(*a, **kw):
            self.torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            self.torch.cuda.synchronize()
            self.t[key] += time.perf_counter() - t0
            if keep:
                self.last_compose = (a, kw)
            return out
        return wrapper

    def __enter__(self):
        solve, compose, to_host = self._saved

        def solver(table, *a, on_device=False):  # the copy back of the host route is counted as such
            if on_device:
                return self._timed("solve", solve)(table, *a, on_device=True)
            res, steps = self._timed("solve", solve)(table, *a, on_device=True)
            out = self._timed("copy", lambda: res.cpu().numpy().reshape(len(table), 6, 2, 2))()
            return out[:, 0], out[:, 1:], steps

        self.pulses.solve_with_jacobian = solver
        self.N.compose_circuits = self._timed("compose", compose, keep=True)
        self.N.to_host = self._timed("copy", to_host)
        return self

    def __exit__(self, *exc):
        self.pulses.solve_with_jacobian, self.N.compose_circuits, self.N.to_host = self._saved

    def reset(self):
        self.t.update(solve=0.0, copy=0.0, compose=0.0)


def _alternate(evaluate, reps, clock):
    """``evaluate(route)`` for "host" and "device" in turn, ``reps`` rounds after one warm-up round -> per route the
    whole step and its split."""
    out = {route: dict(whole=[], solve=[], copy=[], compose=[]) for route in ("host", "device")}
    for rep in range(reps + 1):
        for route in ("host", "device"):
            clock.reset()
            t0 = time.perf_counter()
            evaluate(route)
            whole = time.perf_counter() - t0
            if rep:
                out[route]["whole"].append(whole)
                for key in ("solve", "copy", "compose"):
                    out[route][key].append(clock.t[key])
    res = {}
    for route, t in out.items():
        rest = [w - s - c - k for w, s, c, k in zip(t["whole"], t["solve"], t["copy"], t["compose"])]
        res[route] = dict(whole_step=stats(t["whole"]), solve=stats(t["solve"]), copy_back=stats(t["copy"]))
        if route == "device":
            res[route].update(composition_call=stats(t["compose"]), rest=stats(rest))
        else:
            res[route].update(host_composition_and_rest=stats(rest))
    lo = {route: res[route]["whole_step"] for route in res}
    res["ranges_overlap"] = not (lo["device"]["max_ms"] < lo["host"]["min_ms"] or lo["host"]["max_ms"] < lo["device"]["min_ms"])
    return res


def bench_routes(args) -> list:
    """Cases 4 to 6: the CRX scan step and the joint evaluation on both routes, then the composition call alone."""
    import torch

    from qml_essentials_amd import _native as N
    from qml_essentials_amd import qoc
    from qml_essentials_amd.evolution import Evolution
    from qml_essentials_amd.gates import PulseInformation
    from qml_essentials_amd.script import Script

    steps = 32
    Evolution._solver_defaults.update(solver="magnus4", magnus_steps=steps)
    q = qoc.QOC(**{**qoc.default_qoc_params, "n_samples": args.samples})
    pulse_circuit, target_circuit = q.create_CRX()
    pp = np.asarray(PulseInformation.CRX.params, dtype=np.float64)
    cand = pp * np.random.default_rng(12).uniform(0.5, 1.5, (args.candidates, len(pp)))
    basis = lambda fn: [Script(qoc._with_basis_prep(fn, k, 2), n_qubits=2) for k in range(4)]  # noqa: E731
    scripts = (basis(pulse_circuit), basis(target_circuit))
    results = []
    with _Clock() as clock:
        values = {}

        def scan_step(route):
            values[route] = qoc.unitary_cost_fn(cand, *scripts, args.samples, 2, value_and_grad=True, compose=route)

        res = _alternate(scan_step, args.reps, clock)
        (hv, hg), (dv, dg) = values["host"], values["device"]
        results.append(dict(case="stage-0 scan step, CRX, both routes", candidates=args.candidates, samples=args.samples,
                            params=len(pp), steps=steps, **res,
                            value_difference=float(max(np.abs(a - b).max() for a, b in zip(hv, dv))),
                            gradient_difference=float(max(np.abs(a - b).max() for a, b in zip(hg, dg))),
                            gradient_scale=float(max(np.abs(a).max() for a in hg))))
        # the joint evaluation: the scan batch of the tied RX / RY leaf
        theta, slices, _ = q._build_joint_layout(q.JOINT_LEAVES_DEFAULT)
        specs = q._joint_specs(q.JOINT_TARGETS_DEFAULT, slices, q.JOINT_WEIGHTS_DEFAULT)
        sl = slices["RX"]
        grid, _ = q._build_scan_grid(sl.stop - sl.start, init_pulse_params=theta[sl])
        batch = np.repeat(theta[None], len(grid), axis=0)
        batch[:, sl] = grid

        def joint(route):
            values[route] = qoc.joint_unitary_cost_fn(batch, specs, args.samples, value_and_grad=True, compose=route)

        res = _alternate(joint, max(2, args.reps // 2), clock)
        (hv, hg), (dv, dg) = values["host"], values["device"]
        call = clock.last_compose
        results.append(dict(case="joint evaluation with gradient", targets=len(specs), candidates=len(batch),
                            samples=args.samples, theta=len(theta), steps=steps, **res,
                            value_difference=float(max(np.abs(a - b).max() for a, b in zip(hv, dv))),
                            gradient_difference=float(max(np.abs(a - b).max() for a, b in zip(hg, dg))),
                            gradient_scale=float(max(np.abs(a).max() for a in hg))))
    # the composition call alone: the joint evaluation's tables, pools already on the device
    (circuits, ops, terms, rows, C, mats, coefs, targets, jac, mask), kw = call
    dev = N.current_device()
    on_device = lambda x: None if x is None else (x if hasattr(x, "is_cuda") else torch.from_numpy(x).to(dev))  # noqa: E731
    mats, coefs, targets, jac = (on_device(x) for x in (mats, coefs, targets, jac))
    t_events = []
    for rep in range(args.reps + 1):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        N.compose_circuits(circuits, ops, terms, rows, C, mats, coefs, targets, jac, mask, **kw)
        end.record()
        torch.cuda.synchronize()
        if rep:
            t_events.append(start.elapsed_time(end) * 1e-3)
    lanes = int(sum(-(-C * (int(K["n_params"]) + 1) * 2 ** int(K["n_wires"]) // 4) * 4 for K in circuits))
    table_bytes = int(circuits.nbytes + ops.nbytes + terms.nbytes + rows.nbytes)
    pool_bytes = int(sum(x.numel() * x.element_size() for x in (mats, coefs, targets) if x is not None))
    results.append(dict(case="composition call alone (table upload + launch, HIP events)", circuits=len(circuits),
                        ops=len(ops), terms=len(terms), lanes=lanes, table_bytes=table_bytes, pool_bytes=pool_bytes,
                        jacobian_table_bytes=int(jac.numel() * 16), overlap_bytes_back=int(kw["ov_len"]) * 16,
                        call=stats(t_events)))
    return results


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
    results = [bench_launch(args), bench_scan_step(args)] + bench_routes(args)
    for r in results:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
