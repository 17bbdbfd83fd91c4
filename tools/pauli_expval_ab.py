#!/usr/bin/env python3
"""A/B timing of non-Z expectation values: the Pauli-word kernels (``qmle_expval_pauli``) against the
route they replace (clone + observable as a gate + overlap per observable in complex64, movedim +
einsum per observable in x64 mode).

Rows: the transverse-field Ising observables ``[X_i] + [Z_i Z_{i+1}]`` at n = 20 and 24, batch 4, and a
single two-wire Hermitian at n = 24, each in complex64 and complex128.  Two figures per row and route:
  * ``measure_ms``: the measurement alone on states already in HBM, HIP events around ``--reps`` calls;
  * ``execute_ms``: ``Script.execute(type="expval")`` end to end (circuit + measurement + download),
    host clock (the call ends in a device-to-host copy).
After a warm-up of every leg the two routes alternate for ``--rounds`` rounds, the same ``--reps`` each; every
figure is the median over the rounds, with the spread (max - min) beside it as ``*_spread``.
``measure_ms_new`` is what a caller of ``_native.expval_pauli`` pays per call: the host planner, the workspace
allocation and the upload of the term table as well as the kernels -- ``new_gbs`` = reads x batch x state
bytes over it is therefore a lower bound of the kernels' rate.  ``bytes_ratio`` = 6 x (non-Z observables) /
reads is what the bytes moved promise.  One JSON line per row.

    python tools/pauli_expval_ab.py [--reps 5] [--rounds 5] [--rows ising20,ising24,herm24] [--modes c64,x64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", default="ising20,ising24,herm24")
    ap.add_argument("--modes", default="c64,x64")
    ap.add_argument("--batch", type=int, default=4)
    args = ap.parse_args()

    import torch

    import __graft_entry__ as G

    G.build()
    from qml_essentials_amd import _native as N
    from qml_essentials_amd import jaqsi, simulation, utils
    from qml_essentials_amd import operations as op
    from qml_essentials_amd.script import Script

    def observables(row, n):
        if row.startswith("ising"):
            return ([op.PauliX(w, record=False) for w in range(n)]
                    + [jaqsi.build_parity_observable([w, w + 1]) for w in range(n - 1)])
        rng = np.random.default_rng(0)
        h = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
        return [op.Hermitian(h + h.conj().T, wires=[n // 2, 1], record=False)]

    def circuit(th):
        n = th.shape[-1]
        for q in range(n):
            op.RY(th[q], wires=q)
        for q in range(n - 1):
            op.CX(wires=[q, q + 1])

    def events_ms(fn, reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / reps

    def host_ms(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    new_list = simulation.pauli_term_list
    for row in args.rows.split(","):
        n = int(row[-2:])
        obs = observables(row, n)
        terms = new_list(obs, n)
        non_z = sum(1 for o in obs if op.z_parity_mask(o) is None)
        theta = np.random.default_rng(1).uniform(0, 2 * np.pi, (args.batch, n))
        for mode in args.modes.split(","):
            x64 = mode == "x64"
            with utils.x64_scope(x64):
                script = Script(circuit, n_qubits=n)
                low = simulation.LoweredTape(_tape(script, theta), n)
                if x64:
                    plan = simulation.get_plan(low, N.PLAN_NO_MERGE)
                    states = plan.run64(torch.from_numpy(low.angle_table(args.batch, dtype=np.float64)).cuda(),
                                        "state")
                    old = lambda: simulation._x64_observables(  # noqa: E731
                        states, n, obs, [op.z_parity_mask(o) for o in obs])
                else:
                    plan = simulation.get_plan(low)
                    states = plan.run(torch.from_numpy(low.angle_table(args.batch)).cuda(), "state")
                    old = lambda: simulation._general_expval(states, n, obs)  # noqa: E731
                new = lambda: N.expval_pauli(states, terms, len(obs))  # noqa: E731
                a, b = new(), old()
                diff = float((a.double() - b.double()).abs().max())
                execute = lambda: script.execute(type="expval", obs=obs, args=(theta,), in_axes=(0,))  # noqa: E731
                def execute_with(name):
                    simulation.pauli_term_list = new_list if name == "new" else (lambda *a, **k: None)
                    try:
                        return host_ms(execute, args.reps)
                    finally:
                        simulation.pauli_term_list = new_list

                samples = {}
                for rnd in range(args.rounds + 1):  # round 0 warms every leg up and is dropped
                    for name, fn in (("new", new), ("old", old)):
                        samples.setdefault("measure_ms_" + name, []).append(events_ms(fn, args.reps))
                    for name in ("new", "old"):
                        samples.setdefault("execute_ms_" + name, []).append(execute_with(name))
                res = {}
                for key, vals in samples.items():
                    res[key] = float(np.median(vals[1:]))
                    res[key + "_spread"] = float(max(vals[1:]) - min(vals[1:]))
                reads = N.pauli_reads(n, terms, f64=x64)
                state_bytes = (16 if x64 else 8) << n
                out = dict(row=row, mode=mode, n=n, batch=args.batch, n_obs=len(obs), non_z=non_z, reads=reads,
                           bytes_ratio=6.0 * non_z / reads, max_abs_diff=diff,
                           measure_speedup=res["measure_ms_old"] / res["measure_ms_new"],
                           execute_speedup=res["execute_ms_old"] / res["execute_ms_new"],
                           new_gbs=reads * args.batch * state_bytes / (res["measure_ms_new"] * 1e-3) / 1e9, **res)
                print(json.dumps(out), flush=True)
                del states
                torch.cuda.empty_cache()


def _tape(script, theta):
    """The circuit's tape with the batch of angles as per-sample columns."""
    from qml_essentials_amd.batching import Batched

    return script._record(Batched(np.asarray(theta, dtype=np.float64), []))


if __name__ == "__main__":
    main()
