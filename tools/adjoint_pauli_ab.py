#!/usr/bin/env python3
"""A/B timing of gradients for observables with X / Y / Hermitian factors: ONE adjoint sweep seeded with
``lambda = H psi`` (``Script.vjp`` -> ``qmle_adjoint_gradient_pauli``) against the parameter-shift Jacobian
contracted with the cotangent (``cotangent @ Script.gradient``), which is all there was for these observables
before the sweep had a Pauli seed.

Rows: a Hardware_Efficient-style script (RY RZ RY per wire, a brick of CX; 3 n angles) at 16 and 20 qubits,
batch 8, observables ``[X_0, X_1 Y_2 Z_3, Hermitian on wires (n // 2, 1)]``.  Per row:
  * ``vjp_ms`` / ``shift_ms``: the two routes end to end, host clock around calls that end in a device-to-host
    copy; after a warm-up round the routes alternate for ``--rounds`` rounds of ``--reps`` calls; median over the
    rounds, spread (max - min) beside it as ``*_spread``; ``max_abs_diff`` between their results.
  * ``seed_ms``: ``_native.apply_pauli_sum`` alone on the circuit's states in HBM (HIP events; what a caller pays
    per call: host planner, workspace allocation, table upload, coefficient kernel and the pass) with the
    3-observable list, and ``seed_z_ms`` with an all-Z list of 3 observables (one pass, x = 0 words);
    ``seed_gbs`` = (one read of psi + one write of lambda) x batch x state bytes over it, a lower bound of the
    kernels' rate.
``--trace`` instead runs a few Z sweeps and Pauli sweeps and nothing else: under ``rocprofv3 --kernel-trace
--stats`` the kernel table then holds k_zsum_apply beside k_pauli_apply_tile / k_pauli_coef on the same states.
One JSON line per row.

    python tools/adjoint_pauli_ab.py [--reps 2] [--rounds 3] [--qubits 16,20] [--batch 8] [--trace]
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
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--qubits", default="16,20")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()

    import torch

    import __graft_entry__ as G

    G.build()
    from qml_essentials_amd import _native as N
    from qml_essentials_amd import simulation
    from qml_essentials_amd import operations as op
    from qml_essentials_amd.batching import Batched
    from qml_essentials_amd.script import Script

    def host_ms(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    def events_ms(fn, reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / reps

    for n in (int(q) for q in args.qubits.split(",")):
        def circuit(th):
            for q in range(n):
                op.RY(th[q], wires=q); op.RZ(th[n + q], wires=q); op.RY(th[2 * n + q], wires=q)
            for q in range(0, n - 1, 2):
                op.CX(wires=[q, q + 1])
            for q in range(1, n - 1, 2):
                op.CX(wires=[q, q + 1])

        rng = np.random.default_rng(n)
        h = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
        obs = [op.PauliX(0, record=False),
               op.prod(op.PauliX(1, record=False), op.PauliY(2, record=False), op.PauliZ(3, record=False)),
               op.Hermitian(h + h.conj().T, wires=[n // 2, 1], record=False)]
        z_obs = [op.PauliZ(w, record=False) for w in (0, n // 2, n - 1)]
        B = args.batch
        theta = rng.uniform(0, 2 * np.pi, (B, 3 * n))
        cot = rng.normal(size=(B, len(obs)))
        script = Script(circuit, n_qubits=n)

        vjp = lambda: script.vjp(obs, cot, args=(theta,), in_axes=(0,), pauli_seed=True)[0]  # noqa: E731
        shift = lambda: np.einsum("bk,bkp->bp", cot, script.gradient(obs, args=(theta,), in_axes=(0,))[0])  # noqa: E731
        if args.trace:
            for _ in range(3):
                script.vjp(z_obs, cot, args=(theta,), in_axes=(0,))
                vjp()
            torch.cuda.synchronize()
            continue

        low = simulation.LoweredTape(script._record(Batched(theta, [])), n)
        states = simulation.get_plan(low).run(torch.from_numpy(low.angle_table(B)).cuda(), "state")
        w = torch.from_numpy(cot.astype(np.float32)).cuda()
        terms, z_terms = simulation.pauli_term_list(obs, n), simulation.pauli_term_list(z_obs, n)
        seed = lambda: N.apply_pauli_sum(states, terms, w)      # noqa: E731
        seed_z = lambda: N.apply_pauli_sum(states, z_terms, w)  # noqa: E731

        diff = float(np.abs(vjp() - shift()).max())
        samples = {}
        for _rnd in range(args.rounds + 1):  # round 0 warms every leg up and is dropped
            for name, fn in (("vjp_ms", vjp), ("shift_ms", shift)):
                samples.setdefault(name, []).append(host_ms(fn, args.reps))
            for name, fn in (("seed_ms", seed), ("seed_z_ms", seed_z)):
                samples.setdefault(name, []).append(events_ms(fn, 10 * args.reps))
        res = {}
        for key, vals in samples.items():
            res[key] = float(np.median(vals[1:]))
            res[key + "_spread"] = float(max(vals[1:]) - min(vals[1:]))
        reads, reads_z = N.apply_pauli_reads(n, terms), N.apply_pauli_reads(n, z_terms)
        # a one-pass list moves one read of psi and one write of lambda (both lists here are one pass)
        moved = 2 * B * (8 << n) if reads == 1 and reads_z == 1 else float("nan")
        print(json.dumps(dict(
            n=n, batch=B, angles=3 * n, n_obs=len(obs), words=len({(x, z) for _, x, z, _ in terms}),
            reads=reads, reads_z=reads_z, max_abs_diff=diff, speedup=res["shift_ms"] / res["vjp_ms"],
            seed_gbs=moved / (res["seed_ms"] * 1e-3) / 1e9, seed_z_gbs=moved / (res["seed_z_ms"] * 1e-3) / 1e9,
            **res)), flush=True)
        del states
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
