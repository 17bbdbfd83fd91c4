"""Times the pulse solves of a pulse-mode ``Model(4, 2, "Circuit_19")`` on 256 parameter sets with ``magnus4`` at 256
steps, once with the rotating-wave coefficients and once with the exact ones (frame "drive"):

  * one launch: ``pulses.resolve`` on the recorded tape -- every RX / RY leaf of the tape in one launch of
    ``qmle_pulse_unitaries``, the coefficients evaluated on the device;
  * per gate: what the code could do before that kernel existed -- per leaf one ``ParametrizedHamiltonian.evolve``
    with the coefficient functions of ``PulseEnvelope.build_coeff_fns``: the host evaluates them at every node,
    ships the table ``coef[row][node][term]``, launches ``qmle_evolve_magnus`` and copies the matrices back;
  * the whole call ``model(params, gate_mode="pulse")`` (recording, the solves, lowering, the circuit, the copy back).

Method (profiles/pulse.md): host clock around work that ends with the matrices on the host (both routes finish with
a device-to-host copy, which synchronises); the two routes alternate inside one process, ``--reps`` rounds after one
warm-up round; median, min and max.  The per-gate route is also checked against the one-launch route (largest
difference of any matrix).

    python tools/pulse_bench.py [--qubits 4] [--layers 2] [--batch 256] [--steps 256] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def record_tape(model, params, inputs):
    """The pulse tape of the model for the batch ``params`` [B, layers, n]: one recording, batched arguments."""
    from qml_essentials_amd.batching import Batched
    from qml_essentials_amd.tape import batch_context, recording

    with batch_context(params.shape[0]), recording() as tape:
        model._variational(Batched(params), inputs, pulse_params=model.pulse_params, enc_params=model.enc_params,
                           gate_mode="pulse")
    return tape


def per_gate_route(leaves, steps: int):
    """One generic ``evolve()`` per leaf, host-built coefficient table.  Returns the matrices, leaf by leaf."""
    from qml_essentials_amd import operations as op
    from qml_essentials_amd.batching import Batched
    from qml_essentials_amd.gates import PulseEnvelope, PulseGates
    from qml_essentials_amd.tape import recording

    X, Y = PulseGates.X, PulseGates.Y
    out = []
    with recording():
        for o in leaves:
            fns = PulseEnvelope.build_coeff_fns(PulseEnvelope.get(o.envelope)["fn"], o.omega_c, o.omega_q,
                                                rwa=o.mode == "rwa", frame="lab" if o.mode == "lab" else "drive")
            fx, fy = fns[:2] if o.axis == "X" else fns[2:]
            ham = fx * op.Hermitian(X, wires=o.wires, record=False) + fy * op.Hermitian(Y, wires=o.wires, record=False)
            cols = [np.broadcast_to(np.asarray(v, dtype=np.float64), (o.rows,)) for v in o.env_params + [o.w]]
            packed = np.stack(cols, axis=1)
            packed = Batched(packed, []) if o.batched_request else packed[0]
            T = Batched(np.asarray(o.T), []) if np.ndim(o.T) else float(o.T)
            out.append(ham.evolve(solver="magnus4", magnus_steps=steps)([packed, packed], T).matrix)
    return out


def stats(xs):
    xs = sorted(xs)
    return dict(median_ms=1e3 * xs[len(xs) // 2], min_ms=1e3 * xs[0], max_ms=1e3 * xs[-1])


def run_case(args, rwa: bool) -> dict:
    import torch

    from qml_essentials_amd import pulses
    from qml_essentials_amd.evolution import Evolution
    from qml_essentials_amd.gates import PulseInformation
    from qml_essentials_amd.model import Model

    Evolution.set_solver_defaults(solver="magnus4", magnus_steps=args.steps)
    model = Model(n_qubits=args.qubits, n_layers=args.layers, circuit_type="Circuit_19")
    PulseInformation.set_rwa(rwa)
    rng = np.random.default_rng(7)
    params = rng.uniform(0, 2 * np.pi, (args.batch,) + model.params.shape[1:])
    inputs = np.array([0.3])
    model(params=params, inputs=inputs, gate_mode="pulse")  # (also sets the model's batch shape for the recording)
    tape = record_tape(model, params, inputs)
    leaves = [o for o in tape if isinstance(o, pulses.PulseRotation)]
    solves = sum(o.rows for o in leaves)
    nodes = 2 * args.steps
    t_one, t_gate, t_call, worst = [], [], [], 0.0
    for rep in range(args.reps + 1):
        for o in leaves:
            o._matrix = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        launched = pulses.resolve(tape)
        t1 = time.perf_counter()
        generic = per_gate_route(leaves, args.steps)
        t2 = time.perf_counter()
        model(params=params, inputs=inputs, gate_mode="pulse")
        t3 = time.perf_counter()
        if rep:  # (round 0 warms up)
            t_one.append(t1 - t0), t_gate.append(t2 - t1), t_call.append(t3 - t2)
        worst = max(worst, max(np.abs(np.asarray(o.matrix) - g).max() for o, g in zip(leaves, generic)))
    return dict(case="rwa" if rwa else "exact (drive)", qubits=args.qubits, layers=args.layers, batch=args.batch,
                steps=args.steps, leaves=len(leaves), batched_leaves=sum(o.batched_request for o in leaves),
                solves_requested=solves, solves_launched=launched, launches_one=1, launches_per_gate=len(leaves),
                host_table_mb=sum(o.rows for o in leaves) * nodes * 2 * 8 / 1e6,
                one_launch=stats(t_one), per_gate=stats(t_gate), whole_call=stats(t_call),
                largest_difference=worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=4)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("pulse_bench.py needs a GPU")
    results = [run_case(args, rwa) for rwa in (True, False)]
    for r in results:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
