"""Times the pieces of adjoint gradients through evolved gates on the GPU:

  * ``qmle_evolve_magnus_jac`` against ``qmle_evolve_magnus`` on the shapes of profiles/evolution.md -- 102400 rows x
    256 steps of order 4, dim 2 (3 terms) and dim 4 (4 terms), one direction and four -- with the library's choice of
    lanes; the table derivatives are random numbers of the table's own size (their values do not steer the kernel:
    the series length follows the exponent alone);
  * one gradient of a six-qubit circuit with twelve one-wire evolved gates (static and parametrised, 36 leaf elements)
    by ``Script.vjp(through_evolve=True)`` against central differences through ``Script.execute`` (two forward calls
    per leaf element), and the largest distance between the two;
  * the two-wire streaming moment (``k_adj_moment2<float2>`` and its finishing kernel) at n = 20: a tape with eight
    constant 4x4 gates on different wire pairs, batch 8, swept on the streaming route with all eight flagged and with
    none; the difference over eight is one moment, which reads psi and lambda once (2 x 8 B x 2^20 per sample).

Method: the kernel figures as tools/evolve_bench.py (device events around back-to-back launches, the median of 5
windows of at least 0.3 s); the gradient figures are host clocks around whole calls after one warm-up call, median of
five.  One JSON line per case.

    python tools/evolve_gradient_bench.py [--rows 102400] [--steps 256] [--cases circuit,moment,kernel]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def kernel_cases(torch, N, rows, steps):
    from evolve_bench import device_problem, time_launches

    for dim in (2, 4):
        H, coef, h = device_problem(torch, dim, rows, steps, 4)
        fwd = time_launches(torch, lambda: N.evolve_magnus(H, coef, h, 4))
        for n_dirs in (1, 4):
            g = torch.Generator(device=coef.device).manual_seed(n_dirs)
            dcoef = torch.randn((rows, n_dirs) + tuple(coef.shape[1:]), generator=g, device=coef.device,
                                dtype=torch.float64)
            dh = torch.randn((rows, n_dirs), generator=g, device=coef.device, dtype=torch.float64) / steps
            jac = time_launches(torch, lambda: N.evolve_magnus_jac(H, coef, h, dcoef, dh, 4))
            lanes = N.lib().qmle_evolve_lanes(rows * n_dirs, steps)
            print(json.dumps({"case": "kernel", "dim": dim, "rows": rows, "n_steps": steps, "order": 4, "n_dirs": n_dirs,
                              "lanes_per_row": min(lanes, 16) if dim == 4 else lanes,
                              "forward_ms_median": fwd[0], "jac_ms_median": jac[0], "jac_ms_min": jac[1],
                              "jac_ms_max": jac[2], "jac_over_forward": jac[0] / fwd[0],
                              "jac_over_forward_per_direction": jac[0] / fwd[0] / n_dirs,
                              "dcoef_gib": dcoef.numel() * 8 / 2 ** 30,
                              "tables_gib_per_s": (coef.numel() * n_dirs + dcoef.numel()) * 8 / 2 ** 30 / (jac[0] * 1e-3)}),
                  flush=True)
            del dcoef


def circuit_case():
    import evolution_reference as ER
    from qml_essentials_amd import operations as op
    from qml_essentials_amd import utils
    from qml_essentials_amd.script import Script

    n = 6
    herm = lambda m, w: op.Hermitian(matrix=m, wires=w, record=False)  # noqa: E731
    mats = [0.8 * ER.X + 0.5 * ER.Z, 0.6 * ER.Y - 0.7 * ER.Z, ER.X + 0.3 * ER.Y]

    def circuit(t, p, th):
        for q in range(n):
            op.H(wires=q)
        for q in range(n):  # six static gates, one time each
            herm(mats[q % 3], q).evolve()(t=t[q], wires=q)
        for q in range(n):
            op.CRZ(th[q], wires=[q, (q + 1) % n])
        for q in range(n):  # six driven gates: p0 cos(p1 t) Z + p2 X on [0, T]
            ph = (lambda a, s: a[0] * np.cos(a[1] * s)) * herm(ER.Z, q) + (lambda a, s: a) * herm(ER.X, q)
            ph.evolve(solver="magnus4", magnus_steps=64)([p[q, :2], p[q, 2]], p[q, 3])

    rng = np.random.default_rng(1)
    t, p, th = rng.uniform(0.2, 1.5, n), rng.uniform(0.5, 1.5, (n, 4)), rng.uniform(0.3, 2.5, n)
    obs = [op.PauliZ(wires=q, record=False) for q in range(n)] + [op.PauliX(wires=0, record=False)]
    w = rng.uniform(0.5, 1.5, len(obs))
    script = Script(f=circuit, n_qubits=n)
    out = {"case": "circuit", "n_qubits": n, "evolved_gates": 2 * n, "leaf_elements": int(t.size + p.size + th.size)}
    with utils.x64_scope(True):
        def adjoint():
            return script.vjp(obs, w, args=(t, p, th), argnums=(0, 1, 2), pauli_seed=True, through_evolve=True)

        def cost(a, b, c):
            return float(np.dot(w, np.asarray(script.execute(type="expval", obs=obs, args=(a, b, c)), dtype=np.float64)))

        def differences(eps=1e-5):
            grads = []
            for k, x in enumerate((t, p, th)):
                g = np.zeros(x.size)
                for e in range(x.size):
                    d = np.zeros(x.size)
                    d[e] = eps
                    args_p = [t, p, th]
                    args_m = [t, p, th]
                    args_p[k], args_m[k] = x + d.reshape(x.shape), x - d.reshape(x.shape)
                    g[e] = (cost(*args_p) - cost(*args_m)) / (2 * eps)
                grads.append(g.reshape(x.shape))
            return grads

        def clock(fn, reps):
            fn()
            times = []
            for _ in range(reps):
                a = time.perf_counter()
                res = fn()
                times.append(time.perf_counter() - a)
            return res, float(np.median(times)) * 1e3

        got, out["vjp_ms_median"] = clock(adjoint, 5)
        want, out["central_differences_ms_median"] = clock(differences, 3)
    out["speedup"] = out["central_differences_ms_median"] / out["vjp_ms_median"]
    out["max_distance"] = float(max(np.abs(np.asarray(g) - v).max() for g, v in zip(got, want)))
    out["largest_gradient"] = float(max(np.abs(v).max() for v in want))
    print(json.dumps(out), flush=True)


def moment_case(torch, n=20, batch=8):
    import adjoint_reference as R
    from qml_essentials_amd import adjoint
    from qml_essentials_amd import operations as op
    from qml_essentials_amd.script import Script

    rng = np.random.default_rng(2)
    pairs = [(0, 1), (19, 0), (7, 12), (12, 7), (18, 19), (3, 16), (10, 9), (5, 14)]
    mats = [R.unitary(rng, 2) for _ in pairs]

    def circuit(th):
        for q in range(n):
            op.RX(th[q], wires=q)
        for (a, b), m in zip(pairs, mats):
            op.Operation(wires=[a, b], matrix=m)

    th = rng.uniform(0.3, 2.5, (batch, n))
    _t, low, _n, B, _s, _shapes, _b = Script(f=circuit, n_qubits=n)._trace_for_gradient([], (th,), None, (0,), (0,))
    flagged = [name == "MAT2" for name, _w, _sl, _o in low.ops]
    assert sum(flagged) == len(pairs)
    w = rng.uniform(0.5, 1.5, (B, n))
    groups = [[q] for q in range(n)]
    fused, adjoint.REV_FLAGS_FUSED = adjoint.REV_FLAGS_FUSED, adjoint.REV_FLAGS  # one streaming pass per gate
    try:
        def sweep(flags):
            out = adjoint.adjoint_slot_and_matrices_gradient(low, n, B, groups, w, [True] * low.n_slots, flags)
            torch.cuda.synchronize()
            return out

        def clock(flags):
            sweep(flags)
            times = []
            for _ in range(5):
                a = time.perf_counter()
                sweep(flags)
                times.append(time.perf_counter() - a)
            return float(np.median(times)) * 1e3

        with_ms, without_ms = clock(flagged), clock([False] * len(flagged))
    finally:
        adjoint.REV_FLAGS_FUSED = fused
    per = (with_ms - without_ms) / len(pairs)
    nbytes = 2 * 8 * (1 << n) * B
    print(json.dumps({"case": "moment2", "n_qubits": n, "batch": B, "two_wire_gates": len(pairs),
                      "sweep_ms_with_cotangents": with_ms, "sweep_ms_without": without_ms,
                      "ms_per_moment_and_finish": per, "bytes_per_moment": nbytes,
                      "gb_per_s": nbytes / 1e9 / (per * 1e-3) if per > 0 else None}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=102400)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--cases", default="circuit,moment,kernel", help="comma-separated: circuit, moment, kernel")
    args = ap.parse_args()
    cases = set(args.cases.split(","))
    if not cases <= {"circuit", "moment", "kernel"}:
        raise SystemExit(f"unknown case in {args.cases!r}")
    import torch

    from qml_essentials_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("evolve_gradient_bench needs a GPU: no timing is taken without one")
    if "circuit" in cases:
        circuit_case()
    if "moment" in cases:
        moment_case(torch)
    if "kernel" in cases:
        kernel_cases(torch, N, args.rows, args.steps)


if __name__ == "__main__":
    main()
