"""Times what adjoint gradients through explicit matrices on three and four wires add:

  * the moment pass ``qmle_wide_moment`` (csrc/qmle_wide.hip) at n = 24 .. 28, batch 1, k = 3 and 4, complex64 and
    complex128, on three wire sets -- the top positions, a scattered set and positions 0 .. k - 1 -- as bytes moved
    (one read of psi and one of lambda) over time, beside ``qmle_apply_matrix`` on the same wires in the same session,
    which moves the same bytes (a read and a write of one state);
  * one end-to-end gradient of a circuit with two wide gates by ``Script.vjp(wide_gates=True, through_evolve=True)``
    against central differences through ``Script.execute``, the only route before, and their distance.

Method (profiles/wide_gradient.md): as tools/wide_gate_bench.py -- two warm-up launches, device events around `reps`
back-to-back launches, candidate and yardstick in alternating windows, the median of 5.

    python tools/wide_gradient_bench.py [--qubits 24 25 26 27 28] [--circuit-qubits 12] [--cases moment,circuit]
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

from wide_gate_bench import HBM_PEAK, alternate, wire_sets  # noqa: E402


def moment_leg(torch, N, n, f64, min_seconds):
    import wide_gate_reference as W

    dtype = torch.complex128 if f64 else torch.complex64
    g = torch.Generator(device="cuda").manual_seed(n)
    pair = torch.randn((2, 1 << n, 2), generator=g, device="cuda", dtype=torch.float64 if f64 else torch.float32)
    pair = torch.view_as_complex(pair)
    pair /= torch.linalg.vector_norm(pair, dim=1, keepdim=True)
    psi, lam = pair[:1], pair[1:]
    moved = 2 * psi.numel() * psi.element_size()
    rng = np.random.default_rng(n)
    for k in (3, 4):
        U = torch.from_numpy(W.random_unitaries(rng, 1 << k)).cuda()
        sets = wire_sets(k, n)
        for name in ("top", "scattered", "bottom"):
            wires = sets[name]
            (ms, apply_ms), reps = alternate(torch, [lambda: N.wide_moment(psi, lam, wires, U),
                                                     lambda: N.apply_matrix(psi, wires, U)], min_seconds=min_seconds)
            print(json.dumps({"case": "moment", "n": n, "k": k, "dtype": "complex128" if f64 else "complex64",
                              "wires": name, "positions": sorted(n - 1 - w for w in wires), "ms": ms,
                              "GB_per_s": moved / ms / 1e6, "fraction_of_hbm_peak": moved / (ms * 1e-3) / HBM_PEAK,
                              "apply_ms": apply_ms, "apply_GB_per_s": moved / apply_ms / 1e6,
                              "ratio_to_apply": ms / apply_ms, "reps": reps}), flush=True)
    del pair


def circuit_leg(n, B):
    """RX / CRZ layers around a four-wire and a three-wire static evolution, every angle and both times leaves."""
    import wide_adjoint_reference as A
    from qml_essentials_amd import jaqsi as js
    from qml_essentials_amd import operations as op
    from qml_essentials_amd.script import Script

    case = A.make_case("two", n, B)

    def f(theta, t):
        for st in case.steps:
            if st.kind == "WIDE":
                op.Hermitian(st.H, list(range(len(st.wires))), record=False).evolve()(t[st.angle], wires=list(st.wires))
            elif st.kind in ("CX", "H"):
                getattr(op, st.kind)(wires=list(st.wires))
            else:
                getattr(op, st.kind)(theta[st.angle], wires=list(st.wires))

    obs = [op.PauliZ(wires=0, record=False), js.build_parity_observable([1, n - 1]), op.PauliZ(wires=2, record=False)]
    s = Script(f=f, n_qubits=n)
    kw = dict(args=(case.theta, case.t), in_axes=(0, 0))

    def sweep():
        return s.vjp(obs, case.weights, argnums=(0, 1), through_evolve=True, wide_gates=True, **kw)

    def cost(theta, t):
        e = np.asarray(s.execute(type="expval", obs=obs, args=(theta, t), in_axes=(0, 0)), dtype=np.float64)
        return (e * case.weights).sum(axis=1)

    def differences(h=1e-2):  # (complex64 forward runs: the step that balances truncation against rounding)
        out = []
        for arr, key in ((case.theta, 0), (case.t, 1)):
            g = np.zeros_like(arr)
            for j in range(arr.shape[1]):
                up, dn = arr.copy(), arr.copy()
                up[:, j] += h
                dn[:, j] -= h
                a = (up, case.t) if key == 0 else (case.theta, up)
                b = (dn, case.t) if key == 0 else (case.theta, dn)
                g[:, j] = (cost(*a) - cost(*b)) / (2 * h)
            out.append(g)
        return out

    sweep()
    t0 = time.perf_counter()
    got = sweep()
    t_sweep = time.perf_counter() - t0
    differences()
    t0 = time.perf_counter()
    fd = differences()
    t_fd = time.perf_counter() - t0
    ref = A.gradients(case)
    scale = np.maximum(1.0, np.abs(case.weights).sum(axis=1))[:, None]
    print(json.dumps({"case": "circuit", "n": n, "batch": B, "steps": len(case.steps), "wide_gates": 2,
                      "leaf_elements": int(case.theta.shape[1] + case.t.shape[1]),
                      "vjp_seconds": t_sweep, "central_differences_seconds": t_fd, "speedup": t_fd / t_sweep,
                      "vjp_vs_reference": float(max((np.abs(a - b) / scale).max() for a, b in zip(got, ref[:2]))),
                      "differences_vs_reference": float(max((np.abs(a - b) / scale).max() for a, b in zip(fd, ref[:2])))}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, nargs="+", default=[24, 25, 26, 27, 28])
    ap.add_argument("--circuit-qubits", type=int, default=12)
    ap.add_argument("--circuit-batch", type=int, default=4)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--cases", default="moment,circuit")
    args = ap.parse_args()
    import torch

    from qml_essentials_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("wide_gradient_bench needs a GPU: no timing is taken without one")
    cases = args.cases.split(",")
    if "circuit" in cases:
        circuit_leg(args.circuit_qubits, args.circuit_batch)
    if "moment" in cases:
        for n in args.qubits:
            for f64 in (False, True):
                moment_leg(torch, N, n, f64, args.min_seconds)


if __name__ == "__main__":
    main()
