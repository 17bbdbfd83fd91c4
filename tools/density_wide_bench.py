"""Times ``qmle_density_apply_wide`` (csrc/qmle_density_wide.hip) on a resident vec(rho), in one process, candidate
and yardstick in alternating windows:

  leg 1  ``NQubitDepolarizingChannel`` on 3 and on 4 wires at n = 10 and 12: the new call (automatic form) against the
         route before it -- the ``_WideChannel.kraus_plans`` loop exactly as ``simulation._evolve_density`` ran it: per
         Kraus operator a clone of vec(rho), two padded MAT4 plans in place, and an add into an accumulator.
  leg 2  one unitary on 3 and on 4 wires: the sandwich call against two ``qmle_apply_matrix`` passes over the 2n-wire
         register (U on the ket wires, conj U on the bra wires) -- the same result without new HIP.
  leg 3  both forms forced at n_ops = d/4, d/2, d, 2d: where the measured times cross places the automatic rule.

Every line reports ms per call and the bytes of one read and one write of vec(rho) over that time against the HBM
peak.  vec(rho) is 8 MB at n = 10 and 134 MB at n = 12 in complex64: back-to-back calls on one buffer find it in the
256 MB Infinity Cache, so the rate is a cache rate and may exceed what HBM delivers; the ratios between the legs are
what the figures are for.  Method: two warm-up calls, then device events around `reps` back-to-back calls, reps
chosen so that a window is at least --min-seconds; 5 windows per function, taken in turn; the median is reported.

    python tools/density_wide_bench.py [--qubits 10 12] [--min-seconds 0.2] [--legs 1 2 3] [--out FILE]
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


def alternate(torch, fns, min_seconds, windows=5):
    """Median ms per call of every function, their windows taken in turn."""
    reps = [reps_for(torch, f, min_seconds) for f in fns]
    out = [[] for _ in fns]
    for _ in range(windows):
        for i, f in enumerate(fns):
            out[i].append(window(torch, f, reps[i]))
    return [float(np.median(o)) for o in out], reps


def wires_for(k, n):
    """A scattered set that holds wire n - 1 and wire 0 out of order (a bra target on position 0)."""
    return [n - 1, 0, n // 2] if k == 3 else [1, n - 2, 0, n - 1]


def rho_for(torch, n, f64=False):
    rho = torch.zeros((1, 4 ** n), dtype=torch.complex128 if f64 else torch.complex64, device="cuda")
    rho[0, :: 2 ** n + 1] = 1.0 / 2 ** n  # the maximally mixed state: every leg below leaves it finite
    return rho


def record(out, **kw):
    print(json.dumps(kw), flush=True)
    out.append(kw)


def rates(rho, ms):
    moved = 2 * rho.numel() * rho.element_size()
    return {"ms": ms, "GB_per_s": moved / ms / 1e6, "fraction_of_hbm_peak": moved / (ms * 1e-3) / HBM_PEAK}


def leg1(torch, N, simulation, n, min_seconds, out):
    import density_wide_reference as R

    for k in (3, 4):
        wires = wires_for(k, n)
        kraus = R.depolarizing_kraus(0.1, k)
        dev = torch.from_numpy(kraus).cuda()
        rho = rho_for(torch, n)
        chan = simulation._WideChannel(list(kraus), wires)
        pairs = list(chan.kraus_plans(n))

        def parent():  # simulation._evolve_density before this pass existed
            acc = torch.zeros_like(rho)
            for pair in pairs:
                acc += simulation._apply_segment(pair, 2 * n, 1, rho.clone())
            return acc

        (new_ms, old_ms), reps = alternate(torch, [lambda: N.density_apply_wide(rho, n, wires, dev), parent], min_seconds)
        record(out, leg=1, n=n, k=k, n_ops=len(kraus), wires=wires, form=R.auto_form(k, len(kraus)), **rates(rho, new_ms),
               parent_ms=old_ms, speedup=old_ms / new_ms, reps=reps)


def leg2(torch, N, n, min_seconds, out):
    import density_wide_reference as R

    for f64 in (False, True):
        for k in (3, 4):
            wires = wires_for(k, n)
            U = R.operators("unitary", k, 1, np.random.default_rng(k))[0]
            dU, dUc = torch.from_numpy(U).cuda(), torch.from_numpy(np.conj(U)).cuda()
            rho = rho_for(torch, n, f64)
            ket, bra = wires, [w + n for w in wires]

            def two_passes():
                N.apply_matrix(rho, ket, dU)
                N.apply_matrix(rho, bra, dUc)

            (new_ms, two_ms), reps = alternate(
                torch, [lambda: N.density_apply_wide(rho, n, wires, dU, form="sandwich"), two_passes], min_seconds)
            record(out, leg=2, n=n, k=k, dtype="complex128" if f64 else "complex64", wires=wires, **rates(rho, new_ms),
                   two_passes_ms=two_ms, speedup=two_ms / new_ms, reps=reps)


def leg3(torch, N, n, min_seconds, out):
    import density_wide_reference as R

    for k in (3, 4):
        d, wires = 2 ** k, wires_for(k, n)
        for n_ops in (d // 4, d // 2, d, 2 * d):
            rng = np.random.default_rng([k, n_ops])
            ops = torch.from_numpy(R._ginibre(rng, n_ops, d, d) / np.sqrt(2 * d * n_ops)).cuda()
            rho = rho_for(torch, n)
            (sw, su), reps = alternate(torch, [lambda: N.density_apply_wide(rho, n, wires, ops, form="sandwich"),
                                               lambda: N.density_apply_wide(rho, n, wires, ops, form="superoperator")],
                                       min_seconds)
            rho = rho_for(torch, n)  # (2d non-trace-preserving operators shrink rho over the repetitions: start again)
            record(out, leg=3, n=n, k=k, n_ops=n_ops, sandwich_ms=sw, superoperator_ms=su,
                   sandwich_fraction_of_hbm_peak=rates(rho, sw)["fraction_of_hbm_peak"],
                   superoperator_fraction_of_hbm_peak=rates(rho, su)["fraction_of_hbm_peak"],
                   faster="sandwich" if sw <= su else "superoperator", automatic=R.auto_form(k, n_ops), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, nargs="+", default=[10, 12])
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--legs", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from qml_essentials_amd import _native as N
    from qml_essentials_amd import simulation

    if not torch.cuda.is_available():
        raise SystemExit("density_wide_bench needs a GPU: no timing is taken without one")
    out = []
    for n in args.qubits:
        if 1 in args.legs:
            leg1(torch, N, simulation, n, args.min_seconds, out)
        if 2 in args.legs:
            leg2(torch, N, n, args.min_seconds, out)
        if 3 in args.legs:
            leg3(torch, N, n, args.min_seconds, out)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
