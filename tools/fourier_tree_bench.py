"""Analytic Fourier coefficients (``coefficients.FourierTree``): table build time, ``get_spectrum`` on the device for
B in {1, 256, 4096} parameter sets, the host interpreter on the same batch, and the numeric route that was there
before -- ``Coefficients.get_spectrum`` (FFT of the model sampled on its grid) over the same parameter sets on the
same card.  Prints one markdown table row per model and batch (``profiles/fourier_tree.md`` keeps a run).

    python tools/fourier_tree_bench.py [--batches 1,256,4096] [--max-items 2e10] [--host-max-items 3e8] [--only 5,6]

Times are wall clock around the whole call (recording, table upload, kernel, copy back): the tree's best of
``--repeat`` after one warm-up call, the FFT route's single call on a fresh parameter draw after a warm-up on another.  A (model, batch) whose walk exceeds ``--max-items`` (nodes x grid points x B) is skipped, the host
interpreter beyond ``--host-max-items``.
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qml_essentials_amd import coefficients as CO  # noqa: E402
from qml_essentials_amd.coefficients import Coefficients, FourierTree  # noqa: E402
from qml_essentials_amd.model import Model  # noqa: E402

MODELS = [("Circuit_19", 3, 2), ("Circuit_19", 4, 2), ("Hardware_Efficient", 4, 2), ("Strongly_Entangling", 4, 4),
          ("Hardware_Efficient", 6, 3), ("Strongly_Entangling", 6, 4), ("Hardware_Efficient", 8, 3)]


def best_of(fn, repeat):
    fn()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return min(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,256,4096")
    ap.add_argument("--max-items", type=float, default=2e10)
    ap.add_argument("--host-max-items", type=float, default=3e8)
    ap.add_argument("--workspace-gib", type=float, default=16.0)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated indices into the model list (default: all seven)")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    budget = int(args.workspace_gib * (1 << 30))
    print("| model | rotations | nodes | grid | build s | B | device s | launches | host s | FFT route s | "
          "max abs(device - host) | max abs(device - FFT) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
    chosen = [MODELS[int(i)] for i in args.only.split(",")] if args.only else MODELS
    for ansatz, n, layers in chosen:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = Model(n_qubits=n, n_layers=layers, circuit_type=ansatz, output_qubit=0)
        t0 = time.perf_counter()
        tree = FourierTree(model, evaluate="device", workspace_bytes=budget)
        dag = tree._ensure_dag()
        build = time.perf_counter() - t0
        F = int(np.prod(dag.dims)) if dag.dims else 1
        for B in batches:
            # the FFT route first: warmed up on one draw, timed once on the next (a repeated call with the same
            # parameters would be answered from the model's call cache)
            model.initialize_params(repeat=B)
            Coefficients.get_spectrum(model, shift=True)
            model.initialize_params(repeat=B)
            t0 = time.perf_counter()
            fc, ff = Coefficients.get_spectrum(model, shift=True)
            t_fft = time.perf_counter() - t0
            params = np.array(model.params, dtype=np.float64).reshape(B, *model.params.shape[-2:])
            items = dag.n_nodes * F * B
            row = f"| {ansatz} {n}q/{layers}l | {tree.n_params} | {dag.n_nodes} | {F} | {build:.2f} | {B} |"
            if items > args.max_items:
                print(row + " skipped | | | | | |", flush=True)
                continue
            before = CO.TREE_LAUNCHES
            t_dev, (dev, freqs) = best_of(lambda: tree.get_spectrum(params=params), args.repeat)
            launches = (CO.TREE_LAUNCHES - before) // (args.repeat + 1)
            if items <= args.host_max_items:
                t_host, (host, _) = best_of(lambda: tree.get_spectrum(params=params, evaluate="host"), 1)
                d_host = f"{np.max(np.abs(dev[0] - host[0])):.1e}"
                t_host = f"{t_host:.3f}"
            else:
                t_host, d_host = "-", "-"
            fc = np.asarray(fc).reshape(len(np.asarray(ff)), -1)  # [n_freq, B]
            # the FFT's axis holds the encoding's naive frequencies; compare where the tree's support lies on it
            ffa = np.rint(np.asarray(ff, dtype=np.float64)).astype(np.int64)
            both = [(int(np.flatnonzero(ffa == w)[0]), j) for j, w in enumerate(np.asarray(freqs[0])) if np.any(ffa == w)]
            d_fft = max((np.max(np.abs(fc[i] - dev[0].reshape(B, -1)[:, j])) for i, j in both), default=float("nan"))
            print(row + f" {t_dev:.3f} | {launches} | {t_host} | {t_fft:.4f} | {d_host} | {d_fft:.1e} |", flush=True)


if __name__ == "__main__":
    main()
