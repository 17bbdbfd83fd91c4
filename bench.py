#!/usr/bin/env python3
"""Headline benchmark (BASELINE.json): gate-applies/s and statevectors/s of the
data-reuploading Model hot path at n_qubits=24, batch=1024 per GPU.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A *step* = one call of ``Model(24, 1, "Hardware_Efficient", data_reupload=False)`` on a
batch of 1024 parameter sets per GPU through the drop-in API (``Model.__call__`` ->
``Script.execute`` -> ``libqmle_sv``): 96 reference gates per statevector (72 one-qubit +
24 CX, SURVEY.md 8-d "K2"), PauliZ expectation on all 24 wires.

**What the headline measures (round 2).**  The timed plan is compiled with
``QMLE_PLAN_NO_SPARSE | QMLE_PLAN_NO_ABSORB``: no known-zero tracking and no folding of the
trailing CX layer into the observables -- every one of the 96 counted gates is applied to a
statevector whose 2^24 amplitudes are all read, computed and stored in every HBM pass that
follows the |0..0> initialisation (gate *fusion* stays on: three HBM passes instead of 96).
``value``, ``ms_per_step`` and ``roofline`` come from that run.  With ``--full``, the default engine
(known-zero tracking + observable folding, exact but specific to what a shallow circuit leaves
untouched) is reported under ``exact_shortcuts``; a deeper circuit (``k2_deep``: 24 qubits, 4 layers,
data re-uploading) with both flag sets beside it.

Parameters are synthetic U[0, 2 pi) float32 from ``numpy.random.default_rng(1000)`` and are
resident in HBM (a CUDA tensor) before the timed region; the per-sample angle table is built on
the GPU (``qmle_build_angles``), the statevectors are produced and consumed on the GPU and the
result is a CUDA tensor -- no host<->device traffic inside a step.  Weak scaling: every rank
simulates its own 1024 states and one RCCL all-gather returns the (1024 N, 24) expectation values.

**Ranks.**  ``python bench.py --gpus N`` with N > 1 and no ``WORLD_SIZE`` in the environment is a
*launcher*: the parent never touches the GPU, starts ``python -m torch.distributed.run --nnodes=1
--nproc-per-node N --master-addr 127.0.0.1 ...`` on this same file as a CHILD process (never an
exec), relays rank 0's JSON line and exits with the child's code.  Inside, ``world_size`` must equal
``--gpus`` and the backend must be ``nccl`` (= RCCL; ``QMLE_DIST_BACKEND=gloo`` only for rehearsals
with several ranks on one GPU) or the run exits non-zero.  With ``--full``, besides the weak-scaling K2
step the line carries the strong-scaling legs BASELINE names: C3 (1024 Expressibility pairs split over
the ranks) and C4 (the 4096-point Fourier grid, 512 points per GPU at N = 8).

A plain run does only what the headline needs: set-up, ``--warmup`` untimed steps, ``--steps`` timed
steps, the line.  ``--dump-outputs DIR`` writes what the last timed step returned -- the (1024 N, 24)
<Z> rows -- as ``DIR/expval.npy`` (float32; a fixed, seeded sample of rows above 64 MB), so that two
builds can be compared output for output on the same seeded inputs.

``--full`` adds the legs that take runs of their own (N = 1; each with its own roofline object, parity
check and CPU timing where a CPU form exists): `c2_model_20q_4l` (BASELINE config 2: rates against HBM
and L2), `c3_…` / `c4_…` (configs 3 / 4, sharded over the ranks) with `c3_/c4_saturated_weak`
companions and `collective_ms`, `mw_28q` (config 5), `k1_single_gate_28q` (RX RZ CX CRX CRZ CZ CPhase on
every wire), `k2_unfused`, `k2_autotuned`, `k2_one_stream`, `k2_three_pass`, `k2_circuit19`, `k2_deep`
(per-pass bound), `exact_shortcuts`, `lds_regime`, `adjoint_gradient_20q`, `widened_rows` and
``cpu_baseline`` (the oracle's C/OpenMP port on a bounded sample; its <Z> values are compared with the
GPU's rows for the same parameter sets and a mismatch fails the run).

Rank 0 prints ONE JSON line: ``metric``, ``value``, ``unit``, ``higher_is_better``, ``dtype``,
``ms_per_step`` and ``roofline`` (dominant kernel, timed live with HIP events on the launch stream
during the timed steps), the legs above under ``--full``, and ``summary``, the LAST key: one figure
per leg in ~3 KB.
"""
from __future__ import annotations

import argparse
import contextlib
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec, /opt/skills/guides/MI355X_MICROARCH.md:36
VALU_PEAK_TFLOPS = 157.3  # MI355X fp32 vector peak, same guide
VALU_ISSUE_PER_NOMINAL = 1.6  # vector-issue share of a pass's cycles per unit of nominal flops / peak (SQ counters, round 5)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-qubits", type=int, default=24)
    ap.add_argument("--batch", type=int, default=1024, help="statevectors per GPU per step")
    ap.add_argument("--no-fusion", action="store_true", help="one HBM pass per reference gate")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, run every companion leg (C2-C5 configs, K1, deep / unfused / autotuned "
                         "/ one-stream K2, LDS regime, CPU baselines and parity checks); off: headline only")
    ap.add_argument("--skip-aux", action="store_true", help="with --full: headline only (no K1 / deep / CPU legs)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path returned in its last step as DIR/<name>.npy")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="with --full: CPU baseline budget")
    ap.add_argument("--rendezvous-only", action="store_true",
                    help="start the ranks, run the one collective on a token tensor, print the line's "
                         "rank bookkeeping and stop (launcher / process-group plumbing; needs no GPU)")
    return ap.parse_args(argv)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n_ranks, argv):
    """`--gpus N` without a launcher: start N ranks of this file under torch.distributed.run as a
    CHILD process (this parent has not initialised the GPU and never does; nothing is exec'd),
    relay rank 0's JSON line to stdout and return the child's exit code."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["QMLE_BENCH_LAUNCHED_BY"] = "bench.py"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_ranks}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.abspath(__file__), *argv]
    print("[bench] launching:", " ".join(cmd), file=sys.stderr, flush=True)
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True)
    line = None
    for out in proc.stdout:  # ranks' diagnostics go to stderr; stdout carries the JSON line
        if out.lstrip().startswith("{"):
            line = out.strip()
        else:
            sys.stderr.write(out)
    rc = proc.wait()
    if rc == 0 and line is None:
        print("[bench] the ranks exited without printing a result line", file=sys.stderr)
        rc = 3
    if line is not None:
        print(line, flush=True)
    return rc


@contextlib.contextmanager
def plan_flags(flags):
    from qml_essentials_amd import simulation

    saved = simulation.PLAN_FLAGS
    simulation.PLAN_FLAGS = flags
    try:
        yield
    finally:
        simulation.PLAN_FLAGS = saved


def kernel_of_stage(st, i, n_stages, n, dense):
    """Which kernel a stage launch runs (mirrors launch_tile in qmle_tile.hip / run_batch_masks in qmle_engine.hip)."""
    if st["kind"] != "tile":
        return {"direct": "k_direct_1q", "diag_all": "k_diag_all"}[st["kind"]]
    if i == n_stages - 1:  # <Z> out of the last pass: a single-group pass measures in registers
        k = st["expval_kernel"].replace("_fold", "")
        if k != "k_tile":
            return k
    if dense:
        return "k_tile2" if st.get("fast") else "k_tile"
    if st.get("product") and 0 < i < n_stages - 1:
        live = bin(~st["zero_in"] & ((1 << n) - 1)).count("1")
        return "k_product_stream" if live >= 9 and not st["zero_in"] & 1 else "k_tile_product"
    return "k_tile2" if st.get("fast") else "k_tile"  # (the fast tile path takes known-zero stages too: launch_tile)


def max_over_ranks(value):
    """Every rank's `value` (one float), as a list indexed by rank -- one all-gather."""
    from qml_essentials_amd import distributed

    rank, size = distributed.world()
    if size == 1:
        return [float(value)]
    dev = "cuda" if torch.distributed.get_backend() == "nccl" else "cpu"
    mine = torch.tensor([value], dtype=torch.float64, device=dev)
    every = torch.empty(size, dtype=torch.float64, device=dev)
    torch.distributed.all_gather_into_tensor(every, mine)
    return [float(v) for v in every.cpu()]


def timed_k2(n, B, size, steps, warmup, flags, layers=1, dru=False, x=None, profile=True,
             circuit="Hardware_Efficient", isolate_passes=False):
    """`steps` timed calls of Model(n, layers, circuit) on B parameter sets per rank under plan flags
    `flags`; returns timing, the plan description and the per-stage HIP-event times (rank 0)."""
    from qml_essentials_amd import _native as N
    from qml_essentials_amd import distributed, simulation
    from qml_essentials_amd.model import Model

    rank = distributed.world()[0]
    with plan_flags(flags):
        model = Model(n, layers, circuit, data_reupload=dru)
        rng = np.random.default_rng(1000)
        params = rng.uniform(0, 2 * np.pi, (B * size, *model.params.shape[1:])).astype(np.float32)
        inputs = None if x is None else np.full((1, 1), x, dtype=np.float32)
        # (two rows: the batched tape, whatever B -- the device path compiles the same affine plan for B = 1)
        tape, _ = model.record_tape(params=params[:2] if len(params) > 1 else np.repeat(params, 2, 0), inputs=inputs)
        low = simulation.LoweredTape(tape, n)
        top = simulation.get_plan(low)
        folded = top.describe().get("absorbed_ops", 0)
        plan = top.executed("expval")
        desc = plan.describe()
        params_dev = torch.from_numpy(params).cuda()  # resident in HBM before the timed region
        x_dev = None if inputs is None else torch.from_numpy(inputs).cuda()

        def step():
            return model(params=params_dev) if x_dev is None else model(params=params_dev, inputs=x_dev)

        for _ in range(warmup):
            out = step()
        torch.cuda.synchronize()
        desc = top.executed("expval").describe()  # (the opt-in autotuner re-schedules a plan on its first run)
        distributed.barrier()
        n_stages = len(desc["stages"])
        if profile and rank == 0:
            plan.profile_begin(n_stages * max(8, B) * steps + 16)
        t0 = time.perf_counter()
        for _ in range(steps):
            out = step()
        torch.cuda.synchronize()
        distributed.barrier()
        elapsed = time.perf_counter() - t0
        stage_ms = stage_cnt = overflow = None
        if profile and rank == 0:
            stage_ms, stage_cnt, overflow = plan.profile_end()
        if isolate_passes and profile and size == 1:
            # Round 5: a batch of several chunks keeps two of them in flight, one stage apart, on two streams: the
            # wall-clock above is what a caller gets, but a launch's HIP-event duration then includes the share of
            # the card the other chunk's pass took.  The per-pass figures (bytes / flops against their peaks) are about
            # the kernels themselves: taken from the same steps with the chunks on one stream.
            os.environ["QMLE_NO_CHUNK_OVERLAP"] = "1"
            try:
                step(); torch.cuda.synchronize()
                plan.profile_begin(n_stages * max(8, B) * steps + 16)
                t1 = time.perf_counter()
                for _ in range(steps):
                    out = step()
                torch.cuda.synchronize()
                elapsed_one_stream = time.perf_counter() - t1
                stage_ms, stage_cnt, overflow = plan.profile_end()
            finally:
                os.environ.pop("QMLE_NO_CHUNK_OVERLAP", None)
        else:
            elapsed_one_stream = None
    per_rank = max_over_ranks(elapsed)
    elapsed = max(per_rank)
    assert tuple(out.reshape(-1, n).shape) == (B * size, n) and bool(torch.isfinite(out).all())
    return {"elapsed": elapsed, "elapsed_per_rank": per_rank, "out": out, "desc": desc,
            "n_gates": len(low.ops), "folded": folded,
            "stage_ms": stage_ms, "stage_cnt": stage_cnt, "overflow": overflow, "params": params,
            "elapsed_one_stream": elapsed_one_stream,
            "flags": flags, "steps": steps, "B": B, "n": n}


def families(run, dense):
    """Per-kernel totals over the timed region: device ms (HIP events on the launch stream),
    launches, algorithmic bytes (SURVEY 8-d per gate x gates applied) and bytes really moved."""
    desc, n, B, steps = run["desc"], run["n"], run["B"], run["steps"]
    fam = {}
    ns = len(desc["stages"])
    for i, st in enumerate(desc["stages"]):
        k = kernel_of_stage(st, i, ns, n, dense)
        f = fam.setdefault(k, {"ms": 0.0, "launches": 0, "algo": 0.0, "moved": 0.0, "gates": 0})
        f["ms"] += run["stage_ms"][i]
        f["launches"] += run["stage_cnt"][i]
        states = B * steps
        f["algo"] += st["algo_bytes_per_state"] * states
        moved = st["read_bytes_from_zero"] + st["write_bytes_from_zero"]
        if i == ns - 1 and st["kind"] == "tile":
            moved = st["read_bytes_from_zero"]  # <Z> straight out of the last pass: nothing stored
        f["moved"] += moved * states
        f["gates"] += len(st["src_ops"])
    return fam


def per_pass(run, dense):
    """HIP-event time and bytes of every pass, one entry per stage: what the rocprofv3 kernel
    rows of profiles/ are to be compared with (the all-live initialising pass is two kernels)."""
    desc, n, B, steps = run["desc"], run["n"], run["B"], run["steps"]
    ns = len(desc["stages"])
    out = []
    for i, st in enumerate(desc["stages"]):
        k = kernel_of_stage(st, i, ns, n, dense)
        kernels = [k]
        if dense and i == 0 and st["kind"] == "tile" and k in ("k_tile2", "k_tile"):
            kernels = ["k_fill_zero", f"{k} (one workgroup per state: tile 0, 2^{st['T']} amplitudes)"]
        moved = st["read_bytes_from_zero"] + st["write_bytes_from_zero"]
        if i == ns - 1 and st["kind"] == "tile":
            moved = st["read_bytes_from_zero"]
        cnt = max(1, run["stage_cnt"][i])
        ms = run["stage_ms"][i] / cnt
        per_launch = moved * B * steps / cnt
        out.append({"pass": i + 1, "kernels": kernels, "launches": run["stage_cnt"][i],
                    "avg_launch_ms": round(ms, 5), "bytes_moved_per_launch": round(per_launch),
                    "moved_GBps": round(per_launch / ms / 1e6, 1) if ms > 0 else None})
    return out


def source_sha16():
    """Hash of the sources that decide what a kernel launch moves: profiles/traffic.json records the
    one its PMC counters were collected for, and a mismatch makes `traffic` null (never stale)."""
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "qml-essentials_amd", "csrc")
    for name in sorted(os.listdir(csrc)):  # every translation unit and header of libqmle_sv
        if name.endswith((".hip", ".cpp", ".h")):
            with open(os.path.join(csrc, name), "rb") as f:
                h.update(name.encode() + f.read())
    return h.hexdigest()[:16]


def load_traffic(key, path=None, sha=None):
    """(bytes per launch, source, states per launch, error) for `key` of profiles/traffic.json;
    bytes is None -- with the reason in `error` -- when the file is missing, has no such key, or
    was collected for other kernel sources than the ones in this tree."""
    path = path or os.path.join(ROOT, "profiles", "traffic.json")
    if not os.path.exists(path):
        return None, None, None, "profiles/traffic.json missing"
    try:
        doc = json.load(open(path))
    except Exception as e:  # pragma: no cover
        return None, None, None, f"profiles/traffic.json unreadable: {e}"
    rec = doc.get(key)
    if not rec:
        return None, None, None, f"no PMC record {key!r} in profiles/traffic.json"
    want = rec.get("source_sha16") or doc.get("_source_sha16")
    have = sha or source_sha16()
    if want != have:
        msg = (f"STALE: PMC record {key!r} was collected for kernel sources {want}, this tree is {have}; "
               f"re-run tools/collect_profiles_r04.sh on a GPU box")
        print("bench.py: " + msg, file=sys.stderr)
        return None, None, None, msg
    return rec["hbm_bytes_per_launch"], rec.get("source"), rec.get("states_per_launch"), None


def roofline_of(run, dense, traffic_key=None, prefer=None):
    """`roofline` object of a K2-style run.  achieved / frac are BYTES REALLY MOVED by the dominant
    kernel's launches (the plan compiler's per-pass read + write bytes, which the PMC counters in
    profiles/ confirm) / its HIP-event launch time / the 8 TB/s peak -- a fraction <= 1.  The
    SURVEY 8-d per-reference-gate bytes over the same time are `algorithmic_GBps`; their ratio to
    the bytes moved is the fusion factor (reference gates applied per HBM round trip)."""
    fam = families(run, dense)
    name = max(fam, key=lambda k: fam[k]["ms"])
    if prefer in fam and fam[prefer]["ms"] >= 0.8 * fam[name]["ms"]:
        # (chunks in flight on two streams: the initialising pass's launches stretch while they share the card with the
        # other chunk's measuring pass, and which family's summed HIP-event time is larger flips from run to run; the
        # kernel the PMC record belongs to stays the one reported)
        name = prefer
    dom = fam[name]
    sec = dom["ms"] * 1e-3
    algo = dom["algo"] / sec / 1e9 if sec > 0 else 0.0
    moved = dom["moved"] / sec / 1e9 if sec > 0 else 0.0
    traffic = source = terr = None
    if traffic_key:
        traffic, source, per_rec, terr = load_traffic(traffic_key)
        if traffic is not None:
            # per launch like `achieved`: the counters were collected at `per_rec` states per launch
            per_launch = run["B"] * run["steps"] * sum(
                1 for i, st in enumerate(run["desc"]["stages"])
                if kernel_of_stage(st, i, len(run["desc"]["stages"]), run["n"], dense) == name
            ) / max(1, dom["launches"])
            if per_rec and abs(per_launch - per_rec) > 0.5:
                traffic = round(traffic * per_launch / per_rec)
                source = (source or "") + f" (scaled from {per_rec} to {per_launch:g} states per launch)"
    fam_note = None
    if dense and name == "k_tile2" and run["desc"]["stages"] and run["desc"]["stages"][0]["kind"] == "tile":
        k0 = kernel_of_stage(run["desc"]["stages"][0], 0, len(run["desc"]["stages"]), run["n"], dense)
        fam_note = ("the initialising pass is two launches on the same stream, k_fill_zero (the zeros of every "
                    f"tile but tile 0) + {k0} (tile 0 of every state); both are inside that pass's HIP events "
                    "and its bytes" + ("" if k0 == name else f" (listed under {k0} in all_kernels_ms)"))
    return {
        "bound": "hbm", "kernel": name, "kernel_family_note": fam_note,
        "achieved": round(moved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
        "frac": round(moved / HBM_PEAK_GBPS, 4), "traffic": traffic,
        "traffic_source": source, "traffic_error": terr,
        "avg_launch_ms": round(dom["ms"] / max(1, dom["launches"]), 5),
        "launches": dom["launches"],
        "passes_per_state": sum(1 for i, st in enumerate(run["desc"]["stages"])
                                if kernel_of_stage(st, i, len(run["desc"]["stages"]), run["n"], dense) == name),
        "bytes_moved_per_launch": round(dom["moved"] / max(1, dom["launches"])),
        "algorithmic_bytes_per_launch": round(dom["algo"] / max(1, dom["launches"])),
        "algorithmic_GBps": round(algo, 1),
        "fusion_factor": round(dom["algo"] / dom["moved"], 2) if dom["moved"] else None,
        "kernel_share_of_step": round(dom["ms"] / (run["elapsed"] * 1e3), 4),
        "all_kernels_ms": {k: round(v["ms"], 3) for k, v in fam.items()},
        "per_pass": per_pass(run, dense),
        "note": "achieved / frac = bytes the dominant kernel's launches really read + wrote (plan model, "
                "confirmed by the PMC `traffic`) / their HIP-event time / 8 TB/s.  algorithmic_GBps = SURVEY "
                "8-d bytes (16 D per 1-qubit gate, 8 D per CX) of the reference gates those launches applied "
                "/ the same time; fusion_factor = algorithmic / moved = reference gates' worth of bytes per "
                "HBM round trip (a fused pass applies ~8-30 gates).  The one-pass-per-reference-gate run "
                "(`k2_unfused`) has fusion_factor <= 1 by construction",
        "event_pool_overflow": run["overflow"],
    }


def summarize(run, dense, count_gates=None):
    gates = run["n_gates"] if count_gates is None else count_gates
    el, B, steps = run["elapsed"], run["B"], run["steps"]
    size = run["out"].shape[0] // B
    desc = run["desc"]
    moved = 0.0
    for i, st in enumerate(desc["stages"]):
        m = st["read_bytes_from_zero"] + st["write_bytes_from_zero"]
        if i == len(desc["stages"]) - 1 and st["kind"] == "tile":
            m = st["read_bytes_from_zero"]
        moved += m
    extra = {}
    if run.get("elapsed_one_stream"):
        extra = {"ms_per_step_one_stream": round(run["elapsed_one_stream"] / steps * 1e3, 3),
                 "per_pass_note": "per-pass figures of this leg come from the same steps with the chunks on one stream "
                                  "(QMLE_NO_CHUNK_OVERLAP=1); ms_per_step is the default: two chunks in flight, one stage apart"}
    return {**extra, "ms_per_step": round(el / steps * 1e3, 3),
            "gate_applies_per_s": round(gates * B * size * steps / el, 1),
            "gates_counted_per_state": gates,
            "statevectors_per_s": round(B * size * steps / el, 2),
            "hbm_passes_per_state": len(desc["stages"]),
            "register_tile_groups_per_pass": [len(st.get("fast_groups") or st.get("groups") or [])
                                              for st in desc["stages"]],
            "hbm_bytes_moved_per_state": moved,
            "moved_GBps_per_gpu": round(moved * B * steps / el / 1e9, 1),
            "moved_GBps": round(moved * B * size * steps / el / 1e9, 1),
            "moved_frac_of_8TBps": round(moved * B * steps / el / 1e9 / HBM_PEAK_GBPS, 4)}


def k1_sweep(n=28, reps=24, warmup=8):
    """K1 of SURVEY.md 8-d: one gate per launch on a 2^n state, HIP-event timed, EVERY target
    wire 0..n-1 (control = target + 1 mod n for the controlled gates)."""
    from qml_essentials_amd import _native as N

    D = 1 << n
    st = torch.randn((1, D, 2), device="cuda", dtype=torch.float32)
    st = torch.view_as_complex(st / st.norm()).contiguous()
    ang = torch.full((1, 1), 1.234, device="cuda")
    out = {}
    # SURVEY 8-d bytes per amplitude: dense / diagonal 1-qubit 16, controlled 2x2 (CX, CRX, CRZ) 8 -- the
    # control = 1 half --, controlled phase (CZ, CPhase) 4 -- the |11> quarter (operations.py:1357-1487, 1171-1201)
    for gate, bytes_per_amp in (("RX", 16), ("RZ", 16), ("CX", 8), ("CRX", 8), ("CRZ", 8), ("CZ", 4), ("CPhase", 4)):
        per_wire = []
        for w in range(n):
            wires = [w] if gate in ("RX", "RZ") else [(w + 1) % n, w]
            slots = [0] if gate not in ("CX", "CZ") else []
            plan = N.Plan([(gate, wires, slots, -1)], n, 1, flags=N.PLAN_NO_FUSION)
            ws = torch.empty(plan.workspace_bytes(1, "state"), dtype=torch.uint8, device="cuda")
            for _ in range(warmup):  # (the chip's clock settles over the first milliseconds of a burst)
                N.apply_inplace(plan, ang, st, ws)
            plan.profile_begin(reps + 1)
            for _ in range(reps):
                N.apply_inplace(plan, ang, st, ws)
            ms, cnt, _ = plan.profile_end()
            per_wire.append(sum(ms) / max(1, sum(cnt)))
        gb = [bytes_per_amp * D / t / 1e6 for t in per_wire]
        # what a controlled gate CAN get away with moving: a control on bit positions 0..3 sits inside every
        # 128-byte line (16 amplitudes), so both control values share each line and all 16 D bytes must move
        # whatever the kernel does; higher controls select whole lines and 8 D suffices (SURVEY 8-d's figure)
        att = [bytes_per_amp] * n
        if gate in ("CX", "CRX", "CRZ"):
            att = [16 if (n - 1 - ((w + 1) % n)) <= 3 else 8 for w in range(n)]
        elif gate in ("CZ", "CPhase"):  # control AND target must select whole lines for the quarter to suffice
            att = [bytes_per_amp * (2 if (n - 1 - ((w + 1) % n)) <= 3 else 1) * (2 if (n - 1 - w) <= 3 else 1)
                   for w in range(n)]
        gba = [a * D / t / 1e6 for a, t in zip(att, per_wire)]
        out[gate] = {"bytes_per_amplitude": bytes_per_amp,
                     "attainable_bytes_per_amplitude_per_target_wire": att,
                     "frac_of_8TBps_vs_attainable_min_mean_max": [round(min(gba) / HBM_PEAK_GBPS, 3),
                                                                  round(float(np.mean(gba)) / HBM_PEAK_GBPS, 3),
                                                                  round(max(gba) / HBM_PEAK_GBPS, 3)],
                     "target_wires_at_0.70_or_more_of_attainable": int(sum(g / HBM_PEAK_GBPS >= 0.70 for g in gba)),
                     "ms_min_mean_max": [round(min(per_wire), 4), round(float(np.mean(per_wire)), 4),
                                         round(max(per_wire), 4)],
                     "frac_of_8TBps_min_mean_max": [round(min(gb) / HBM_PEAK_GBPS, 3),
                                                    round(float(np.mean(gb)) / HBM_PEAK_GBPS, 3),
                                                    round(max(gb) / HBM_PEAK_GBPS, 3)],
                     "slowest_target_wire": int(np.argmax(per_wire)),
                     "ms_per_target_wire": [round(t, 4) for t in per_wire]}
    del st
    torch.cuda.empty_cache()
    return out


def _wall(fn, reps):
    """Median wall-clock of `fn` over `reps` calls -- `fn` returns HOST values, so a call is complete
    when it returns; each call starts from a synchronised device and a barrier, and counts as the
    max over ranks (the job is done when the slowest rank is).  Then, in calls of their own (an
    event record costs the host ~5 us, which the wall-clock of a 0.2 ms call should not carry), the
    GPU's share: HIP events on the launch stream around the call (first launch enqueued -> last
    kernel done), median over the calls on this rank."""
    from qml_essentials_amd import distributed

    ts, gs = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        distributed.barrier()
        t0 = time.perf_counter()
        out = fn()
        ts.append(max(max_over_ranks(time.perf_counter() - t0)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        gs.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], out, sorted(gs)[len(gs) // 2]


def collective_ms(rows_per_rank, cols, reps=15):
    """The ONE collective of a sharded call by itself: `all_gather_rows` of (rows_per_rank x world, cols) float32
    results, each rank contributing its block -- median ms over `reps`, max over ranks (None for one rank: a
    single-rank call runs no collective).  Device tensors under nccl (RCCL), host tensors under a gloo rehearsal."""
    from qml_essentials_amd import distributed

    rank, size = distributed.world()
    if size == 1:
        return None
    dev = "cuda" if torch.distributed.get_backend() == "nccl" else "cpu"
    block = torch.full((rows_per_rank, cols) if cols > 1 else (rows_per_rank,), float(rank), dtype=torch.float32, device=dev)
    ts = []
    for i in range(reps + 3):
        if dev == "cuda":
            torch.cuda.synchronize()
        distributed.barrier()
        t0 = time.perf_counter()
        full = distributed.all_gather_rows(block, rows_per_rank * size)
        if dev == "cuda":
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if i >= 3:
            ts.append(dt)
    assert full.shape[0] == rows_per_rank * size
    return round(max(max_over_ranks(sorted(ts)[len(ts) // 2])) * 1e3, 4)


# saturated weak-scaling companions of the two strong-scaling legs: at 8 ranks C3 is 128
# pairs and C4 512 grid points per GPU -- pure latency; these keep every GPU full whatever the world size
C3_SATURATED_PAIRS_PER_RANK = 16384
C4_SATURATED_POINTS_PER_RANK = 32768


def expressibility_leg(n=12, samples=1024, reps=21, warm=100, scaling="strong"):
    """BASELINE config 3 (strong scaling): KL-to-Haar, 12 qubits, 1024 pairs (2048 states), HE 3
    layers, no DRU; the PAIRS are split over the ranks, one all-gather of 1024 floats."""
    from qml_essentials_amd import distributed
    from qml_essentials_amd.expressibility import Expressibility
    from qml_essentials_amd.model import Model

    m = Model(n, 3, "Hardware_Efficient", data_reupload=False)
    Expressibility.kl_divergence_to_haar(m, n_samples=max(64, distributed.world()[1]), n_bins=75, random_key=1)
    for _ in range(warm):  # ~20 ms: past the clock transient that follows the HBM-bound headline steps
        Expressibility.kl_divergence_to_haar(m, n_samples=samples, n_bins=75, random_key=1000)
    sec, kl, gpu_ms = _wall(lambda: Expressibility.kl_divergence_to_haar(m, n_samples=samples, n_bins=75,
                                                                         random_key=1000), reps)
    size = distributed.world()[1]
    per_rank = [hi - lo for lo, hi in distributed.all_shard_bounds(samples, size)]
    return {"seconds": round(sec, 6), "gpu_ms": round(gpu_ms, 4), "kl": float(np.mean(kl)), "n_qubits": n, "pairs": samples,
            "pairs_per_rank": per_rank, "pairs_per_s": round(samples / sec, 1),
            "scaling": scaling, "collective": f"one all-gather of the fidelities ({samples * 4 / 1024:g} KiB)",
            "collective_ms": collective_ms(max(per_rank), 1),
            "note": "median of %d calls, max over ranks; the whole call: parameter sampling (on the GPU), 2 x pairs states, "
                    "fidelities, histogram (GPU), one device -> host copy of the 75 counts, KL on the host; gpu_ms = HIP events "
                    "around the call on the launch stream" % reps}


def fourier_grid_leg(n=10, layers=6, points=4096, reps=21, warm=100, scaling="strong"):
    """BASELINE config 4 (strong scaling): Model(10, 6, HE) on the 2^12-point input grid,
    expval averaged over the wires; the GRID is split over the ranks (512 points per GPU at N = 8),
    one all-gather of (4096, 10) floats; the FFT of the 4096 values runs on the host."""
    from qml_essentials_amd import distributed
    from qml_essentials_amd.coefficients import Coefficients
    from qml_essentials_amd.model import Model

    m = Model(n, layers, "Hardware_Efficient")
    x = torch.from_numpy((2 * np.pi * np.arange(points) / points).astype(np.float32).reshape(-1, 1)).cuda()

    def call():
        # what Coefficients._fourier_transform does with its own (device-resident) grid: one
        # device -> host copy of the 4096 values, float64 real-input FFT on the host (16 us)
        y = m(inputs=x, force_mean=True)
        return Coefficients._fft_real(y.cpu().numpy().astype(np.float64))

    for _ in range(warm):  # ~20 ms of warm-up, as for the other legs
        call()
    sec, coeffs, gpu_ms = _wall(call, reps)
    size = distributed.world()[1]
    per_rank = [hi - lo for lo, hi in distributed.all_shard_bounds(points, size)]
    return {"seconds": round(sec, 6), "gpu_ms": round(gpu_ms, 4), "n_qubits": n, "n_layers": layers, "grid_points": points,
            "points_per_rank": per_rank, "points_per_s": round(points / sec, 1),
            "c0": float(coeffs[0].real), "max_abs_coeff_beyond_degree": float(np.abs(coeffs[layers * n + 1:points // 2]).max()),
            "scaling": scaling, "collective": f"one all-gather of the expectation values ({points * n * 4 / 1024:g} KiB)",
            "collective_ms": collective_ms(max(per_rank), n),
            "note": "median of %d calls, max over ranks; circuit batch on the GPU, one device -> host copy of the values, "
                    "float64 FFT on the host; gpu_ms = HIP events around the call on the launch stream" % reps}


def sampling_loops_cpu(budget_pairs=128, budget_points=384):
    """CPU restatement of BASELINE configs 3 and 4 timed beside the GPU legs (rank 0, N = 1): the
    NumPy-einsum oracle (oracle/einsum_sim.py, one thread, complex64 like the reference's default)
    on a bounded sample of the SAME parameter sets / grid points, extrapolated to the full loop, and
    compared with the GPU's fidelities / expectation values (complex128 oracle, 1e-6)."""
    from oracle import circuits as OC, einsum_sim as OE
    from qml_essentials_amd.expressibility import Expressibility
    from qml_essentials_amd.model import Model

    out = {}
    n, S = 12, 1024
    m = Model(n, 3, "Hardware_Efficient", data_reupload=False)
    fid = Expressibility._sample_state_fidelities(m, S, random_key=1000).cpu().numpy()
    params = np.asarray(m.params)
    spec = OC.ModelSpec(n, 3, "Hardware_Efficient", data_reupload=False)
    idx = np.random.default_rng(0).choice(S, budget_pairs, replace=False)
    t0 = time.perf_counter()
    for i in idx:
        a = OE.simulate_pure(OC.model_tape(spec, params[i], [0.0]), n, np.complex64)
        b = OE.simulate_pure(OC.model_tape(spec, params[i + S], [0.0]), n, np.complex64)
        abs(np.vdot(a, b)) ** 2
    sec = time.perf_counter() - t0
    worst = 0.0
    for i in idx[:8]:
        a = OE.simulate_pure(OC.model_tape(spec, params[i], [0.0]), n, np.complex128)
        b = OE.simulate_pure(OC.model_tape(spec, params[i + S], [0.0]), n, np.complex128)
        worst = max(worst, abs(float(fid[i]) - abs(np.vdot(a, b)) ** 2))
    if worst > 1e-5:
        raise SystemExit(f"bench.py: GPU fidelities differ from the CPU oracle by {worst:.3e}")
    out["c3"] = {"seconds_full_loop_extrapolated": round(sec * S / budget_pairs, 3), "cores": 1, "kind": "port",
                 "sample": f"{budget_pairs} of the {S} pairs ({2 * budget_pairs} statevectors, 144 gates each), "
                           f"oracle/einsum_sim.py complex64, {sec:.2f} s",
                 "max_abs_diff_gpu_vs_fp64_oracle": worst}
    n, G = 10, 4096
    m = Model(n, 6, "Hardware_Efficient")
    p = np.asarray(m.params[0])
    grid = (np.arange(G, dtype=np.float64) * 2 * np.pi / G).astype(np.float32).reshape(G, 1)
    gpu = np.asarray(m(inputs=grid, force_mean=True))
    spec = OC.ModelSpec(n, 6, "Hardware_Efficient")
    obs = [("PauliZ", [q]) for q in range(n)]
    idx = np.random.default_rng(1).choice(G, budget_points, replace=False)
    t0 = time.perf_counter()
    for k in idx:
        OE.simulate_and_measure(OC.model_tape(spec, p, [float(grid[k, 0])]), n, "expval", obs, np.complex64)
    sec = time.perf_counter() - t0
    worst = 0.0
    for k in idx[:8]:
        want = OE.simulate_and_measure(OC.model_tape(spec, p, [float(grid[k, 0])]), n, "expval", obs, np.complex128)
        worst = max(worst, abs(float(gpu[k]) - float(np.mean(want))))
    if worst > 1e-5:
        raise SystemExit(f"bench.py: GPU grid values differ from the CPU oracle by {worst:.3e}")
    out["c4"] = {"seconds_full_loop_extrapolated": round(sec * G / budget_points, 3), "cores": 1, "kind": "port",
                 "sample": f"{budget_points} of the {G} grid points (340 gates + <Z> on 10 wires each), "
                           f"oracle/einsum_sim.py complex64, {sec:.2f} s",
                 "max_abs_diff_gpu_vs_fp64_oracle": worst}
    return out


def lds_regime_leg(n, layers, dru, batch, meas, reps=10):
    """Whole-state-in-LDS regime (n <= 14): circuit (+ measurement) of `batch` states in ONE launch;
    `kernel_ms` = HIP events around the whole call on the GPU (angle table, fp64 matrix builder,
    circuit launch), `circuit_launch_ms` = the circuit launch alone.  SURVEY 8-d: the bound is LDS bandwidth / fp32 VALU, HBM traffic is parameters
    in and results out -- reported as states/s and executed fp32 TFLOP/s against the vector peak,
    not as an HBM fraction."""
    from qml_essentials_amd import _native as N
    from qml_essentials_amd import simulation
    from qml_essentials_amd.model import Model

    model = Model(n, layers, "Hardware_Efficient", data_reupload=dru)
    rng = np.random.default_rng(1000)
    params = rng.uniform(0, 2 * np.pi, (batch, *model.params.shape[1:])).astype(np.float32)
    x = None if not dru else np.full((1, 1), 0.5, dtype=np.float32)
    tape, _ = model.record_tape(params=params[:2], inputs=x)
    low = simulation.LoweredTape(tape, n)
    top = simulation.get_plan(low)
    plan = top.executed(meas)
    desc = plan.describe()
    pd = torch.from_numpy(params).cuda()
    xd = None if x is None else torch.from_numpy(x).cuda()
    kw = dict(execution_type=meas)

    def call():
        return model(params=pd, **kw) if xd is None else model(params=pd, inputs=xd, **kw)

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    # whole call on the GPU: angle table (qmle_build_angles) + per-sample matrices in fp64
    # (k_build_matrices) + the circuit / measurement launch; the stage events cover the last only
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    plan.profile_begin(len(desc["stages"]) * reps * 4 + 16)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    ms, cnt, _ = plan.profile_end()
    kernel_ms = e0.elapsed_time(e1) / reps
    circuit_launch_ms = sum(ms) / reps
    flops = desc["flops_per_state"] * batch
    tf = flops / (kernel_ms * 1e-3) / 1e12 if kernel_ms > 0 else 0.0
    lds_bytes = 0.0  # one LDS round trip (read + write of the 8 D-byte state) per register-tile group
    for st in desc["stages"]:
        lds_bytes += 16.0 * (1 << n) * max(1, len(st.get("fast_groups") or st.get("groups") or []))
    return {"n_qubits": n, "gates_per_state": len(low.ops), "operators_applied_per_state": desc["n_lowered"],
            "states_per_launch": batch, "measurement": meas, "whole_state_lds": desc["whole_state_lds"],
            "kernel_ms": round(kernel_ms, 5), "circuit_launch_ms": round(circuit_launch_ms, 5),
            "launches": int(sum(cnt) / reps),
            "states_per_s": round(batch / (kernel_ms * 1e-3), 1),
            "gate_applies_per_s": round(len(low.ops) * batch / (kernel_ms * 1e-3), 1),
            "fp32_flops_per_state": desc["flops_per_state"],
            "tflops": round(tf, 2), "valu_peak_tflops": VALU_PEAK_TFLOPS,
            "frac_of_valu_peak": round(tf / VALU_PEAK_TFLOPS, 4),
            "lds_GBps": round(lds_bytes * batch / (kernel_ms * 1e-3) / 1e9, 1),
            "bound": "lds/valu"}


def k2_unfused_leg(n, B, steps=2):
    """SURVEY 8-d `achieved_unfused`: one HBM pass per REFERENCE gate (QMLE_PLAN_NO_FUSION | NO_MERGE,
    all amplitudes live, nothing folded) -- what simulation.py:102-103 does.  frac = the SURVEY 8-d
    bytes of the 96 gates / the summed HIP-event time of their launches / 8 TB/s, <= 1 by construction."""
    from qml_essentials_amd import _native as N

    fl = N.PLAN_NO_SPARSE | N.PLAN_NO_ABSORB | N.PLAN_NO_FUSION | N.PLAN_NO_MERGE
    run = timed_k2(n, B, 1, steps, 1, fl, isolate_passes=True)
    desc = run["desc"]
    states = B * steps
    kinds = {}
    for i, st in enumerate(desc["stages"]):
        k = kinds.setdefault(st["kind"], {"ms": 0.0, "launches": 0, "algo": 0.0, "passes": 0})
        k["ms"] += run["stage_ms"][i]
        k["launches"] += run["stage_cnt"][i]
        k["algo"] += st["algo_bytes_per_state"] * states
        k["passes"] += 1
    d = kinds.get("direct", {"ms": 0.0, "launches": 0, "algo": 0.0, "passes": 0})
    sec = d["ms"] * 1e-3
    gbps = d["algo"] / sec / 1e9 if sec > 0 else 0.0
    return {"ms_per_step": round(run["elapsed"] / steps * 1e3, 3), "batch": B, "steps": steps,
            "gate_applies_per_s": round(run["n_gates"] * states / run["elapsed"], 1),
            "statevectors_per_s": round(states / run["elapsed"], 2),
            "hbm_passes_per_state": len(desc["stages"]),
            "roofline": {"bound": "hbm", "kernel": "k_direct_1q", "achieved": round(gbps, 1),
                         "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(gbps / HBM_PEAK_GBPS, 4),
                         "avg_launch_ms": round(d["ms"] / max(1, d["launches"]), 5),
                         "launches": d["launches"], "passes_per_state": d["passes"],
                         "algorithmic_bytes_per_launch": round(d["algo"] / max(1, d["launches"])),
                         "fusion_factor": 1.0,
                         "note": "every reference gate is its own in-place HBM pass (k_direct_1q); the first "
                                 "launch of a state also holds the |0..0> initialisation; <Z> is one more "
                                 "read (k_expval_partial), outside this kernel's time"},
            "max_abs_diff_vs_headline_expvals": None, "_out": run["out"]}


L2_PEAK_GBPS = 34500.0          # aggregate L2, /opt/skills/guides/MI355X_MICROARCH.md:316
MALL_GATHER_GBPS = 8600.0       # Infinity-Cache-resident table, measured gather rate, same guide :349


def pass_table(run, dense):
    """Every pass of a profiled run: kernel, register-tile groups, HIP-event time per state, bytes moved per
    state and nominal flops, each as a rate and as a fraction of its peak (8 TB/s, 157.3 TFLOP/s fp32), and
    which of the two the pass is nearer to: `hbm` or `valu+lds` (register-tile groups: packed-FMA issue and LDS
    round trips; counters in profiles/r05_deep_default_sq.txt); `launch` for passes under 3 us per launch."""
    desc, n, B, steps = run["desc"], run["n"], run["B"], run["steps"]
    ns = len(desc["stages"])
    rows = []
    for i, st in enumerate(desc["stages"]):
        moved = st["read_bytes_from_zero"] + st["write_bytes_from_zero"]
        if i == ns - 1 and st["kind"] == "tile":
            moved = st["read_bytes_from_zero"]
        us = run["stage_ms"][i] * 1e3 / (B * steps)
        gbps = moved / us / 1e3 if us > 0 else 0.0
        groups = len(st.get("fast_groups") or st.get("groups") or [])
        launch_us = run["stage_ms"][i] * 1e3 / max(1, run["stage_cnt"][i])
        # fp32 flops of the pass's operators: nominal for all-live plans, else charged for the amplitudes that can
        # be non-zero when each operator is applied (qmle_plan.cpp stage_flops_per_state)
        fl = st.get("flops_per_state", 0.0) if dense else st.get("flops_live_per_state", st.get("flops_per_state", 0.0))
        tf = fl / us / 1e6 if us > 0 else 0.0
        hbm_frac, valu_frac = gbps / HBM_PEAK_GBPS, tf / VALU_PEAK_TFLOPS
        # (nominal flops / peak understates the vector unit's load: the counters show 69-76 % of the cycles issuing vector
        # instructions at a nominal 0.40-0.45 -- r05_k2_headline_sq.txt, r05_deep_default_sq.txt -- so the two sides are
        # compared with that factor)
        bound = "launch" if launch_us < 3.0 else (
            "hbm" if hbm_frac >= VALU_ISSUE_PER_NOMINAL * valu_frac and hbm_frac >= 0.3 else "valu+lds")
        rows.append({"pass": i + 1, "kernel": kernel_of_stage(st, i, ns, n, dense), "T": st.get("T"),
                     "groups": groups, "ops": len(st["src_ops"]), "operators": st.get("n_lowered"), "us_per_state": round(us, 3),
                     "bytes_moved_per_state": int(moved), "moved_GBps": round(gbps, 1), "hbm_frac": round(hbm_frac, 3),
                     "tflops": round(tf, 1), "valu_frac": round(valu_frac, 3), "bound": bound})
    return rows


def valu_roofline(run, dense):
    """The vector-unit side of a run whose passes are not HBM-bound: fp32 flops of the operators the plan applies
    (14 per amplitude for a dense 2x2, 6 for a diagonal one, halved per control, 0 for X / CX) -- for plans that
    track known zeros charged only for the amplitudes that can be non-zero when the operator is applied
    (stage_flops_per_state in qmle_plan.cpp) -- / the summed HIP-event time of the passes."""
    sec = sum(run["stage_ms"]) * 1e-3 / (run["B"] * run["steps"])
    key = "flops_per_state" if dense else "flops_live_per_state"
    flops = sum(st.get(key, st.get("flops_per_state", 0.0)) for st in run["desc"]["stages"])
    tf = flops / sec / 1e12 if sec > 0 else 0.0
    return {"bound": "valu", "achieved": round(tf, 2), "peak": VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(tf / VALU_PEAK_TFLOPS, 4), "fp32_flops_per_state": flops,
            "flops_counted": "nominal (every amplitude live)" if dense else "live amplitudes only (known zeros discounted)"}


def bound_of(rows):
    """Time-weighted verdict over a pass table: share of the step spent in passes of each kind."""
    tot = sum(r["us_per_state"] for r in rows) or 1.0
    share = {}
    for r in rows:
        share[r["bound"]] = share.get(r["bound"], 0.0) + r["us_per_state"] / tot
    top = max(share, key=share.get)
    return top, {k: round(v, 3) for k, v in sorted(share.items())}


def c2_leg(cpu_seconds=6.0):
    """BASELINE config 2: Model(20, 4, Hardware_Efficient), data re-uploading, input 0.5, expval on all 20 wires
    (480 reference gates per state, model.py:1572-1737) -- the regime where a state (8 MiB) fits the L2 / the
    Infinity Cache: single sample, batches of 256 and 1024 parameter sets under the default engine, batch 1024
    with every amplitude live beside it.  Rates are quoted against BOTH the HBM peak and the L2 figure; bytes
    are the executed plan's passes.  CPU: the oracle's C/OpenMP port on the same parameter sets, every <Z> row
    compared (complex64 both sides: 1e-5)."""
    from oracle import c_port, circuits as OC  # the checker (cpu_baseline leg)
    from qml_essentials_amd import _native as N

    n, layers = 20, 4
    out = {"workload": "Model(20, 4, Hardware_Efficient), data re-uploading, input 0.5, <Z> on 20 wires, 480 gates/state"}
    runs = {}
    for label, B, steps, fl in (("single_sample", 1, 40, 0), ("batch_256", 256, 8, 0), ("batch_1024", 1024, 4, 0),
                                ("batch_1024_all_live", 1024, 4, N.PLAN_NO_SPARSE | N.PLAN_NO_ABSORB)):
        run = timed_k2(n, B, 1, steps, 3, fl, layers=layers, dru=True, x=0.5, isolate_passes=True)
        dense = fl != 0
        sm = summarize(run, dense)
        rows = pass_table(run, dense)
        fam = families(run, dense)
        name = max(fam, key=lambda k: fam[k]["ms"])
        dom = fam[name]
        gbps = dom["moved"] / (dom["ms"] * 1e-3) / 1e9 if dom["ms"] > 0 else 0.0
        top, share = bound_of(rows)
        kernel_ms = sum(run["stage_ms"]) / steps
        out[label] = {
            "batch": B, "steps": steps, "ms_per_step": sm["ms_per_step"], "kernel_ms_per_step": round(kernel_ms, 4),
            "statevectors_per_s": sm["statevectors_per_s"], "gate_applies_per_s": sm["gate_applies_per_s"],
            "gates_counted_per_state": sm["gates_counted_per_state"],
            "operators_executed_per_state": run["desc"]["n_lowered"],
            "hbm_passes_per_state": sm["hbm_passes_per_state"],
            "bytes_moved_per_state": sm["hbm_bytes_moved_per_state"],
            "step_moved_GBps": round(sm["hbm_bytes_moved_per_state"] * B / (kernel_ms * 1e-3) / 1e9, 1) if kernel_ms > 0 else None,
            "roofline": {"bound": top, "time_share_by_bound": share, "kernel": name,
                         "achieved": round(gbps, 1), "unit": "GB/s",
                         "peak": HBM_PEAK_GBPS, "frac": round(gbps / HBM_PEAK_GBPS, 4),
                         "peak_l2": L2_PEAK_GBPS, "frac_of_l2": round(gbps / L2_PEAK_GBPS, 4),
                         "valu": valu_roofline(run, dense),
                         "infinity_cache_gather_GBps": MALL_GATHER_GBPS,
                         "avg_launch_ms": round(dom["ms"] / max(1, dom["launches"]), 5), "launches": dom["launches"],
                         "kernel_share_of_step": round(dom["ms"] / (run["elapsed"] * 1e3), 4),
                         "all_kernels_ms": {k: round(v["ms"], 3) for k, v in fam.items()},
                         "note": "achieved = bytes the dominant kernel's launches read + wrote (the executed plan's "
                                 "passes) / their HIP-event time; a 20-qubit state is 8 MiB: one launch's states "
                                 "(<= 4 GiB in flight) do not fit the 256 MiB Infinity Cache beyond ~32 states, so "
                                 "batches stream from HBM and the single sample runs out of L2 / Infinity Cache"},
            "per_pass": rows}
        runs[label] = run
    # CPU port on the batch's own parameter sets + parity of every row it computes
    spec = OC.ModelSpec(n, layers, "Hardware_Efficient")
    threads = c_port.lib().svc_max_threads()
    rows_p = runs["batch_256"]["params"]
    gpu = runs["batch_256"]["out"].reshape(-1, n).cpu().numpy()
    gpu_live = runs["batch_1024_all_live"]["out"].reshape(-1, n).cpu().numpy()
    done, worst, worst_live, t0 = 0, 0.0, 0.0, time.perf_counter()
    while done < min(32, len(rows_p)):
        tape = OC.model_tape(spec, rows_p[done], [0.5])
        psi = c_port.simulate(tape, n)
        ez = c_port.expval_z(psi, n, list(range(n)))
        worst = max(worst, float(np.abs(ez - gpu[done]).max()))
        worst_live = max(worst_live, float(np.abs(ez - gpu_live[done]).max()))
        done += 1
        if time.perf_counter() - t0 >= cpu_seconds:
            break
    el = time.perf_counter() - t0
    if max(worst, worst_live) > 1e-5:
        raise SystemExit(f"bench.py: C2 GPU <Z> differs from the CPU oracle port by {max(worst, worst_live):.3e} (> 1e-5)")
    single = runs["single_sample"]["out"].reshape(-1, n).cpu().numpy()
    tape = OC.model_tape(spec, runs["single_sample"]["params"][0], [0.5])
    ez1 = c_port.expval_z(c_port.simulate(tape, n), n, list(range(n)))
    worst1 = float(np.abs(ez1 - single[0]).max())
    if worst1 > 1e-5:
        raise SystemExit(f"bench.py: C2 single-sample GPU <Z> differs from the CPU oracle port by {worst1:.3e}")
    gates = sum(1 for g in tape if g[0] != "Barrier")
    out["cpu_baseline"] = {"value": round(done * gates / el, 2), "unit": "gate-applies/s", "cores": threads, "kind": "port",
                           "statevectors_per_s": round(done / el, 3), "ms_per_state": round(el / done * 1e3, 2),
                           "sample": f"{done} of the batch's parameter sets (same tape: {gates} gates + <Z> on {n} wires), "
                                     f"oracle/sv_cpu.c with {threads} OpenMP threads, {el:.1f} s; every row compared with the GPU's",
                           "max_abs_diff_vs_gpu_expvals": {"batch_256": worst, "batch_1024_all_live": worst_live,
                                                           "single_sample": worst1}}
    return out


def k2_circuit19_leg(n, B, size, steps, warmup):
    """SURVEY 8-d K2's second tape: Circuit_19 (RX, RZ per wire + a ring of CRX: 48 one-qubit + 24 CRX gates at
    n = 24, ansaetze.py:671-683), one layer, no data re-uploading, every amplitude live, batch B."""
    from qml_essentials_amd import _native as N

    fl = N.PLAN_NO_SPARSE | N.PLAN_NO_ABSORB
    run = timed_k2(n, B, size, steps, warmup, fl, circuit="Circuit_19", isolate_passes=True)
    sm = summarize(run, True)
    rf = roofline_of(run, True, None)
    sm["operators_executed_per_state"] = run["desc"]["n_lowered"]
    sm["roofline"] = {k: rf[k] for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "avg_launch_ms", "launches",
                                          "passes_per_state", "bytes_moved_per_launch", "algorithmic_bytes_per_launch",
                                          "algorithmic_GBps", "fusion_factor", "kernel_share_of_step", "all_kernels_ms", "per_pass")}
    sm["workload"] = (f"Model({n}, 1, Circuit_19, data_reupload=False), {run['n_gates']} gates/state, all amplitudes live, "
                      f"batch {B}, {steps} timed steps")
    return sm, run


def _he_layer_ops(n):
    """One Hardware_Efficient layer as native ops (RY RZ RY per wire + the two CX brick layers,
    ansaetze.py:713-733) -- wire pairs from the product's own Topology."""
    from qml_essentials_amd.topologies import Topology

    ops = [(g, [q], [i * n + q], -1) for i, g in enumerate(("RY", "RZ", "RY")) for q in range(n)]
    ops += [("CX", [a, b], [], -1) for a, b in Topology.bricks(n, mirror=False) +
            Topology.bricks(n, offset=-1, modulo=True, wrap=True, mirror=False)]
    return ops, 3 * n


def widened_rows_leg():
    """SURVEY 8-f rows through the drop-in API (wall-clock per call, median of 5 after a warm-up; host arrays in and
    out): a noisy model (vec(rho) on the doubled register, compiled call), Bell measurements on two copies of the state,
    shot estimates.  Parity: the noisy <Z> of a 3-qubit model against oracle/noise.py's density evolution (2e-6)."""
    from oracle import noise as ON
    from qml_essentials_amd.entanglement import Entanglement
    from qml_essentials_amd.model import Model
    from qml_essentials_amd.tape import recording
    from qml_essentials_amd.utils import PRNGKey

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests"))
    from helpers import frontend_to_oracle

    noise = {"BitFlip": 0.01, "PhaseFlip": 0.02, "Depolarizing": 0.03, "AmplitudeDamping": 0.05, "PhaseDamping": 0.06}
    rng = np.random.default_rng(1000)

    def wall(fn, reps=5):
        fn(); torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        return round(sorted(ts)[len(ts) // 2] * 1e3, 3)

    out = {}
    x = np.array([0.5], dtype=np.float32)
    for n, layers, B in ((8, 3, 256), (10, 2, 64)):
        m = Model(n, layers, "Hardware_Efficient")
        P = rng.uniform(0, 2 * np.pi, (B, *m.params.shape[1:])).astype(np.float32)
        out[f"noisy_model_{n}q_{layers}l_batch{B}_expval_ms"] = wall(
            lambda: m(params=P, inputs=x, noise_params=dict(noise), execution_type="expval"))
    m = Model(3, 2, "Hardware_Efficient")
    P = rng.uniform(0, 2 * np.pi, (4, *m.params.shape[1:]))
    got = m(params=P, inputs=x, noise_params=dict(noise), execution_type="expval")
    err = 0.0
    for b in range(4):
        with recording() as tape:
            m._variational(P[b], x, random_key=PRNGKey(0), noise_params=m.noise_params)
        rho = ON.simulate_mixed(frontend_to_oracle(tape), 3)
        idx = np.arange(8)
        want = [float(np.real(np.diag(rho) * (1 - 2 * ((idx >> (2 - q)) & 1))).sum()) for q in range(3)]
        err = max(err, float(np.abs(np.asarray(got[b]) - np.array(want)).max()))
    assert err < 2e-6, err
    out["noisy_expval_max_abs_diff_vs_oracle_density"] = err
    m = Model(10, 2, "Hardware_Efficient")
    out["bell_measurements_10q_256samples_ms"] = wall(
        lambda: Entanglement.bell_measurements(m, n_samples=256, random_key=PRNGKey(1000)), reps=3)
    ms = Model(10, 2, "Hardware_Efficient", shots=1024)
    P = rng.uniform(0, 2 * np.pi, (256, *ms.params.shape[1:])).astype(np.float32)
    out["expval_from_1024_shots_10q_batch256_ms"] = wall(lambda: ms(params=P, inputs=x, execution_type="expval"))
    out["note"] = ("SURVEY 8-f rows, wall-clock per API call with host arrays in and out; start-of-round-5 figures and the "
                   "CPU oracle beside them: profiles/r05_next_rows.md")
    return out


def mw_28q_leg(n=28, reps=100, warmup=25):
    """BASELINE config 5: Meyer-Wallach of ONE 2^28 statevector (2 GiB, HE layer applied to |0..0>),
    HIP events around `reps` calls.  Two forms: `resident` -- qmle_meyer_wallach on a state that
    already lies in HBM (three reads) -- and `fused` -- QMLE_MEAS_MEYER_WALLACH, where the circuit's
    last pass reports the sums of its own tile from LDS and two reads remain; `fused_ms` is what
    Entanglement.meyer_wallach spends after the circuit = (circuit + Meyer-Wallach) - (circuit alone).
    frac = the 8 D-byte single read of SURVEY 8-d / time / 8 TB/s; moved_frac = bytes the reads of
    the call really fetch / time / 8 TB/s."""
    from qml_essentials_amd import _native as N

    ops, slots = _he_layer_ops(n)
    ang = torch.from_numpy(np.random.default_rng(6).uniform(0, 6.28, (1, slots)).astype(np.float32)).cuda()
    plan = N.Plan(ops, n, slots)
    st = plan.run(ang, "state")

    def timed(fn):
        for _ in range(warmup):  # ~25 ms: past the clock transient that follows an idle period
            out = fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, out

    ms, q = timed(lambda: N.meyer_wallach(st))
    ws_s = torch.empty(plan.workspace_bytes(1, "state"), dtype=torch.uint8, device="cuda")
    ws_m = torch.empty(plan.workspace_bytes(1, "mw"), dtype=torch.uint8, device="cuda")
    circ_ms, _ = timed(lambda: plan.run(ang, "state", out=st, workspace=ws_s))
    # the default route since round 5: the last pass reports its tile's sums (lean epilogue, streaming stores), two reads remain
    both_ms, qf = timed(lambda: plan.run(ang, "mw", workspace=ws_m))
    os.environ["QMLE_MW_FUSE_TILED"] = "0"  # (read per call) the three stand-alone reads behind the circuit
    try:
        dflt_ms, qd = timed(lambda: plan.run(ang, "mw", workspace=ws_m))
    finally:
        del os.environ["QMLE_MW_FUSE_TILED"]
    fused_ms = both_ms - circ_ms
    D8 = 8.0 * (1 << n)
    reads = N.mw_reads(n)
    traffic, source, _, terr = load_traffic(f"meyer_wallach:n{n}")
    f_traffic, f_source, _, f_terr = load_traffic(f"meyer_wallach_fused:n{n}")
    if abs(float(qf[0, 0]) - float(q[0])) > 2e-6:
        raise SystemExit(f"bench.py: fused Meyer-Wallach {float(qf[0, 0])} differs from the resident one {float(q[0])}")
    del st, ws_s, ws_m
    torch.cuda.empty_cache()
    return {"ms": round(ms, 4), "Q": float(q[0]), "n_qubits": n, "state_bytes": int(D8),
            "reads_of_the_state_per_call": reads, "calls_timed": reps, "calls_warmup": warmup,
            "fused_ms": round(fused_ms, 4), "circuit_ms": round(circ_ms, 4), "circuit_plus_mw_ms": round(both_ms, 4),
            "after_circuit_ms_stand_alone_reads": round(dflt_ms - circ_ms, 4), "Q_stand_alone_reads": float(qd[0, 0]),
            "fused_adopted_for_tiled_states": True,
            "fused_note": "QMLE_MEAS_MEYER_WALLACH (what Entanglement.meyer_wallach runs): the circuit's last pass reports the "
                          "sums of its own tile from LDS -- for tiled states the cross terms of its 8 positions above 3 and "
                          "the populations; positions 0..3 come from the first of the two later reads, which is HBM-bound "
                          "with issue slots to spare -- and stores the state with streaming stores, so the later reads do "
                          "not run into its write-back.  fused_ms = (circuit + Meyer-Wallach) - (circuit alone); "
                          "after_circuit_ms_stand_alone_reads = the same with QMLE_MW_FUSE_TILED=0 (three reads of the stored state); "
                          "ms = qmle_meyer_wallach on a state that already lies in HBM (three reads)",
            "fused_reads_after_the_circuit": reads - 1, "Q_fused": float(qf[0, 0]),
            "fused_roofline": {"bound": "hbm+valu", "kernel": "tile_mw_row in the circuit's last pass + k_mw_read_later_low + k_mw_read_later",
                               "byte_floor_ms": round((reads - 1) * D8 / (HBM_PEAK_GBPS * 1e6), 4),
                               "valu_issue_floor_ms_of_the_epilogue": round((1 << n) / 16 / 64 / 1024 * (2 * 64 + 31 * 6 + 60) * 4 / 2.1e6, 4),
                               "achieved": round(D8 / fused_ms / 1e6, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                               "frac": round(D8 / fused_ms / 1e6 / HBM_PEAK_GBPS, 4),
                               "moved_frac": round((reads - 1) * D8 / fused_ms / 1e6 / HBM_PEAK_GBPS, 4),
                               "traffic": f_traffic, "traffic_source": f_source, "traffic_error": f_terr,
                               "note": "time after the circuit = (circuit + Meyer-Wallach) - (circuit alone), same plan, "
                                       "HIP events over back-to-back calls; traffic = PMC bytes fetched by the two later reads.  "
                                       "byte_floor = the two later reads at 8 TB/s; the epilogue's issue floor = its vector "
                                       "instructions per work item and tile (128 packed fmas of cross terms, 31 values x 6 "
                                       "DPP adds of the wave reduction, ~60 for populations / addresses) x 4 cycles on 1024 SIMDs "
                                       "at 2.1 GHz: the producing pass issues vector instructions 85 % of its cycles "
                                       "(profiles/r05_mw_sq_fused.txt), so the epilogue is paid in full"},
            "roofline": {"bound": "hbm", "kernel": "k_mw_read_first + 2 x k_mw_read_later", "achieved": round(D8 / ms / 1e6, 1),
                         "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(D8 / ms / 1e6 / HBM_PEAK_GBPS, 4),
                         "moved_GBps": round(reads * D8 / ms / 1e6, 1),
                         "moved_frac": round(reads * D8 / ms / 1e6 / HBM_PEAK_GBPS, 4),
                         "traffic": traffic, "traffic_source": source, "traffic_error": terr,
                         "note": "resident state: frac counts ONE read of the state (8 D bytes, SURVEY 8-d) per call; the "
                                 "call reads it reads_of_the_state_per_call times (moved_frac); traffic = PMC bytes "
                                 "fetched per call"}}


def mw_cpu_baseline(n_small=24, n_full=28):
    """CPU restatement of BASELINE config 5 beside the GPU leg: the NumPy oracle's qubit purities
    (oracle/analysis.py, one thread) on the same kind of state at n_small qubits -- one 2^28 state
    costs the oracle minutes -- extrapolated by the state size, and compared with the GPU's
    purities of that very state."""
    from oracle import analysis as OA  # the checker (cpu_baseline leg)
    from qml_essentials_amd import _native as N

    n = n_small
    ops, slots = _he_layer_ops(n)
    ang = torch.from_numpy(np.random.default_rng(6).uniform(0, 6.28, (1, slots)).astype(np.float32)).cuda()
    plan = N.Plan(ops, n, slots)
    st = plan.run(ang, "state")
    q, pur = N.meyer_wallach(st, return_purities=True)
    fused = plan.run(ang, "mw")  # the same purities out of the producing pass
    if float((fused[0, 1:] - pur[0]).abs().max()) > 2e-6:
        raise SystemExit("bench.py: fused and resident Meyer-Wallach purities differ")
    psi = st[0].cpu().numpy()
    t0 = time.perf_counter()
    OA.qubit_purities_pure(psi, n)  # complex64, like the reference's default: the timed run
    sec = time.perf_counter() - t0
    want = OA.qubit_purities_pure(psi.astype(np.complex128), n)  # the checker: fp64 sums
    worst = float(np.abs(pur[0].cpu().numpy().astype(np.float64) - want).max())
    if worst > 1e-5:
        raise SystemExit(f"bench.py: GPU qubit purities differ from the CPU oracle by {worst:.3e}")
    return {"seconds_extrapolated": round(sec * 2.0 ** (n_full - n_small), 2), "cores": 1, "kind": "port",
            "sample": f"one {n_small}-qubit state of the same circuit (128 MiB; {sec:.2f} s for its {n_small} "
                      f"purities with oracle/analysis.py qubit_purities_pure), scaled by 2^{n_full - n_small}",
            "max_abs_diff_gpu_vs_fp64_oracle_purities": worst}


def cpu_baseline(n, params_rows, budget_s, gpu_rows):
    """Oracle C/OpenMP port on a bounded sample of the same workload (rank 0, N=1); its <Z>
    values must equal the GPU's rows for the same parameter sets (atol 1e-5) or the run fails."""
    from oracle import c_port, circuits as OC

    spec = OC.ModelSpec(n, 1, "Hardware_Efficient", data_reupload=False)
    threads = c_port.lib().svc_max_threads()
    done, t0, worst, per_state = 0, time.perf_counter(), 0.0, []
    while True:
        t1 = time.perf_counter()
        tape = OC.model_tape(spec, params_rows[done], [0.0])
        psi = c_port.simulate(tape, n)
        ez = c_port.expval_z(psi, n, list(range(n)))
        per_state.append(time.perf_counter() - t1)
        worst = max(worst, float(np.max(np.abs(ez - gpu_rows[done]))))
        done += 1
        el = time.perf_counter() - t0
        if el >= budget_s or done >= min(64, len(params_rows)):
            break
    if worst > 1e-5:
        raise SystemExit(f"bench.py: GPU <Z> differs from the CPU oracle port by {worst:.3e} (> 1e-5)")
    gates = sum(1 for g in tape if g[0] != "Barrier")
    return {"value": round(done * gates / el, 2), "unit": "gate-applies/s", "cores": threads,
            "kind": "port", "statevectors_per_s": round(done / el, 4),
            "max_abs_diff_vs_gpu_expvals": worst,
            # the host is shared (other tenants of the 8-GPU box): the spread of the sample, not one number
            "gate_applies_per_s_fastest_median_slowest_state": [round(gates / t, 1) for t in
                                                                (min(per_state), float(np.median(per_state)), max(per_state))],
            "sample": f"{done} of the statevectors of one step (same tape: {gates} gates + <Z> on "
                      f"{n} wires, n={n}), oracle/sv_cpu.c with {threads} OpenMP threads (parallel "
                      f"first-touch initialisation), {el:.1f} s; every <Z> row compared with the GPU's"}


def cpu_einsum_legs(n, params_row, budget_s=6.0):
    """The two other CPU legs of SURVEY 8-d on ONE statevector of the step, bounded: the literal
    NumPy-einsum restatement (oracle/einsum_sim.py, one thread) and the same contraction with
    torch.einsum on all threads (closest analogue of XLA-CPU intra-op threading,
    script.py:308-311).  Gates are timed one by one until the budget is spent."""
    from oracle import circuits as OC, einsum_sim as OE, gates as G

    spec = OC.ModelSpec(n, 1, "Hardware_Efficient", data_reupload=False)
    tape = [g for g in OC.model_tape(spec, params_row, [0.0]) if g[0] != "Barrier"]
    comp = [(G.matrix(name, params).astype(np.complex64).reshape((2,) * (2 * len(wires))),
             OE.einsum_subscript(n, len(wires), tuple(wires))) for name, wires, params in tape]
    out = {}
    psi = np.zeros((2,) * n, dtype=np.complex64)
    psi[(0,) * n] = 1
    t0, k = time.perf_counter(), 0
    for gt, sub in comp:
        psi = np.einsum(sub, gt, psi)
        k += 1
        if time.perf_counter() - t0 > budget_s:
            break
    el = time.perf_counter() - t0
    out["numpy_einsum_1thread"] = {"gate_applies_per_s": round(k / el, 3), "gates_timed": k,
                                   "seconds": round(el, 2)}
    th = torch.get_num_threads()
    psi_t = torch.zeros((2,) * n, dtype=torch.complex64)
    psi_t[(0,) * n] = 1
    t0, k = time.perf_counter(), 0
    for gt, sub in comp:
        psi_t = torch.einsum(sub, torch.from_numpy(gt), psi_t)
        k += 1
        if time.perf_counter() - t0 > budget_s:
            break
    el = time.perf_counter() - t0
    out["torch_einsum_all_threads"] = {"gate_applies_per_s": round(k / el, 3), "gates_timed": k,
                                       "threads": th, "seconds": round(el, 2)}
    return out


def adjoint_gradient_wallclock(n=20, layers=4):
    """Extra: gradient of mean_q <Z_q> w.r.t. all parameters of BASELINE config 2's model
    (20 qubits, 4 layers, 300 parameters) by the fused adjoint sweep, CUDA tensors in and out."""
    from qml_essentials_amd.model import Model

    m = Model(n, layers, "Hardware_Efficient")
    p = torch.tensor(np.asarray(m.params[0]), dtype=torch.float32, device="cuda")
    x = torch.tensor([[0.5]], dtype=torch.float32, device="cuda")
    cot = torch.ones((1,), dtype=torch.float32, device="cuda")
    m.vjp_device(p, x, cot, force_mean=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        g, _ = m.vjp_device(p, x, cot, force_mean=True)
    torch.cuda.synchronize()
    return {"ms": round((time.perf_counter() - t0) / 10 * 1e3, 3), "n_qubits": n,
            "n_params": int(p.numel()), "finite": bool(torch.isfinite(g).all())}


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, max_bytes=DUMP_MAX_BYTES):
    """Write every array of `arrays` (name -> tensor / array) as out_dir/<name>.npy in float32 (float64 stays
    float64).  When they hold more than `max_bytes` together, each keeps a fixed, seeded sample of its rows
    (the same rows for the same shape, so that two builds can be compared file for file)."""
    host = {}
    for name, v in arrays.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        v = np.asarray(v)
        host[name] = v.astype(np.float64 if v.dtype == np.float64 else np.float32, copy=False)
    total = sum(v.nbytes for v in host.values())
    if total > max_bytes:
        for name, v in host.items():
            keep = max(1, int(v.shape[0] * max_bytes // total))
            rows = np.sort(np.random.default_rng(0).choice(v.shape[0], size=keep, replace=False))
            host[name] = np.ascontiguousarray(v[rows])
    os.makedirs(out_dir, exist_ok=True)
    for name, v in host.items():
        np.save(os.path.join(out_dir, name + ".npy"), v)
    return {name: list(v.shape) for name, v in host.items()}


def rank_bookkeeping(a, rank, size):
    """World checks shared by the full run and --rendezvous-only: the job must have exactly
    --gpus ranks on the nccl (RCCL) backend -- gloo only when QMLE_DIST_BACKEND asks for a rehearsal
    -- and every rank must answer the one collective the data path uses (all_gather_into_tensor)."""
    from qml_essentials_amd import distributed

    if size != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but the process group has {size} rank(s); launch with "
                         f"`python bench.py --gpus {a.gpus}` (spawns the ranks) or torch.distributed.run "
                         f"--nproc-per-node {a.gpus}")
    backend = torch.distributed.get_backend() if size > 1 else None
    if size > 1 and backend != "nccl" and os.environ.get("QMLE_DIST_BACKEND") != backend:
        raise SystemExit(f"bench.py: {size} ranks on backend {backend!r}; the data path needs nccl (RCCL)")
    token = np.array([[rank, os.getpid()]], dtype=np.float64)
    if size > 1:
        dev = "cuda" if backend == "nccl" else "cpu"
        token = distributed.all_gather_rows(torch.from_numpy(token).to(dev), size).cpu().numpy()
    seen = [int(r) for r in token[:, 0]]
    if seen != list(range(size)) or len({int(p) for p in token[:, 1]}) != size:
        raise SystemExit(f"bench.py: all-gather returned ranks {seen} for world size {size}")
    return {"ranks_seen": seen, "collective_backend": backend or "none (single rank)",
            "launched_by": os.environ.get("QMLE_BENCH_LAUNCHED_BY", "torch.distributed.run" if size > 1 else "python")}


def main(argv=None):
    a = parse_args(argv)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # launcher: this process has not touched the GPU (import torch does not) and never will
        raise SystemExit(launch_ranks(a.gpus, sys.argv[1:] if argv is None else list(argv)))
    from qml_essentials_amd import distributed
    import __graft_entry__ as entry

    rank, size = distributed.init_from_env()
    books = rank_bookkeeping(a, rank, size)
    if a.rendezvous_only:
        distributed.barrier()
        # the one collective of each sharded leg, by itself, on the payloads the legs gather (every rank takes part)
        legs = {"c3_expressibility_12q_1024pairs": {"rows_per_rank": -(-1024 // size), "cols": 1},
                "c4_fourier_10q_6l_4096grid": {"rows_per_rank": -(-4096 // size), "cols": 10},
                "c3_saturated_weak": {"rows_per_rank": C3_SATURATED_PAIRS_PER_RANK, "cols": 1},
                "c4_saturated_weak": {"rows_per_rank": C4_SATURATED_POINTS_PER_RANK, "cols": 10}}
        for leg in legs.values():
            leg["collective_ms"] = collective_ms(leg["rows_per_rank"], leg["cols"], reps=5)
            leg["payload_bytes_per_rank"] = leg["rows_per_rank"] * leg["cols"] * 4
        if rank == 0:
            print(json.dumps({"rendezvous_only": True, "n_gpus": size, **books, "scaling_legs": legs}), flush=True)
        if size > 1:
            torch.distributed.destroy_process_group()
        return
    if rank == 0:
        with contextlib.redirect_stdout(sys.stderr):  # stdout carries the ONE JSON line only
            entry.build()
    distributed.barrier()
    from qml_essentials_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X; there is no CPU fallback")
    if size == 1:
        torch.cuda.set_device(0)

    n, B = a.n_qubits, a.batch
    DENSE = N.PLAN_NO_SPARSE | N.PLAN_NO_ABSORB
    head_flags = DENSE | (N.PLAN_NO_FUSION if a.no_fusion else 0)
    head = timed_k2(n, B, size, a.steps, a.warmup, head_flags)
    dumped = None
    if a.dump_outputs and rank == 0:
        # the (B x ranks, n) <Z> rows the last timed call returned, on the seeded parameter sets
        dumped = dump_outputs(a.dump_outputs, {"expval": head["out"].reshape(-1, n)})

    aux = a.full and not a.skip_aux
    c3 = c4 = c3s = c4s = None
    if aux:  # sharded over all ranks -> every rank takes part
        c3 = expressibility_leg()
        c4 = fourier_grid_leg()
        c3s = expressibility_leg(samples=C3_SATURATED_PAIRS_PER_RANK * size, reps=7, warm=5, scaling="weak")
        c4s = fourier_grid_leg(points=C4_SATURATED_POINTS_PER_RANK * size, reps=7, warm=5, scaling="weak")
    if rank != 0:
        distributed.barrier()
        return
    n_gates = head["n_gates"]
    total_states = B * size * a.steps
    elapsed = head["elapsed"]
    hs = summarize(head, True)
    roofline = roofline_of(head, True, None if a.no_fusion else f"k_tile2:n{n}:dense", prefer="k_tile2")
    # Round 5: the step is two passes (first tile on the top positions, then ONE measuring pass that applies the
    # rest) instead of three: half the bytes, two thirds of the time -- and the measuring pass sits between HBM and
    # the vector unit.  Both sides per pass, and the time-weighted verdict, beside the bytes-moved figure above
    # (`roofline.bound` stays the contract's field for `achieved` / `peak`: bytes moved against HBM).
    try:
        rows = pass_table(head, True)
        top_bound, share = bound_of(rows)
        roofline["per_pass_both_sides"] = rows
        roofline["time_share_by_bound"] = share
        roofline["nearest_bound_by_time"] = top_bound
        roofline["valu"] = valu_roofline(head, True)
        roofline["overlap_note"] = ("two chunks of 32 states are in flight, one stage apart, on two internal streams (the fill of one "
                                    "beside the measuring pass of the other): avg_launch_ms / achieved / frac above are live HIP-event "
                                    "figures of launches that share the card; `isolated_launch` (--full) has the same kernel alone, "
                                    "step_moved_frac_of_8TBps the bytes of the whole step over its wall-clock")
        roofline["counters_note"] = ("SQ counters of the same plan (profiles/r05_k2_headline_sq.txt): the measuring k_tile2 pass "
                                     "issues vector instructions 69 % of its cycles (81 % of them the packed FMAs of its 11 dense "
                                     "2x2 gates), LDS 35 % busy with 20 % bank conflicts: nearer the vector unit than HBM, whatever "
                                     "the nominal-flops fraction above says; the initialising pass is a 6.4 TB/s fill")
    except Exception as e:  # pragma: no cover
        roofline["per_pass_both_sides"] = {"error": repr(e)}
    result = {
        "metric": "gate_applies_per_s", "value": round(n_gates * total_states / elapsed, 1),
        "unit": "gate-applies/s",
        "n_gpus": size, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(elapsed / a.steps * 1e3, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "complex64", "data": "synthetic",
        "config": {"workload": f"K2 all-live: Model({n}, 1, Hardware_Efficient, data_reupload=False) "
                               f"expval on all wires, {n_gates} gates/state (72 1q + 24 CX at n=24) "
                               f"ALL applied to the state, every amplitude read/computed/stored in "
                               f"every pass after the |0..0> initialisation (whose one non-zero tile per state "
                               f"the plan places where it saves a pass) (QMLE_PLAN_NO_SPARSE | "
                               f"QMLE_PLAN_NO_ABSORB), batch {B} statevectors per GPU per step",
                   "n_qubits": n, "batch_per_gpu": B, "gates_per_state": n_gates,
                   "gates_applied_to_the_state": n_gates - head["folded"],
                   "operators_executed_per_state": head["desc"]["n_lowered"],
                   "hbm_passes_per_state": hs["hbm_passes_per_state"], "fusion": not a.no_fusion,
                   "known_zero_tracking": False, "observable_folding": False,
                   "parallelism": f"batch-sharded x{size}"},
        **books,
        "elapsed_s_per_rank_min_max": [round(min(head["elapsed_per_rank"]), 6),
                                       round(max(head["elapsed_per_rank"]), 6)],
        "statevectors_per_s": round(total_states / elapsed, 2),
        "hbm_bytes_moved_per_state": hs["hbm_bytes_moved_per_state"],
        "step_moved_GBps": hs["moved_GBps"], "step_moved_GBps_per_gpu": hs["moved_GBps_per_gpu"],
        "step_moved_frac_of_8TBps": hs["moved_frac_of_8TBps"],
        "roofline": roofline,
        "full": a.full,
    }
    if dumped is not None:
        result["dumped_outputs"] = {"dir": a.dump_outputs, "shapes": dumped}
    if c3 is not None:
        result["c3_expressibility_12q_1024pairs"] = c3
        result["c4_fourier_10q_6l_4096grid"] = c4
        result["c3_saturated_weak"] = c3s
        result["c4_saturated_weak"] = c4s
    if aux and size == 1 and not a.no_fusion:
        # SURVEY 8-d `achieved_unfused`: one HBM pass per reference gate, no 1-qubit merging
        try:
            uf = k2_unfused_leg(n, min(B, 128))
            out_uf = uf.pop("_out")
            uf["max_abs_diff_vs_headline_expvals"] = float((out_uf - head["out"][:out_uf.shape[0]]).abs().max())
            result["k2_unfused"] = uf
            del out_uf
        except Exception as e:  # pragma: no cover
            result["k2_unfused"] = {"error": str(e)}
        # the same all-live step after the product's opt-in plan autotuner (qmle_plan_autotune: the cost model's best
        # schedules x the last stage's paddings timed on this device, the fastest kept -- the headline above is the
        # model's own choice, untuned)
        try:
            N.set_autotune(True)
            try:
                tn = timed_k2(n, B, size, 5, 2, head_flags)
            finally:
                N.set_autotune(False)
            ts = summarize(tn, True)
            result["k2_autotuned"] = {
                "ms_per_step": ts["ms_per_step"], "gate_applies_per_s": ts["gate_applies_per_s"],
                "moved_frac_of_8TBps": ts["moved_frac_of_8TBps"], "candidate": tn["desc"].get("candidate"),
                "autotuned": tn["desc"].get("autotuned"),
                "per_pass": [{k: p_[k] for k in ("pass", "avg_launch_ms", "moved_GBps")} for p_ in per_pass(tn, True)],
                "last_stage_bits": tn["desc"]["stages"][-1]["bits"],
                "max_abs_diff_vs_headline_expvals": float((tn["out"] - head["out"]).abs().max()),
                "note": "QMLE_AUTOTUNE / set_autotune(True): opt-in, one-off timing of the candidates on the first run of a "
                        "plan; the headline does not use it"}
            del tn
        except Exception as e:  # pragma: no cover
            result["k2_autotuned"] = {"error": repr(e)}
        # the same step with its chunks on ONE stream (QMLE_NO_CHUNK_OVERLAP=1, read per call): the kernels' launch
        # durations in isolation -- in the headline two chunks are in flight one stage apart, so a launch shares the card
        # with the other chunk's pass and its HIP-event duration is longer than the kernel needs alone
        try:
            os.environ["QMLE_NO_CHUNK_OVERLAP"] = "1"
            try:
                t1 = timed_k2(n, B, size, 5, 2, head_flags)
            finally:
                os.environ.pop("QMLE_NO_CHUNK_OVERLAP", None)
            s1 = summarize(t1, True)
            r1 = roofline_of(t1, True, None, prefer="k_tile2")
            result["k2_one_stream"] = {
                "ms_per_step": s1["ms_per_step"], "gate_applies_per_s": s1["gate_applies_per_s"],
                "moved_frac_of_8TBps": s1["moved_frac_of_8TBps"],
                "roofline": {k: r1[k] for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "avg_launch_ms")},
                "per_pass": [{k: p_[k] for k in ("pass", "avg_launch_ms", "moved_GBps")} for p_ in per_pass(t1, True)],
                "max_abs_diff_vs_headline_expvals": float((t1["out"] - head["out"]).abs().max()),
                "note": "QMLE_NO_CHUNK_OVERLAP=1: chunks one after the other on the caller's stream (rounds 1-4)"}
            roofline["isolated_launch"] = {"avg_launch_ms": r1["avg_launch_ms"], "achieved": r1["achieved"], "frac": r1["frac"],
                                           "note": "the dominant kernel's launches with nothing else on the card (k2_one_stream)"}
            del t1
        except Exception as e:  # pragma: no cover
            result["k2_one_stream"] = {"error": repr(e)}
        # the round-3/4 schedule of the same step (first tile on the LOW positions: initialising pass, read+write
        # pass, measuring pass -- QMLE_NO_TOP_FIRST=1, read per compile): what BENCH_r03 / r04 measured, kept as a
        # companion so that the two-pass headline can be read against it (more bytes at a higher HBM fraction)
        try:
            from qml_essentials_amd import simulation as _sim

            os.environ["QMLE_NO_TOP_FIRST"] = "1"
            os.environ["QMLE_NO_CHUNK_OVERLAP"] = "1"
            _sim.clear_plan_cache()
            try:
                tp = timed_k2(n, B, size, 5, 2, head_flags)
            finally:
                os.environ.pop("QMLE_NO_TOP_FIRST", None)
                os.environ.pop("QMLE_NO_CHUNK_OVERLAP", None)
                _sim.clear_plan_cache()
            t3 = summarize(tp, True)
            r3 = roofline_of(tp, True, None)
            result["k2_three_pass"] = {
                "ms_per_step": t3["ms_per_step"], "gate_applies_per_s": t3["gate_applies_per_s"],
                "hbm_passes_per_state": t3["hbm_passes_per_state"], "moved_frac_of_8TBps": t3["moved_frac_of_8TBps"],
                "candidate": tp["desc"].get("candidate"),
                "roofline": {k: r3[k] for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "avg_launch_ms")},
                "per_pass": [{k: p_[k] for k in ("pass", "avg_launch_ms", "moved_GBps")} for p_ in per_pass(tp, True)],
                "max_abs_diff_vs_headline_expvals": float((tp["out"] - head["out"]).abs().max()),
                "note": "QMLE_NO_TOP_FIRST=1 QMLE_NO_CHUNK_OVERLAP=1: the schedule the cost model picked before round 5's top-first candidates, chunks on one stream -- the step as rounds 3-4 ran it"}
            del tp
        except Exception as e:  # pragma: no cover
            result["k2_three_pass"] = {"error": repr(e)}
        # the default engine on the same workload: exact, but specific to what a one-layer circuit
        # from |0..0> leaves untouched (known zeros never read / computed / stored, trailing CX layer
        # folded into Z-parity observables) -- NOT a throughput figure for gate application
        sc = timed_k2(n, B, size, a.steps, a.warmup, 0, isolate_passes=True)
        s2 = summarize(sc, False)
        s2["roofline"] = {k: v for k, v in roofline_of(sc, False, None).items()
                          if k in ("kernel", "achieved", "frac", "algorithmic_GBps", "fusion_factor", "avg_launch_ms")}
        s2["gates_folded_into_observables"] = sc["folded"]
        s2["max_abs_diff_vs_headline_expvals"] = float((sc["out"] - head["out"]).abs().max())
        s2["note"] = ("default plan flags: known-zero tracking + observable folding; counts all "
                      f"{n_gates} reference gates although {sc['folded']} act on the observables and most "
                      "amplitudes are never touched")
        result["exact_shortcuts"] = s2
        del sc
        # SURVEY 8-d K2, second tape: Circuit_19 (48 one-qubit + 24 CRX), all amplitudes live
        try:
            c19, run19 = k2_circuit19_leg(n, B, size, 5, 2)
            from oracle import c_port, circuits as OC  # the checker: a few rows against the C port

            spec19 = OC.ModelSpec(n, 1, "Circuit_19", data_reupload=False)
            rows19 = run19["out"][:3].cpu().numpy()
            worst19 = 0.0
            for k in range(3):
                psi = c_port.simulate(OC.model_tape(spec19, run19["params"][k], [0.0]), n)
                worst19 = max(worst19, float(np.abs(c_port.expval_z(psi, n, list(range(n))) - rows19[k]).max()))
            if worst19 > 1e-5:
                raise SystemExit(f"bench.py: Circuit_19 GPU <Z> differs from the CPU oracle port by {worst19:.3e}")
            c19["max_abs_diff_vs_cpu_port_expvals_3_rows"] = worst19
            result["k2_circuit19"] = c19
            del run19
        except SystemExit:
            raise
        except Exception as e:  # pragma: no cover
            result["k2_circuit19"] = {"error": repr(e)}
        # a deeper circuit: 4 layers with data re-uploading = 5 ansatz + 4 encoding layers
        try:
            deep = {}
            for label, fl in (("all_live", DENSE), ("default_flags", 0)):
                d = timed_k2(n, B, size, 3, 1, fl, layers=4, dru=True, x=0.5, isolate_passes=True)
                deep[label] = summarize(d, fl != 0)
                deep[label]["operators_executed_per_state"] = d["desc"]["n_lowered"]
                rf = roofline_of(d, fl != 0, None)
                rows = pass_table(d, fl != 0)
                top, share = bound_of(rows)
                deep[label]["roofline"] = {k: v for k, v in rf.items()
                                           if k in ("kernel", "achieved", "peak", "unit", "frac", "algorithmic_GBps",
                                                    "fusion_factor", "avg_launch_ms", "launches", "kernel_share_of_step")}
                # what limits the step: time share of its passes by the resource each is nearer to
                deep[label]["roofline"]["bound"] = top
                deep[label]["roofline"]["time_share_by_bound"] = share
                deep[label]["roofline"]["valu"] = valu_roofline(d, fl != 0)
                deep[label]["per_pass"] = rows
                del d
            deep["workload"] = (f"Model({n}, 4, Hardware_Efficient) with data re-uploading, input 0.5: "
                                f"{deep['all_live']['gates_counted_per_state']} gates/state, batch {B}, 3 timed steps")
            result["k2_deep"] = deep
        except Exception as e:  # pragma: no cover
            result["k2_deep"] = {"error": str(e)}
    if aux and size == 1:
        gpu_rows = head["out"][:64].cpu().numpy()
        result["cpu_baseline"] = cpu_baseline(n, head["params"][:64], a.cpu_seconds, gpu_rows)
        try:
            result["cpu_baseline"]["other_legs"] = cpu_einsum_legs(n, head["params"][0])
        except Exception as e:  # pragma: no cover
            result["cpu_baseline"]["other_legs"] = {"error": str(e)}
        del head
        torch.cuda.empty_cache()
        # BASELINE configs 3 / 4 on the host's CPU (bounded sample of the same loops) + parity
        try:
            cpu_loops = sampling_loops_cpu()
            if c3 is not None:
                c3["cpu_baseline"] = cpu_loops["c3"]
            if c4 is not None:
                c4["cpu_baseline"] = cpu_loops["c4"]
        except SystemExit:
            raise
        except Exception as e:  # pragma: no cover
            result["sampling_loops_cpu_error"] = str(e)
        # BASELINE config 2 (n = 20: the L2 / Infinity-Cache regime)
        try:
            result["c2_model_20q_4l"] = c2_leg()
        except SystemExit:
            raise
        except Exception as e:  # pragma: no cover
            result["c2_model_20q_4l"] = {"error": repr(e)}
        # LDS-resident regime (n <= 14 is bound by LDS / fp32 VALU, not by HBM)
        try:
            result["lds_regime"] = {
                "c3_states_12q": lds_regime_leg(12, 3, False, 2048, "state"),
                "c3_states_12q_saturated": lds_regime_leg(12, 3, False, 32768, "state"),
                "c4_expval_10q": lds_regime_leg(10, 6, True, 4096, "expval"),
                "c4_expval_10q_saturated": lds_regime_leg(10, 6, True, 65536, "expval"),
            }
        except Exception as e:  # pragma: no cover
            result["lds_regime"] = {"error": str(e)}
        for key, fn in (("k1_single_gate_28q", k1_sweep), ("mw_28q", mw_28q_leg),
                        ("adjoint_gradient_20q", adjoint_gradient_wallclock), ("widened_rows", widened_rows_leg)):
            try:
                result[key] = fn()
            except Exception as e:  # pragma: no cover - e.g. not enough free HBM
                result[key] = {"error": str(e)}
        if isinstance(result.get("mw_28q"), dict) and "error" not in result["mw_28q"]:
            try:
                result["mw_28q"]["cpu_baseline"] = mw_cpu_baseline()
            except SystemExit:
                raise
            except Exception as e:  # pragma: no cover
                result["mw_28q"]["cpu_baseline"] = {"error": str(e)}
    result["summary"] = summary_of(result)  # LAST key: a compact trailer the tail of the line always shows
    distributed.barrier()
    print(json.dumps(result), flush=True)


def summary_of(r):
    """Compact trailer (the LAST key of the line, < 4 KB): one figure per leg, so that a record which keeps only
    the tail of stdout still shows every leg's number.  Every entry repeats a value that sits in full under the
    key of the same name earlier in the line."""
    def g(d, *path, default=None):
        for k in path:
            if not isinstance(d, dict) or k not in d:
                return default
            d = d[k]
        return d

    out = {"k2_headline": {"ms_per_step": r.get("ms_per_step"), "gate_applies_per_s": r.get("value"),
                           "frac": g(r, "roofline", "frac"), "kernel": g(r, "roofline", "kernel"),
                           "per_pass_ms": [p["avg_launch_ms"] for p in g(r, "roofline", "per_pass", default=[])]}}
    out["k2_headline"]["time_share_by_bound"] = g(r, "roofline", "time_share_by_bound")
    out["k2_headline"]["valu_frac"] = g(r, "roofline", "valu", "frac")
    out["k2_headline"]["step_moved_frac"] = r.get("step_moved_frac_of_8TBps")
    if isinstance(r.get("k2_autotuned"), dict):
        out["k2_autotuned"] = {"ms_per_step": g(r, "k2_autotuned", "ms_per_step"), "error": g(r, "k2_autotuned", "error")}
    if isinstance(r.get("k2_one_stream"), dict):
        out["k2_one_stream"] = {"ms_per_step": g(r, "k2_one_stream", "ms_per_step"), "frac": g(r, "k2_one_stream", "roofline", "frac"),
                                "error": g(r, "k2_one_stream", "error")}
    if isinstance(r.get("k2_three_pass"), dict):
        out["k2_three_pass"] = {"ms_per_step": g(r, "k2_three_pass", "ms_per_step"), "frac": g(r, "k2_three_pass", "roofline", "frac"),
                                "error": g(r, "k2_three_pass", "error")}
    for key in ("k2_unfused", "k2_circuit19"):
        if isinstance(r.get(key), dict):
            out[key] = {"ms_per_step": g(r, key, "ms_per_step"), "frac": g(r, key, "roofline", "frac"),
                        "kernel": g(r, key, "roofline", "kernel"), "error": g(r, key, "error")}
    for lab in ("all_live", "default_flags"):
        if isinstance(g(r, "k2_deep", lab), dict):
            out["k2_deep_" + lab] = {"ms_per_step": g(r, "k2_deep", lab, "ms_per_step"),
                                     "frac": g(r, "k2_deep", lab, "roofline", "frac"),
                                     "bound": g(r, "k2_deep", lab, "roofline", "bound"),
                                     "valu_frac": g(r, "k2_deep", lab, "roofline", "valu", "frac"),
                                     "time_share_by_bound": g(r, "k2_deep", lab, "roofline", "time_share_by_bound")}
    c2 = r.get("c2_model_20q_4l")
    if isinstance(c2, dict):
        out["c2_model_20q_4l"] = {lab: {"ms_per_step": g(c2, lab, "ms_per_step"), "kernel_ms": g(c2, lab, "kernel_ms_per_step"),
                                       "frac_hbm": g(c2, lab, "roofline", "frac"), "frac_l2": g(c2, lab, "roofline", "frac_of_l2"),
                                       "valu_frac": g(c2, lab, "roofline", "valu", "frac"),
                                       "bound": g(c2, lab, "roofline", "bound")}
                                 for lab in ("single_sample", "batch_256", "batch_1024", "batch_1024_all_live") if lab in c2}
        out["c2_model_20q_4l"]["cpu_ms_per_state"] = g(c2, "cpu_baseline", "ms_per_state")
        out["c2_model_20q_4l"]["cpu_cores"] = g(c2, "cpu_baseline", "cores")
        out["c2_model_20q_4l"]["error"] = c2.get("error")
    for key in ("c3_expressibility_12q_1024pairs", "c4_fourier_10q_6l_4096grid", "c3_saturated_weak", "c4_saturated_weak"):
        if isinstance(r.get(key), dict):
            out[key] = {"seconds": g(r, key, "seconds"), "gpu_ms": g(r, key, "gpu_ms"), "collective_ms": g(r, key, "collective_ms"),
                        "cpu_seconds": g(r, key, "cpu_baseline", "seconds_full_loop_extrapolated")}
    lds = r.get("lds_regime")
    if isinstance(lds, dict):
        out["lds_regime"] = {k: {"frac_of_valu_peak": v.get("frac_of_valu_peak"), "states_per_s": v.get("states_per_s"),
                                 "kernel_ms": v.get("kernel_ms")} if isinstance(v, dict) else v for k, v in lds.items()}
    k1 = r.get("k1_single_gate_28q")
    if isinstance(k1, dict):
        out["k1_single_gate_28q"] = {gname: {"frac_min_mean_max": v.get("frac_of_8TBps_min_mean_max"),
                                             "vs_attainable_min_mean_max": v.get("frac_of_8TBps_vs_attainable_min_mean_max"),
                                             "wires_ge_0.70_of_attainable": v.get("target_wires_at_0.70_or_more_of_attainable")}
                                     if isinstance(v, dict) else v for gname, v in k1.items()}
    mw = r.get("mw_28q")
    if isinstance(mw, dict):
        out["mw_28q"] = {"ms": mw.get("ms"), "frac": g(mw, "roofline", "frac"), "moved_frac": g(mw, "roofline", "moved_frac"),
                         "traffic": g(mw, "roofline", "traffic"), "fused_ms": mw.get("fused_ms"), "fused_frac": g(mw, "fused_roofline", "frac"),
                         "fused_traffic": g(mw, "fused_roofline", "traffic"), "stand_alone_after_circuit_ms": mw.get("after_circuit_ms_stand_alone_reads"),
                         "bound": g(mw, "roofline", "bound"), "error": mw.get("error")}
    out["adjoint_gradient_20q_ms"] = g(r, "adjoint_gradient_20q", "ms")
    if isinstance(r.get("widened_rows"), dict):
        out["widened_rows"] = {k: v for k, v in r["widened_rows"].items() if k.endswith("_ms") or k == "error"}
    out["cpu_baseline_gate_applies_per_s"] = g(r, "cpu_baseline", "value")
    return out


if __name__ == "__main__":
    main()
