"""CPU-only: `bench.py --gpus N` starts N ranks by itself, the traffic guard
refuses stale PMC records (item 3), and the JSON-line bookkeeping is what the driver parses."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True,
                          env=env, timeout=timeout, cwd=ROOT)


def test_gpus_2_spawns_two_ranks_through_the_launcher():
    """The parent never touches the GPU; it starts torch.distributed.run as a child and relays rank
    0's ONE JSON line.  gloo here (no GPU in this container): on a GPU box the same path runs nccl."""
    p = _run(["--gpus", "2", "--rendezvous-only"], {"QMLE_DIST_BACKEND": "gloo"})
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["ranks_seen"] == [0, 1]
    assert rec["collective_backend"] == "gloo" and rec["launched_by"] == "bench.py"
    assert "torch.distributed.run" in p.stderr and "--nproc-per-node=2" in p.stderr
    # the one collective of every sharded leg timed by itself, on the payload the leg gathers --
    # the strong-scaling legs (C3: 1024 pairs, C4: 4096 x 10 values) and their saturated weak-scaling companions
    legs = rec["scaling_legs"]
    assert set(legs) == {"c3_expressibility_12q_1024pairs", "c4_fourier_10q_6l_4096grid",
                         "c3_saturated_weak", "c4_saturated_weak"}
    assert legs["c3_expressibility_12q_1024pairs"]["rows_per_rank"] == 512
    assert legs["c4_fourier_10q_6l_4096grid"]["payload_bytes_per_rank"] == 2048 * 10 * 4
    assert legs["c3_saturated_weak"]["rows_per_rank"] == 16384 and legs["c4_saturated_weak"]["rows_per_rank"] == 32768
    for leg in legs.values():
        assert leg["collective_ms"] is not None and 0.0 < leg["collective_ms"] < 5000.0


def test_world_size_must_match_gpus():
    """A run whose process group is not --gpus ranks wide exits non-zero instead of printing a
    line with a wrong n_gpus (round 2: `--gpus 8` ran one rank and said n_gpus 1)."""
    p = _run(["--gpus", "3", "--rendezvous-only"], {"WORLD_SIZE": "1", "RANK": "0"})
    assert p.returncode != 0
    assert "--gpus 3" in p.stderr and not p.stdout.strip()


def test_non_nccl_backend_needs_an_explicit_rehearsal_switch():
    p = _run(["--gpus", "2", "--rendezvous-only"])  # no GPU here -> gloo, but nobody asked for it
    assert p.returncode != 0
    assert "needs nccl" in p.stderr


def test_single_rank_bookkeeping():
    p = _run(["--gpus", "1", "--rendezvous-only"])
    assert p.returncode == 0, p.stderr[-2000:]
    rec = json.loads(p.stdout.strip())
    assert rec["n_gpus"] == 1 and rec["ranks_seen"] == [0] and rec["launched_by"] == "python"


def test_stale_traffic_records_are_refused(tmp_path):
    sys.path.insert(0, ROOT)
    import bench

    sha = bench.source_sha16()
    path = tmp_path / "traffic.json"
    path.write_text(json.dumps({
        "fresh": {"hbm_bytes_per_launch": 123, "source": "x", "states_per_launch": 32, "source_sha16": sha},
        "stale": {"hbm_bytes_per_launch": 456, "source": "x", "source_sha16": "0" * 16},
        "unsigned": {"hbm_bytes_per_launch": 789}}))
    assert bench.load_traffic("fresh", str(path)) == (123, "x", 32, None)
    for key in ("stale", "unsigned", "absent"):
        got = bench.load_traffic(key, str(path))
        assert got[0] is None and got[3], (key, got)
    assert "STALE" in bench.load_traffic("stale", str(path))[3]


def test_committed_traffic_file_is_signed():
    """Every record bench.py reads carries the hash of the kernel sources it was collected for
    (the hash may lag behind the tree while kernels are being edited: then bench.py reports
    traffic null + the reason; it never reports stale bytes)."""
    doc = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
    for key in ("k_tile2:n24:dense", "meyer_wallach:n28"):
        assert key in doc, key
        assert len(doc[key].get("source_sha16", "")) == 16, key


def test_plain_run_is_headline_only_and_full_is_opt_in():
    """A plain `bench.py --gpus 1 --steps N --warmup W` times the headline and nothing else; every companion leg
    waits for --full, and --steps / --warmup are taken as given."""
    sys.path.insert(0, ROOT)
    import bench

    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_writes_float_arrays_and_caps_the_size(tmp_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench

    expval = torch.linspace(-1, 1, 1024 * 24).reshape(1024, 24)
    shapes = bench.dump_outputs(str(tmp_path / "a"), {"expval": expval})
    got = np.load(tmp_path / "a" / "expval.npy")
    assert shapes == {"expval": [1024, 24]} and got.dtype == np.float32
    assert np.array_equal(got, expval.numpy())
    x64 = np.arange(12.0).reshape(4, 3)
    bench.dump_outputs(str(tmp_path / "d"), {"x": x64})
    assert np.load(tmp_path / "d" / "x.npy").dtype == np.float64
    # above the cap: a seeded sample of rows, the same rows every time
    cap = 24 * 4 * 100
    shapes = bench.dump_outputs(str(tmp_path / "b"), {"expval": expval}, max_bytes=cap)
    first = np.load(tmp_path / "b" / "expval.npy")
    assert first.nbytes <= cap and shapes == {"expval": list(first.shape)} and first.shape[1] == 24
    bench.dump_outputs(str(tmp_path / "c"), {"expval": expval}, max_bytes=cap)
    assert np.array_equal(first, np.load(tmp_path / "c" / "expval.npy"))
    assert all(any(np.array_equal(r, e) for e in expval.numpy()) for r in first[:5])
