"""The plain benchmark run on a GPU: headline only, the contract's keys, and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["metric"] == "gate_applies_per_s" and rec["unit"] == "gate-applies/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "complex64"
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["full"] is False and "cpu_baseline" not in rec and "k1_single_gate_28q" not in rec
    expval = np.load(out / "expval.npy")
    assert expval.dtype == np.float32 and expval.shape == (1024, 24)
    assert np.isfinite(expval).all() and np.abs(expval).max() <= 1 + 1e-5
    assert rec["dumped_outputs"]["shapes"] == {"expval": [1024, 24]}
    # the rows are <Z> of the seeded parameter sets: the first and the last against the oracle's C port
    sys.path.insert(0, ROOT)
    from oracle import c_port, circuits as OC
    from qml_essentials_amd.model import Model

    shape = Model(24, 1, "Hardware_Efficient", data_reupload=False).params.shape[1:]
    params = np.random.default_rng(1000).uniform(0, 2 * np.pi, (1024, *shape)).astype(np.float32)
    spec = OC.ModelSpec(24, 1, "Hardware_Efficient", data_reupload=False)
    for k in (0, 1023):
        psi = c_port.simulate(OC.model_tape(spec, params[k], [0.0]), 24)
        assert np.abs(c_port.expval_z(psi, 24, list(range(24))) - expval[k]).max() < 1e-5, k
