"""``bench.py`` as the checks run it: a plain one-GPU run with ``--dump-outputs`` (and ``--full``)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_result_line_and_dumped_outputs(tmp_path):
    """One result line whose ``ms_per_step`` is the timed span over exactly ``--steps`` steps, and
    the last timed step's outputs on disk: one finite cost per timed step, the update ratios of
    the three weights, the six parameters (fp32; the 4 M-element weights as fixed-size samples),
    at most 64 MB in all. ``--full`` is accepted and (nothing lives behind it) changes no field."""
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "512", "--full", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=240, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["unit"] == "samples/s" and res["higher_is_better"] is True
    assert res["dtype"] == "bf16" and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(512 / (res["ms_per_step"] * 1e-3), rel=1e-3)
    files = {p.name: np.load(p) for p in out.iterdir()}
    assert sorted(files) == ["costs.npy"] + [f"param_{i:02d}.npy" for i in range(6)] + ["weight_upd_ratio.npy"]
    assert sum(os.path.getsize(out / n) for n in files) <= 64 << 20
    assert files["costs.npy"].dtype == np.float64 and files["costs.npy"].shape == (3,)
    assert files["weight_upd_ratio.npy"].shape == (3,) and (files["weight_upd_ratio.npy"] > 0).all()
    assert all(np.isfinite(a).all() for a in files.values())
    cap = (48 << 20) // 4 // 6
    sizes = [1024 * 4096, 4096, 4096 * 4096, 4096, 4096 * 1024, 1024]
    for i, n in enumerate(sizes):
        p = files[f"param_{i:02d}.npy"]
        assert p.dtype == np.float32 and p.shape == (min(n, cap),)
    assert files["param_00.npy"].std() > 0  # weights; the zero-initialised biases have moved too
    assert np.abs(files["param_01.npy"]).max() > 0
