"""bench.py's command line on the GPU: a plain run prints the headline line alone and --dump-outputs writes the last
timed frame; --full adds the per-pass, roofline and CPU-baseline figures (checked by the --full runs of
test_gpu_distributed.py and tools/gpu.sh)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ("roofline", "ms_per_pass", "ms_per_group", "ms_per_group_unfused", "gbs_per_pass", "cpu_baseline")


def test_plain_run_headline_and_dump(tmp_path):
    W, H, steps = 320, 180, 3
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
           "--width", str(W), "--height", str(H), "--dump-outputs", str(dump)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), p.stdout
    out = json.loads(lines[0])
    assert out["unit"] == "frames/sec" and out["higher_is_better"] is True and out["steps"] == steps
    assert out["value"] > 0 and out["ms_per_step"] > 0
    # one GPU: value is frames per second of the timed steps, ms_per_step the time of one of them
    assert abs(out["value"] * out["ms_per_step"] - 1e3) < 1.0
    assert out["full"] is False and not any(k in out for k in FULL_ONLY)
    files = sorted(f.name for f in dump.iterdir())
    assert files == ["color.npy", "exposure.npy", "output.npy", "resolved.npy"]
    arrays = {f[:-4]: np.load(dump / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for n in ("output", "color", "resolved"):
        assert arrays[n].shape == (W * H, 4)
    # a rendered frame: 8-bit framebuffer values that vary over the image, finite HDR colour and exposure
    assert arrays["output"].min() >= 0 and arrays["output"].max() <= 255 and arrays["output"][:, :3].std() > 1.0
    assert np.isfinite(arrays["color"]).all() and arrays["color"][:, :3].max() > 0
    assert np.isfinite(arrays["resolved"]).all() and arrays["exposure"].shape == (1,) and np.isfinite(arrays["exposure"]).all()
