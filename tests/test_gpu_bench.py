"""A plain bench.py run on the GPU: the line carries the headline only (no
side legs, no oracle check), --steps sets the timed steps, ms_per_step and
value agree, and --dump-outputs writes the timed frame's planes, which are
the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_LEGS = ("configs", "cold_mall", "families", "tile_batch", "intra_wavefront", "recorder", "film_grain", "cdef",
             "superres", "loop_filter", "loop_restoration", "cpu_baseline")


def test_plain_run_headline_and_dump(pkg, oracle, tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    import dav1d_mirror_amd.workload as wl
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "1080p-mc", "--dump-outputs", str(tmp_path / "out")],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["full"] is False
    assert d["unit"] == "Gpixels/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert not [k for k in SIDE_LEGS if k in d] and "bit_exact_vs_oracle" not in d["config"]
    assert d["ms_per_step"] > 0
    # value is the frame's pixels over the time of one step (both rounded in the line)
    assert d["value"] == pytest.approx(d["config"]["pixels_per_frame"] / (d["ms_per_step"] * 1e-3) / 1e9, rel=2e-3)
    assert d["roofline"]["kernel_us"] <= d["ms_per_step"] * 1e3 * (1 + 1e-3)

    c = dict(bench.CONFIGS["1080p-mc"])
    c.pop("label")
    fd = wl.make_frame(wl.FrameConfig(**c))
    hf = oracle.HostFrame(fd)
    hf.run(threads=4)
    assert sorted(os.listdir(tmp_path / "out")) == ["u.npy", "v.npy", "y.npy"]
    for name, want in zip(("y", "u", "v"), hf.dst):
        got = np.load(tmp_path / "out" / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got, want.astype(np.float32)), name
