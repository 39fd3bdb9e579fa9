"""bench.py --dump-outputs / --full: the options exist, a plain run keeps the
side legs off, and dump_outputs writes the timed frame's planes whole, as
float32, under the names a comparison of two builds expects."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Frame:
    def __init__(self, planes):
        self.planes = planes

    def planes_host(self):
        return self.planes


def test_dump_outputs_writes_float32_planes(tmp_path):
    rng = np.random.default_rng(3)
    for dt, hi in ((np.uint8, 256), (np.uint16, 1024)):
        planes = [rng.integers(0, hi, size=s).astype(dt) for s in ((18, 34), (9, 17), (9, 17))]
        out = tmp_path / f"d{hi}" / "nested"        # created on demand
        bench.dump_outputs(str(out), _Frame(planes))
        assert sorted(os.listdir(out)) == ["u.npy", "v.npy", "y.npy"]
        for name, want in zip(("y", "u", "v"), planes):
            got = np.load(out / f"{name}.npy")
            assert got.dtype == np.float32 and got.shape == want.shape
            assert np.array_equal(got, want.astype(np.float32)) and np.array_equal(got.astype(dt), want)


def test_dump_of_every_config_fits_64mb():
    for c in bench.CONFIGS.values():
        w, h = c["width"], c["height"]
        px = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
        assert px * 4 <= 64 * 1000 * 1000, (c["label"], px * 4)


def test_full_and_dump_options(monkeypatch, capsys):
    """--full is off by default and --steps / --dump-outputs parse; a bad
    step count is an error, not a division by zero later."""
    import pytest
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0", "--dry-run"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code != 0 and "--steps" in capsys.readouterr().err
    monkeypatch.setattr(sys, "argv", ["bench.py", "--help"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--full" in text and "--dump-outputs DIR" in text
