"""Time the film grain entries on the device for one 4K picture with grain on
every plane: dav1d_gpu_apply_grain_* (prep + every strip), and the split
entries on their own, dav1d_gpu_prep_grain_* and
dav1d_gpu_apply_grain_rows_*(0, rows).

Each figure is HIP events around --steps back-to-back calls on one stream,
after a warm-up, repeated --reps times; the variants are interleaved within
every repetition so that drift hits all of them alike.  The line reports the
median, minimum and maximum per call over the repetitions (the spread).

--compare-lib PATH times dav1d_gpu_apply_grain_* of another build of the
library (the parent commit's, say) in the same process and the same
interleave, on the same batch, and checks that both write the same pixels.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bpc", type=int, default=8)
    ap.add_argument("--bdmax", type=int, default=1023)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--compare-lib", default=None)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5 (the spread is part of the result)")
    import numpy as np
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    import dav1d_mirror_amd.grain as grain
    assert torch.cuda.is_available(), "needs a GPU"
    c = grain.make_grain_case(seed=5, width=a.width, height=a.height, bpc=a.bpc, bitdepth_max=a.bdmax,
                              lag=3, num_y=8, csfl=False, num_uv=(6, 6), overlap=True)
    dev = grain.DeviceGrain(c)
    s = torch.cuda.current_stream()
    variants = {"apply_grain": lambda: dev.launch(s), "prep_grain": lambda: dev.launch_prep(s),
                "apply_grain_rows": lambda: dev.launch_rows(0, dev.strips, s)}
    same = None
    if a.compare_lib:
        other = ctypes.CDLL(os.path.abspath(a.compare_lib))
        fn = getattr(other, f"dav1d_gpu_apply_grain_{8 if a.bpc == 8 else 16}bpc")
        fn.argtypes = [ctypes.POINTER(pkg.abi.FilmGrainBatch), ctypes.c_void_p]
        fn.restype = ctypes.c_int

        def launch_other():
            rc = fn(ctypes.byref(dev.batch), ctypes.c_void_p(s.cuda_stream))
            assert rc == 0, rc
        variants["apply_grain_compare_lib"] = launch_other
        dev.launch(s)
        torch.cuda.synchronize()
        mine = [t.clone() for t in dev.outs]
        for t in dev.outs:
            t.zero_()
        launch_other()
        torch.cuda.synchronize()
        same = all(bool(torch.equal(x, y)) for x, y in zip(mine, dev.outs))
    for f in variants.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.reps):
        for k, f in variants.items():
            e0.record(s)
            for _ in range(a.steps):
                f()
            e1.record(s)
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / a.steps)
    outs, _, _ = ge.load_oracle().apply_grain(c)
    dev.launch(s)
    torch.cuda.synchronize()
    res = {"frame": f"{a.width}x{a.height}", "bpc": a.bpc, "steps": a.steps, "reps": a.reps,
           "bit_exact": all(bool(np.array_equal(x, y)) for x, y in zip(dev.outputs_host(), outs)),
           "us_per_call": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                               "max": round(max(v), 2)} for k, v in us.items()}}
    if same is not None:
        res["compare_lib_same_pixels"] = same
    print(json.dumps(res))


if __name__ == "__main__":
    main()
