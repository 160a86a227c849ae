#!/usr/bin/env python3
"""Device time of the reference's ``resize_image`` (pcdms_amd.pose.resize_image -> preprocess.resize_cv, one launch of pcdm_resize_cv_u8) for the
two frames the pose chain makes: one 1101 x 750 picture -> its 512 detection frame (768 x 512, area resampling) and one 256 x 176 picture -> 512
(768 x 512, Lanczos4).  ``preprocess.resize`` (Pillow bicubic, the default frame) runs at the same sizes on the same device, the two alternating
inside every repetition: HIP events around ``--iters`` back-to-back calls on an input that stays on the device (tables cached), the median of
``--reps`` such windows after ``--warmup`` unmeasured calls.  Recorded, not gated.  Prints one JSON line; ``--out`` writes it as well.

    python tools/bench_resize_cv.py --out profiles/resize_cv_bench.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import pcdms_amd as P  # noqa: E402


def window(call, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    result = {"what": "HIP-event microseconds per detection frame (tools/bench_resize_cv.py); median of %d x %d calls, resize_image and Pillow "
                      "bicubic alternating" % (args.reps, args.iters),
              "device": torch.cuda.get_device_name(0), "us_per_frame": {}}
    for H, W in ((1101, 750), (256, 176)):
        img = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
        Hd, Wd = P.detect_size(H, W, 512)
        calls = {"resize_image": lambda: P.resize_image(img, 512), "pillow_bicubic": lambda: P.resize(img, (Wd, Hd))}
        for call in calls.values():
            for _ in range(args.warmup):
                call()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, call in calls.items():
                times[k].append(window(call, args.iters))
        rule = "lanczos4" if 512 / min(H, W) > 1 else "area"
        result["us_per_frame"][f"{H}x{W}->{Hd}x{Wd}"] = {"rule": rule, **{k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                                                                             "max": round(max(v), 2)} for k, v in times.items()}}
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
