#!/usr/bin/env python3
"""Device time of one pose map (pcdms_amd.pose.draw_pose, P = 1, hands on) at 512 x 512 and 1024 x 1024, without and with the bilinear resize
to an image resolution 1.5 times as large: HIP events around ``--iters`` back-to-back calls on inputs that stay on the device, the median of
``--reps`` such measurements after ``--warmup`` unmeasured calls.  Recorded, not gated.  Prints one JSON line; ``--out`` writes it as well.

    python tools/bench_pose.py --out profiles/pose_bench.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    result = {"what": "HIP-event microseconds per pose map, one person, hands on (tools/bench_pose.py); median of %d x %d calls" % (args.reps, args.iters),
              "device": torch.cuda.get_device_name(0), "us_per_map": {}}
    for side in (512, 1024):
        kp = torch.from_numpy((side * (0.5 + 0.2 * rng.standard_normal((1, 1, 134, 2)))).astype(np.float32)).to(dev)
        sc = torch.full((1, 1, 134), 0.9, device=dev)
        for label, image_size in (("draw", None), ("draw_and_resize", (side * 3 // 2, side * 3 // 2))):
            out = torch.empty((1, *(image_size or (side, side)), 3), dtype=torch.uint8, device=dev)
            call = lambda: P.draw_pose(kp, sc, (side, side), image_size=image_size, out=out)  # noqa: E731
            for _ in range(args.warmup):
                call()
            times = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    call()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) * 1000.0 / args.iters)
            result["us_per_map"][f"{side}x{side}_{label}"] = {"median": round(statistics.median(times), 2), "min": round(min(times), 2),
                                                             "max": round(max(times), 2)}
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
