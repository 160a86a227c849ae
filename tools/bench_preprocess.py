#!/usr/bin/env python3
"""Per-pair input preparation of the stage-2 driver: the host path (four PIL bicubic resizes, two canvases, two ``to_tensor_normalized``, one
``CLIPImageProcessor()`` call, three copies to the device) against the device path (four uploads of the raw uint8 pixels, then
``pcdms_amd.preprocess``), from the same decoded images, in one process, interleaved, medians of wall time with a device synchronisation at
the end of each.  Also the HIP-event time of the kernels alone.  Prints one JSON line; ``--out`` writes it to a file as well.

    python tools/bench_preprocess.py --reps 30 --out profiles/preprocess_bench.json
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch
from PIL import Image

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import pcdms_amd as P  # noqa: E402


def _driver():
    spec = importlib.util.spec_from_file_location("stage2_driver", ROOT / "tools" / "stage2_batchtest_inpaint_model.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--src", type=int, nargs=2, default=(750, 1101), help="width height of the decoded images")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from transformers import CLIPImageProcessor
    drv, proc, dev = _driver(), CLIPImageProcessor(), torch.device("cuda:0")
    rng = np.random.default_rng(0)
    ws, hs = args.src
    raws = [rng.integers(0, 256, (hs, ws, 3), dtype=np.uint8) for _ in range(4)]     # source, target, source pose, target pose

    def host(W, H):
        s_img, t_img, s_pose, t_pose = (Image.fromarray(a).resize((W, H), Image.BICUBIC) for a in raws)
        a = Image.new("RGB", (2 * W, H))
        a.paste(s_img, (0, 0))
        b = Image.new("RGB", (2 * W, H))
        b.paste(s_pose, (0, 0))
        b.paste(t_pose, (W, 0))
        pix = proc(images=s_img, return_tensors="pt").pixel_values
        out = pix.to(dev), drv.to_tensor_normalized(a).unsqueeze(0).to(dev), drv.to_tensor_normalized(b).unsqueeze(0).to(dev)
        torch.cuda.synchronize()
        return out

    def device(W, H):
        s, t, sp, tp = (torch.from_numpy(a).to(dev) for a in raws)
        vae_image, st_pose, s_u8 = P.stage2_inputs(s, sp, tp, W, H)
        t_u8 = P.resize(t, (W, H))
        out = P.clip_pixel_values(s_u8), vae_image, st_pose, t_u8
        torch.cuda.synchronize()
        return out

    def kernels(W, H):
        """HIP-event time of the device path without the uploads, and of one source resize alone"""
        s, t, sp, tp = (torch.from_numpy(a).to(dev) for a in raws)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        P.resize(s, (W, H))
        ev[1].record()
        _, _, s_u8 = P.stage2_inputs(s, sp, tp, W, H)
        P.resize(t, (W, H))
        P.clip_pixel_values(s_u8)
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])

    result = {"source": [ws, hs], "reps": args.reps, "device_name": torch.cuda.get_device_name(0), "sizes": {}}
    for W, H in ((352, 512), (512, 512)):
        h, d = host(W, H), device(W, H)
        assert torch.equal(h[0], d[0]) and torch.equal(h[1], d[1]) and torch.equal(h[2], d[2]), "device path differs from the host path"
        th, td, k1, ka = [], [], [], []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            host(W, H)
            t1 = time.perf_counter()
            device(W, H)
            t2 = time.perf_counter()
            a, b = kernels(W, H)
            if i >= args.warmup:
                th.append((t1 - t0) * 1e3)
                td.append((t2 - t1) * 1e3)
                k1.append(a)
                ka.append(b)
        med = statistics.median
        result["sizes"][f"{W}x{H}"] = {
            "host_ms": round(med(th), 3), "host_ms_min_max": [round(min(th), 3), round(max(th), 3)],
            "device_ms_with_uploads": round(med(td), 3), "device_ms_min_max": [round(min(td), 3), round(max(td), 3)],
            "device_kernels_ms_hip_events": round(med(ka), 4), "one_source_resize_ms_hip_events": round(med(k1), 4),
            "speedup": round(med(th) / med(td), 2), "outputs_bit_identical": True}
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
