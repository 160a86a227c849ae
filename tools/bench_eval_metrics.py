#!/usr/bin/env python3
"""The kernels of tools/calculate_metrics.py at the paper's two evaluation sizes (750 x 1101 sources -> 176 x 256 and -> 352 x 512), N = 16:
the OpenCV-cubic resize of a batch (16 launches of ``preprocess.resize_cv_cubic``), ``metrics.l1`` + ``metrics.mae`` and
``metrics.ssim_box(win_size=51)``, each against a torch restatement of the same arithmetic on the same device.  Every shape is warmed up first;
a timed window is ``--iters`` back-to-back calls between two HIP events, the two versions alternate, and the medians over ``--reps`` windows
are reported with their minimum and maximum.  Nobody has measured these before: the numbers are recorded, no threshold is set.  Prints one JSON
line; ``--out`` writes it to a file as well.

    python tools/bench_eval_metrics.py --out profiles/eval_metrics_bench.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pcdms_amd import metrics, preprocess  # noqa: E402


def _axis(n_in, n_out, dev):
    """(clamped tap indices int64 [n_out, 4], fp32 coefficients [n_out, 4]) of one axis, as include/pcdm.h: pcdm_resize_cubic_f32 states them"""
    scale = 1.0 / (float(n_out) / float(n_in))
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    t = f - s
    A, one = np.float32(-0.75), np.float32(1)
    t1, t2 = t + one, one - t
    c0 = ((A * t1 - np.float32(5) * A) * t1 + np.float32(8) * A) * t1 - np.float32(4) * A
    c1 = ((A + np.float32(2)) * t - (A + np.float32(3))) * t * t + one
    c2 = ((A + np.float32(2)) * t2 - (A + np.float32(3))) * t2 * t2 + one
    c = np.stack([c0, c1, c2, one - c0 - c1 - c2], axis=1)
    idx = np.clip(s.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return torch.from_numpy(idx).to(dev), torch.from_numpy(c).to(dev)


def torch_resize(src_u8, tabs, out):
    """the same two passes with torch gathers in fp32: src uint8 [N, Hs, Ws, 3] -> out fp32 [N, Hd, Wd, 3] / 255"""
    (ix, cx), (iy, cy) = tabs
    a = src_u8.float()
    h = a[:, :, ix[:, 0]] * cx[:, 0, None]
    for k in range(1, 4):
        h = h + a[:, :, ix[:, k]] * cx[:, k, None]
    v = h[:, iy[:, 0]] * cy[:, 0, None, None]
    for k in range(1, 4):
        v = v + h[:, iy[:, k]] * cy[:, k, None, None]
    return torch.div(v, 255.0, out=out)


def torch_absdiff(a, b):
    d, s = (a - b).abs().double().sum((1, 2, 3)), (a + b).double().sum((1, 2, 3))
    return (d / (a[0].numel())).float(), (d / s).float()


def torch_ssim_box(cand, ref, w=51, R=1.0):
    """fp64 mean filters through avg_pool2d (stride 1: the interior only), sample covariance"""
    x, y = cand.permute(0, 3, 1, 2).double(), ref.permute(0, 3, 1, 2).double()
    c1, c2, cn = (0.01 * R) ** 2, (0.03 * R) ** 2, w * w / (w * w - 1.0)
    ux, uy = F.avg_pool2d(x, w, 1), F.avg_pool2d(y, w, 1)
    vx, vy, vxy = cn * (F.avg_pool2d(x * x, w, 1) - ux * ux), cn * (F.avg_pool2d(y * y, w, 1) - uy * uy), cn * (F.avg_pool2d(x * y, w, 1) - ux * uy)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    return s.mean((1, 2, 3)).float()


def window_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def compare(ours, theirs, iters, reps, warmup):
    for _ in range(warmup):
        ours()
        theirs()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):
        a.append(window_ms(ours, iters))
        b.append(window_ms(theirs, iters))
    med = statistics.median
    return {"hip_ms": round(med(a), 4), "hip_ms_min_max": [round(min(a), 4), round(max(a), 4)], "torch_ms": round(med(b), 4),
            "torch_ms_min_max": [round(min(b), 4), round(max(b), 4)], "torch_over_hip": round(med(b) / med(a), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--src", type=int, nargs=2, default=(750, 1101), help="width height of the decoded images")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, (Ws, Hs) = args.n, args.src
    g = torch.Generator(device="cpu").manual_seed(0)
    base = torch.randint(0, 256, (Hs, Ws, 3), generator=g, dtype=torch.int16)
    gen_u8 = torch.stack([(base + torch.randint(-20, 21, base.shape, generator=g, dtype=torch.int16)).clamp(0, 255) for _ in range(N)]).to(torch.uint8).to(dev)
    gt_u8 = torch.stack([(base + torch.randint(-5, 6, base.shape, generator=g, dtype=torch.int16)).clamp(0, 255) for _ in range(N)]).to(torch.uint8).to(dev)
    result = {"source": [Ws, Hs], "n": N, "reps": args.reps, "iters_per_window": args.iters, "device_name": torch.cuda.get_device_name(0),
              "timing": "HIP events around back-to-back calls, medians over the windows, the two versions alternating", "sizes": {}}
    for W, H in ((176, 256), (352, 512)):
        pred, gt = torch.empty((N, H, W, 3), device=dev), torch.empty((N, H, W, 3), device=dev)
        tpred = torch.empty_like(pred)
        tabs = (_axis(Ws, W, dev), _axis(Hs, H, dev))

        def hip_resize(src=gen_u8, out=pred):
            for i in range(N):
                preprocess.resize_cv_cubic(src[i], (W, H), divisor=255.0, out=out, index=i)
        hip_resize()
        hip_resize(gt_u8, gt)
        torch_resize(gen_u8, tabs, tpred)
        torch.cuda.synchronize()
        entry = {"resize_vs_torch_max_abs_diff": float((pred - tpred).abs().max())}
        entry["resize_batch"] = compare(hip_resize, lambda: torch_resize(gen_u8, tabs, tpred), args.iters, args.reps, args.warmup)
        l1, mae, (tl1, tmae) = metrics.l1(pred, gt), metrics.mae(pred, gt), torch_absdiff(pred, gt)
        entry["l1_mae_vs_torch_max_rel_diff"] = float(max(((l1 - tl1).abs() / tl1).max(), ((mae - tmae).abs() / tmae).max()))
        entry["l1_mae"] = compare(lambda: (metrics.l1(pred, gt), metrics.mae(pred, gt)), lambda: torch_absdiff(pred, gt), args.iters, args.reps,
                                  args.warmup)
        sb, tsb = metrics.ssim_box(pred, gt, win_size=51, data_range=1.0), torch_ssim_box(pred, gt)
        entry["ssim_box_vs_torch_max_abs_diff"] = float((sb - tsb).abs().max())
        entry["ssim_box_51"] = compare(lambda: metrics.ssim_box(pred, gt, win_size=51, data_range=1.0), lambda: torch_ssim_box(pred, gt), args.iters,
                                       args.reps, args.warmup)
        result["sizes"][f"{W}x{H}"] = entry
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
