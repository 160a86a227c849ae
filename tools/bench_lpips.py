"""Time the device LPIPS (pcdms_amd.metrics.LPIPS) at N = 4, 512 x 352 against a torch fp32 restatement on the same device, and each of its
five fp32-MFMA convolutions on its own (fraction of the 155 TF/s fp32-MFMA rate).  Synthetic weights; median HIP-event time.

    python tools/bench_lpips.py [--out profiles/lpips_bench.json]
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

CONVS = ((64, 3, 11, 4, 2), (192, 64, 5, 1, 2), (384, 192, 3, 1, 1), (256, 384, 3, 1, 1), (256, 256, 3, 1, 1))
NAMES = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
FP32_MFMA_PEAK = 155e12


def median_us(fn, iters=30, warmup=5):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=352)
    args = ap.parse_args()
    from pcdms_amd import metrics, ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    sd = {}
    for l, (name, (co, ci, k, _, _)) in enumerate(zip(NAMES, CONVS)):
        sd[f"{name}.weight"] = (torch.rand(co, ci, k, k, generator=g) * 2 - 1) / math.sqrt(ci * k * k)
        sd[f"{name}.bias"] = (torch.rand(co, generator=g) * 2 - 1) * 0.1
        sd[f"lin{l}.model.1.weight"] = torch.rand(1, co, 1, 1, generator=g)
    model = metrics.LPIPS().load_state_dict(sd)
    N, H, W = args.n, args.height, args.width
    x0 = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    x1 = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    wd = {k: v.to(dev) for k, v in sd.items()}
    shift = torch.tensor((-.030, -.088, -.188), device=dev).view(1, 3, 1, 1)
    scale = torch.tensor((.458, .448, .450), device=dev).view(1, 3, 1, 1)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False

    def torch_lpips():
        h = torch.cat([x0, x1]).permute(0, 3, 1, 2).float() / 255.0
        h = (h - shift) / scale
        tot = 0
        for l, (name, (_, _, _, s, p)) in enumerate(zip(NAMES, CONVS)):
            if l in (1, 2):
                h = F.max_pool2d(h, 3, 2)
            h = F.relu(F.conv2d(h, wd[f"{name}.weight"], wd[f"{name}.bias"], stride=s, padding=p))
            n = h / (h.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            tot = tot + (wd[f"lin{l}.model.1.weight"] * (n[:N] - n[N:]) ** 2).sum(1).mean((1, 2))
        return tot

    dev_val = model(x0, x1)[:, 0, 0, 0]
    ref_val = torch_lpips()
    res = {"N": N, "H": H, "W": W, "device": torch.cuda.get_device_name(0),
           "max_abs_diff_device_vs_torch_fp32": float((dev_val - ref_val).abs().max()),
           "lpips_device_us": median_us(lambda: model(x0, x1)), "lpips_torch_fp32_us": median_us(torch_lpips), "convs": []}
    hw, flops_all, us_all = (H, W), 0.0, 0.0
    for l, (co, ci, k, s, p) in enumerate(CONVS):
        if l in (1, 2):
            hw = ((hw[0] - 3) // 2 + 1, (hw[1] - 3) // 2 + 1)
        pw = ops.pack_lpips_conv(sd[f"{NAMES[l]}.weight"], sd[f"{NAMES[l]}.bias"], dev)
        x = torch.rand(2 * N, hw[0], hw[1], pw["cin"], device=dev)
        us = median_us(lambda: ops.conv2d_f32(x, pw, stride=s, pad=p, relu=True))
        ho, wo = (hw[0] + 2 * p - k) // s + 1, (hw[1] + 2 * p - k) // s + 1
        flops = 2.0 * 2 * N * ho * wo * co * ci * k * k
        res["convs"].append({"layer": l + 1, "in": list(hw), "out": [ho, wo], "us": us, "gflop": flops / 1e9, "tflops": flops / us / 1e6,
                             "fraction_of_fp32_mfma_peak": flops / (us * 1e-6) / FP32_MFMA_PEAK})
        flops_all, us_all, hw = flops_all + flops, us_all + us, (ho, wo)
    res["conv_total_us"], res["conv_total_gflop"] = us_all, flops_all / 1e9
    res["conv_fraction_of_fp32_mfma_peak"] = flops_all / (us_all * 1e-6) / FP32_MFMA_PEAK
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
