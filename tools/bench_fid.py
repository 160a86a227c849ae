"""Time the device InceptionV3 trunk (pcdms_amd.metrics.InceptionV3Features, dims 2048) on N = 64 uint8 images of 512 x 352 against a torch fp32
restatement of the same trunk on the same device (the one tests/test_fid.py checks it against), with the achieved fraction of the 157 TFLOP/s
fp32-MFMA rate.  Synthetic weights; median HIP-event time.

    python tools/bench_fid.py [--out profiles/fid_bench.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

FP32_MFMA_PEAK = 157e12


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def trunk_flops(n):
    """2 x multiply-adds of the 94 convolutions on a 299 x 299 input, from the layer table"""
    from pcdms_amd.metrics import INCEPTION_CONVS
    size = {"Conv2d_1a_3x3": 149, "Conv2d_2a_3x3": 147, "Conv2d_2b_3x3": 147, "Conv2d_3b_1x1": 73, "Conv2d_4a_3x3": 71, "Mixed_5": 35, "Mixed_6": 17,
            "Mixed_7": 8}
    total = 0
    for name, co, ci, kh, kw in INCEPTION_CONVS:
        side = size.get(name) or size[name[:7]]
        if name in ("Mixed_6a.branch3x3", "Mixed_6a.branch3x3dbl_3"):
            side = 17                                    # the stride-2 outputs of the 35 x 35 block
        elif name.startswith("Mixed_6a"):
            side = 35
        elif name in ("Mixed_7a.branch3x3_2", "Mixed_7a.branch7x7x3_4"):
            side = 8
        elif name.startswith("Mixed_7a"):
            side = 17
        total += 2 * side * side * co * ci * kh * kw
    return float(total) * n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=352)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    from pcdms_amd import metrics
    from tests import test_fid as T
    dev = torch.device("cuda:0")
    sd = T._state_dict()
    model = metrics.InceptionV3Features(2048).load_state_dict(sd)
    N, H, W = args.n, args.height, args.width
    x = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    wd = {k: v.to(dev) for k, v in sd.items()}
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    scale, shift = torch.tensor(T.SCALE, device=dev).view(1, 3, 1, 1), torch.tensor(T.SHIFT, device=dev).view(1, 3, 1, 1)

    def torch_trunk():
        h = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2).float() / 255.0, size=(299, 299), mode="bilinear", align_corners=False)
        return T._trunk(h * scale + shift, 2048, dtype=torch.float32, sd=wd, as_tensor=True)

    got, ref = model(x), torch_trunk()
    flops = trunk_flops(N)
    dev_ms, torch_ms = median_ms(lambda: model(x), args.iters, 2), median_ms(torch_trunk, args.iters, 2)
    res = {"N": N, "H": H, "W": W, "dims": 2048, "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "max_rel_diff_device_vs_torch_fp32": float((got - ref).abs().max() / ref.abs().max()),
           "trunk_device_ms": dev_ms, "trunk_torch_fp32_ms": torch_ms, "conv_gflop": flops / 1e9,
           "fraction_of_fp32_mfma_peak": flops / (dev_ms * 1e-3) / FP32_MFMA_PEAK}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
