"""Time the device whole-body pose estimator (pcdms_amd.pose.DWPoseEstimator, DWPose-l at 384 x 288, flip test on) for R = 1 and R = 8 boxes
against a torch fp32 restatement of the same network on the same device (tests/test_dwpose.py: Ref), and count its FLOPs and launches.
``call_ms`` is a whole call (one pcdm_dwpose_forward: crop, network, decode); ``host_driven_network_ms`` the same network launched kernel by kernel
from Python; ``torch_fp32_network_ms`` the restatement (network only).  The three alternate inside every iteration.  Synthetic weights; medians of
HIP-event windows.  The numbers are recorded, not gated.  (The restatement is the test suite's, as tools/bench_fid.py takes its trunk from there.)

    python tools/bench_dwpose.py [--out profiles/dwpose_bench.json]
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def median_ms_interleaved(fns, iters=60, warmup=5):
    """Median HIP-event milliseconds of each callable, the callables alternating inside every iteration so that clock and thermal drift fall on
    all of them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--boxes", type=int, nargs="+", default=[1, 8])
    args = ap.parse_args()
    from pcdms_amd import ops, pose
    from tests.test_dwpose import FULL, Ref, _shapes
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    sd = {}
    for k, shp in _shapes(FULL).items():
        if k.endswith("weight") and len(shp) >= 2:
            sd[k] = torch.randn(shp, generator=g) * math.sqrt(2.0 / math.prod(shp[1:]))
        elif k.endswith(("bn.weight", "running_var", ".g", "scale")):
            sd[k] = torch.rand(shp, generator=g) + 0.5
        elif k == "head.gau.gamma":
            sd[k] = torch.randn(shp, generator=g) * 0.1 + 0.3
        else:
            sd[k] = (torch.rand(shp, generator=g) * 2 - 1) * 0.1
    est = pose.DWPoseEstimator(sd, **FULL)
    W, H = FULL["input_size"]
    ref = Ref({k: v.to(dev) for k, v in sd.items()}, Win=W, Hin=H, widen=1.0, deepen=1.0)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    img = torch.randint(0, 256, (1, 768, 512, 3), dtype=torch.uint8, generator=g).to(dev)
    res = {"input": [H, W], "flip_test": True, "device": torch.cuda.get_device_name(0), "cases": []}
    for R in args.boxes:
        boxes = torch.tensor([[20.0 + 9 * r, 30.0 + 5 * r, 400.0 + 9 * r, 700.0 + 5 * r] for r in range(R)]).to(dev)
        index = torch.zeros(R, dtype=torch.int32, device=dev)
        est(img, boxes, index)                                                 # uploads the weights
        crops = ops.pose_crop(img, boxes, index, (H, W), flip=True)
        nchw = crops[..., :3].permute(0, 3, 1, 2).contiguous()
        w = est._weights(dev)
        got = est._head(est._backbone(crops, w), w)
        want = ref.chain(nchw, dt=torch.float32)["head.cls"]
        ops.LAUNCH_LOG, est._taps = [], {}                                     # the host-driven schedule issues the same launches one by one: count them
        try:
            est(img, boxes, index)
            torch.cuda.synchronize()
            log = ops.LAUNCH_LOG
        finally:
            ops.LAUNCH_LOG, est._taps = None, None
        flops = sum(e[1] for e in log if e[0] == "conv2d_f32_act")
        ms = median_ms_interleaved({"call_ms": lambda: est(img, boxes, index),
                                    "host_driven_network_ms": lambda: est._head(est._backbone(crops, w), w),
                                    "torch_fp32_network_ms": lambda: ref.chain(nchw, dt=torch.float32)["head.cls"]})
        res["cases"].append({
            "boxes": R, "crops": 2 * R,
            "max_rel_diff_logits_device_vs_torch_fp32": float(((got - want).abs().max() / want.abs().max()).item()),
            **ms, "conv_gflop": flops / 1e9, "conv_tflops_in_call": flops / ms["call_ms"] / 1e9, "launches": len(log),
            "launches_by_kind": {n: sum(1 for e in log if e[0] == n) for n in sorted({e[0] for e in log})}})
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
