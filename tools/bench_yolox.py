"""Time the device person detector (pcdms_amd.pose.PersonDetector, YOLOX-l at 640 x 640) for N = 1 and N = 8 images against a torch fp32
restatement of the same network on the same device (tests/test_person_detector.py: Ref), and count its FLOPs and launches.  ``call_ms`` is a
whole call (one pcdm_detect_forward: prep, network, decode, both NMS passes); ``host_driven_network_ms`` the same network launched kernel by
kernel from Python; ``torch_fp32_network_ms`` the restatement (network only).  The three alternate inside every iteration.  Synthetic weights;
medians of HIP-event windows.  The numbers are recorded, not gated.  (The restatement is the test suite's, as tools/bench_dwpose.py takes its
own from there.)

    python tools/bench_yolox.py [--out profiles/yolox_bench.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tools.bench_dwpose import median_ms_interleaved  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    from pcdms_amd import ops, pose
    from tests.test_person_detector import FULL, _full_sd, _ref
    dev = torch.device("cuda:0")
    sd = _full_sd()
    det = pose.PersonDetector(sd, **FULL)
    ref = _ref({k: v.to(dev) for k, v in sd.items()}, FULL)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    S = FULL["size"]
    res = {"input": [S, S], "device": torch.cuda.get_device_name(0), "cases": []}
    for N in args.images:
        img = torch.randint(0, 256, (N, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(N)).to(dev)
        det(img)                                                               # uploads the weights
        focus = ops.detect_prep(img, S)
        nchw = focus.permute(0, 3, 1, 2).contiguous()
        w = det._weights(dev)
        got = det._network(focus, w)[0]
        want = ref.chain(nchw, dt=torch.float32)["head.0"].permute(0, 2, 3, 1)
        got = torch.cat([got[..., :5], got[..., 8:8 + det.C]], -1)
        ops.LAUNCH_LOG, det._taps = [], {}                                     # the host-driven schedule issues the same launches one by one: count them
        try:
            det(img)
            torch.cuda.synchronize()
            log = ops.LAUNCH_LOG
        finally:
            ops.LAUNCH_LOG, det._taps = None, None
        flops = sum(e[1] for e in log if e[0] == "conv2d_f32_act")
        ms = median_ms_interleaved({"call_ms": lambda: det(img),
                                    "host_driven_network_ms": lambda: det._network(focus, w),
                                    "torch_fp32_network_ms": lambda: ref.chain(nchw, dt=torch.float32)["head.2"]}, iters=args.iters, warmup=3)
        res["cases"].append({
            "images": N,
            "max_rel_diff_head0_device_vs_torch_fp32": float(((got - want).abs().max() / want.abs().max()).item()),
            **ms, "conv_gflop": flops / 1e9, "conv_tflops_in_call": flops / ms["call_ms"] / 1e9, "launches": len(log),
            "launches_by_kind": {n: sum(1 for e in log if e[0] == n) for n in sorted({e[0] for e in log})}})
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
