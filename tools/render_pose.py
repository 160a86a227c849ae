#!/usr/bin/env python3
"""Render the DWPose pose map of a keypoint file on the device and write it as an image.

    python tools/render_pose.py KEYPOINTS.npz OUT.png [--image_resolution R] [--faces] [--no_hands]

KEYPOINTS.npz holds ``keypoints`` fp32 [P, 134, 2] (OpenPose order, what the reference's ``Wholebody.__call__`` returns) or [P, 133, 2] (mmpose's
COCO-WholeBody order), ``scores`` fp32 [P, 134 | 133] and ``size`` = (width, height) of the detection frame the keypoints are pixels of.  The map
is what ``DWposeDetector.__call__`` draws from those keypoints (pcdms_amd/pose.py); with ``--image_resolution`` it is resized as the detector
resizes it for ``image_resolution``.  The stage-2 driver reads the same files with ``--pose_source keypoints``.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import pcdms_amd as P  # noqa: E402


def load_keypoints(path, device):
    """-> (keypoints [P, J, 2], scores [P, J] on ``device``, (H, W) of the detection frame)."""
    with np.load(path) as f:
        kp, sc, size = f["keypoints"].astype(np.float32), f["scores"].astype(np.float32), [int(v) for v in f["size"]]
    if kp.ndim != 3 or sc.shape != kp.shape[:2] or len(size) != 2:
        raise ValueError(f"{path}: keypoints [P, J, 2], scores [P, J] and size (width, height): got {kp.shape}, {sc.shape}, {size}")
    return torch.from_numpy(kp).to(device), torch.from_numpy(sc).to(device), (size[1], size[0])


def render(path, device, image_resolution=None, hands=True, faces=False) -> torch.Tensor:
    """The map of one keypoint file, uint8 [H, W, 3] on ``device``."""
    kp, sc, (H, W) = load_keypoints(path, device)
    image_size = None if image_resolution is None else P.detect_size(H, W, image_resolution)
    return P.draw_pose(kp, sc, (H, W), image_size=image_size, hands=hands, faces=faces)[0]


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="Render the pose map of a keypoint file (keypoints, scores, size) on the device.")
    p.add_argument("keypoints")
    p.add_argument("out")
    p.add_argument("--image_resolution", type=int, default=None, help="resize the map as DWposeDetector does for image_resolution (default: keep the detection size)")
    p.add_argument("--faces", action="store_true", help="draw the face points (the reference has that layer commented out)")
    p.add_argument("--no_hands", action="store_true")
    p.add_argument("--device", default="cuda")
    args = p.parse_args(argv)
    img = render(args.keypoints, torch.device(args.device), args.image_resolution, not args.no_hands, args.faces)
    Image.fromarray(img.cpu().numpy()).save(args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
