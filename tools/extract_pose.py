#!/usr/bin/env python3
"""Estimate the whole-body pose of pictures on the device and write the pose map and the keypoints.

    python tools/extract_pose.py IMAGE... --weights CKPT --out DIR [--det_weights CKPT] [--image_size W H] [--detect_resolution R] [--faces]
                                 [--frame_resize {pillow,reference}]
                                 [--no_hands] [--input_size W H --widen_factor F --deepen_factor F]   (a checkpoint of another size than DWPose-l)

The reference's ``single_extract_pose.py`` on pcdms_amd: each picture is resized to ``--image_size`` (Pillow bicubic, default 1024 x 1024), the
DWPose-l estimator (``--weights``: mmpose's ``dw-ll_ucoco_384.pth``) runs on the detection frame of ``--detect_resolution`` (default 512) and the
map is drawn and resized for ``image_resolution`` = the image height, as ``DWposeDetector.__call__`` does.  For every IMAGE this writes
``DIR/<stem>_pose.png`` and ``DIR/<stem>_pose.npz`` with ``keypoints`` fp32 [P, 133, 2], ``scores`` fp32 [P, 133] and ``size`` = (width, height) of
the detection frame -- the file tools/render_pose.py and the stage-2 driver's ``--pose_source keypoints`` read.

With ``--det_weights`` (mmdet's YOLOX-l checkpoint) the person boxes come from the detector on the detection frame, as in the reference: label 0,
score > 0.5, mmpose's NMS; a picture without a detection gets its whole frame.  Without it the person box is the whole picture (what the
reference falls back to when its detector finds nothing; it suits pictures of one person) unless ``--box X1 Y1 X2 Y2`` (pixels of the resized
picture, repeatable) is given.  ``--frame_resize reference`` makes the detection frame as the reference does, with ``resize_image`` (OpenCV's 8-bit
Lanczos4 when the picture is enlarged, its area resampling otherwise, restated on the device); the default, ``pillow``, keeps Pillow's bicubic.
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


def extract(estimator, path, device, image_size=(1024, 1024), detect_resolution=512, boxes=None, hands=True, faces=False, detector=None,
            frame_resize="pillow"):
    """-> (pose map uint8 [H, W, 3], keypoints [P, 133, 2], scores [P, 133] on ``device``, (Hd, Wd) of the detection frame)"""
    img = P.resize(torch.from_numpy(np.array(Image.open(path).convert("RGB"))).to(device), image_size)
    if boxes is not None:   # given in pixels of the resized picture; the estimator works on the detection frame
        Hd, Wd = P.detect_size(image_size[1], image_size[0], detect_resolution)
        boxes = torch.tensor(boxes, dtype=torch.float32) * torch.tensor([Wd / image_size[0], Hd / image_size[1]] * 2, dtype=torch.float32)
    return P.estimate_pose_map(estimator, img, detect_resolution=detect_resolution, image_resolution=image_size[1], boxes=boxes, hands=hands,
                               faces=faces, return_keypoints=True, detector=detector, frame_resize=frame_resize)


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="Whole-body pose maps and keypoints of pictures, estimated on the device (DWPose-l).")
    p.add_argument("images", nargs="+")
    p.add_argument("--weights", required=True, help="the mmpose DWPose-l checkpoint (dw-ll_ucoco_384.pth)")
    p.add_argument("--out", required=True, help="output directory")
    p.add_argument("--image_size", type=int, nargs=2, default=(1024, 1024), metavar=("W", "H"))
    p.add_argument("--detect_resolution", type=int, default=512)
    p.add_argument("--frame_resize", choices=("pillow", "reference"), default="pillow",
                   help="how the detection frame is made: Pillow bicubic (default) or the reference's resize_image (cv2 Lanczos4 / area)")
    p.add_argument("--box", type=float, nargs=4, action="append", metavar=("X1", "Y1", "X2", "Y2"), help="a person box (default: the whole picture)")
    p.add_argument("--faces", action="store_true", help="draw the face points (the reference has that layer commented out)")
    p.add_argument("--no_hands", action="store_true")
    p.add_argument("--input_size", type=int, nargs=2, default=(288, 384), metavar=("W", "H"), help="the network's crop size (DWPose-l: 288 384)")
    p.add_argument("--widen_factor", type=float, default=1.0, help="CSPNeXt widen_factor of the checkpoint (DWPose-l: 1)")
    p.add_argument("--deepen_factor", type=float, default=1.0, help="CSPNeXt deepen_factor of the checkpoint (DWPose-l: 1)")
    p.add_argument("--det_weights", default=None, help="the mmdet YOLOX-l checkpoint: person boxes from the detector (default: the whole picture)")
    p.add_argument("--det_size", type=int, default=640, help="the detector's square input size (YOLOX-l: 640)")
    p.add_argument("--det_widen_factor", type=float, default=1.0, help="widen_factor of --det_weights (YOLOX-l: 1)")
    p.add_argument("--det_deepen_factor", type=float, default=1.0, help="deepen_factor of --det_weights (YOLOX-l: 1)")
    p.add_argument("--det_num_classes", type=int, default=80, help="classes of --det_weights (COCO: 80; class 0 is the person)")
    p.add_argument("--device", default="cuda")
    args = p.parse_args(argv)
    device = torch.device(args.device)
    estimator = P.DWPoseEstimator.from_checkpoint(args.weights, input_size=tuple(args.input_size), widen_factor=args.widen_factor,
                                                  deepen_factor=args.deepen_factor)
    detector = None
    if args.det_weights:
        detector = P.PersonDetector.from_checkpoint(args.det_weights, size=args.det_size, widen_factor=args.det_widen_factor,
                                                    deepen_factor=args.det_deepen_factor, num_classes=args.det_num_classes)
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    for path in args.images:
        pose, kp, sc, (Hd, Wd) = extract(estimator, path, device, tuple(args.image_size), args.detect_resolution, args.box, not args.no_hands, args.faces,
                                         detector, args.frame_resize)
        stem = Path(path).stem
        Image.fromarray(pose.cpu().numpy()).save(out / f"{stem}_pose.png")
        np.savez(out / f"{stem}_pose.npz", keypoints=kp.cpu().numpy(), scores=sc.cpu().numpy(), size=np.array([Wd, Hd], np.int64))
    return 0


if __name__ == "__main__":
    sys.exit(main())
