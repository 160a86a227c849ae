"""DWPose pose maps from keypoints on the device: everything ``controlnet_aux``'s ``DWposeDetector.__call__`` does AFTER its two networks.

The reference draws its pose maps on the host with OpenCV (``single_extract_pose.py`` -> ``DWposeDetector.__call__`` -> ``draw_pose``) and the
drivers read them back as image files.  Here keypoints -- from any detector, from text files, interpolated or edited -- become the uint8 map
on the device in two launches of csrc/pose_draw.hip (include/pcdm.h: pcdm_pose_draw), plus one for the optional bilinear resize to the image
resolution (pcdm_resize_linear_u8).  The result feeds ``preprocess.resize`` / ``stage2_inputs`` unchanged.  The detector networks (YOLOX,
DWPose-l) are not part of this package.

From keypoints to integer primitives the kernels repeat the reference's operations in its order and precision.  The raster rules -- which
pixels an ellipse, a disc and a line cover -- are this project's own integer statement of OpenCV's; OpenCV is not a dependency, and parity
with its rasteriser is not pinned by a test here (tests/test_pose.py pins the rules against Pillow's), the same standing as
``preprocess.resize_cv_cubic``.  After the first call on a device (which uploads 3 KB of constants) nothing here synchronises with the host, so
``draw_pose`` can sit inside a captured graph.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple, Union

import torch

from . import ops

MAX_PERSONS, MAX_SIDE = 32, 4096
_MMPOSE_IDX = [17, 6, 8, 10, 7, 9, 12, 14, 16, 13, 15, 2, 1, 4, 3]
_OPENPOSE_IDX = [1, 2, 3, 4, 6, 7, 8, 9, 10, 12, 13, 14, 15, 16, 17]
_TABLES: Dict[str, torch.Tensor] = {}


def wholebody_to_openpose(keypoints133, scores133) -> Tuple[torch.Tensor, torch.Tensor]:
    """COCO-WholeBody order (mmpose: ``[..., 133, 2]`` keypoints, ``[..., 133]`` scores) -> the 134-joint OpenPose order ``Wholebody.__call__``
    returns (dwpose/wholebody.py:97-119): the neck, the fp32 mean of the two shoulders, is inserted at 17 with score 1 iff both shoulder scores
    are ``> 0.3`` (else 0), then the body joints are permuted.  fp32 tensors on the inputs' device."""
    kp = torch.as_tensor(keypoints133, dtype=torch.float32)
    sc = torch.as_tensor(scores133, dtype=torch.float32).to(kp.device)
    if kp.shape[-2:] != (133, 2) or sc.shape != kp.shape[:-1]:
        raise ValueError(f"keypoints [..., 133, 2] and scores [..., 133]: got {tuple(kp.shape)} and {tuple(sc.shape)}")
    thr = torch.tensor(0.3, dtype=torch.float32, device=kp.device)
    neck = (kp[..., 5, :] + kp[..., 6, :]) / 2
    neck_sc = ((sc[..., 5] > thr) & (sc[..., 6] > thr)).to(torch.float32)
    kp = torch.cat([kp[..., :17, :], neck.unsqueeze(-2), kp[..., 17:, :]], dim=-2)
    sc = torch.cat([sc[..., :17], neck_sc.unsqueeze(-1), sc[..., 17:]], dim=-1)
    kp_o, sc_o = kp.clone(), sc.clone()
    kp_o[..., _OPENPOSE_IDX, :] = kp[..., _MMPOSE_IDX, :]
    sc_o[..., _OPENPOSE_IDX] = sc[..., _MMPOSE_IDX]
    return kp_o, sc_o


def detect_size(H: int, W: int, resolution: int) -> Tuple[int, int]:
    """``(H, W)`` of ``controlnet_aux.util.resize_image(image, resolution)``: the shorter side scaled to ``resolution``, both sides rounded to
    multiples of 64 (``np.round``: half to even)."""
    H, W = float(H), float(W)
    k = float(resolution) / min(H, W)
    H *= k
    W *= k
    return int(round(H / 64.0)) * 64, int(round(W / 64.0)) * 64


def _tables(device: torch.device) -> torch.Tensor:
    key = str(device)
    if key not in _TABLES:
        _TABLES[key] = torch.tensor(ops.pose_tables(), dtype=torch.int32).to(device)
    return _TABLES[key]


def _one_map(kp: torch.Tensor, sc: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    if kp.dim() != 3 or kp.shape[1] not in (133, 134) or kp.shape[2] != 2 or tuple(sc.shape) != tuple(kp.shape[:2]):
        raise ValueError(f"a map's keypoints are [P, 133 | 134, 2] and its scores [P, 133 | 134]: got {tuple(kp.shape)} and {tuple(sc.shape)}")
    kp, sc = kp.to(torch.float32), sc.to(torch.float32)
    return wholebody_to_openpose(kp, sc) if kp.shape[1] == 133 else (kp, sc)


def draw_pose(keypoints: Union[torch.Tensor, Sequence[torch.Tensor]], scores: Union[torch.Tensor, Sequence[torch.Tensor]], detect_size: Sequence[int], *,
              image_size: Optional[Sequence[int]] = None, hands: bool = True, faces: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The pose maps ``DWposeDetector.__call__`` returns, uint8 ``[M, H, W, 3]`` on the inputs' device.

    ``keypoints`` ``[M, P, J, 2]`` and ``scores`` ``[M, P, J]`` (or one map without the leading ``M``), ``J`` = 134 in OpenPose order or 133 in
    mmpose's (converted by ``wholebody_to_openpose``), in pixels of the ``detect_size`` = ``(H, W)`` detection frame.  Maps with different
    person counts: pad with score 0, or pass sequences of per-map tensors and they are padded here.  ``hands`` / ``faces``: the two optional
    layers (the reference draws hands and has faces commented out).  ``image_size`` = ``(H, W)``: the map is drawn at ``detect_size`` and
    resized with OpenCV's 8-bit INTER_LINEAR, as the detector does for ``image_resolution``.  At most 32 persons a map and 4096 pixels a side."""
    if isinstance(keypoints, torch.Tensor):
        if keypoints.dim() == 3:
            keypoints, scores = keypoints.unsqueeze(0), scores.unsqueeze(0)
        if keypoints.dim() != 4 or scores.dim() != 3 or keypoints.shape[0] != scores.shape[0]:
            raise ValueError(f"keypoints [M, P, J, 2] and scores [M, P, J]: got {tuple(keypoints.shape)} and {tuple(scores.shape)}")
        maps = [_one_map(k, s) for k, s in zip(keypoints, scores)] if keypoints.shape[0] else []
        dev = keypoints.device
    else:
        if len(keypoints) != len(scores):
            raise ValueError("as many score tensors as keypoint tensors")
        maps = [_one_map(k, s) for k, s in zip(keypoints, scores)]
        if not maps:
            raise ValueError("an empty sequence of maps has no device: pass a [0, P, J, 2] tensor")
        dev = maps[0][0].device
    H, W = int(detect_size[0]), int(detect_size[1])
    M, P = len(maps), max([k.shape[0] for k, _ in maps], default=0)
    if not (0 < H <= MAX_SIDE and 0 < W <= MAX_SIDE):
        raise ValueError(f"detect_size (H, W) must lie in 1 .. {MAX_SIDE}: {tuple(detect_size)}")
    if P > MAX_PERSONS:
        raise ValueError(f"at most {MAX_PERSONS} persons a map: {P}")
    kp = torch.zeros((M, P, 134, 2), dtype=torch.float32, device=dev)
    sc = torch.zeros((M, P, 134), dtype=torch.float32, device=dev)
    for m, (k, s) in enumerate(maps):
        kp[m, :k.shape[0]] = k
        sc[m, :k.shape[0]] = s
    final = (H, W) if image_size is None else (int(image_size[0]), int(image_size[1]))
    if final[0] <= 0 or final[1] <= 0:
        raise ValueError(f"image_size must be positive: {tuple(image_size)}")
    if out is None:
        out = torch.empty((M, *final, 3), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (M, *final, 3) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous uint8 [{M}, {final[0]}, {final[1]}, 3] tensor on {dev}")
    if M == 0:
        return out
    n = ops.pose_ws_bytes(M, P)
    if n < 0:
        raise ValueError(f"the library refuses {M} maps of {P} persons")
    ws = torch.empty(n // 4, dtype=torch.int32, device=dev).view(torch.uint8) if n > 0 else None
    canvas = out if final == (H, W) else torch.empty((M, H, W, 3), dtype=torch.uint8, device=dev)
    ops.pose_draw(kp, sc, _tables(dev), canvas, ws, hands=hands, faces=faces)
    return out if canvas is out else ops.resize_linear_u8(canvas, out)
