"""DWPose pose maps from keypoints on the device: everything ``controlnet_aux``'s ``DWposeDetector.__call__`` does AFTER its two networks.

The reference draws its pose maps on the host with OpenCV (``single_extract_pose.py`` -> ``DWposeDetector.__call__`` -> ``draw_pose``) and the
drivers read them back as image files.  Here keypoints -- from any detector, from text files, interpolated or edited -- become the uint8 map
on the device in two launches of csrc/pose_draw.hip (include/pcdm.h: pcdm_pose_draw), plus one for the optional bilinear resize to the image
resolution (pcdm_resize_linear_u8).  The result feeds ``preprocess.resize`` / ``stage2_inputs`` unchanged.

The keypoints themselves come from ``DWPoseEstimator``: the reference's second network (the top-down whole-body DWPose-l of mmpose: CSPNeXt-l,
RTMCC head, SimCC decoding) in exact fp32 on the device, image + person boxes -> 133 keypoints and scores per box; ``estimate_pose_map`` chains
it with the drawing.  The boxes come from ``PersonDetector``: the reference's first network (mmdet's YOLOX-l) with its label, score and NMS
filters, image -> person boxes (``detect_people``; ``estimate_pose_map(..., detector=...)``).  Without a detector and without boxes the box is
the whole image -- what the reference does when its detector finds nothing (dwpose/wholebody.py:78-79).  ``resize_image`` is
``controlnet_aux.util.resize_image``, the frame both networks see: OpenCV's 8-bit Lanczos4 when the picture is enlarged, its area resampling
otherwise (``preprocess.resize_cv``; restated from OpenCV's published generic path, coefficient details have differed between OpenCV releases and
parity with the ``cv2`` package is not pinned by a test).  ``estimate_pose_map`` makes its frame with it under ``frame_resize="reference"``; the
default, ``"pillow"``, keeps ``preprocess.resize`` (Pillow bicubic).  mmpose, mmdet and mmcv are not
dependencies; both networks are restated from their published definitions (include/pcdm.h) and checked against fp64 restatements on synthetic
weights (tests/test_dwpose.py, tests/test_person_detector.py), so parity with mmpose and mmdet on the published checkpoints is NOT pinned by a
test that runs by default.

From keypoints to integer primitives the kernels repeat the reference's operations in its order and precision.  The raster rules -- which
pixels an ellipse, a disc and a line cover -- are this project's own integer statement of OpenCV's; OpenCV is not a dependency, and parity
with its rasteriser is not pinned by a test here (tests/test_pose.py pins the rules against Pillow's), the same standing as
``preprocess.resize_cv_cubic``.  After the first call on a device (which uploads 3 KB of constants) nothing here synchronises with the host, so
``draw_pose`` can sit inside a captured graph.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import ctypes as C

import torch

from . import _lib, ops, preprocess

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


def resize_image(image_u8: torch.Tensor, resolution: int) -> torch.Tensor:
    """``controlnet_aux.util.resize_image(image, resolution)`` on the device: uint8 ``[H, W, 3]`` (or ``[M, H, W, 3]``) -> the ``detect_size`` frame,
    with ``cv2.INTER_LANCZOS4`` when ``k = resolution / min(H, W) > 1`` and ``cv2.INTER_AREA`` otherwise (``preprocess.resize_cv``)."""
    if image_u8.dim() not in (3, 4) or image_u8.shape[-1] != 3 or image_u8.dtype != torch.uint8:
        raise ValueError(f"an image is uint8 [H, W, 3] or [M, H, W, 3]: got {image_u8.dtype} {tuple(image_u8.shape)}")
    H, W = int(image_u8.shape[-3]), int(image_u8.shape[-2])
    Hd, Wd = detect_size(H, W, resolution)
    k = float(resolution) / min(float(H), float(W))
    return preprocess.resize_cv(image_u8, (Wd, Hd), "lanczos4" if k > 1 else "area")


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


# ------------------------------------------------------------------------------------------------ the whole-body estimator
def _coco_wholebody_flip() -> List[int]:
    """COCO-WholeBody's published left / right pairs (mmpose configs/_base_/datasets/coco_wholebody.py: the ``swap`` fields) as the index list
    ``flip_indices``: entry k is the keypoint that k becomes in the mirrored image."""
    pairs = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16), (17, 20), (18, 21), (19, 22)]
    pairs += [(23 + i, 39 - i) for i in range(8)]                                      # face contour
    pairs += [(40 + i, 49 - i) for i in range(5)]                                      # eyebrows
    pairs += [(54, 58), (55, 57)]                                                      # nostrils
    pairs += [(59, 68), (60, 67), (61, 66), (62, 65), (63, 70), (64, 69)]              # eyes
    pairs += [(71, 77), (72, 76), (73, 75), (78, 82), (79, 81), (83, 87), (84, 86), (88, 90)]   # mouth
    pairs += [(91 + i, 112 + i) for i in range(21)]                                    # hands
    idx = list(range(133))
    for a, b in pairs:
        idx[a], idx[b] = b, a
    return idx


COCO_WHOLEBODY_FLIP = tuple(_coco_wholebody_flip())
_ARCH_P5 = ((64, 128, 3, True, False), (128, 256, 6, True, False), (256, 512, 6, True, False), (512, 1024, 3, False, True))
_HIDDEN, _GAU_S, _GAU_E = 256, 128, 512                    # RTMCCHead: hidden_dims, gau_cfg s, hidden_dims x expansion_factor 2
_BN = ("weight", "bias", "running_mean", "running_var")


class DWPoseEstimator:
    """The top-down whole-body pose estimator of the reference's ``DWposeDetector`` (``src/configs/dwpose-l_384x288.py``: mmdet ``CSPNeXt``
    backbone, P5, channel attention, SiLU; mmpose ``RTMCCHead`` with one GAU block; SimCC decoding with flip test) in exact fp32 on the device.

    ``estimator(images_u8, boxes)`` -> ``(keypoints [R, K, 2], scores [R, K])`` on the device, keypoints in pixels of the image, scores the raw
    SimCC logits (``min`` of the two axes' maxima), COCO-WholeBody order -- what ``inference_topdown`` + ``merge_data_samples`` give
    ``Wholebody.__call__``.  ``state_dict``: mmpose's own key names (``backbone.*``, ``head.*``); unknown or missing keys raise and are named.
    ``input_size`` is ``(width, height)`` as in the config; ``bn_eps`` is torch's default 1e-5 because the config overrides ``norm_cfg`` with a
    bare ``SyncBN``; ``flip_indices`` defaults to COCO-WholeBody's published pairs (133 keypoints only).  Every BatchNorm is folded into its
    convolution in fp64 and rounded to fp32 once.  A call is ONE C call (pcdm_dwpose_forward: a fixed sequence of launches of csrc/pose_net.hip and
    pcdm_conv2d_f32_act on one workspace, no host synchronisation, so it can be captured in a graph); with the ``_taps`` test hook set, the same
    launches are issued from here one by one and every intermediate tensor is recorded -- bit for bit the same result."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], *, input_size: Sequence[int] = (288, 384), widen_factor: float = 1.0,
                 deepen_factor: float = 1.0, num_keypoints: int = 133, bn_eps: float = 1e-5, flip_indices: Optional[Sequence[int]] = None):
        self.Win, self.Hin = int(input_size[0]), int(input_size[1])
        if self.Win <= 0 or self.Hin <= 0 or self.Win % 32 or self.Hin % 32:
            raise ValueError(f"input_size (width, height) must be positive multiples of 32 (the backbone's stride): {tuple(input_size)}")
        self.K, self.bn_eps = int(num_keypoints), float(bn_eps)
        if not 0 < self.K <= 256:
            raise ValueError(f"num_keypoints must lie in 1 .. 256 (the gated-attention kernel's token limit): {num_keypoints}")
        if flip_indices is None:
            flip_indices = COCO_WHOLEBODY_FLIP if self.K == 133 else None
        elif sorted(int(i) for i in flip_indices) != list(range(self.K)):
            raise ValueError(f"flip_indices must be a permutation of 0 .. {self.K - 1}")
        self.flip_indices = None if flip_indices is None else [int(i) for i in flip_indices]
        self.stem = int(_ARCH_P5[0][0] * widen_factor)
        self.stages = [(int(ci * widen_factor), int(co * widen_factor), max(round(nb * deepen_factor), 1), ident, spp)
                       for ci, co, nb, ident, spp in _ARCH_P5]
        if self.stem % 8 or any(co % 8 for _, co, _, _, _ in self.stages):
            raise ValueError(f"widen_factor {widen_factor} gives channel counts that are no multiples of 8 (branches are slices of four-channel groups)")
        self._taps: Optional[Dict[str, torch.Tensor]] = None
        self._dev: Dict[str, dict] = {}
        self._host = self._pack(dict(state_dict))

    # ---------------------------------------------------------------- weights
    def expected_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """Every key of mmpose's state dict for this configuration (``num_batches_tracked`` of the BatchNorms is accepted and ignored)."""
        exp: Dict[str, Tuple[int, ...]] = {}

        def cm(name, co, ci, k, groups=1):
            exp[f"{name}.conv.weight"] = (co, ci // groups, k, k)
            for b in _BN:
                exp[f"{name}.bn.{b}"] = (co,)

        c = self.stem
        cm("backbone.stem.0", c // 2, 3, 3); cm("backbone.stem.1", c // 2, c // 2, 3); cm("backbone.stem.2", c, c // 2, 3)
        for s, (ci, co, nb, _, spp) in enumerate(self.stages, 1):
            cm(f"backbone.stage{s}.0", co, ci, 3)
            if spp:
                cm(f"backbone.stage{s}.1.conv1", co // 2, co, 1); cm(f"backbone.stage{s}.1.conv2", co, 2 * co, 1)
            n, mid = f"backbone.stage{s}.{2 if spp else 1}", co // 2
            cm(f"{n}.main_conv", mid, co, 1); cm(f"{n}.short_conv", mid, co, 1); cm(f"{n}.final_conv", co, 2 * mid, 1)
            for b in range(nb):
                cm(f"{n}.blocks.{b}.conv1", mid, mid, 3)
                cm(f"{n}.blocks.{b}.conv2.depthwise_conv", mid, mid, 5, groups=mid)
                cm(f"{n}.blocks.{b}.conv2.pointwise_conv", mid, mid, 1)
            exp[f"{n}.attention.fc.weight"], exp[f"{n}.attention.fc.bias"] = (2 * mid, 2 * mid, 1, 1), (2 * mid,)
        P = (self.Hin // 32) * (self.Win // 32)
        exp.update({"head.final_layer.weight": (self.K, self.stages[-1][1], 7, 7), "head.final_layer.bias": (self.K,), "head.mlp.0.g": (1,),
                    "head.mlp.1.weight": (_HIDDEN, P), "head.gau.ln.g": (1,), "head.gau.uv.weight": (2 * _GAU_E + _GAU_S, _HIDDEN),
                    "head.gau.o.weight": (_HIDDEN, _GAU_E), "head.gau.gamma": (2, _GAU_S), "head.gau.beta": (2, _GAU_S),
                    "head.gau.res_scale.scale": (_HIDDEN,), "head.cls_x.weight": (2 * self.Win, _HIDDEN), "head.cls_y.weight": (2 * self.Hin, _HIDDEN)})
        return exp

    def _pack(self, sd: Dict[str, torch.Tensor]) -> dict:
        exp = self.expected_shapes()
        sd = {k: v for k, v in sd.items() if not k.endswith(".num_batches_tracked")}
        missing, unknown = sorted(k for k in exp if k not in sd), sorted(k for k in sd if k not in exp)
        bad = [f"{k}: {tuple(sd[k].shape)} vs {exp[k]}" for k in exp if k in sd and tuple(sd[k].shape) != exp[k]]
        if missing or unknown or bad:
            raise KeyError(f"DWPoseEstimator state dict (mmpose's key names): missing {missing[:8]}{'...' if len(missing) > 8 else ''}, "
                           f"unknown {unknown[:8]}{'...' if len(unknown) > 8 else ''}, shape {bad[:8]}")
        f64 = lambda k: sd[k].detach().to("cpu", torch.float64)   # noqa: E731
        f32 = lambda k: sd[k].detach().to("cpu", torch.float32).contiguous()   # noqa: E731
        host: dict = {}
        for k in exp:
            if not k.endswith(".conv.weight"):
                continue
            name = k[:-len(".conv.weight")]
            g, b, m, v = (f64(f"{name}.bn.{t}") for t in _BN)
            scale = g / torch.sqrt(v + self.bn_eps)
            w, bias = (f64(k) * scale.view(-1, 1, 1, 1)).to(torch.float32), (b - m * scale).to(torch.float32)
            if name.endswith("depthwise_conv"):
                host[name] = {"w": w.view(w.shape[0], 25).t().contiguous(), "bias": bias.contiguous()}
            else:
                host[name] = ops.pack_lpips_conv(w, bias, "cpu")
        for s, (_, _, _, _, spp) in enumerate(self.stages, 1):
            n = f"backbone.stage{s}.{2 if spp else 1}.attention.fc"
            host[n] = {"w": f32(f"{n}.weight").view(exp[f"{n}.bias"][0], -1).contiguous(), "bias": f32(f"{n}.bias")}
        host["head.final_layer"] = ops.pack_lpips_conv(f32("head.final_layer.weight"), f32("head.final_layer.bias"), "cpu")
        lin = lambda w: ops.pack_lpips_conv(w.view(w.shape[0], w.shape[1], 1, 1), None, "cpu")   # noqa: E731
        host["head.mlp.1"], host["head.gau.uv"], host["head.gau.o"] = lin(f32("head.mlp.1.weight")), lin(f32("head.gau.uv.weight")), lin(f32("head.gau.o.weight"))
        host["head.cls"] = lin(torch.cat([f32("head.cls_x.weight"), f32("head.cls_y.weight")], 0))   # one launch: x bins, then y bins
        for k in ("head.mlp.0.g", "head.gau.ln.g", "head.gau.gamma", "head.gau.beta", "head.gau.res_scale.scale"):
            host[k] = f32(k)
        return host

    @classmethod
    def from_checkpoint(cls, path, **kwargs) -> "DWPoseEstimator":
        """An mmpose ``.pth`` (``{"state_dict": ...}`` or the bare state dict), read with ``weights_only=True``; ``kwargs`` as for the constructor."""
        ck = torch.load(str(path), map_location="cpu", weights_only=True)
        if isinstance(ck, dict) and isinstance(ck.get("state_dict"), dict):
            ck = ck["state_dict"]
        return cls(dict(ck), **kwargs)

    def _weights(self, device: torch.device) -> dict:
        key = str(device)
        if key not in self._dev:
            w = {n: ({k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in p.items()} if isinstance(p, dict) else p.to(device))
                 for n, p in self._host.items()}
            w["flip"] = None if self.flip_indices is None else torch.tensor(self.flip_indices, dtype=torch.int32).to(device)
            self._dev[key] = w
        return self._dev[key]

    def _conv_order(self) -> Tuple[List[str], List[str]]:
        """(the packed convolutions, the depthwise layers) by name in schedule order = pcdm_dwpose_weights' order (include/pcdm.h)"""
        convs, dws = [f"backbone.stem.{i}" for i in range(3)], []
        for s, (_, _, nb, _, spp) in enumerate(self.stages, 1):
            convs.append(f"backbone.stage{s}.0")
            if spp:
                convs += [f"backbone.stage{s}.1.conv1", f"backbone.stage{s}.1.conv2"]
            n = f"backbone.stage{s}.{2 if spp else 1}"
            convs += [f"{n}.main_conv", f"{n}.short_conv"]
            for b in range(nb):
                convs += [f"{n}.blocks.{b}.conv1", f"{n}.blocks.{b}.conv2.pointwise_conv"]
                dws.append(f"{n}.blocks.{b}.conv2.depthwise_conv")
            convs.append(f"{n}.final_conv")
        return convs + ["head.final_layer", "head.mlp.1", "head.gau.uv", "head.gau.o", "head.cls"], dws

    def _c_args(self, device: torch.device):
        """(pcdm_dwpose_config, pcdm_dwpose_weights) for ``pcdm_dwpose_forward`` on ``device`` (the pointer arrays are kept alive with the weights)"""
        w = self._weights(device)
        if "c_args" not in w:
            cfg = _lib.DWPoseConfig(Hin=self.Hin, Win=self.Win, K=self.K, stem=self.stem, n_stages=len(self.stages))
            for i, (_, co, nb, ident, spp) in enumerate(self.stages):
                cfg.out[i], cfg.blocks[i], cfg.identity[i], cfg.spp[i] = co, nb, int(ident), int(spp)
            convs, dws = self._conv_order()
            arr = lambda names, key: (C.c_void_p * len(names))(*[ops._ptr(w[n][key]) for n in names])   # noqa: E731
            keep = [arr(convs, "w"), arr(convs, "bias"), arr(dws, "w"), arr(dws, "bias")]
            wt = _lib.DWPoseWeights(n_conv=len(convs), n_dw=len(dws))
            wt.conv_w, wt.conv_b, wt.dw_w, wt.dw_b = (C.cast(a, C.POINTER(C.c_void_p)) for a in keep)
            for i, (_, _, _, _, spp) in enumerate(self.stages):
                fc = w[f"backbone.stage{i + 1}.{2 if spp else 1}.attention.fc"]
                wt.fc_w[i], wt.fc_b[i] = ops._ptr(fc["w"]), ops._ptr(fc["bias"])
            wt.mlp_g, wt.ln_g = ops._ptr(w["head.mlp.0.g"]), ops._ptr(w["head.gau.ln.g"])
            wt.gamma, wt.beta, wt.res_scale = ops._ptr(w["head.gau.gamma"]), ops._ptr(w["head.gau.beta"]), ops._ptr(w["head.gau.res_scale.scale"])
            wt.flip_idx = ops._ptr(w["flip"])
            w["c_args"] = (cfg, wt, keep)
        return w["c_args"][0], w["c_args"][1]

    def _tap(self, name: str, t: torch.Tensor) -> torch.Tensor:
        """Test hook (tests/test_dwpose.py): with ``self._taps`` a dict, a clone of every tensor a later launch reads is recorded under ``name``."""
        if self._taps is not None:
            self._taps[name] = t.clone()
        return t

    # ---------------------------------------------------------------- the schedule
    def _backbone(self, x: torch.Tensor, w: dict) -> torch.Tensor:
        """crops fp32 NHWC [B, Hin, Win, 4] -> the stride-32 feature map fp32 NHWC [B, Hin / 32, Win / 32, C]"""
        tap, silu = self._tap, ops.CONV_ACT_SILU
        for i in range(3):
            x = tap(f"stem.{i}", ops.conv2d_f32_act(x, w[f"backbone.stem.{i}"], stride=2 if i == 0 else 1, pad=(1, 1), act=silu))
        for s, (_, co, nb, ident, spp) in enumerate(self.stages, 1):
            x = tap(f"stage{s}.down", ops.conv2d_f32_act(x, w[f"backbone.stage{s}.0"], stride=2, pad=(1, 1), act=silu))
            B, h, wd = (int(v) for v in x.shape[:3])
            mid = co // 2
            if spp:   # conv1 -> slice 0 of the concatenation; the 5 / 9 / 13 pools are the 5 x 5 maximum cascaded, each into the next slice
                cat = torch.empty((B, h, wd, 4 * mid), dtype=torch.float32, device=x.device)
                ops.conv2d_f32_act(x, w[f"backbone.stage{s}.1.conv1"], act=silu, out=cat)
                for j in range(3):
                    ops.maxpool5_f32(cat, mid, cat, in_offset=j * mid, offset=(j + 1) * mid)
                tap(f"stage{s}.spp.cat", cat)
                x = tap(f"stage{s}.spp", ops.conv2d_f32_act(cat, w[f"backbone.stage{s}.1.conv2"], act=silu))
            x = self._csp_layer(x, w, s)
        return x

    def _csp_layer(self, x: torch.Tensor, w: dict, s: int) -> torch.Tensor:
        """stage ``s``'s CSPLayer on fp32 NHWC [B, h, w, out]: the two branches are the halves of ONE tensor (main | short), so the concatenation
        costs no copy, and the channel attention is folded into ``final_conv`` as a scale of its A operand"""
        tap, silu = self._tap, ops.CONV_ACT_SILU
        _, co, nb, ident, spp = self.stages[s - 1]
        B, h, wd = (int(v) for v in x.shape[:3])
        n, mid = f"backbone.stage{s}.{2 if spp else 1}", co // 2
        cat = torch.empty((B, h, wd, 2 * mid), dtype=torch.float32, device=x.device)
        ops.conv2d_f32_act(x, w[f"{n}.main_conv"], act=silu, out=cat)
        ops.conv2d_f32_act(x, w[f"{n}.short_conv"], act=silu, out=cat, offset=mid)
        tap(f"stage{s}.csp.in", cat)
        for b in range(nb):   # the block rewrites the main slice in place: its last convolution reads `u`, adds and writes the slice
            t = tap(f"stage{s}.blocks.{b}.conv1", ops.conv2d_f32_act(cat, w[f"{n}.blocks.{b}.conv1"], pad=(1, 1), act=silu))
            dw = w[f"{n}.blocks.{b}.conv2.depthwise_conv"]
            u = tap(f"stage{s}.blocks.{b}.dw", ops.dwconv5_silu_f32(t, dw["w"], dw["bias"], torch.empty_like(t)))
            ops.conv2d_f32_act(u, w[f"{n}.blocks.{b}.conv2.pointwise_conv"], act=silu, residual=cat if ident else None, out=cat)
            tap(f"stage{s}.blocks.{b}", cat)
        fc = w[f"{n}.attention.fc"]
        att = tap(f"stage{s}.att", ops.fc_hsigmoid_f32(tap(f"stage{s}.pool", ops.global_avgpool_f32(cat)), fc["w"], fc["bias"]))
        return tap(f"stage{s}", ops.conv2d_f32_act(cat, w[f"{n}.final_conv"], act=silu, a_scale=att))

    def _head(self, x: torch.Tensor, w: dict) -> torch.Tensor:
        """the feature map -> the SimCC logits fp32 [B K, 2 Win + 2 Hin] (x bins, then y bins)"""
        tap, K = self._tap, self.K
        B, h, wd = (int(v) for v in x.shape[:3])
        P, rows = h * wd, B * K
        f = tap("head.final_layer", ops.conv2d_f32_act(x, w["head.final_layer"], pad=(3, 3)))              # [B, h, wd, K]: token k = channel k
        t = tap("head.mlp.0", ops.scalenorm_f32(f, B, K, P, (P * K, 1, K), w["head.mlp.0.g"]))
        x1 = tap("head.mlp.1", ops.conv2d_f32_act(t.view(1, 1, rows, -1), w["head.mlp.1"]))
        hn, short = ops.scalenorm_f32(x1, 1, rows, _HIDDEN, (0, _HIDDEN, 1), w["head.gau.ln.g"], side_scale=w["head.gau.res_scale.scale"])
        tap("head.gau.ln", hn); tap("head.gau.shortcut", short)
        uv = tap("head.gau.uv", ops.conv2d_f32_act(hn.view(1, 1, rows, _HIDDEN), w["head.gau.uv"], act=ops.CONV_ACT_SILU))
        core = tap("head.gau.core", ops.gau_core_f32(uv.view(rows, -1), B, w["head.gau.gamma"], w["head.gau.beta"]))
        x2 = tap("head.gau", ops.conv2d_f32_act(core.view(1, 1, rows, _GAU_E), w["head.gau.o"], residual=short.view(1, 1, rows, _HIDDEN)))
        return tap("head.cls", ops.conv2d_f32_act(x2, w["head.cls"])).view(rows, -1)

    def __call__(self, images_u8: torch.Tensor, boxes: Optional[torch.Tensor] = None, image_index: Optional[torch.Tensor] = None,
                 flip_test: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """``images_u8`` uint8 RGB ``[N, H, W, 3]`` (or one ``[H, W, 3]``) on the device; ``boxes`` fp32 ``[R, 4]`` = (x1, y1, x2, y2) in pixels, on the
        device or anything ``torch.as_tensor`` takes (None: one box per image, the whole image); ``image_index`` int ``[R]``: the image of each box
        (None: all boxes belong to the one image, or box r to image r when R = N).  ``flip_test``: average with the mirrored crop's output, as
        the config's ``test_cfg``."""
        if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8 or images_u8.dim() not in (3, 4) or images_u8.shape[-1] != 3:
            raise ValueError(f"images are uint8 [N, H, W, 3] or [H, W, 3]: got {getattr(images_u8, 'dtype', type(images_u8))} "
                             f"{tuple(getattr(images_u8, 'shape', ()))}")
        img = (images_u8 if images_u8.dim() == 4 else images_u8.unsqueeze(0)).contiguous()
        N, H, W = (int(v) for v in img.shape[:3])
        dev = img.device
        if N == 0 or H == 0 or W == 0:
            raise ValueError(f"empty images: {tuple(img.shape)}")
        if boxes is None:
            if image_index is not None:
                raise ValueError("image_index needs boxes")
            boxes = torch.zeros((N, 4), dtype=torch.float32, device=dev)       # (filled on the device: nothing here copies from the host)
            boxes[:, 2], boxes[:, 3] = float(W), float(H)
        boxes = torch.as_tensor(boxes, dtype=torch.float32).to(dev).contiguous()
        if boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.shape[0] == 0:
            raise ValueError(f"boxes are [R, 4] with R >= 1: got {tuple(boxes.shape)}")
        R = int(boxes.shape[0])
        if image_index is None:
            if N != 1 and R != N:
                raise ValueError(f"{R} boxes for {N} images: pass image_index")
            image_index = torch.zeros(R, dtype=torch.int32, device=dev) if N == 1 else torch.arange(R, dtype=torch.int32, device=dev)
        else:
            image_index = torch.as_tensor(image_index)
            if tuple(image_index.shape) != (R,) or image_index.dtype.is_floating_point:
                raise ValueError(f"image_index is an integer [{R}] tensor: got {tuple(image_index.shape)} {image_index.dtype}")
            if image_index.device.type == "cpu" and (int(image_index.min()) < 0 or int(image_index.max()) >= N):
                raise ValueError(f"image_index must lie in 0 .. {N - 1}")
        image_index = image_index.to(dev, torch.int32).contiguous()
        flip = bool(flip_test)
        if flip and self.flip_indices is None:
            raise ValueError(f"flip_test needs flip_indices for {self.K} keypoints")
        w = self._weights(dev)
        if self._taps is None:   # the product path: the whole schedule as one C call on one workspace
            cfg, wt = self._c_args(dev)
            n = ops.dwpose_ws_bytes(cfg, R, flip)
            if n < 0:
                raise ValueError(f"the library refuses {R} boxes for this configuration")
            return ops.dwpose_forward(img, boxes, image_index, flip, cfg, wt, torch.empty(n // 4, dtype=torch.float32, device=dev))
        crops = self._tap("crop", ops.pose_crop(img, boxes, image_index, (self.Hin, self.Win), flip=flip))
        logits = self._head(self._backbone(crops, w), w)
        kp, sc = ops.simcc_decode(logits, 2 * self.Win, R, self.K, w["flip"] if flip else None, boxes, (self.Hin, self.Win))
        return self._tap("keypoints", kp), self._tap("scores", sc)

    forward = __call__


# ------------------------------------------------------------------------------------------------ the person detector
_YOLOX_P5 = ((64, 128, 3, True, False), (128, 256, 9, True, False), (256, 512, 9, True, False), (512, 1024, 3, False, True))
MAX_CANDIDATES = 1024                                      # the NMS kernel's limit (include/pcdm.h: pcdm_nms_f32)


class PersonDetector:
    """The person detector of the reference's ``DWposeDetector`` (``src/configs/yolox_l_8xb8-300e_coco.py``: mmdet ``CSPDarknet`` P5, ``YOLOXPAFPN``,
    ``YOLOXHead``) in exact fp32 on the device, with what ``Wholebody.__call__`` does to its output: label ``class_id`` (0: person), score >
    ``score_thr`` (0.5), then mmpose's ``nms(0.7)``.

    ``detector(images_u8)`` -> ``(boxes [N, max_det, 4], scores [N, max_det], count [N], overflow [N])`` on the device, without a synchronisation:
    boxes (x1, y1, x2, y2) in pixels of the image, in score order, rows beyond ``count`` zero; ``overflow`` is set where more than
    ``max_candidates`` (default 512, at most 1024) priors passed the thresholds or more than ``max_det`` (default 32, what ``draw_pose`` takes)
    boxes survived -- then the best ``max_candidates`` and the first ``max_det`` are used.  ``state_dict``: mmdet's own key names (``backbone.*``,
    ``neck.*``, ``bbox_head.*``); ``num_batches_tracked`` and keys that start with ``ema_`` (the published v2 checkpoint carries them) are ignored,
    anything else that is unknown or missing raises and is named.  Every BatchNorm (eps 1e-3) is folded into its convolution in fp64 and rounded
    to fp32 once; ``main_conv`` / ``short_conv`` and ``conv_reg`` / ``conv_obj`` run as one convolution each (bit-identical per output).  A call is
    ONE C call (pcdm_detect_forward); with the ``_taps`` test hook set the same launches are issued from here one by one and every intermediate
    tensor is recorded -- bit for bit the same result.  The network is restated from its definition (include/pcdm.h): parity with mmdet on the
    published checkpoint is not pinned by a test that runs by default."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], *, size: int = 640, widen_factor: float = 1.0, deepen_factor: float = 1.0,
                 num_classes: int = 80, class_id: int = 0, score_thr: float = 0.5, nms_thr: float = 0.65, pose_nms_thr: float = 0.7,
                 max_candidates: int = 512, max_det: int = MAX_PERSONS, bn_eps: float = 1e-3):
        self.S, self.C, self.class_id = int(size), int(num_classes), int(class_id)
        if not 32 <= self.S <= MAX_SIDE or self.S % 32:
            raise ValueError(f"size must be a multiple of 32 (the backbone's stride) in 32 .. {MAX_SIDE}: {size}")
        if not 0 < self.C <= 1024 or not 0 <= self.class_id < self.C:
            raise ValueError(f"num_classes in 1 .. 1024 and class_id below it: {num_classes}, {class_id}")
        if not 0 < int(max_det) <= int(max_candidates) <= MAX_CANDIDATES:
            raise ValueError(f"1 <= max_det <= max_candidates <= {MAX_CANDIDATES}: {max_det}, {max_candidates}")
        self.max_candidates, self.max_det = int(max_candidates), int(max_det)
        self.score_thr, self.nms_thr, self.pose_nms_thr, self.bn_eps = float(score_thr), float(nms_thr), float(pose_nms_thr), float(bn_eps)
        self.stem, self.head = int(_YOLOX_P5[0][0] * widen_factor), int(256 * widen_factor)
        self.stages = [(int(ci * widen_factor), int(co * widen_factor), max(round(nb * deepen_factor), 1), ident, spp)
                       for ci, co, nb, ident, spp in _YOLOX_P5]
        self.neck_blocks = max(round(3 * deepen_factor), 1)
        if self.stem % 8 or self.head % 8 or any(co % 8 for _, co, _, _, _ in self.stages):
            raise ValueError(f"widen_factor {widen_factor} gives channel counts that are no multiples of 8 (branches are slices of four-channel groups)")
        self.C4 = (self.C + 3) // 4 * 4
        self._taps: Optional[Dict[str, torch.Tensor]] = None
        self._dev: Dict[str, dict] = {}
        self._host = self._pack(dict(state_dict))

    # ---------------------------------------------------------------- weights
    def _csp_layers(self) -> List[Tuple[str, int, int, int]]:
        """every CSP layer as (module name, in, out, blocks), backbone first"""
        _, o1, o2, o3 = (co for _, co, _, _, _ in self.stages)
        out = [(f"backbone.stage{s}.{2 if spp else 1}", co, co, nb) for s, (_, co, nb, _, spp) in enumerate(self.stages, 1)]
        nb = self.neck_blocks
        return out + [("neck.top_down_blocks.0", 2 * o2, o2, nb), ("neck.top_down_blocks.1", 2 * o1, o1, nb),
                      ("neck.bottom_up_blocks.0", 2 * o1, o2, nb), ("neck.bottom_up_blocks.1", 2 * o2, o3, nb)]

    def expected_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """Every key of mmdet's state dict for this configuration (``num_batches_tracked`` and ``ema_*`` are accepted and ignored)."""
        exp: Dict[str, Tuple[int, ...]] = {}

        def cm(name, co, ci, k):
            exp[f"{name}.conv.weight"] = (co, ci, k, k)
            for b in _BN:
                exp[f"{name}.bn.{b}"] = (co,)

        _, o1, o2, o3 = (co for _, co, _, _, _ in self.stages)
        cm("backbone.stem.conv", self.stem, 12, 3)
        for s, (ci, co, _, _, spp) in enumerate(self.stages, 1):
            cm(f"backbone.stage{s}.0", co, ci, 3)
            if spp:
                cm(f"backbone.stage{s}.1.conv1", co // 2, co, 1); cm(f"backbone.stage{s}.1.conv2", co, 2 * co, 1)
        for n, ci, co, nb in self._csp_layers():
            mid = co // 2
            cm(f"{n}.main_conv", mid, ci, 1); cm(f"{n}.short_conv", mid, ci, 1); cm(f"{n}.final_conv", co, 2 * mid, 1)
            for b in range(nb):
                cm(f"{n}.blocks.{b}.conv1", mid, mid, 1); cm(f"{n}.blocks.{b}.conv2", mid, mid, 3)
        cm("neck.reduce_layers.0", o2, o3, 1); cm("neck.reduce_layers.1", o1, o2, 1)
        cm("neck.downsamples.0", o1, o1, 3); cm("neck.downsamples.1", o2, o2, 3)
        for i, c in enumerate((o1, o2, o3)):
            cm(f"neck.out_convs.{i}", self.head, c, 1)
            for j in range(2):
                cm(f"bbox_head.multi_level_cls_convs.{i}.{j}", self.head, self.head, 3); cm(f"bbox_head.multi_level_reg_convs.{i}.{j}", self.head, self.head, 3)
            for t, co in (("cls", self.C), ("reg", 4), ("obj", 1)):
                exp[f"bbox_head.multi_level_conv_{t}.{i}.weight"], exp[f"bbox_head.multi_level_conv_{t}.{i}.bias"] = (co, self.head, 1, 1), (co,)
        return exp

    def _pack(self, sd: Dict[str, torch.Tensor]) -> dict:
        exp = self.expected_shapes()
        sd = {k: v for k, v in sd.items() if not k.endswith(".num_batches_tracked") and not k.startswith("ema_")}
        missing, unknown = sorted(k for k in exp if k not in sd), sorted(k for k in sd if k not in exp)
        bad = [f"{k}: {tuple(sd[k].shape)} vs {exp[k]}" for k in exp if k in sd and tuple(sd[k].shape) != exp[k]]
        if missing or unknown or bad:
            raise KeyError(f"PersonDetector state dict (mmdet's key names): missing {missing[:8]}{'...' if len(missing) > 8 else ''}, "
                           f"unknown {unknown[:8]}{'...' if len(unknown) > 8 else ''}, shape {bad[:8]}")
        f64 = lambda k: sd[k].detach().to("cpu", torch.float64)   # noqa: E731

        def folded(name):
            g, b, m, v = (f64(f"{name}.bn.{t}") for t in _BN)
            scale = g / torch.sqrt(v + self.bn_eps)
            return (f64(f"{name}.conv.weight") * scale.view(-1, 1, 1, 1)).to(torch.float32), (b - m * scale).to(torch.float32)

        def padded(w, b, co):   # zero rows up to co outputs: the padding channels come out exactly 0
            return torch.cat([w, w.new_zeros((co - w.shape[0], *w.shape[1:]))]), torch.cat([b, b.new_zeros(co - b.shape[0])])

        host: dict = {}
        merged = {n for n, _, _, _ in self._csp_layers()}
        for k in exp:
            if not k.endswith(".conv.weight"):
                continue
            name = k[:-len(".conv.weight")]
            mod, _, leaf = name.rpartition(".")
            if mod in merged and leaf == "short_conv":
                continue
            w, b = folded(name)
            if mod in merged and leaf == "main_conv":   # (main | short) as one convolution: its outputs are the concatenation
                w2, b2 = folded(f"{mod}.short_conv")
                w, b, name = torch.cat([w, w2]), torch.cat([b, b2]), f"{mod}.main_short"
            host[name] = ops.pack_lpips_conv(w, b, "cpu")
        for i in range(3):
            f32 = lambda k: sd[k].detach().to("cpu", torch.float32)   # noqa: E731
            pre = "bbox_head.multi_level_conv_"
            host[f"{pre}cls.{i}"] = ops.pack_lpips_conv(*padded(f32(f"{pre}cls.{i}.weight"), f32(f"{pre}cls.{i}.bias"), self.C4), "cpu")
            w = torch.cat([f32(f"{pre}reg.{i}.weight"), f32(f"{pre}obj.{i}.weight")])
            b = torch.cat([f32(f"{pre}reg.{i}.bias"), f32(f"{pre}obj.{i}.bias")])
            host[f"{pre}regobj.{i}"] = ops.pack_lpips_conv(*padded(w, b, 8), "cpu")
        return host

    @classmethod
    def from_checkpoint(cls, path, **kwargs) -> "PersonDetector":
        """An mmdet ``.pth`` (``{"state_dict": ...}`` or the bare state dict), read with ``weights_only=True``; ``kwargs`` as for the constructor."""
        ck = torch.load(str(path), map_location="cpu", weights_only=True)
        if isinstance(ck, dict) and isinstance(ck.get("state_dict"), dict):
            ck = ck["state_dict"]
        return cls(dict(ck), **kwargs)

    def _weights(self, device: torch.device) -> dict:
        key = str(device)
        if key not in self._dev:
            self._dev[key] = {n: {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in p.items()} for n, p in self._host.items()}
        return self._dev[key]

    def _conv_order(self) -> List[str]:
        """the packed convolutions by name in schedule order = pcdm_detect_weights' order (include/pcdm.h)"""
        def csp(n, nb):
            return [f"{n}.main_short"] + [f"{n}.blocks.{b}.conv{j}" for b in range(nb) for j in (1, 2)] + [f"{n}.final_conv"]
        convs = ["backbone.stem.conv"]
        for s, (_, _, nb, _, spp) in enumerate(self.stages, 1):
            convs.append(f"backbone.stage{s}.0")
            if spp:
                convs += [f"backbone.stage{s}.1.conv1", f"backbone.stage{s}.1.conv2"]
            convs += csp(f"backbone.stage{s}.{2 if spp else 1}", nb)
        nb = self.neck_blocks
        convs += ["neck.reduce_layers.0"] + csp("neck.top_down_blocks.0", nb) + ["neck.reduce_layers.1"] + csp("neck.top_down_blocks.1", nb)
        convs += ["neck.downsamples.0"] + csp("neck.bottom_up_blocks.0", nb) + ["neck.downsamples.1"] + csp("neck.bottom_up_blocks.1", nb)
        convs += [f"neck.out_convs.{i}" for i in range(3)]
        for i in range(3):
            for t, last in (("cls", "cls"), ("reg", "regobj")):
                convs += [f"bbox_head.multi_level_{t}_convs.{i}.{j}" for j in range(2)] + [f"bbox_head.multi_level_conv_{last}.{i}"]
        return convs

    def _c_args(self, device: torch.device):
        """(pcdm_detect_config, pcdm_detect_weights) for ``pcdm_detect_forward`` on ``device`` (the pointer arrays are kept alive with the weights)"""
        w = self._weights(device)
        if "c_args" not in w:
            cfg = _lib.DetectConfig(S=self.S, num_classes=self.C, class_id=self.class_id, stem=self.stem, head=self.head, neck_blocks=self.neck_blocks,
                                    max_candidates=self.max_candidates, max_det=self.max_det, score_thr=self.score_thr, nms_thr=self.nms_thr,
                                    pose_nms_thr=self.pose_nms_thr)
            for i, (_, co, nb, _, _) in enumerate(self.stages):
                cfg.out[i], cfg.blocks[i] = co, nb
            convs = self._conv_order()
            keep = [(C.c_void_p * len(convs))(*[ops._ptr(w[n][key]) for n in convs]) for key in ("w", "bias")]
            wt = _lib.DetectWeights(n_conv=len(convs))
            wt.conv_w, wt.conv_b = (C.cast(a, C.POINTER(C.c_void_p)) for a in keep)
            w["c_args"] = (cfg, wt, keep)
        return w["c_args"][0], w["c_args"][1]

    def _tap(self, name: str, t: torch.Tensor) -> torch.Tensor:
        """Test hook (tests/test_person_detector.py): with ``self._taps`` a dict, a clone of every tensor a later launch reads is recorded."""
        if self._taps is not None:
            self._taps[name] = t.clone()
        return t

    # ---------------------------------------------------------------- the schedule, launch by launch (pcdm_detect_forward issues the same)
    def _csp(self, x: torch.Tensor, cin: int, in_offset: int, w: dict, n: str, tag: str, cout: int, nb: int, ident: bool, out: Optional[torch.Tensor] = None,
             offset: int = 0) -> torch.Tensor:
        """CSP layer ``n`` on the channels ``[in_offset, in_offset + cin)`` of ``x``: the two branches are the halves of ONE tensor (main | short)
        written by one convolution, the blocks rewrite the main half in place, ``final_conv`` writes the channels from ``offset`` of ``out``"""
        tap, silu, mid = self._tap, ops.CONV_ACT_SILU, cout // 2
        assert w[f"{n}.main_short"]["cin"] == cin
        cat = ops.conv2d_f32_act(x, w[f"{n}.main_short"], act=silu, in_offset=in_offset)
        tap(f"{tag}.csp.in", cat)
        for b in range(nb):
            t = tap(f"{tag}.blocks.{b}.conv1", ops.conv2d_f32_act(cat, w[f"{n}.blocks.{b}.conv1"], act=silu))
            ops.conv2d_f32_act(t, w[f"{n}.blocks.{b}.conv2"], pad=(1, 1), act=silu, residual=cat if ident else None, out=cat)
            tap(f"{tag}.blocks.{b}", cat)
        y = ops.conv2d_f32_act(cat, w[f"{n}.final_conv"], act=silu, out=out, offset=offset)
        tap(tag, y if out is None else out[..., offset:offset + cout].contiguous())
        return y

    def _network(self, focus: torch.Tensor, w: dict) -> List[torch.Tensor]:
        """the Focus tensor fp32 [N, S/2, S/2, 12] -> the three head tensors fp32 [N, S/stride, S/stride, 8 + C4]"""
        tap, silu = self._tap, ops.CONV_ACT_SILU
        N, dev = int(focus.shape[0]), focus.device
        (_, o0, b0, _, _), (_, o1, b1, _, _), (_, o2, b2, _, _), (_, o3, b3, _, _) = self.stages
        s8, s16, s32, nb = self.S // 8, self.S // 16, self.S // 32, self.neck_blocks
        new = lambda s, c: torch.empty((N, s, s, c), dtype=torch.float32, device=dev)   # noqa: E731
        td0, td1, bu0, bu1 = new(s16, 2 * o2), new(s8, 2 * o1), new(s16, 2 * o1), new(s32, 2 * o2)
        x = tap("stem", ops.conv2d_f32_act(focus, w["backbone.stem.conv"], pad=(1, 1), act=silu))
        x = tap("stage1.down", ops.conv2d_f32_act(x, w["backbone.stage1.0"], stride=2, pad=(1, 1), act=silu))
        x = self._csp(x, o0, 0, w, "backbone.stage1.1", "stage1", o0, b0, True)
        x = tap("stage2.down", ops.conv2d_f32_act(x, w["backbone.stage2.0"], stride=2, pad=(1, 1), act=silu))
        self._csp(x, o1, 0, w, "backbone.stage2.1", "stage2", o1, b1, True, out=td1, offset=o1)                 # c3: the second half of td1
        x = tap("stage3.down", ops.conv2d_f32_act(td1, w["backbone.stage3.0"], stride=2, pad=(1, 1), act=silu, in_offset=o1))
        self._csp(x, o2, 0, w, "backbone.stage3.1", "stage3", o2, b2, True, out=td0, offset=o2)                 # c4: the second half of td0
        x = tap("stage4.down", ops.conv2d_f32_act(td0, w["backbone.stage4.0"], stride=2, pad=(1, 1), act=silu, in_offset=o2))
        spp = new(s32, 2 * o3)   # conv1 -> slice 0; the 5 / 9 / 13 pools are the 5 x 5 maximum cascaded, each into the next slice
        ops.conv2d_f32_act(x, w["backbone.stage4.1.conv1"], act=silu, out=spp)
        for j in range(3):
            ops.maxpool5_f32(spp, o3 // 2, spp, in_offset=j * (o3 // 2), offset=(j + 1) * (o3 // 2))
        tap("stage4.spp.cat", spp)
        x = tap("stage4.spp", ops.conv2d_f32_act(spp, w["backbone.stage4.1.conv2"], act=silu))
        c5 = self._csp(x, o3, 0, w, "backbone.stage4.2", "stage4", o3, b3, False)
        ops.conv2d_f32_act(c5, w["neck.reduce_layers.0"], act=silu, out=bu1, offset=o2)                           # r5
        ops.upsample2_nearest_f32(bu1, o2, td0, in_offset=o2)
        tap("neck.td0.cat", td0)
        t4 = self._csp(td0, 2 * o2, 0, w, "neck.top_down_blocks.0", "neck.t4", o2, nb, False)
        ops.conv2d_f32_act(t4, w["neck.reduce_layers.1"], act=silu, out=bu0, offset=o1)                           # r4
        ops.upsample2_nearest_f32(bu0, o1, td1, in_offset=o1)
        tap("neck.td1.cat", td1)
        p3 = self._csp(td1, 2 * o1, 0, w, "neck.top_down_blocks.1", "neck.p3", o1, nb, False)
        ops.conv2d_f32_act(p3, w["neck.downsamples.0"], stride=2, pad=(1, 1), act=silu, out=bu0)
        tap("neck.bu0.cat", bu0)
        p4 = self._csp(bu0, 2 * o1, 0, w, "neck.bottom_up_blocks.0", "neck.p4", o2, nb, False)
        ops.conv2d_f32_act(p4, w["neck.downsamples.1"], stride=2, pad=(1, 1), act=silu, out=bu1)
        tap("neck.bu1.cat", bu1)
        p5 = self._csp(bu1, 2 * o2, 0, w, "neck.bottom_up_blocks.1", "neck.p5", o3, nb, False)
        feats = [tap(f"head.{i}.f", ops.conv2d_f32_act(p, w[f"neck.out_convs.{i}"], act=silu)) for i, p in enumerate((p3, p4, p5))]
        heads = []
        for i, f in enumerate(feats):
            head = torch.empty((*f.shape[:3], 8 + self.C4), dtype=torch.float32, device=dev)
            for t, last, off in (("cls", "cls", 8), ("reg", "regobj", 0)):
                a = tap(f"head.{i}.{t}.0", ops.conv2d_f32_act(f, w[f"bbox_head.multi_level_{t}_convs.{i}.0"], pad=(1, 1), act=silu))
                b = tap(f"head.{i}.{t}.1", ops.conv2d_f32_act(a, w[f"bbox_head.multi_level_{t}_convs.{i}.1"], pad=(1, 1), act=silu))
                ops.conv2d_f32_act(b, w[f"bbox_head.multi_level_conv_{last}.{i}"], out=head, offset=off)
            heads.append(tap(f"head.{i}", head))
        return heads

    def select(self, boxes: torch.Tensor, scores: torch.Tensor, candidates: torch.Tensor):
        """the two greedy passes on decoded priors: mmcv's ``nms`` (IoU > ``nms_thr``, offset 0), then mmpose's over the survivors (``pose_nms_thr``,
        +1 on every width and height) -> ``(boxes [N, max_det, 4], scores [N, max_det], count [N], overflow [N])``"""
        first = ops.nms_f32(boxes, scores, candidates, thr=self.nms_thr, offset=0.0, max_candidates=self.max_candidates, max_det=self.max_candidates,
                            want_boxes=False)
        self._tap("nms.keep", first["keep"])
        r = ops.nms_f32(boxes, scores, first["keep"], thr=self.pose_nms_thr, offset=1.0, max_candidates=self.max_candidates, max_det=self.max_det,
                        overflow_in=first["overflow"], want_keep=self._taps is not None)
        if self._taps is not None:
            self._tap("nms2.keep", r["keep"])
        return r["boxes"], r["scores"], r["count"], r["overflow"]

    def __call__(self, images_u8: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """``images_u8`` uint8 RGB ``[N, H, W, 3]`` (or one ``[H, W, 3]``) on the device."""
        if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8 or images_u8.dim() not in (3, 4) or images_u8.shape[-1] != 3:
            raise ValueError(f"images are uint8 [N, H, W, 3] or [H, W, 3]: got {getattr(images_u8, 'dtype', type(images_u8))} "
                             f"{tuple(getattr(images_u8, 'shape', ()))}")
        img = (images_u8 if images_u8.dim() == 4 else images_u8.unsqueeze(0)).contiguous()
        N, H, W = (int(v) for v in img.shape[:3])
        if N == 0 or H == 0 or W == 0:
            raise ValueError(f"empty images: {tuple(img.shape)}")
        ops.detect_resized(H, W, self.S)                                       # (raises for a size the library refuses)
        dev = img.device
        w = self._weights(dev)
        if self._taps is None:   # the product path: the whole schedule as one C call on one workspace
            cfg, wt = self._c_args(dev)
            n = ops.detect_ws_bytes(cfg, N)
            if n < 0:
                raise ValueError(f"the library refuses {N} images for this configuration")
            return ops.detect_forward(img, cfg, wt, torch.empty(n // 4, dtype=torch.float32, device=dev))
        heads = self._network(self._tap("focus", ops.detect_prep(img, self.S)), w)
        boxes, scores, labels, cand = ops.detect_decode(heads, self.S, self.C, self.class_id, self.score_thr, (H, W))
        for k, v in (("decode.boxes", boxes), ("decode.scores", scores), ("decode.labels", labels), ("decode.candidates", cand)):
            self._tap(k, v)
        return self.select(boxes, scores, cand)

    forward = __call__


def detect_people(detector: PersonDetector, images_u8: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(boxes [R, 4], image_index [R])`` in the form ``DWPoseEstimator.__call__`` takes: every image's detected persons in score order, and for
    an image without a detection its whole frame (the reference's fallback, dwpose/wholebody.py:78-79).  The counts are read back from the device
    (one small copy, one synchronisation) because R is a tensor size."""
    img = images_u8 if images_u8.dim() == 4 else images_u8.unsqueeze(0)
    boxes, _, count, _ = detector(img)
    H, W = int(img.shape[1]), int(img.shape[2])
    out, index = [], []
    for n, c in enumerate(count.tolist()):
        out.append(boxes[n, :c] if c else boxes.new_tensor([[0.0, 0.0, float(W), float(H)]]))
        index += [n] * max(c, 1)
    return torch.cat(out), torch.tensor(index, dtype=torch.int32).to(boxes.device)


def estimate_pose_map(estimator: DWPoseEstimator, image_u8: torch.Tensor, *, detect_resolution: int = 512, image_resolution: int = 512,
                      boxes=None, hands: bool = True, faces: bool = False, return_keypoints: bool = False,
                      detector: Optional[PersonDetector] = None, frame_resize: str = "pillow"):
    """``DWposeDetector.__call__(image, detect_resolution, image_resolution)``: uint8 RGB ``[H, W, 3]`` on the device -> the pose map uint8
    ``[H', W', 3]``, (H', W') = ``detect_size(H, W, image_resolution)``.  The image is resized to the detection frame
    ``detect_size(H, W, detect_resolution)`` -- ``frame_resize="pillow"`` (the default): with ``preprocess.resize`` (Pillow bicubic);
    ``"reference"``: with ``resize_image``, the reference's cv2 Lanczos4 / area resampling -- the estimator runs on ``boxes`` (pixels of the
    detection frame), and every box's person is drawn.  ``boxes`` None: with a
    ``detector`` they are ``detect_people(detector, frame)`` -- the reference's whole pipeline, pixels -> boxes -> keypoints -> map; without one
    the box is the whole frame, what the reference does when its detector finds nothing.
    ``return_keypoints``: ``(map, keypoints [R, 133, 2], scores [R, 133], (Hd, Wd))`` -- what tools/extract_pose.py writes next to the image."""
    if image_u8.dim() != 3 or image_u8.dtype != torch.uint8 or image_u8.shape[2] != 3:
        raise ValueError(f"an image is uint8 [H, W, 3]: got {image_u8.dtype} {tuple(image_u8.shape)}")
    if frame_resize not in ("pillow", "reference"):
        raise ValueError(f"frame_resize must be 'pillow' or 'reference', not {frame_resize!r}")
    H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
    Hd, Wd = detect_size(H, W, detect_resolution)
    frame = preprocess.resize(image_u8, (Wd, Hd)) if frame_resize == "pillow" else resize_image(image_u8, detect_resolution)
    if boxes is None and detector is not None:
        boxes, _ = detect_people(detector, frame)
    kp, sc = estimator(frame, boxes)
    kp134, sc134 = wholebody_to_openpose(kp, sc)
    pose_map = draw_pose(kp134, sc134, (Hd, Wd), image_size=detect_size(H, W, image_resolution), hands=hands, faces=faces)[0]
    return (pose_map, kp, sc, (Hd, Wd)) if return_keypoints else pose_map
