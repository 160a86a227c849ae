"""DWPose pose maps from keypoints on the device: everything ``controlnet_aux``'s ``DWposeDetector.__call__`` does AFTER its two networks.

The reference draws its pose maps on the host with OpenCV (``single_extract_pose.py`` -> ``DWposeDetector.__call__`` -> ``draw_pose``) and the
drivers read them back as image files.  Here keypoints -- from any detector, from text files, interpolated or edited -- become the uint8 map
on the device in two launches of csrc/pose_draw.hip (include/pcdm.h: pcdm_pose_draw), plus one for the optional bilinear resize to the image
resolution (pcdm_resize_linear_u8).  The result feeds ``preprocess.resize`` / ``stage2_inputs`` unchanged.

The keypoints themselves come from ``DWPoseEstimator``: the reference's second network (the top-down whole-body DWPose-l of mmpose: CSPNeXt-l,
RTMCC head, SimCC decoding) in exact fp32 on the device, image + person boxes -> 133 keypoints and scores per box; ``estimate_pose_map`` chains
it with the drawing.  The person detector (YOLOX-l) is NOT part of this package: boxes come from the caller, and without boxes the box is the
whole image -- what the reference does when its detector finds nothing (dwpose/wholebody.py:78-79), which suits frames that hold one person.
Nor is ``controlnet_aux.util.resize_image`` (cv2 Lanczos / area resampling): the detection frame is made with ``preprocess.resize``.  mmpose and
mmdet are not dependencies; the network is restated from its published definition (include/pcdm.h) and checked against an fp64 restatement on
synthetic weights (tests/test_dwpose.py), so parity with mmpose on the published checkpoint is NOT pinned by a test that runs by default.

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
            arr = lambda names, key: (C.c_void_p * len(names))(*[w[n][key].data_ptr() for n in names])   # noqa: E731
            keep = [arr(convs, "w"), arr(convs, "bias"), arr(dws, "w"), arr(dws, "bias")]
            wt = _lib.DWPoseWeights(n_conv=len(convs), n_dw=len(dws))
            wt.conv_w, wt.conv_b, wt.dw_w, wt.dw_b = (C.cast(a, C.POINTER(C.c_void_p)) for a in keep)
            for i, (_, _, _, _, spp) in enumerate(self.stages):
                fc = w[f"backbone.stage{i + 1}.{2 if spp else 1}.attention.fc"]
                wt.fc_w[i], wt.fc_b[i] = fc["w"].data_ptr(), fc["bias"].data_ptr()
            wt.mlp_g, wt.ln_g = w["head.mlp.0.g"].data_ptr(), w["head.gau.ln.g"].data_ptr()
            wt.gamma, wt.beta, wt.res_scale = w["head.gau.gamma"].data_ptr(), w["head.gau.beta"].data_ptr(), w["head.gau.res_scale.scale"].data_ptr()
            wt.flip_idx = None if w["flip"] is None else w["flip"].data_ptr()
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


def estimate_pose_map(estimator: DWPoseEstimator, image_u8: torch.Tensor, *, detect_resolution: int = 512, image_resolution: int = 512,
                      boxes=None, hands: bool = True, faces: bool = False, return_keypoints: bool = False):
    """``DWposeDetector.__call__(image, detect_resolution, image_resolution)`` without the person detector: uint8 RGB ``[H, W, 3]`` on the device
    -> the pose map uint8 ``[H', W', 3]``, (H', W') = ``detect_size(H, W, image_resolution)``.  The image is resized to the detection frame
    ``detect_size(H, W, detect_resolution)`` with ``preprocess.resize`` (Pillow bicubic; the reference's cv2 Lanczos / area resampling is not
    restated), the estimator runs on ``boxes`` (pixels of the detection frame; None: the whole frame), and every box's person is drawn.
    ``return_keypoints``: ``(map, keypoints [R, 133, 2], scores [R, 133], (Hd, Wd))`` -- what tools/extract_pose.py writes next to the image."""
    if image_u8.dim() != 3 or image_u8.dtype != torch.uint8 or image_u8.shape[2] != 3:
        raise ValueError(f"an image is uint8 [H, W, 3]: got {image_u8.dtype} {tuple(image_u8.shape)}")
    H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
    Hd, Wd = detect_size(H, W, detect_resolution)
    frame = preprocess.resize(image_u8, (Wd, Hd))
    kp, sc = estimator(frame, boxes)
    kp134, sc134 = wholebody_to_openpose(kp, sc)
    pose_map = draw_pose(kp134, sc134, (Hd, Wd), image_size=detect_size(H, W, image_resolution), hands=hands, faces=faces)[0]
    return (pose_map, kp, sc, (Hd, Wd)) if return_keypoints else pose_map
