"""Input preparation of the evaluation drivers on the device: Pillow-exact bicubic resize, the stage-2 canvases, ToTensor + Normalize and the
CLIP processor's pixel values, from the decoded uint8 pixels.

Per pair the reference's stage-2 driver resizes four images with ``Image.resize((W, H), Image.BICUBIC)``, pastes two canvases, normalises them
and runs ``CLIPImageProcessor()`` on the source, all on the host (stage2_batchtest_inpaint_model.py:135-149).  Here the decoded image is uploaded once
as uint8 ``[H, W, 3]`` and everything after it is the HIP kernels of csrc/image_prep.hip (include/pcdm.h: pcdm_resample_u8 / pcdm_u8_to_nchw).  Pillow's
8-bit resampler is integer arithmetic (22-bit fixed-point weights, a horizontal pass rounded to uint8, then a vertical pass), so the bytes are
Pillow's bytes, and the two float conversions repeat the operation order of their host originals, so the fp32 tensors are bit-identical as well.

The weight tables are built here in Python fp64, the way Pillow's ``precompute_coeffs`` / ``normalize_coeffs_8bpc`` build them, cached per
``(in, out, filter, device)`` and uploaded once.  Apart from that first upload of a new table nothing in this module synchronises with the host:
once the tables of a size are cached (one eager call), ``stage2_inputs`` + ``clip_pixel_values`` can sit inside a captured graph.  Decoding
PNG / JPEG stays on the host.  CPU tensors are refused, as everywhere in ``ops``.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_PRECISION_BITS = 32 - 8 - 2     # Pillow: weights of 8-bit images are 22-bit fixed point


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTERS = {"bicubic": (_bicubic, 2.0)}     # name -> (kernel, support)


def coeff_table(n_in: int, n_out: int, resample: str = "bicubic") -> Tuple[list, list, list, int]:
    """``(lo, count, coeff, k)`` of one axis, Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` step by step in fp64: output ``o`` reads
    ``count[o]`` inputs from ``lo[o]`` with the integer weights ``coeff[o * k : o * k + count[o]]`` (the rest of the row is zero)."""
    if resample not in _FILTERS:
        raise ValueError(f"resample must be one of {sorted(_FILTERS)}, not {resample!r}")
    f, support = _FILTERS[resample]
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = support * filterscale
    k = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    lo, count, coeff = [], [], [0] * (n_out * k)
    for o in range(n_out):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            coeff[o * k + x] = int(-0.5 + v * (1 << _PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << _PRECISION_BITS))
        lo.append(xmin)
        count.append(xmax)
    return lo, count, coeff, k


_TABLES: Dict[tuple, Tuple[torch.Tensor, int]] = {}


def _table(n_in: int, n_out: int, resample: str, device: torch.device) -> Tuple[Optional[torch.Tensor], int]:
    """The device table [lo | count | coeff] of one axis and its row length k; (None, 0) for an axis that keeps its size (Pillow skips it)."""
    if n_in == n_out:
        if resample not in _FILTERS:
            raise ValueError(f"resample must be one of {sorted(_FILTERS)}, not {resample!r}")
        return None, 0
    key = (n_in, n_out, resample, str(device))
    if key not in _TABLES:
        lo, count, coeff, k = coeff_table(n_in, n_out, resample)
        _TABLES[key] = (torch.tensor(lo + count + coeff, dtype=torch.int32).to(device), k)
    return _TABLES[key]


def _image(image_u8: torch.Tensor) -> torch.Tensor:
    if image_u8.dim() != 3 or image_u8.shape[2] not in (1, 3) or image_u8.dtype != torch.uint8:
        raise ValueError(f"an image is uint8 [H, W, 3] (or [H, W, 1]): got {image_u8.dtype} {tuple(image_u8.shape)}")
    return image_u8.contiguous()


def resize(image_u8: torch.Tensor, size: Sequence[int], *, out: Optional[torch.Tensor] = None, at: Sequence[int] = (0, 0),
           resample: str = "bicubic") -> torch.Tensor:
    """``Image.fromarray(image).resize(size, Image.BICUBIC)`` on the device, byte for byte: uint8 ``[H, W, 3]`` -> uint8 ``[size[1], size[0], 3]``
    (``size`` is ``(width, height)``, as in Pillow).  ``out``: an existing uint8 canvas ``[Hc, Wc, 3]`` to paste into at pixel ``at`` =
    ``(x0, y0)``; bytes outside the window keep their values and the canvas is returned."""
    src = _image(image_u8)
    Wd, Hd = int(size[0]), int(size[1])
    if Wd <= 0 or Hd <= 0:
        raise ValueError(f"size must be positive: {tuple(size)}")
    Hs, Ws, C = src.shape
    if out is None:
        if tuple(at) != (0, 0):
            raise ValueError("at= needs out=")
        out = torch.empty((Hd, Wd, C), dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or out.dim() != 3 or out.shape[2] != C or not out.is_contiguous() or out.device != src.device:
        raise ValueError(f"out must be a contiguous uint8 [Hc, Wc, {C}] canvas on {src.device}")
    if Hs > Ws * 100 and Hd < Hs and Ws != Wd:
        # Image.resize (Pillow 12) shrinks an image more than 100 times taller than wide vertically FIRST, as two resizes; every other image
        # takes the horizontal pass first, which is what one call of the kernel does
        src = resize(src, (Ws, Hd), resample=resample)
        Hs = Hd
    xtab, kx = _table(Ws, Wd, resample, src.device)
    ytab, ky = _table(Hs, Hd, resample, src.device)
    n = ops.resample_ws_bytes(Hs, Ws, Hd, Wd, C, ky)
    ws = torch.empty(n, dtype=torch.uint8, device=src.device) if n > 0 else None
    return ops.resample_u8(src, xtab, kx, ytab, ky, out, (Wd, Hd), at, ws)


def to_tensor_normalized(image_u8: torch.Tensor, window: Optional[Sequence[int]] = None) -> torch.Tensor:
    """fp32 ``[1, 3, H, W]`` = ``(x / 255 - 0.5) / 0.5``: ``transforms.ToTensor()`` + ``Normalize([0.5], [0.5])`` of the drivers, bit for bit, over
    the window ``(x0, y0, W, H)`` of a uint8 ``[H, W, 3]`` image (default: all of it)."""
    src = _image(image_u8)
    win = tuple(int(v) for v in window) if window is not None else (0, 0, src.shape[1], src.shape[0])
    C = src.shape[2]
    out = torch.empty((1, C, win[3], win[2]), dtype=torch.float32, device=src.device)
    return ops.u8_to_nchw(src, win, out, mode=0, scale=255.0, mean=(0.5,) * C, std=(0.5,) * C)


def clip_resize_size(height: int, width: int, size: int) -> Tuple[int, int]:
    """``(height, width)`` after the processor's shortest-edge resize (transformers ``get_resize_output_image_size(default_to_square=False)``)."""
    short, long = (width, height) if width <= height else (height, width)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if width <= height else (new_short, new_long)


def clip_pixel_values(image_u8: torch.Tensor, size: int = 224, crop: int = 224, mean: Sequence[float] = OPENAI_CLIP_MEAN,
                      std: Sequence[float] = OPENAI_CLIP_STD) -> torch.Tensor:
    """``CLIPImageProcessor()(images=image, return_tensors="pt").pixel_values`` on the device, fp32 ``[1, 3, crop, crop]``: shortest edge to
    ``size`` by the processor's output-size rule, Pillow bicubic, centre crop, then ``float32(float64(p) * (1 / 255))`` and ``(x - mean) / std`` in
    fp32 -- the operation order of the processor's numpy rescale and normalize, so the values are bit-identical."""
    src = _image(image_u8)
    if src.shape[2] != 3:
        raise ValueError("clip_pixel_values takes an RGB image")
    Hn, Wn = clip_resize_size(src.shape[0], src.shape[1], int(size))
    if crop > Hn or crop > Wn:
        raise ValueError(f"centre crop {crop} exceeds the resized image {Wn} x {Hn} (the processor would pad; not supported)")
    small = src if (Hn, Wn) == tuple(src.shape[:2]) else resize(src, (Wn, Hn))
    out = torch.empty((1, 3, crop, crop), dtype=torch.float32, device=src.device)
    return ops.u8_to_nchw(small, ((Wn - crop) // 2, (Hn - crop) // 2, crop, crop), out, mode=1, scale=1 / 255, mean=tuple(mean), std=tuple(std))


def stage2_inputs(s_img: torch.Tensor, s_pose: torch.Tensor, t_pose: torch.Tensor, W: int, H: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The stage-2 driver's per-pair tensors from the decoded source image and the two pose maps (uint8 ``[h, w, 3]`` on the device, any sizes):
    ``(vae_image, st_pose, s_img_u8)`` -- ``vae_image`` fp32 ``[1, 3, H, 2W]``, the normalised ``[source | black]`` canvas; ``st_pose`` fp32
    ``[1, 3, H, 2W]``, the normalised ``[source pose | target pose]`` canvas; ``s_img_u8`` uint8 ``[H, W, 3]``, the resized source for
    ``clip_pixel_values``.  The pose maps are resized straight into their halves of the canvas."""
    dev = s_img.device
    canvas = torch.zeros((2, H, 2 * W, 3), dtype=torch.uint8, device=dev)     # (black where nothing is pasted)
    s_img_u8 = resize(s_img, (W, H))
    resize(s_img_u8, (W, H), out=canvas[0])          # (both axes keep their size: the paste is a copy launch)
    resize(s_pose, (W, H), out=canvas[1])
    resize(t_pose, (W, H), out=canvas[1], at=(W, 0))
    return to_tensor_normalized(canvas[0]), to_tensor_normalized(canvas[1]), s_img_u8


def stage3_inputs(s_img: torch.Tensor, gen_t_img: torch.Tensor, W: int, H: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The stage-3 driver's per-pair tensors: ``(vae_gen_t_image, s_img_u8)`` -- the stage-2 result resized and normalised, fp32 ``[1, 3, H, W]``,
    and the resized source, uint8 ``[H, W, 3]``, for ``clip_pixel_values``."""
    return to_tensor_normalized(resize(gen_t_img, (W, H))), resize(s_img, (W, H))


def resize_cv_cubic(image: torch.Tensor, size: Sequence[int], *, divisor: Optional[float] = None, layout: str = "nhwc",
                    out: Optional[torch.Tensor] = None, index: int = 0) -> torch.Tensor:
    """``cv2.resize(image.astype(np.float32), size, interpolation=cv2.INTER_CUBIC)`` (``/ divisor`` when given) on the device -- the resize the
    reference's metric scripts put in front of every metric (metrics.py: calculate_from_disk).  ``image``: uint8 or fp32 ``[H, W, 3]``; ``size`` is
    ``(width, height)`` as in OpenCV.  The result is fp32, not rounded and not clipped (it overshoots below 0 and above 255), written as image
    ``index`` of the batch ``out``: ``[N, size[1], size[0], 3]`` for ``layout="nhwc"`` (SSIM, PSNR, L1, MAE) or ``[N, 3, size[1], size[0]]`` for
    ``"nchw"`` (LPIPS, FID); without ``out`` a batch of one is allocated.  The batch is returned; its other images are not touched.

    This is a different resampler from ``resize`` (Pillow's): no antialiasing when reducing, A = -0.75, fp32 arithmetic.  OpenCV is not a dependency:
    the algorithm is restated (include/pcdm.h: pcdm_resize_cubic_f32) and checked against an fp64 restatement (tests/test_eval_metrics.py), so
    parity with the ``cv2`` package itself is NOT pinned by a test here -- the same standing as LPIPS and FID.  One launch, no host synchronisation."""
    if layout not in ("nhwc", "nchw"):
        raise ValueError(f"layout must be 'nhwc' or 'nchw', not {layout!r}")
    if image.dim() != 3 or image.shape[2] != 3 or image.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"an image is uint8 or fp32 [H, W, 3]: got {image.dtype} {tuple(image.shape)}")
    Wd, Hd = int(size[0]), int(size[1])
    if Wd <= 0 or Hd <= 0:
        raise ValueError(f"size must be positive: {tuple(size)}")
    if divisor is not None and not divisor > 0:
        raise ValueError(f"divisor must be positive: {divisor!r}")
    shape = (Hd, Wd, 3) if layout == "nhwc" else (3, Hd, Wd)
    if out is None:
        if index != 0:
            raise ValueError("index= needs out=")
        out = torch.empty((1, *shape), dtype=torch.float32, device=image.device)
    elif out.dtype != torch.float32 or out.dim() != 4 or tuple(out.shape[1:]) != shape or not out.is_contiguous() or out.device != image.device:
        raise ValueError(f"out must be a contiguous fp32 [N, {', '.join(str(v) for v in shape)}] batch on {image.device}")
    if not 0 <= int(index) < out.shape[0]:
        raise ValueError(f"index {index} outside the batch of {out.shape[0]}")
    return ops.resize_cubic_f32(image.contiguous(), out, int(index), nchw=layout == "nchw", divisor=0.0 if divisor is None else float(divisor))


# ------------------------------------------------------------------------------------------------ cv2.resize(uint8, INTER_LANCZOS4 | INTER_AREA)
_F32 = np.float32
_FLT_EPSILON, _DBL_EPSILON = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)
_COEF_SCALE = 2048                           # OpenCV: INTER_RESIZE_COEF_SCALE = 1 << 11
_S45 = 0.70710678118654752440
_LANCZOS_CS = ((1.0, 0.0), (-_S45, -_S45), (0.0, 1.0), (_S45, -_S45), (-1.0, 0.0), (_S45, _S45), (0.0, -1.0), (-_S45, _S45))


def cv_scale(n_in: int, n_out: int) -> float:
    """OpenCV's per-axis scale: ``1.0 / ((double)n_out / (double)n_in)``."""
    return 1.0 / (float(n_out) / float(n_in))


def cv_lanczos4_coeffs(t) -> list:
    """The eight fp32 Lanczos4 coefficients of the fraction ``t`` (fp32), OpenCV's ``interpolateLanczos4`` (include/pcdm.h: rule 0)."""
    t = _F32(t)
    if t < _F32(_FLT_EPSILON):
        return [_F32(v) for v in (0, 0, 0, 1, 0, 0, 0, 0)]
    y0 = -(float(t) + 3.0) * math.pi / 4
    s0, c0 = math.sin(y0), math.cos(y0)
    c, total = [], _F32(0)
    for i, (a, b) in enumerate(_LANCZOS_CS):
        y = -(float(t) + 3.0 - i) * math.pi / 4
        c.append(_F32((a * s0 + b * c0) / (y * y)))
        total = _F32(total + c[-1])
    inv = _F32(_F32(1) / total)
    return [_F32(v * inv) for v in c]


def _cv_fixed(v) -> int:
    """``saturate_cast<short>(v * INTER_RESIZE_COEF_SCALE)``: one fp32 product, rounded to nearest even"""
    return int(min(max(np.rint(_F32(_F32(v) * _F32(_COEF_SCALE))), -32768), 32767))


def cv_lanczos4_table(n_in: int, n_out: int) -> list:
    """``[s (n_out) | coeff (n_out * 8)]`` of one axis (include/pcdm.h: pcdm_resize_cv_u8, rule 0)."""
    scale = cv_scale(n_in, n_out)
    ofs, coeff = [], []
    for d in range(n_out):
        f = _F32((d + 0.5) * scale - 0.5)
        s = math.floor(float(f))
        ofs.append(int(s))
        coeff += [_cv_fixed(c) for c in cv_lanczos4_coeffs(_F32(f - _F32(s)))]
    return ofs + coeff


def cv_area_table(n_in: int, n_out: int) -> list:
    """``[count (n_out) | source (n_out * k) | weight bits (n_out * k)]`` of one axis, ``k = int(scale) + 2``: OpenCV's ``computeResizeAreaTab``
    regrouped per output (include/pcdm.h: rule 2)."""
    scale = cv_scale(n_in, n_out)
    k = int(scale) + 2
    count, src, w = [], [0] * (n_out * k), [_F32(0)] * (n_out * k)
    for d in range(n_out):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, n_in - f1)
        s1, s2 = math.ceil(f1), min(math.floor(f2), n_in - 1)
        s1 = min(s1, s2)
        ent = []
        if s1 - f1 > 1e-3:
            ent.append((s1 - 1, _F32((s1 - f1) / cell)))
        ent += [(j, _F32(1.0 / cell)) for j in range(s1, s2)]
        if f2 - s2 > 1e-3:
            ent.append((s2, _F32(min(min(f2 - s2, 1.0), cell) / cell)))
        assert len(ent) <= k, (n_in, n_out, d, len(ent), k)
        count.append(len(ent))
        for j, (si, a) in enumerate(ent):
            src[d * k + j], w[d * k + j] = int(si), a
    return count + src + np.asarray(w, dtype=np.float32).view(np.int32).tolist()


def cv_area_linear_table(n_in: int, n_out: int, clamp_frac: bool) -> list:
    """``[s (n_out) | w0, w1 (n_out * 2)]`` of one axis: the bilinear form INTER_AREA takes when an axis enlarges (include/pcdm.h: rule 3);
    ``clamp_frac``: the x axis, where an index at the last column loses its fraction."""
    scale = cv_scale(n_in, n_out)
    inv = 1.0 / scale
    ofs, coeff = [], []
    for d in range(n_out):
        s = math.floor(d * scale)
        t = _F32((d + 1) - (s + 1) * inv)
        t = _F32(0) if t <= 0 else _F32(t - np.floor(t))
        if clamp_frac and s >= n_in - 1:
            s, t = n_in - 1, _F32(0)
        ofs.append(int(s))
        coeff += [_cv_fixed(_F32(_F32(1) - t)), _cv_fixed(t)]
    return ofs + coeff


_CV_TABLES: Dict[tuple, torch.Tensor] = {}


def _cv_table(n_in: int, n_out: int, rule: int, is_x: bool, device: torch.device) -> torch.Tensor:
    key = (n_in, n_out, rule, is_x and rule == ops.RESIZE_CV_AREA_LINEAR, str(device))
    if key not in _CV_TABLES:
        if rule == ops.RESIZE_CV_LANCZOS4:
            tab = cv_lanczos4_table(n_in, n_out)
        elif rule == ops.RESIZE_CV_AREA:
            tab = cv_area_table(n_in, n_out)
        else:
            tab = cv_area_linear_table(n_in, n_out, is_x)
        t = torch.empty(len(tab), dtype=torch.int32, device=device)
        t.copy_(torch.tensor(tab, dtype=torch.int32))
        _CV_TABLES[key] = t
    return _CV_TABLES[key]


def cv_area_rule(Hs: int, Ws: int, Hd: int, Wd: int) -> int:
    """The arithmetic ``cv2.resize(..., INTER_AREA)`` takes for these sizes: the integer-ratio box, true area, or -- when either axis enlarges --
    its bilinear emulation."""
    sx, sy = cv_scale(Ws, Wd), cv_scale(Hs, Hd)
    if sx >= 1.0 and sy >= 1.0:
        if abs(sx - round(sx)) < _DBL_EPSILON and abs(sy - round(sy)) < _DBL_EPSILON:
            return ops.RESIZE_CV_AREA_INT
        return ops.RESIZE_CV_AREA
    return ops.RESIZE_CV_AREA_LINEAR


def resize_cv(image_u8: torch.Tensor, size: Sequence[int], interpolation: str = "lanczos4") -> torch.Tensor:
    """``cv2.resize(image, size, interpolation=cv2.INTER_LANCZOS4 | cv2.INTER_AREA)`` on the device: uint8 ``[H, W, 3]`` or ``[M, H, W, 3]`` ->
    the same rank at ``size`` = ``(width, height)``.  ``"lanczos4"``: eight taps per axis in OpenCV's 8-bit fixed point, no antialiasing when
    reducing.  ``"area"``: what OpenCV picks for the sizes -- the integer box (2 x 2 in integers, otherwise one fp32 multiply), true area in fp32,
    or the 8-bit bilinear form when either axis enlarges.  Equal sizes copy.

    OpenCV is not a dependency: the rules are restated from its published generic path (include/pcdm.h: pcdm_resize_cv_u8) and checked against an
    independent restatement and their fp64 definitions (tests/test_resize_cv.py); coefficient details have differed between OpenCV releases, so
    parity with the ``cv2`` package itself is NOT pinned by a test here -- the same standing as ``resize_cv_cubic``.  The per-axis tables are built
    here on the host (the sines and cosines of Lanczos4 are never taken on the device), cached per ``(in, out, rule, device)`` and uploaded once;
    after that one launch, no host synchronisation."""
    if interpolation not in ("lanczos4", "area"):
        raise ValueError(f"interpolation must be 'lanczos4' or 'area', not {interpolation!r}")
    if image_u8.dim() not in (3, 4) or image_u8.shape[-1] != 3 or image_u8.dtype != torch.uint8:
        raise ValueError(f"an image is uint8 [H, W, 3] or [M, H, W, 3]: got {image_u8.dtype} {tuple(image_u8.shape)}")
    Wd, Hd = int(size[0]), int(size[1])
    if Wd <= 0 or Hd <= 0:
        raise ValueError(f"size must be positive: {tuple(size)}")
    src = (image_u8 if image_u8.dim() == 4 else image_u8.unsqueeze(0)).contiguous()
    M, Hs, Ws = (int(v) for v in src.shape[:3])
    if Hs <= 0 or Ws <= 0:
        raise ValueError(f"empty image: {tuple(image_u8.shape)}")
    rule = ops.RESIZE_CV_LANCZOS4 if interpolation == "lanczos4" else cv_area_rule(Hs, Ws, Hd, Wd)
    xtab = ytab = None
    if (Hs, Ws) != (Hd, Wd) and rule != ops.RESIZE_CV_AREA_INT:
        xtab, ytab = _cv_table(Ws, Wd, rule, True, src.device), _cv_table(Hs, Hd, rule, False, src.device)
    out = torch.empty((M, Hd, Wd, 3), dtype=torch.uint8, device=src.device)
    ops.resize_cv_u8(src, out, rule, xtab, ytab)
    return out if image_u8.dim() == 4 else out[0]
