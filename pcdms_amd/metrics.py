"""Image metrics of the evaluation drivers on the device: Gaussian-weighted SSIM, PSNR and the best-of-N sample pick.

The reference's drivers decode N samples per pair, copy them to the host and keep the one with the best
``skimage.metrics.structural_similarity(..., gaussian_weights=True, sigma=1.2, use_sample_covariance=False)`` against the target
(stage2_batchtest_inpaint_model.py:203-219).  Here the decoded uint8 NHWC batch (``output_type="uint8"``) is scored where it lies by the HIP
kernels of csrc/misc.hip (include/pcdm.h: pcdm_ssim / pcdm_psnr / pcdm_select_image); nothing in this module synchronises with the host, so
``pick_best`` can sit in the middle of a device-resident chain or inside a captured graph.

Images are NHWC with 3 channels, uint8 or fp32 (candidates and reference the same type): ``cand`` [N, H, W, 3] (or [H, W, 3]), ``ref``
[1 | N, H', W', 3] (or [H', W', 3]).  A window is ``(x0, y0, W, H)`` into its own image and defaults to the whole image -- the right half of a
[source | target] canvas is scored against a stand-alone target with no crop copy.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import ops

Window = Optional[Sequence[int]]


def _prep(cand: torch.Tensor, ref: torch.Tensor, cand_window: Window, ref_window: Window):
    if cand.dim() == 3:
        cand = cand.unsqueeze(0)
    if ref.dim() == 3:
        ref = ref.unsqueeze(0)
    if cand.dim() != 4 or ref.dim() != 4:
        raise ValueError(f"images are NHWC [N, H, W, 3]: got {tuple(cand.shape)} and {tuple(ref.shape)}")
    if cand.dtype != ref.dtype or cand.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"candidates and reference must both be uint8 or both fp32: got {cand.dtype} and {ref.dtype}")
    if cand.device != ref.device:
        raise ValueError(f"candidates on {cand.device}, reference on {ref.device}")
    cw = tuple(int(v) for v in cand_window) if cand_window is not None else (0, 0, cand.shape[2], cand.shape[1])
    rw = tuple(int(v) for v in ref_window) if ref_window is not None else (0, 0, ref.shape[2], ref.shape[1])
    return cand.contiguous(), ref.contiguous(), cw, rw


def _workspace(cand: torch.Tensor, ref: torch.Tensor, cw, sigma: float) -> torch.Tensor:
    n = ops.metrics_ws_bytes(cand.shape[0], ref.shape[0], cw[2], cw[3], sigma)
    # (a refused problem still reaches the library, which answers -1 and writes nothing)
    return torch.empty(max(n, 8) // 8, dtype=torch.float64, device=cand.device)


def ssim(cand: torch.Tensor, ref: torch.Tensor, *, sigma: float = 1.2, data_range: Optional[float] = None, cand_window: Window = None,
         ref_window: Window = None) -> torch.Tensor:
    """fp32 [N] on the device: skimage's Gaussian-weighted SSIM of every candidate against the reference.  ``data_range`` None: max - min of
    the candidate's window (what the drivers pass)."""
    cand, ref, cw, rw = _prep(cand, ref, cand_window, ref_window)
    scores = torch.empty(cand.shape[0], dtype=torch.float32, device=cand.device)
    return ops.ssim(cand, ref, cw, rw, scores, None, _workspace(cand, ref, cw, sigma), sigma=sigma, data_range=data_range)


def psnr(cand: torch.Tensor, ref: torch.Tensor, *, data_range: float = 255, cand_window: Window = None, ref_window: Window = None) -> torch.Tensor:
    """fp32 [N] on the device: 10 log10(data_range^2 / mse) per candidate, +inf for identical windows."""
    cand, ref, cw, rw = _prep(cand, ref, cand_window, ref_window)
    out = torch.empty(cand.shape[0], dtype=torch.float32, device=cand.device)
    return ops.psnr(cand, ref, cw, rw, None, out, _workspace(cand, ref, cw, 0.0), data_range=data_range)


def mse(cand: torch.Tensor, ref: torch.Tensor, *, cand_window: Window = None, ref_window: Window = None) -> torch.Tensor:
    """fp32 [N] on the device: mean squared difference per candidate (exact integer accumulation for uint8)."""
    cand, ref, cw, rw = _prep(cand, ref, cand_window, ref_window)
    out = torch.empty(cand.shape[0], dtype=torch.float32, device=cand.device)
    ops.psnr(cand, ref, cw, rw, out, None, _workspace(cand, ref, cw, 0.0), data_range=255.0)
    return out


def pick_best(cand: torch.Tensor, ref: torch.Tensor, *, cand_window: Window = None, ref_window: Window = None, sigma: float = 1.2,
              out: str = "uint8") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(image, index, scores)``, all on the device: the window of the candidate with the best SSIM (``np.argmax`` rules: the first maximum
    wins, a NaN score ranks as the maximum), its index (int32 [1]) and the fp32 [N] scores.  ``out="uint8"``: image uint8 [H, W, 3];
    ``out="normalized"``: fp32 [1, 3, H, W] = (x / 255 - 0.5) / 0.5, the drivers' ``to_tensor_normalized`` -- the stage-3 input."""
    if out not in ("uint8", "normalized"):
        raise ValueError(f"out must be 'uint8' or 'normalized', not {out!r}")
    cand, ref, cw, rw = _prep(cand, ref, cand_window, ref_window)
    if cand.dtype != torch.uint8:
        raise ValueError("pick_best selects from uint8 candidates")
    dev = cand.device
    scores = torch.empty(cand.shape[0], dtype=torch.float32, device=dev)
    index = torch.empty(1, dtype=torch.int32, device=dev)
    ops.ssim(cand, ref, cw, rw, scores, index, _workspace(cand, ref, cw, sigma), sigma=sigma)
    W, H = cw[2], cw[3]
    image = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev) if out == "normalized" else torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    ops.select_image(cand, cw, index, image, out == "normalized")
    return image, index, scores
