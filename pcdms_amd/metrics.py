"""Image metrics of the evaluation drivers on the device: Gaussian-weighted SSIM, PSNR, LPIPS (AlexNet) and the best-of-N sample pick.

The reference's drivers decode N samples per pair, copy them to the host and keep the one with the best
``skimage.metrics.structural_similarity(..., gaussian_weights=True, sigma=1.2, use_sample_covariance=False)`` against the target
(stage2_batchtest_inpaint_model.py:203-219).  Here the decoded uint8 NHWC batch (``output_type="uint8"``) is scored where it lies by the HIP
kernels of csrc/misc.hip (include/pcdm.h: pcdm_ssim / pcdm_psnr / pcdm_select_image); nothing in this module synchronises with the host, so
``pick_best`` can sit in the middle of a device-resident chain or inside a captured graph.

Images are NHWC with 3 channels, uint8 or fp32 (candidates and reference the same type): ``cand`` [N, H, W, 3] (or [H, W, 3]), ``ref``
[1 | N, H', W', 3] (or [H', W', 3]).  A window is ``(x0, y0, W, H)`` into its own image and defaults to the whole image -- the right half of a
[source | target] canvas is scored against a stand-alone target with no crop copy.

``LPIPS`` is the paper's second per-pair metric (the reference's metrics.py calls the ``lpips`` package): LPIPS v0.1 with the AlexNet trunk in
exact fp32 on the fp32-input MFMA (include/pcdm.h: pcdm_lpips).  Neither ``lpips`` nor ``torchvision`` is a dependency: the network is restated
from its published definition and checked against an fp64 restatement with synthetic weights (tests/test_lpips.py), so parity with the upstream
packages on their checkpoints is NOT pinned by a test here -- the same standing as the diffusers restatements.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib, ops

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
              out: str = "uint8", metric: str = "ssim", lpips: Optional["LPIPS"] = None,
              normalize: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(image, index, scores)``, all on the device: the window of the candidate with the best SSIM (``np.argmax`` rules: the first maximum
    wins, a NaN score ranks as the maximum), its index (int32 [1]) and the fp32 [N] scores.  ``out="uint8"``: image uint8 [H, W, 3];
    ``out="normalized"``: fp32 [1, 3, H, W] = (x / 255 - 0.5) / 0.5, the drivers' ``to_tensor_normalized`` -- the stage-3 input.
    ``metric="lpips"`` with ``lpips=`` an ``LPIPS`` model: the candidate with the LOWEST LPIPS instead (``np.argmin`` rules: the first minimum
    wins, a NaN ranks as the minimum; ``normalize`` as in ``LPIPS.__call__``); ``sigma`` is not used then."""
    if out not in ("uint8", "normalized"):
        raise ValueError(f"out must be 'uint8' or 'normalized', not {out!r}")
    if metric not in ("ssim", "lpips"):
        raise ValueError(f"metric must be 'ssim' or 'lpips', not {metric!r}")
    if (metric == "lpips") != (lpips is not None):
        raise ValueError("metric='lpips' needs lpips=<an LPIPS model>, and only that metric takes one")
    cand, ref, cw, rw = _prep(cand, ref, cand_window, ref_window)
    if cand.dtype != torch.uint8:
        raise ValueError("pick_best selects from uint8 candidates")
    dev = cand.device
    index = torch.empty(1, dtype=torch.int32, device=dev)
    if metric == "lpips":
        scores = lpips._run(cand, ref, cw, rw, normalize, index)[0]
    else:
        scores = torch.empty(cand.shape[0], dtype=torch.float32, device=dev)
        ops.ssim(cand, ref, cw, rw, scores, index, _workspace(cand, ref, cw, sigma), sigma=sigma)
    W, H = cw[2], cw[3]
    image = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev) if out == "normalized" else torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    ops.select_image(cand, cw, index, image, out == "normalized")
    return image, index, scores


# ------------------------------------------------------------------------------------------------ LPIPS
_LPIPS_SHIFT, _LPIPS_SCALE = (-.030, -.088, -.188), (.458, .448, .450)
_ALEX_CONVS = ((64, 3, 11), (192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3))     # (Cout, Cin, k) of conv1..5 = the five taps
_LPIPS_SLICES = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")   # the lpips package's names
_ALEX_FEATURES = ("features.0", "features.3", "features.6", "features.8", "features.10")            # torchvision's alexnet


class LPIPS:
    """LPIPS v0.1, ``net="alex"``, eval mode, on the device.  ``model(img0, img1)`` -> fp32 [N, 1, 1, 1] (the ``lpips`` package's shape, so the
    reference's ``[:, 0, 0, 0].mean()`` works unchanged).

    Images: fp32 NCHW [N, 3, H, W] (as the package takes them) or uint8 NHWC [N, H, W, 3] (as the decoder leaves them; x = p / 255), both the same
    type; ``img1`` may have batch 1 and is then compared with every image of ``img0``.  ``normalize=True`` maps [0, 1] inputs to the [-1, 1] the
    network was trained on (x <- 2 x - 1).  **The reference's evaluation does not**: ``LPIPS.calculate_from_disk`` (metrics.py:484-498) feeds
    [0, 1] images without the remap, so ``normalize=False`` on uint8 images reproduces the number the reference's evaluation prints, and
    ``normalize=True`` is LPIPS as its authors define it.  That quirk is reproduced, not corrected.  H, W >= 31."""

    def __init__(self, net: str = "alex"):
        if net != "alex":
            raise NotImplementedError(f"only net='alex' is implemented (the reference's evaluation uses it), not {net!r}")
        self.net = net
        self.packed: Dict[str, torch.Tensor] = {}      # host tensors: conv{l}.w / conv{l}.bias in the library's layout, lin{l}
        self._dev: Dict[str, tuple] = {}               # device -> (tensors, pcdm_lpips_weights)

    # -- weights
    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> "LPIPS":
        """The ``lpips`` package's layout (``net.slice1.0.weight`` ... ``net.slice5.10.bias``, ``lin{0..4}.model.1.weight``; the duplicate
        ``lins.*`` keys are ignored, ``scaling_layer.shift`` / ``.scale`` must equal the constants) or the two-file form merged into one dict
        (torchvision's ``features.{0,3,6,8,10}.*`` + the ``lin*.model.1.weight`` of the package's ``alex.pth``)."""
        names = _LPIPS_SLICES if f"{_LPIPS_SLICES[0]}.weight" in sd else _ALEX_FEATURES
        for key, want in (("scaling_layer.shift", _LPIPS_SHIFT), ("scaling_layer.scale", _LPIPS_SCALE)):
            if key in sd and not torch.equal(sd[key].detach().flatten().to("cpu", torch.float32), torch.tensor(want, dtype=torch.float32)):
                raise ValueError(f"{key} = {sd[key].flatten().tolist()} is not LPIPS v0.1's {want}: the kernel applies the constants")
        packed: Dict[str, torch.Tensor] = {}
        for l, (name, (cout, cin, k)) in enumerate(zip(names, _ALEX_CONVS)):
            for suffix in ("weight", "bias"):
                if f"{name}.{suffix}" not in sd:
                    raise KeyError(f"{name}.{suffix} is missing (neither the lpips layout nor torchvision features + lin weights)")
            w, b = sd[f"{name}.weight"], sd[f"{name}.bias"]
            if tuple(w.shape) != (cout, cin, k, k) or tuple(b.shape) != (cout,):
                raise ValueError(f"{name}: weight {tuple(w.shape)} / bias {tuple(b.shape)}, AlexNet has {(cout, cin, k, k)} / {(cout,)}")
            pw = ops.pack_lpips_conv(w, b, "cpu")
            packed[f"conv{l}.w"], packed[f"conv{l}.bias"] = pw["w"], pw["bias"]
            if f"lin{l}.model.1.weight" not in sd:
                raise KeyError(f"lin{l}.model.1.weight is missing")
            lin = sd[f"lin{l}.model.1.weight"]
            if lin.numel() != cout or tuple(lin.shape) not in ((1, cout, 1, 1), (cout,)):
                raise ValueError(f"lin{l}.model.1.weight {tuple(lin.shape)}, expected (1, {cout}, 1, 1)")
            packed[f"lin{l}"] = lin.detach().to("cpu", torch.float32).reshape(cout).contiguous().clone()
        self.packed, self._dev = packed, {}
        return self

    @classmethod
    def from_pretrained(cls, path, lin_path=None, net: str = "alex") -> "LPIPS":
        """A ``.pth`` / ``.pt`` / ``.bin`` (torch.load) or ``.safetensors`` file in either layout; the two-file form passes torchvision's alexnet
        checkpoint as ``path`` and the package's ``alex.pth`` as ``lin_path``."""
        def read(p):
            if str(p).endswith(".safetensors"):
                from safetensors.torch import load_file
                return load_file(str(p))
            return torch.load(str(p), map_location="cpu", weights_only=True)
        sd = dict(read(path))
        if lin_path is not None:
            sd.update(read(lin_path))
        return cls(net).load_state_dict(sd)

    def _weights(self, device: torch.device):
        if not self.packed:
            raise RuntimeError("LPIPS has no weights: load_state_dict / from_pretrained first")
        key = str(device)
        if key not in self._dev:
            t = {k: v.to(device) for k, v in self.packed.items()}
            w = _lib.LpipsWeights()
            for l in range(5):
                w.conv_w[l], w.conv_b[l], w.lin[l] = t[f"conv{l}.w"].data_ptr(), t[f"conv{l}.bias"].data_ptr(), t[f"lin{l}"].data_ptr()
            self._dev[key] = (t, w)
        return self._dev[key][1]

    # -- forward
    def _run(self, img0, img1, w0, w1, normalize, argmin=None):
        N, dev = img0.shape[0], img0.device
        if img1.shape[0] not in (1, N):
            raise ValueError(f"img1 has batch {img1.shape[0]}: 1 or img0's {N}")
        if (w0[2], w0[3]) != (w1[2], w1[3]):
            raise ValueError(f"the two windows differ in size: {w0[2:]} and {w1[2:]}")
        nbytes = ops.lpips_ws_bytes(N, img1.shape[0], w0[3], w0[2])
        if nbytes < 0:
            raise ValueError(f"LPIPS (alex) needs windows of at least 31 x 31 pixels (the second max-pool): got {w0[2]} x {w0[3]} (W x H), batch {N}")
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        out = torch.empty(N, dtype=torch.float32, device=dev)
        layers = torch.empty((5, N), dtype=torch.float32, device=dev)
        ops.lpips(img0, img1, w0, w1, self._weights(dev), out, layers, argmin, ws, normalize=normalize)
        return out, layers

    def __call__(self, img0: torch.Tensor, img1: torch.Tensor, normalize: bool = False, cand_window: Window = None, ref_window: Window = None,
                 return_layers: bool = False):
        if img0.dim() != 4 or img1.dim() != 4 or img0.dtype != img1.dtype or img0.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"images are fp32 [N, 3, H, W] or uint8 [N, H, W, 3], both the same: got {tuple(img0.shape)} {img0.dtype} and "
                             f"{tuple(img1.shape)} {img1.dtype}")
        if img0.device != img1.device:
            raise ValueError(f"img0 on {img0.device}, img1 on {img1.device}")
        hw = (lambda t: (t.shape[2], t.shape[3])) if img0.dtype == torch.float32 else (lambda t: (t.shape[1], t.shape[2]))
        chan = 1 if img0.dtype == torch.float32 else 3
        if img0.shape[chan] != 3 or img1.shape[chan] != 3:
            raise ValueError(f"three channels expected: got {tuple(img0.shape)} and {tuple(img1.shape)}")
        w0 = tuple(int(v) for v in cand_window) if cand_window is not None else (0, 0, hw(img0)[1], hw(img0)[0])
        w1 = tuple(int(v) for v in ref_window) if ref_window is not None else (0, 0, hw(img1)[1], hw(img1)[0])
        out, layers = self._run(img0.contiguous(), img1.contiguous(), w0, w1, bool(normalize))
        out = out.view(-1, 1, 1, 1)
        return (out, layers) if return_layers else out

    forward = __call__
