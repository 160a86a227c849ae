"""Image metrics of the evaluation drivers on the device: Gaussian-weighted SSIM, PSNR, LPIPS (AlexNet) and the best-of-N sample pick.

The reference's drivers decode N samples per pair, copy them to the host and keep the one with the best
``skimage.metrics.structural_similarity(..., gaussian_weights=True, sigma=1.2, use_sample_covariance=False)`` against the target
(stage2_batchtest_inpaint_model.py:203-219).  Here the decoded uint8 NHWC batch (``output_type="uint8"``) is scored where it lies by the HIP
kernels of csrc/image_metrics.hip (include/pcdm.h: pcdm_ssim / pcdm_psnr / pcdm_select_image); nothing in this module synchronises with the host, so
``pick_best`` can sit in the middle of a device-resident chain or inside a captured graph.

Images are NHWC with 3 channels, uint8 or fp32 (candidates and reference the same type): ``cand`` [N, H, W, 3] (or [H, W, 3]), ``ref``
[1 | N, H', W', 3] (or [H', W', 3]).  A window is ``(x0, y0, W, H)`` into its own image and defaults to the whole image -- the right half of a
[source | target] canvas is scored against a stand-alone target with no crop copy.

``LPIPS`` is the paper's second per-pair metric (the reference's metrics.py calls the ``lpips`` package): LPIPS v0.1 with the AlexNet trunk in
exact fp32 on the fp32-input MFMA (csrc/eval_nets.hip; include/pcdm.h: pcdm_lpips).  Neither ``lpips`` nor ``torchvision`` is a dependency: the network is restated
from its published definition and checked against an fp64 restatement with synthetic weights (tests/test_lpips.py), so parity with the upstream
packages on their checkpoints is NOT pinned by a test here -- the same standing as the diffusers restatements.

``InceptionV3Features`` / ``FIDStatistics`` / ``frechet_distance`` / ``FID`` are the third metric, the reference's FID (inception.py,
metrics.py:23-257): the InceptionV3 trunk in exact fp32 and the fp64 statistics on the device (csrc/eval_nets.hip; include/pcdm.h: pcdm_inception_features,
pcdm_fid_accumulate, pcdm_fid_finalize), the Frechet distance itself on the host in fp64.  Same standing: restated, checked on synthetic weights
(tests/test_fid.py), parity with torchvision's checkpoint not pinned.

``l1`` / ``mae`` / ``ssim_box`` are the remaining per-pair numbers of the reference's metric scripts (metrics.py: compare_l1, compare_mae and the
``ssim`` array: skimage's uniform 51 x 51 window with the sample covariance; include/pcdm.h: pcdm_absdiff, pcdm_ssim_box);
tools/calculate_metrics.py is the whole script.  Same standing: restated, checked against fp64 (tests/test_eval_metrics.py), scikit-image parity
not pinned.
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


def l1(cand: torch.Tensor, ref: torch.Tensor, *, cand_window: Window = None, ref_window: Window = None) -> torch.Tensor:
    """fp32 [N] on the device: the reference's ``compare_l1``, ``mean |a - b|`` per candidate (fp64 sums; exact integer sums for uint8)."""
    cand, ref, cw, rw = _prep(cand, ref, cand_window, ref_window)
    out = torch.empty(cand.shape[0], dtype=torch.float32, device=cand.device)
    ops.absdiff(cand, ref, cw, rw, out, None, _workspace(cand, ref, cw, 0.0))
    return out


def mae(cand: torch.Tensor, ref: torch.Tensor, *, cand_window: Window = None, ref_window: Window = None) -> torch.Tensor:
    """fp32 [N] on the device: the reference's ``compare_mae``, ``sum |a - b| / sum (a + b)`` per candidate; NaN or inf where the denominator is
    zero, as numpy divides."""
    cand, ref, cw, rw = _prep(cand, ref, cand_window, ref_window)
    out = torch.empty(cand.shape[0], dtype=torch.float32, device=cand.device)
    ops.absdiff(cand, ref, cw, rw, None, out, _workspace(cand, ref, cw, 0.0))
    return out


def ssim_box(cand: torch.Tensor, ref: torch.Tensor, *, win_size: int = 51, data_range: Optional[float] = None, cand_window: Window = None,
             ref_window: Window = None) -> torch.Tensor:
    """fp32 [N] on the device: ``skimage.metrics.structural_similarity(ref, cand[n], win_size=win_size, data_range=data_range, channel_axis=2)``
    with skimage's defaults -- a ``win_size`` x ``win_size`` uniform window and the sample covariance; the ``ssim`` array of the reference's
    ``<W>_<H>_metrics.npz`` (win_size 51, data_range 1).  ``win_size`` odd, 3 .. 51, not larger than the window; ``data_range`` None: max - min of
    the candidate's window.  scikit-image is not a dependency: restated and checked against an fp64 restatement (tests/test_eval_metrics.py),
    parity with the package itself NOT pinned -- the same standing as LPIPS and FID."""
    cand, ref, cw, rw = _prep(cand, ref, cand_window, ref_window)
    n = ops.ssim_box_ws_bytes(cand.shape[0], ref.shape[0], cw[2], cw[3], win_size)
    ws = torch.empty(max(n, 8) // 8, dtype=torch.float64, device=cand.device)     # (a refused problem still reaches the library: -1, nothing written)
    scores = torch.empty(cand.shape[0], dtype=torch.float32, device=cand.device)
    return ops.ssim_box(cand, ref, cw, rw, scores, ws, win_size=win_size, data_range=data_range)


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
                w.conv_w[l], w.conv_b[l], w.lin[l] = ops._ptr(t[f"conv{l}.w"]), ops._ptr(t[f"conv{l}.bias"]), ops._ptr(t[f"lin{l}"])
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


# ------------------------------------------------------------------------------------------------ FID
def _inception_convs():
    """(name, Cout, Cin, kh, kw) of the 94 BasicConv2d of torchvision's inception_v3 trunk in module order = pcdm_inception_weights' order."""
    convs = [("Conv2d_1a_3x3", 32, 3, 3, 3), ("Conv2d_2a_3x3", 32, 32, 3, 3), ("Conv2d_2b_3x3", 64, 32, 3, 3), ("Conv2d_3b_1x1", 80, 64, 1, 1),
             ("Conv2d_4a_3x3", 192, 80, 3, 3)]
    for name, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        convs += [(f"{name}.{b}", co, ci, kh, kw) for b, co, ci, kh, kw in (
            ("branch1x1", 64, cin, 1, 1), ("branch5x5_1", 48, cin, 1, 1), ("branch5x5_2", 64, 48, 5, 5), ("branch3x3dbl_1", 64, cin, 1, 1),
            ("branch3x3dbl_2", 96, 64, 3, 3), ("branch3x3dbl_3", 96, 96, 3, 3), ("branch_pool", pf, cin, 1, 1))]
    convs += [(f"Mixed_6a.{b}", co, ci, 3 if b != "branch3x3dbl_1" else 1, 3 if b != "branch3x3dbl_1" else 1) for b, co, ci in (
        ("branch3x3", 384, 288), ("branch3x3dbl_1", 64, 288), ("branch3x3dbl_2", 96, 64), ("branch3x3dbl_3", 96, 96))]
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        convs += [(f"{name}.{b}", co, ci, kh, kw) for b, co, ci, kh, kw in (
            ("branch1x1", 192, 768, 1, 1), ("branch7x7_1", c7, 768, 1, 1), ("branch7x7_2", c7, c7, 1, 7), ("branch7x7_3", 192, c7, 7, 1),
            ("branch7x7dbl_1", c7, 768, 1, 1), ("branch7x7dbl_2", c7, c7, 7, 1), ("branch7x7dbl_3", c7, c7, 1, 7), ("branch7x7dbl_4", c7, c7, 7, 1),
            ("branch7x7dbl_5", 192, c7, 1, 7), ("branch_pool", 192, 768, 1, 1))]
    convs += [(f"Mixed_7a.{b}", co, ci, kh, kw) for b, co, ci, kh, kw in (
        ("branch3x3_1", 192, 768, 1, 1), ("branch3x3_2", 320, 192, 3, 3), ("branch7x7x3_1", 192, 768, 1, 1), ("branch7x7x3_2", 192, 192, 1, 7),
        ("branch7x7x3_3", 192, 192, 7, 1), ("branch7x7x3_4", 192, 192, 3, 3))]
    for name, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        convs += [(f"{name}.{b}", co, ci, kh, kw) for b, co, ci, kh, kw in (
            ("branch1x1", 320, cin, 1, 1), ("branch3x3_1", 384, cin, 1, 1), ("branch3x3_2a", 384, 384, 1, 3), ("branch3x3_2b", 384, 384, 3, 1),
            ("branch3x3dbl_1", 448, cin, 1, 1), ("branch3x3dbl_2", 384, 448, 3, 3), ("branch3x3dbl_3a", 384, 384, 1, 3),
            ("branch3x3dbl_3b", 384, 384, 3, 1), ("branch_pool", 192, cin, 1, 1))]
    assert len(convs) == 94
    return tuple(convs)


INCEPTION_CONVS = _inception_convs()
INCEPTION_CONVS_BY_DIM = {64: 3, 192: 5, 768: 70, 2048: 94}      # the reference's BLOCK_INDEX_BY_DIM: how many convolutions each output needs
BN_EPS = 1e-3


class InceptionV3Features:
    """The feature extractor of the reference's FID (inception.py: ``InceptionV3([BLOCK_INDEX_BY_DIM[dims]])`` followed by the spatial mean that
    metrics.py applies): torchvision's ``inception_v3`` trunk, eval mode, in exact fp32 on the device.  ``model(images)`` -> fp32 ``[N, dims]``.

    Images are in [0, 1]: fp32 NCHW [N, 3, H, W] or uint8 NHWC [N, H, W, 3] (x = p / 255), optionally a ``window`` (x0, y0, W, H) of them, as
    ``LPIPS`` takes them.  ``resize_input``: ``F.upsample(x, (299, 299), mode='bilinear')`` (align_corners False, no antialias);
    ``False`` feeds the window at its own size (at least 75 x 75 for ``dims=2048``).  ``normalize_input``: the reference's remap
    ``x[c] * (s_c / 0.5) + (m_c - 0.5) / 0.5``.  **Torchvision means that formula for [-1, 1] inputs; the reference feeds it [0, 1] images.**  The
    quirk is reproduced, not corrected, as LPIPS's is.  Every BatchNorm (eps 1e-3, running statistics) is folded into its convolution's weight
    and bias in fp64 and rounded to fp32 once.  ``torchvision`` is not a dependency; the trunk is checked against an fp64 restatement with
    synthetic weights (tests/test_fid.py), so parity with torchvision on its checkpoint is NOT pinned here."""

    def __init__(self, dims: int = 2048, resize_input: bool = True, normalize_input: bool = True):
        if dims not in INCEPTION_CONVS_BY_DIM:
            raise ValueError(f"dims must be one of {sorted(INCEPTION_CONVS_BY_DIM)} (the reference's BLOCK_INDEX_BY_DIM), not {dims!r}")
        self.dims, self.resize_input, self.normalize_input = dims, bool(resize_input), bool(normalize_input)
        self.packed: list = []                         # host: per convolution {"w", "bias"} in the library's layout
        self._dev: Dict[str, tuple] = {}

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> "InceptionV3Features":
        """torchvision's ``inception_v3`` layout: ``<layer>.conv.weight`` and ``<layer>.bn.{weight, bias, running_mean, running_var}`` for the
        convolutions this ``dims`` needs; ``AuxLogits.*``, ``fc.*``, ``num_batches_tracked`` and later layers are ignored."""
        packed = []
        for name, cout, cin, kh, kw in INCEPTION_CONVS[:INCEPTION_CONVS_BY_DIM[self.dims]]:
            keys = [f"{name}.conv.weight"] + [f"{name}.bn.{k}" for k in ("weight", "bias", "running_mean", "running_var")]
            for k in keys:
                if k not in sd:
                    raise KeyError(f"{k} is missing (torchvision's inception_v3 layout)")
            w, (g, b, m, v) = sd[keys[0]], (sd[k] for k in keys[1:])
            if tuple(w.shape) != (cout, cin, kh, kw):
                raise ValueError(f"{name}.conv.weight: shape {tuple(w.shape)}, InceptionV3 has {(cout, cin, kh, kw)}")
            for k, t in zip(keys[1:], (g, b, m, v)):
                if tuple(t.shape) != (cout,):
                    raise ValueError(f"{k}: shape {tuple(t.shape)}, InceptionV3 has {(cout,)}")
            g, b, m, v = (t.detach().to("cpu", torch.float64) for t in (g, b, m, v))
            scale = g / torch.sqrt(v + BN_EPS)
            wf = (w.detach().to("cpu", torch.float64) * scale.view(-1, 1, 1, 1)).to(torch.float32)
            pw = ops.pack_lpips_conv(wf, (b - m * scale).to(torch.float32), "cpu")
            packed.append({"w": pw["w"], "bias": pw["bias"]})
        self.packed, self._dev = packed, {}
        return self

    @classmethod
    def from_pretrained(cls, path, dims: int = 2048, resize_input: bool = True, normalize_input: bool = True) -> "InceptionV3Features":
        """A ``.pth`` / ``.pt`` (torch.load) or ``.safetensors`` file of torchvision's ``inception_v3`` state dict."""
        if str(path).endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(str(path))
        else:
            sd = torch.load(str(path), map_location="cpu", weights_only=True)
        return cls(dims, resize_input, normalize_input).load_state_dict(dict(sd))

    def _weights(self, device: torch.device):
        if not self.packed:
            raise RuntimeError("InceptionV3Features has no weights: load_state_dict / from_pretrained first")
        key = str(device)
        if key not in self._dev:
            t = [{k: v.to(device) for k, v in p.items()} for p in self.packed]
            w = _lib.InceptionWeights()
            for i, p in enumerate(t):
                w.w[i], w.bias[i] = ops._ptr(p["w"]), ops._ptr(p["bias"])
            self._dev[key] = (t, w)
        return self._dev[key][1]

    def __call__(self, images: torch.Tensor, window: Window = None) -> torch.Tensor:
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"images are fp32 [N, 3, H, W] or uint8 [N, H, W, 3]: got {getattr(images, 'dtype', type(images))} "
                             f"{tuple(getattr(images, 'shape', ()))}")
        f32 = images.dtype == torch.float32
        H, W = (images.shape[2], images.shape[3]) if f32 else (images.shape[1], images.shape[2])
        if images.shape[1 if f32 else 3] != 3:
            raise ValueError(f"three channels expected: got {tuple(images.shape)}")
        win = tuple(int(v) for v in window) if window is not None else (0, 0, W, H)
        if len(win) != 4 or win[0] < 0 or win[1] < 0 or win[2] < 1 or win[3] < 1 or win[0] + win[2] > W or win[1] + win[3] > H:
            raise ValueError(f"window {win} (x0, y0, W, H) does not lie inside the {W} x {H} image")
        N, dev = images.shape[0], images.device
        weights = self._weights(dev)
        h, w = (299, 299) if self.resize_input else (win[3], win[2])
        nbytes = ops.inception_ws_bytes(N, h, w, self.dims)
        if nbytes < 0:
            raise ValueError(f"InceptionV3 (dims={self.dims}) cannot take a batch of {N} inputs of {w} x {h} (W x H): without resize_input the full "
                             "trunk needs at least 75 x 75 pixels")
        ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
        out = torch.empty((N, self.dims), dtype=torch.float32, device=dev)
        return ops.inception_features(images.contiguous(), win, weights, out, ws, dims=self.dims, resize=self.resize_input,
                                      normalize=self.normalize_input)

    forward = __call__


class FIDStatistics:
    """Running fp64 sum and Gram matrix of feature rows on the device; ``finalize()`` -> ``(mu, sigma)`` = ``np.mean(act, 0)``,
    ``np.cov(act, rowvar=False)`` in fp64.  One thread owns each entry and adds the samples in order, so the state is bit-identical however the
    samples are split into batches.  ``save`` / ``load`` use the reference's ``.npz`` format (keys ``mu``, ``sigma``)."""

    def __init__(self, dims: int):
        self.dims, self.count = int(dims), 0
        self.sum: Optional[torch.Tensor] = None
        self.gram: Optional[torch.Tensor] = None
        self._final: Optional[Tuple[torch.Tensor, torch.Tensor]] = None      # a loaded file: nothing to accumulate

    def update(self, features: torch.Tensor) -> "FIDStatistics":
        if self._final is not None:
            raise RuntimeError("statistics loaded from a file cannot take more samples")
        if features.dim() != 2 or features.shape[1] != self.dims or features.dtype != torch.float32:
            raise ValueError(f"features are fp32 [N, {self.dims}]: got {features.dtype} {tuple(features.shape)}")
        if self.sum is None:
            self.sum = torch.zeros(self.dims, dtype=torch.float64, device=features.device)
            self.gram = torch.zeros((self.dims, self.dims), dtype=torch.float64, device=features.device)
        elif self.sum.device != features.device:
            raise ValueError(f"features on {features.device}, statistics on {self.sum.device}")
        if features.shape[0]:
            ops.fid_accumulate(features.contiguous(), self.sum, self.gram)
            self.count += features.shape[0]
        return self

    def finalize(self) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._final is not None:
            return self._final
        if self.count < 2:
            raise ValueError(f"a covariance needs at least two samples: {self.count} accumulated")
        return ops.fid_finalize(self.sum, self.gram, self.count)

    def save(self, path) -> None:
        import numpy as np
        mu, sigma = self.finalize()
        with open(path, "wb") as f:      # (a file object: np.savez would append ".npz" to a bare name)
            np.savez(f, mu=mu.cpu().numpy(), sigma=sigma.cpu().numpy())

    @classmethod
    def load(cls, path) -> "FIDStatistics":
        import numpy as np
        with np.load(str(path)) as f:
            mu, sigma = torch.from_numpy(np.asarray(f["mu"], dtype=np.float64)), torch.from_numpy(np.asarray(f["sigma"], dtype=np.float64))
        if mu.dim() != 1 or tuple(sigma.shape) != (mu.shape[0], mu.shape[0]):
            raise ValueError(f"{path}: mu {tuple(mu.shape)}, sigma {tuple(sigma.shape)}")
        st = cls(mu.shape[0])
        st._final = (mu, sigma)
        return st


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """d^2 = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2), on the host in fp64.  S1 S2 is similar to the symmetric positive semi-definite
    S1^1/2 S2 S1^1/2, so tr sqrt(S1 S2) is the sum of the square roots of that matrix's eigenvalues (clamped at 0), from two
    ``torch.linalg.eigh`` on the CPU.  This replaces the reference's ``scipy.linalg.sqrtm(S1 S2)`` with its "singular product" retry on
    S + eps I and its discarded imaginary part: no scipy, no fallback, finite for rank-deficient covariances (fewer samples than features); the
    two agree wherever ``sqrtm`` is finite."""
    def t(a):
        return (a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(a)).to("cpu", torch.float64)
    mu1, sigma1, mu2, sigma2 = t(mu1).flatten(), t(sigma1), t(mu2).flatten(), t(sigma2)
    D = mu1.shape[0]
    if mu2.shape[0] != D or tuple(sigma1.shape) != (D, D) or tuple(sigma2.shape) != (D, D):
        raise ValueError(f"mean and covariance shapes differ: {tuple(mu1.shape)} {tuple(sigma1.shape)} {tuple(mu2.shape)} {tuple(sigma2.shape)}")
    w, v = torch.linalg.eigh((sigma1 + sigma1.T) / 2)
    root1 = (v * w.clamp_min(0).sqrt()) @ v.T
    m = root1 @ ((sigma2 + sigma2.T) / 2) @ root1
    tr_sqrt = torch.linalg.eigvalsh((m + m.T) / 2).clamp_min(0).sqrt().sum()
    diff = mu1 - mu2
    return float(diff.dot(diff) + torch.trace(sigma1) + torch.trace(sigma2) - 2 * tr_sqrt)


class FID:
    """``FID(model)`` with ``model`` an ``InceptionV3Features``: ``statistics(batches)`` runs every image batch through the trunk and accumulates
    on the device; ``fid(a, b)`` is the Frechet distance of two ``FIDStatistics`` (or ``(mu, sigma)`` pairs, or ``.npz`` paths).
    ``drop_remainder=B`` reproduces the reference, which processes ``len(images) // B`` full batches of ``B`` = 128 and silently drops the rest
    (metrics.py:170-198): only the first ``(n // B) * B`` images count."""

    def __init__(self, model: InceptionV3Features):
        self.model = model

    def statistics(self, batches, *, drop_remainder: Optional[int] = None) -> FIDStatistics:
        st = FIDStatistics(self.model.dims)
        feats = [self.model(b) for b in batches]
        if drop_remainder:
            B, n = int(drop_remainder), sum(f.shape[0] for f in feats)
            keep = n // B * B if n >= B else n        # (a set smaller than one batch: the reference shrinks the batch to the set)
            feats = [torch.cat(feats)[:keep]] if feats else []
        for f in feats:
            st.update(f)
        return st

    @staticmethod
    def _stats(s):
        if isinstance(s, FIDStatistics):
            return s.finalize()
        if isinstance(s, (str, bytes)) or hasattr(s, "__fspath__"):
            return FIDStatistics.load(s).finalize()
        return s

    def __call__(self, stats_a, stats_b) -> float:
        (m1, s1), (m2, s2) = self._stats(stats_a), self._stats(stats_b)
        return frechet_distance(m1, s1, m2, s2)
