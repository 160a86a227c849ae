"""Thin tensor-level wrappers over the C-ABI of libpcdm.so (include/pcdm.h).

PyTorch is used for device memory and streams only; every op here is one call into the
hand-written HIP library on the caller's current stream.  Tensors must live on a ROCm device
(``cuda``); CPU tensors are accepted only when the loaded library is the test emulator build.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from pathlib import Path
from dataclasses import dataclass
from typing import Optional, Sequence, Union

import torch

from . import _lib
from ._lib import GemmParams

EPI_STORE, EPI_GEGLU, EPI_SPLIT_VT, EPI_NCHW_F32 = 0, 1, 2, 3
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2
BF16 = torch.bfloat16
LAUNCH_LOG: Optional[list] = None  # set to [] by bench.py to time individual launches with HIP events
LAUNCH_KEYS: Optional[list] = None  # set to [] by tools/tune_in_step.py: (index into LAUNCH_LOG, tuning-table key) of every table-driven GEMM launch
LAUNCH_SPANS: Optional[list] = None  # ... and ("ln" key, first, end) = the LAUNCH_LOG entries of every LayerNorm -> Linear pair
LN_REFUSED: Optional[set] = None   # set to set() by tools/tune_in_step.py: the "ln" keys whose table-named fused call the library refused (-1)
AUTOTUNE = True                    # pick the GEMM tile configuration per problem shape at first use (GPU only)
DEFER_SPLITK = os.environ.get("PCDM_DEFER_SPLITK", "1") != "0"   # split-K reduce folded into the consuming GroupNorm (A/B switch)


def _stream(t: torch.Tensor) -> Optional[int]:
    if t.is_cuda:
        return torch.cuda.current_stream(t.device).cuda_stream
    if not _lib.is_emulator():
        raise RuntimeError("pcdms_amd ops need tensors on the MI355X (device 'cuda'); there is no CPU path")
    return None


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(rc: int, name: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{name} failed with code {rc}")


def _c(t: torch.Tensor, dtype) -> torch.Tensor:
    assert t.dtype == dtype and t.is_contiguous(), (t.dtype, dtype, t.is_contiguous())
    return t


def _cn(t: Optional[torch.Tensor], dtype, numel: int, what: str) -> Optional[torch.Tensor]:
    """an optional operand the kernel indexes as ``numel`` contiguous elements of ``dtype`` (more is fine: a table, a wider buffer)"""
    if t is not None:
        assert t.dtype == dtype and t.is_contiguous() and t.numel() >= numel, (what, t.dtype, dtype, t.is_contiguous(), t.numel(), numel)
    return t


# ------------------------------------------------------------------------------------ GEMM tiles, tuner and workspace state
ROWGEMM_TILES = (31, 32, 33, 34, 35, 36)   # rowgemm.hip (K = 320): id -> (BM, BN) below
STATS_TILES = (2, 4, 5, 6, 7, 8, 10, 18)   # gemm_ext.hip EXT = 3: the tiles whose STORE epilogue can also write LayerNorm partials (row_stats)
_STATS_VALID: dict = {}
LN_TILED = os.environ.get("PCDM_LN_TILED", "1") != "0"
LN_TILED_TILES = (18, 4, 7, 17, 26, 8, 2)   # gemm.hip dispatch_tile_ln(): the tiled instances that take a folded LayerNorm (any K; row statistics
#                                             from the A tiles as they pass through LDS) -- levels 1-3 of the UNet, the prior, the encoders
LN_PARTIALS_TILES = (23,)                     # consumers of producer partials only (mode 2; round 6: the 176-row GEGLU-capable tile)
# gemm.hip dispatch_tile(): id -> (BM, BN)
TILE_SHAPES = {1: (256, 128), 2: (64, 64), 3: (256, 64), 4: (128, 128), 5: (128, 64), 6: (256, 64), 7: (128, 128),
               8: (64, 64), 9: (256, 128), 10: (128, 64), 11: (256, 128), 12: (256, 64), 13: (256, 64), 14: (256, 64),
               15: (128, 64), 16: (512, 64), 17: (256, 256), 18: (128, 128),
               21: (192, 320), 26: (192, 256), 22: (176, 320), 23: (176, 256),
               31: (192, 128), 32: (192, 64), 33: (96, 128), 34: (192, 64), 35: (128, 64), 36: (64, 64)}
_TUNED: dict = {}
_WS: dict = {}
_WS_RETIRED: list = []   # outgrown workspaces are kept: a captured hipGraph may still hold their address
_WS_GEN: dict = {}
TUNE_ITERS = 3     # timed launches per candidate (tools/tune_gemm_shapes.py raises it for the committed table)
TUNE_REPEATS = 1
TUNE_COLD = False  # tools/tune_gemm_shapes.py --cold: evict L2 / Infinity Cache before every timed launch (inside the denoise step a
#                    GEMM never finds its 1.74 GB of weights cached; back-to-back launches of one problem do)
_FLUSH: dict = {}


def _launch(t: torch.Tensor, call, name: str, work: float, info: tuple, *extra, key=None) -> int:
    """``rc = call()`` (one C call that launches one kernel on ``t``'s stream).  While ``LAUNCH_LOG`` is a list and ``t`` is on the device, the
    call is bracketed by two HIP events on the launch stream and a launch that was accepted (rc 0) is appended as ``(name, algorithmic work, e0,
    e1, info, *extra)``; ``key``: its tuning-table key, for ``LAUNCH_KEYS``.  A refused call (rc -1: nothing was launched) leaves no entry."""
    if LAUNCH_LOG is None or not t.is_cuda:
        return call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = call()
    if rc == 0:
        e1.record()
        LAUNCH_LOG.append((name, work, e0, e1, info, *extra))
        if LAUNCH_KEYS is not None and key is not None:
            LAUNCH_KEYS.append((len(LAUNCH_LOG) - 1, key))
    return rc


def _time_launches(fn, iters: int) -> float:
    """Milliseconds between two HIP events around ``iters`` back-to-back calls of ``fn`` on the current stream (the tuners)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


# ------------------------------------------------------------------------------------ norms
def groupnorm_ws(B: int, C: int, device) -> torch.Tensor:
    n = _lib.lib().pcdm_groupnorm_ws_floats(B, C)
    return torch.zeros(n, dtype=torch.float32, device=device)   # arrival counters must start at zero


def groupnorm_cluster_timeouts(ws: torch.Tensor) -> int:
    """How many workgroups of the in-launch-exchange GroupNorm path gave up waiting for their partners (and computed alone) since the
    workspace was allocated; 0 unless something else held CUs during a launch.  Synchronous (diagnostics / tests)."""
    n = C.c_uint(0)
    _chk(_lib.lib().pcdm_groupnorm_cluster_timeouts(_ptr(ws), C.byref(n), None), "pcdm_groupnorm_cluster_timeouts")
    return int(n.value)


class DeferredGemm:
    """What ``gemm(..., defer_reduce=True)`` returns when the tuned configuration splits K: the fp32 partial slabs are in the split-K
    workspace, the reduce launch has NOT run, ``out`` (the bf16 tensor the GEMM would have written) is still unwritten.  The next
    ``groupnorm`` takes this object as its first source (``pcdm_groupnorm_splitk``): it reduces while it loads, and writes ``out`` iff
    ``store`` (something else -- a residual, a skip -- reads the tensor later).  Nothing else may touch the split-K workspace in between."""

    __slots__ = ("part", "split_k", "M", "N", "Npad", "bias", "rowvec", "ldrv", "rowvec_step", "rowvec_step_stride", "rowvec_step_count", "step_error", "rpb", "residual", "ldr", "out",
                 "store", "keep")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def shape(self):
        return self.out.shape

    def tensor(self) -> torch.Tensor:
        """The bf16 tensor -- valid once the consuming GroupNorm has run with ``store``."""
        assert self.store, "this deferred GEMM's tensor is never written (only its GroupNorm reads it)"
        return self.out


def as_tensor(x: Union[torch.Tensor, "DeferredGemm"]) -> torch.Tensor:
    return x.tensor() if isinstance(x, DeferredGemm) else x


def groupnorm(x1: Union[torch.Tensor, "DeferredGemm"], x2: Optional[torch.Tensor], B: int, HW: int, groups: int, eps: float,
              gamma: torch.Tensor, beta: torch.Tensor, silu: bool, out: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """x1 [B*HW, C1] (+ optional x2 [B*HW, C2]) bf16 -> out [B*HW, C1+C2] bf16.  x1 may be a ``DeferredGemm``."""
    C1 = x1.shape[-1]
    C2 = 0 if x2 is None else x2.shape[-1]
    _c(out, BF16); _c(gamma, torch.float32); _c(beta, torch.float32)
    assert out.numel() == B * HW * (C1 + C2) and gamma.numel() >= C1 + C2 and beta.numel() >= C1 + C2
    assert x2 is None or (_c(x2, BF16).numel() == B * HW * C2)
    assert _c(ws, torch.float32).numel() >= _lib.lib().pcdm_groupnorm_ws_floats(B, C1 + C2)
    if isinstance(x1, DeferredGemm):
        d = x1
        assert d.M == B * HW and d.N == C1 and (d.rowvec is None or d.rpb == HW), "rowvec rows must be the GroupNorm's batch entries"
        sp = _lib.GnSplitKSrc()
        sp.part, sp.split_k, sp.M, sp.N, sp.Npad = d.part, d.split_k, d.M, d.N, d.Npad
        sp.bias, sp.rowvec, sp.ldrv, sp.residual, sp.ldr = d.bias, d.rowvec, d.ldrv, d.residual, d.ldr
        sp.rowvec_step, sp.rowvec_step_stride = d.rowvec_step, d.rowvec_step_stride
        sp.rowvec_step_count, sp.step_error = d.rowvec_step_count, d.step_error
        sp.pre_out, sp.store_pre = _ptr(_c(d.out, BF16)), int(d.store)
        fn, call = "pcdm_groupnorm_splitk", lambda: _lib.lib().pcdm_groupnorm_splitk(
            C.byref(sp), _ptr(x2), C2, B, HW, groups, eps, _ptr(gamma), _ptr(beta), int(silu), _ptr(out), _ptr(ws), _stream(out))
    else:
        assert _c(x1, BF16).numel() == B * HW * C1
        fn, call = "pcdm_groupnorm", lambda: _lib.lib().pcdm_groupnorm(
            _ptr(x1), C1, _ptr(x2), C2, B, HW, groups, eps, _ptr(gamma), _ptr(beta), int(silu), _ptr(out), _ptr(ws), _stream(x1))
    # algorithmic bytes: the tensor read once + written once
    _chk(_launch(out, call, "groupnorm", 2.0 * B * HW * (C1 + C2) * 2, (B, HW, C1 + C2)), fn)
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: torch.Tensor) -> torch.Tensor:
    rows, Cc = x.shape
    _c(x, BF16); _c(out, BF16)
    assert out.numel() == x.numel()
    _cn(gamma, torch.float32, Cc, "gamma"); _cn(beta, torch.float32, Cc, "beta")
    _chk(_launch(x, lambda: _lib.lib().pcdm_layernorm(_ptr(x), _ptr(out), rows, Cc, eps, _ptr(gamma), _ptr(beta), _stream(x)),
                 "layernorm", 2.0 * rows * Cc * 2, (rows, Cc)), "pcdm_layernorm")
    return out


# ------------------------------------------------------------------------------------ weights
def _round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


@dataclass
class PackedWeight:
    """bf16 [Npad, K] (K contiguous) + fp32 bias[Npad] as the GEMM kernel wants them."""
    w: torch.Tensor
    bias: Optional[torch.Tensor]
    N: int
    K: int
    Npad: int
    cin: int = 0       # conv: (padded) input channels
    geglu: bool = False
    alg_nk: int = 0    # algorithmic N*K (un-padded; GEGLU counts both halves) for FLOP accounting
    exec_nk: int = 0   # N*K the launch really contracts when that is LESS than the algorithmic figure (the phase-decomposed upsample convolution); 0: = alg_nk
    wsum: Optional[torch.Tensor] = None   # fp32 [Npad]: row sums of the packed bf16 weights when they carry a folded LayerNorm


def pack_linear(w: torch.Tensor, bias: Optional[torch.Tensor], device, pad_to: int = 64) -> PackedWeight:
    """nn.Linear / 1x1-conv weight [N, K(,1,1)] -> packed."""
    w = w.reshape(w.shape[0], -1).float()
    N, K = w.shape
    assert K % 64 == 0, K
    Npad = _round_up(N, pad_to)
    wp = torch.zeros(Npad, K, dtype=torch.float32)
    wp[:N] = w
    bp = None
    if bias is not None:
        bp = torch.zeros(Npad, dtype=torch.float32)
        bp[:N] = bias.float()
        bp = bp.to(device)
    return PackedWeight(wp.to(BF16).to(device), bp, N, K, Npad, alg_nk=N * K)


def pack_conv3x3(w: torch.Tensor, bias: Optional[torch.Tensor], device, pad_to: int = 64) -> PackedWeight:
    """Conv2d weight [N, Cin, 3, 3] -> [Npad, 9*Cin_pad] with k = (ky*3+kx)*Cin_pad + c."""
    N, Cin = w.shape[:2]
    Cp = _round_up(Cin, 64)
    wp = torch.zeros(N, 3, 3, Cp, dtype=torch.float32)
    wp[..., :Cin] = w.float().permute(0, 2, 3, 1)
    pw = pack_linear(wp.reshape(N, 9 * Cp), bias, device, pad_to)
    pw.cin = Cp
    pw.alg_nk = N * 9 * Cin
    return pw


def pack_conv3x3_shortcut(w: torch.Tensor, bias: Optional[torch.Tensor], w_sc: torch.Tensor, bias_sc: Optional[torch.Tensor], device) -> PackedWeight:
    """ResnetBlock2D's conv2 [N, C, 3, 3] and conv_shortcut [N, Cx(,1,1)] as ONE contraction: rows [9 C_pad taps | Cx], bias = the sum.  The
    launch reads conv2's input through the taps and the block's input (one tensor or the two halves of the skip concat) through the extra K
    (``gemm(..., conv=..., a2=, a3=)``): out = conv2(h) + conv_shortcut(x), exactly the residual sum of resnet.py's forward."""
    N, Cin = w.shape[:2]
    Cp = _round_up(Cin, 64)
    wp = torch.zeros(N, 3, 3, Cp, dtype=torch.float32)
    wp[..., :Cin] = w.float().permute(0, 2, 3, 1)
    ws = w_sc.reshape(N, -1).float()
    assert ws.shape[1] % 64 == 0, ws.shape
    b = None
    if bias is not None or bias_sc is not None:
        b = (bias.float() if bias is not None else 0) + (bias_sc.float() if bias_sc is not None else 0)
    pw = pack_linear(torch.cat([wp.reshape(N, 9 * Cp), ws], 1), b, device)
    pw.cin = Cp
    pw.alg_nk = N * (9 * Cin + ws.shape[1])
    return pw


UPSAMPLE_TAP_LUT = sum(((3 * (a + i) + b + j) << (16 * (2 * a + b) + 4 * (2 * i + j))) for a in (0, 1) for b in (0, 1) for i in (0, 1) for j in (0, 1))


def pack_upsample_phases(w: torch.Tensor, bias: Optional[torch.Tensor], device) -> PackedWeight:
    """Upsample2D's ``conv3x3(nearest x2 (x))`` [N, C, 3, 3] as FOUR 2x2 convolutions of the low-res input, one per output phase (a, b) =
    (row parity, column parity): output pixel (2y + a, 2x + b) reads low-res rows {y - 1 + a, y + a} and columns {x - 1 + b, x + b}; the taps
    of the 3x3 kernel that land on the same low-res pixel are SUMMED (fp64, then bf16 like any weight).  Rows [phase 2a + b][N], K = [4 taps][C]
    with the tap order (i, j) of ``UPSAMPLE_TAP_LUT``: one launch with ``tap_group_n = N`` on the low-res tensor, 4/9 of the FLOPs of the
    convolution on the upsampled one, then ``pixel_shuffle2``.  Exact algebra; zero padding agrees (the upsampled border row -1 is low-res row -1)."""
    N, Cin = w.shape[:2]
    assert Cin % 64 == 0 and N % 64 == 0, (N, Cin)
    w = w.double()
    rows = {0: ([0], [1, 2]), 1: ([0, 1], [2])}      # phase parity -> (taps summed into window position 0, position 1)
    blocks = []
    for a in (0, 1):
        for b in (0, 1):
            k = torch.zeros(N, 2, 2, Cin, dtype=torch.float64)
            for i in (0, 1):
                for j in (0, 1):
                    k[:, i, j] = sum(w[:, :, ky, kx] for ky in rows[a][i] for kx in rows[b][j])
            blocks.append(k.reshape(N, 4 * Cin))
    pw = pack_linear(torch.cat(blocks, 0).float(), None if bias is None else bias.float().repeat(4), device)
    pw.cin = Cin
    pw.alg_nk = N * 9 * Cin * 4    # algorithmic FLOPs stay those of the 3x3 convolution on the upsampled tensor: 2 (4 M) N 9 C
    pw.exec_nk = 4 * N * 4 * Cin   # ... what the launch executes: 4/9 of them
    return pw


def pixel_shuffle2(x: torch.Tensor, out: torch.Tensor, B: int, H: int, W: int, Cc: int) -> torch.Tensor:
    """[B*H*W, 4*Cc] (phase-major columns) -> NHWC [B, 2H, 2W, Cc] (as [B*2H*2W, Cc]): the second half of the phase-decomposed upsample convolution."""
    assert x.dtype == BF16 and out.dtype == BF16 and x.is_contiguous() and out.is_contiguous() and x.numel() == out.numel() == B * H * W * 4 * Cc
    assert Cc % 8 == 0 and x.device == out.device, (Cc, x.device, out.device)
    _chk(_lib.lib().pcdm_pixel_shuffle2(_ptr(x), _ptr(out), B, H, W, Cc, _stream(x)), "pcdm_pixel_shuffle2")
    return out


def freeu_ws_bytes(B: int, H: int, W: int, C1: int, C2: int) -> int:
    """Workspace bytes of ``freeu`` at this shape: 0 while the plane takes the one-launch form; -1 for a shape ``pcdm_freeu`` refuses."""
    return int(_lib.lib().pcdm_freeu_ws_bytes(B, H, W, C1, C2))


def freeu(hidden: torch.Tensor, skip: torch.Tensor, skip_out: torch.Tensor, B: int, H: int, W: int, b: float, s: float,
          hidden_out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None):
    """FreeU in front of one decoder resnet (``pcdm_freeu``): ``hidden`` [B*H*W, C1] and ``skip`` [B*H*W, C2] bf16 NHWC rows; the first C1/2 backbone
    channels times ``b`` (in place unless ``hidden_out`` is given), the skip's lowest frequencies times ``s`` into ``skip_out`` (``skip`` itself is
    not written).  ``ws``: ``freeu_ws_bytes`` bytes for planes beyond the one-launch size.  Returns ``(hidden_out, skip_out)``."""
    ho = hidden if hidden_out is None else hidden_out
    assert all(t.dtype == BF16 and t.is_contiguous() and t.dim() == 2 and t.shape[0] == B * H * W for t in (hidden, ho, skip, skip_out))
    assert ho.shape == hidden.shape and skip_out.shape == skip.shape
    C1, C2 = hidden.shape[1], skip.shape[1]
    need = freeu_ws_bytes(B, H, W, C1, C2)
    assert need >= 0, (B, H, W, C1, C2)
    if need > 0 or ws is not None:
        assert ws is not None and ws.is_contiguous() and ws.numel() * ws.element_size() >= need and ws.device == skip.device, \
            f"pcdm_freeu needs a workspace of {need} bytes at this shape"
    call = lambda: _lib.lib().pcdm_freeu(_ptr(hidden), _ptr(ho), _ptr(skip), _ptr(skip_out), B, H, W, C1, C2, float(b), float(s), _ptr(ws),  # noqa: E731
                                         _stream(skip))
    _chk(_launch(skip, call, "freeu", 14.0 * B * H * W * C2, (B, H, W, C1, C2)), "pcdm_freeu")
    return ho, skip_out


def pack_geglu(w: torch.Tensor, bias: torch.Tensor, device) -> PackedWeight:
    """GEGLU proj weight [2*D, K] (rows [h | gate]) -> rows interleaved per 64 as [32 h | 32 gate]."""
    w = w.float()
    D2, K = w.shape
    D = D2 // 2
    Dp = _round_up(D, 64)
    wh = torch.zeros(Dp, K); wh[:D] = w[:D]
    wg = torch.zeros(Dp, K); wg[:D] = w[D:]
    bh = torch.zeros(Dp); bh[:D] = bias[:D].float()
    bg = torch.zeros(Dp); bg[:D] = bias[D:].float()
    wp = torch.stack([wh.view(Dp // 32, 32, K), wg.view(Dp // 32, 32, K)], dim=1).reshape(2 * Dp, K)
    bp = torch.stack([bh.view(Dp // 32, 32), bg.view(Dp // 32, 32)], dim=1).reshape(2 * Dp)
    return PackedWeight(wp.to(BF16).to(device), bp.to(device), D, K, 2 * Dp, geglu=True, alg_nk=2 * D * K)


def fold_layernorm(w: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor):
    """LayerNorm(x; gamma, beta) @ w^T + bias  ==  x_hat @ (w diag(gamma))^T + (bias + w beta)  with x_hat = (x - mean) rstd.
    Returns (w diag(gamma), bias + w beta) in fp32."""
    w, gamma, beta = w.float().cpu(), gamma.float().cpu(), beta.float().cpu()
    b = w @ beta
    if bias is not None:
        b = b + bias.float().cpu()
    return w * gamma[None, :], b


def _with_wsum(pw: PackedWeight) -> PackedWeight:
    pw.wsum = pw.w.float().sum(dim=1).contiguous()   # of the bf16 values the MFMA multiplies, in the packed row order
    return pw


def pack_linear_ln(w, bias, gamma, beta, device, pad_to: int = 64) -> PackedWeight:
    """``pack_linear`` of a Linear that follows a LayerNorm, with the LayerNorm folded in (pcdm_gemm_params.ln_wsum)."""
    wf, bf = fold_layernorm(w, bias, gamma, beta)
    return _with_wsum(pack_linear(wf, bf, device, pad_to))


def pack_geglu_ln(w, bias, gamma, beta, device) -> PackedWeight:
    wf, bf = fold_layernorm(w, bias, gamma, beta)
    return _with_wsum(pack_geglu(wf, bf, device))


# ------------------------------------------------------------------------------------ GEMM / conv
def gemm(a: torch.Tensor, pw: PackedWeight, out: torch.Tensor, *, a2: Optional[torch.Tensor] = None, a3: Optional[torch.Tensor] = None,
         rowvec: Optional[torch.Tensor] = None, rows_per_batch: Optional[int] = None,
         residual: Optional[torch.Tensor] = None, res_mod: int = 0, epilogue: int = EPI_STORE,
         out2: Optional[torch.Tensor] = None, vt_col0: int = 0, conv: Optional[dict] = None, tile: int = 0,
         use_bias: bool = True, split_k: int = 1, w_ld: int = 0, act: int = ACT_NONE, zero_rows: int = 0,
         ln: Optional[tuple] = None, ln_buf: Optional[torch.Tensor] = None, pw_ln: Optional[PackedWeight] = None,
         defer_reduce: Optional[bool] = None, dup_rows: int = 0, rowvec_step: Optional[torch.Tensor] = None,
         rowvec_step_stride: int = 0, row_stats: Optional[torch.Tensor] = None, rowvec_step_count: int = 0,
         step_error: Optional[torch.Tensor] = None, tap_lut: int = 0, tap_group_n: int = 0) -> Union[torch.Tensor, "DeferredGemm"]:
    """out = epilogue(A @ W^T).  ``a`` [M, K1] (linear; optional ``a2`` [M, K2] = channel concat) or
    NHWC [B, Hi, Wi, cin] with ``conv=dict(B,Hi,Wi,Ho,Wo,stride,upsample)``.  A convolution whose packed weight has EXTRA K behind the nine
    taps (``pack_conv3x3_shortcut``: K = 9 cin + cx) contracts on over a 1x1 convolution of ``a2`` [M, c1] (and ``a3`` [M, cx - c1]) at the
    output pixel -- ResnetBlock2D's conv2 + conv_shortcut over the block's (concatenated) input as one launch (pcdm_gemm_params.a3, ABI 5).

    ``ln=(gamma, beta, eps)``: out = epilogue(LayerNorm(A) @ W^T).  With ``pw_ln`` (the same Linear packed by ``pack_linear_ln`` /
    ``pack_geglu_ln``: LayerNorm folded into the weights) no LayerNorm pass is needed at all: the A-in-registers kernel (tiles 31..36, K = 320; 34
    = four waves, two workgroups per CU: the one in use at level 0) takes the row statistics from the rows it holds, the tiled
    instances of ``LN_TILED_TILES`` (any K: levels 1-3) from the A tiles as they pass through LDS; otherwise the rows go through
    ``pcdm_layernorm`` into ``ln_buf`` [M, K] first (the tuner times all forms, the LayerNorm launch included, and keeps the fastest).

    ``defer_reduce`` (``True``: the reduced tensor is also read by something other than the next GroupNorm -- it gets written by that
    GroupNorm; ``False``-but-not-``None`` i.e. ``0``: only the next GroupNorm reads it): when the configuration in use splits K, skip the
    reduce launch and return a ``DeferredGemm`` for ``ops.groupnorm`` to consume.  The caller promises that the very next user of the
    result is that GroupNorm and that no other split-K GEMM runs in between.  ``None``: never defer.

    ``rowvec_step`` (device int32 counter) / ``rowvec_step_stride`` (floats): the row-vector block in use is ``rowvec + *rowvec_step *
    rowvec_step_stride`` -- the per-step slice of a table that holds the time-embedding projections of every denoise step.  ``rowvec_step_count``
    (> 0: the blocks behind ``rowvec``) bounds the counter ON THE DEVICE: a value outside ``[0, count)`` is clamped into the table and ``step_error``
    (device int32) set to 1 -- the launch never reads beyond the table (pcdm_gemm_params.rowvec_step_count, ABI 4).

    ``dup_rows`` (conv only): ``out`` has ``M + dup_rows`` rows; rows ``m + dup_rows`` get the same contraction with THEIR row-vector /
    residual rows (``pcdm_gemm_params.dup_rows``: the CFG-shared prefix of the UNet)."""
    if ln is not None and conv is None and a2 is None and ln_buf is not None:
        return _gemm_ln(a, pw, pw_ln, out, ln, ln_buf, rows_per_batch=rows_per_batch, epilogue=epilogue, out2=out2, vt_col0=vt_col0,
                        tile=tile, row_stats=row_stats)
    assert ln is None
    p = GemmParams()
    assert a.dtype == BF16 and a.stride(-1) == 1 and (conv is None or a.is_contiguous())
    p.a = _ptr(a)
    p.ldw = w_ld
    if conv is not None:
        p.conv = 1
        p.B, p.Hi, p.Wi, p.Ho, p.Wo = conv["B"], conv["Hi"], conv["Wi"], conv["Ho"], conv["Wo"]
        p.stride, p.upsample, p.cin = conv.get("stride", 1), conv.get("upsample", 0), pw.cin
        p.no_pad_lo = conv.get("no_pad_lo", 0)
        assert a.numel() == p.B * p.Hi * p.Wi * pw.cin, (a.shape, pw.cin)
        M = p.B * p.Ho * p.Wo
        if tap_group_n:      # a subset of the nine taps per output-channel group (pack_upsample_phases; pcdm_gemm_params.tap_lut)
            assert a2 is None and a3 is None and pw.K % pw.cin == 0 and pw.K // pw.cin <= 4, (pw.K, pw.cin)
            p.tap_lut, p.tap_group_n = int(tap_lut), int(tap_group_n)
        elif a2 is not None:   # extra K: the 1x1 sources behind the taps
            assert a2.dtype == BF16 and a2.dim() == 2 and a2.shape[0] == M and a2.stride(-1) == 1
            p.a2, p.lda2, p.c1 = _ptr(a2), a2.stride(0), a2.shape[1]
            cx = a2.shape[1]
            if a3 is not None:
                assert a3.dtype == BF16 and a3.dim() == 2 and a3.shape[0] == M and a3.stride(-1) == 1
                p.a3, p.lda3 = _ptr(a3), a3.stride(0)
                cx += a3.shape[1]
            assert pw.K == 9 * pw.cin + cx, (pw.K, pw.cin, cx)
        else:
            assert a3 is None and pw.K == 9 * pw.cin, (pw.K, pw.cin)
    else:
        M = a.shape[0]
        p.lda = a.stride(0)
        p.c1 = a.shape[1]
        assert a3 is None
        if a2 is not None:
            assert a2.dtype == BF16 and a2.stride(-1) == 1
            p.a2 = _ptr(a2)
            p.lda2 = a2.stride(0)
            assert a.shape[1] + a2.shape[1] == pw.K
        else:
            assert a.shape[1] == pw.K, (a.shape, pw.K)
    p.w = _ptr(pw.w)
    p.M, p.N, p.K, p.Npad = M, pw.N, pw.K, pw.Npad
    p.bias = _ptr(pw.bias) if (use_bias and pw.bias is not None) else None
    p.rows_per_batch = rows_per_batch or M
    if rowvec is not None:
        assert rowvec.dtype == torch.float32 and rowvec.shape[-1] == pw.N and rowvec.stride(-1) == 1
        p.rowvec = _ptr(rowvec)
        p.ldrv = rowvec.stride(0)
        if rowvec_step is not None:
            assert rowvec_step.dtype == torch.int32 and rowvec_step.device == rowvec.device
            p.rowvec_step, p.rowvec_step_stride = _ptr(rowvec_step), int(rowvec_step_stride)
            p.rowvec_step_count = int(rowvec_step_count)
            if step_error is not None:
                assert step_error.dtype == torch.int32 and step_error.device == rowvec.device
                p.step_error = _ptr(step_error)
    if residual is not None:
        _c(residual, BF16)
        p.residual = _ptr(residual)
        p.ldr = residual.stride(0) if residual.dim() == 2 else pw.N
        p.res_mod = res_mod
    p.epilogue = epilogue
    p.act = act
    p.zero_rows = zero_rows   # (linear) A rows < zero_rows are declared all-zero: never read
    p.dup_rows = dup_rows
    assert not dup_rows or (conv is not None and out.shape[0] >= M + dup_rows)
    p.vt_col0 = vt_col0
    p.out = _ptr(out)
    p.ldo = out.stride(0) if (out.dim() == 2 and epilogue != EPI_NCHW_F32) else pw.N
    if out2 is not None:
        p.out2 = _ptr(out2)
        p.ldo2 = out2.shape[-1]
    stream = _stream(a)
    split = 1
    key = None
    if tile == 0 and AUTOTUNE:
        key = (M, pw.Npad, pw.K, p.conv, p.stride + (10 if p.no_pad_lo else 0) + (20 if tap_group_n else 0), p.upsample, epilogue,
               a2 is not None, residual is not None) + ((True,) if zero_rows else ((2,) if dup_rows else ()))   # (w_ld does not change the best tile)
        tile, split = _TUNED.get(key, (0, 1))
        if tile in ROWGEMM_TILES and (rowvec is not None or act != ACT_NONE or (residual is not None and res_mod < M)):
            # the key does not carry these (none of the UNet's K = 320 residual linears has them): the A-in-registers kernel the table names for the
            # shape cannot serve this call -- the library's heuristic tile does (a table entry is a preference, never a reason to refuse a launch)
            tile, split = 0, 1
        elif tile == 0 and a.is_cuda and not torch.cuda.is_current_stream_capturing():   # (the emulator build runs the library's heuristic)
            tile, split = _TUNED[key] = _autotune(p, stream, pw, epilogue, a.device, out)
    elif split_k > 1:
        split = split_k
    p.tile = tile
    if row_stats is not None:
        # producer of LayerNorm partials (pcdm_gemm_params.row_stats_out): [M][N / 32][2] fp32, written by the STORE epilogue of the tiles that
        # have such an instance; any other configuration leaves the buffer alone and says so (the consumer then takes its own statistics)
        ok = tile in STATS_TILES and split == 1 and conv is None and epilogue == EPI_STORE and act == ACT_NONE and pw.N % 32 == 0
        _STATS_VALID[row_stats.untyped_storage().data_ptr()] = ok   # (keyed on the storage: a consumer may read a row slice of the buffer)
        if ok:
            assert row_stats.dtype == torch.float32 and row_stats.is_contiguous() and row_stats.numel() >= M * (pw.N // 32) * 2
            p.row_stats_out = _ptr(row_stats)
    deferred = None
    if split > 1:
        ws = _splitk_ws(a.device, split * M * pw.Npad)
        p.split_k, p.ws, p.ws_floats = split, _ptr(ws), ws.numel()
        if defer_reduce is not None and DEFER_SPLITK and epilogue == EPI_STORE and act == ACT_NONE and (residual is None or res_mod in (0, M)) \
                and (rowvec is None or (rows_per_batch and M % rows_per_batch == 0)) and out.is_contiguous() and out.shape == (M, pw.N):
            p.defer_reduce = 1
            deferred = DeferredGemm(part=_ptr(ws), split_k=split, M=M, N=pw.N, Npad=pw.Npad, bias=p.bias, rowvec=p.rowvec,
                                    ldrv=p.ldrv if rowvec is not None else 0, rowvec_step=p.rowvec_step, rowvec_step_stride=p.rowvec_step_stride,
                                    rowvec_step_count=p.rowvec_step_count, step_error=p.step_error,
                                    rpb=p.rows_per_batch, residual=p.residual, ldr=p.ldr, out=out,
                                    store=bool(defer_reduce), keep=(ws, rowvec, residual, pw, rowvec_step, step_error))
    # algorithmic FLOPs stay the un-hoisted 2*M*N*K also when zero_rows skips part of the contraction; the sixth field is what
    # the launch executes
    _chk(_launch(a, lambda: _lib.lib().pcdm_gemm(C.byref(p), stream), "gemm_kernel", 2.0 * M * pw.alg_nk,
                 (M, pw.N, pw.K, bool(conv), tile, split), 2.0 * (M - zero_rows) * (pw.exec_nk or pw.alg_nk), key=key), "pcdm_gemm")
    return out if deferred is None else deferred


def row_stats_valid(row_stats: Optional[torch.Tensor]) -> bool:
    """did the last ``gemm(..., row_stats=buf)`` on this buffer actually write the partials?"""
    return row_stats is not None and _STATS_VALID.get(row_stats.untyped_storage().data_ptr(), False)


def ln_wants_row_stats(M: int, pw: "PackedWeight", epilogue: int) -> bool:
    """should the producer of the rows of this LayerNorm -> Linear pair write partials (``gemm(..., row_stats=)``)?  Yes when the pair's tuned
    choice merges partials (mode 2), and while the pair is untuned (the tuner can only measure mode 2 if it is handed partials)."""
    if not LN_TILED or pw.K == 320 or pw.K % 64 or pw.K > 1280:
        return False
    ch = _TUNED.get(("ln", M, pw.Npad, pw.K, epilogue))
    return ch is None or (len(ch) > 1 and ch[0] > 0 and ch[1] == 2)


def row_stats_reference(a: torch.Tensor) -> torch.Tensor:
    """[M][K / 32][2] {sum, M2 about the run's own mean} of every 32-column run of ``a`` (torch; the tuner and the tests)."""
    M, K = a.shape
    v = a.float().view(M, K // 32, 32)
    sm = v.sum(-1)
    return torch.stack([sm, ((v - sm.unsqueeze(-1) / 32) ** 2).sum(-1)], -1).contiguous()


def _gemm_ln(a, pw, pw_ln, out, ln, ln_buf, *, rows_per_batch, epilogue, out2, vt_col0, tile, row_stats=None):
    """LayerNorm + GEMM: folded into the A-in-registers kernel (K = 320) or an extended instance of the tiled kernel when that wins for the
    shape, two launches otherwise.  Tuned choice per shape = (tile, mode): mode 1 = the kernel takes the row statistics itself, mode 2 = it
    merges the partials its producer wrote (``row_stats``; falls back to mode 1 on the same tile when the producer could not write them).
    For tools/tune_in_step.py, ``LAUNCH_SPANS`` gets the entries of ``LAUNCH_LOG`` the pair produced -- one launch or two, depending on the table."""
    gamma, beta, eps = ln
    M = a.shape[0]
    assert a.dtype == BF16 and a.stride(1) == 1 and a.shape[1] == pw.K and ln_buf.shape[0] >= M
    key = ("ln", M, pw.Npad, pw.K, epilogue)
    span0 = len(LAUNCH_LOG) if (LAUNCH_SPANS is not None and LAUNCH_LOG is not None and not tile) else None
    have_stats = row_stats_valid(row_stats)
    choice = (tile, 2 if have_stats else 1) if tile else _TUNED.get(key)   # (an explicit tile: partials are used when there are valid ones)
    if not LN_TILED and not tile and pw.K != 320:   # PCDM_LN_TILED=0: A/B switch -- levels 1-3 keep their LayerNorm launches
        pw_ln = None
    stream = _stream(a)

    def fused(t, stats=None):
        p = GemmParams()
        p.a, p.lda, p.c1 = _ptr(a), a.stride(0), a.shape[1]
        p.w, p.M, p.N, p.K, p.Npad = _ptr(pw_ln.w), M, pw_ln.N, pw_ln.K, pw_ln.Npad
        p.bias = _ptr(pw_ln.bias)
        p.rows_per_batch = rows_per_batch or M
        p.epilogue, p.vt_col0 = epilogue, vt_col0
        p.out = _ptr(out)
        p.ldo = out.stride(0)
        if out2 is not None:
            p.out2, p.ldo2 = _ptr(out2), out2.shape[-1]
        p.ln_wsum, p.ln_eps = _ptr(_c(pw_ln.wsum, torch.float32)), float(eps)
        if stats is not None:
            p.ln_row_stats = _ptr(stats)
        p.tile = t
        return _lib.lib().pcdm_gemm(C.byref(p), stream)

    def two_launches():
        n = layernorm(a, gamma, beta, eps, ln_buf[:M])
        return gemm(n, pw, out, rows_per_batch=rows_per_batch, epilogue=epilogue, out2=out2, vt_col0=vt_col0)

    foldable = pw_ln is not None and pw_ln.wsum is not None
    assert foldable or not tile
    if foldable and choice is None and AUTOTUNE and a.is_cuda and not torch.cuda.is_current_stream_capturing():
        two_launches()                         # (tunes the plain GEMM of this shape on the way)
        ref = out.float().clone()

        def timed(fn):   # one warm launch, then TUNE_ITERS timed ones
            fn()
            return _time_launches(fn, TUNE_ITERS)
        best, best_t = (0, 1), timed(two_launches)
        ref_stats = row_stats_reference(a) if (row_stats is not None and pw.K != 320 and pw.K % 64 == 0 and pw.K <= 1280) else None   # (a caller that has a producer)
        for t in (ROWGEMM_TILES if pw.K == 320 else ()) + LN_TILED_TILES + LN_PARTIALS_TILES:
            for md in (1, 2):
                st_ = None if md == 1 else ref_stats
                if (md == 2 and (st_ is None or t in ROWGEMM_TILES)) or fused(t, st_) != 0:   # (the library refuses what a tile cannot do: Npad not a
                    continue                                                                    #  multiple of its BN, GEGLU on a 32-wide wave tile, ...)
                if not bool(((out.float() - ref).abs().max() <= 3e-2 * ref.abs().max() + 1e-3).item()):
                    continue
                tt = timed(lambda: fused(t, st_))
                if tt < best_t:
                    best, best_t = (t, md), tt
        choice = _TUNED[key] = best
    md = 1
    if isinstance(choice, tuple):
        choice, md = choice[0], (choice[1] if len(choice) > 1 else 1)
    if choice and foldable:
        stats = row_stats if (md == 2 and have_stats) else None     # (mode 2 without valid partials: the same tile takes its own statistics)
        # The table key does not hold rows_per_batch: (2816, 3840, 1280, q|k|v^T) is level 2 at UNet batch 8 (352 tokens per image: fine) and
        # level 3 at batch 32 (88 tokens: the folded instances need a multiple of 32 for the V^T pass and refuse).  A refusal (-1) comes
        # before anything is launched: take the two-launch form then -- also inside a graph capture.
        rc = _launch(a, lambda: fused(choice, stats), "gemm_kernel", 2.0 * M * pw.alg_nk, (M, pw.N, pw.K, False, choice, 1), 2.0 * M * pw.alg_nk,
                     key=None if tile else key)
        if rc == -1 and not tile:
            if LN_REFUSED is not None:
                LN_REFUSED.add(key)
            two_launches()
        else:
            _chk(rc, "pcdm_gemm (LayerNorm folded)")
    else:
        two_launches()
    if span0 is not None:
        LAUNCH_SPANS.append((key, span0, len(LAUNCH_LOG)))
    return out


def workspace_generation(device) -> int:
    """Changes whenever the split-K workspace of ``device`` is re-allocated (a graph captured before that must be re-captured
    to use the new one; the old one stays allocated, so replaying a stale graph is slow-path-correct, never a use-after-free)."""
    return _WS_GEN.get(torch.device(device), 0)


def _splitk_ws(device, floats: int) -> torch.Tensor:
    """fp32 split-K workspace (one per device; only grows outside graph capture; never freed)."""
    ws = _WS.get(device)
    if ws is None or ws.numel() < floats:
        if ws is not None and device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("split-K workspace would grow during graph capture")
        if ws is not None:
            _WS_RETIRED.append(ws)
        ws = _WS[device] = torch.empty(max(floats, 1 << 24), dtype=torch.float32, device=device)
        _WS_GEN[device] = _WS_GEN.get(device, 0) + 1
    return ws


def _flush_caches(device):
    buf = _FLUSH.get(device)
    if buf is None:
        buf = _FLUSH[device] = torch.empty(96 << 20, dtype=torch.float32, device=device)   # 384 MiB > 256 MiB Infinity Cache
    buf.zero_()


def _autotune(p: GemmParams, stream, pw: PackedWeight, epilogue: int, device, out: Optional[torch.Tensor] = None):
    """Time every valid (tile configuration, split-K factor) of gemm.hip on this exact problem (HIP events on
    the launch stream, 1 warm + TUNE_ITERS timed launches each, best of TUNE_REPEATS) and return the fastest.
    Runs once per problem shape, outside graph capture; the launches are idempotent (same inputs, same output)."""
    fn = _lib.lib().pcdm_gemm
    nkt = pw.K // 64
    best, best_t = (0, 1), float("inf")
    ref = None   # output of the first valid configuration: a candidate that disagrees with it is never selected
    for tile, (bm, bn) in TILE_SHAPES.items():
        ntiles = -(-p.M // bm) * (pw.Npad // bn if pw.Npad % bn == 0 else 0)
        if ntiles == 0:
            continue
        splits = [1]
        if tile in ROWGEMM_TILES and (pw.K != 320 or p.conv):
            continue
        if epilogue == EPI_STORE and tile not in ROWGEMM_TILES:   # split K only when the tile grid alone cannot fill the 256 CUs
            splits += [s for s in (2, 3, 4, 6, 8, 12, 16) if ntiles * s <= 1024 and nkt // s >= 4 and ntiles < 512]
        for sk in splits:
            p.tile = tile
            if sk > 1:
                ws = _splitk_ws(device, sk * p.M * pw.Npad)
                p.split_k, p.ws, p.ws_floats = sk, _ptr(ws), ws.numel()
            else:
                p.split_k, p.ws, p.ws_floats = 0, None, 0
            if fn(C.byref(p), stream) != 0:   # configuration not valid for this N / epilogue
                break
            if out is not None:
                cur = out.float()
                if ref is None:
                    ref = cur.clone()
                elif not bool(((cur - ref).abs().max() <= 2e-2 * ref.abs().max() + 1e-3).item()):
                    continue
            t = float("inf")
            for _ in range(TUNE_REPEATS):
                if TUNE_COLD:
                    evs = []
                    for _ in range(TUNE_ITERS):
                        _flush_caches(device)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn(C.byref(p), stream)
                        e1.record()
                        evs.append((e0, e1))
                    evs[-1][1].synchronize()
                    t = min(t, sum(a.elapsed_time(b) for a, b in evs))
                    continue
                t = min(t, _time_launches(lambda: fn(C.byref(p), stream), TUNE_ITERS))
            if t < best_t:
                best, best_t = (tile, sk), t
    p.split_k, p.ws, p.ws_floats = 0, None, 0
    if best[0] == 0:
        raise RuntimeError("no valid GEMM tile configuration")
    return best


# ---- committed per-shape tuning table (measured on MI355X by tools/tune_gemm_shapes.py); shapes not in the table
# are tuned online at first use.  Keys: "M,Npad,K,conv,stride,upsample,epilogue,two_source,residual".
TUNING_FILE = Path(os.environ.get("PCDM_TUNING_TABLE") or Path(__file__).resolve().parent / "tuning" / "gfx950.json")   # (env: A/B runs)


def load_tuning(path: Path = TUNING_FILE) -> int:
    if not Path(path).exists():
        return 0
    tab = json.loads(Path(path).read_text())
    for k, v in tab.get("gemm", {}).items():
        key = tuple((x == "True") if x in ("True", "False") else (int(x) if x.lstrip("-").isdigit() else x) for x in k.split(","))
        _TUNED[key] = (int(v[0]), int(v[1]))
    return len(tab.get("gemm", {}))


def save_tuning(path: Path = TUNING_FILE, note: str = "") -> None:
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    tab = {"note": note, "gemm": {",".join(str(x) for x in k): list(v) for k, v in sorted(_TUNED.items(), key=lambda kv: str(kv[0]))}}
    Path(path).write_text(json.dumps(tab, indent=0))


if os.environ.get("PCDM_NO_TUNING_TABLE") != "1":   # (the online autotuner alone, for A/B runs)
    load_tuning()


def flash_attn(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, B: int, H: int, Lq: int,
               Lk: int, scale: Optional[float] = None, thr: Optional[float] = None) -> torch.Tensor:
    """q [B*Lq, ldq], k [B*Lk, ldk] (views allowed: row stride = .stride(0)), vt [B, H*64, ldvt], out [B*Lq, ldo]."""
    for t in (q, k, vt, out):
        assert t.dtype == BF16
    assert q.stride(1) == 1 and k.stride(1) == 1 and vt.is_contiguous() and out.stride(1) == 1
    scale = scale if scale is not None else 1.0 / math.sqrt(64)
    args = (_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(vt), vt.shape[-1], _ptr(out), out.stride(0), B, H, Lq, Lk, scale)
    if thr is None:
        call = lambda: _lib.lib().pcdm_flash_attn(*args, _stream(q))  # noqa: E731
    else:   # explicit lazy-rescale threshold (log2 units; 0 = eager online softmax)
        call = lambda: _lib.lib().pcdm_flash_attn_thr(*args, float(thr), _stream(q))  # noqa: E731
    _chk(_launch(q, call, "flash_attn_kernel", 4.0 * B * H * Lq * Lk * 64, (B, H, Lq, Lk)), "pcdm_flash_attn")
    return out


def attn_wide(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, B: int, Lq: int, Lk: int,
              scale: Optional[float] = None) -> torch.Tensor:
    """One head of width d = vt.shape[1] (64 <= d <= 512, d % 64 == 0): q [B*Lq, ldq], k [B*Lk, ldk] (views allowed: row stride =
    .stride(0), columns [0, d) used), vt [B, d, ldvt] with ldvt >= Lk, out [B*Lq, ldo] (columns [0, d) written)."""
    for t in (q, k, vt, out):
        assert t.dtype == BF16
    assert q.stride(1) == 1 and k.stride(1) == 1 and vt.is_contiguous() and vt.dim() == 3 and out.stride(1) == 1
    d = vt.shape[1]
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    _chk(_launch(q, lambda: _lib.lib().pcdm_attn_wide(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(vt), vt.shape[-1], _ptr(out), out.stride(0),
                                                      B, Lq, Lk, d, scale, _stream(q)),
                 "attn_wide_kernel", 4.0 * B * Lq * Lk * d, (B, Lq, Lk, d)), "pcdm_attn_wide")
    return out


FP8 = torch.uint8   # e4m3 bytes (torch.float8_e4m3fn views of these buffers are never computed on by PyTorch)


def quantize_fp8(x: torch.Tensor, out: torch.Tensor, cols: Optional[int] = None, scale: float = 1.0) -> torch.Tensor:
    """bf16 [rows, >= cols] (row stride = .stride(0)) -> e4m3 bytes out [rows, cols_pad]; columns >= cols are zeroed."""
    assert x.dtype == BF16 and out.dtype == FP8 and x.stride(-1) == 1 and out.stride(-1) == 1 and x.dim() == 2 and out.dim() == 2
    rows = x.shape[0]
    cols = cols if cols is not None else x.shape[1]
    assert out.shape[0] == rows and 1 <= cols <= x.shape[1] and cols <= out.shape[1] and out.shape[1] % 8 == 0, (x.shape, out.shape, cols)
    _chk(_lib.lib().pcdm_quantize_fp8(_ptr(x), _ptr(out), rows, cols, out.shape[1], x.stride(0), out.stride(0), float(scale), _stream(x)),
         "pcdm_quantize_fp8")
    return out


def flash_attn_fp8(q: torch.Tensor, k8: torch.Tensor, vt8: torch.Tensor, out: torch.Tensor, B: int, H: int, Lq: int, Lk: int,
                   scale: Optional[float] = None, k_descale: float = 1.0, v_descale: float = 1.0, thr: float = 5.0) -> torch.Tensor:
    """q bf16 [B*Lq, ldq]; k8 e4m3 [B*Lk, ldk]; vt8 e4m3 [B, H*64, ldvt]; out bf16 [B*Lq, ldo]."""
    assert q.dtype == BF16 and out.dtype == BF16 and k8.dtype == FP8 and vt8.dtype == FP8
    assert q.stride(1) == 1 and k8.stride(1) == 1 and vt8.is_contiguous() and out.stride(1) == 1
    scale = scale if scale is not None else 1.0 / math.sqrt(64)
    _chk(_launch(q, lambda: _lib.lib().pcdm_flash_attn_fp8(_ptr(q), q.stride(0), _ptr(k8), k8.stride(0), _ptr(vt8), vt8.shape[-1], _ptr(out),
                                                           out.stride(0), B, H, Lq, Lk, scale, float(k_descale), float(v_descale), float(thr),
                                                           _stream(q)),
                 "flash_attn_fp8_kernel", 4.0 * B * H * Lq * Lk * 64, (B, H, Lq, Lk)), "pcdm_flash_attn_fp8")
    return out


# ------------------------------------------------------------------------------------ small ops
def timestep_embedding(t_dev: torch.Tensor, step_dev: Optional[torch.Tensor], out: torch.Tensor, flip: bool = True,
                       shift: float = 0.0, step_error: Optional[torch.Tensor] = None) -> torch.Tensor:
    """t_dev: int64 or float32 device table (a float table keeps its fractional timesteps: ``pcdm_timestep_embedding_f32``).  The counter is
    bounded into the table's ``t_dev.numel()`` rows on the device; a counter outside it sets ``step_error`` (int32 device tensor) to 1."""
    assert t_dev.dtype in (torch.int64, torch.float32) and t_dev.is_contiguous() and t_dev.numel() >= 1
    assert out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 2
    _cn(step_dev, torch.int32, 1, "step_dev"); _cn(step_error, torch.int32, 1, "step_error")
    B, dim = out.shape
    fn = _lib.lib().pcdm_timestep_embedding if t_dev.dtype == torch.int64 else _lib.lib().pcdm_timestep_embedding_f32
    _chk(fn(_ptr(t_dev), t_dev.numel(), _ptr(step_dev), _ptr(step_error), _ptr(out), B, dim, int(flip), shift, _stream(out)),
         "pcdm_timestep_embedding")
    return out


def timestep_embedding_rows(t_dev: torch.Tensor, out: torch.Tensor, flip: bool = True, shift: float = 0.0) -> torch.Tensor:
    """out[i, :] = Timesteps(t_dev[i]) for a whole timestep table (fp32 [n, dim]); t_dev int64 or float32 (``pcdm_timestep_embedding_rows_f32``)."""
    assert t_dev.dtype in (torch.int64, torch.float32) and t_dev.is_contiguous()
    assert out.dtype == torch.float32 and out.shape[0] == t_dev.numel() and out.is_contiguous()
    fn = _lib.lib().pcdm_timestep_embedding_rows if t_dev.dtype == torch.int64 else _lib.lib().pcdm_timestep_embedding_rows_f32
    _chk(fn(_ptr(t_dev), t_dev.numel(), _ptr(out), out.shape[1], int(flip), shift, _stream(out)), "pcdm_timestep_embedding_rows")
    return out


def time_class_combine(emb_t: torch.Tensor, cls: Optional[torch.Tensor], out: torch.Tensor, B: int) -> torch.Tensor:
    """out[i * B + b] = bf16(silu(emb_t[i] + cls[b])): emb_t fp32 [n, D], cls fp32 [B, D] or None, out bf16 [n * B, D]."""
    n, D = emb_t.shape
    _c(emb_t, torch.float32); _c(out, BF16)
    assert out.shape == (n * B, D) and (cls is None or (_c(cls, torch.float32).shape == (B, D)))
    _chk(_lib.lib().pcdm_time_class_combine(_ptr(emb_t), _ptr(cls), _ptr(out), n, B, D, _stream(out)), "pcdm_time_class_combine")
    return out


def small_linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *,
                 add: Optional[torch.Tensor] = None, act_in: bool = False, act_out: Union[bool, int] = False) -> torch.Tensor:
    """x fp32 [B,K], w bf16 [N,K] -> out fp32 [B,N].  act_out: True/1 = SiLU before ``add``, 2 = SiLU after it."""
    _c(x, torch.float32); _c(w, BF16); _c(out, torch.float32)
    B, K = x.shape
    N = w.shape[0]
    assert tuple(w.shape) == (N, K) and tuple(out.shape) == (B, N), (x.shape, w.shape, out.shape)
    _cn(bias, torch.float32, N, "bias")
    assert add is None or (_c(add, torch.float32).numel() == B * N), "add is fp32 [B, N]"
    _chk(_lib.lib().pcdm_small_linear(_ptr(x), _ptr(w), _ptr(bias), _ptr(add), _ptr(out), B, K, N, int(act_in),
                                      int(act_out), _stream(x)), "pcdm_small_linear")
    return out


def _assemble_operands(latents, rep, mask, masked, out):
    """the extents ``pcdm_assemble_input(_ex)`` indexes (the C call is handed no sizes of mask / masked / out)"""
    assert latents.dim() == 4 and latents.shape[1] == 4 and rep >= 1, (latents.shape, rep)
    N, _, h, w = latents.shape
    _c(latents, torch.float32); _c(masked, torch.float32); _c(out, BF16)
    assert masked.dim() == 4 and tuple(masked.shape[1:]) == (4, h, w) and masked.shape[0] in (1, rep * N), (masked.shape, latents.shape, rep)
    assert out.dim() == 4 and tuple(out.shape[:3]) == (rep * N, h, w) and out.shape[3] % 8 == 0 and out.shape[3] >= 16, (out.shape, latents.shape, rep)
    if mask is not None:
        _c(mask, torch.float32)
        assert mask.dim() == 4 and tuple(mask.shape[1:]) == (1, h, w) and mask.shape[0] in (1, rep * N), (mask.shape, latents.shape, rep)


def assemble_input(latents: torch.Tensor, rep: int, mask: Optional[torch.Tensor], masked: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """latents fp32 [N,4,h,w]; mask [1|rep*N,1,h,w] or None (no mask channel: stage 3); masked [1|rep*N,4,h,w]
    -> out bf16 [rep*N,h,w,cpad]."""
    _assemble_operands(latents, rep, mask, masked, out)
    N, _, h, w = latents.shape
    cpad = out.shape[-1]
    _chk(_lib.lib().pcdm_assemble_input(_ptr(latents), N, rep, _ptr(mask), 1 if mask is None else mask.shape[0], _ptr(masked),
                                        masked.shape[0], _ptr(out), h, w, cpad, _stream(out)), "pcdm_assemble_input")
    return out


def assemble_input_ex(latents: torch.Tensor, rep: int, mask: Optional[torch.Tensor], masked: torch.Tensor, out: torch.Tensor,
                      scale_tab: Optional[torch.Tensor] = None, scale_col: int = 0, step_dev: Optional[torch.Tensor] = None,
                      step_error: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``assemble_input`` with ``scheduler.scale_model_input`` folded in (pcdm_assemble_input_ex): the latent channels are multiplied by
    ``scale_tab[*step_dev, scale_col]`` (fp32 device table [rows, stride]) before their rounding to bf16; ``scale_tab=None``: ``assemble_input``."""
    _assemble_operands(latents, rep, mask, masked, out)
    N, _, h, w = latents.shape
    rows = stride = 1
    if scale_tab is not None:
        _c(scale_tab, torch.float32)
        assert scale_tab.dim() == 2 and 0 <= scale_col < scale_tab.shape[1]
        rows, stride = scale_tab.shape
    _cn(step_dev, torch.int32, 1, "step_dev"); _cn(step_error, torch.int32, 1, "step_error")
    _chk(_lib.lib().pcdm_assemble_input_ex(_ptr(latents), N, rep, _ptr(mask), 1 if mask is None else mask.shape[0], _ptr(masked),
                                           masked.shape[0], _ptr(out), h, w, out.shape[-1], _ptr(scale_tab), stride, int(scale_col), rows,
                                           _ptr(step_dev), _ptr(step_error), _stream(out)), "pcdm_assemble_input_ex")
    return out


def nchw_to_nhwc_bf16(x: torch.Tensor, out: Optional[torch.Tensor] = None, cpad: Optional[int] = None) -> torch.Tensor:
    """NCHW (any float dtype) -> NHWC bf16, channels zero-padded to ``cpad``."""
    B, Cc, H, W = x.shape
    x = _c(x.float().contiguous(), torch.float32)
    cpad = cpad or _round_up(Cc, 8)
    if out is None:
        out = torch.empty(B, H, W, cpad, dtype=BF16, device=x.device)
    assert out.shape[-1] == cpad and _c(out, BF16).numel() == B * H * W * cpad
    _chk(_lib.lib().pcdm_nchw_f32_to_nhwc_bf16(_ptr(x), _ptr(out), B, Cc, cpad, H * W, _stream(x)), "nchw_to_nhwc")
    return out


def nhwc_bf16_to_nchw(x: torch.Tensor, B: int, Cc: int, H: int, W: int) -> torch.Tensor:
    assert x.numel() == B * H * W * Cc, (x.shape, B, Cc, H, W)
    out = torch.empty(B, Cc, H, W, dtype=torch.float32, device=x.device)
    _chk(_lib.lib().pcdm_nhwc_bf16_to_nchw_f32(_ptr(_c(x, BF16)), _ptr(out), B, Cc, H * W, _stream(x)), "nhwc_to_nchw")
    return out


def f32_to_bf16(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    x = _c(x, torch.float32)
    if out is None:
        out = torch.empty(x.shape, dtype=BF16, device=x.device)
    assert _c(out, BF16).numel() == x.numel()
    _chk(_lib.lib().pcdm_f32_to_bf16(_ptr(x), _ptr(out), x.numel(), _stream(x)), "f32_to_bf16")
    return out


def cfg_step(eps: torch.Tensor, cfg: bool, g: float, x: Optional[torch.Tensor], x_prev: Optional[torch.Tensor],
             coef: Optional[torch.Tensor], step_dev: Optional[torch.Tensor] = None,
             noise: Optional[torch.Tensor] = None, eps_out: Optional[torch.Tensor] = None,
             step_error: Optional[torch.Tensor] = None) -> None:
    """pcdm_cfg_step: coef fp32 [rows, 4] on the device (None: the CFG combine alone, no table); the counter is bounded into its rows on the
    device and a counter outside them sets ``step_error`` (int32 device tensor) to 1."""
    n = eps.numel() // (2 if cfg else 1)
    _c(eps, torch.float32)
    assert eps.numel() == (2 * n if cfg else n) and n >= 1
    for what, t in (("x", x), ("noise", noise), ("x_prev", x_prev), ("eps_out", eps_out)):
        assert t is None or _c(t, torch.float32).numel() == n, (what, t.numel(), n)
    assert (x_prev is None) == (x is None) == (coef is None), "x, x_prev and coef come together (eps_out alone: the CFG combine only)"
    _cn(coef, torch.float32, 4, "coef"); _cn(step_dev, torch.int32, 1, "step_dev"); _cn(step_error, torch.int32, 1, "step_error")
    assert coef is None or (coef.dim() == 2 and coef.shape[1] == 4), "coef is [rows, 4]"
    _chk(_lib.lib().pcdm_cfg_step(_ptr(eps), int(cfg), g, _ptr(x), _ptr(noise), _ptr(x_prev), _ptr(eps_out),
                                  _ptr(coef), 0 if coef is None else coef.shape[0], _ptr(step_dev), _ptr(step_error), n, _stream(eps)),
         "pcdm_cfg_step")


def unipc_step(eps: torch.Tensor, cfg: bool, g: float, x: torch.Tensor, m1: torch.Tensor, m2: torch.Tensor, last: torch.Tensor,
               coef: torch.Tensor, step_dev: Optional[torch.Tensor] = None, step_error: Optional[torch.Tensor] = None) -> None:
    """pcdm_unipc_step: CFG combine + one UniPC step in place on (x, m1, m2, last); coef fp32 [rows, 12] on the device.  The counter is bounded
    into the rows on the device; a counter outside them sets ``step_error`` (int32 device tensor) to 1."""
    n = x.numel()
    for t in (eps, x, m1, m2, last, coef):
        _c(t, torch.float32)
    assert eps.numel() == (2 * n if cfg else n) and m1.numel() == m2.numel() == last.numel() == n
    assert coef.dim() == 2 and coef.shape[1] == 12, "coef is [rows, 12]"
    _cn(step_dev, torch.int32, 1, "step_dev"); _cn(step_error, torch.int32, 1, "step_error")
    _chk(_lib.lib().pcdm_unipc_step(_ptr(eps), int(cfg), float(g), _ptr(x), _ptr(m1), _ptr(m2), _ptr(last), _ptr(coef), coef.shape[0],
                                    _ptr(step_dev), _ptr(step_error), n, _stream(x)), "pcdm_unipc_step")


def dpmpp_step(eps: torch.Tensor, cfg: bool, g: float, x: torch.Tensor, m1: torch.Tensor, noise_all: Optional[torch.Tensor],
               coef: torch.Tensor, step_dev: Optional[torch.Tensor] = None, step_error: Optional[torch.Tensor] = None) -> None:
    """pcdm_dpmpp_step: CFG combine + one DPM-Solver++ step in place on (x, m1); coef fp32 [rows, 8], noise_all fp32
    [rows, x.numel()] (or None), both on the device.  The counter is bounded into the rows on the device; a counter outside them sets
    ``step_error`` (int32 device tensor) to 1."""
    n = x.numel()
    for t in (eps, x, m1, coef):
        _c(t, torch.float32)
    assert eps.numel() == (2 * n if cfg else n) and m1.numel() == n
    assert coef.dim() == 2 and coef.shape[1] == 8, "coef is [rows, 8]"
    _cn(step_dev, torch.int32, 1, "step_dev"); _cn(step_error, torch.int32, 1, "step_error")
    if noise_all is not None:
        assert tuple(_c(noise_all, torch.float32).shape) == (coef.shape[0], n), "noise_all is [rows, n] with the rows of coef"
    _chk(_lib.lib().pcdm_dpmpp_step(_ptr(eps), int(cfg), float(g), _ptr(x), _ptr(m1), _ptr(noise_all), _ptr(coef), coef.shape[0],
                                    _ptr(step_dev), _ptr(step_error), n, _stream(x)), "pcdm_dpmpp_step")


#: row layout of the ``pcdm_multistep_step`` table (include/pcdm.h PCDM_MS_*)
MS_ROW, MS_CX, MS_CS, MS_C0, MS_C1, MS_C2, MS_C3, MS_CZ, MS_IN_SCALE, MS_SAVE, MS_PUSH = 12, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9


def multistep_step(eps: torch.Tensor, cfg: bool, g: float, x: torch.Tensor, xs: torch.Tensor, h1: torch.Tensor, h2: torch.Tensor,
                   h3: torch.Tensor, noise_all: Optional[torch.Tensor], coef: torch.Tensor, step_dev: Optional[torch.Tensor] = None,
                   step_error: Optional[torch.Tensor] = None) -> None:
    """pcdm_multistep_step: CFG combine + one Euler / Euler-ancestral / LMS / PLMS step in place on (x, xs, h1, h2, h3); coef fp32
    [rows, 12], noise_all fp32 [rows, x.numel()] (or None), both on the device."""
    n = x.numel()
    for t in (eps, x, xs, h1, h2, h3, coef):
        _c(t, torch.float32)
    assert eps.numel() == (2 * n if cfg else n) and xs.numel() == h1.numel() == h2.numel() == h3.numel() == n
    assert coef.dim() == 2 and coef.shape[1] == MS_ROW
    assert len({t.data_ptr() for t in (x, xs, h1, h2, h3)}) == 5, "the five state slots are distinct buffers"
    if noise_all is not None:
        assert _c(noise_all, torch.float32).numel() == coef.shape[0] * n
    _cn(step_dev, torch.int32, 1, "step_dev"); _cn(step_error, torch.int32, 1, "step_error")
    _chk(_lib.lib().pcdm_multistep_step(_ptr(eps), int(cfg), float(g), _ptr(x), _ptr(xs), _ptr(h1), _ptr(h2), _ptr(h3), _ptr(noise_all),
                                        _ptr(coef), coef.shape[0], _ptr(step_dev), _ptr(step_error), n, _stream(x)), "pcdm_multistep_step")


def unclip_step(pred: torch.Tensor, cfg: bool, g: float, x: torch.Tensor, noise: Optional[torch.Tensor], out: torch.Tensor,
                coefs: Sequence[float]) -> torch.Tensor:
    """pcdm_unclip_step: coefs = (p_x, p_e, clip, c_x0, c_x, c_noise, out_scale, out_shift); fp32 tensors."""
    _c(pred, torch.float32); _c(x, torch.float32); _c(out, torch.float32)
    n = x.numel()
    assert pred.numel() == (2 * n if cfg else n) and out.numel() == n and len(coefs) == 8
    if noise is not None:
        assert _c(noise, torch.float32).numel() == n
    carr = (C.c_float * 8)(*[float(c) for c in coefs])
    _chk(_lib.lib().pcdm_unclip_step(_ptr(pred), int(cfg), float(g), _ptr(x), _ptr(noise), _ptr(out), carr, n, _stream(x)),
         "pcdm_unclip_step")
    return out


def unclip_step_dev(pred: torch.Tensor, cfg: bool, g: float, x: torch.Tensor, noise_all: Optional[torch.Tensor], coef: torch.Tensor,
                    step_dev: Optional[torch.Tensor], step_error: Optional[torch.Tensor] = None) -> None:
    """pcdm_unclip_step_dev: in place on x; coef fp32 [rows, 8], noise_all fp32 [rows, x.numel()] (or None), both on the device.  The counter
    is bounded into the rows on the device; a counter outside them sets ``step_error`` (int32 device tensor) to 1."""
    _c(pred, torch.float32); _c(x, torch.float32); _c(coef, torch.float32)
    n = x.numel()
    assert pred.numel() == (2 * n if cfg else n)
    assert coef.dim() == 2 and coef.shape[1] == 8, "coef is [rows, 8]"
    _cn(step_dev, torch.int32, 1, "step_dev"); _cn(step_error, torch.int32, 1, "step_error")
    if noise_all is not None:
        assert tuple(_c(noise_all, torch.float32).shape) == (coef.shape[0], n), "noise_all is [rows, n] with the rows of coef"
    _chk(_lib.lib().pcdm_unclip_step_dev(_ptr(pred), int(cfg), float(g), _ptr(x), _ptr(noise_all), _ptr(coef), coef.shape[0],
                                         _ptr(step_dev), _ptr(step_error), n, _stream(x)), "pcdm_unclip_step_dev")


def lincomb(out: torch.Tensor, xs: Sequence[torch.Tensor], cs: Sequence[float]) -> torch.Tensor:
    n = len(xs)
    assert 1 <= n <= 6 and len(cs) == n
    for t in xs:
        _c(t, torch.float32)
        assert t.numel() == out.numel()
    _c(out, torch.float32)
    arr = (C.c_void_p * n)(*[_ptr(t) for t in xs])
    carr = (C.c_float * n)(*[float(c) for c in cs])
    _chk(_lib.lib().pcdm_lincomb(_ptr(out), n, arr, carr, out.numel(), _stream(out)), "pcdm_lincomb")
    return out


def rescale_noise_cfg(cfg_eps: torch.Tensor, text_eps: torch.Tensor, out: torch.Tensor, guidance_rescale: float) -> torch.Tensor:
    """fp32 [N, ...] tensors; per-sample std matching (ref stage2_inpaint_pipeline.py:52-63)."""
    _c(cfg_eps, torch.float32); _c(text_eps, torch.float32); _c(out, torch.float32)
    N = cfg_eps.shape[0]
    assert text_eps.numel() == cfg_eps.numel() == out.numel()
    _chk(_lib.lib().pcdm_rescale_noise_cfg(_ptr(cfg_eps), _ptr(text_eps), _ptr(out), N, cfg_eps.numel() // N,
                                           float(guidance_rescale), _stream(out)), "pcdm_rescale_noise_cfg")
    return out


def softmax_rows(s: torch.Tensor, out: torch.Tensor, scale: float) -> torch.Tensor:
    """fp32 [rows, cols] -> bf16 [rows, cols] = softmax(scale * s, dim=-1)."""
    assert s.dtype == torch.float32 and out.dtype == BF16 and s.stride(1) == 1 and out.stride(1) == 1
    rows, cols = s.shape
    assert out.dim() == 2 and out.shape[0] == rows and out.shape[1] >= cols, (s.shape, out.shape)
    _chk(_lib.lib().pcdm_softmax_rows(_ptr(s), _ptr(out), rows, cols, s.stride(0), out.stride(0), float(scale), _stream(s)),
         "pcdm_softmax_rows")
    return out


def gaussian_sample(moments: torch.Tensor, noise: torch.Tensor, out: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """moments fp32 [B, 2 zc, H, W] (mean | logvar), noise fp32 [B, zc, H, W] -> out = (mean + exp(0.5 clamp(logvar)) noise) scale
    (include/pcdm.h: pcdm_gaussian_sample)."""
    _c(moments, torch.float32); _c(noise, torch.float32); _c(out, torch.float32)
    B, c2 = int(moments.shape[0]), int(moments.shape[1])
    assert moments.dim() >= 3 and c2 % 2 == 0 and noise.numel() == out.numel() == moments.numel() // 2 and noise.shape[0] == B, (moments.shape, noise.shape, out.shape)
    HW = moments.numel() // (B * c2)
    _chk(_lib.lib().pcdm_gaussian_sample(_ptr(moments), _ptr(noise), _ptr(out), B, c2 // 2, HW, float(scale), _stream(out)), "pcdm_gaussian_sample")
    return out


def image_to_uint8(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """x fp32 [B, cstride, H, W] (the first 3 channels) -> out uint8 [B, H, W, 3]: VaeImageProcessor.postprocess (include/pcdm.h: pcdm_image_to_uint8)."""
    _c(x, torch.float32); _c(out, torch.uint8)
    B, cs = int(x.shape[0]), int(x.shape[1])
    assert x.dim() == 4 and cs >= 3 and tuple(out.shape) == (B, x.shape[2], x.shape[3], 3), (x.shape, out.shape)
    _chk(_lib.lib().pcdm_image_to_uint8(_ptr(x), _ptr(out), B, cs, int(x.shape[2] * x.shape[3]), _stream(out)), "pcdm_image_to_uint8")
    return out


def advance_step(step_dev: torch.Tensor) -> None:
    _cn(step_dev, torch.int32, 1, "step_dev")
    _chk(_lib.lib().pcdm_advance_step(_ptr(step_dev), _stream(step_dev)), "pcdm_advance_step")


# ------------------------------------------------------------------------------------ image metrics (pcdms_amd/metrics.py is the public surface)
def _win(w: Sequence[int]):
    return (C.c_int32 * 4)(*[int(v) for v in w])


def _images(cand: torch.Tensor, ref: torch.Tensor) -> int:
    assert cand.dim() == 4 and ref.dim() == 4 and cand.dtype == ref.dtype and cand.dtype in (torch.uint8, torch.float32), (cand.shape, ref.shape, cand.dtype, ref.dtype)
    assert cand.is_contiguous() and ref.is_contiguous() and cand.device == ref.device
    return int(cand.dtype == torch.float32)


def metrics_ws_bytes(N: int, ref_n: int, W: int, H: int, sigma: float) -> int:
    """Workspace bytes of ``ssim`` at this sigma (and of ``psnr``; sigma <= 0: of ``psnr`` alone); -1: the library refuses the problem."""
    return int(_lib.lib().pcdm_metrics_ws_bytes(N, ref_n, W, H, float(sigma)))


def ssim(cand: torch.Tensor, ref: torch.Tensor, cand_win: Sequence[int], ref_win: Sequence[int], scores: torch.Tensor, argmax: Optional[torch.Tensor],
         ws: torch.Tensor, *, sigma: float = 1.2, data_range: Optional[float] = None) -> torch.Tensor:
    """cand [N, Hc, Wc, 3], ref [1 | N, Hr, Wr, 3], both uint8 or both fp32; windows (x0, y0, W, H); scores fp32 [N], argmax int32 [1] or None
    (include/pcdm.h: pcdm_ssim).  data_range None: max - min of each candidate's window."""
    f32 = _images(cand, ref)
    _c(scores, torch.float32)
    if argmax is not None:
        _c(argmax, torch.int32)
    _chk(_lib.lib().pcdm_ssim(_ptr(cand), cand.shape[0], cand.shape[1], cand.shape[2], _win(cand_win), _ptr(ref), ref.shape[0], ref.shape[1], ref.shape[2],
                              _win(ref_win), cand.shape[3], f32, float(sigma), -1.0 if data_range is None else float(data_range), _ptr(scores),
                              _ptr(argmax), _ptr(ws), ws.numel() * ws.element_size(), _stream(cand)), "pcdm_ssim")
    return scores


def psnr(cand: torch.Tensor, ref: torch.Tensor, cand_win: Sequence[int], ref_win: Sequence[int], mse: Optional[torch.Tensor], out: Optional[torch.Tensor],
         ws: torch.Tensor, *, data_range: float = 255.0) -> Optional[torch.Tensor]:
    """mse / out fp32 [N]: mean squared difference and 10 log10(data_range^2 / mse) over the windows (include/pcdm.h: pcdm_psnr)."""
    f32 = _images(cand, ref)
    for t in (mse, out):
        if t is not None:
            _c(t, torch.float32)
    _chk(_lib.lib().pcdm_psnr(_ptr(cand), cand.shape[0], cand.shape[1], cand.shape[2], _win(cand_win), _ptr(ref), ref.shape[0], ref.shape[1], ref.shape[2],
                              _win(ref_win), cand.shape[3], f32, float(data_range), _ptr(mse), _ptr(out), _ptr(ws), ws.numel() * ws.element_size(),
                              _stream(cand)), "pcdm_psnr")
    return out


def absdiff(cand: torch.Tensor, ref: torch.Tensor, cand_win: Sequence[int], ref_win: Sequence[int], l1: Optional[torch.Tensor],
            mae: Optional[torch.Tensor], ws: torch.Tensor) -> None:
    """l1 / mae fp32 [N]: mean |a - b| and sum |a - b| / sum (a + b) over the windows (include/pcdm.h: pcdm_absdiff); ws as for ``psnr``."""
    f32 = _images(cand, ref)
    for t in (l1, mae):
        if t is not None:
            _c(t, torch.float32)
    N, W, H = cand.shape[0], int(cand_win[2]), int(cand_win[3])
    call = lambda: _lib.lib().pcdm_absdiff(_ptr(cand), N, cand.shape[1], cand.shape[2], _win(cand_win), _ptr(ref), ref.shape[0], ref.shape[1],  # noqa: E731
                                           ref.shape[2], _win(ref_win), cand.shape[3], f32, _ptr(l1), _ptr(mae), _ptr(ws),
                                           ws.numel() * ws.element_size(), _stream(cand))
    _chk(_launch(cand, call, "absdiff", 3.0 * N * W * H * 3, (N, H, W, f32)), "pcdm_absdiff")


def ssim_box_ws_bytes(N: int, ref_n: int, W: int, H: int, win_size: int) -> int:
    """Workspace bytes of ``ssim_box``; -1: the library refuses the problem."""
    return int(_lib.lib().pcdm_ssim_box_ws_bytes(N, ref_n, W, H, int(win_size)))


def ssim_box(cand: torch.Tensor, ref: torch.Tensor, cand_win: Sequence[int], ref_win: Sequence[int], scores: torch.Tensor, ws: torch.Tensor, *,
             win_size: int = 51, data_range: Optional[float] = None) -> torch.Tensor:
    """scores fp32 [N]: skimage's uniform-window SSIM with the sample covariance (include/pcdm.h: pcdm_ssim_box).  data_range None: max - min of
    each candidate's window."""
    f32 = _images(cand, ref)
    _c(scores, torch.float32)
    N, W, H, w = cand.shape[0], int(cand_win[2]), int(cand_win[3]), int(win_size)
    call = lambda: _lib.lib().pcdm_ssim_box(_ptr(cand), N, cand.shape[1], cand.shape[2], _win(cand_win), _ptr(ref), ref.shape[0], ref.shape[1],  # noqa: E731
                                            ref.shape[2], _win(ref_win), cand.shape[3], f32, w, -1.0 if data_range is None else float(data_range),
                                            _ptr(scores), _ptr(ws), ws.numel() * ws.element_size(), _stream(cand))
    _chk(_launch(cand, call, "ssim_box", 10.0 * N * 3 * max(W - w + 1, 0) * max(H - w + 1, 0) * 2 * w, (N, H, W, w)), "pcdm_ssim_box")
    return scores


def select_image(cand: torch.Tensor, win: Sequence[int], index: torch.Tensor, out: torch.Tensor, normalized: bool) -> torch.Tensor:
    """out <- the window of cand[index[0]] (uint8 [N, Hc, Wc, 3]; index int32 on the device): uint8 [H, W, 3], or fp32 [1, 3, H, W] =
    (x / 255 - 0.5) / 0.5 when ``normalized`` (include/pcdm.h: pcdm_select_image)."""
    assert cand.dim() == 4
    _c(cand, torch.uint8); _c(index, torch.int32); _c(out, torch.float32 if normalized else torch.uint8)
    _chk(_lib.lib().pcdm_select_image(_ptr(cand), cand.shape[0], cand.shape[1], cand.shape[2], _win(win), cand.shape[3], _ptr(index), _ptr(out),
                                      int(normalized), _stream(cand)), "pcdm_select_image")
    return out


# ------------------------------------------------------------------------------------ LPIPS (pcdms_amd/metrics.py: LPIPS is the public surface)
def pack_lpips_conv(w: torch.Tensor, bias: Optional[torch.Tensor], device) -> dict:
    """fp32 [Cout, Cin, kh, kw] (+ bias [Cout]) -> the packed fp32 operand of ``conv2d_f32`` on ``device`` (include/pcdm.h: pcdm_pack_lpips_conv):
    ``{"w", "bias", "cout", "cin" (padded to 4), "kh", "kw"}``."""
    assert w.dim() == 4, w.shape
    w = w.detach().to("cpu", torch.float32).contiguous()
    b = None if bias is None else bias.detach().to("cpu", torch.float32).contiguous()
    Cout, Cin, kh, kw = (int(v) for v in w.shape)
    assert b is None or tuple(b.shape) == (Cout,), (b.shape, Cout)
    K, cp = C.c_int(0), C.c_int(0)
    lib = _lib.lib()
    Npad = lib.pcdm_pack_lpips_conv(None, None, Cout, Cin, kh, kw, None, None, C.byref(K), C.byref(cp))
    if Npad < 0:
        raise RuntimeError(f"pcdm_pack_lpips_conv refuses {tuple(w.shape)}")
    pw, pb = torch.empty(K.value * Npad, dtype=torch.float32), torch.empty(Npad, dtype=torch.float32)
    _chk(min(0, lib.pcdm_pack_lpips_conv(_ptr(w), _ptr(b), Cout, Cin, kh, kw, _ptr(pw), _ptr(pb), None, None)), "pcdm_pack_lpips_conv")
    return {"w": pw.to(device), "bias": pb.to(device), "cout": Cout, "cin": cp.value, "kh": kh, "kw": kw}


def conv2d_f32(x: torch.Tensor, pw: dict, *, stride: int = 1, pad: int = 0, relu: bool = False) -> torch.Tensor:
    """x NHWC fp32 [B, Hi, Wi, pw["cin"]] -> NHWC fp32 [B, Ho, Wo, Cout]: exact-fp32 implicit-GEMM convolution + bias (+ ReLU) on the fp32-input
    MFMA (include/pcdm.h: pcdm_conv2d_f32)."""
    _c(x, torch.float32)
    B, Hi, Wi, Cin = (int(v) for v in x.shape)
    assert Cin == pw["cin"], (Cin, pw["cin"])
    Ho, Wo = (Hi + 2 * pad - pw["kh"]) // stride + 1, (Wi + 2 * pad - pw["kw"]) // stride + 1
    if Ho < 1 or Wo < 1:
        raise ValueError(f"a {pw['kh']} x {pw['kw']} kernel does not fit a {Hi} x {Wi} image padded by {pad}")
    out = torch.empty((B, Ho, Wo, pw["cout"]), dtype=torch.float32, device=x.device)
    _chk(_lib.lib().pcdm_conv2d_f32(_ptr(x), B, Hi, Wi, Cin, _ptr(pw["w"]), _ptr(pw["bias"]), pw["cout"], pw["kh"], pw["kw"], int(stride), int(pad),
                                    int(relu), _ptr(out), _stream(x)), "pcdm_conv2d_f32")
    return out


def maxpool3s2_f32(x: torch.Tensor) -> torch.Tensor:
    """MaxPool2d(3, stride 2), no padding, on NHWC fp32 (include/pcdm.h: pcdm_maxpool3s2_f32)."""
    _c(x, torch.float32)
    B, Hi, Wi, Cn = (int(v) for v in x.shape)
    if Hi < 3 or Wi < 3:
        raise ValueError(f"no 3 x 3 window in a {Hi} x {Wi} image")
    out = torch.empty((B, (Hi - 3) // 2 + 1, (Wi - 3) // 2 + 1, Cn), dtype=torch.float32, device=x.device)
    _chk(_lib.lib().pcdm_maxpool3s2_f32(_ptr(x), B, Hi, Wi, Cn, _ptr(out), _stream(x)), "pcdm_maxpool3s2_f32")
    return out


def lpips_ws_bytes(N: int, ref_n: int, H: int, W: int) -> int:
    """Workspace bytes of ``lpips``; -1: the library refuses the problem (sides below 31 among others)."""
    return int(_lib.lib().pcdm_lpips_ws_bytes(N, ref_n, H, W))


def lpips(img0: torch.Tensor, img1: torch.Tensor, win0: Sequence[int], win1: Sequence[int], weights: "_lib.LpipsWeights", out: torch.Tensor,
          layers: Optional[torch.Tensor], argmin: Optional[torch.Tensor], ws: torch.Tensor, *, normalize: bool) -> torch.Tensor:
    """img0 / img1 uint8 NHWC [n, Hi, Wi, 3] or fp32 NCHW [n, 3, Hi, Wi] (both the same), img1 with batch 1 or img0's; out fp32 [N], layers fp32
    [5, N] or None, argmin int32 [1] or None (include/pcdm.h: pcdm_lpips)."""
    assert img0.dim() == 4 and img1.dim() == 4 and img0.dtype == img1.dtype and img0.dtype in (torch.uint8, torch.float32)
    assert img0.is_contiguous() and img1.is_contiguous() and img0.device == img1.device
    f32 = int(img0.dtype == torch.float32)
    (H0, W0), (H1, W1) = (img0.shape[2:], img1.shape[2:]) if f32 else (img0.shape[1:3], img1.shape[1:3])
    assert (img0.shape[1] if f32 else img0.shape[3]) == 3 and (img1.shape[1] if f32 else img1.shape[3]) == 3, (img0.shape, img1.shape)
    _c(out, torch.float32)
    if layers is not None:
        _c(layers, torch.float32)
    if argmin is not None:
        _c(argmin, torch.int32)
    _chk(_lib.lib().pcdm_lpips(_ptr(img0), img0.shape[0], int(H0), int(W0), _win(win0), _ptr(img1), img1.shape[0], int(H1), int(W1), _win(win1), f32,
                               int(normalize), C.byref(weights), _ptr(out), _ptr(layers), _ptr(argmin), _ptr(ws), ws.numel() * ws.element_size(),
                               _stream(img0)), "pcdm_lpips")
    return out


# ------------------------------------------------------------------------------------ FID (pcdms_amd/metrics.py: InceptionV3Features, FIDStatistics)
def conv2d_f32_ex(x: torch.Tensor, pw: dict, *, stride: int = 1, pad: Sequence[int] = (0, 0), relu: bool = False, out: Optional[torch.Tensor] = None,
                  offset: int = 0) -> torch.Tensor:
    """``conv2d_f32`` with ``pad = (pad_h, pad_w)`` and, with ``out`` NHWC fp32 [B, Ho, Wo, pitch], the result written into its channels
    ``[offset, offset + Cout)`` and nothing else of it touched (include/pcdm.h: pcdm_conv2d_f32_ex)."""
    _c(x, torch.float32)
    B, Hi, Wi, Cin = (int(v) for v in x.shape)
    assert Cin == pw["cin"], (Cin, pw["cin"])
    ph, pwd = int(pad[0]), int(pad[1])
    Ho, Wo = (Hi + 2 * ph - pw["kh"]) // stride + 1, (Wi + 2 * pwd - pw["kw"]) // stride + 1
    if Ho < 1 or Wo < 1:
        raise ValueError(f"a {pw['kh']} x {pw['kw']} kernel does not fit a {Hi} x {Wi} image padded by {(ph, pwd)}")
    if out is None:
        out = torch.empty((B, Ho, Wo, pw["cout"]), dtype=torch.float32, device=x.device)
    _c(out, torch.float32)
    if out.dim() != 4 or tuple(out.shape[:3]) != (B, Ho, Wo) or out.device != x.device:
        raise ValueError(f"out {tuple(out.shape)} on {out.device}: expected [{B}, {Ho}, {Wo}, pitch] on {x.device}")
    _chk(_lib.lib().pcdm_conv2d_f32_ex(_ptr(x), B, Hi, Wi, Cin, _ptr(pw["w"]), _ptr(pw["bias"]), pw["cout"], pw["kh"], pw["kw"], int(stride), ph, pwd,
                                       int(relu), _ptr(out), int(out.shape[3]), int(offset), _stream(x)), "pcdm_conv2d_f32_ex")
    return out


def maxpool3s2_f32_ex(x: torch.Tensor, out: torch.Tensor, offset: int = 0) -> torch.Tensor:
    """MaxPool2d(3, stride 2) of NHWC fp32 ``x`` into the channels ``[offset, offset + C)`` of ``out`` [B, Ho, Wo, pitch]
    (include/pcdm.h: pcdm_maxpool3s2_f32_ex)."""
    _c(x, torch.float32); _c(out, torch.float32)
    B, Hi, Wi, Cn = (int(v) for v in x.shape)
    if Hi < 3 or Wi < 3 or tuple(out.shape[:3]) != (B, (Hi - 3) // 2 + 1, (Wi - 3) // 2 + 1) or out.device != x.device:
        raise ValueError(f"x {tuple(x.shape)}, out {tuple(out.shape)}")
    _chk(_lib.lib().pcdm_maxpool3s2_f32_ex(_ptr(x), B, Hi, Wi, Cn, _ptr(out), int(out.shape[3]), int(offset), _stream(x)), "pcdm_maxpool3s2_f32_ex")
    return out


def avgpool3_f32(x: torch.Tensor) -> torch.Tensor:
    """F.avg_pool2d(x, 3, 1, 1) (count_include_pad) on NHWC fp32 (include/pcdm.h: pcdm_avgpool3_f32)."""
    _c(x, torch.float32)
    B, H, W, Cn = (int(v) for v in x.shape)
    out = torch.empty_like(x)
    _chk(_lib.lib().pcdm_avgpool3_f32(_ptr(x), B, H, W, Cn, _ptr(out), _stream(x)), "pcdm_avgpool3_f32")
    return out


def global_avgpool_f32(x: torch.Tensor) -> torch.Tensor:
    """NHWC fp32 [B, H, W, C] -> fp32 [B, C]: the spatial mean, summed in fp64 in pixel order (include/pcdm.h: pcdm_global_avgpool_f32)."""
    _c(x, torch.float32)
    B, H, W, Cn = (int(v) for v in x.shape)
    out = torch.empty((B, Cn), dtype=torch.float32, device=x.device)
    call = lambda: _lib.lib().pcdm_global_avgpool_f32(_ptr(x), B, H * W, Cn, _ptr(out), _stream(x))  # noqa: E731
    _chk(_launch(x, call, "global_avgpool", float(x.numel()), (B, H, W, Cn)), "pcdm_global_avgpool_f32")
    return out


def _image_batch(img: torch.Tensor):
    assert img.dim() == 4 and img.dtype in (torch.uint8, torch.float32) and img.is_contiguous(), (img.shape, img.dtype)
    f32 = int(img.dtype == torch.float32)
    H, W = (img.shape[2:]) if f32 else (img.shape[1:3])
    assert (img.shape[1] if f32 else img.shape[3]) == 3, img.shape
    return f32, int(H), int(W)


def inception_input(img: torch.Tensor, win: Sequence[int], *, resize: bool, normalize: bool) -> torch.Tensor:
    """uint8 NHWC [N, Hi, Wi, 3] or fp32 NCHW [N, 3, Hi, Wi], window (x0, y0, W, H) -> fp32 NHWC [N, 299 | H, 299 | W, 4]: the bilinear resample and
    the reference's remap (include/pcdm.h: pcdm_inception_input)."""
    f32, H, W = _image_batch(img)
    Ho, Wo = (299, 299) if resize else (int(win[3]), int(win[2]))
    out = torch.empty((img.shape[0], Ho, Wo, 4), dtype=torch.float32, device=img.device)
    _chk(_lib.lib().pcdm_inception_input(_ptr(img), img.shape[0], H, W, _win(win), f32, int(resize), int(normalize), _ptr(out), _stream(img)),
         "pcdm_inception_input")
    return out


def inception_ws_bytes(B: int, H: int, W: int, dims: int) -> int:
    """Workspace bytes of ``inception_features`` for an H x W network input; -1: the library refuses the problem."""
    return int(_lib.lib().pcdm_inception_ws_bytes(int(B), int(H), int(W), int(dims)))


def inception_features(img: torch.Tensor, win: Sequence[int], weights: "_lib.InceptionWeights", out: torch.Tensor, ws: torch.Tensor, *, dims: int,
                       resize: bool, normalize: bool) -> torch.Tensor:
    """The InceptionV3 trunk as one C call: out fp32 [N, dims] (include/pcdm.h: pcdm_inception_features)."""
    f32, H, W = _image_batch(img)
    _c(out, torch.float32)
    assert out.device == img.device and ws.device == img.device
    _chk(_lib.lib().pcdm_inception_features(_ptr(img), img.shape[0], H, W, _win(win), f32, int(resize), int(normalize), int(dims), C.byref(weights),
                                            _ptr(out), _ptr(ws), ws.numel() * ws.element_size(), _stream(img)), "pcdm_inception_features")
    return out


def fid_accumulate(feat: torch.Tensor, total: torch.Tensor, gram: torch.Tensor) -> None:
    """total fp64 [D] += sum_b feat[b], gram fp64 [D, D] += sum_b feat[b] feat[b]^T for feat fp32 [B, D] (include/pcdm.h: pcdm_fid_accumulate)."""
    _c(feat, torch.float32); _c(total, torch.float64); _c(gram, torch.float64)
    B, D = (int(v) for v in feat.shape)
    assert tuple(total.shape) == (D,) and tuple(gram.shape) == (D, D) and total.device == feat.device and gram.device == feat.device
    _chk(_lib.lib().pcdm_fid_accumulate(_ptr(feat), B, D, _ptr(total), _ptr(gram), _stream(feat)), "pcdm_fid_accumulate")


def fid_finalize(total: torch.Tensor, gram: torch.Tensor, n: int):
    """-> (mu fp64 [D], sigma fp64 [D, D]) on the device: the mean and the ddof-1 covariance of the n accumulated samples
    (include/pcdm.h: pcdm_fid_finalize)."""
    _c(total, torch.float64); _c(gram, torch.float64)
    D = int(total.shape[0])
    assert tuple(total.shape) == (D,) and tuple(gram.shape) == (D, D) and gram.device == total.device, (total.shape, gram.shape)
    mu, sigma = torch.empty_like(total), torch.empty_like(gram)
    _chk(_lib.lib().pcdm_fid_finalize(_ptr(total), _ptr(gram), int(n), D, _ptr(mu), _ptr(sigma), _stream(total)), "pcdm_fid_finalize")
    return mu, sigma


# ------------------------------------------------------------------------------------ input preparation (pcdms_amd/preprocess.py is the public surface)
def resample_ws_bytes(Hs: int, Ws: int, Hd: int, Wd: int, channels: int, ky: int) -> int:
    """Workspace bytes of ``resample_u8`` (0: one launch, no workspace); -1: the library refuses the problem."""
    return int(_lib.lib().pcdm_resample_ws_bytes(Hs, Ws, Hd, Wd, channels, ky))


def resample_u8(src: torch.Tensor, xtab: Optional[torch.Tensor], kx: int, ytab: Optional[torch.Tensor], ky: int, dst: torch.Tensor, size: Sequence[int],
                at: Sequence[int], ws: Optional[torch.Tensor]) -> torch.Tensor:
    """src uint8 [Hs, Ws, C] -> the window ``size`` = (Wd, Hd) at pixel ``at`` = (x0, y0) of the uint8 canvas dst [Hc, Wc, C], by the int32 device
    tables of the two axes (None: the axis keeps its size); include/pcdm.h: pcdm_resample_u8."""
    _c(src, torch.uint8); _c(dst, torch.uint8)
    assert src.dim() == 3 and dst.dim() == 3 and src.shape[2] == dst.shape[2] and src.device == dst.device, (src.shape, dst.shape)
    Wd, Hd = int(size[0]), int(size[1])
    x0, y0 = int(at[0]), int(at[1])
    if x0 < 0 or y0 < 0 or x0 + Wd > dst.shape[1] or y0 + Hd > dst.shape[0]:
        raise ValueError(f"a {Wd} x {Hd} window at ({x0}, {y0}) leaves the {dst.shape[1]} x {dst.shape[0]} canvas")
    for t in (xtab, ytab):
        if t is not None:
            _c(t, torch.int32)
    _chk(_lib.lib().pcdm_resample_u8(_ptr(src), src.shape[0], src.shape[1], src.shape[2], _ptr(xtab), int(kx), _ptr(ytab), int(ky), _ptr(dst), Hd, Wd,
                                     dst.shape[1] * dst.shape[2], x0, y0, _ptr(ws), 0 if ws is None else ws.numel(), _stream(src)), "pcdm_resample_u8")
    return dst


def u8_to_nchw(src: torch.Tensor, win: Sequence[int], out: torch.Tensor, *, mode: int, scale: float, mean: Sequence[float],
               std: Sequence[float]) -> torch.Tensor:
    """out fp32 [1, C, H, W] <- (x - mean[c]) / std[c] over the window (x0, y0, W, H) of src uint8 [Hs, Ws, C]; mode 0: x = float(p) / float(scale),
    mode 1: x = float(double(p) * scale) (include/pcdm.h: pcdm_u8_to_nchw)."""
    _c(src, torch.uint8); _c(out, torch.float32)
    Cn = src.shape[2]
    assert src.dim() == 3 and out.numel() == Cn * int(win[2]) * int(win[3]) and len(mean) == Cn and len(std) == Cn
    _chk(_lib.lib().pcdm_u8_to_nchw(_ptr(src), src.shape[0], src.shape[1], Cn, _win(win), int(mode), float(scale), (C.c_float * Cn)(*mean),
                                    (C.c_float * Cn)(*std), _ptr(out), _stream(src)), "pcdm_u8_to_nchw")
    return out


def resize_cubic_f32(src: torch.Tensor, dst: torch.Tensor, index: int, *, nchw: bool, divisor: float = 0.0) -> torch.Tensor:
    """src uint8 / fp32 [Hs, Ws, 3] -> image ``index`` of the fp32 batch dst, [N, Hd, Wd, 3] or (``nchw``) [N, 3, Hd, Wd]: OpenCV's INTER_CUBIC
    for float images, divided by ``divisor`` when it is positive (include/pcdm.h: pcdm_resize_cubic_f32)."""
    assert src.dim() == 3 and dst.dim() == 4 and src.dtype in (torch.uint8, torch.float32) and src.is_contiguous() and src.device == dst.device, \
        (src.shape, src.dtype, dst.shape)
    _c(dst, torch.float32)
    N = dst.shape[0]
    chan, Hd, Wd = (dst.shape[1], dst.shape[2], dst.shape[3]) if nchw else (dst.shape[3], dst.shape[1], dst.shape[2])
    if chan != src.shape[2]:
        raise ValueError(f"source {tuple(src.shape)} and destination {tuple(dst.shape)} ({'NCHW' if nchw else 'NHWC'}) differ in channels")
    call = lambda: _lib.lib().pcdm_resize_cubic_f32(_ptr(src), int(src.dtype == torch.float32), src.shape[0], src.shape[1], src.shape[2], _ptr(dst),  # noqa: E731
                                                    N, Hd, Wd, int(index), int(bool(nchw)), float(divisor), _stream(src))
    _chk(_launch(src, call, "resize_cubic", 2.0 * 3 * Hd * Wd * 8 * 2, (src.shape[0], src.shape[1], Hd, Wd)), "pcdm_resize_cubic_f32")
    return dst


# ------------------------------------------------------------------------------------ pose maps (pcdms_amd/pose.py is the public surface)
POSE_TABLE_INTS = 740


def pose_tables() -> list:
    """The host-built constants of ``pose_draw``: {C, S} of every whole degree, then the 20 hand-edge colours (include/pcdm.h: pcdm_pose_tables)."""
    buf = (C.c_int32 * POSE_TABLE_INTS)()
    _chk(_lib.lib().pcdm_pose_tables(buf, POSE_TABLE_INTS), "pcdm_pose_tables")
    return list(buf)


def pose_ws_bytes(M: int, P: int) -> int:
    """Workspace bytes of ``pose_draw``; -1: the library refuses the problem."""
    return int(_lib.lib().pcdm_pose_ws_bytes(int(M), int(P)))


def pose_draw(keypoints: torch.Tensor, scores: torch.Tensor, tables: torch.Tensor, out: torch.Tensor, ws: Optional[torch.Tensor], *, hands: bool,
              faces: bool) -> torch.Tensor:
    """keypoints fp32 [M, P, 134, 2], scores fp32 [M, P, 134] -> out uint8 [M, H, W, 3], the pose maps (include/pcdm.h: pcdm_pose_draw)."""
    _c(keypoints, torch.float32); _c(scores, torch.float32); _c(tables, torch.int32); _c(out, torch.uint8)
    M, P = int(keypoints.shape[0]), int(keypoints.shape[1])
    assert tuple(keypoints.shape) == (M, P, 134, 2) and tuple(scores.shape) == (M, P, 134) and out.dim() == 4 and out.shape[0] == M and out.shape[3] == 3
    assert tables.numel() == POSE_TABLE_INTS and keypoints.device == scores.device == tables.device == out.device
    call = lambda: _lib.lib().pcdm_pose_draw(_ptr(keypoints), _ptr(scores), M, P, out.shape[1], out.shape[2], int(bool(hands)), int(bool(faces)),  # noqa: E731
                                             _ptr(tables), _ptr(out), _ptr(ws), 0 if ws is None else ws.numel(), _stream(out))
    _chk(_launch(out, call, "pose_draw", float(out.numel()), (M, P, out.shape[1], out.shape[2])), "pcdm_pose_draw")
    return out


def resize_linear_u8(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """src uint8 [M, Hs, Ws, 3] -> dst uint8 [M, Hd, Wd, 3]: OpenCV's 8-bit INTER_LINEAR (include/pcdm.h: pcdm_resize_linear_u8)."""
    _c(src, torch.uint8); _c(dst, torch.uint8)
    assert src.dim() == 4 and dst.dim() == 4 and src.shape[0] == dst.shape[0] and src.shape[3] == 3 and dst.shape[3] == 3 and src.device == dst.device
    call = lambda: _lib.lib().pcdm_resize_linear_u8(_ptr(src), src.shape[0], src.shape[1], src.shape[2], _ptr(dst), dst.shape[1], dst.shape[2],  # noqa: E731
                                                    _stream(src))
    _chk(_launch(src, call, "resize_linear_u8", float(dst.numel()), tuple(src.shape[1:3]) + tuple(dst.shape[1:3])), "pcdm_resize_linear_u8")
    return dst


RESIZE_CV_LANCZOS4, RESIZE_CV_AREA_INT, RESIZE_CV_AREA, RESIZE_CV_AREA_LINEAR = 0, 1, 2, 3   # pcdm_resize_cv_u8's `rule`


def resize_cv_table_ints(n_in: int, n_out: int, rule: int) -> int:
    """int32 entries of one axis table of ``resize_cv_u8`` (include/pcdm.h: pcdm_resize_cv_u8); 0: the rule reads no table."""
    if rule == RESIZE_CV_LANCZOS4:
        return n_out * 9
    if rule == RESIZE_CV_AREA_LINEAR:
        return n_out * 3
    if rule == RESIZE_CV_AREA:
        return n_out * (1 + 2 * (int(1.0 / (float(n_out) / float(n_in))) + 2))
    return 0


def resize_cv_u8(src: torch.Tensor, dst: torch.Tensor, rule: int, xtab: Optional[torch.Tensor] = None, ytab: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src uint8 [M, Hs, Ws, 3] -> dst uint8 [M, Hd, Wd, 3]: OpenCV's 8-bit INTER_LANCZOS4 / INTER_AREA in the arithmetic ``rule`` names, by the int32
    device tables of the two axes (None where the rule reads none: integer-ratio area, equal sizes); include/pcdm.h: pcdm_resize_cv_u8."""
    _c(src, torch.uint8); _c(dst, torch.uint8)
    assert src.dim() == 4 and dst.dim() == 4 and src.shape[0] == dst.shape[0] and src.shape[3] == 3 and dst.shape[3] == 3 and src.device == dst.device, \
        (src.shape, dst.shape)
    rule = int(rule)
    if rule not in (RESIZE_CV_LANCZOS4, RESIZE_CV_AREA_INT, RESIZE_CV_AREA, RESIZE_CV_AREA_LINEAR):
        raise ValueError(f"rule must be 0 .. 3: {rule}")
    (Hs, Ws), (Hd, Wd) = (int(v) for v in src.shape[1:3]), (int(v) for v in dst.shape[1:3])
    same = (Hs, Ws) == (Hd, Wd)
    for t, n_in, n_out, what in ((xtab, Ws, Wd, "xtab"), (ytab, Hs, Hd, "ytab")):
        need = 0 if same else resize_cv_table_ints(n_in, n_out, rule)
        if need == 0:
            assert t is None, f"{what}: rule {rule} reads no table for {n_in} -> {n_out}"
        else:
            assert t is not None and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == need and t.device == src.device, \
                (what, None if t is None else (t.dtype, t.is_contiguous(), t.numel()), need)
    call = lambda: _lib.lib().pcdm_resize_cv_u8(_ptr(src), src.shape[0], Hs, Ws, _ptr(dst), Hd, Wd, rule, _ptr(xtab), _ptr(ytab), _stream(src))  # noqa: E731
    _chk(_launch(src, call, "resize_cv_u8", float(dst.numel()), (Hs, Ws, Hd, Wd, rule)), "pcdm_resize_cv_u8")
    return dst


# ------------------------------------------------------------------------------------ pose estimator (pcdms_amd/pose.py: DWPoseEstimator is the public surface)
CONV_ACT_NONE, CONV_ACT_RELU, CONV_ACT_SILU = 0, 1, 2


def pose_crop(images: torch.Tensor, boxes: torch.Tensor, image_index: Optional[torch.Tensor], size: Sequence[int], *, flip: bool) -> torch.Tensor:
    """images uint8 [N, H, W, 3], boxes fp32 [R, 4] (x1, y1, x2, y2), image_index int32 [R] or None (image 0) -> the normalised crops fp32 NHWC
    [R or 2 R, Hin, Win, 4], ``size`` = (Hin, Win); with ``flip`` the second half is the first mirrored in x (include/pcdm.h: pcdm_pose_crop)."""
    _c(images, torch.uint8); _c(boxes, torch.float32)
    assert images.dim() == 4 and images.shape[3] == 3 and boxes.dim() == 2 and boxes.shape[1] == 4 and boxes.device == images.device, \
        (images.shape, boxes.shape)
    N, H, W = (int(v) for v in images.shape[:3])
    R, Hin, Win = int(boxes.shape[0]), int(size[0]), int(size[1])
    if image_index is not None:
        _c(image_index, torch.int32)
        assert tuple(image_index.shape) == (R,) and image_index.device == images.device
    out = torch.empty((R * (2 if flip else 1), Hin, Win, 4), dtype=torch.float32, device=images.device)
    call = lambda: _lib.lib().pcdm_pose_crop(_ptr(images), N, H, W, _ptr(boxes), _ptr(image_index), R, int(bool(flip)), Hin, Win, _ptr(out),  # noqa: E731
                                             _stream(images))
    _chk(_launch(images, call, "pose_crop", float(out.numel()), (N, H, W, R, Hin, Win)), "pcdm_pose_crop")
    return out


def conv2d_f32_act(x: torch.Tensor, pw: dict, *, stride: int = 1, pad: Sequence[int] = (0, 0), act: int = CONV_ACT_NONE, in_offset: int = 0,
                   residual: Optional[torch.Tensor] = None, res_offset: int = 0, a_scale: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, offset: int = 0) -> torch.Tensor:
    """``conv2d_f32_ex`` reading the channels ``[in_offset, in_offset + pw["cin"])`` of ``x`` NHWC fp32 [B, Hi, Wi, pitch], with an activation
    selector (``CONV_ACT_*``), an optional ``residual`` NHWC [B, Ho, Wo, pitch] whose channels ``[res_offset, res_offset + Cout)`` are added after the
    activation, and an optional ``a_scale`` fp32 [B, Cin] multiplied into the input per image and channel (include/pcdm.h: pcdm_conv2d_f32_act)."""
    _c(x, torch.float32)
    B, Hi, Wi, ldi = (int(v) for v in x.shape)
    Cin, Cout = pw["cin"], pw["cout"]
    ph, pwd = int(pad[0]), int(pad[1])
    Ho, Wo = (Hi + 2 * ph - pw["kh"]) // stride + 1, (Wi + 2 * pwd - pw["kw"]) // stride + 1
    if Ho < 1 or Wo < 1:
        raise ValueError(f"a {pw['kh']} x {pw['kw']} kernel does not fit a {Hi} x {Wi} image padded by {(ph, pwd)}")
    if out is None:
        out = torch.empty((B, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    _c(out, torch.float32)
    if out.dim() != 4 or tuple(out.shape[:3]) != (B, Ho, Wo) or out.device != x.device:
        raise ValueError(f"out {tuple(out.shape)} on {out.device}: expected [{B}, {Ho}, {Wo}, pitch] on {x.device}")
    ldr = 0
    if residual is not None:
        _c(residual, torch.float32)
        if residual.dim() != 4 or tuple(residual.shape[:3]) != (B, Ho, Wo) or residual.device != x.device:
            raise ValueError(f"residual {tuple(residual.shape)}: expected [{B}, {Ho}, {Wo}, pitch] on {x.device}")
        ldr = int(residual.shape[3])
    if a_scale is not None:
        _c(a_scale, torch.float32)
        if tuple(a_scale.shape) != (B, Cin) or a_scale.device != x.device:
            raise ValueError(f"a_scale {tuple(a_scale.shape)}: expected [{B}, {Cin}] on {x.device}")
    call = lambda: _lib.lib().pcdm_conv2d_f32_act(_ptr(x), B, Hi, Wi, Cin, ldi, int(in_offset), _ptr(pw["w"]), _ptr(pw["bias"]), Cout, pw["kh"],  # noqa: E731
                                                  pw["kw"], int(stride), ph, pwd, int(act), _ptr(residual), ldr, int(res_offset), _ptr(a_scale),
                                                  _ptr(out), int(out.shape[3]), int(offset), _stream(x))
    work = 2.0 * B * Ho * Wo * Cout * pw["kh"] * pw["kw"] * Cin
    _chk(_launch(x, call, "conv2d_f32_act", work, (B, Hi, Wi, Cin, Cout, pw["kh"], pw["kw"], stride)), "pcdm_conv2d_f32_act")
    return out


def dwconv5_silu_f32(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, *, in_offset: int = 0, offset: int = 0) -> torch.Tensor:
    """Depthwise 5 x 5 (pad 2) + bias + SiLU of the channels ``[in_offset, in_offset + C)`` of ``x`` NHWC fp32 into the channels ``[offset, offset + C)``
    of ``out``; ``w`` fp32 [25, C], ``bias`` [C] (include/pcdm.h: pcdm_dwconv5_silu_f32)."""
    _c(x, torch.float32); _c(w, torch.float32); _c(bias, torch.float32); _c(out, torch.float32)
    B, H, W, ldi = (int(v) for v in x.shape)
    Cn = int(bias.shape[0])
    assert tuple(w.shape) == (25, Cn) and tuple(out.shape[:3]) == (B, H, W) and out.device == x.device == w.device == bias.device, (x.shape, w.shape, out.shape)
    call = lambda: _lib.lib().pcdm_dwconv5_silu_f32(_ptr(x), B, H, W, Cn, ldi, int(in_offset), _ptr(w), _ptr(bias), _ptr(out), int(out.shape[3]),  # noqa: E731
                                                    int(offset), _stream(x))
    _chk(_launch(x, call, "dwconv5_silu", 50.0 * B * H * W * Cn, (B, H, W, Cn)), "pcdm_dwconv5_silu_f32")
    return out


def maxpool5_f32(x: torch.Tensor, Cn: int, out: torch.Tensor, *, in_offset: int = 0, offset: int = 0) -> torch.Tensor:
    """MaxPool2d(5, stride 1, pad 2) of the channels ``[in_offset, in_offset + Cn)`` of ``x`` NHWC fp32 into the channels ``[offset, offset + Cn)`` of
    ``out`` (which may be ``x``: disjoint slices); include/pcdm.h: pcdm_maxpool5_f32."""
    _c(x, torch.float32); _c(out, torch.float32)
    B, H, W, ldi = (int(v) for v in x.shape)
    assert tuple(out.shape[:3]) == (B, H, W) and out.device == x.device, (x.shape, out.shape)
    call = lambda: _lib.lib().pcdm_maxpool5_f32(_ptr(x), B, H, W, int(Cn), ldi, int(in_offset), _ptr(out), int(out.shape[3]), int(offset),  # noqa: E731
                                                _stream(x))
    _chk(_launch(x, call, "maxpool5", 25.0 * B * H * W * Cn, (B, H, W, Cn)), "pcdm_maxpool5_f32")
    return out


def fc_hsigmoid_f32(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """fp32 [B, C] -> hardsigmoid(x w^T + bias) with ``w`` [C, C] (include/pcdm.h: pcdm_fc_hsigmoid_f32)."""
    _c(x, torch.float32); _c(w, torch.float32); _c(bias, torch.float32)
    B, Cn = (int(v) for v in x.shape)
    assert tuple(w.shape) == (Cn, Cn) and tuple(bias.shape) == (Cn,) and w.device == x.device == bias.device, (x.shape, w.shape)
    out = torch.empty_like(x)
    call = lambda: _lib.lib().pcdm_fc_hsigmoid_f32(_ptr(x), B, Cn, _ptr(w), _ptr(bias), _ptr(out), _stream(x))  # noqa: E731
    _chk(_launch(x, call, "fc_hsigmoid", 2.0 * B * Cn * Cn, (B, Cn)), "pcdm_fc_hsigmoid_f32")
    return out


def scalenorm_f32(x: torch.Tensor, B: int, rows: int, dim: int, strides: Sequence[int], g: torch.Tensor, *, eps: float = 1e-5,
                  side_scale: Optional[torch.Tensor] = None) -> Union[torch.Tensor, tuple]:
    """ScaleNorm over ``dim`` elements of each of the ``B * rows`` rows of fp32 ``x``, element i of row (b, k) at flat index ``b strides[0] + k
    strides[1] + i strides[2]`` -> fp32 [B rows, dim rounded up to 4] (the padding columns 0); with ``side_scale`` fp32 [dim] also
    ``x * side_scale``, fp32 [B rows, dim] (include/pcdm.h: pcdm_scalenorm_f32)."""
    _c(x, torch.float32); _c(g, torch.float32)
    bs, rs, es = (int(v) for v in strides)
    if min(B, rows, dim, es) <= 0 or min(bs, rs) < 0 or (B - 1) * bs + (rows - 1) * rs + (dim - 1) * es >= x.numel():
        raise ValueError(f"{B} x {rows} rows of {dim} elements with strides {tuple(strides)} leave a tensor of {x.numel()} elements")
    out = torch.empty((B * rows, (dim + 3) // 4 * 4), dtype=torch.float32, device=x.device)
    side = None
    if side_scale is not None:
        _c(side_scale, torch.float32)
        assert tuple(side_scale.shape) == (dim,) and side_scale.device == x.device
        side = torch.empty((B * rows, dim), dtype=torch.float32, device=x.device)
    call = lambda: _lib.lib().pcdm_scalenorm_f32(_ptr(x), int(B), int(rows), int(dim), bs, rs, es, float(eps), _ptr(g), _ptr(out),  # noqa: E731
                                                 int(out.shape[1]), _ptr(side_scale), _ptr(side), int(dim), _stream(x))
    _chk(_launch(x, call, "scalenorm", 3.0 * B * rows * dim, (B, rows, dim)), "pcdm_scalenorm_f32")
    return out if side is None else (out, side)


def gau_core_f32(uv: torch.Tensor, B: int, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """uv fp32 [B T, 2 e + 128] = (u | v | base), gamma / beta fp32 [2, 128] -> fp32 [B T, e] = u * (relu(q k^T / sqrt(128))^2 v) per crop of T tokens
    (include/pcdm.h: pcdm_gau_core_f32)."""
    _c(uv, torch.float32); _c(gamma, torch.float32); _c(beta, torch.float32)
    rows, ld = (int(v) for v in uv.shape)
    e = (ld - 128) // 2
    if B <= 0 or rows % B or e <= 0 or 2 * e + 128 != ld or tuple(gamma.shape) != (2, 128) or tuple(beta.shape) != (2, 128):
        raise ValueError(f"uv {tuple(uv.shape)} for {B} crops, gamma {tuple(gamma.shape)}, beta {tuple(beta.shape)}")
    T = rows // B
    out = torch.empty((rows, e), dtype=torch.float32, device=uv.device)
    call = lambda: _lib.lib().pcdm_gau_core_f32(_ptr(uv), int(B), T, e, _ptr(gamma), _ptr(beta), _ptr(out), _stream(uv))  # noqa: E731
    _chk(_launch(uv, call, "gau_core", 2.0 * B * T * T * (128 + e), (B, T, e)), "pcdm_gau_core_f32")
    return out


def simcc_decode(logits: torch.Tensor, x_bins: int, R: int, K: int, flip_idx: Optional[torch.Tensor], boxes: torch.Tensor, size: Sequence[int]):
    """SimCC logits fp32 [R2 K, x bins + y bins] (x first; R2 = 2 R with ``flip_idx`` int32 [K]: the flip merge) and the boxes fp32 [R, 4] ->
    (keypoints fp32 [R, K, 2] in image pixels, scores fp32 [R, K]); ``size`` = (Hin, Win) (include/pcdm.h: pcdm_simcc_decode)."""
    _c(logits, torch.float32); _c(boxes, torch.float32)
    flip = flip_idx is not None
    rows = R * K * (2 if flip else 1)
    if R <= 0 or K <= 0 or logits.dim() != 2 or logits.shape[0] != rows or not 0 < x_bins < logits.shape[1] or tuple(boxes.shape) != (R, 4):
        raise ValueError(f"logits {tuple(logits.shape)} ({x_bins} x bins) and boxes {tuple(boxes.shape)} for {R} boxes of {K} keypoints, flip {flip}")
    if flip:
        _c(flip_idx, torch.int32)
        assert tuple(flip_idx.shape) == (K,) and flip_idx.device == logits.device
    ld = int(logits.shape[1])
    kp = torch.empty((R, K, 2), dtype=torch.float32, device=logits.device)
    sc = torch.empty((R, K), dtype=torch.float32, device=logits.device)
    call = lambda: _lib.lib().pcdm_simcc_decode(_ptr(logits), ld, int(x_bins), logits.data_ptr() + 4 * int(x_bins), ld, ld - int(x_bins), int(R),  # noqa: E731
                                                int(K), int(flip), _ptr(flip_idx), _ptr(boxes), int(size[0]), int(size[1]), _ptr(kp), _ptr(sc),
                                                _stream(logits))
    _chk(_launch(logits, call, "simcc_decode", float(logits.numel()), (R, K)), "pcdm_simcc_decode")
    return kp, sc


def dwpose_ws_bytes(cfg: "_lib.DWPoseConfig", R: int, flip: bool) -> int:
    """Workspace bytes of ``dwpose_forward``; -1: the library refuses the configuration."""
    return int(_lib.lib().pcdm_dwpose_ws_bytes(C.byref(cfg), int(R), int(bool(flip))))


def dwpose_forward(images: torch.Tensor, boxes: torch.Tensor, image_index: torch.Tensor, flip: bool, cfg: "_lib.DWPoseConfig",
                   weights: "_lib.DWPoseWeights", ws: torch.Tensor):
    """The whole estimator as one C call: images uint8 [N, H, W, 3], boxes fp32 [R, 4], image_index int32 [R] -> (keypoints fp32 [R, K, 2], scores
    fp32 [R, K]) (include/pcdm.h: pcdm_dwpose_forward)."""
    _c(images, torch.uint8); _c(boxes, torch.float32); _c(image_index, torch.int32)
    N, H, W = (int(v) for v in images.shape[:3])
    R = int(boxes.shape[0])
    assert images.dim() == 4 and images.shape[3] == 3 and tuple(boxes.shape) == (R, 4) and tuple(image_index.shape) == (R,)
    assert boxes.device == images.device == image_index.device == ws.device
    kp = torch.empty((R, cfg.K, 2), dtype=torch.float32, device=images.device)
    sc = torch.empty((R, cfg.K), dtype=torch.float32, device=images.device)
    _chk(_lib.lib().pcdm_dwpose_forward(_ptr(images), N, H, W, _ptr(boxes), _ptr(image_index), R, int(bool(flip)), C.byref(cfg), C.byref(weights),
                                        _ptr(kp), _ptr(sc), _ptr(ws), ws.numel() * ws.element_size(), _stream(images)), "pcdm_dwpose_forward")
    return kp, sc


# ------------------------------------------------------------------------------------ person detector (pcdms_amd/pose.py: PersonDetector is the public surface)
def detect_resized(H: int, W: int, S: int) -> tuple:
    """(Hr, Wr) of the aspect-preserving resize into the detector's S x S canvas (include/pcdm.h: pcdm_detect_resized)."""
    hr, wr = C.c_int(0), C.c_int(0)
    if _lib.lib().pcdm_detect_resized(int(H), int(W), int(S), C.byref(hr), C.byref(wr)) != 0:
        raise ValueError(f"the library refuses a {H} x {W} image for a {S} x {S} detector")
    return hr.value, wr.value


def detect_prep(images: torch.Tensor, S: int) -> torch.Tensor:
    """images uint8 RGB [N, H, W, 3] -> the detector's Focus tensor fp32 [N, S/2, S/2, 12] (include/pcdm.h: pcdm_detect_prep)."""
    _c(images, torch.uint8)
    assert images.dim() == 4 and images.shape[3] == 3, images.shape
    N, H, W = (int(v) for v in images.shape[:3])
    S = int(S)
    out = torch.empty((N, S // 2, S // 2, 12), dtype=torch.float32, device=images.device)
    call = lambda: _lib.lib().pcdm_detect_prep(_ptr(images), N, H, W, S, _ptr(out), _stream(images))  # noqa: E731
    _chk(_launch(images, call, "detect_prep", float(out.numel()), (N, H, W, S)), "pcdm_detect_prep")
    return out


def upsample2_nearest_f32(x: torch.Tensor, Cn: int, out: torch.Tensor, *, in_offset: int = 0, offset: int = 0) -> torch.Tensor:
    """Nearest x 2 of the channels ``[in_offset, in_offset + Cn)`` of ``x`` NHWC fp32 [B, H, W, pitch] into the channels ``[offset, offset + Cn)`` of
    ``out`` [B, 2 H, 2 W, pitch] (include/pcdm.h: pcdm_upsample2_nearest_f32)."""
    _c(x, torch.float32); _c(out, torch.float32)
    B, H, W, ldi = (int(v) for v in x.shape)
    assert tuple(out.shape[:3]) == (B, 2 * H, 2 * W) and out.device == x.device, (x.shape, out.shape)
    call = lambda: _lib.lib().pcdm_upsample2_nearest_f32(_ptr(x), B, H, W, int(Cn), ldi, int(in_offset), _ptr(out), int(out.shape[3]), int(offset),  # noqa: E731
                                                         _stream(x))
    _chk(_launch(x, call, "upsample2_nearest", 4.0 * B * H * W * Cn, (B, H, W, Cn)), "pcdm_upsample2_nearest_f32")
    return out


def detect_decode(heads: Sequence[torch.Tensor], S: int, num_classes: int, class_id: int, score_thr: float, image_size: Sequence[int]):
    """The three head tensors fp32 [N, S/stride, S/stride, 8 + C4] -> (boxes fp32 [N, P, 4] in pixels of the ``image_size`` = (H, W) image, scores
    [N, P], labels int32 [N, P], candidates int32 [N, P]) (include/pcdm.h: pcdm_detect_decode)."""
    h8, h16, h32 = heads
    S, Cn = int(S), int(num_classes)
    N, ldh = int(h8.shape[0]), 8 + (Cn + 3) // 4 * 4
    for h, st in zip(heads, (8, 16, 32)):
        _c(h, torch.float32)
        assert tuple(h.shape) == (N, S // st, S // st, ldh) and h.device == h8.device, (h.shape, (N, S // st, S // st, ldh))
    P = 21 * (S // 32) ** 2
    boxes = torch.empty((N, P, 4), dtype=torch.float32, device=h8.device)
    scores = torch.empty((N, P), dtype=torch.float32, device=h8.device)
    labels = torch.empty((N, P), dtype=torch.int32, device=h8.device)
    cand = torch.empty((N, P), dtype=torch.int32, device=h8.device)
    call = lambda: _lib.lib().pcdm_detect_decode(_ptr(h8), _ptr(h16), _ptr(h32), N, S, Cn, int(class_id), float(score_thr), int(image_size[0]),  # noqa: E731
                                                 int(image_size[1]), _ptr(boxes), _ptr(scores), _ptr(labels), _ptr(cand), _stream(h8))
    _chk(_launch(h8, call, "detect_decode", float(N * P * ldh), (N, S, Cn)), "pcdm_detect_decode")
    return boxes, scores, labels, cand


def nms_f32(boxes: torch.Tensor, scores: torch.Tensor, flags: torch.Tensor, *, thr: float, offset: float, max_candidates: int, max_det: int,
            overflow_in: Optional[torch.Tensor] = None, want_keep: bool = True, want_boxes: bool = True) -> dict:
    """One greedy NMS pass per image over the flagged boxes (include/pcdm.h: pcdm_nms_f32): boxes fp32 [N, P, 4], scores [N, P], flags int32 [N, P] ->
    ``{"keep" int32 [N, P], "boxes" [N, max_det, 4], "scores" [N, max_det], "count" int32 [N], "overflow" int32 [N]}``."""
    _c(boxes, torch.float32); _c(scores, torch.float32); _c(flags, torch.int32)
    N, P = (int(v) for v in scores.shape)
    assert tuple(boxes.shape) == (N, P, 4) and tuple(flags.shape) == (N, P) and boxes.device == scores.device == flags.device
    dev = boxes.device
    if overflow_in is not None:
        _c(overflow_in, torch.int32)
        assert tuple(overflow_in.shape) == (N,) and overflow_in.device == dev
    if not (0 < int(max_det) <= int(max_candidates)):
        raise ValueError(f"1 <= max_det <= max_candidates: {max_det}, {max_candidates}")
    keep = torch.empty((N, P), dtype=torch.int32, device=dev) if want_keep else None
    ob = torch.empty((N, int(max_det), 4), dtype=torch.float32, device=dev) if want_boxes else None
    os_ = torch.empty((N, int(max_det)), dtype=torch.float32, device=dev) if want_boxes else None
    count = torch.empty(N, dtype=torch.int32, device=dev)
    overflow = torch.empty(N, dtype=torch.int32, device=dev)
    call = lambda: _lib.lib().pcdm_nms_f32(_ptr(boxes), _ptr(scores), _ptr(flags), N, P, int(max_candidates), int(max_det), float(thr), float(offset),  # noqa: E731
                                           _ptr(overflow_in), _ptr(keep), _ptr(ob), _ptr(os_), _ptr(count), _ptr(overflow), _stream(boxes))
    _chk(_launch(boxes, call, "nms", float(N * P), (N, P, max_candidates, max_det)), "pcdm_nms_f32")
    return {"keep": keep, "boxes": ob, "scores": os_, "count": count, "overflow": overflow}


def detect_ws_bytes(cfg: "_lib.DetectConfig", N: int) -> int:
    """Workspace bytes of ``detect_forward``; -1: the library refuses the configuration."""
    return int(_lib.lib().pcdm_detect_ws_bytes(C.byref(cfg), int(N)))


def detect_forward(images: torch.Tensor, cfg: "_lib.DetectConfig", weights: "_lib.DetectWeights", ws: torch.Tensor):
    """The whole detector as one C call: images uint8 [N, H, W, 3] -> (boxes fp32 [N, max_det, 4], scores [N, max_det], count int32 [N], overflow
    int32 [N]) (include/pcdm.h: pcdm_detect_forward)."""
    _c(images, torch.uint8)
    assert images.dim() == 4 and images.shape[3] == 3 and images.device == ws.device
    N, H, W = (int(v) for v in images.shape[:3])
    dev = images.device
    boxes = torch.empty((N, cfg.max_det, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((N, cfg.max_det), dtype=torch.float32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    overflow = torch.empty(N, dtype=torch.int32, device=dev)
    _chk(_lib.lib().pcdm_detect_forward(_ptr(images), N, H, W, C.byref(cfg), C.byref(weights), _ptr(boxes), _ptr(scores), _ptr(count), _ptr(overflow),
                                        _ptr(ws), ws.numel() * ws.element_size(), _stream(images)), "pcdm_detect_forward")
    return boxes, scores, count, overflow
