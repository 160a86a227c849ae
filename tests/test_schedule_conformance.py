"""Stage-by-stage conformance of the UNet and VAE schedules against fp64 (the layer between the state dict and the kernels).

The kernels have their own fp64 suites (tests/test_gemm_conformance.py, test_attn_conformance.py, test_norm_conformance.py,
test_small_ops_conformance.py).  What composes them -- ``_pack`` (composed ``conv2s`` / ``ffo`` weights, LayerNorm-folded copies, the
concatenated ``time_emb_proj`` with its ``toff`` offsets, ``qkv`` / ``kv2``, the phase-decomposed upsampler), the ``resnet`` / ``transformer``
closures, ``prepare_conditioning`` and the VAE's ``_resnet`` / ``_mid`` / ``encode`` / ``_decode_buf`` -- was judged through the end of the network
only (rel-L2 of eps <= 2.5e-2), a tolerance under which one wrong layer disappears.  Here every tensor the schedule materialises is
compared with an fp64 restatement of the ONE stage that wrote it.

* **Teacher forcing.**  A stage's inputs are the product's own recorded tensors of the stage before (the ``_taps`` hook of
  pcdms_amd/unet.py and pcdms_amd/vae.py), so only that stage's error is measured.
* **Reference.**  ``torch.nn.functional`` in fp64 from the STATE DICT (``synth_state_dict(random_affine=True)``, every >= 2-D weight
  pre-rounded to bf16) -- never from a packed buffer.  Layouts (NHWC rows, the V^T pitch, ``vt_col0``, the phase-major columns of the
  upsampler, the ``dup_rows`` halves, the zero-context rows) are undone here from their documented form.
* **Yardstick.**  ``e_ref`` = rel-L2 from that reference of the SAME restatement (one function, a rounding argument) run in fp32 with
  every op boundary rounded to bf16.  fp32 outputs (``temb``, eps, moments, ``img4``, the embedding MLPs) round the operands only.
* **Bound.**  product <= 2 x e_ref per stage.  The product rounds at fewer points than the yardstick; the factor covers its re-rounded
  composed / folded weights (one more bf16 rounding per operand) and its different summation order.
* **Exception, derived.**  Where a stage's operands are bf16 already and its output is fp32 (``temb``, eps, ``img4``: a GEMM of
  recorded bf16 tensors with bf16 weights), nothing is left for the yardstick to round: e_ref is the fp32 accumulation error of
  ``F.conv2d`` / ``F.linear`` alone and carries no information about bf16: two summation orders of the same exact products, whose
  distance from fp64 differs by chance (measured on the MI355X: device / e_ref between 0.6 and 1.7).  There the bound is the larger of
  2 x e_ref and the accumulation bound of a K-term fp32 contraction: every partial sum is at most S = sum |a||w| + |bias| and each of
  the K additions rounds by at most 2^-24 of it, so |out - ref| <= K 2^-24 S per element in the worst case and sqrt(K) 2^-24 S as the
  random walk of K independent roundings; rel-L2 over the >= 1e3 outputs of a stage is the root MEAN square of that walk, so
  sqrt(K) 2^-24 ||S|| / ||ref|| bounds it without a margin for the maximum (tests/test_gemm_conformance.py and test_lpips.py state the same
  bound per element, with one).  K = the contraction length.  It is ~1e-5: three hundred times below one bf16 rounding, and
  ``test_faults_are_seen`` holds the faults of these stages to twice THIS bound.
* **The bound bites** (``test_faults_are_seen``, CPU only): every fault of a fixed list, applied to the reference side, must move the stage
  by >= 4 x e_ref (twice the bound).  The product's stand-in there is the yardstick chain itself.  Faults the reference cannot lift
  that far are named in profiles/schedule_conformance_values.json and may number at most 5 % of the list.

Measured values per stage and case: profiles/schedule_conformance_values.json; the worst ratio per model and backend goes through
tests/parity_record.check.
"""
from __future__ import annotations

import json
import math
import time
from pathlib import Path
from typing import Callable, Dict, List

import pytest
import torch
import torch.nn.functional as F

from oracle import vae as OV
from oracle.unet import UNetConfig, synth_state_dict
from pcdms_amd import ops
from pcdms_amd.unet import Stage2_InapintUNet2DConditionModel, UNet2DConditionModel
from pcdms_amd.vae import AutoencoderKL
from tests import parity_record
from tests.test_unet import _kwargs

ROOT = Path(__file__).resolve().parent.parent
VALUES_OUT = parity_record.OUT.parent / "schedule_conformance_values.json"   # the scratch directory of a test run (tests/parity_record.py)
FACTOR = 2.0          # product <= FACTOR x e_ref
BITE = 2.0 * FACTOR   # a fault must reach BITE x e_ref
BF = torch.bfloat16


def qbf(x: torch.Tensor) -> torch.Tensor:
    return x.to(BF).to(x.dtype)


def ident(x: torch.Tensor) -> torch.Tensor:
    return x


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def round_weights(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {k: (v.to(BF).float() if v.dim() >= 2 else v.float()) for k, v in sd.items()}


# ---------------------------------------------------------------------------------------------------------------- stages
class Stage:
    """One launch group of the schedule: ``fn(P, ins, q, fault)`` restates it on logical tensors (NCHW or [B, N, C]) in the dtype of its
    inputs; ``q`` rounds at the op boundaries inside it.  ``keys``: the state-dict tensors it reads.  ``fp32``: the product's output is fp32
    (the yardstick does not round it).  ``K``: contraction length of a stage whose operands are recorded bf16 tensors and whose output is
    fp32 (the derived accumulation bound of the module docstring); 0 elsewhere."""

    def __init__(self, name, ins, fn, keys=(), fp32=False, K=0, structural=()):
        self.name, self.ins, self.fn, self.keys, self.fp32, self.K, self.structural = name, list(ins), fn, list(keys), fp32, K, list(structural)

    def run(self, sd, T, dtype, q, fault=None, sub=None):
        P = _Params(sd, dtype, sub)
        out = self.fn(P, [None if n is None else (T[n].to(dtype) if torch.is_tensor(T[n]) and T[n].is_floating_point() else T[n]) for n in self.ins], q, fault)
        return out if (self.fp32 or q is ident) else q(out)


class _Params:
    def __init__(self, sd, dtype, sub=None):
        self.sd, self.dtype, self.sub = sd, dtype, sub or {}

    def __call__(self, key):
        return self.sd[self.sub.get(key, key)].to(self.dtype)

    def has(self, key):
        return key in self.sd


def _gn(x, G, P, p, eps, silu, q):
    y = F.group_norm(x, G, P(p + "weight"), P(p + "bias"), eps)
    return F.silu(q(y)) if silu else y


def _conv(x, P, p, **kw):
    return F.conv2d(x, P(p + "weight"), P(p + "bias"), **kw)


def _lin(x, P, p, bias=True):
    w = P(p + "weight")
    return F.linear(x, w.reshape(w.shape[0], -1), P(p + "bias") if bias else None)


def _ln(x, P, p):
    return F.layer_norm(x, (x.shape[-1],), P(p + "weight"), P(p + "bias"), 1e-5)


def _tokens(x):   # NCHW -> [B, HW, C]
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B, H * W, C)


def _attention(qh, kh, vh, heads, q, fault=None):
    """softmax(q k^T / sqrt(d)) v per head; [B, N, C] tensors, head h = channels [h d, (h + 1) d)."""
    B, N, C = qh.shape
    d = C // heads

    def split(t):
        if fault == "heads_dH":   # channels split as [d, H] instead of [H, d]
            return t.view(B, t.shape[1], d, heads).permute(0, 3, 1, 2)
        return t.view(B, t.shape[1], heads, d).transpose(1, 2)
    s = q(split(qh) @ split(kh).transpose(-1, -2) * d ** -0.5)
    o = q(torch.softmax(s, -1)) @ split(vh)
    if fault == "heads_dH":
        return o.permute(0, 2, 3, 1).reshape(B, N, C)
    return o.transpose(1, 2).reshape(B, N, C)


def _timestep_embedding(t, dim, dtype):
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=dtype) / half)
    a = t.to(dtype)[:, None] * f[None, :]
    return torch.cat([torch.cos(a), torch.sin(a)], -1)   # flip_sin_to_cos


class Plan:
    """The stage list of one model at one shape + how each product tap becomes a logical tensor."""

    def __init__(self):
        self.stages: List[Stage] = []
        self.layout: Dict[str, Callable] = {}     # logical tap name -> fn(product taps) -> tensor (bf16 / fp32 as recorded)
        self.optional: set = set()                # stages that exist only where the product recorded their tensor
        self.exact: List[Callable] = []           # extra exact checks on the product's taps: fn(T) -> None

    def add(self, stage: Stage, layout: Callable, optional=False):
        self.stages.append(stage)
        self.layout[stage.name] = layout
        if optional:
            self.optional.add(stage.name)


def _rows_nchw(name, B, H, W, cols=None):
    def f(taps):
        t = taps[name]
        b = t.shape[0] // (H * W)
        assert t.shape[0] == b * H * W and b in (B, B // 2), (name, t.shape, B, H, W)
        t = t.view(b, H, W, t.shape[-1])
        if cols is not None:
            assert not t[..., cols:].any(), f"{name}: padding channels not zero"
            t = t[..., :cols]
        return t.permute(0, 3, 1, 2)
    return f


def _rows_tok(name, N):
    return lambda taps: taps[name].view(-1, N, taps[name].shape[-1])


def _vt_tok(t, N):
    """V^T [B, C, pitch] (keys along the last axis, pitch = N rounded up to 16 bytes) -> V [B, N, C].  The padding columns are multiplied by
    P = 0 in the attention: they may hold an earlier, shorter sequence's values (the buffer is shared by shape) but must be finite."""
    assert t.shape[-1] == (N + 7) // 8 * 8 and torch.isfinite(t.float()).all(), "V^T pitch / padding"
    return t[..., :N].transpose(1, 2)


def unet_plan(cfg: UNetConfig, B, h, w, L, n0, *, pose=True, shared=False, t3=False, phase=True) -> Plan:
    pl = Plan()
    boc, G, eps, Lb = cfg.block_out_channels, cfg.norm_num_groups, cfg.norm_eps, cfg.layers_per_block
    nlev = len(boc)
    temb_dim = boc[0] * 4
    has_cls = cfg.class_embed_type == "projection"
    tk = lambda p: [p + "weight", p + "bias"]   # noqa: E731

    # ---- embeddings
    def f_mlp(p):
        def f(P, x, q):   # fp32 inside the product: the yardstick rounds the operands of each Linear only
            return _lin(q(F.silu(_lin(q(x), P, p + "linear_1."))), P, p + "linear_2.")
        return f
    if has_cls:
        pl.add(Stage("cls_emb", ["cl"], lambda P, I, q, ft: f_mlp("class_embedding.")(P, I[0].reshape(B, -1), q),
                     tk("class_embedding.linear_1.") + tk("class_embedding.linear_2."), fp32=True), lambda t: t["cls_emb"])

    def f_emb(P, I, q, ft):
        e = f_mlp("time_embedding.")(P, _timestep_embedding(I[0].expand(B), boc[0], P.dtype), q)
        if has_cls:
            e = e + f_mlp("class_embedding.")(P, I[1].reshape(B, -1), q)
        return F.silu(e)
    emb_keys = tk("time_embedding.linear_1.") + tk("time_embedding.linear_2.") + \
        (tk("class_embedding.linear_1.") + tk("class_embedding.linear_2.") if has_cls else [])
    pl.add(Stage("emb_act", ["t", "cl" if has_cls else None], f_emb, emb_keys, fp32=True), lambda t: t["emb_act"])
    pl.add(Stage("emb_bf", ["emb_act"], lambda P, I, q, ft: I[0]), lambda t: t["emb_bf"])

    # ---- inputs
    pl.add(Stage("x_in", ["sample"], lambda P, I, q, ft: I[0]), _rows_nchw("x_in_rows", B, h, w, cfg.in_channels))
    if pose:
        pl.add(Stage("pose_nhwc", ["pose"], lambda P, I, q, ft: I[0].expand(B, -1, -1, -1)), _rows_nchw("pose_rows", B, h, w))

    def f_ctx(P, I, q, ft):
        e = I[0].flip(0) if ft == "ctx_swapped" else I[0]   # the conditional and unconditional rows swapped
        return e[n0:]
    pl.add(Stage("ctx", ["ehs"], f_ctx, structural=["ctx_swapped"]), lambda t: t["ctx"].view(B - n0, L, -1))

    def f_conv_in(P, I, q, ft):
        y = _conv(I[0], P, "conv_in.", padding=1)
        if pose:
            y = q(y)
            pz = I[1]
            if ft == "pose_half":   # pose added to the first half of the batch only
                pz = torch.cat([pz[: B // 2], torch.zeros_like(pz[B // 2:])])
            y = y + pz
        return y
    pl.add(Stage("conv_in.out", ["x_in", "pose_nhwc" if pose else None], f_conv_in, tk("conv_in."), structural=["pose_half"] if pose else []),
           _rows_nchw("conv_in.out", B, h, w))

    # ---- blocks
    resnets: List[tuple] = []   # (prefix, toff, cout) in the order of the concatenated time_emb_proj

    def resnet(p, x, skip, cin, cout, hh, ww, first=False):
        sh = shared and first
        has_sc = cin != cout
        toff = sum(r[2] for r in resnets)
        resnets.append((p, toff, cout))
        pl.add(Stage(p + "temb", ["emb_bf"], lambda P, I, q, ft: _lin(I[0], P, p + "time_emb_proj."), tk(p + "time_emb_proj."), fp32=True, K=temb_dim,
                     structural=["toff"]), lambda t: t["temb"][:, toff: toff + cout])

        def cat(I, ft):
            if skip is None:
                return I[0]
            return torch.cat([I[1], I[0]] if ft == "skip_swapped" else [I[0], I[1]], 1)

        def f_n1(P, I, q, ft):
            xx = cat(I, ft)
            return _gn(xx[: B // 2] if sh else xx, G, P, p + "norm1.", eps, True, q)
        pl.add(Stage(p + "n1", [x, skip], f_n1, tk(p + "norm1."), structural=["skip_swapped"] if skip else []), _rows_nchw(p + "n1", B, hh, ww))

        def f_h1(P, I, q, ft):
            y = q(_conv(I[0], P, p + "conv1.", padding=1))
            if sh:   # the contraction once, written for both CFG halves (dup_rows)
                y = torch.cat([y, y])
            return y + I[1][:, :, None, None]
        pl.add(Stage(p + "h1", [p + "n1", p + "temb"], f_h1, tk(p + "conv1.")), _rows_nchw(p + "h1", B, hh, ww), optional=True)
        pl.add(Stage(p + "n2", [p + "n1", p + "temb"], lambda P, I, q, ft: _gn(q(f_h1(P, I, q, ft)), G, P, p + "norm2.", eps, True, q),
                     tk(p + "conv1.") + tk(p + "norm2.")), _rows_nchw(p + "n2", B, hh, ww))

        def f_out(P, I, q, ft):
            y = q(_conv(I[0], P, p + "conv2.", padding=1))
            xx = cat(I[1:], ft)
            if has_sc:
                xx = q(_conv(xx, P, p + "conv_shortcut."))
            return xx + y
        pl.add(Stage(p + "out", [p + "n2", x, skip], f_out, tk(p + "conv2.") + (tk(p + "conv_shortcut.") if has_sc else []),
                     structural=["skip_swapped"] if skip else []), _rows_nchw(p + "out", B, hh, ww))
        return p + "out"

    def transformer(p, x, c, heads, hh, ww):
        N, b = hh * ww, p + "transformer_blocks.0."
        Bc = B - n0
        pl.add(Stage(p + "n0", [x], lambda P, I, q, ft: _gn(I[0], G, P, p + "norm.", 1e-6, False, q), tk(p + "norm.")), _rows_nchw(p + "n0", B, hh, ww))
        pl.add(Stage(p + "t0", [p + "n0"], lambda P, I, q, ft: _lin(_tokens(I[0]), P, p + "proj_in."), tk(p + "proj_in.")), _rows_tok(p + "t0", N))

        def f_qkv(P, I, q, ft):
            n = q(_ln(I[0], P, b + "norm1."))
            return torch.cat([_lin(n, P, b + f"attn1.to_{s}.", False) for s in "qkv"], -1)
        pl.add(Stage(p + "qkv", [p + "t0"], f_qkv, tk(b + "norm1.") + [b + f"attn1.to_{s}.weight" for s in "qkv"]),
               lambda t: torch.cat([t[p + "qk"].view(B, N, 2 * c), _vt_tok(t[p + "vt"], N)], -1))
        pl.add(Stage(p + "at", [p + "qkv"], lambda P, I, q, ft: _attention(*I[0].split(c, -1), heads, q, ft),
                     structural=["heads_dH"] if heads > 1 and N > 1 else []),   # (one head, or one key: the split does not matter)
               _rows_tok(p + "at", N))
        pl.add(Stage(p + "t1", [p + "at", p + "t0"], lambda P, I, q, ft: q(_lin(I[0], P, b + "attn1.to_out.0.")) + I[1], tk(b + "attn1.to_out.0.")),
               _rows_tok(p + "t1", N))
        pl.add(Stage(p + "q2", [p + "t1"], lambda P, I, q, ft: _lin(q(_ln(I[0][n0:], P, b + "norm2.")), P, b + "attn2.to_q.", False),
                     tk(b + "norm2.") + [b + "attn2.to_q.weight"]), _rows_tok(p + "q2", N))
        pl.add(Stage(p + "kv2", ["ctx"], lambda P, I, q, ft: torch.cat([_lin(I[0], P, b + f"attn2.to_{s}.", False) for s in "kv"], -1),
                     [b + "attn2.to_k.weight", b + "attn2.to_v.weight"]),
               lambda t: torch.cat([t[p + "k2"].view(Bc, L, c), _vt_tok(t[p + "vt2"], L)], -1))
        pl.add(Stage(p + "at2", [p + "q2", p + "kv2"], lambda P, I, q, ft: _attention(I[0], *I[1].split(c, -1), heads, q, ft),
                     structural=["heads_dH"] if heads > 1 else []),
               _rows_tok(p + "at2", N))

        def f_t2(P, I, q, ft):   # the zero-context entries: attn2(x) == to_out.0.bias
            a = torch.cat([torch.zeros(n0, N, c, dtype=I[0].dtype), I[0]])
            return q(_lin(a, P, b + "attn2.to_out.0.")) + I[1]
        pl.add(Stage(p + "t2", [p + "at2", p + "t1"], f_t2, tk(b + "attn2.to_out.0.")), _rows_tok(p + "t2", N))

        def f_ff(P, I, q, ft):
            pr = q(_lin(q(_ln(I[0], P, b + "norm3.")), P, b + "ff.net.0.proj."))
            a, g = pr.chunk(2, -1)
            if ft == "geglu_swapped":
                a, g = g, a
            return a * q(F.gelu(g))
        pl.add(Stage(p + "ff", [p + "t2"], f_ff, tk(b + "norm3.") + tk(b + "ff.net.0.proj."), structural=["geglu_swapped"]), _rows_tok(p + "ff", N))

        def f_t3(P, I, q, ft):
            return q(_lin(I[0], P, b + "ff.net.2.")) + I[1]

        def f_proj(P, t3_, xx, q):
            y = q(_lin(t3_, P, p + "proj_out."))
            return y.reshape(B, hh, ww, c).permute(0, 3, 1, 2) + xx
        if t3:
            pl.add(Stage(p + "t3", [p + "ff", p + "t2"], f_t3, tk(b + "ff.net.2.")), _rows_tok(p + "t3", N))
            pl.add(Stage(p + "out", [p + "t3", x], lambda P, I, q, ft: f_proj(P, I[0], I[1], q), tk(p + "proj_out.")), _rows_nchw(p + "out", B, hh, ww))
        else:
            pl.add(Stage(p + "out", [p + "ff", p + "t2", x], lambda P, I, q, ft: f_proj(P, q(f_t3(P, I[:2], q, ft)), I[2], q),
                         tk(b + "ff.net.2.") + tk(p + "proj_out.")), _rows_nchw(p + "out", B, hh, ww))

        def zero_rows_exact(T):   # product only: bit for bit bf16(to_out.0.bias + residual) behind an all-zero context
            if n0 and "__sd" in T:
                want = (T["__sd"][b + "attn2.to_out.0.bias"].float() + T[p + "t1"][:n0].float()).to(BF)
                assert torch.equal(T[p + "t2"][:n0].to(BF), want), f"{p}t2: zero-context rows != to_out.0.bias + residual"
        pl.exact.append(zero_rows_exact)
        return p + "out"

    x = "conv_in.out"
    skips = [(x, h, w, boc[0])]
    hh, ww, ch = h, w, boc[0]
    for i, typ in enumerate(cfg.down_block_types):
        for j in range(Lb):
            x = resnet(f"down_blocks.{i}.resnets.{j}.", x, None, ch, boc[i], hh, ww, first=(i == 0 and j == 0))
            ch = boc[i]
            if typ == "CrossAttnDownBlock2D":
                x = transformer(f"down_blocks.{i}.attentions.{j}.", x, ch, cfg.attention_head_dim[i], hh, ww)
            skips.append((x, hh, ww, ch))
        if i != nlev - 1:
            p = f"down_blocks.{i}.downsamplers.0."
            ho, wo = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
            pl.add(Stage(p + "out", [x], (lambda p: lambda P, I, q, ft: _conv(I[0], P, p + "conv.", stride=2, padding=1))(p), tk(p + "conv.")),
                   _rows_nchw(p + "out", B, ho, wo))
            x, hh, ww = p + "out", ho, wo
            skips.append((x, hh, ww, ch))
    x = resnet("mid_block.resnets.0.", x, None, ch, ch, hh, ww)
    x = transformer("mid_block.attentions.0.", x, ch, cfg.attention_head_dim[-1], hh, ww)
    x = resnet("mid_block.resnets.1.", x, None, ch, ch, hh, ww)
    rev, rheads = list(reversed(boc)), list(reversed(cfg.attention_head_dim))
    for i, typ in enumerate(cfg.up_block_types):
        for j in range(Lb + 1):
            sk, sh_, sw_, sc_ = skips.pop()
            assert (sh_, sw_) == (hh, ww)
            x = resnet(f"up_blocks.{i}.resnets.{j}.", x, sk, ch + sc_, rev[i], hh, ww)
            ch = rev[i]
            if typ == "CrossAttnUpBlock2D":
                x = transformer(f"up_blocks.{i}.attentions.{j}.", x, ch, rheads[i], hh, ww)
        if i != nlev - 1:
            p = f"up_blocks.{i}.upsamplers.0."
            ho, wo = skips[-1][1], skips[-1][2]
            f_up = (lambda p, ho, wo: lambda P, I, q, ft: _conv(F.interpolate(I[0], size=(ho, wo), mode="nearest"), P, p + "conv.", padding=1))(p, ho, wo)
            if phase and (ho, wo) == (2 * hh, 2 * ww):   # phase-major columns: ph[b, y, x, (2 a + b') C + c] = out[b, 2 y + a, 2 x + b', c]
                pl.add(Stage(p + "ph", [x], f_up, tk(p + "conv.")),
                       (lambda p, hh, ww, ch: lambda t: t[p + "ph"].view(B, hh, ww, 2, 2, ch).permute(0, 5, 1, 3, 2, 4).reshape(B, ch, 2 * hh, 2 * ww))(p, hh, ww, ch),
                       optional=True)
            pl.add(Stage(p + "out", [x], f_up, tk(p + "conv.")), _rows_nchw(p + "out", B, ho, wo))
            x, hh, ww = p + "out", ho, wo
    pl.add(Stage("norm_out", [x], lambda P, I, q, ft: _gn(I[0], G, P, "conv_norm_out.", eps, True, q), tk("conv_norm_out.")), _rows_nchw("norm_out", B, h, w))
    pl.add(Stage("eps", ["norm_out"], lambda P, I, q, ft: _conv(I[0], P, "conv_out.", padding=1), tk("conv_out."), fp32=True, K=9 * boc[0]), lambda t: t["eps"])
    pl.resnets = resnets
    return pl


def vae_plan(cfg: OV.VAEConfig, B, H, W, which: str, *, phase=True) -> Plan:
    """``which``: "encode" (H x W the image) or "decode" (H x W the latent)."""
    pl = Plan()
    boc, G, Lb, zc = cfg.block_out_channels, cfg.norm_num_groups, cfg.layers_per_block, cfg.latent_channels
    tk = lambda p: [p + "weight", p + "bias"]   # noqa: E731

    def resnet(p, x, cin, cout, hh, ww):
        has_sc = cin != cout
        pl.add(Stage(p + "n1", [x], lambda P, I, q, ft: _gn(I[0], G, P, p + "norm1.", 1e-6, True, q), tk(p + "norm1.")), _rows_nchw(p + "n1", B, hh, ww))
        pl.add(Stage(p + "h1", [p + "n1"], lambda P, I, q, ft: _conv(I[0], P, p + "conv1.", padding=1), tk(p + "conv1.")), _rows_nchw(p + "h1", B, hh, ww))
        pl.add(Stage(p + "n2", [p + "h1"], lambda P, I, q, ft: _gn(I[0], G, P, p + "norm2.", 1e-6, True, q), tk(p + "norm2.")), _rows_nchw(p + "n2", B, hh, ww))
        if has_sc:
            pl.add(Stage(p + "sc", [x], lambda P, I, q, ft: _conv(I[0], P, p + "conv_shortcut."), tk(p + "conv_shortcut.")), _rows_nchw(p + "sc", B, hh, ww))
        pl.add(Stage(p + "out", [p + "n2", p + "sc" if has_sc else x], lambda P, I, q, ft: q(_conv(I[0], P, p + "conv2.", padding=1)) + I[1], tk(p + "conv2.")),
               _rows_nchw(p + "out", B, hh, ww))
        return p + "out"

    def mid(p, x, c, hh, ww):
        N, a = hh * ww, p + "attentions.0."
        x = resnet(p + "resnets.0.", x, c, c, hh, ww)
        pl.add(Stage(a + "n", [x], lambda P, I, q, ft: _gn(I[0], G, P, a + "group_norm.", 1e-6, False, q), tk(a + "group_norm.")), _rows_nchw(a + "n", B, hh, ww))
        pl.add(Stage(a + "qkv", [a + "n"], lambda P, I, q, ft: torch.cat([_lin(_tokens(I[0]), P, a + f"to_{s}.") for s in "qkv"], -1),
                     sum((tk(a + f"to_{s}.") for s in "qkv"), [])),
               lambda t: torch.cat([t[a + "qk"].view(B, N, 2 * c), _vt_tok(t[a + "vt"], N)], -1))
        pl.add(Stage(a + "at", [a + "qkv"], lambda P, I, q, ft: _attention(*I[0].split(c, -1), 1, q)), _rows_tok(a + "at", N))
        pl.add(Stage(a + "out", [a + "at", x], lambda P, I, q, ft: q(_lin(I[0], P, a + "to_out.0.")).reshape(B, hh, ww, c).permute(0, 3, 1, 2) + I[1],
                     tk(a + "to_out.0.")), _rows_nchw(a + "out", B, hh, ww))
        return resnet(p + "resnets.1.", a + "out", c, c, hh, ww)

    if which == "encode":
        pl.add(Stage("encoder.in", ["image"], lambda P, I, q, ft: I[0]), _rows_nchw("encoder.in_rows", B, H, W, cfg.in_channels))
        pl.add(Stage("encoder.conv_in.out", ["encoder.in"], lambda P, I, q, ft: _conv(I[0], P, "encoder.conv_in.", padding=1), tk("encoder.conv_in.")),
               _rows_nchw("encoder.conv_in.out", B, H, W))
        x, ch, hh, ww = "encoder.conv_in.out", boc[0], H, W
        for i in range(len(boc)):
            for j in range(Lb):
                x = resnet(f"encoder.down_blocks.{i}.resnets.{j}.", x, ch, boc[i], hh, ww)
                ch = boc[i]
            if i != len(boc) - 1:   # Downsample2D(padding=0): zero pad bottom / right only
                p = f"encoder.down_blocks.{i}.downsamplers.0."
                pl.add(Stage(p + "out", [x], (lambda p: lambda P, I, q, ft: _conv(F.pad(I[0], (0, 1, 0, 1)), P, p + "conv.", stride=2))(p), tk(p + "conv.")),
                       _rows_nchw(p + "out", B, hh // 2, ww // 2))
                x, hh, ww = p + "out", hh // 2, ww // 2
        x = mid("encoder.mid_block.", x, ch, hh, ww)
        pl.add(Stage("encoder.norm_out", [x], lambda P, I, q, ft: _gn(I[0], G, P, "encoder.conv_norm_out.", 1e-6, True, q), tk("encoder.conv_norm_out.")),
               _rows_nchw("encoder.norm_out", B, hh, ww))
        # conv_out then quant_conv: two layers in the state dict (the yardstick rounds quant_conv's operand), ONE launch in the product, whose
        # composed weight Wq Wo is rounded to bf16 once more
        pl.add(Stage("moments", ["encoder.norm_out"], lambda P, I, q, ft: _conv(q(_conv(I[0], P, "encoder.conv_out.", padding=1)), P, "quant_conv."),
                     tk("encoder.conv_out.") + tk("quant_conv."), fp32=True), lambda t: t["moments"])
    else:
        pl.add(Stage("decoder.in", ["z"], lambda P, I, q, ft: I[0]), _rows_nchw("decoder.in_rows", B, H, W, zc))
        pl.add(Stage("zq", ["decoder.in"], lambda P, I, q, ft: _conv(I[0], P, "post_quant_conv."), tk("post_quant_conv.")), _rows_nchw("zq", B, H, W, zc))
        rev = list(reversed(boc))
        pl.add(Stage("decoder.conv_in.out", ["zq"], lambda P, I, q, ft: _conv(I[0], P, "decoder.conv_in.", padding=1), tk("decoder.conv_in.")),
               _rows_nchw("decoder.conv_in.out", B, H, W))
        x = mid("decoder.mid_block.", "decoder.conv_in.out", rev[0], H, W)
        ch, hh, ww = rev[0], H, W
        for i in range(len(boc)):
            for j in range(Lb + 1):
                x = resnet(f"decoder.up_blocks.{i}.resnets.{j}.", x, ch, rev[i], hh, ww)
                ch = rev[i]
            if i != len(boc) - 1:
                p = f"decoder.up_blocks.{i}.upsamplers.0."
                f_up = (lambda p: lambda P, I, q, ft: _conv(F.interpolate(I[0], scale_factor=2.0, mode="nearest"), P, p + "conv.", padding=1))(p)
                if phase:
                    pl.add(Stage(p + "ph", [x], f_up, tk(p + "conv.")),
                           (lambda p, hh, ww, ch: lambda t: t[p + "ph"].view(B, hh, ww, 2, 2, ch).permute(0, 5, 1, 3, 2, 4).reshape(B, ch, 2 * hh, 2 * ww))(p, hh, ww, ch),
                           optional=True)
                pl.add(Stage(p + "out", [x], f_up, tk(p + "conv.")), _rows_nchw(p + "out", B, 2 * hh, 2 * ww))
                x, hh, ww = p + "out", 2 * hh, 2 * ww
        pl.add(Stage("decoder.norm_out", [x], lambda P, I, q, ft: _gn(I[0], G, P, "decoder.conv_norm_out.", 1e-6, True, q), tk("decoder.conv_norm_out.")),
               _rows_nchw("decoder.norm_out", B, hh, ww))

        def img_layout(t):
            assert not t["img4"][:, cfg.out_channels:].any(), "img4: the padding channel is not zero"
            return t["img4"][:, : cfg.out_channels]
        pl.add(Stage("img4", ["decoder.norm_out"], lambda P, I, q, ft: _conv(I[0], P, "decoder.conv_out.", padding=1), tk("decoder.conv_out."),
                     fp32=True, K=9 * ch), img_layout)
    return pl


# ---------------------------------------------------------------------------------------------------------------- comparison
def _abs_bound(stage: Stage, sd, T) -> torch.Tensor:
    """sum |a||w| + |bias| per output element of a K-term contraction stage (the accumulation bound of the module docstring)."""
    sd_abs = {k: v.abs() for k, v in sd.items()}
    Tabs = {n: (T[n].abs() if n is not None and torch.is_tensor(T[n]) and T[n].is_floating_point() else (T[n] if n is not None else None)) for n in stage.ins}
    # (moments: |Wq| (|Wo| |a| + |bo|) + |bq| bounds the composed contraction too)
    return stage.run(sd_abs, Tabs, torch.float64, ident)


def _bound(st: Stage, sd, T, ref, e_ref) -> float:
    bound = FACTOR * e_ref
    if st.K:
        bound = max(bound, math.sqrt(st.K) * 2.0 ** -24 * (_abs_bound(st, sd, T).norm() / ref.norm()).item())
    return bound


def compare(pl: Plan, sd, T):
    """Every stage of the plan against fp64 with teacher forcing.  ``T``: logical taps (+ the raw inputs).  Returns rows
    (name, e_ref, e_dev, bound) and the failures."""
    rows, fails = [], []
    for st in pl.stages:
        if st.name not in T:
            assert st.name in pl.optional, f"tap missing: {st.name}"
            continue
        ref = st.run(sd, T, torch.float64, ident)
        yard = st.run(sd, T, torch.float32, qbf)
        got = T[st.name]
        assert got.shape == ref.shape, (st.name, got.shape, ref.shape)
        assert torch.isfinite(got.float()).all(), st.name
        e_ref, e_dev = rel(yard, ref), rel(got, ref)
        bound = _bound(st, sd, T, ref, e_ref)
        rows.append((st.name, e_ref, e_dev, bound))
        if not e_dev <= bound:
            fails.append(f"{st.name}: device {e_dev:.3e} > bound {bound:.3e} (e_ref {e_ref:.3e})")
    return rows, fails


def _record(case: str, backend_name: str, rows, extra=None):
    try:
        VALUES_OUT.parent.mkdir(exist_ok=True)
        cur = json.loads(VALUES_OUT.read_text()) if VALUES_OUT.exists() else {}
        cur[f"{backend_name}/{case}"] = dict(stages={n: dict(e_ref=float(f"{a:.4g}"), device=float(f"{b:.4g}"), ratio=float(f"{b / c * FACTOR:.4g}") if c else 0.0)
                                                     for n, a, b, c in rows}, **(extra or {}))
        VALUES_OUT.write_text(json.dumps(cur, indent=0, sort_keys=True))
    except OSError:
        pass


def _worst(rows) -> float:
    """Worst device / bound ratio in units of e_ref (the bound is FACTOR)."""
    return max((b / c * FACTOR) for _, _, b, c in rows if c > 0)


def _finish(model: str, case: str, backend, rows, fails, extra=None):
    _record(case, backend.name, rows, extra)
    for n, a, b, c in rows:
        print(f"{case:28s} {n:58s} e_ref {a:.3e} device {b:.3e} ratio {b / c * FACTOR if c else 0:.3f}")
    assert not fails, f"{case}: {len(fails)} of {len(rows)} stages beyond {FACTOR} x e_ref\n" + "\n".join(fails)
    parity_record.check(f"schedule_conformance/{model}/{backend.name}/{case}", _worst(rows), FACTOR)


# ---------------------------------------------------------------------------------------------------------------- UNet cases
def _unet_inputs(cfg, B, h, w, L, n0, pose=True, shared=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(B, cfg.in_channels, h, w, generator=g)
    if shared:
        s = torch.cat([s[: B // 2], s[: B // 2]])
    e = torch.randn(B, L, cfg.cross_attention_dim, generator=g)
    e[:n0] = 0
    c = None if cfg.projection_class_embeddings_input_dim is None else torch.randn(B, 1, cfg.projection_class_embeddings_input_dim, generator=g) * 0.4
    p = torch.randn(1, cfg.block_out_channels[0], h, w, generator=g) * 0.1 if pose else None
    return s, e, c, p


def _unet_logical(pl: Plan, taps, sd, raw) -> dict:
    """Product taps -> logical tensors (on the host), by the documented layouts."""
    t = {k: v.detach().cpu() for k, v in taps.items()}
    x_in = t["x_in"]
    t["x_in_rows"] = x_in.reshape(-1, x_in.shape[-1])
    if "pose_nhwc" in t:
        t["pose_rows"] = t["pose_nhwc"].reshape(-1, t["pose_nhwc"].shape[-1])
    T = dict(raw)
    for name, f in pl.layout.items():
        try:
            T[name] = f(t)
        except KeyError:
            assert name in pl.optional, f"tap missing: {name}"
    T["__sd"] = sd
    return T


def _run_unet(backend, cfg, B, h, w, L, n0, *, cls=Stage2_InapintUNet2DConditionModel, pose=True, shared=False, force=None, t=981, c_schedule=False):
    """One tapped forward of the Python schedule.  ``force``: fn(recorded problem keys, table) that pins table entries after a first,
    recording forward (tests/test_unet_ctx.py's table forcing)."""
    from pcdms_amd import unet as U
    dev = backend.device
    sd = round_weights(synth_state_dict(cfg, seed=0, random_affine=True))
    m = cls(**_kwargs(cfg), layers_per_block=cfg.layers_per_block)
    m.load_state_dict(sd)
    m.to(dev)
    s, e, c, p = _unet_inputs(cfg, B, h, w, L, n0, pose, shared)
    tt = torch.tensor([t], dtype=torch.int64, device=dev)
    m._pack()
    x_in = ops.nchw_to_nhwc_bf16(s.to(dev), cpad=m._w["conv_in"].cin)

    def forward(taps):
        m._taps = taps
        try:
            cond = m.prepare_conditioning(B, h, w, e.to(dev), None if c is None else c.to(dev), None if p is None else p.to(dev), zero_ctx_batches=n0,
                                          shared_cfg_input=shared)
            assert cond.shared_halves == shared
            out = m._forward_nhwc(x_in, B, h, w, tt, cond).clone()
        finally:
            m._taps = None
        backend.sync()
        return out
    wall = None
    if force is not None or not backend.is_emu:
        forward(None)                      # records the problem keys (and, on the GPU, tunes unseen shapes)
        if force is not None:
            force()
        t0 = time.perf_counter()
        plain = forward(None)
        wall = time.perf_counter() - t0
    taps: dict = {}
    out = forward(taps)
    if wall is not None:
        assert torch.equal(out, plain), "the tap hook changed the result"
    assert torch.equal(taps["eps"].cpu(), out.cpu())
    pl = unet_plan(cfg, B, h, w, L, n0, pose=pose, shared=shared, t3=not U.FUSE_FF_OUT, phase=U.PHASE_UPSAMPLE)
    raw = dict(sample=s, t=torch.tensor([t]), ehs=e, cl=c, pose=p)
    T = _unet_logical(pl, taps, sd, raw)
    for f in pl.exact:
        f(T)
    if c_schedule:   # pcdm_unet_forward has no taps: its eps must equal the Python schedule's bit for bit
        from pcdms_amd.unet_ctx import UNetContext
        ctx = UNetContext(m)
        pose_b = ctx.prepare_conditioning(B, h, w, e, c, p, zero_ctx_batches=n0)
        out_c = ctx.forward(x_in, tt, None, B, h, w, pose_b)
        backend.sync()
        assert torch.equal(out_c, out), (out_c - out).abs().max()
    rows, fails = compare(pl, sd, T)
    return pl, taps, rows, fails, wall


def _tiny_shape(backend):
    return (2, 8, 8, 5, 1) if backend.is_emu else (4, 16, 24, 10, 2)


def test_unet_tiny(backend):
    pl, taps, rows, fails, _ = _run_unet(backend, UNetConfig.tiny(), *_tiny_shape(backend))
    # existing keys of the hook keep their meaning (tests/test_fullsize_parity.py reads them)
    assert torch.equal(taps["conv_in"], taps["conv_in.out"]) and torch.equal(taps["down0.0"], taps["down_blocks.0.attentions.0.out"])
    assert torch.equal(taps["ds0"], taps["down_blocks.0.downsamplers.0.out"]) and torch.equal(taps["up1.0"], taps["up_blocks.1.attentions.0.out"])
    assert any(n.endswith(".ph") for n, *_ in rows)          # the phase-decomposed upsampler ran
    _finish("unet", "tiny", backend, rows, fails)


def test_unet_tiny_unfused(backend, monkeypatch):
    """``FUSE_SHORTCUT`` / ``FUSE_FF_OUT`` off: conv_shortcut and ff.net.2 as launches of their own (``sc`` / ``t3`` are materialised)."""
    from pcdms_amd import unet as U
    monkeypatch.setattr(U, "FUSE_SHORTCUT", False)
    monkeypatch.setattr(U, "FUSE_FF_OUT", False)
    pl, taps, rows, fails, _ = _run_unet(backend, UNetConfig.tiny(), *_tiny_shape(backend))
    assert any(n.endswith(".t3") for n, *_ in rows) and any(k.endswith(".sc") for k in taps)
    _finish("unet", "tiny_unfused", backend, rows, fails)


@pytest.mark.gpu
def test_unet_shared_cfg_input(gpu_backend):
    """``shared_cfg_input=True``: conv_in, the first norm1 and the first conv1's contraction for B/2 entries, written for both halves."""
    pl, taps, rows, fails, _ = _run_unet(gpu_backend, UNetConfig.tiny(), 4, 16, 24, 10, 2, shared=True)
    assert taps["down_blocks.0.resnets.0.n1"].shape[0] == 2 * 16 * 24
    _finish("unet", "shared_cfg", gpu_backend, rows, fails)


class _Rec(dict):
    def __init__(self, *a):
        super().__init__(*a)
        self.seen = []

    def get(self, k, d=None):
        self.seen.append(k)
        return super().get(k, d)


@pytest.mark.gpu
def test_unet_forced_splitk_and_folded_layernorm(gpu_backend, monkeypatch):
    """Every 3x3 convolution on a split-K configuration with the reduce deferred into the consuming GroupNorm, and the LayerNorm ->
    Linear pairs on the folded instances with producer partials (the table forcing of tests/test_unet_ctx.py)."""
    cfg = UNetConfig.tiny()
    rec = _Rec(ops._TUNED)
    monkeypatch.setattr(ops, "_TUNED", rec)
    made = []
    orig = ops.DeferredGemm.__init__
    monkeypatch.setattr(ops.DeferredGemm, "__init__", lambda self, **kw: (made.append(kw["store"]), orig(self, **kw))[1])
    widths = set(cfg.block_out_channels)
    n = {}

    def force():
        conv = ln = prod = 0
        for k in set(rec.seen):
            if k[0] == "ln":
                _, M, Npad, K, epi = k
                if K % 64 == 0 and K != 320 and (epi != ops.EPI_GEGLU or Npad % 128 == 0):
                    dict.__setitem__(rec, k, (4 if epi == ops.EPI_GEGLU else 2, 2))
                    ln += 1
            elif isinstance(k[0], int) and k[3] and k[6] == ops.EPI_STORE and k[2] // 64 >= 4 and k[1] % 64 == 0:
                dict.__setitem__(rec, k, (2, 2))
                conv += 1
            elif isinstance(k[0], int) and not k[3] and k[6] == ops.EPI_STORE and k[2] in widths and k[1] == k[2] and \
                    ((not k[7] and len(k) == 9) or (len(k) == 10 and k[9] is True)):
                dict.__setitem__(rec, k, (2, 1))
                prod += 1
        n.update(conv=conv, ln=ln, prod=prod)
        del made[:]
    pl, taps, rows, fails, _ = _run_unet(gpu_backend, cfg, 4, 16, 24, 10, 2, force=force)
    assert n["conv"] >= 6 and n["ln"] >= 6 and n["prod"] >= 4, n
    assert any(made) and not all(made)                         # stored (block outputs) and not stored (conv1) deferrals both happened
    assert not any(k.endswith("resnets.0.h1") for k in taps if k.startswith("mid_block"))   # a deferred conv1 has no bf16 tensor
    _finish("unet", "forced_splitk_lnf", gpu_backend, rows, fails)


@pytest.mark.gpu
def test_unet_stage3_topology_odd_latent(gpu_backend):
    """The stock ``UNet2DConditionModel`` (in_channels 8, no class embedding, no pose) at latent 12 x 10: 12 -> 6 -> 3 -> 2 and 10 -> 5 -> 3 -> 2, so
    two upsamplers take the gather form (2 -> 3, 3 -> 5) and one the phase form."""
    cfg = UNetConfig.tiny(in_channels=8, class_embed_type=None, projection_class_embeddings_input_dim=None)
    pl, taps, rows, fails, _ = _run_unet(gpu_backend, cfg, 2, 12, 10, 7, 1, cls=UNet2DConditionModel, pose=False)
    assert "cls_emb" not in taps and "pose_nhwc" not in taps
    assert sum(k.endswith("upsamplers.0.ph") for k in taps) < sum(k.endswith("upsamplers.0.out") for k in taps)
    _finish("unet", "stage3_12x10", gpu_backend, rows, fails)


@pytest.mark.gpu
def test_unet_320_640(gpu_backend):
    """The smallest configuration with a 320-wide and a 640-wide cross-attention level: the K = 320 folded-LayerNorm weights of the
    A-in-registers kernel and the 640 LNF instances, which the tiny configuration never reaches.  Also: the C schedule's eps at these widths
    equals the Python schedule's bit for bit."""
    cfg = UNetConfig.tiny(block_out_channels=(320, 640, 640, 640), attention_head_dim=(5, 10, 10, 10))
    pl, taps, rows, fails, wall = _run_unet(gpu_backend, cfg, 2, 8, 8, 5, 1, c_schedule=True)
    print(f"320/640 forward after tuning: {wall * 1e3:.1f} ms")
    _finish("unet", "c320_640", gpu_backend, rows, fails, extra=dict(forward_ms=round(wall * 1e3, 2)))


# ---------------------------------------------------------------------------------------------------------------- VAE cases
def _vae_model(backend, cfg, seed=0):
    sd = round_weights(OV.synth_state_dict(cfg, seed))
    m = AutoencoderKL(block_out_channels=cfg.block_out_channels, layers_per_block=cfg.layers_per_block, latent_channels=cfg.latent_channels,
                      norm_num_groups=cfg.norm_num_groups)
    m.load_state_dict(sd)
    return sd, m.to(backend.device)


def _vae_logical(pl, taps, raw):
    t = {k: v.detach().cpu() for k, v in taps.items()}
    for k in ("encoder.in", "decoder.in"):
        if k in t:
            t[k + "_rows"] = t[k].reshape(-1, t[k].shape[-1])
    T = dict(raw)
    for name, f in pl.layout.items():
        try:
            T[name] = f(t)
        except KeyError:
            assert name in pl.optional, f"tap missing: {name}"
    return T


def _run_vae(backend, B, H, W):
    from pcdms_amd import unet as U
    cfg = OV.VAEConfig.tiny()
    sd, m = _vae_model(backend, cfg)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    z = torch.randn(B, 4, H // 8, W // 8, generator=g)
    dev = backend.device
    if not backend.is_emu:   # (tunes unseen shapes)
        m.encode(x.to(dev)), m._decode_buf(z.to(dev))
    taps: dict = {}
    m._taps = taps
    try:
        mom = m.encode(x.to(dev)).latent_dist.parameters
        backend.sync()
        enc_taps = dict(taps)
        taps.clear()
        img = m._decode_buf(z.to(dev)).clone()
        backend.sync()
        dec_taps = dict(taps)
    finally:
        m._taps = None
    assert torch.equal(enc_taps["moments"], mom) and torch.equal(dec_taps["img4"], img)
    out = []
    for which, tp, raw, hw in (("encode", enc_taps, dict(image=x), (H, W)), ("decode", dec_taps, dict(z=z), (H // 8, W // 8))):
        pl = vae_plan(cfg, B, hw[0], hw[1], which, phase=U.PHASE_UPSAMPLE)
        rows, fails = compare(pl, sd, _vae_logical(pl, tp, raw))
        out.append((which, rows, fails))
    return out


def test_vae_tiny(backend):
    B, H, W = (1, 64, 64) if backend.is_emu else (2, 128, 192)
    for which, rows, fails in _run_vae(backend, B, H, W):
        _finish("vae", f"tiny_{which}", backend, rows, fails)


@pytest.mark.gpu
def test_vae_mid_tokens_not_a_multiple_of_128(gpu_backend):
    """72 x 88: 9 x 11 = 99 mid-block tokens, the tail of ``attn_wide``'s 128-key blocks."""
    for which, rows, fails in _run_vae(gpu_backend, 1, 72, 88):
        _finish("vae", f"72x88_{which}", gpu_backend, rows, fails)


# ---------------------------------------------------------------------------------------------------------------- the bound bites
def _chain(pl: Plan, sd, raw) -> dict:
    """The product's stand-in without a device: the yardstick run as a chain (each stage fed the bf16 tensor of the stage before)."""
    T = dict(raw)
    for st in pl.stages:
        T[st.name] = st.run(sd, T, torch.float32, qbf).double()
    return T


def _faults_of(sd, key):
    """(name, faulted tensor) of every fault kind that applies to this parameter tensor."""
    v = sd[key]
    stem = key[: key.rfind(".") + 1]
    is_norm = sd[stem + "weight"].dim() == 1
    if key.endswith("bias"):
        yield ("beta_zero" if is_norm else "bias_zero"), torch.zeros_like(v)
        return
    if is_norm:
        yield "gamma_one", torch.ones_like(v)
        return
    for nm, dim in (("out_rows_zero", 0), ("in_cols_zero", 1)):   # the last 32 (at most half) output rows / input columns (3x3: channels)
        n = min(32, v.shape[dim] // 2)
        f = v.clone()
        f.narrow(dim, v.shape[dim] - n, n).zero_()
        yield nm, f
    if v.dim() == 4 and v.shape[-1] == 3:
        f = v.clone()
        f[:, :, 1, 1] = 0   # the centre tap: the only one a 1 x 1 level reads
        yield "tap_zero", f


def _fault_list(pl: Plan, sd):
    """(fault name, stage, kwargs of Stage.run) over every parameter tensor of every stage + the structural faults."""
    for st in pl.stages:
        for key in st.keys:
            for nm, f in _faults_of(sd, key):
                yield f"{key}:{nm}@{st.name}", key, st, dict(sd={**sd, key: f})
        for s in st.structural:
            if s == "toff":   # a neighbouring resnet's time_emb_proj of the same width
                p = st.name[: -len("temb")]
                i = [r[0] for r in pl.resnets].index(p)
                nb = next((r for r in pl.resnets[i + 1:] + pl.resnets[:i][::-1] if r[2] == pl.resnets[i][2]), None)
                if nb is None:
                    continue
                sub = {p + "time_emb_proj.weight": nb[0] + "time_emb_proj.weight", p + "time_emb_proj.bias": nb[0] + "time_emb_proj.bias"}
                yield f"{p}time_emb_proj:wrong_toff@{st.name}", None, st, dict(sd=sd, sub=sub)
            else:
                yield f"{s}@{st.name}", None, st, dict(sd=sd, fault=s)


def _seen(pl: Plan, sd, raw):
    """Per fault: the best over the stages that own it of (distance of the stand-in from the faulted reference) / e_ref (in general: / half the
    stage's bound)."""
    T = _chain(pl, sd, raw)
    unit = {}   # bound / FACTOR: e_ref, except for the stages with the derived accumulation bound
    for st in pl.stages:
        ref = st.run(sd, T, torch.float64, ident)
        unit[st.name] = _bound(st, sd, T, ref, rel(T[st.name], ref)) / FACTOR
    best: Dict[str, float] = {}
    for name, key, st, kw in _fault_list(pl, sd):
        bad = st.run(kw["sd"], T, torch.float64, ident, fault=kw.get("fault"), sub=kw.get("sub"))
        # (a fault that changes the stage's shape is seen by ``compare``'s shape assertion)
        ratio = rel(T[st.name], bad) / max(unit[st.name], 1e-300) if bad.shape == T[st.name].shape else math.inf
        fid = name.split("@")[0] if key is not None else name   # a parameter fault is seen if ANY stage that reads the tensor sees it
        best[fid] = max(best.get(fid, 0.0), ratio)
    return best


def test_faults_are_seen():
    """Every fault of the list moves its stage by >= 4 x e_ref (twice the bound); the ones that do not are named and number <= 5 %."""
    torch.manual_seed(0)
    unseen, total = {}, 0
    for model, cases in (("unet", [dict(), dict(t3=True)]), ("vae", ["encode", "decode"])):
        for case in cases:
            if model == "unet":
                cfg = UNetConfig.tiny()
                B, h, w, L, n0 = 2, 8, 8, 5, 1
                sd = round_weights(synth_state_dict(cfg, seed=0, random_affine=True))
                s, e, c, p = _unet_inputs(cfg, B, h, w, L, n0)
                pl = unet_plan(cfg, B, h, w, L, n0, **case)
                raw = dict(sample=s, t=torch.tensor([981]), ehs=e, cl=c, pose=p)
                label = "unet/tiny" + ("_unfused" if case else "")
            else:
                cfg = OV.VAEConfig.tiny()
                sd = round_weights(OV.synth_state_dict(cfg, 0))
                g = torch.Generator().manual_seed(1)
                x = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
                z = torch.randn(1, 4, 8, 8, generator=g)
                pl = vae_plan(cfg, 1, *((64, 64) if case == "encode" else (8, 8)), case)
                raw = dict(image=x) if case == "encode" else dict(z=z)
                label = f"vae/tiny_{case}"
            best = _seen(pl, sd, raw)
            total += len(best)
            for k, r in best.items():
                if r < BITE:
                    unseen[f"{label}:{k}"] = round(r, 3)
    try:
        VALUES_OUT.parent.mkdir(exist_ok=True)
        (VALUES_OUT.parent / "schedule_conformance_unseen_faults.json").write_text(json.dumps(dict(faults=total, unseen=unseen), indent=0, sort_keys=True))
    except OSError:
        pass
    print(f"{len(unseen)} of {total} faults below {BITE} x e_ref:", json.dumps(unseen, indent=0, sort_keys=True))
    assert total >= 800
    assert len(unseen) <= 0.05 * total, (len(unseen), total)
    committed = json.loads((ROOT / "profiles" / "schedule_conformance_values.json").read_text())["unseen_faults"]
    assert set(unseen) <= set(committed), sorted(set(unseen) - set(committed))   # every unseen fault is named in the values file


if __name__ == "__main__":   # refresh profiles/schedule_conformance_values.json from the files the tests left in the scratch directory
    dst = ROOT / "profiles" / "schedule_conformance_values.json"
    old = json.loads(dst.read_text()) if dst.exists() else {}
    cases = dict(old.get("cases", {}))
    if VALUES_OUT.exists():
        cases.update(json.loads(VALUES_OUT.read_text()))
    uf = VALUES_OUT.parent / "schedule_conformance_unseen_faults.json"
    faults = json.loads(uf.read_text()) if uf.exists() else dict(faults=old.get("faults", 0), unseen=old.get("unseen_faults", {}))
    uc = VALUES_OUT.parent / "cond_stack_unseen_faults.json"   # (tests/test_cond_stack_conformance.py)
    cs = json.loads(uc.read_text()) if uc.exists() else dict(faults=old.get("cond_stack_faults", 0), unseen=old.get("cond_stack_unseen_faults", {}))
    dst.write_text(json.dumps(dict(
        note="per stage: e_ref = rel-L2 of the bf16-boundary yardstick from fp64, device = rel-L2 of the product from fp64 (teacher forcing), "
             "ratio = device in units of the stage's bound / 2 (<= 2 passes); emu/ = lane emulator, gpu/ = MI355X.  unseen_faults: the faults of "
             "test_faults_are_seen that move their stage by less than 4 x e_ref (value = the multiple reached); cond_stack_*: the same for tests/test_cond_stack_conformance.py  (tests/test_schedule_conformance.py)",
        faults=faults["faults"], unseen_faults=faults["unseen"], cond_stack_faults=cs["faults"], cond_stack_unseen_faults=cs["unseen"],
        cases=cases), indent=0, sort_keys=True) + "\n")
    print(dst, len(cases), "cases;", len(faults["unseen"]), "of", faults["faults"], "faults unseen")
