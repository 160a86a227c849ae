"""Conformance of the head_dim-64 attention kernels (``pcdm_flash_attn``, ``pcdm_flash_attn_thr``, ``pcdm_flash_attn_fp8``; the shift-invariance
cases also on ``pcdm_attn_wide``) against an fp64 reference, with a derived per-element bound.

Reference.  ``o = softmax(q k^T scale) v`` in fp64 from the operands the kernel multiplies: the bf16 values for the bf16 kernels; for the fp8
kernel ``e4m3(k)``, ``e4m3(v)`` (the library's own ``pcdm_quantize_fp8``, cross-checked against torch's e4m3 cast) and
``e4m3(q * scale * log2e * 2^-e) * 2^e`` with the per-query power of two of the kernel's range guard (e = 0 unless the scaled row exceeds 448).

Bound, per output element.  u = 2^-8 (bf16 unit roundoff), p = the fp64 softmax, o = p v:

* the kernel rounds ``q * scale * log2e`` to bf16 once (relative u per element, so at most ``u * sum_i |q_i k_i| * scale`` per score) and
  subtracts a bf16 reference m inside the contraction (m is of the size of the scores; u of it at most): per query
  ``ds = 2u * max_k sum_i |q_i k_i| * scale``;
* a score error e_k with |e_k| <= ds changes the softmax to first order by ``p_k (e_k - sum_j p_j e_j)``, whose range over k is 2 ds, and
  ``sum_k p_k (e_k - e_bar)(v_k - o)`` is the change of o: at most ``2 ds * sum_k p_k |v_k - o|``;
* P is rounded to bf16 for the PV product while the row sum adds the un-rounded P (the default path; the MFMA row sum adds the rounded P,
  which is inside the same term): ``u * sum_k p_k |v_k|`` for the numerator and as much again for the fp32 accumulation of numerator and
  denominator over up to thousands of keys and the reciprocal: ``2u * sum_k p_k |v_k|``;
* the result is rounded to bf16: ``u |o|``.

``|out - o| <= 2 ds * sum_k p_k |v_k - o|  +  2u * sum_k p_k |v_k|  +  u |o|``.

fp8: the same form with e4m3's unit roundoff 2^-4 in place of u for the Q rounding (``ds = (2^-4 + u) * ...``: the subtracted reference stays
bf16) and for the P rounding (``2 * 2^-4 * sum_k p_k |v_k|``); the final rounding is bf16.  Always against the quantised-operand reference.
``pcdm_attn_wide`` multiplies the fp32 scores by the scale (no bf16 rounding of q): the bf16 bound holds for it with room.

Agreement of the thresholds.  The results at the three thresholds are also compared with each other.  The score error is common to them (the
same rounded q; any reference m gives the same mathematics), but each result carries its own P rounding (the reference differs, so the
mantissas of P do) and its own final rounding: ``|out_a - out_b| <= 2 * u sum_k p_k |v_k|  +  2 * u |o|``, which is the bound above plus one
more ``u |o|`` -- the second result's final rounding, the one term the single-result bound does not hold.  (Without it: measured on MI355X at
B 2, H 5, 5632 x 5632, operands x 3, a one-hot row with v = 164/512 came out as 163/512 at thr <= 12 and 165/512 at thr = 16 -- P of the leading
key rounds down by 2^-8 relative with one reference and up with the other, each result 0.52 of the bound from the fp64 value, 1.02 of it
from each other: two bf16 neighbours of the correctly rounded value.)

The tolerance bites (``test_tolerance_bites``): on short or peaky rows the same comparison against a reference with the tail key dropped,
with one zero key appended (what a missing tail mask computes) and -- bf16 kernel -- with the row sum taken from the bf16-rounded P and
scaled by 1 + 2^-6 must FAIL.  (The third does not apply to the fp8 kernel: its row sum IS the sum of the rounded P, and 2^-6 lies inside
the e4m3 term of its bound.)

Every output is a column window of a wider buffer filled with a bf16 NaN pattern, with guard rows in front and behind: nothing outside
``[B*Lq, H*64]`` may be written, and no element inside may be left.  q / k are column views of one fused buffer; ``ldvt`` takes the minimum,
the minimum + one unit and more than a key tile beyond ``64 ceil(Lk / 64)``.  On the GPU every accepted call runs twice, bit-identical, and
the largest err / bound per kernel family goes to the parity record.  ``PCDM_ATTN_ROWSUM=mfma`` and ``PCDM_ATTN_XCD=0`` are read when the
library is loaded: a reduced set runs in a fresh child process per switch (``python -m tests.test_attn_conformance``).
"""
from __future__ import annotations

import functools
import hashlib
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from pcdms_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
BF16 = torch.bfloat16
F64 = torch.float64
U = 2.0 ** -8                   # bf16 unit roundoff
U8 = 2.0 ** -4                  # e4m3 unit roundoff
LOG2E = 1.44269504088896341
SENT16 = 0x7FA5                 # a bf16 NaN pattern no kernel produces from finite operands
NEG = 88.7                      # exp(-88.7) ~ 2^-128: below it exp2 of the first-tile rescale overflowed
THRS = {"bf16": (None, 0.0, 16.0), "fp8": (5.0, 0.0, 8.0), "wide": (None,)}
FAMILY = {"bf16": "flash_attn", "fp8": "flash_attn_fp8", "wide": "attn_wide"}
WORST = {}                      # family -> largest err / bound seen in this process

LKS = (1, 2, 7, 8, 9, 31, 33, 63, 64, 65, 127, 128, 129, 191, 193, 258)
LQS = (1, 31, 32, 33, 127, 128, 129, 260)
# (B, H, Lq, Lk): every Lk once with a ragged last query block ...
RAGGED = ((1, 1, 1, 1), (1, 1, 31, 2), (2, 1, 32, 7), (1, 2, 33, 8), (1, 1, 127, 9), (1, 1, 129, 31), (3, 2, 260, 33), (1, 1, 33, 63),
          (1, 5, 33, 64), (2, 1, 31, 65), (1, 1, 129, 127), (1, 2, 1, 128), (1, 1, 33, 129), (1, 1, 127, 191), (3, 1, 32, 193), (1, 2, 260, 258))
# ... and once with full ones
FULL = tuple((2, 2, 256, lk) if lk == 64 else (1, 2, 128, lk) if lk in (9, 129) else (1, 1, 128, lk) for lk in LKS)
SHAPES = RAGGED + FULL
SHAPE_DISTS = ("diffuse", "hot3", "onehot_last", "qzero", "hot6")          # cycled over SHAPES (q = 0: a tail key let in is seen at any Lk)
DISTS = ("diffuse", "hot3", "hot6", "onehot_first", "onehot_mid", "onehot_last", "ties", "qzero", "rising", "falling", "neg1", "neg2", "neg4",
         "first_neg", "later_neg", "pos")
SHIFT_DISTS = ("neg1", "neg2", "neg4", "first_neg", "later_neg", "pos")   # also run on pcdm_attn_wide, d = 64 and 512
DIST_SHAPES = ((2, 1, 33, 193), (1, 1, 128, 192))                          # ragged (3 tiles + a tail key tile) / full (3 tiles)
# self- and cross-attention of every UNet level at the flagship workload (352 x 512 images on a 704 x 512 canvas: latent 64 x 88 -> 5632, 1408,
# 352 tokens, 88 in the middle; heads 5, 10, 20, 20; the context is 258 tokens): (H, Lq, Lk)
UNET_SHAPES = ((5, 5632, 5632), (10, 1408, 1408), (20, 352, 352), (20, 88, 88), (5, 5632, 258), (10, 1408, 258), (20, 352, 258), (20, 88, 258))


def _wgs(B, H, Lq):
    return B * H * ((Lq + 127) // 128)


def test_shape_list_covers_the_residues():
    assert {s[3] for s in RAGGED} == set(LKS) and {s[3] for s in FULL} == set(LKS)
    assert all(s[2] % 128 for s in RAGGED) and not any(s[2] % 128 for s in FULL)
    assert {s[2] for s in SHAPES} == set(LQS) | {256}
    assert {s[1] for s in SHAPES} == {1, 2, 5} and {s[0] for s in SHAPES} == {1, 2, 3}
    n = [_wgs(*s[:3]) for s in SHAPES]
    assert any(w > 8 and w % 8 for w in n) and any(w < 8 for w in n) and any(w % 8 == 0 for w in n)   # attn_block_coords: ragged, short, even


# ------------------------------------------------------------------------------------------------ case generator
def _block(dist: str, Lq: int, Lk: int, d: int, g: torch.Generator):
    """q [Lq, d], k [Lk, d], v [Lk, d] (fp64, before the bf16 rounding) of one (batch, head).  q1 is scaled so that a key a * q1 scores 32 a
    against it at scale d^-1/2, whatever d."""
    def rn(*s):
        return torch.randn(*s, generator=g, dtype=F64)
    q1 = rn(d)
    q1 = q1 * math.sqrt(32.0 * math.sqrt(d)) / q1.norm()
    v = rn(Lk, d)
    tile = (torch.arange(Lk) // 64).to(F64)[:, None]
    if dist == "diffuse":
        return rn(Lq, d), rn(Lk, d), v
    if dist in ("hot3", "hot6"):
        a = float(dist[3:])
        return a * rn(Lq, d), a * rn(Lk, d), v
    if dist.startswith("onehot"):                      # one key at 6 x the common direction of the queries: its score leads by ~48
        qa = q1 / 2
        k = rn(Lk, d)
        k[{"first": 0, "mid": Lk // 2, "last": Lk - 1}[dist[7:]]] = 6 * qa
        return qa + 0.1 * rn(Lq, d), k, v
    if dist == "ties":                                 # all keys equal: out = mean of V
        return rn(Lq, d), rn(1, d).repeat(Lk, 1), v
    if dist == "qzero":
        return torch.zeros(Lq, d, dtype=F64), rn(Lk, d), v
    if dist in ("rising", "falling"):                  # the tile maximum moves by 12 (17.3 in log2 units > the largest thr) every tile
        sgn = 1.0 if dist == "rising" else -1.0
        return q1 + 0.05 * rn(Lq, d), sgn * 0.375 * tile * q1 + 0.3 * rn(Lk, d), v
    q = q1 + 0.02 * rn(Lq, d)
    k = 0.3 * rn(Lk, d)
    if dist.startswith("neg"):                         # every score near -96 m
        k = k - 3.0 * float(dist[3:]) * q1
    elif dist == "first_neg":                          # the first key tile near -96, the rest ordinary
        k[:64] -= 3.0 * q1
    elif dist == "later_neg":
        k[64:] -= 3.0 * q1
    elif dist == "pos":
        k = k + 3.0 * q1
    else:
        raise ValueError(dist)
    return q, k, v


def _check_ranges(dist, q, k, d):
    """the score ranges the distribution's name promises (of the bf16 operands)"""
    s = q.double() @ k.double().t() / math.sqrt(d)
    if dist.startswith("neg"):
        assert s.max().item() < -NEG * float(dist[3:]), (dist, s.max().item())
    if dist == "first_neg" and k.shape[0] > 64:
        assert s[:, :64].max().item() < -NEG and s[:, 64:].min().item() > -20, dist
    if dist == "later_neg" and k.shape[0] > 64:
        assert s[:, 64:].max().item() < -NEG and s[:, :64].min().item() > -20, dist
    if dist == "pos":
        assert s.min().item() > NEG, (dist, s.min().item())


@functools.lru_cache(maxsize=4)
def make_case(dist: str, B: int, H: int, Lq: int, Lk: int, d: int = 64, seed: int = 0):
    """bf16 q [B*Lq, H*d], k [B*Lk, H*d], v [B*Lk, H*d] on the CPU"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * Lq + 13 * Lk + B + 3 * H + d)
    q = torch.empty(B, Lq, H, d, dtype=BF16)
    k = torch.empty(B, Lk, H, d, dtype=BF16)
    v = torch.empty(B, Lk, H, d, dtype=BF16)
    for b in range(B):
        for h in range(H):
            qb, kb, vb = _block(dist, Lq, Lk, d, g)
            q[b, :, h], k[b, :, h], v[b, :, h] = qb.to(BF16), kb.to(BF16), vb.to(BF16)
            if b == 0 and h == 0:
                _check_ranges(dist, q[b, :, h], k[b, :, h], d)
    return q.view(B * Lq, H * d), k.view(B * Lk, H * d), v.view(B * Lk, H * d)


# ------------------------------------------------------------------------------------------------ fp64 reference and bound
def _e4m3(x: torch.Tensor) -> torch.Tensor:
    """OCP e4m3fn round trip (RNE, saturating): torch's own cast, the test's quantiser"""
    return x.float().clamp(-448, 448).to(torch.float8_e4m3fn).float()


def fp8_operands(q, k, v, H, scale):
    """the operands as flash_attn_fp8_kernel multiplies them, q in score units (so that s = q k scale as for the bf16 kernel)"""
    c = (torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    qs = (q.float() * c).view(q.shape[0], H, 64)
    amax = qs.abs().amax(-1, keepdim=True)
    e = torch.where(amax > 448, torch.ceil(torch.log2(amax / 448)), torch.zeros_like(amax))
    qq = (_e4m3(qs * 2.0 ** -e).double() * 2.0 ** e.double()).view(q.shape[0], -1) / c.double()
    return qq, _e4m3(k).double(), _e4m3(v).double()


class Ref:
    """fp64 attention of [rows, H*d] operands and the per-element bound of the module docstring; everything [B, H, Lq, .] inside"""

    def __init__(self, q, k, v, B, H, Lq, Lk, d, scale, uq=U, up=U, dev="cpu"):
        self.dims = (B, H, Lq, Lk, d)
        qh = q.to(dev).double().view(B, Lq, H, d).transpose(1, 2)
        kh = k.to(dev).double().view(B, Lk, H, d).transpose(1, 2)
        self.vh = v.to(dev).double().view(B, Lk, H, d).transpose(1, 2)
        self.s = qh @ kh.transpose(-1, -2) * scale
        ds = (uq + U) * (qh.abs() @ kh.abs().transpose(-1, -2)).amax(-1, keepdim=True) * scale
        p = torch.softmax(self.s, -1)
        self.o = p @ self.vh
        spread = torch.empty_like(self.o)
        for i in range(d):                       # sum_k p_k |v_k - o|, one head dim at a time (no [Lq, Lk, d] temporary)
            spread[..., i] = (p * (self.vh[..., None, :, i] - self.o[..., :, None, i]).abs()).sum(-1)
        self.bound = 2 * ds * spread + 2 * up * (p @ self.vh.abs()) + U * self.o.abs()
        del p, spread

    def flat(self, t):
        B, H, Lq, Lk, d = self.dims
        return t.transpose(1, 2).reshape(B * Lq, H * d).cpu()

    def ratio(self, got: torch.Tensor, against=None) -> float:
        """max of |got - ref| / bound over the elements (inf for a non-finite output)"""
        ref = self.flat(self.o if against is None else against)
        bound = self.flat(self.bound)
        if not bool(torch.isfinite(got).all()):
            return float("inf")
        err = (got - ref).abs()
        return torch.where(err == 0, torch.zeros_like(err), err / bound).max().item()

    # ---- deliberately wrong references
    def drop_tail(self):
        return torch.softmax(self.s[..., :-1], -1) @ self.vh[..., :-1, :]

    def zero_key(self):
        s = torch.cat([self.s, torch.zeros_like(self.s[..., :1])], -1)
        return torch.softmax(s, -1)[..., :-1] @ self.vh

    def rowsum_rounded(self):
        P = torch.exp(self.s - self.s.amax(-1, keepdim=True))
        Pr = P.float().to(BF16).double()
        return (Pr @ self.vh) / (Pr.sum(-1, keepdim=True) * (1 + 2.0 ** -6))


def make_ref(kind, q, k, v, B, H, Lq, Lk, d, scale, dev="cpu") -> Ref:
    if kind == "fp8":
        return Ref(*fp8_operands(q, k, v, H, scale), B, H, Lq, Lk, d, scale, uq=U8, up=U8, dev=dev)
    return Ref(q, k, v, B, H, Lq, Lk, d, scale, dev=dev)


# ------------------------------------------------------------------------------------------------ launching into sentinel-guarded windows
def _sent(n: int, dev) -> torch.Tensor:
    return torch.full((n,), SENT16, dtype=torch.int16, device=dev).view(BF16)


def ldvt_for(kind: str, Lk: int, mode: int) -> int:
    """0: the minimum; 1: one unit more; 2: more than a key tile beyond 64 ceil(Lk / 64)"""
    unit = 16 if kind == "fp8" else 8
    lo = (Lk + unit - 1) // unit * unit
    return (lo, lo + unit, (Lk + 63) // 64 * 64 + 64 + unit)[mode]


class Launch:
    """The device buffers of one attention problem: q | k column views of one fused buffer, V^T with a chosen pitch and padding, the output
    a column window of a sentinel-filled buffer with a guard row in front and behind."""

    def __init__(self, kind, q, k, v, B, H, Lq, Lk, dev, d=64, ldvt_mode=0, pad=None, scale=None):
        self.kind, self.dev, self.B, self.H, self.Lq, self.Lk, self.d = kind, dev, B, H, Lq, Lk, d
        self.scale = scale if scale is not None else d ** -0.5
        Cc = H * d
        self.Cc = Cc
        qk = torch.zeros(B * max(Lq, Lk), 2 * Cc, dtype=BF16)
        qk[: B * Lq, :Cc] = q
        qk[: B * Lk, Cc:] = k
        self.qk = qk.to(dev)
        self.q, self.k = self.qk[: B * Lq, :Cc], self.qk[: B * Lk, Cc:]
        self.ldvt = ldvt_for(kind, Lk, ldvt_mode)
        vt_src = torch.empty(B, Cc, Lk, dtype=BF16)                          # (fresh strides: a size-1 dimension keeps the permuted ones)
        vt_src.copy_(v.view(B, Lk, Cc).permute(0, 2, 1))
        if kind == "fp8":
            self.k8 = torch.empty(B * Lk, Cc, dtype=torch.uint8, device=dev)
            ops.quantize_fp8(self.k, self.k8)
            self.vt8 = torch.full((B * Cc, self.ldvt), 0x7f, dtype=torch.uint8, device=dev)
            ops.quantize_fp8(vt_src.view(B * Cc, Lk).to(dev), self.vt8, cols=Lk)   # writes the padding as zero
            if dev.type == "cuda":
                torch.cuda.synchronize()
            assert torch.equal(self.k8.cpu().view(torch.float8_e4m3fn).float(), _e4m3(k)), "pcdm_quantize_fp8 differs from the e4m3 cast (K)"
            v8 = self.vt8.cpu()
            assert torch.equal(v8.view(torch.float8_e4m3fn).float()[:, :Lk], _e4m3(vt_src.view(B * Cc, Lk))) and bool((v8[:, Lk:] == 0).all())
            if pad is not None:
                self.vt8[:, Lk:] = pad
        else:
            fill = pad if pad is not None else (float("nan") if kind == "wide" else 0.0)   # wide: the padding is never used
            vt = torch.full((B, Cc, self.ldvt), fill, dtype=BF16)
            vt[:, :, :Lk] = vt_src
            self.vt = vt.to(dev)
        self.ldo = Cc + 16
        self.rows = B * Lq
        self.obuf = _sent((self.rows + 2) * self.ldo + 16, dev)
        self.optr = self.obuf.data_ptr() + 2 * (self.ldo + 8)

    def reset(self):
        self.obuf.view(torch.int16).fill_(SENT16)

    def __call__(self, thr=None, **over) -> int:
        """one call; ``over`` replaces single arguments (the refusal tests)"""
        L = _lib.lib()
        s = None if self.dev.type == "cpu" else torch.cuda.current_stream().cuda_stream
        a = dict(q=self.q.data_ptr(), ldq=self.q.stride(0), k=self.k.data_ptr(), ldk=self.k.stride(0), ldvt=self.ldvt, o=self.optr, ldo=self.ldo,
                 B=self.B, H=self.H, Lq=self.Lq, Lk=self.Lk, scale=self.scale)
        if self.kind == "fp8":
            a.update(k=self.k8.data_ptr(), ldk=self.k8.stride(0), vt=self.vt8.data_ptr(), thr=5.0 if thr is None else thr, kd=1.0, vd=1.0)
            a.update(over)
            return L.pcdm_flash_attn_fp8(a["q"], a["ldq"], a["k"], a["ldk"], a["vt"], a["ldvt"], a["o"], a["ldo"], a["B"], a["H"], a["Lq"], a["Lk"],
                                         a["scale"], a["kd"], a["vd"], a["thr"], s)
        a.update(vt=self.vt.data_ptr(), thr=thr)
        a.update(over)
        if self.kind == "wide":
            return L.pcdm_attn_wide(a["q"], a["ldq"], a["k"], a["ldk"], a["vt"], a["ldvt"], a["o"], a["ldo"], a["B"], a["Lq"], a["Lk"], self.d,
                                    a["scale"], s)
        if a["thr"] is None:
            return L.pcdm_flash_attn(a["q"], a["ldq"], a["k"], a["ldk"], a["vt"], a["ldvt"], a["o"], a["ldo"], a["B"], a["H"], a["Lq"], a["Lk"],
                                     a["scale"], s)
        return L.pcdm_flash_attn_thr(a["q"], a["ldq"], a["k"], a["ldk"], a["vt"], a["ldvt"], a["o"], a["ldo"], a["B"], a["H"], a["Lq"], a["Lk"],
                                     a["scale"], float(a["thr"]), s)

    def sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()

    def untouched(self) -> bool:
        self.sync()
        return bool((self.obuf.view(torch.int16) == SENT16).all())

    def result(self):
        """(the window as fp64 [B*Lq, Cc] on the CPU, number of elements written outside it, number of window elements left unwritten)"""
        self.sync()
        o = self.obuf.cpu()
        body = o[: (self.rows + 2) * self.ldo].view(self.rows + 2, self.ldo)
        win = body[1: self.rows + 1, 8: 8 + self.Cc]
        mask = torch.ones_like(body, dtype=torch.bool)
        mask[1: self.rows + 1, 8: 8 + self.Cc] = False
        outside = int((body[mask].view(torch.int16) != SENT16).sum()) + int((o[(self.rows + 2) * self.ldo:].view(torch.int16) != SENT16).sum())
        left = int((win.contiguous().view(torch.int16) == SENT16).sum())
        return win.double(), outside, left


def run_case(backend, kind, dist, B, H, Lq, Lk, d=64, ldvt_mode=0, thrs=None, seed=0, fails=None, want_out=False):
    """One problem on one kernel at every threshold: the output window against the fp64 reference within the bound, nothing written outside,
    the thresholds agreeing with each other within the bound + u |o| (two final roundings), bit-identical reruns on the GPU.  Returns the largest err / bound."""
    q, k, v = make_case(dist, B, H, Lq, Lk, d, seed)
    dev = backend.device
    L = Launch(kind, q, k, v, B, H, Lq, Lk, dev, d=d, ldvt_mode=ldvt_mode)
    ref = make_ref(kind, q, k, v, B, H, Lq, Lk, d, L.scale, dev=dev)
    where = f"{backend.name} {kind} {dist} B{B} H{H} Lq{Lq} Lk{Lk} d{d} ldvt{L.ldvt}"
    own = [] if fails is None else fails
    outs, worst = [], 0.0
    for thr in (thrs or THRS[kind]):
        L.reset()
        rc = L(thr)
        if rc != 0:
            own.append(f"{where} thr {thr}: rc {rc}")
            continue
        got, outside, left = L.result()
        if not backend.is_emu:                   # run again: bit-identical (a race shows up as a difference)
            first = L.obuf.clone()
            assert L(thr) == 0
            L.sync()
            if not torch.equal(first.view(torch.int16), L.obuf.view(torch.int16)):
                own.append(f"{where} thr {thr}: two runs differ")
        if outside or left:
            own.append(f"{where} thr {thr}: {outside} elements written outside the window, {left} inside left unwritten")
        r = ref.ratio(got)
        worst = max(worst, r)
        if not r <= 1.0:
            own.append(f"{where} thr {thr}: err / bound = {r:.3g}" + ("" if math.isfinite(r) else f" ({int((~torch.isfinite(got)).sum())} non-finite)"))
        else:
            outs.append((thr, got))
    bound = ref.flat(ref.bound) + U * ref.flat(ref.o).abs()      # two results: the final bf16 rounding enters twice (module docstring)
    for i in range(len(outs)):
        for j in range(i + 1, len(outs)):
            dif = (outs[i][1] - outs[j][1]).abs()
            if not bool((dif <= bound).all()):
                own.append(f"{where}: thr {outs[i][0]} and {outs[j][0]} differ by {(dif / bound).nan_to_num(0).max().item():.3g} x the pair bound")
    fam = FAMILY[kind]
    WORST[fam] = max(WORST.get(fam, 0.0), worst if math.isfinite(worst) else 1e30)
    if fails is None:
        assert not own, "\n".join(own)
    return (worst, outs, ref) if want_out else worst


def _record(backend):
    """GPU: the largest err / bound per kernel family so far, to the parity record (asserted <= 1)"""
    if backend.is_emu:
        return
    from tests import parity_record
    for fam, w in WORST.items():
        parity_record.check(f"attn_conformance_{fam}_err_over_bound", w, 1.0)


def _finish(backend, fails):
    try:
        _record(backend)
    except AssertionError as e:
        fails.append(str(e))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ shapes and distributions
GROUPS = 8


@pytest.mark.parametrize("group", range(GROUPS))
def test_shapes(backend, group):
    """every Lk residue with a ragged and with a full last query block, the Lq / H / B values and the grid kinds of the issue's list"""
    fails = []
    for i in range(group, len(SHAPES), GROUPS):
        B, H, Lq, Lk = SHAPES[i]
        for kind in ("bf16", "fp8"):
            run_case(backend, kind, SHAPE_DISTS[i % len(SHAPE_DISTS)], B, H, Lq, Lk, ldvt_mode=i % 3, fails=fails)
    _finish(backend, fails)


@pytest.mark.parametrize("dist", DISTS)
def test_distributions(backend, dist):
    """every score distribution on a ragged and a full shape, every threshold; the shift-invariance cases on pcdm_attn_wide too"""
    fails = []
    for i, (B, H, Lq, Lk) in enumerate(DIST_SHAPES):
        for kind in ("bf16", "fp8"):
            run_case(backend, kind, dist, B, H, Lq, Lk, ldvt_mode=(i + DISTS.index(dist)) % 3, fails=fails)
    if dist in SHIFT_DISTS:
        for d in (64, 512):
            run_case(backend, "wide", dist, 2, 1, 33, 193, d=d, ldvt_mode=1, fails=fails)
    _finish(backend, fails)


@pytest.mark.parametrize("dist", ("ties", "qzero"))
def test_ties_give_the_mean_of_v(dist):
    """the reference of the tie cases is what the issue says it is (so the cases above check out = mean of V)"""
    B, H, Lq, Lk = DIST_SHAPES[0]
    q, k, v = make_case(dist, B, H, Lq, Lk)
    ref = Ref(q, k, v, B, H, Lq, Lk, 64, 0.125)
    mean = v.double().view(B, Lk, H * 64).mean(1, keepdim=True).expand(B, Lq, H * 64).reshape(B * Lq, H * 64)
    assert (ref.flat(ref.o) - mean).abs().max().item() < 1e-12


def test_single_key_is_v(backend):
    """Lk = 1: out = v, within the last two terms of the bound (the first vanishes: v_k - o = 0)"""
    B, H, Lq, Lk = 2, 2, 33, 1
    for kind in ("bf16", "fp8"):
        w, outs, ref = run_case(backend, kind, "hot3", B, H, Lq, Lk, want_out=True)
        vq = make_case("hot3", B, H, Lq, Lk)[2]
        vq = (_e4m3(vq) if kind == "fp8" else vq).double().view(B, 1, H * 64).expand(B, Lq, H * 64).reshape(B * Lq, H * 64)
        up = U8 if kind == "fp8" else U
        for thr, got in outs:
            assert bool(((got - vq).abs() <= (2 * up + U) * vq.abs()).all()), (kind, thr)
    _record(backend)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(UNET_SHAPES)))
def test_unet_shapes(gpu_backend, idx):
    """the UNet's own attention shapes (352 x 512 workload, 258 context tokens), two images, diffuse and hot operands."""
    H, Lq, Lk = UNET_SHAPES[idx]
    fails = []
    for kind in ("bf16", "fp8"):
        for dist in ("diffuse", "hot3"):
            run_case(gpu_backend, kind, dist, 2, H, Lq, Lk, ldvt_mode=idx % 3, fails=fails)
            make_case.cache_clear()
    _finish(gpu_backend, fails)


# ------------------------------------------------------------------------------------------------ the tolerance bites
BITE_SHAPES = ((1, 1, 33, 9), (1, 2, 128, 64), (2, 1, 33, 129), (1, 1, 128, 192), (1, 1, 33, 193), (1, 1, 129, 258))


def _bite_inputs(what: str, B, H, Lq, Lk):
    """short or peaky rows on which the wrong reference is far from the right one"""
    if what == "zero_key":        # one key near -2, the others near -48: an appended key of score 0 would take 7/8 of the weight of a peaky row
        g = torch.Generator().manual_seed(Lk)
        q1 = torch.randn(64, generator=g, dtype=F64)
        q1 = q1 * 16.0 / q1.norm()
        q = (q1 + 0.02 * torch.randn(Lq, 64, generator=g, dtype=F64)).to(BF16).repeat(B, H)
        k = -1.5 * q1 + 0.3 * torch.randn(Lk, 64, generator=g, dtype=F64)
        k[Lk // 2] = -0.0625 * q1
        return q, k.to(BF16).repeat(B, H), make_case("diffuse", B, H, Lq, Lk)[2]
    return make_case("onehot_last", B, H, Lq, Lk)     # the tail key carries the row; P = 1 exactly, so only the scaled row sum moves o


@pytest.mark.parametrize("shape", BITE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tolerance_bites(backend, shape):
    """The comparison that passes against the right reference fails against each wrong one (module docstring)."""
    B, H, Lq, Lk = shape
    dev = backend.device
    for kind in ("bf16", "fp8"):
        for what in ("drop_tail", "zero_key") + (("rowsum_rounded",) if kind == "bf16" else ()):
            q, k, v = _bite_inputs(what, B, H, Lq, Lk)
            L = Launch(kind, q, k, v, B, H, Lq, Lk, dev)
            ref = make_ref(kind, q, k, v, B, H, Lq, Lk, 64, L.scale, dev=dev)
            assert L(None) == 0
            got, outside, left = L.result()
            assert outside == 0 and left == 0
            r = ref.ratio(got)
            assert r <= 1.0, f"{kind} {what} {shape}: err / bound = {r:.3g} against the right reference"
            rw = ref.ratio(got, against=getattr(ref, what)())
            assert rw > 1.0, f"{kind} {what} {shape}: the tolerance does not see the wrong reference (err / bound = {rw:.3g})"


# ------------------------------------------------------------------------------------------------ V^T padding contract
@pytest.mark.parametrize("Lk", (1, 9, 60, 70, 129))
def test_vt_padding_contract(backend, Lk):
    """include/pcdm.h: the columns [Lk, ldvt) of V^T are multiplied by an exact zero -- any finite value there gives the bits zero padding
    gives (bf16: 3e38 and a finite sentinel; fp8: the largest e4m3 value and a sentinel byte)."""
    B, H, Lq = 2, 1, 33
    q, k, v = make_case("diffuse", B, H, Lq, Lk)
    for kind, pads in (("bf16", (0.0, 3e38, -1234.0)), ("fp8", (0, 0x7e, 0xa5))):
        for mode in (1, 2):
            outs = []
            for pad in pads:
                L = Launch(kind, q, k, v, B, H, Lq, Lk, backend.device, ldvt_mode=mode, pad=pad)
                assert L(None) == 0
                got, outside, left = L.result()
                assert outside == 0 and left == 0 and bool(torch.isfinite(got).all()), (kind, mode, pad)
                outs.append(got)
            assert all(torch.equal(outs[0], o) for o in outs[1:]), f"{kind} Lk {Lk} ldvt mode {mode}: the padding value reaches the output"


# ------------------------------------------------------------------------------------------------ refusals
def _refusals(kind: str, L: Launch, emu: bool):
    """(what, overrides, expected rc) for every rule of include/pcdm.h"""
    big = 1 << 30
    r = [(f"{n} NULL", {n: None}, -1) for n in ("q", "k", "vt", "o")]
    r += [(f"{n} = {val}", {n: val}, -1) for n in ("B", "H", "Lq", "Lk") for val in (0, -1)]
    if kind == "bf16":
        ld = dict(ldq=L.q.stride(0), ldk=L.k.stride(0), ldvt=L.ldvt, ldo=L.ldo)
        r += [(f"{n} + 4", {n: ld[n] + 4}, -1) for n in ld]
        r += [(f"{n} + 8 bytes", {n: {"q": L.q.data_ptr(), "k": L.k.data_ptr(), "vt": L.vt.data_ptr(), "o": L.optr}[n] + 8}, -1)
              for n in ("q", "k", "vt", "o")]
        r += [("thr < 0", dict(thr=-0.5), -1), ("thr > 16", dict(thr=16.5), -1), ("thr NaN", dict(thr=float("nan")), -1)]
        r += [("Lk ldk = 2^30", dict(Lk=1, ldk=big), -2)]          # (Lk = 1: were it launched, only key row 0 would be read)
        if emu:                                                     # (were it launched, 2 GiB beyond the buffer would be read: host logic only)
            r += [("64 ldvt = 2^30", dict(ldvt=big // 64), -2)]
    else:
        r += [("ldq + 4", dict(ldq=L.q.stride(0) + 4), -1), ("ldk + 8", dict(ldk=L.k8.stride(0) + 8), -1), ("ldvt + 8", dict(ldvt=L.ldvt + 8), -1),
              ("ldo + 2", dict(ldo=L.ldo + 2), -1)]
        r += [(f"{n} + 8 bytes", {n: {"q": L.q.data_ptr(), "k": L.k8.data_ptr(), "vt": L.vt8.data_ptr()}[n] + 8}, -1) for n in ("q", "k", "vt")]
        r += [("o + 4 bytes", dict(o=L.optr + 4), -1)]
        r += [("thr < 0", dict(thr=-0.5), -1), ("thr > 8", dict(thr=8.5), -1), ("thr NaN", dict(thr=float("nan")), -1)]
        r += [(f"{n} = {val}", {n: val}, -1) for n in ("kd", "vd") for val in (0.0, -1.0, float("nan"))]
        r += [("Lk ldk = 2^31", dict(Lk=1, ldk=2 * big), -2)]
        if emu:
            r += [("64 ldvt = 2^31", dict(ldvt=2 * big // 64), -2)]
    r += [("ldvt < Lk", dict(ldvt=L.Lk // 16 * 16), -1)]
    return r


def test_refusals(backend):
    """every refusal rule of include/pcdm.h for the three entry points: the stated return code, and the output untouched"""
    B, H, Lq, Lk = 2, 1, 40, 70
    q, k, v = make_case("diffuse", B, H, Lq, Lk)
    fails = []
    for kind in ("bf16", "fp8"):
        L = Launch(kind, q, k, v, B, H, Lq, Lk, backend.device)
        for entry_thr in ((None, 8.0) if kind == "bf16" else (5.0,)):     # pcdm_flash_attn and pcdm_flash_attn_thr
            for what, over, want in _refusals(kind, L, backend.is_emu):
                if entry_thr is None and "thr" in over:
                    continue
                L.reset()
                rc = L(**{"thr": entry_thr, **over})
                if rc != want or not L.untouched():
                    fails.append(f"{kind} thr {entry_thr} {what}: rc {rc}, expected {want}; output {'untouched' if L.untouched() else 'WRITTEN'}")
        # the boundary values are accepted
        for thr in ((0.0, 16.0) if kind == "bf16" else (0.0, 8.0)):
            L.reset()
            if L(thr) != 0:
                fails.append(f"{kind}: thr {thr} refused")
        L.sync()
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ the load-time switches, in a child process
REDUCED_SHAPES = ((1, 1, 33, 9), (3, 2, 260, 33), (2, 2, 256, 64), (2, 1, 31, 65), (1, 1, 128, 128), (1, 1, 33, 129), (1, 2, 260, 258))
DIGEST_CASE = ("diffuse", 3, 2, 260, 33)


def _digest(backend) -> str:
    """the bits of the bf16 kernel's default-threshold output on one case (18 workgroups: a non-trivial XCD placement)"""
    dist, B, H, Lq, Lk = DIGEST_CASE
    q, k, v = make_case(dist, B, H, Lq, Lk)
    L = Launch("bf16", q, k, v, B, H, Lq, Lk, backend.device)
    assert L(None) == 0
    L.sync()
    return hashlib.sha256(L.obuf.cpu().view(torch.int16).numpy().tobytes()).hexdigest()


def _child_main(which: str) -> int:
    """``python -m tests.test_attn_conformance emu|gpu``: one case per shape class and per distribution, in this (fresh) process"""
    from tests.conftest import Backend
    if which == "emu":
        from tests.emu import build_emu
        _lib.use_library(build_emu.load())
        backend = Backend("emu", torch.device("cpu"))
    else:
        _lib.load()
        assert torch.cuda.is_available() and not _lib.is_emulator()
        backend = Backend("gpu", torch.device("cuda:0"))
    fails = []
    for i, (B, H, Lq, Lk) in enumerate(REDUCED_SHAPES):
        for kind in ("bf16", "fp8"):
            run_case(backend, kind, "diffuse", B, H, Lq, Lk, ldvt_mode=i % 3, fails=fails)
    for i, dist in enumerate(DISTS):
        B, H, Lq, Lk = DIST_SHAPES[0]
        for kind in ("bf16", "fp8"):
            run_case(backend, kind, dist, B, H, Lq, Lk, ldvt_mode=i % 3, thrs=THRS[kind][:2], fails=fails)
    print("\n".join(fails))
    print("WORST " + " ".join(f"{k}={v:.4g}" for k, v in sorted(WORST.items())))
    print("DIGEST " + _digest(backend), flush=True)
    return 1 if fails else 0


@pytest.mark.parametrize("switch", ("PCDM_ATTN_ROWSUM=mfma", "PCDM_ATTN_XCD=0"))
def test_load_time_switches(backend, switch):
    """The MFMA row sum and the plain grid are selected when the library is loaded: a reduced set in a fresh child process per switch (started
    once, under a timeout; its non-zero exit is the failure).  The switch must have taken: the plain grid gives the default's bits (placement
    only), the MFMA row sum (rounded P) does not."""
    env = {k: v for k, v in os.environ.items() if k not in ("PCDM_ATTN_ROWSUM", "PCDM_ATTN_XCD")}
    name, val = switch.split("=")
    env[name] = val
    p = subprocess.run([sys.executable, "-m", "tests.test_attn_conformance", backend.name], cwd=str(ROOT), env=env, timeout=900,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, f"{switch}: child exit {p.returncode}\n{p.stdout[-4000:]}"
    lines = p.stdout.splitlines()
    digest = [ln.split()[1] for ln in lines if ln.startswith("DIGEST ")]
    assert len(digest) == 1, p.stdout[-2000:]
    if not backend.is_emu:
        from tests import parity_record
        for item in next(ln for ln in lines if ln.startswith("WORST ")).split()[1:]:
            fam, w = item.split("=")
            parity_record.check(f"attn_conformance_{fam}_{name.lower()}_err_over_bound", float(w), 1.0)
    if "PCDM_ATTN_ROWSUM" in os.environ or "PCDM_ATTN_XCD" in os.environ:
        return                                   # (this process does not run the defaults: nothing to compare the bits with)
    mine = _digest(backend)
    if name == "PCDM_ATTN_XCD":
        assert digest[0] == mine, "PCDM_ATTN_XCD=0 changed the result"
    else:
        assert digest[0] != mine, "PCDM_ATTN_ROWSUM=mfma gave the bits of the VALU row sum: the switch was not read"


if __name__ == "__main__":
    sys.exit(_child_main(sys.argv[1] if len(sys.argv) > 1 else "emu"))
