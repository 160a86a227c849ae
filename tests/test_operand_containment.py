"""Operand containment: no kernel READS outside the tensors it is given (the conformance suites judge values, tests/test_workspace_containment.py
judges where the library writes and what it reads of fresh memory).

The GEMM, rowgemm and attention kernels address their operands through buffer descriptors of 2^31 - 1 bytes: only per-lane predicates keep
them inside; rows ``[N, Npad)`` of W and the V^T padding of a key tile are read by design; callers size slack by hand where an activation slice
stands in as W; vector bodies have scalar tails.  A read past a tensor is invisible on the GPU until the tensor happens to end where a mapping
ends.  Three instruments:

* GUARD PAGES (CPU, lane emulator, child processes).  ``CASES`` holds one entry per entry point that takes a device pointer: the smallest shapes
  that take each tail path, every pointer operand -- outputs included -- at exactly the extent include/pcdm.h documents (for an operand with a row
  stride: ``(rows - 1) ld + cols`` elements), in memory that ends (side "end") or starts (side "start") at a ``PROT_NONE`` page
  (tests/guarded.py).  One byte read or written beyond an operand kills the child with SIGSEGV; the parent names the case, prints the child's
  Python stack, and restarts the child behind that case.  SCHEDULES run whole tiny models with every weight, input and ``torch.empty`` /
  ``torch.zeros`` buffer guarded at its end: that checks the slack the callers count by hand.
* FILLS (GPU, product library; ``-m gpu``).  The same cases with every operand at its exact extent inside a larger device buffer that has 4 KiB
  in front of it and 4 KiB behind it, holding 0x00, 0xFF and the finite pattern 0x3C in turn: the outputs must be bit-identical.  Everything
  read is mapped memory, so this half is safe by construction -- but it sees ONLY over-reads that reach a result (0 x NaN, a maximum, a sum): a
  value that is loaded and then masked goes unseen.  Code under ``#ifndef PCDM_EMU`` (the GroupNorm cluster kernel, the product build's
  intrinsics) is seen by this half alone.
* WRAPPER EXTENTS (host).  A recording stub in place of the library (nothing can launch): every ``ops.*`` wrapper must raise before the stub
  is called when an operand is one element short, of the wrong dtype, or non-contiguous.

The last section shows that each instrument bites.  Per case, profiles/operand_containment_values.json records the guarded operands, the
largest alignment gap (<= 15 bytes) and the child's wall time: recorded, not gated."""
from __future__ import annotations

import ctypes as C
import fcntl
import json
import math
import os
import re
import subprocess
import sys
import tempfile
import time
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from pcdms_amd import _lib, ops
from pcdms_amd._lib import GemmParams
from tests import guarded as G

ROOT = Path(__file__).resolve().parent.parent
VALUES = ROOT / "profiles" / "operand_containment_values.json"
BF16, F32, U8, I32, I64, F64 = torch.bfloat16, torch.float32, torch.uint8, torch.int32, torch.int64, torch.float64
CASES: dict = {}


def case(family: str, *exports: str, sides=("end", "start")):
    """register ``fn(P) -> outputs`` (``P``: a ``guarded.Place``) under its name without the ``case_`` prefix"""
    def deco(fn):
        name = fn.__name__[len("case_"):]
        assert name not in CASES
        CASES[name] = SimpleNamespace(family=family, exports=exports, fn=fn, sides=sides)
        return fn
    return deco


def rn(seed: int, *shape, dtype=F32, scale: float = 1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def ru8(seed: int, *shape):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int32).to(U8)


Z = G._ORIG["zeros"]                                        # torch's own ``zeros``: host-side preparation inside a case is not an allocation of the library's


def lib():
    return _lib.lib()


def ptr(t):
    return None if t is None else t.data_ptr()


def stream(P):
    return torch.cuda.current_stream(P.device).cuda_stream if P.device.type == "cuda" else None


def ok(rc, what=""):
    assert rc == 0, f"the library refused the case ({rc}) {what}"


def run_guarded(name: str, side: str):
    """one case on guard pages (the child process) -> (operands guarded, allocations guarded, largest alignment gap)"""
    P = G.GuardedPlace(side)
    with G.GuardedAllocs(P) as al:
        CASES[name].fn(P)
    assert P.count > 0, f"{name}: no operand was guarded: the case tests nothing"
    assert al.count > 0 or not CASES[name].family.startswith("schedules_"), f"{name}: the allocation patch intercepted nothing"
    assert P.max_gap <= 15, (name, P.max_gap)
    return P.count, al.count, P.max_gap


# ================================================================================================ the table: norms
@case("norms", "pcdm_layernorm")
def case_layernorm(P):
    out = []
    for Cn in (72, 320, 1000):            # the generic kernel with a tail, the register-resident instance, the generic kernel over several trips
        y = P.out((3, Cn), BF16)
        ops.layernorm(P(rn(Cn, 3, Cn, dtype=BF16)), P(rn(1, Cn)), P(rn(2, Cn)), 1e-5, y)
        out.append(y)
    return out


def _gn_ws(P, B, Cn):
    return P(Z(lib().pcdm_groupnorm_ws_floats(B, Cn), dtype=F32))


def _groupnorm(P, B, HW, C1, C2, groups, silu=True):
    Cn = C1 + C2
    y = P.out((B * HW, Cn), BF16)
    x2 = P(rn(4, B * HW, C2, dtype=BF16)) if C2 else None
    ops.groupnorm(P(rn(3, B * HW, C1, dtype=BF16)), x2, B, HW, groups, 1e-5, P(rn(5, Cn)), P(rn(6, Cn)), silu, y, _gn_ws(P, B, Cn))
    return y


@case("norms", "pcdm_groupnorm", "pcdm_groupnorm_ws_floats", "pcdm_groupnorm_cluster_timeouts")
def case_groupnorm(P):
    # 64 ch x 5, 96 ch x 7 (group size 3: the two-kernel path), the concat 64 + 96, 32 + 32 at HW 1
    out = [_groupnorm(P, 2, 5, 64, 0, 32), _groupnorm(P, 1, 7, 96, 0, 32), _groupnorm(P, 2, 7, 64, 96, 32), _groupnorm(P, 3, 1, 32, 32, 8)]
    assert ops.groupnorm_cluster_timeouts(_gn_ws(P, 2, 64)) == 0
    return out


@case("norms", "pcdm_groupnorm")
def case_groupnorm_paths(P):
    # the single-pass kernel at 256 / 512 / 1024 threads (64 octets per row: HW <= 32 / 64 / 128), the two-kernel path with a ragged last
    # chunk, its second trip over the channels (C > 2048), rows below the rows held per pass
    return [_groupnorm(P, 2, 30, 512, 0, 1), _groupnorm(P, 1, 60, 200, 312, 1), _groupnorm(P, 1, 100, 512, 0, 1, silu=False),
            _groupnorm(P, 1, 201, 512, 0, 1), _groupnorm(P, 1, 37, 3072, 0, 3), _groupnorm(P, 2, 3, 24, 0, 8), _groupnorm(P, 2, 37, 40, 56, 8)]


def _gn_splitk(P, B, HW, C1, C2, groups, sk, store, step=None):
    M, Npad = B * HW, (C1 + 63) // 64 * 64
    sp = _lib.GnSplitKSrc()
    part = P(rn(7, sk * M * Npad, scale=0.5))
    bias, rv, res = P(rn(8, Npad)), P(rn(9, (3 if step is not None else 1) * B, C1)), P(rn(10, M, C1, dtype=BF16))
    pre = P.out((M, C1), BF16)
    sp.part, sp.split_k, sp.M, sp.N, sp.Npad = ptr(part), sk, M, C1, Npad
    sp.bias, sp.rowvec, sp.ldrv, sp.residual, sp.ldr = ptr(bias), ptr(rv), C1, ptr(res), C1
    keep = [part, bias, rv, res, pre]
    if step is not None:
        st, err = P(torch.tensor([step], dtype=I32)), P(Z(1, dtype=I32))
        sp.rowvec_step, sp.rowvec_step_stride, sp.rowvec_step_count, sp.step_error = ptr(st), B * C1, 3, ptr(err)
        keep += [st, err]
    sp.pre_out, sp.store_pre = ptr(pre), int(store)
    Cn = C1 + C2
    x2 = P(rn(4, M, C2, dtype=BF16)) if C2 else None
    g, b, y, ws = P(rn(5, Cn)), P(rn(6, Cn)), P.out((M, Cn), BF16), _gn_ws(P, B, Cn)
    ok(lib().pcdm_groupnorm_splitk(C.byref(sp), ptr(x2), C2, B, HW, groups, 1e-5, ptr(g), ptr(b), 1, ptr(y), ptr(ws), stream(P)), "groupnorm_splitk")
    return [y] + ([pre] if store else []) + keep[5:][1:]


@case("norms", "pcdm_groupnorm_splitk")
def case_groupnorm_splitk(P):
    # single-pass with a second source and a step counter (the last block of the table), the two-kernel path (group size 3: reduce launch first),
    # Npad 8 above N
    return [_gn_splitk(P, 2, 30, 200, 312, 1, 2, True, step=2), _gn_splitk(P, 2, 7, 24, 0, 8, 3, False), _gn_splitk(P, 1, 5, 56, 72, 8, 2, True, step=7)]


# ================================================================================================ the table: GEMM
def _t():
    from tests import test_gemm_conformance as T
    return T


def _bc(*a):
    """``build_case`` of the GEMM conformance suite (cached there: built with torch's own allocators, whichever side runs first)"""
    with G.unpatched():
        return _t().build_case(*a)


def _gemm(P, c, tile: int, extra: int = 0, w_ld: int = 0):
    """one ``pcdm_gemm`` call of a tests/test_gemm_conformance.py ``Case``: every operand at its exact extent; ``extra``: elements added to every
    row stride (0: tight).  -> (rc, outputs)"""
    T = _t()
    p = GemmParams()
    keep, outs = [], []

    def put(t, align=16):
        keep.append(P(t, align))
        return keep[-1]

    def put_rows(t, align=16):
        keep.append(P.rows(t, t.shape[1] + extra, align))
        return keep[-1]
    if c.conv is None:
        a = put_rows(c.a[:-1] if c.extra.get("short_a") else c.a)              # (short_a: the bite of the last section)
        p.a, p.lda, p.c1 = ptr(a), a.stride(0), a.shape[1]
        if c.a2 is not None:
            a2 = put_rows(c.a2)
            p.a2, p.lda2 = ptr(a2), a2.stride(0)
    else:
        g = c.conv
        p.a, p.conv = ptr(put(c.a.contiguous())), 1
        p.B, p.Hi, p.Wi, p.Ho, p.Wo, p.stride, p.upsample, p.cin = g["B"], g["Hi"], g["Wi"], g["Ho"], g["Wo"], g["stride"], g["upsample"], g["cin"]
        p.no_pad_lo = g.get("no_pad_lo", 0)
        if c.a2 is not None:
            a2 = put_rows(c.a2)
            p.a2, p.lda2, p.c1 = ptr(a2), a2.stride(0), c.a2.shape[1]
        if c.a3 is not None:
            a3 = put_rows(c.a3)
            p.a3, p.lda3 = ptr(a3), a3.stride(0)
        p.tap_lut, p.tap_group_n = c.tap_lut, c.tap_group_n
    if w_ld:                                                  # an activation slice as W: rows [0, Npad) at stride w_ld, the last one K long
        w = P.rows(c.w, w_ld)
        keep.append(w)
        p.ldw = w_ld
    else:
        w = put(c.w)
    p.w, p.M, p.N, p.K, p.Npad = ptr(w), c.M, c.N, c.K, c.Npad
    if c.bias is not None:
        p.bias = ptr(put(c.bias.float().contiguous()))
    p.rows_per_batch = c.rpb or c.M
    if c.rowvec is not None:
        step = c.extra.get("step")
        rv = put(c.rowvec.float().contiguous())
        p.rowvec, p.ldrv = ptr(rv), rv.stride(0)
        if step is not None:                                   # c.rowvec holds ``count`` blocks of M / rpb rows
            count = c.extra["step_count"]
            p.rowvec_step, p.rowvec_step_stride = ptr(put(torch.tensor([step], dtype=I32), 4)), rv.numel() // count
            p.rowvec_step_count, p.step_error = count, ptr(put(Z(1, dtype=I32), 4))
            outs.append(keep[-1])
    if c.residual is not None:
        r = put_rows(c.residual)
        p.residual, p.ldr, p.res_mod = ptr(r), r.stride(0), c.res_mod
    p.epilogue, p.vt_col0, p.act, p.zero_rows, p.dup_rows = c.epi, c.vt_col0, c.act, c.zero_rows, c.dup_rows
    if c.ln:
        p.ln_wsum, p.ln_eps = ptr(put(c.w.float().sum(1).contiguous())), c.ln_eps
        if c.ln_mode == 2:
            p.ln_row_stats = ptr(put(ops.row_stats_reference(c.a)))
    R, ncol = c.out_rows, c.out_cols
    if c.epi == T.NCHW:
        o = P.out((c.M * c.N,), F32)
        p.out, p.ldo = ptr(o), c.N
    else:
        o = P.out_rows(R, ncol, (ncol + 7) // 8 * 8 + extra, BF16)
        p.out, p.ldo = ptr(o), o.stride(0)
    outs.append(o)
    if c.epi == T.SPLIT_VT:
        B, cv = c.M // c.rpb, c.N - c.vt_col0
        o2 = P.out_rows(B * cv, c.rpb, (c.rpb + 7) // 8 * 8 + extra, BF16)
        p.out2, p.ldo2 = ptr(o2), o2.stride(0)
        outs.append(o2)
    if c.row_stats_out:
        rs = P.out((c.M * (c.N // 32) * 2,), F32)
        p.row_stats_out = ptr(rs)
        outs.append(rs)
    if c.split_k > 1:
        ws = P.out((c.split_k * c.M * c.Npad,), F32)
        p.split_k, p.ws, p.ws_floats = c.split_k, ptr(ws), ws.numel()
        keep.append(ws)
    p.tile = tile
    rc = lib().pcdm_gemm(C.byref(p), stream(P))
    return rc, outs


def _lin(M, N, K, Npad=None, seed=0, **kw):
    T = _t()
    Npad = Npad or (N + 63) // 64 * 64
    with G.unpatched():
        w, bias = T._pack_rows(rn(seed + 2, N, K) / math.sqrt(K), Npad), T._vec(N, Npad, seed + 3)
    return T.Case(name="lin", M=M, N=N, K=K, Npad=Npad, a=rn(seed + 1, M, K, dtype=BF16), w=w, bias=bias, **kw)


def _both_ld(P, c, tile, what):
    """tight, then every row stride one unit (8 elements) wider with a tight last row.  ``tile`` None: the first tile configuration that takes
    the case (tests/test_gemm_conformance.py ``expect_accept``)"""
    if tile is None:
        tile = next(t for t in (2, 5, 4, 18, 17) if _t().expect_accept(t, c))
    out = []
    for extra in (0, 8):
        rc, o = _gemm(P, c, tile, extra)
        ok(rc, f"{what} tile {tile} extra {extra}")
        out += o
    return out


@case("gemm", "pcdm_gemm")
def case_gemm_linear(P):
    out = []
    for M, N in ((70, 72), (1, 8)):
        c = _lin(M, N, 64)
        out += _both_ld(P, c, 0, "linear")
        c.residual, c.res_mod = rn(5, M, N, dtype=BF16), M
        out += _both_ld(P, c, 0, "linear + residual")
    c = _lin(70, 72, 128, c1=64)                               # a2: the channel concat
    c.a, c.a2 = c.a[:, :64].contiguous(), rn(6, 70, 64, dtype=BF16)
    out += _both_ld(P, c, 0, "a2")
    c = _lin(70, 72, 64, rpb=35)
    c.rowvec = rn(7, 2, 72)
    out += _both_ld(P, c, 0, "rowvec")
    c.residual, c.res_mod = rn(5, 37, 72, dtype=BF16), 37      # a broadcast residual of 37 rows
    out += _both_ld(P, c, 0, "residual broadcast")
    return out


@case("gemm", "pcdm_gemm")
def case_gemm_epilogues(P):
    T = _t()
    out = []
    c = _lin(27, 128, 64, rpb=9, epi=T.SPLIT_VT, vt_col0=64)   # SPLIT_VT at T 9
    out += _both_ld(P, c, 0, "split_vt")
    c = _lin(2 * 11, 4, 64, rpb=11, epi=T.NCHW)                # NCHW_F32 at N 4
    out += _both_ld(P, c, 0, "nchw")
    for feat in ("geglu", "act_silu", "act_gelu"):
        out += _both_ld(P, _bc(feat, 256, 64, False), None, feat)
    return out


def _conv(B, Hi, Wi, N, cin=64, stride=1, upsample=0, seed=0, **kw):
    T = _t()
    if upsample:
        Ho, Wo = 2 * Hi, 2 * Wi
    elif kw.get("no_pad_lo"):
        Ho, Wo = (Hi - 2) // stride + 1, (Wi - 2) // stride + 1
    else:
        Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    geo = dict(B=B, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, stride=stride, upsample=upsample, cin=cin, no_pad_lo=kw.pop("no_pad_lo", 0))
    K, Npad = 9 * cin, (N + 63) // 64 * 64
    with G.unpatched():
        w, bias = T._pack_rows(rn(seed + 2, N, K) / math.sqrt(K), Npad), T._vec(N, Npad, seed + 3)
    return T.Case(name="conv", M=B * Ho * Wo, N=N, K=K, Npad=Npad, a=rn(seed + 1, B, Hi, Wi, cin, dtype=BF16), w=w, bias=bias,
                  conv=geo, **kw)


@case("gemm", "pcdm_gemm")
def case_gemm_conv3x3(P):
    out = []
    out += _both_ld(P, _conv(1, 5, 7, 72), 0, "conv s1")
    out += _both_ld(P, _conv(2, 5, 7, 64, stride=2), 0, "conv s2")
    out += _both_ld(P, _conv(1, 1, 1, 64), 0, "conv 1x1")
    out += _both_ld(P, _conv(1, 5, 7, 64, split_k=3), 2, "conv split-K 3")
    out += _both_ld(P, _conv(1, 3, 4, 64, upsample=1), 0, "conv x2 upsample")
    out += _both_ld(P, _conv(1, 6, 8, 64, stride=2, no_pad_lo=1), 0, "conv no_pad_lo")
    return out


@case("gemm", "pcdm_gemm")
def case_gemm_features(P):
    T = _t()
    out = []
    for feat in ("conv_dup_rows", "conv_extra_a2", "conv_extra_a2_a3", "conv_taps4", "conv_taps1", "zero_rows", "two_source", "split_k2",
                 "residual_bcast", "split_vt_ragged", "row_stats"):
        out += _both_ld(P, _bc(feat, 256, 256 if feat in ("two_source", "split_k2") else 64, False), None, feat)
    return out


@case("gemm", "pcdm_gemm")
def case_gemm_rowvec_step(P):
    out = []
    for step in (0, 2, 5):                                    # the first block, the last one, and a counter beyond the table (clamped on the device)
        c = _lin(70, 72, 64, rpb=35)
        c.rowvec = rn(7, 3 * 2, 72)
        c.extra.update(step=step, step_count=3)
        out += _both_ld(P, c, 0, f"rowvec_step {step}")
    return out


@case("gemm", "pcdm_gemm")
def case_gemm_folded_layernorm(P):
    T = _t()
    out = []
    for feat, tile in (("ln1_store", 2), ("ln1_split_vt", 4), ("ln2_store", 2), ("ln2_store", 23), ("ln2_geglu", 23), ("ln1_geglu", 18)):
        out += _both_ld(P, _bc(feat, T._npad_for(tile), 128, False), tile, f"{feat}")
    return out


@case("gemm", "pcdm_gemm")
def case_gemm_ldw_activation_slice(P):
    """an activation slice as W (the per-head Q of the CLIP attention): Npad rows at stride ldw are read, the last one K long"""
    T = _t()
    out = []
    c = _lin(9, 12, 64, Npad=64, rpb=9, epi=T.NCHW)
    c.bias = None
    for w_ld in (64, 2 * 80):
        for extra in (0, 8):
            rc, o = _gemm(P, c, 0, extra, w_ld=w_ld)
            ok(rc, f"ldw {w_ld} extra {extra}")
            out += o
    return out


TILED = tuple(t for t in sorted(ops.TILE_SHAPES) if t not in ops.ROWGEMM_TILES)


@case("gemm_tiles", "pcdm_gemm")
def case_gemm_every_tile(P):
    """every tiled configuration at M = one tile + 1 row, one N tile, N 8 below Npad"""
    out = []
    for t in TILED:
        bm, bn = ops.TILE_SHAPES[t]
        out += _both_ld(P, _lin(bm + 1, bn - 8, 64, Npad=bn, seed=t), t, "one tile + 1 row")
    return out


@case("rowgemm", "pcdm_gemm")
def case_rowgemm(P):
    T = _t()
    out = []
    for t, M in ((31, 70), (33, 97), (36, 1), (35, 129), (32, 193)):
        bn = ops.TILE_SHAPES[t][1]
        c = _lin(M, bn - 8, 320, Npad=bn, seed=t)
        c.residual, c.res_mod = rn(5, M, c.N, dtype=BF16), M
        out += _both_ld(P, c, t, f"rowgemm {t}")
    out += _both_ld(P, _bc("geglu", 256, 320, False), 34, "rowgemm 34 GEGLU")
    out += _both_ld(P, _bc("ln1_store", 256, 320, False), 31, "rowgemm 31 folded LayerNorm")
    out += _both_ld(P, _bc("ln1_split_vt", 256, 320, False), 33, "rowgemm 33 folded LayerNorm, SPLIT_VT")
    return out


# ================================================================================================ the table: attention
def _attn(P, kind, B, H, Lq, Lk, ldvt, d=64, extra=0):
    Cn = H * d
    q, k = rn(1, B * Lq, Cn, dtype=BF16), rn(2, B * Lk, Cn, dtype=BF16)
    vt = Z(B, Cn, ldvt, dtype=BF16)
    vt[:, :, :Lk] = rn(3, B, Cn, Lk, dtype=BF16)
    qd, o = P.rows(q, Cn + extra), P.out_rows(B * Lq, Cn, Cn + extra, BF16)
    if kind == "bf16":
        ops.flash_attn(qd, P.rows(k, Cn + extra), P(vt), o, B, H, Lq, Lk)      # vt: whole rows (the padding of the last key tile is read by design)
    elif kind == "fp8":
        k8 = ops.quantize_fp8(P(k), P.out_rows(B * Lk, Cn, Cn + 2 * extra, U8))       # (the operands of the attention are the outputs of these)
        vt8 = ops.quantize_fp8(P(vt.view(B * Cn, ldvt)), P.out((B * Cn, ldvt), U8), cols=Lk)
        ops.flash_attn_fp8(qd, k8, vt8.view(B, Cn, ldvt), o, B, H, Lq, Lk)
    else:                                                                      # wide: columns [Lk, ldvt) are never used -> a tight last row
        kd = P.rows(k, Cn + extra)
        vd = P.rows(vt.view(B * Cn, ldvt)[:, :Lk], ldvt)
        ok(lib().pcdm_attn_wide(ptr(qd), qd.stride(0), ptr(kd), kd.stride(0), ptr(vd), ldvt, ptr(o), o.stride(0), B, Lq, Lk, d, d ** -0.5, stream(P)),
           "attn_wide")
    return o


@case("attention", "pcdm_flash_attn", "pcdm_flash_attn_thr")
def case_flash_attn(P):
    out = []
    for extra in (0, 8):
        out += [_attn(P, "bf16", 2, 2, 33, 9, 16, extra=extra), _attn(P, "bf16", 1, 1, 1, 1, 8, extra=extra), _attn(P, "bf16", 1, 2, 129, 65, 72, extra=extra)]
    q, k, vt, o = P(rn(1, 33, 64, dtype=BF16)), P(rn(2, 9, 64, dtype=BF16)), P(rn(3, 1, 64, 16, dtype=BF16)), P.out((33, 64), BF16)
    out.append(ops.flash_attn(q, k, vt, o, 1, 1, 33, 9, thr=0.0))
    return out


@case("attention", "pcdm_flash_attn_fp8", "pcdm_quantize_fp8")
def case_flash_attn_fp8(P):
    return [_attn(P, "fp8", 2, 2, 33, 9, 16, extra=e) for e in (0, 8)] + [_attn(P, "fp8", 1, 2, 129, 65, 80, extra=e) for e in (0, 8)]


@case("attention", "pcdm_attn_wide")
def case_attn_wide(P):
    return [_attn(P, "wide", 2, 1, 33, 9, 16, d=64, extra=e) for e in (0, 8)] + [_attn(P, "wide", 1, 1, 5, 70, 72, d=512, extra=e) for e in (0, 8)]


@case("attention", "pcdm_quantize_fp8")
def case_quantize_fp8(P):
    out = []
    x = rn(1, 5, 13, dtype=BF16)
    for ldx, ax in ((13, 2), (16, 16), (21, 2)):               # x: natural 2-byte alignment, any ldx >= cols; y: 8 bytes
        y = P.out_rows(5, 16, 16, U8, 8)
        out.append(ops.quantize_fp8(P.rows(x, ldx, ax), y, cols=13))
    y = P.out_rows(5, 16, 24, U8, 8)
    out.append(ops.quantize_fp8(P.rows(x, 24), y, cols=13))
    return out


@case("attention", "pcdm_softmax_rows")
def case_softmax_rows(P):
    out = []
    for cols in (1, 37):
        for lds, ldp in ((cols, cols), (cols + 3, cols + 5)):
            o = P.out_rows(3, cols, ldp, BF16, 2)
            out.append(ops.softmax_rows(P.rows(rn(cols, 3, cols), lds, 4), o, 0.125))
    return out


# ================================================================================================ the table: embeddings, layout, sampler steps
@case("steps", "pcdm_small_linear")
def case_small_linear(P):
    x, w = rn(1, 3, 8), rn(2, 5, 8, dtype=BF16)
    return [ops.small_linear(P(x), P(w), P(rn(3, 5)), P.out((3, 5), F32), add=P(rn(4, 3, 5)), act_in=True, act_out=2),
            ops.small_linear(P(x), P(w), None, P.out((3, 5), F32))]


@case("steps", "pcdm_timestep_embedding", "pcdm_timestep_embedding_f32", "pcdm_timestep_embedding_rows", "pcdm_timestep_embedding_rows_f32")
def case_timestep_embedding(P):
    out = []
    for t in (torch.tensor([801, 401, 1], dtype=I64), torch.tensor([801.0, 400.25, 1.0])):
        for step in (2, _beyond(P, 3)):                       # the last row, and a counter beyond the table (clamped to it: the flag is an output)
            err = P(Z(1, dtype=I32), 4)
            out += [ops.timestep_embedding(P(t), P(torch.tensor([step], dtype=I32), 4), P.out((3, 64), F32), step_error=err), err]
        out.append(ops.timestep_embedding(P(t[:1]), None, P.out((1, 6), F32), flip=False, shift=1.0))
        out.append(ops.timestep_embedding_rows(P(t), P.out((3, 64), F32)))
        out.append(ops.timestep_embedding_rows(P(t), P.out((3, 6), F32), flip=False))
    return out


@case("steps", "pcdm_time_class_combine")
def case_time_class_combine(P):
    return [ops.time_class_combine(P(rn(1, 3, 72)), P(rn(2, 2, 72)), P.out((6, 72), BF16), 2),
            ops.time_class_combine(P(rn(1, 3, 5)), None, P.out((3, 5), BF16), 1)]


@case("steps", "pcdm_assemble_input", "pcdm_assemble_input_ex")
def case_assemble_input(P):
    out = []
    lat, mask, masked = rn(1, 2, 4, 3, 5), rn(2, 1, 1, 3, 5), rn(3, 4, 4, 3, 5)
    out.append(ops.assemble_input(P(lat), 2, P(mask), P(masked), P.out((4, 3, 5, 16), BF16)))
    out.append(ops.assemble_input(P(lat), 1, None, P(masked[:1]), P.out((2, 3, 5, 16), BF16)))
    tab = rn(4, 3, ops.MS_ROW)
    for step in (2, 9):                                       # the last row, and a counter beyond the table
        err = P(Z(1, dtype=I32), 4)
        out += [ops.assemble_input_ex(P(lat), 2, P(mask.expand(4, 1, 3, 5).contiguous()), P(masked), P.out((4, 3, 5, 16), BF16), P(tab), ops.MS_IN_SCALE,
                                      P(torch.tensor([step], dtype=I32), 4), err), err]
    return out


@case("steps", "pcdm_nchw_f32_to_nhwc_bf16", "pcdm_nhwc_bf16_to_nchw_f32", "pcdm_f32_to_bf16", "pcdm_pixel_shuffle2", "pcdm_advance_step")
def case_layout(P):
    out = [ops.nchw_to_nhwc_bf16(P(rn(1, 2, 3, 3, 5)), P.out((2, 3, 5, 8), BF16)), ops.nhwc_bf16_to_nchw(P(rn(2, 2 * 15, 8, dtype=BF16)), 2, 8, 3, 5),
           ops.nhwc_bf16_to_nchw(P(rn(2, 15, 3, dtype=BF16), 2), 1, 3, 3, 5)]
    for n in (1, 63, 257):
        out.append(ops.f32_to_bf16(P(rn(n, n)), P.out((n,), BF16, 2)))
    out.append(ops.pixel_shuffle2(P(rn(3, 2 * 3 * 5, 32, dtype=BF16)), P.out((2 * 6 * 10, 8), BF16), 2, 3, 5, 8))
    st = P(torch.tensor([3], dtype=I32), 4)
    ops.advance_step(st)
    return out + [st]


def _state(P, n, k, seed=0):
    return [P(rn(seed + i, n)) for i in range(k)]


def _beyond(P, rows):
    """a step counter beyond a table of ``rows`` rows.  Guard pages (CPU): 9 with 3 rows.  Fills (GPU): ``rows`` -- the first row behind the
    table, which even an unbounded read finds inside the window's 4 KiB margin while a row is at most that long (asserted by the callers'
    shapes: the widest row here is 260 floats)"""
    assert rows == 3 and G.WindowPlace.MARGIN >= 260 * 4
    return rows if P.device.type == "cuda" else 9


@case("steps", "pcdm_cfg_step")
def case_cfg_step(P):
    out = []
    for n in (1, 63, 260):
        for step in (2, _beyond(P, 3)):                       # the last row, and a counter beyond the table
            coef, st, err = P(rn(9, 3, 4)), P(torch.tensor([step], dtype=I32), 4), P(Z(1, dtype=I32), 4)
            xp, eo = P.out((n,), F32), P.out((n,), F32)
            ops.cfg_step(P(rn(1, 2 * n)), True, 7.5, P(rn(2, n)), xp, coef, st, noise=P(rn(3, n)), eps_out=eo, step_error=err)
            out += [xp, eo, err]
        xp = P.out((n,), F32)
        ops.cfg_step(P(rn(1, n)), False, 1.0, P(rn(2, n)), xp, P(rn(9, 3, 4)), None)
        out.append(xp)
        eo = P.out((n,), F32)                                 # the CFG combine alone: no table
        ops.cfg_step(P(rn(1, 2 * n)), True, 7.5, None, None, None, eps_out=eo)
        out.append(eo)
    return out


@case("steps", "pcdm_multistep_step")
def case_multistep_step(P):
    out = []
    for n in (1, 63, 260):
        for cfg, noise, step in ((True, True, 2), (False, False, None), (True, True, 7)):
            coef = rn(9, 3, ops.MS_ROW)
            coef[:, ops.MS_SAVE:ops.MS_PUSH + 1] = 1.0
            st = _state(P, n, 5, seed=n)
            err = P(Z(1, dtype=I32), 4)
            ops.multistep_step(P(rn(1, (2 if cfg else 1) * n)), cfg, 2.0, *st, P(rn(8, 3, n)) if noise else None, P(coef),
                               None if step is None else P(torch.tensor([step], dtype=I32), 4), err)
            out += st + [err]
    return out


@case("steps", "pcdm_unipc_step", "pcdm_dpmpp_step")
def case_unipc_dpmpp_step(P):
    out = []
    for n in (1, 63, 260):
        for cfg, step in ((True, 2), (False, None), (True, _beyond(P, 3))):     # the last row, no counter, a counter beyond the tables
            st = _state(P, n, 4, seed=n)
            c12 = rn(9, 3, 12)
            c12[:, 2] = 1.0
            e1, e2 = P(Z(1, dtype=I32), 4), P(Z(1, dtype=I32), 4)
            ops.unipc_step(P(rn(1, (2 if cfg else 1) * n)), cfg, 2.0, *st, P(c12), P(torch.tensor([2 if step is None else step], dtype=I32), 4), e1)
            s2 = _state(P, n, 2, seed=n + 7)
            ops.dpmpp_step(P(rn(1, (2 if cfg else 1) * n)), cfg, 2.0, *s2, P(rn(8, 3, n)) if cfg else None, P(rn(10, 3, 8)),
                           None if step is None else P(torch.tensor([step], dtype=I32), 4), e2)
            out += st + s2 + [e1, e2]
    return out


@case("steps", "pcdm_unclip_step", "pcdm_unclip_step_dev")
def case_unclip_step(P):
    out = []
    c8 = (1.1875, -0.640625, 1.5, 0.4375, 0.5625, 0.21875, 1.25, -0.09375)
    for n in (1, 63, 260):
        for cfg in (True, False):
            out.append(ops.unclip_step(P(rn(1, (2 if cfg else 1) * n)), cfg, 4.0, P(rn(2, n)), P(rn(3, n)) if cfg else None, P.out((n,), F32), c8))
            for step in (2, _beyond(P, 3)):                   # the last row, and a counter beyond the tables
                x, err = P(rn(2, n)), P(Z(1, dtype=I32), 4)
                ops.unclip_step_dev(P(rn(1, (2 if cfg else 1) * n)), cfg, 4.0, x, P(rn(8, 3, n)) if cfg else None, P(torch.tensor([c8] * 3)),
                                    P(torch.tensor([step], dtype=I32), 4), err)
                out += [x, err]
    return out


@case("steps", "pcdm_lincomb", "pcdm_rescale_noise_cfg")
def case_lincomb_rescale(P):
    out = []
    for n in (1, 63, 260):
        out.append(ops.lincomb(P.out((n,), F32), [P(rn(i, n)) for i in range(6)], (0.75, -1.3125, 0.40625, 2.5, -0.15625, 0.9375)))
    out.append(ops.lincomb(P.out((5,), F32), [P(rn(1, 5))], (2.0,)))
    out.append(ops.rescale_noise_cfg(P(rn(1, 2, 37)), P(rn(2, 2, 37)), P.out((2, 37), F32), 0.7))
    return out


@case("steps", "pcdm_gaussian_sample", "pcdm_image_to_uint8")
def case_vae_helpers(P):
    B, zc, HW = 2, 4, 15
    mom, noise, o = P(rn(1, B, 2 * zc, HW)), P(rn(2, B, zc, HW)), P.out((B, zc, HW), F32)
    ok(lib().pcdm_gaussian_sample(ptr(mom), ptr(noise), ptr(o), B, zc, HW, 0.18215, stream(P)))
    x, u = P(rn(3, B, 3, HW)), P.out((B, HW, 3), U8, 1)
    ok(lib().pcdm_image_to_uint8(ptr(x), ptr(u), B, 3, HW, stream(P)))
    x8 = rn(4, B, 8, HW)[:, :, :]                              # cstride 8: the last image ends behind its third channel
    x8 = P(x8.reshape(-1)[:(B - 1) * 8 * HW + 3 * HW])
    u8 = P.out((B, HW, 3), U8, 1)
    ok(lib().pcdm_image_to_uint8(ptr(x8), ptr(u8), B, 8, HW, stream(P)))
    return [o, u, u8]


@case("steps", "pcdm_freeu", "pcdm_freeu_ws_bytes")
def case_freeu(P):
    out = []
    for B, H, W, C1, C2 in ((2, 3, 5, 16, 8), (1, 8, 8, 64, 72), (1, 1, 1, 8, 8), (1, 19, 19, 16, 8)):   # 19 x 19 = 361 > 355: two launches, a workspace
        nb = ops.freeu_ws_bytes(B, H, W, C1, C2)
        assert nb >= 0 and (nb > 0) == (H * W > 355)
        ws = P.out((nb,), U8) if nb else None
        ho, so = P.out((B * H * W, C1), BF16), P.out((B * H * W, C2), BF16)
        ops.freeu(P(rn(1, B * H * W, C1, dtype=BF16)), P(rn(2, B * H * W, C2, dtype=BF16)), so, B, H, W, 1.25, 0.5, hidden_out=ho, ws=ws)
        h = P(rn(1, B * H * W, C1, dtype=BF16))
        ops.freeu(h, P(rn(2, B * H * W, C2, dtype=BF16)), P.out((B * H * W, C2), BF16), B, H, W, 1.25, 0.5, ws=ws)      # in place
        out += [ho, so, h]
    return out


# ================================================================================================ the table: fp32 nets (LPIPS, FID, pose, detector)
def _pw(P, cout, cin, kh, kw, seed=0, bias=True):
    with G.unpatched():                                       # (host packing: the packed tensors are placed below)
        pw = ops.pack_lpips_conv(rn(seed, cout, cin, kh, kw, scale=0.2), rn(seed + 1, cout) if bias else None, "cpu")
    return dict(pw, w=P(pw["w"]), bias=P(pw["bias"]))


def _nhwc(x, cpad):
    """NCHW fp32 -> NHWC with the channels zero-padded to ``cpad``"""
    B, Cn, H, W = x.shape
    o = Z(B, H, W, cpad)
    o[..., :Cn] = x.permute(0, 2, 3, 1)
    return o


@case("nets", "pcdm_conv2d_f32", "pcdm_conv2d_f32_ex", "pcdm_pack_lpips_conv")
def case_conv2d_f32(P):
    out = []
    for cout in (5, 133):
        pw = _pw(P, cout, 4, 3, 3, seed=cout)
        x = P(_nhwc(rn(1, 2, 4, 7, 9), pw["cin"]))
        out.append(ops.conv2d_f32(x, pw, stride=2, pad=1, relu=True))
        out.append(ops.conv2d_f32_ex(x, pw, stride=2, pad=(1, 0)))
        o = P.out((2, 7, 9, (cout + 3) // 4 * 4 + 8), F32)     # into the channels [4, 4 + cout) of a wider tensor
        out.append(ops.conv2d_f32_ex(x, pw, pad=(1, 1), out=o, offset=4))
    pw = _pw(P, 8, 3, 11, 11, seed=3)                          # LPIPS conv1: 11 x 11, stride 4, 3 channels padded to 4
    out.append(ops.conv2d_f32(P(_nhwc(rn(2, 1, 3, 31, 31), pw["cin"])), pw, stride=4, pad=2, relu=True))
    pw = _pw(P, 6, 8, 1, 7, seed=4)                            # the 1 x 7 / 7 x 1 convolutions of InceptionV3
    out.append(ops.conv2d_f32_ex(P(rn(3, 1, 5, 9, 8)), pw, pad=(0, 3)))
    return out


@case("nets", "pcdm_conv2d_f32_act")
def case_conv2d_f32_act(P):
    out = []
    pw = _pw(P, 12, 8, 3, 3, seed=5)
    x = P(rn(1, 2, 5, 7, 20))                                  # reads the channels [12, 20) of a 20-channel tensor: the last slice of the last pixel
    res, asc = P(rn(2, 2, 5, 7, 15)), P(rn(3, 2, 8))
    o = P.out((2, 5, 7, 20), F32)                              # writes the channels [8, 20)
    out.append(ops.conv2d_f32_act(x, pw, pad=(1, 1), act=ops.CONV_ACT_SILU, in_offset=12, residual=res, res_offset=3, a_scale=asc, out=o, offset=8))
    out.append(ops.conv2d_f32_act(x, pw, stride=2, pad=(1, 1), act=ops.CONV_ACT_RELU))
    pw1 = _pw(P, 5, 4, 1, 1, seed=6)
    out.append(ops.conv2d_f32_act(P(rn(4, 1, 1, 1, 4)), pw1))
    return out


@case("nets", "pcdm_maxpool3s2_f32", "pcdm_maxpool3s2_f32_ex", "pcdm_avgpool3_f32", "pcdm_global_avgpool_f32", "pcdm_maxpool5_f32",
      "pcdm_upsample2_nearest_f32", "pcdm_dwconv5_silu_f32")
def case_pools(P):
    out = []
    x = P(rn(1, 2, 7, 9, 8))
    out.append(ops.maxpool3s2_f32(x))
    out.append(ops.maxpool3s2_f32_ex(x, P.out((2, 3, 4, 12), F32), offset=4))
    out.append(ops.maxpool3s2_f32(P(rn(2, 1, 3, 3, 4))))
    out += [ops.avgpool3_f32(x), ops.avgpool3_f32(P(rn(3, 1, 1, 1, 4))), ops.global_avgpool_f32(x), ops.global_avgpool_f32(P(rn(3, 1, 1, 1, 3)))]
    x12 = P(rn(4, 2, 2, 3, 12))
    out.append(ops.maxpool5_f32(x12, 4, P.out((2, 2, 3, 12), F32), in_offset=8, offset=8))
    out.append(ops.maxpool5_f32(P(rn(5, 1, 9, 12, 4)), 4, P.out((1, 9, 12, 4), F32)))
    out.append(ops.upsample2_nearest_f32(x12, 4, P.out((2, 4, 6, 12), F32), in_offset=8, offset=8))
    out.append(ops.upsample2_nearest_f32(P(rn(6, 1, 1, 1, 4)), 4, P.out((1, 2, 2, 4), F32)))
    for Cn, H, W in ((4, 1, 1), (36, 9, 12)):
        xx = P(rn(7, 2, H, W, Cn + 4))
        out.append(ops.dwconv5_silu_f32(xx, P(rn(8, 25, Cn)), P(rn(9, Cn)), P.out((2, H, W, Cn + 8), F32), in_offset=4, offset=8))
    return out


@case("nets", "pcdm_fc_hsigmoid_f32", "pcdm_scalenorm_f32", "pcdm_gau_core_f32", "pcdm_simcc_decode")
def case_pose_head(P):
    out = [ops.fc_hsigmoid_f32(P(rn(1, 3, 12)), P(rn(2, 12, 12)), P(rn(3, 12)))]
    # ScaleNorm over dim 6 of a transposed tensor [B, dim, rows]: element i of row (b, k) at b dim rows + k + i rows
    B, rows, dim = 2, 5, 6
    out += list(ops.scalenorm_f32(P(rn(4, B, dim, rows)), B, rows, dim, (dim * rows, 1, rows), P(rn(5, 1)), side_scale=P(rn(6, dim))))
    out.append(ops.scalenorm_f32(P(rn(4, 3, 8)), 1, 3, 8, (0, 8, 1), P(rn(5, 1))))
    e = 8
    out.append(ops.gau_core_f32(P(rn(7, 2 * 5, 2 * e + 128, scale=0.3)), 2, P(rn(8, 2, 128)), P(rn(9, 2, 128))))
    R, K, xb, yb = 2, 7, 12, 20
    boxes = torch.tensor([[4.0, 3.0, 40.0, 60.0], [-8.0, 10.0, 45.0, 66.0]])
    out += list(ops.simcc_decode(P(rn(10, 2 * R * K, xb + yb)), xb, R, K, P(torch.arange(K - 1, -1, -1, dtype=I32), 4), P(boxes), (10, 6)))
    out += list(ops.simcc_decode(P(rn(10, R * K, xb + yb)), xb, R, K, None, P(boxes), (10, 6)))
    return out


@case("nets", "pcdm_pose_crop", "pcdm_detect_prep", "pcdm_detect_decode", "pcdm_nms_f32")
def case_pose_detect_io(P):
    out = []
    img = P(ru8(1, 2, 23, 17, 3), 1)
    boxes = torch.tensor([[4.0, 3.0, 12.0, 20.0], [-8.0, -10.0, 30.0, 40.0], [14.0, 18.0, 16.9, 22.9], [-5.0, 5.0, 3.0, 30.0]])   # boxes that leave the image
    out.append(ops.pose_crop(img, P(boxes), P(torch.tensor([0, 1, 1, 0], dtype=I32), 4), (16, 12), flip=True))
    out.append(ops.pose_crop(img, P(boxes[:1]), None, (16, 12), flip=False))
    out.append(ops.detect_prep(img, 32))
    out.append(ops.detect_prep(P(ru8(2, 1, 9, 40, 3), 1), 32))
    S, Cn = 32, 5
    heads = [P(rn(3 + i, 2, S // st, S // st, 8 + 8)) for i, st in enumerate((8, 16, 32))]
    bx, sc, lab, cand = ops.detect_decode(heads, S, Cn, 0, 0.3, (23, 17))
    out += [bx, sc, lab, cand]
    N, Pn = 2, 21
    b0 = torch.rand(N, Pn, 2, generator=torch.Generator().manual_seed(4)) * 20
    bb = torch.cat([b0, b0 + 6.0], -1)
    r = ops.nms_f32(P(bb), P(torch.rand(N, Pn, generator=torch.Generator().manual_seed(5))), P(torch.ones(N, Pn, dtype=I32), 4), thr=0.5, offset=1.0,
                    max_candidates=16, max_det=4, overflow_in=P(Z(N, dtype=I32), 4))
    out += list(r.values())
    r = ops.nms_f32(P(bb), P(torch.rand(N, Pn, generator=torch.Generator().manual_seed(5))), P(torch.ones(N, Pn, dtype=I32), 4), thr=0.5, offset=0.0,
                    max_candidates=32, max_det=32, want_keep=False)
    return out + [r["boxes"], r["scores"], r["count"], r["overflow"]]


@case("nets", "pcdm_inception_input", "pcdm_fid_accumulate", "pcdm_fid_finalize")
def case_fid_io(P):
    out = []
    img8, imgf = P(ru8(1, 2, 17, 23, 3), 1), P(torch.rand(2, 3, 17, 23, generator=torch.Generator().manual_seed(2)))
    for win in ((0, 0, 23, 17), (10, 6, 13, 11)):              # the whole image; a window in the bottom right corner
        out.append(ops.inception_input(img8, win, resize=False, normalize=True))
        out.append(ops.inception_input(imgf, win, resize=False, normalize=False))
    out.append(ops.inception_input(P(ru8(3, 1, 5, 4, 3), 1), (1, 1, 3, 4), resize=True, normalize=True))
    D = 5
    tot, gram = P(Z(D, dtype=F64)), P(Z(D, D, dtype=F64))
    ops.fid_accumulate(P(rn(4, 3, D)), tot, gram)
    out += [tot, gram] + list(ops.fid_finalize(tot, gram, 3))
    return out


# ================================================================================================ the table: image metrics and input preparation
def _metric_ws(P, N, ref_n, W, H, sigma):
    return P.out((ops.metrics_ws_bytes(N, ref_n, W, H, sigma),), U8, 8)


@case("image", "pcdm_ssim", "pcdm_psnr", "pcdm_absdiff", "pcdm_ssim_box", "pcdm_select_image", "pcdm_metrics_ws_bytes", "pcdm_ssim_box_ws_bytes")
def case_image_metrics(P):
    out = []
    H, W, N = 17, 23, 2
    for f32 in (False, True):
        mk = (lambda s, n: torch.rand(n, H, W, 3, generator=torch.Generator().manual_seed(s))) if f32 else (lambda s, n: ru8(s, n, H, W, 3))
        al = 4 if f32 else 1
        # windows touching each border of the image: the whole image, the top left, the bottom right, the right edge
        for cw, rw, ref_n in (((0, 0, W, H), (0, 0, W, H), 1), ((0, 0, 11, 9), (12, 8, 11, 9), N), ((12, 8, 11, 9), (0, 0, 11, 9), 1), ((14, 3, 9, 11), (14, 6, 9, 11), N)):
            cand, ref = P(mk(1, N), al), P(mk(2, ref_n), al)
            ww, hh = cw[2], cw[3]
            out.append(ops.ssim(cand, ref, cw, rw, P.out((N,), F32, 4), P.out((1,), I32, 4), _metric_ws(P, N, ref_n, ww, hh, 1.2), sigma=1.2,
                                data_range=None if f32 else 255.0))
            mse, ps = P.out((N,), F32, 4), P.out((N,), F32, 4)
            ops.psnr(cand, ref, cw, rw, mse, ps, _metric_ws(P, N, ref_n, ww, hh, 0.0), data_range=1.0 if f32 else 255.0)
            l1, mae = P.out((N,), F32, 4), P.out((N,), F32, 4)
            ops.absdiff(cand, ref, cw, rw, l1, mae, _metric_ws(P, N, ref_n, ww, hh, 0.0))
            out += [mse, ps, l1, mae]
            out.append(ops.ssim_box(cand, ref, cw, rw, P.out((N,), F32, 4), P.out((ops.ssim_box_ws_bytes(N, ref_n, ww, hh, 7),), U8, 8), win_size=7,
                                    data_range=None if f32 else 255.0))
            if not f32:
                idx = P(torch.tensor([N - 1], dtype=I32), 4)
                out.append(ops.select_image(cand, cw, idx, P.out((hh, ww, 3), U8, 1), False))
                out.append(ops.select_image(cand, cw, idx, P.out((1, 3, hh, ww), F32, 4), True))
    return out


@case("image", "pcdm_resample_u8", "pcdm_u8_to_nchw", "pcdm_resize_cubic_f32", "pcdm_resize_linear_u8", "pcdm_resample_ws_bytes")
def case_image_prep(P):
    from pcdms_amd import preprocess
    out = []
    for (Hs, Ws), (Wd, Hd) in (((41, 29), (11, 17)), ((23, 19), (31, 52)), ((50, 44), (44, 21))):   # 41 -> 17 rows, 23 -> 52 rows, one axis kept
        out.append(preprocess.resize(P(ru8(Hs, Hs, Ws, 3), 1), (Wd, Hd)))
        out.append(preprocess.resize_cv_cubic(P(ru8(Hs, Hs, Ws, 3), 1), (Wd, Hd)))
        out.append(preprocess.resize_cv_cubic(P(torch.rand(Hs, Ws, 3, generator=torch.Generator().manual_seed(Ws)), 4), (Wd, Hd), divisor=255.0, layout="nchw"))
    src = P(ru8(5, 17, 23, 3), 1)
    for win in ((0, 0, 23, 17), (12, 8, 11, 9)):
        o = P.out((1, 3, win[3], win[2]), F32, 4)
        out.append(ops.u8_to_nchw(src, win, o, mode=0, scale=255.0, mean=(0.5, 0.4, 0.3), std=(0.2, 0.3, 0.4)))
    out.append(ops.resize_linear_u8(P(ru8(6, 2, 17, 23, 3), 1), P.out((2, 31, 11, 3), U8, 1)))
    out.append(ops.resize_linear_u8(P(ru8(6, 1, 5, 4, 3), 1), P.out((1, 2, 9, 3), U8, 1)))
    return out


@case("image", "pcdm_pose_draw", "pcdm_pose_ws_bytes")
def case_pose_draw(P):
    from pcdms_amd import pose
    g = torch.Generator().manual_seed(3)
    kp = torch.rand(2, 2, 134, 2, generator=g) * torch.tensor([40 + 8.0, 48 + 8.0]) - 4.0       # some joints outside the frame
    sc = torch.rand(2, 2, 134, generator=g)
    return [pose.draw_pose(P(kp, 4), P(sc, 4), (48, 40)), pose.draw_pose(P(kp, 4), P(sc, 4), (48, 40), image_size=(31, 27), faces=True)]


@case("host", "pcdm_pack_linear", "pcdm_pack_conv3x3", "pcdm_pack_geglu", "pcdm_pack_lpips_conv")
def case_host_packers(P):
    """the host packers, as plain host code: fp32 sources and packed destinations on guard pages"""
    out = []
    N, K, Npad = 5, 64, 64
    w, b = P(rn(1, N, K)), P(rn(2, N))
    ow, ob = P.out((Npad, K), BF16), P.out((Npad,), F32)
    assert lib().pcdm_pack_linear(ptr(w), ptr(b), N, K, 64, ptr(ow), ptr(ob)) == Npad
    out += [ow, ob]
    cin, cp = 3, 64
    w, b = P(rn(3, N, cin, 3, 3)), P(rn(4, N))
    ow, ob = P.out((Npad, 9 * cp), BF16), P.out((Npad,), F32)
    assert lib().pcdm_pack_conv3x3(ptr(w), ptr(b), N, cin, 64, ptr(ow), ptr(ob), None, None) == Npad
    out += [ow, ob]
    D = 40
    w, b = P(rn(5, 2 * D, K)), P(rn(6, 2 * D))
    ow, ob = P.out((2 * 64, K), BF16), P.out((2 * 64,), F32)
    assert lib().pcdm_pack_geglu(ptr(w), ptr(b), D, K, ptr(ow), ptr(ob)) == 2 * 64
    out += [ow, ob]
    w, b = P(rn(7, 5, 3, 3, 3)), P(rn(8, 5))
    Kc, cpad = C.c_int(0), C.c_int(0)
    npad = lib().pcdm_pack_lpips_conv(None, None, 5, 3, 3, 3, None, None, C.byref(Kc), C.byref(cpad))
    assert npad > 0
    ow, ob = P.out((Kc.value * npad,), F32), P.out((npad,), F32)
    assert lib().pcdm_pack_lpips_conv(ptr(w), ptr(b), 5, 3, 3, 3, ptr(ow), ptr(ob), None, None) >= 0
    return out + [ow, ob]


# ================================================================================================ schedules: whole tiny models, every buffer guarded
def guard_tree(P, obj, seen=None):
    """every contiguous tensor reachable through dicts, lists, tuples and ``PackedWeight`` fields replaced by a guarded copy (one copy per
    tensor object, so aliases stay aliases)"""
    seen = {} if seen is None else seen
    if isinstance(obj, torch.Tensor):
        if id(obj) not in seen:
            seen[id(obj)] = (P(obj) if obj.is_contiguous() and obj.numel() and obj.device.type == P.device.type else obj, obj)
        return seen[id(obj)][0]
    if isinstance(obj, dict):
        for k in list(obj):
            obj[k] = guard_tree(P, obj[k], seen)
    elif isinstance(obj, list):
        obj[:] = [guard_tree(P, v, seen) for v in obj]
    elif isinstance(obj, tuple):
        return tuple(guard_tree(P, v, seen) for v in obj)
    elif isinstance(obj, ops.PackedWeight):
        for f in ("w", "bias", "wsum"):
            setattr(obj, f, guard_tree(P, getattr(obj, f), seen))
    return obj


def guard_model(P, m):
    """pack the model's weights now and move every one of them to guarded memory, before the first forward"""
    if hasattr(m, "_w"):
        if m._w is None:
            m._pack()
        m._w = guard_tree(P, m._w)
    for attr in ("_host", "packed"):            # (the pose networks and the metric networks: ``.to(cpu)`` of these is the tensor itself)
        if getattr(m, attr, None):
            setattr(m, attr, guard_tree(P, getattr(m, attr)))
    return m


def _emu_backend():
    from tests.conftest import Backend
    return Backend("emu", torch.device("cpu"))


def _wc():
    from tests import test_workspace_containment as W
    return W


def _schedule(family, name):
    def deco(fn):
        fn.__name__ = "case_" + name
        return case(family, sides=("end",))(fn)
    return deco


def _cond_inputs(name):
    """name -> (the inputs of the tiny model, fn(model, *guarded inputs) -> outputs): the shapes and seeds of ``_cond_stack_cases``"""
    r = lambda *shape, seed=4: rn(seed, *shape)                                                                  # noqa: E731
    if name == "prior":
        px, ppe, psp, ptp = r(2, 1, 1024, seed=8), r(2, 1, 1024, seed=9) * 0.5, r(2, 1, 36, seed=10).abs(), r(2, 1, 36, seed=11).abs()
        return (px, px * 0.5, ppe, psp, ptp), lambda m, a, b, pe, sp, tp: (m(a, 457, pe, sp, tp).predicted_image_embedding,
                                                                           m(b, 12, pe, sp, tp).predicted_image_embedding)
    x, fn = {"dinov2_swiglu": (r(2, 3, 28, 42, seed=5), lambda m, x: (lambda o: (o.last_hidden_state, o.pooler_output))(m(x))),
             "dinov2_gelu": (r(1, 3, 28, 28, seed=5), lambda m, x: (m(x).last_hidden_state,)),
             "clip_dh80": (r(2, 3, 28, 28, seed=12), lambda m, x: tuple(m(x, return_dict=False))),
             "clip_dh64": (r(2, 3, 28, 28, seed=12), lambda m, x: tuple(m(x, return_dict=False))),
             "pose_embedding": (r(1, 3, 16, 24, seed=2).tanh(), lambda m, x: (m(x),)),
             "image_proj_model_p": (r(1, 9, 128), lambda m, x: (m(x),)),
             "image_projection": (r(3, 64, seed=7), lambda m, x: (m(x),))}[name]
    return (x,), fn


def _cond_case(name, family):
    @_schedule(family, name)
    def fn(P):
        from tests.test_cond_stack_conformance import synth_sd
        build, seed, _ = _wc()._cond_stack_cases(_emu_backend())[name]        # (the model and its weights; the inputs are built and guarded here)
        m = build()
        m.load_state_dict(synth_sd(build(), seed=seed))
        guard_model(P, m.to("cpu"))
        inputs, call = _cond_inputs(name)
        return call(m, *[P(t) for t in inputs])
    return fn


for _i, _n in enumerate(("dinov2_swiglu", "dinov2_gelu", "clip_dh80", "clip_dh64", "prior", "pose_embedding", "image_proj_model_p", "image_projection")):
    _cond_case(_n, f"schedules_cond{_i % 2}")


@_schedule("schedules_vae", "vae_3x5")
def _vae(P):
    from oracle import vae as O
    from tests.test_vae_any_size import _build
    g = torch.Generator().manual_seed(20)
    x, z = torch.rand(1, 3, 24, 40, generator=g) * 2 - 1, torch.randn(1, 4, 3, 5, generator=g)
    _, m = _build(torch.device("cpu"), O.VAEConfig.tiny(), seed=7)
    guard_model(P, m)
    return (m.encode(P(x)).latent_dist.parameters, m.decode(P(z), return_dict=False)[0], m.decode_to_uint8(P(z)))


def _unet_case(name, fp8, ctx):
    @_schedule("schedules_unet", name)
    def fn(P):
        W = _wc()
        be = _emu_backend()
        B, h, w, L, n0, pose_b = 2, 7, 9, 5, 1, 1
        cfg = W._unet_config("two_level")
        m = guard_model(P, W._unet_model(be, cfg, fp8=fp8))
        inp = tuple(P(t) for t in W._unet_inputs(cfg, B, h, w, L, n0, pose_b))
        if not ctx:
            return W._python_schedule(be, m, inp, B, h, w, n0, False)[1:]
        x_in = ops.nchw_to_nhwc_bf16(inp[0], cpad=m._w["conv_in"].cin)
        uc = W.UNetContext(m)
        out = W._c_schedule(be, uc, x_in, inp, B, h, w, n0, False)
        # ... and the float-timestep forms on a guarded table, the step counter on its last row
        _, e, c, p = inp
        pb = uc.prepare_conditioning(B, h, w, e, c, p, zero_ctx_batches=n0, shared_cfg_input=False)
        ts = P(torch.tensor([801.0, 400.25, 1.0]), 4)
        uc.prepare_timesteps(ts, B, h, w)
        return out + (uc.forward(x_in, ts, P(torch.tensor([2], dtype=I32), 4), B, h, w, pb),)
    return fn


_unet_case("unet_python", False, False)
_unet_case("unet_python_fp8", True, False)
_unet_case("unet_context", False, True)


@_schedule("schedules_pose", "dwpose_r3_flip")
def _dwpose(P):
    W = _wc()
    est = guard_model(P, W._dw_estimator(32, 32, 133))
    img, boxes, index = W._dw_inputs(_emu_backend(), 3)
    return tuple(est(P(img, 1), P(boxes), P(index, 4), flip_test=True))


@_schedule("schedules_pose", "detector_s64")
def _detector(P):
    W = _wc()
    det = guard_model(P, W._detector(64))
    return tuple(det(P(W._det_images(_emu_backend(), 3, True), 1)))


@_schedule("schedules_pose", "lpips_31")
def _lpips(P):
    W = _wc()
    m = guard_model(P, W._lpips_model())
    a, b = W._lpips_images(_emu_backend(), 3, 1, "u8", 31, 31)
    return tuple(m(P(a, 1), P(b, 1), normalize=True, return_layers=True))


@_schedule("schedules_pose", "inception_35")
def _inception(P):
    from tests import test_fid as F
    W = _wc()
    m = guard_model(P, W._inception_model(64, False))
    return (m(P(F._dev(F._images(2, 35, 35, 11, "f32"), _emu_backend()))),)


SCHEDULE_FAMILIES = tuple(sorted({c.family for c in CASES.values() if c.family.startswith("schedules_")}))
KERNEL_FAMILIES = tuple(sorted({c.family for c in CASES.values() if not c.family.startswith(("schedules_", "bite_"))}))


# ================================================================================================ the instruments bite: the CPU children
def _bite(name):
    def deco(fn):
        fn.__name__ = "case_" + name
        return case("bite_" + name, sides=("end",))(fn)
    return deco


@_bite("memmove")
def _bite_memmove(P):
    """no library involved: 32 bytes copied from 16 bytes before the end of a guarded buffer"""
    src = P(Z(64, dtype=U8))
    dst = (C.c_char * 32)()
    C.memmove(dst, src.data_ptr() + 64 - 16, 32)


@_bite("f32_to_bf16")
def _bite_f32_to_bf16(P):
    n = 1024                                                   # 4096 bytes: the buffer ends exactly at the protected page
    x, y = P(rn(1, n)), P.out((n + 1,), BF16, 2)
    ok(lib().pcdm_f32_to_bf16(ptr(x), ptr(y), n + 1, None))


@_bite("gemm_short_a")
def _bite_gemm_short_a(P):
    """a linear GEMM whose A holds M - 1 rows"""
    c = _lin(70, 72, 64)
    c.extra["short_a"] = True
    _gemm(P, c, 0)


BITES = ("memmove", "f32_to_bf16", "gemm_short_a")


# ================================================================================================ the parent side
_LINE = re.compile(r"^(BEGIN|END) (\S+) (\S+)(?: guarded=(\d+) allocs=(\d+) gap=(\d+) seconds=([\d.]+) calls=(\S+))?$")


def _run_child(family, after=None):
    cmd = [sys.executable, "-m", "tests.operand_guard_child", family] + (["--after", after] if after else [])
    r = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=3000)
    done, open_ = {}, None
    for line in r.stdout.splitlines():
        m = _LINE.match(line.strip())
        if not m:
            continue
        if m.group(1) == "BEGIN":
            open_ = (m.group(2), m.group(3))
        else:
            assert open_ == (m.group(2), m.group(3)), (open_, line)
            done[open_] = dict(guarded=int(m.group(4)), allocations=int(m.group(5)), max_gap_bytes=int(m.group(6)), seconds=float(m.group(7)),
                               calls=[] if m.group(8) == "-" else m.group(8).split(","))
            open_ = None
    return r, done, open_


def _record_values(done):
    try:
        with open(Path(tempfile.gettempdir()) / "pcdm_operand_containment_values.lock", "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)                                   # (the CPU suite runs under pytest-xdist: one writer at a time)
            values = json.loads(VALUES.read_text()) if VALUES.exists() else {}
            for (name, side), v in done.items():
                values.setdefault(name, {})[side] = v
            VALUES.write_text(json.dumps(values, indent=1, sort_keys=True) + "\n")
    except OSError:
        pass                                                                   # a read-only checkout still runs the assertions


def _guard_family(family):
    """all cases of a family in one child; a child that dies is restarted behind the case it left open, so one finding does not hide the rest"""
    from tests.emu import build_emu
    build_emu.build()
    names = [n for n, c in CASES.items() if c.family == family]
    findings, after, seen = [], None, {}
    for _ in range(len(names) + 1):
        r, done, open_ = _run_child(family, after)
        seen.update(done)
        if r.returncode == 0 and open_ is None:
            break
        findings.append(f"{family}: the child ended with status {r.returncode} " + (f"in case '{open_[0]}', side '{open_[1]}'" if open_ else "outside any case")
                        + "\n" + r.stderr[-6000:])
        if open_ is None or open_[0] == names[-1]:
            break
        after = open_[0]
    _record_values(seen)
    assert not findings, "\n\n".join(findings)
    want = {(n, s) for n in names for s in CASES[n].sides}
    assert set(seen) == want, want - set(seen)
    assert all(v["guarded"] > 0 and v["max_gap_bytes"] <= 15 for v in seen.values())
    for (n, sd), v in seen.items():
        if family.startswith("schedules_"):
            assert v["allocations"] > 0, f"{n}: the allocation patch intercepted nothing"
            reached = [e for e, cases in NETWORK_CALLS.items() if n in cases]
        else:
            reached = CASES[n].exports
        assert set(reached) <= set(v["calls"]), f"{n}/{sd} declares entry points it does not call: {sorted(set(reached) - set(v['calls']))}"
    print(f"{family}: " + ", ".join(f"{n}/{s} {v['guarded']} operands + {v['allocations']} allocations guarded" for (n, s), v in sorted(seen.items())))


@pytest.mark.parametrize("family", KERNEL_FAMILIES)
def test_kernels_on_guard_pages(family):
    _guard_family(family)


@pytest.mark.parametrize("family", SCHEDULE_FAMILIES)
def test_schedules_on_guard_pages(family):
    _guard_family(family)


@pytest.mark.parametrize("name", BITES)
def test_guard_pages_bite(name):
    """each of these reads 16 bytes, one element or one row beyond a guarded operand: the child must die of SIGSEGV inside the case, and the
    parent must be able to name it"""
    from tests.emu import build_emu
    build_emu.build()
    r, done, open_ = _run_child("bite_" + name)
    assert r.returncode == -11, (r.returncode, r.stderr[-2000:])
    assert open_ == (name, "end") and not done, (open_, done)
    assert "Segmentation fault" in r.stderr and "test_operand_containment.py" in r.stderr, r.stderr[-2000:]     # faulthandler: the Python stack


def test_guarded_layout():
    """``guarded``: alignment, gap and contents on both sides, for sizes around the alignment and the page"""
    for side in ("end", "start"):
        for align in (1, 2, 4, 8, 16):
            for n in (1, 13, 16, 4095, 4096, 4097):
                t, gap = G.guarded_bytes(n, side, align)
                assert t.numel() == n and t.data_ptr() % align == 0 and 0 <= gap < align
                if side == "end":
                    assert (t.data_ptr() + n + gap) % G.PAGE == 0 and gap == -n % align
                else:
                    assert t.data_ptr() % G.PAGE == 0
                t.fill_(7)
                assert int(t.sum()) == 7 * n
    x = rn(1, 5, 13, dtype=BF16)
    P = G.GuardedPlace("end")
    xr = P.rows(x, 21, 2)
    assert torch.equal(xr, x) and xr.stride() == (21, 1) and P.max_gap == 0 and P.count == 1
    assert torch.equal(G.guarded(x, "start", 16), x)


# ================================================================================================ completeness
# Entry points without a device pointer: size / layout queries, host-only helpers, the red-zone hooks and the management calls of the UNet context.
EXEMPT = ("pcdm_version", "pcdm_is_emulator", "pcdm_pose_tables", "pcdm_detect_resized", "pcdm_set_workspace_redzone", "pcdm_get_workspace_redzone",
          "pcdm_unet_create", "pcdm_unet_destroy", "pcdm_unet_last_error", "pcdm_unet_set_weight", "pcdm_unet_set_vector", "pcdm_unet_set_tile",
          "pcdm_unet_set_attention_fp8", "pcdm_unet_set_freeu", "pcdm_unet_get_tile", "pcdm_unet_workspace_init", "pcdm_unet_prepare_conditioning",
          "pcdm_unet_prepare_timesteps", "pcdm_unet_prepare_timesteps_f32", "pcdm_unet_set_shared_cfg_input", "pcdm_unet_step_overflow",
          "pcdm_unet_time_table_bytes", "pcdm_unet_workspace_bytes")
# The whole-network calls: covered by the schedules (each name -> the schedule cases that run it).
NETWORK_CALLS = {"pcdm_unet_forward": ("unet_context",), "pcdm_unet_forward_f32": ("unet_context",), "pcdm_dwpose_forward": ("dwpose_r3_flip",),
                 "pcdm_detect_forward": ("detector_s64",), "pcdm_lpips": ("lpips_31",), "pcdm_inception_features": ("inception_35",)}


def test_every_export_is_in_the_table():
    covered = {e for c in CASES.values() for e in c.exports}
    assert covered <= set(_lib.EXPORTS), covered - set(_lib.EXPORTS)
    for name, cases in NETWORK_CALLS.items():
        assert all(c in CASES for c in cases), name
    missing = [e for e in _lib.EXPORTS if e not in covered and e not in NETWORK_CALLS and e not in EXEMPT
               and not e.endswith(("_ws_bytes", "_ws_floats", "_layout"))]
    assert not missing, f"entry points with a device pointer and no case in the table: {missing}"
    for e in EXEMPT:
        assert e in _lib.EXPORTS and e not in covered, e


# ================================================================================================ the GPU half: three fills around every operand
FILLS = (0x00, 0xFF, 0x3C)                                   # zeros, NaN in every float format, and a finite pattern
KERNEL_CASES = tuple(n for n, c in CASES.items() if c.family in KERNEL_FAMILIES and c.family != "host")   # (the packers are host code)


def _flat(o):
    if isinstance(o, torch.Tensor):
        return [o]
    if isinstance(o, dict):
        o = list(o.values())
    return [t for v in (o or ()) for t in _flat(v)] if isinstance(o, (list, tuple)) else []


def _bits_of(t):
    """the bytes of the tensor's elements (its view's, for a strided window), on the host"""
    t = t.detach()
    return t.contiguous().reshape(-1).view(U8).cpu() if t.numel() else t.reshape(-1).cpu()


def run_fills(name, device, fn=None):
    """the case with its operands inside larger buffers holding each of ``FILLS``: the outputs must be bit-identical"""
    got = {}
    for fill in FILLS:
        P = G.WindowPlace(device, fill)
        with G.GuardedAllocs(P):
            outs = _flat((fn or CASES[name].fn)(P))
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()
        assert P.count > 0 and outs, f"{name}: nothing was placed or returned: the case tests nothing"
        got[fill] = [_bits_of(t) for t in outs]
    for fill in FILLS[1:]:
        assert len(got[fill]) == len(got[FILLS[0]])
        for i, (a, b) in enumerate(zip(got[FILLS[0]], got[fill])):
            assert a.shape == b.shape and torch.equal(a, b), (
                f"{name}: output {i} differs between the surroundings 0x00 and {fill:#04x} ({int((a != b).sum())} bytes, first at byte "
                f"{int((a != b).nonzero()[0])}): memory outside an operand reaches the result")


@pytest.mark.gpu
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_fills_gpu(gpu_backend, monkeypatch, name):
    monkeypatch.setattr(ops, "AUTOTUNE", False)               # (explicit tiles, or the library's heuristic: no tuning launches on windowed operands)
    run_fills(name, gpu_backend.device)


def _overread_by_one(P):
    n = 1000
    x, y = P(rn(1, n)), P.out((n + 1,), BF16, 2)
    ok(lib().pcdm_f32_to_bf16(ptr(x), ptr(y), n + 1, stream(P)))
    return [y]


@pytest.mark.gpu
def test_fills_bite_gpu(gpu_backend):
    """``pcdm_f32_to_bf16`` told to convert one element more than x holds: the element behind x is the surroundings' byte pattern"""
    with pytest.raises(AssertionError, match=r"overread: output 0 differs between the surroundings 0x00 and 0xff \(2 bytes, first at byte 2000\)"):
        run_fills("overread", gpu_backend.device, _overread_by_one)


def test_fills_bite_host():
    """the same on host memory with the emulator build (the comparison itself, without a GPU)"""
    from tests.emu import build_emu
    _lib.use_library(build_emu.load())
    with pytest.raises(AssertionError, match=r"overread: output 0 differs between the surroundings 0x00 and 0xff \(2 bytes, first at byte 2000\)"):
        run_fills("overread", "cpu", _overread_by_one)
    run_fills("layout", "cpu")


# ================================================================================================ wrapper extents (host only)
class _Stub:
    """stands in for the library: records the calls and answers 0 to every one; nothing can launch"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("pcdm_"):
            raise AttributeError(name)

        def f(*a):
            if not name.endswith(("_ws_floats", "_ws_bytes")):                 # (size queries take no pointer)
                self.calls.append(name)
            return 0
        return f


@pytest.fixture
def stub(monkeypatch):
    st = _Stub()
    monkeypatch.setattr(_lib, "_lib", st)
    monkeypatch.setattr(_lib, "_is_emu", True)
    return st


def _z(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


# name -> (call(**operands), operands); every operand is a tensor the wrapper hands to the library as a pointer
def _wrapper_calls():
    n, I = 6, I32
    return {
        "cfg_step": (lambda eps, x, noise, x_prev, eps_out, coef, step, err: ops.cfg_step(eps, True, 2.0, x, x_prev, coef, step, noise=noise, eps_out=eps_out,
                                                                                          step_error=err),
                     dict(eps=_z(2 * n), x=_z(n), noise=_z(n), x_prev=_z(n), eps_out=_z(n), coef=_z(3, 4), step=_z(2, dtype=I), err=_z(2, dtype=I))),
        "small_linear": (lambda x, w, bias, add, out: ops.small_linear(x, w, bias, out, add=add),
                         dict(x=_z(3, 8), w=_z(5, 8, dtype=BF16), bias=_z(5), add=_z(3, 5), out=_z(3, 5))),
        "nhwc_bf16_to_nchw": (lambda x: ops.nhwc_bf16_to_nchw(x, 2, 8, 3, 5), dict(x=_z(2, 15, 8, dtype=BF16))),
        "nchw_to_nhwc_bf16": (lambda out: ops.nchw_to_nhwc_bf16(_z(2, 3, 3, 5), out), dict(out=_z(2, 3, 5, 8, dtype=BF16))),   # (x is converted)
        "f32_to_bf16": (lambda x, out: ops.f32_to_bf16(x, out), dict(x=_z(n), out=_z(n, dtype=BF16))),
        "timestep_embedding": (lambda t, step, out, err: ops.timestep_embedding(t, step, out, step_error=err),
                               dict(t=_z(3, dtype=I64), step=_z(2, dtype=I), out=_z(2, 64), err=_z(2, dtype=I))),
        "timestep_embedding_rows": (lambda t, out: ops.timestep_embedding_rows(t, out), dict(t=_z(3, dtype=I64), out=_z(3, 64))),
        "time_class_combine": (lambda e, c, out: ops.time_class_combine(e, c, out, 2), dict(e=_z(3, 8), c=_z(2, 8), out=_z(6, 8, dtype=BF16))),
        "advance_step": (lambda step: ops.advance_step(step), dict(step=_z(2, dtype=I))),
        "pixel_shuffle2": (lambda x, out: ops.pixel_shuffle2(x, out, 2, 3, 5, 8), dict(x=_z(30, 32, dtype=BF16), out=_z(120, 8, dtype=BF16))),
        "gaussian_sample": (lambda m, noise, out: ops.gaussian_sample(m, noise, out), dict(m=_z(2, 8, 3, 5), noise=_z(2, 4, 3, 5), out=_z(2, 4, 3, 5))),
        "image_to_uint8": (lambda x, out: ops.image_to_uint8(x, out), dict(x=_z(2, 4, 3, 5), out=_z(2, 3, 5, 3, dtype=U8))),
        "layernorm": (lambda x, g, b, out: ops.layernorm(x, g, b, 1e-5, out), dict(x=_z(3, 72, dtype=BF16), g=_z(72), b=_z(72), out=_z(3, 72, dtype=BF16))),
        "groupnorm": (lambda x1, x2, g, b, out: ops.groupnorm(x1, x2, 2, 5, 8, 1e-5, g, b, True, out, _z(8)),   # (ws: sized by a query the stub answers 0)
                      dict(x1=_z(10, 32, dtype=BF16), x2=_z(10, 32, dtype=BF16), g=_z(64), b=_z(64), out=_z(10, 64, dtype=BF16))),
        "unipc_step": (lambda eps, x, m1, m2, last, coef, step, err: ops.unipc_step(eps, True, 2.0, x, m1, m2, last, coef, step, err),
                       dict(eps=_z(2 * n), x=_z(n), m1=_z(n), m2=_z(n), last=_z(n), coef=_z(3, 12), step=_z(2, dtype=I), err=_z(2, dtype=I))),
        "dpmpp_step": (lambda eps, x, m1, noise, coef, step, err: ops.dpmpp_step(eps, True, 2.0, x, m1, noise, coef, step, err),
                       dict(eps=_z(2 * n), x=_z(n), m1=_z(n), noise=_z(3, n), coef=_z(3, 8), step=_z(2, dtype=I), err=_z(2, dtype=I))),
        "multistep_step": (lambda eps, x, xs, h1, h2, h3, noise, coef, step, err: ops.multistep_step(eps, True, 2.0, x, xs, h1, h2, h3, noise, coef, step, err),
                           dict(eps=_z(2 * n), x=_z(n), xs=_z(n), h1=_z(n), h2=_z(n), h3=_z(n), noise=_z(3, n), coef=_z(3, 12), step=_z(2, dtype=I),
                                err=_z(2, dtype=I))),
        "unclip_step": (lambda pred, x, noise, out: ops.unclip_step(pred, True, 2.0, x, noise, out, (1.0,) * 8),
                        dict(pred=_z(2 * n), x=_z(n), noise=_z(n), out=_z(n))),
        "unclip_step_dev": (lambda pred, x, noise, coef, step, err: ops.unclip_step_dev(pred, True, 2.0, x, noise, coef, step, err),
                            dict(pred=_z(2 * n), x=_z(n), noise=_z(3, n), coef=_z(3, 8), step=_z(2, dtype=I), err=_z(2, dtype=I))),
        "assemble_input": (lambda lat, mask, masked, out: ops.assemble_input(lat, 2, mask, masked, out),
                           dict(lat=_z(2, 4, 3, 5), mask=_z(4, 1, 3, 5), masked=_z(4, 4, 3, 5), out=_z(4, 3, 5, 16, dtype=BF16))),
        "assemble_input_ex": (lambda lat, mask, masked, out, tab, step, err: ops.assemble_input_ex(lat, 2, mask, masked, out, tab, 7, step, err),
                              dict(lat=_z(2, 4, 3, 5), mask=_z(1, 1, 3, 5), masked=_z(1, 4, 3, 5), out=_z(4, 3, 5, 16, dtype=BF16), tab=_z(3, 12),
                                   step=_z(2, dtype=I), err=_z(2, dtype=I))),
        "quantize_fp8": (lambda out: ops.quantize_fp8(_z(5, 16, dtype=BF16), out, cols=13), dict(out=_z(5, 16, dtype=U8))),   # (x: any row stride)
        "quantize_fp8_x": (lambda x: ops.quantize_fp8(x, _z(5, 16, dtype=U8), cols=16), dict(x=_z(5, 16, dtype=BF16))),
        "freeu": (lambda hid, ho, skip, so: ops.freeu(hid, skip, so, 1, 19, 19, 1.25, 0.5, hidden_out=ho, ws=_z(4096, dtype=U8)),   # (ws: sized by a query
                  dict(hid=_z(361, 16, dtype=BF16), ho=_z(361, 16, dtype=BF16), skip=_z(361, 8, dtype=BF16), so=_z(361, 8, dtype=BF16))),  # the stub answers 0)
        "fid_accumulate": (lambda feat, tot, gram: ops.fid_accumulate(feat, tot, gram), dict(feat=_z(3, 5), tot=_z(5, dtype=F64), gram=_z(5, 5, dtype=F64))),
        "fid_finalize": (lambda tot, gram: ops.fid_finalize(tot, gram, 3), dict(tot=_z(5, dtype=F64), gram=_z(5, 5, dtype=F64))),
        "lincomb": (lambda out, a, b: ops.lincomb(out, [a, b], (1.0, 2.0)), dict(out=_z(n), a=_z(n), b=_z(n))),
        "rescale_noise_cfg": (lambda a, b, out: ops.rescale_noise_cfg(a, b, out, 0.7), dict(a=_z(2, n), b=_z(2, n), out=_z(2, n))),
    }


# operands that are tables or scalars-on-the-device, read at a row the device chooses: more rows than needed is fine, so "one element short" of
# the tensor above still holds what the call needs -- they are driven down to nothing instead
_TABLES = {"step", "err", "coef", "t", "tab"}
_OTHER = {F32: F64, F64: F32, BF16: torch.float16, I32: I64, I64: I32, U8: torch.int8}


def _spoiled(t, name, kind):
    if kind == "short":
        return t.reshape(-1)[:0] if name in _TABLES else t.reshape(-1)[:-1]
    if kind == "dtype":
        return t.to(_OTHER[t.dtype])
    wide = torch.zeros(*t.shape[:-1], t.shape[-1] * 2, dtype=t.dtype)[..., ::2]
    assert wide.shape == t.shape and not wide.is_contiguous()
    return wide


WRAPPERS = tuple(_wrapper_calls())


@pytest.mark.parametrize("name", WRAPPERS)
def test_wrapper_refuses_before_the_library_is_called(stub, name):
    call, operands = _wrapper_calls()[name]
    call(**operands)
    assert stub.calls, "the well-formed call does not reach the library: the case tests nothing"
    for key in operands:
        for kind in ("short", "dtype", "strided"):
            del stub.calls[:]
            bad = dict(operands, **{key: _spoiled(operands[key], key, kind)})
            with pytest.raises((AssertionError, ValueError, RuntimeError, TypeError, IndexError)):
                call(**bad)
            assert not stub.calls, f"ops.{name}: operand '{key}' ({kind}) reached the library ({stub.calls})"


@pytest.mark.parametrize("name", ("cfg_step", "unipc_step", "dpmpp_step", "unclip_step_dev"))
def test_wrapper_refuses_a_step_table_of_another_shape(stub, name):
    """the row count the library bounds the counter with is ``coef.shape[0]``: a 1-D coef (no row count), a coef of another row width, a coef one
    row short of noise_all and a step_error of the wrong dtype are refused before the library is called"""
    call, operands = _wrapper_calls()[name]
    call(**operands)
    assert stub.calls
    coef = operands["coef"]
    bad = [("a 1-D coef", dict(coef=coef.reshape(-1))), ("a coef of another row width", dict(coef=_z(3, coef.shape[1] + 4))),
           ("a step_error of the wrong dtype", dict(err=_z(2, dtype=I64))), ("a float step_error", dict(err=_z(2)))]
    if "noise" in operands and operands["noise"].dim() == 2:
        bad.append(("coef one row short of noise_all", dict(coef=coef[:-1].contiguous())))
        bad.append(("noise_all one row short of coef", dict(noise=operands["noise"][:-1].contiguous())))
        bad.append(("a flat noise_all", dict(noise=operands["noise"].reshape(-1))))
    for what, change in bad:
        del stub.calls[:]
        with pytest.raises(AssertionError):
            call(**dict(operands, **change))
        assert not stub.calls, f"ops.{name}: {what} reached the library"


def test_wrapper_check_removed_reaches_the_stub(stub, monkeypatch):
    """the instrument bites: with the operand check taken out of ``ops`` a short ``bias`` reaches the library, and the test above would say so"""
    call, operands = _wrapper_calls()["small_linear"]
    bad = dict(operands, bias=operands["bias"][:-1])
    with pytest.raises(AssertionError):
        call(**bad)
    assert not stub.calls
    monkeypatch.setattr(ops, "_cn", lambda t, *a: t)
    call(**bad)
    assert stub.calls == ["pcdm_small_linear"]



def test_workspaces_sized_by_a_query_are_checked():
    """``groupnorm`` and ``freeu`` size their workspace by a query the stub answers 0: with the emulator build's answer a workspace one element
    short is refused before anything is launched (the output keeps its bytes)"""
    from tests.emu import build_emu
    _lib.use_library(build_emu.load())
    B, H, W, C1, C2 = 1, 19, 19, 16, 8
    need = ops.freeu_ws_bytes(B, H, W, C1, C2)
    assert need > 0
    hid, skip, so = _z(361, C1, dtype=BF16), _z(361, C2, dtype=BF16), torch.full((361, C2), 3.0, dtype=BF16)
    for ws in (None, _z(need - 1, dtype=U8), _z(2 * need, dtype=U8)[::2]):
        with pytest.raises(AssertionError):
            ops.freeu(hid, skip, so, B, H, W, 1.25, 0.5, ws=ws)
    n = lib().pcdm_groupnorm_ws_floats(2, 64)
    out = torch.full((10, 64), 3.0, dtype=BF16)
    for ws in (_z(n - 1), _z(n, dtype=F64)):
        with pytest.raises(AssertionError):
            ops.groupnorm(_z(10, 64, dtype=BF16), None, 2, 5, 8, 1e-5, _z(64), _z(64), True, out, ws)
    assert bool((so == 3.0).all()) and bool((out == 3.0).all())


# ---- which wrappers the stub test drives
# ``ops`` wrappers that the case table calls (directly, or through pcdms_amd.preprocess / pcdms_amd.pose) but the stub test above does NOT drive yet:
# their operand checks are whatever the wrapper has today and are not under test.  README.md and DESIGN.md carry the same list.
NOT_DRIVEN = ("absdiff", "avgpool3_f32", "conv2d_f32", "conv2d_f32_act", "conv2d_f32_ex", "detect_decode", "detect_prep", "dwconv5_silu_f32",
              "fc_hsigmoid_f32", "flash_attn", "flash_attn_fp8", "gau_core_f32", "global_avgpool_f32", "groupnorm_cluster_timeouts", "inception_input",
              "maxpool3s2_f32", "maxpool3s2_f32_ex", "maxpool5_f32", "nms_f32", "pose_crop", "pose_draw", "psnr", "resample_u8", "resize_cubic_f32",
              "resize_linear_u8", "scalenorm_f32", "select_image", "simcc_decode", "softmax_rows", "ssim", "ssim_box", "u8_to_nchw",
              "upsample2_nearest_f32")
_NO_POINTER = ("freeu_ws_bytes", "metrics_ws_bytes", "ssim_box_ws_bytes", "pack_lpips_conv", "row_stats_reference")   # size queries, host code


def test_driven_and_undriven_wrappers_are_all_the_table_uses():
    """the wrappers the table's cases call = the ones the stub test drives + ``NOT_DRIVEN``, so neither list can drift from the table"""
    import inspect
    src = "".join(inspect.getsource(c.fn) for c in CASES.values()) + inspect.getsource(_attn) + inspect.getsource(_groupnorm) + inspect.getsource(_pw) \
        + inspect.getsource(_metric_ws)
    used = set(re.findall(r"\bops\.([a-z_0-9]+)\(", src)) - set(_NO_POINTER)
    used |= {"resample_u8", "resize_cubic_f32", "pose_draw"}                  # behind preprocess.resize / resize_cv_cubic and pose.draw_pose
    driven = {n[:-2] if n.endswith("_x") else n for n in WRAPPERS}
    assert driven.isdisjoint(NOT_DRIVEN)
    assert used - driven == set(NOT_DRIVEN), (sorted(used - driven - set(NOT_DRIVEN)), sorted(set(NOT_DRIVEN) - (used - driven)))
