"""Conformance of ``pcdm_gemm``: every tile configuration x every feature, and every tuning-table entry, against fp64.

``test_tile_feature_matrix`` runs each tile id of ``ops.TILE_SHAPES`` through every feature case of ``FEATURES`` (epilogues, operands and flags,
the convolution forms, the folded LayerNorm, the row-statistics producer):

* the return code must match ``expect_accept``, a predicate written from the rules of include/pcdm.h and the ``return -1`` lines of gemm.hip /
  ``launch_gemm`` / gemm_ext.hip / rowgemm.hip -- a tile that starts or stops taking a feature fails here, naming both;
* an accepted call must match an fp64 reference computed from the bf16-rounded operands, within the bf16 rounding of the result plus a
  K-scaled accumulation term, and must NOT match the same reference with one output channel perturbed (the tolerance bites);
* nothing outside the output is written: every output (``out``, ``out2`` of SPLIT_VT, the fp32 NCHW tensor, the row-statistics partials) is a
  window of a wider sentinel-filled buffer -- the columns N..Npad included -- and the split-K workspace is sentinel-filled before the launch
  (it must not be read as output) and guarded behind ``ws_floats``;
* on the GPU every accepted call runs twice and must be bit-identical (races the lane emulator cannot show).

``test_tuning_table_entries`` decodes every key of pcdms_amd/tuning/gfx950.json and runs the entry's (tile, split_k, mode) on a proxy problem
that keeps every property the acceptance rules read (emulator), or at the key's own Npad / K / flags with M cut to two M tiles + a tail (GPU).
"""
from __future__ import annotations

import ctypes as C
import functools
import json
import math
import zlib
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional

import pytest
import torch
import torch.nn.functional as F

from pcdms_amd import _lib, ops
from pcdms_amd._lib import GemmParams

BF16 = torch.bfloat16
STORE, GEGLU, SPLIT_VT, NCHW = ops.EPI_STORE, ops.EPI_GEGLU, ops.EPI_SPLIT_VT, ops.EPI_NCHW_F32
SENT16 = 0x7FA5                 # a bf16 NaN pattern no kernel produces from finite operands
SENT32 = 0x7FA5A5A5             # its fp32 twin
GUARD = 64                      # elements of sentinel in front of and behind every flat output / workspace

# gemm.hip dispatch_tile / rowgemm.hip: id -> (BM, BN, waves along M, waves along N, fragment size)
TILE_CFG = {1: (256, 128, 4, 2, 32), 2: (64, 64, 2, 2, 32), 3: (256, 64, 4, 2, 32), 4: (128, 128, 2, 2, 32), 5: (128, 64, 2, 2, 32),
            6: (256, 64, 4, 2, 32), 7: (128, 128, 2, 2, 32), 8: (64, 64, 2, 2, 32), 9: (256, 128, 4, 2, 32), 10: (128, 64, 2, 2, 32),
            11: (256, 128, 4, 2, 32), 12: (256, 64, 4, 2, 32), 13: (256, 64, 4, 1, 32), 14: (256, 64, 4, 1, 32), 15: (128, 64, 2, 1, 32),
            16: (512, 64, 8, 1, 32), 17: (256, 256, 2, 4, 32), 18: (128, 128, 4, 2, 32), 21: (192, 320, 2, 4, 16), 22: (176, 320, 2, 4, 16),
            23: (176, 256, 2, 4, 16), 26: (192, 256, 2, 4, 16),
            31: (192, 128, 4, 2, 16), 32: (192, 64, 4, 2, 16), 33: (96, 128, 2, 4, 16), 34: (192, 64, 4, 1, 16), 35: (128, 64, 4, 1, 16),
            36: (64, 64, 4, 1, 16)}
ROWGEMM = (31, 32, 33, 34, 35, 36)
NEEDS128 = (1, 4, 7, 9, 11, 18)                 # gemm.hip: tiles that need Npad (and tap_group_n) % 128 == 0
LN_TILES = (2, 4, 7, 8, 17, 18, 26)             # gemm_ext.hip EXT 1 / 2: folded-LayerNorm consumers
LN_PARTIALS_ONLY = (23,)                        # ... EXT 2 only (producer partials)
STATS_TILES = (2, 4, 5, 6, 7, 8, 10, 18)        # gemm_ext.hip EXT 3: row-statistics producers
ROWGEMM_K = 320


def test_tile_tables_agree_with_ops():
    assert set(TILE_CFG) == set(ops.TILE_SHAPES)
    for t, (bm, bn, *_r) in TILE_CFG.items():
        assert ops.TILE_SHAPES[t] == (bm, bn), t
    assert tuple(ROWGEMM) == tuple(ops.ROWGEMM_TILES)
    assert set(LN_TILES) == set(ops.LN_TILED_TILES) and set(LN_PARTIALS_ONLY) == set(ops.LN_PARTIALS_TILES)
    assert set(STATS_TILES) == set(ops.STATS_TILES)


# ------------------------------------------------------------------------------------------------ problem description
@dataclass
class Case:
    name: str
    M: int
    N: int
    K: int
    Npad: int
    a: torch.Tensor                       # bf16: [M, lda] (linear; the first c1 columns are read) or NHWC [B, Hi, Wi, cin]
    w: torch.Tensor                       # bf16 [Npad, K] (rows >= N zero; GEGLU: interleaved [32 h | 32 gate] per 64)
    bias: Optional[torch.Tensor] = None   # fp32 [Npad]
    a2: Optional[torch.Tensor] = None     # bf16 [M, lda2]: second linear source (columns c1..K) or the first 1x1 source of the conv extra K
    a3: Optional[torch.Tensor] = None
    c1: int = 0
    conv: Optional[dict] = None           # B, Hi, Wi, Ho, Wo, stride, upsample, cin
    rowvec: Optional[torch.Tensor] = None  # fp32 [nb, N]
    rpb: int = 0
    residual: Optional[torch.Tensor] = None  # bf16 [rows, N]
    res_mod: int = 0
    epi: int = STORE
    vt_col0: int = 0
    act: int = 0
    zero_rows: int = 0
    split_k: int = 1
    dup_rows: int = 0
    tap_lut: int = 0
    tap_group_n: int = 0
    ln: bool = False                      # the weights carry a folded LayerNorm: w, bias are W diag(gamma), b + W beta
    ln_mode: int = 0                      # 1: statistics in the K loop; 2: from ln_row_stats
    row_stats_out: bool = False
    ln_eps: float = 1e-5
    extra: dict = field(default_factory=dict)

    @property
    def out_rows(self) -> int:
        return self.M + self.dup_rows

    @property
    def out_cols(self) -> int:
        return self.vt_col0 if self.epi == SPLIT_VT else self.N

    @property
    def L(self) -> int:
        return self.rpb or self.M


def _ldo(c: Case) -> int:
    """the row pitch of ``out``: wider than the row (a window of a wider buffer)"""
    return c.extra.get("ldo", (c.out_cols + 7) // 8 * 8 + 16)


_DEV = torch.device("cpu")     # where operands are drawn and the fp64 reference runs (the GPU table test: the device, see _run_table)


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device=_DEV).manual_seed(seed), device=_DEV)


def _rnd(shape, seed, scale=1.0, offset=0.0):
    return (_randn(shape, seed) * scale + offset).to(BF16)


def _pack_rows(w_n_k: torch.Tensor, Npad: int) -> torch.Tensor:
    N, K = w_n_k.shape
    wp = torch.zeros(Npad, K, dtype=BF16, device=w_n_k.device)
    wp[:N] = w_n_k.to(BF16)
    return wp


def _vec(n: int, Npad: int, seed: int, scale: float = 1.0) -> torch.Tensor:
    v = torch.zeros(Npad, device=_DEV)
    v[:n] = _randn((n,), seed) * scale
    return v


# ------------------------------------------------------------------------------------------------ the expected-accept predicate
def expect_accept(t: int, c: Case) -> bool:
    """Whether ``pcdm_gemm`` takes this call on tile ``t`` -- the library's documented rules, restated (include/pcdm.h; gemm.hip pcdm_gemm,
    launch_gemm in gemm_kernel.inc, gemm_ext.hip dispatch_ext, rowgemm.hip launch_rowgemm / launch_rg)."""
    BM, BN, WGM, WGN, F_ = TILE_CFG[t]
    M, N, K, Npad = c.M, c.N, c.K, c.Npad
    ldo = _ldo(c)
    # ---- pcdm_gemm, before any tile is looked at
    if N % 4 or Npad % 64 or Npad < N or K % 64:
        return False
    if c.dup_rows and (not c.conv or c.epi != STORE or c.act or c.split_k > 1 or N % 8 or ldo % 8):
        return False
    if c.dup_rows and c.rowvec is not None and (c.rpb < 32 or c.dup_rows % c.rpb):
        return False
    if c.zero_rows and c.conv:
        return False
    if c.act == ops.ACT_GELU and c.epi == GEGLU:
        return False
    if c.split_k > 1 and (c.epi != STORE or c.split_k > K // 64):
        return False
    if c.conv and c.tap_group_n:
        ntaps = K // c.conv["cin"]
        if not 1 <= ntaps <= 4 or N % c.tap_group_n or N // c.tap_group_n > 4 or c.tap_group_n % 64:
            return False
        for g in range(N // c.tap_group_n):
            grp = (c.tap_lut >> (16 * g)) & ((1 << (4 * ntaps)) - 1)     # only the nibbles of the ntaps taps are read (pcdm.h)
            if any(((grp >> (4 * i)) & 15) > 8 for i in range(ntaps)) or (grp == 0 and ntaps == 4):
                return False
    if c.epi == GEGLU and (c.bias is None or Npad % 128 or 2 * N > Npad):
        return False
    if c.epi == SPLIT_VT and c.vt_col0 % 4:
        return False
    # ---- the A-in-registers kernel (tiles 31..36)
    if t in ROWGEMM:
        WNC = BN // WGN
        if c.row_stats_out or c.conv or K != ROWGEMM_K or c.a2 is not None or c.split_k > 1 or c.rowvec is not None:
            return False
        if c.act and c.epi != GEGLU:
            return False
        if c.epi not in (STORE, GEGLU, SPLIT_VT) or ldo % 8 or N % 8:
            return False
        if c.residual is not None and (c.res_mod or M) < M:
            return False
        if c.epi == GEGLU and c.residual is not None:
            return False
        if c.ln and c.zero_rows:
            return False
        if Npad % BN or Npad > 2560 or (c.epi == GEGLU and WNC != 64):
            return False
        if c.epi == SPLIT_VT and (c.vt_col0 % WNC or c.L % 16 or M % 16):
            return False
        return True                                   # (ln_row_stats is not read: the kernel holds the whole rows and takes their statistics)
    uneven = (BM // F_) % WGM != 0
    WN = BN // WGN
    tgn = c.tap_group_n
    # ---- folded LayerNorm on the tiled kernel (gemm_ext.hip EXT 1 / 2)
    if c.ln:
        if c.conv or c.a2 is not None or c.split_k > 1 or c.rowvec is not None or c.residual is not None or c.act or c.zero_rows or N % 8 or ldo % 8:
            return False
        if c.row_stats_out or c.epi not in (STORE, GEGLU, SPLIT_VT):
            return False
        if c.epi == SPLIT_VT and (c.vt_col0 % 64 or c.L % 32 or M % 32):
            return False
        if c.epi == GEGLU and t in (2, 8):
            return False
        if (t in (4, 7, 18) and Npad % 128) or (t in (17, 26, 23) and Npad % 256):
            return False
        if c.ln_mode == 2 and K > 1280:
            return False
        if t not in LN_TILES and not (t in LN_PARTIALS_ONLY and c.ln_mode == 2):
            return False
        return Npad % BN == 0 and not (c.epi == GEGLU and WN != 64) and not (uneven and c.epi == SPLIT_VT)
    # ---- row-statistics producer (gemm_ext.hip EXT 3)
    if c.row_stats_out:
        if c.conv or c.split_k > 1 or c.act or c.dup_rows or c.epi != STORE or N % 32 or ldo % 8:
            return False
        if c.residual is not None and (c.res_mod or M) < M:
            return False
        if c.rowvec is not None and c.rpb < 32:
            return False
        if t in (4, 7, 18) and Npad % 128:
            return False
        return t in STATS_TILES and Npad % BN == 0
    # ---- the plain tiled kernel (dispatch_tile + launch_gemm)
    n128 = Npad % 128 == 0 and (tgn == 0 or tgn % 128 == 0)
    if c.epi == GEGLU and t not in NEEDS128 and t < 13:
        return False
    if (t in NEEDS128 and not n128) or (t == 17 and Npad % 256):
        return False
    if Npad % BN or (tgn and tgn % BN):
        return False
    if c.epi == GEGLU and WN != 64:
        return False
    if uneven and c.epi == SPLIT_VT:
        return False
    return True


# ------------------------------------------------------------------------------------------------ the feature cases
def _npad_for(t: int) -> int:
    """the Npad a tile runs the feature cases at: two or more N tiles of its width, a multiple of 128 (GEGLU)"""
    return {64: 256, 128: 256, 256: 512, 320: 640}[TILE_CFG[t][1]]


FEATURES = ["store", "store_n8", "rowvec", "residual", "residual_bcast", "act_silu", "act_gelu", "geglu", "split_vt32", "split_vt_ragged",
            "nchw", "two_source", "zero_rows", "split_k2", "split_k_odd", "conv_s1", "conv_s2", "conv_up", "conv_dup_rows", "conv_extra_a2",
            "conv_extra_a2_a3", "conv_taps4", "conv_taps1", "ln1_store", "ln1_geglu", "ln1_split_vt", "ln2_store", "ln2_geglu",
            "ln2_split_vt", "row_stats"]
SPLIT_ODD = {"emu": 3, "gpu": 7}


def _conv_geom(kind: str, big: bool) -> dict:
    if kind == "s1":
        B, Hi, Wi = (2, 7, 9) if not big else (2, 17, 23)
        return dict(B=B, Hi=Hi, Wi=Wi, Ho=Hi, Wo=Wi, stride=1, upsample=0)
    if kind == "s2":
        B, Hi, Wi = (2, 9, 11) if not big else (2, 33, 45)
        return dict(B=B, Hi=Hi, Wi=Wi, Ho=(Hi - 1) // 2 + 1, Wo=(Wi - 1) // 2 + 1, stride=2, upsample=0)
    B, Hi, Wi = (2, 4, 5) if not big else (2, 9, 11)
    return dict(B=B, Hi=Hi, Wi=Wi, Ho=2 * Hi, Wo=2 * Wi, stride=1, upsample=1)


@functools.lru_cache(maxsize=None)
def build_case(feat: str, Npad: int, K: int, big: bool) -> Case:
    """The CPU-side operands of one feature case at one Npad (the reference is computed once per case and shared by the tiles that run it)."""
    s = zlib.crc32(f"{feat},{Npad},{K},{big}".encode()) % 1000
    M = 150 if not big else 3 * 256 + 37
    N = Npad - 4 if feat == "store" else Npad - 8
    ldo = N + 24 if N % 8 == 0 else N + 12
    base = dict(name=feat, extra=dict(ldo=ldo))
    if feat.startswith("conv"):
        cin = 64 if not big else 128
        geo = _conv_geom({"conv_s2": "s2", "conv_up": "up"}.get(feat, "s1"), big)
        M = geo["B"] * geo["Ho"] * geo["Wo"]
        x = _rnd((geo["B"], geo["Hi"], geo["Wi"], cin), s + 1)
        if feat in ("conv_taps4", "conv_taps1"):
            ntaps = 4 if feat == "conv_taps4" else 1
            tgn = Npad // 2
            if ntaps == 4:       # two phases of the Upsample2D decomposition, with stale high bits above group 1 (never read)
                lut = (ops.UPSAMPLE_TAP_LUT & 0xFFFF) | (((ops.UPSAMPLE_TAP_LUT >> 48) & 0xFFFF) << 16) | (0xABCD << 32)
            else:                # group 0 uses tap 0 only (a group table of 0), group 1 tap 8 with stale nibbles above it
                lut = 0 | (0xFFF8 << 16)
            K_ = ntaps * cin
            w = _pack_rows(torch.randn(Npad, K_, generator=torch.Generator().manual_seed(s + 2)) / math.sqrt(K_), Npad)
            return Case(**base, M=M, N=Npad, K=K_, Npad=Npad, a=x, w=w, bias=_vec(Npad, Npad, s + 3),
                        conv=dict(geo, cin=cin), tap_lut=lut, tap_group_n=tgn)
        cx = {"conv_extra_a2": 64, "conv_extra_a2_a3": 128}.get(feat, 0)
        K_ = 9 * cin + cx
        w = _pack_rows(torch.randn(N, K_, generator=torch.Generator().manual_seed(s + 2)) / math.sqrt(K_), Npad)
        c = Case(**base, M=M, N=N, K=K_, Npad=Npad, a=x, w=w, bias=_vec(N, Npad, s + 3), conv=dict(geo, cin=cin))
        if cx:
            c.a2 = _rnd((M, 64 + 8), s + 4)[:, :64]                # a pitch wider than the channels
            c.c1 = 64
            if cx > 64:
                c.a3 = _rnd((M, 64 + 16), s + 5)[:, :64]
        if feat == "conv_dup_rows":
            c.rpb = geo["Ho"] * geo["Wo"]
            c.dup_rows = M
            c.rowvec = torch.randn(2 * geo["B"], N, generator=torch.Generator().manual_seed(s + 6))
            c.residual = _rnd((2 * M, N), s + 7)
            c.res_mod = 0
        if feat == "conv_s1":
            c.residual = _rnd((M, N), s + 7)
        return c
    lnf = feat.startswith("ln")
    if feat in ("split_vt32", "ln1_split_vt", "ln2_split_vt"):
        B, L = (2, 64) if not big else (3, 256)
        M = B * L
    elif feat == "split_vt_ragged":
        B, L = (3, 37) if not big else (3, 277)
        M = B * L
    elif feat == "nchw":
        B, L = (2, 75) if not big else (3, 267)
        M = B * L
    a = _rnd((M, K + 8), s + 1, offset=0.7 if lnf else 0.0)[:, :K]   # (a row pitch wider than K; a LayerNorm input with a mean)
    w = torch.randn(Npad, K, generator=torch.Generator().manual_seed(s + 2)) / math.sqrt(K)
    c = Case(**base, M=M, N=N, K=K, Npad=Npad, a=a, w=_pack_rows(w[:N], Npad), bias=_vec(N, Npad, s + 3))
    if feat == "rowvec":
        c.rpb = M // 3 if M % 3 == 0 else M
        c.rowvec = torch.randn(M // c.rpb, N, generator=torch.Generator().manual_seed(s + 4))
    if feat in ("residual", "zero_rows", "split_k2", "split_k_odd", "split_k12", "row_stats"):
        c.residual = _rnd((M, N + 16), s + 5)[:, :N]
        c.res_mod = M
    if feat == "residual_bcast":
        c.res_mod = 37
        c.residual = _rnd((37, N), s + 5)
    if feat in ("act_silu", "act_gelu"):
        c.act = ops.ACT_SILU if feat == "act_silu" else ops.ACT_GELU
        c.rpb = M // 2 if M % 2 == 0 else M
        c.rowvec = torch.randn(M // c.rpb, N, generator=torch.Generator().manual_seed(s + 4))
    if feat in ("geglu", "ln1_geglu", "ln2_geglu"):
        D = Npad // 2 - 32
        wg = torch.randn(2 * D, K, generator=torch.Generator().manual_seed(s + 2)) / math.sqrt(K)
        pg = ops.pack_geglu(wg, torch.randn(2 * D, generator=torch.Generator().manual_seed(s + 3)), "cpu")
        assert pg.Npad == Npad, (pg.Npad, Npad)
        c.w, c.bias, c.N, c.epi = pg.w, pg.bias, D, GEGLU
        c.extra["ldo"] = D + 24
    if feat in ("split_vt32", "split_vt_ragged", "ln1_split_vt", "ln2_split_vt"):
        c.epi, c.rpb = SPLIT_VT, L
        c.vt_col0 = {256: 192, 512: 384, 640: 448}[Npad]     # inside an N tile of the 128- / 256- / 320-wide tiles (and a 80-wide wave tile)
        c.extra["ldo"] = c.vt_col0 + 8
        c.extra["B"] = M // L
    if feat == "nchw":
        c.epi, c.rpb, c.N = NCHW, L, 68
        c.w = _pack_rows(w[:68], Npad)
        c.bias = _vec(68, Npad, s + 3)
    if feat == "two_source":
        c.c1 = 192
        c.a = c.a[:, :c.c1]
        c.a2 = _rnd((M, K - c.c1 + 24), s + 6)[:, :K - c.c1]
    if feat == "zero_rows":
        c.zero_rows = 70 if not big else 300
        c.a = c.a.clone()
        c.a[:c.zero_rows] = float("nan")          # declared zero: never read (a read would poison the outputs)
    if feat == "split_k2":
        c.split_k = 2
    if feat in ("split_k_odd", "split_k12"):
        c.split_k = 12 if feat == "split_k12" else SPLIT_ODD["gpu" if big else "emu"]
        c.rpb = M // 2 if M % 2 == 0 else M
        c.rowvec = torch.randn(M // c.rpb, N, generator=torch.Generator().manual_seed(s + 4))
    if lnf:
        c.ln, c.ln_mode = True, int(feat[2])
        if c.rpb == 0:
            c.rpb = M
    if feat == "row_stats":
        c.N = Npad - 32
        c.w = _pack_rows(w[:c.N], Npad)
        c.bias = _vec(c.N, Npad, s + 3)
        c.residual = c.residual[:, :c.N]
        c.rpb = 50 if M % 50 == 0 else M
        c.rowvec = torch.randn(M // c.rpb, c.N, generator=torch.Generator().manual_seed(s + 4))
        c.row_stats_out = True
        c.extra["ldo"] = c.N + 24
    return c


# ------------------------------------------------------------------------------------------------ fp64 reference
def _acc_ref(c: Case, absval: bool = False) -> torch.Tensor:
    """sum_k A[m, k] W[n, k] in fp64 over the bf16 operands, [M, Npad] (absval: the same with |A|, |W| -- the accumulation-error scale)."""
    f = (lambda t: t.double().abs()) if absval else (lambda t: t.double())
    W = f(c.w)
    if c.conv is None:
        A = f(c.a)
        if c.zero_rows:
            A = A.clone()
            A[:c.zero_rows] = 0
        if c.a2 is not None:
            A = torch.cat([A, f(c.a2)], 1)
        return A @ W.t()
    g = c.conv
    cin = g["cin"]
    x = f(c.a).permute(0, 3, 1, 2)                                          # NCHW
    if g["upsample"]:
        x = F.interpolate(x, size=(g["Ho"], g["Wo"]), mode="nearest")
    xp = F.pad(x, (1, 1, 1, 1))
    B, Ho, Wo, st = g["B"], g["Ho"], g["Wo"], g["stride"]

    def tap(k):
        ky, kx = divmod(k, 3)
        return xp[:, :, ky: ky + st * (Ho - 1) + 1: st, kx: kx + st * (Wo - 1) + 1: st].permute(0, 2, 3, 1).reshape(B * Ho * Wo, cin)
    if c.tap_group_n:
        ntaps = c.K // cin
        acc = torch.zeros(c.M, c.Npad, dtype=torch.float64, device=W.device)
        for gi in range(c.N // c.tap_group_n):
            n0, n1 = gi * c.tap_group_n, (gi + 1) * c.tap_group_n
            for i in range(ntaps):
                k = (c.tap_lut >> (16 * gi + 4 * i)) & 15
                acc[:, n0:n1] += tap(k) @ W[n0:n1, i * cin:(i + 1) * cin].t()
        return acc
    cols = torch.cat([tap(k) for k in range(9)], 1)                          # [M, 9 cin], k = tap * cin + c
    if c.a2 is not None:
        cols = torch.cat([cols, f(c.a2)] + ([f(c.a3)] if c.a3 is not None else []), 1)
    return cols @ W.t()


def reference(c: Case):
    """(expected outputs, error scale): outputs as a dict of fp64 tensors in the layout of the buffers the launch writes."""
    acc = _acc_ref(c)
    S = _acc_ref(c, absval=True)
    if c.ln:
        A = c.a.double()
        mean = A.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(A.var(1, unbiased=False, keepdim=True) + c.ln_eps)
        wsum = c.w.double().sum(1)
        acc = rstd * (acc - mean * wsum[None, :])
        S = rstd * (S + mean.abs() * wsum.abs()[None, :])
    rows = torch.arange(c.out_rows)
    src = rows % c.M
    v = acc[src]
    Sv = S[src]
    if c.bias is not None:
        v = v + c.bias.double()[None, :]
    if c.epi == GEGLU:
        D = c.N
        j = torch.arange(D)
        hi, gi = (j // 32) * 64 + j % 32, (j // 32) * 64 + 32 + j % 32
        h, gt = v[:, hi], v[:, gi]
        ga = F.silu(gt) if c.act == ops.ACT_SILU else F.gelu(gt)
        out = h * ga
        scale = (Sv[:, hi] * ga.abs() + 1.13 * h.abs() * Sv[:, gi]).max().item()
        return {"out": out}, scale
    v = v[:, : c.N]
    Sv = Sv[:, : c.N]
    if c.rowvec is not None:
        v = v + c.rowvec.double()[rows // c.rpb]
    if c.act:
        v = F.silu(v) if c.act == ops.ACT_SILU else F.gelu(v)
        Sv = 1.13 * Sv
    if c.residual is not None:
        v = v + c.residual.double()[rows % (c.res_mod or c.M) if not c.dup_rows else rows]
    scale = Sv.max().item()
    if c.epi == NCHW:
        B = c.M // c.rpb
        return {"nchw": v.view(B, c.rpb, c.N).permute(0, 2, 1).contiguous()}, scale
    if c.epi == SPLIT_VT:
        B = c.M // c.rpb
        return {"out": v[:, : c.vt_col0], "out2": v[:, c.vt_col0:].reshape(B, c.rpb, c.N - c.vt_col0).permute(0, 2, 1).contiguous()}, scale
    return {"out": v}, scale


def _within(got: torch.Tensor, ref: torch.Tensor, scale: float, K: int, bf16_out: bool) -> torch.Tensor:
    """elementwise: bf16 output rounding (2^-8 relative: an ulp of the result) + a K-scaled fp32 accumulation term on the |A||W| scale"""
    rel = 2.0 ** -8 if bf16_out else 2.0 ** -20
    bound = rel * ref.abs() + 2.0 ** -22 * math.sqrt(K) * 8 * scale + 2e-6
    return torch.isfinite(got) & ((got - ref).abs() <= bound)


# ------------------------------------------------------------------------------------------------ launching into sentinel-guarded windows
def _sent_like(n: int, dtype, dev) -> torch.Tensor:
    if dtype == BF16:
        return torch.full((n,), SENT16, dtype=torch.int16, device=dev).view(BF16)
    return torch.full((n,), SENT32, dtype=torch.int32, device=dev).view(torch.float32)


def _is_sent(t: torch.Tensor) -> torch.Tensor:
    if t.dtype == BF16:
        return t.view(torch.int16) == SENT16
    return t.view(torch.int32) == SENT32


class Launch:
    """The device buffers of one call: each output is a window of a sentinel-filled buffer."""

    def __init__(self, c: Case, dev, tile: int):
        self.c, self.dev = c, dev
        p = GemmParams()
        self.keep = []

        def put(t):
            if t is None:
                return None
            d = t.to(dev)
            self.keep.append(d)
            return d
        if c.conv is None:
            a = put(c.a)
            p.a, p.lda, p.c1 = a.data_ptr(), a.stride(0), a.shape[1]
            if c.a2 is not None:
                a2 = put(c.a2)
                p.a2, p.lda2 = a2.data_ptr(), a2.stride(0)
        else:
            g = c.conv
            a = put(c.a.contiguous())
            p.a, p.conv = a.data_ptr(), 1
            p.B, p.Hi, p.Wi, p.Ho, p.Wo, p.stride, p.upsample, p.cin = g["B"], g["Hi"], g["Wi"], g["Ho"], g["Wo"], g["stride"], g["upsample"], g["cin"]
            if c.a2 is not None:
                a2 = put(c.a2)
                p.a2, p.lda2, p.c1 = a2.data_ptr(), a2.stride(0), c.a2.shape[1]
            if c.a3 is not None:
                a3 = put(c.a3)
                p.a3, p.lda3 = a3.data_ptr(), a3.stride(0)
            p.tap_lut, p.tap_group_n = c.tap_lut, c.tap_group_n
        w = put(c.w)
        p.w, p.M, p.N, p.K, p.Npad = w.data_ptr(), c.M, c.N, c.K, c.Npad
        if c.bias is not None:
            p.bias = put(c.bias.float().contiguous()).data_ptr()
        p.rows_per_batch = c.rpb or c.M
        if c.rowvec is not None:
            rv = put(c.rowvec.float().contiguous())
            p.rowvec, p.ldrv = rv.data_ptr(), rv.stride(0)
        if c.residual is not None:
            r = put(c.residual)
            p.residual, p.ldr, p.res_mod = r.data_ptr(), r.stride(0), c.res_mod
        p.epilogue, p.vt_col0, p.act, p.zero_rows, p.dup_rows = c.epi, c.vt_col0, c.act, c.zero_rows, c.dup_rows
        if c.ln:
            wsum = put(c.w.float().sum(1).contiguous())
            p.ln_wsum, p.ln_eps = wsum.data_ptr(), c.ln_eps
            if c.ln_mode == 2:
                p.ln_row_stats = put(ops.row_stats_reference(c.a)).data_ptr()
        # outputs
        R, ncol = c.out_rows, c.out_cols
        self.ldo = _ldo(c)
        if c.epi == NCHW:
            self.flat = _sent_like(2 * GUARD + c.M * c.N, torch.float32, dev)
            p.out, p.ldo = self.flat.data_ptr() + 4 * GUARD, c.N
        else:
            self.obuf = _sent_like((R + 2) * self.ldo + 16, BF16, dev).view(-1)
            p.out, p.ldo = self.obuf.data_ptr() + 2 * (self.ldo + 8), self.ldo
        if c.epi == SPLIT_VT:
            B = c.M // c.rpb
            self.ldo2 = (c.rpb + 7) // 8 * 8 + 8
            self.o2 = _sent_like(2 * GUARD + B * (c.N - c.vt_col0) * self.ldo2, BF16, dev)
            p.out2, p.ldo2 = self.o2.data_ptr() + 2 * GUARD, self.ldo2
        if c.row_stats_out:
            self.rs = _sent_like(2 * GUARD + c.M * (c.N // 32) * 2, torch.float32, dev)
            p.row_stats_out = self.rs.data_ptr() + 4 * GUARD
        if c.split_k > 1:
            n = c.split_k * c.M * c.Npad
            self.ws = _sent_like(n + GUARD, torch.float32, dev)
            p.split_k, p.ws, p.ws_floats = c.split_k, self.ws.data_ptr(), n
        p.tile = tile
        self.p = p

    def __call__(self) -> int:
        return _lib.lib().pcdm_gemm(C.byref(self.p), None if self.dev.type == "cpu" else torch.cuda.current_stream().cuda_stream)

    def snapshot(self):
        bufs = [getattr(self, k) for k in ("flat", "obuf", "o2", "rs", "ws") if hasattr(self, k)]
        return [b.detach().clone().cpu() for b in bufs]

    def outputs(self):
        """(windows, list of (name, bytes outside every window) that must still hold the sentinel)"""
        c = self.c
        got, outside = {}, []
        if c.epi == NCHW:
            f = self.flat.cpu()
            got["nchw"] = f[GUARD: GUARD + c.M * c.N].view(c.M // c.rpb, c.N, c.rpb).double()
            outside += [("nchw guard", torch.cat([f[:GUARD], f[GUARD + c.M * c.N:]]))]
        else:
            o = self.obuf.cpu()
            R, ncol = c.out_rows, c.out_cols
            body = o[: (R + 2) * self.ldo].view(R + 2, self.ldo)
            got["out"] = body[1: R + 1, 8: 8 + ncol].double()
            mask = torch.ones_like(body, dtype=torch.bool)
            mask[1: R + 1, 8: 8 + ncol] = False
            outside += [("out outside the window (incl. columns N..Npad)", body[mask]), ("out tail", o[(R + 2) * self.ldo:])]
        if c.epi == SPLIT_VT:
            o2 = self.o2.cpu()
            B, cv = c.M // c.rpb, c.N - c.vt_col0
            body = o2[GUARD: GUARD + B * cv * self.ldo2].view(B, cv, self.ldo2)
            got["out2"] = body[:, :, : c.rpb].double()
            outside += [("out2 guard", torch.cat([o2[:GUARD], o2[GUARD + B * cv * self.ldo2:]])), ("out2 tokens >= L", body[:, :, c.rpb:])]
        if c.row_stats_out:
            r = self.rs.cpu()
            n = c.M * (c.N // 32) * 2
            got["row_stats"] = r[GUARD: GUARD + n].view(c.M, c.N // 32, 2).double()
            outside += [("row_stats guard", torch.cat([r[:GUARD], r[GUARD + n:]]))]
        if c.split_k > 1:
            outside += [("split-K workspace beyond ws_floats", self.ws.cpu()[c.split_k * c.M * c.Npad:])]
        return got, outside


def _check(c: Case, tile: int, L: Launch, ref: dict, scale: float, where: str):
    got, outside = L.outputs()
    for name, t in outside:
        assert bool(_is_sent(t).all()), f"{where}: tile {tile} wrote {name} ({int((~_is_sent(t)).sum())} elements)"
    for name, r in ref.items():
        bf16 = name != "nchw"
        ok = _within(got[name], r, scale, c.K, bf16)
        bad = int((~ok).sum())
        assert bad == 0, (f"{where}: tile {tile}, {name}: {bad} of {ok.numel()} elements off, max err "
                          f"{(got[name] - r).abs().nan_to_num(float('inf')).max().item():.4g} (scale {scale:.4g})")
        # the tolerance bites: one output channel off by 2^-5 of the output scale must fail
        pert = r.clone()
        d = r.pow(2).mean().sqrt().item() / 32 + 1e-3
        if name == "out":
            pert[:, -1] += d
        else:                                              # [B, channel, token]
            pert[:, -1, :] += d
        assert not bool(_within(got[name], pert, scale, c.K, bf16).all()), f"{where}: tile {tile}, {name}: the tolerance does not see a wrong channel"
    if c.row_stats_out:
        o = got["out"].float().to(BF16).float()            # the bf16 values stored
        rs_ref = ops.row_stats_reference(o).double()
        rs = got["row_stats"]
        tol = 1e-5 * o.abs().view(c.M, -1, 32).double().sum(-1).unsqueeze(-1) * torch.tensor([1.0, 0.0]).double() + \
            torch.tensor([1e-5, 0.0]).double() + 2e-5 * rs_ref.abs() + 1e-5
        assert bool(((rs - rs_ref).abs() <= tol).all()), f"{where}: tile {tile}: row statistics off by {(rs - rs_ref).abs().max().item():.3g}"


# ------------------------------------------------------------------------------------------------ §1: tile x feature matrix
def _feature_K(feat: str, tile: int, big: bool) -> int:
    if not big or tile in ROWGEMM:
        return ROWGEMM_K
    return 1280


def _run_matrix(tile: int, backend, feats):
    big = not backend.is_emu
    fails = []
    for feat in feats:
        key = (feat, _npad_for(tile), _feature_K(feat, tile, big), big)
        c = build_case(*key)
        L = Launch(c, backend.device, tile)
        rc = L()
        backend.sync()
        want = expect_accept(tile, c)
        if (rc == 0) != want:
            fails.append(f"tile {tile} x {feat}: rc {rc}, expected {'accept' if want else 'refuse (-1)'}")
            continue
        if rc != 0:
            assert rc == -1, f"tile {tile} x {feat}: rc {rc}"
            continue
        ref, scale = _ref_cached(*key)
        _check(c, tile, L, ref, scale, f"{backend.name} {feat}")
        if not backend.is_emu:                   # run again: bit-identical (a race shows up as a difference)
            first = L.snapshot()
            assert L() == 0
            backend.sync()
            for x, y in zip(first, L.snapshot()):
                assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"tile {tile} x {feat}: two runs differ"
    assert not fails, "\n".join(fails)


@functools.lru_cache(maxsize=None)
def _ref_cached(*key):
    return reference(build_case(*key))


@pytest.mark.parametrize("tile", sorted(TILE_CFG))
def test_tile_feature_matrix(backend, tile):
    _run_matrix(tile, backend, FEATURES + ([] if backend.is_emu else ["split_k12"]))


# ------------------------------------------------------------------------------------------------ §2: every tuning-table entry
TABLE = json.loads((Path(ops.__file__).resolve().parent / "tuning" / "gfx950.json").read_text())["gemm"]   # (the committed table)
UNET_WIDTHS = (1280, 640, 320, 64)                       # conv input widths (64: conv_in) -- K = 9 cin + cx is ambiguous without them
TOKENS = (5632, 1408, 352, 88, 4096, 1024, 256, 64, 258)  # rows per image of the UNet levels (768 x 512 and 512 x 512 latents) and the
#                                                          context tokens of the cross-attention k | v


def decode_key(key: str) -> dict:
    f = key.split(",")
    if f[0] == "ln":
        return dict(ln=True, M=int(f[1]), Npad=int(f[2]), K=int(f[3]), epi=int(f[4]), conv=0, stride=0, upsample=0, two=False, res=False, flag=0)
    flag = 0 if len(f) == 9 else (1 if f[9] == "True" else int(f[9]))
    return dict(ln=False, M=int(f[0]), Npad=int(f[1]), K=int(f[2]), conv=int(f[3]), stride=int(f[4]), upsample=int(f[5]), epi=int(f[6]),
                two=f[7] == "True", res=f[8] == "True", flag=flag)


def _conv_widths(d: dict):
    """(cin, cx) of a convolution key: stride field 21 = a tap subset (K = 4 cin); otherwise K = 9 cin + cx, cx > 0 iff two-source"""
    K = d["K"]
    if d["stride"] == 21:
        return K // 4, 0
    if not d["two"]:
        assert K % 9 == 0, K
        return K // 9, 0
    cin = next(c for c in UNET_WIDTHS if K - 9 * c > 0 and (K - 9 * c) % 64 == 0)
    return cin, K - 9 * cin


def _vt_col0(Npad: int) -> int:
    """q | k | v (N = 3 C) -> 2 C; k | v of the context (N = 2 C) -> C"""
    return 2 * Npad // 3 if Npad % 3 == 0 and Npad // 3 in (320, 640, 1280) else Npad // 2


def _status(n: int):
    return (n % 16 == 0, n % 32 == 0)


def _token_proxies(M: int, big: bool):
    """(B', L') per UNet token count that divides M: L' keeps L's divisibility by 16 and by 32, B' that of M (emulator); the GPU keeps L
    and takes as many images as two M tiles need"""
    out = []
    for L in TOKENS:
        if M % L:
            continue
        if big:
            out.append((max(1, min(M // L, 1 + 600 // L)), L))
            continue
        Lp = L % 64 + 64 if L % 64 else 64
        Bp = next(b for b in (1, 2, 4, 8, 16, 32) if _status(b * Lp) == _status(M))
        out.append((Bp, Lp))
    return list(dict.fromkeys(out)) or [(1, M if big or M <= 256 else (M % 64 + 64 if M % 64 else 64))]


def table_cases(key: str, choice, big: bool):
    """The problems an entry is run on: one, or one per candidate token count (SPLIT_VT).  Emulator: a proxy that keeps every property the
    acceptance rules read -- Npad mod 64 / 128 / 256 / 320 (and > 2560 for the A-in-registers tiles), tap_group_n mod the N tile, K mod 64,
    K <= 1280, split_k <= K / 64, epilogue, conv kind, two-source, residual and flag; GPU: the key's own Npad, K and flags, M cut to two M
    tiles of the entry's tile + a tail."""
    d = decode_key(key)
    tile, second = int(choice[0]), int(choice[1])
    split, mode = (1, second) if d["ln"] else (second, 0)
    BM = TILE_CFG[tile][0] if tile else 256
    Npad, K = d["Npad"], d["K"]
    if not big and tile not in ROWGEMM and Npad > 3840:
        Npad -= 1280 * ((Npad - 3840 + 1279) // 1280)          # same residue mod 1280 = lcm(64, 128, 256, 320)
    seed = zlib.crc32(key.encode()) % 1000
    Mt = min(d["M"], 2 * BM + 37) if big else min(d["M"], 136)
    cases = []
    epi = d["epi"]
    if d["conv"]:
        cin, cx = _conv_widths(d)
        if not big:
            taps = 4 if d["stride"] == 21 else 9
            cx = 64 if cx else 0
            cin = 64 if taps * 64 + cx >= 64 * split else 128
        if d["stride"] == 21:
            K = 4 * cin
            tgn = d["Npad"] // 4                                    # (N = 4 Cout: one group per output phase)
            if not big:
                tgn = tgn % 1280 or 1280                            # same residue mod every N tile width; two groups
                Npad = 2 * tgn
        else:
            K = 9 * cin + cx
        Wd = 8 if not big else 16
        rows = max(1, -(-Mt // Wd))
        if d["upsample"]:
            geo = dict(B=1, Hi=max(1, rows // 4) + 1, Wi=Wd // 2, stride=1, upsample=1)
            geo.update(Ho=2 * geo["Hi"], Wo=2 * geo["Wi"])
        elif d["stride"] == 2:
            geo = dict(B=1, Hi=2 * rows + 1, Wi=2 * Wd + 1, stride=2, upsample=0)
            geo.update(Ho=rows + 1, Wo=Wd + 1)
        else:
            geo = dict(B=1 if big else 2, Hi=rows if big else max(1, rows // 2), Wi=Wd + 1, stride=1, upsample=0)
            geo.update(Ho=geo["Hi"], Wo=geo["Wi"])
        M = geo["B"] * geo["Ho"] * geo["Wo"]
        N = 4 if epi == NCHW else Npad
        x = _rnd((geo["B"], geo["Hi"], geo["Wi"], cin), seed + 1)
        w = _weights(N, K, Npad)
        c = Case(name=key, M=M, N=N, K=K, Npad=Npad, a=x, w=w, bias=_vec(N, Npad, seed + 3), conv=dict(geo, cin=cin), epi=epi, split_k=split)
        if cx:
            c.a2, c.c1 = _rnd((M, cx), seed + 4), cx
        if d["stride"] == 21:
            c.tap_group_n = tgn
            c.tap_lut = ops.UPSAMPLE_TAP_LUT
        if epi == NCHW:
            c.rpb = geo["Ho"] * geo["Wo"]
        if d["flag"] == 2:
            c.dup_rows = M
        if d["res"]:
            c.residual, c.res_mod = _rnd((M + c.dup_rows, N), seed + 5), 0
        return tile, [c]
    if not big:
        K = ROWGEMM_K if K == ROWGEMM_K else max(128, 64 * split)
    N = Npad // 2 if epi == GEGLU else Npad
    shapes = [(None, Mt)] if epi != SPLIT_VT else [(L, B * L) for (B, L) in _token_proxies(d["M"], big)]
    if epi == NCHW:
        shapes = [(Mt, Mt)]
    for L, M in shapes:
        a = _rnd((M, K), seed + 1, offset=0.5 if d["ln"] else 0.0)
        if epi == GEGLU:
            w, bias = _geglu_weights(N, K)
        else:
            w = _weights(N, K, Npad)
            bias = _vec(N, Npad, seed + 3)
        if d["ln"] and tile == 0:            # (0, 1): LayerNorm launch + the plain GEMM on the library's heuristic tile
            a = F.layer_norm(a.double(), (K,)).to(BF16)
        c = Case(name=key, M=M, N=N, K=K, Npad=Npad, a=a, w=w, bias=bias, epi=epi, split_k=split, rpb=L or 0)
        if epi == SPLIT_VT:
            c.vt_col0 = _vt_col0(Npad)
        if d["ln"] and tile:
            c.ln, c.ln_mode = True, mode
        if d["two"]:
            c.a, c.a2, c.c1 = a[:, :64], a[:, 64:], 64
        if d["res"]:
            c.residual, c.res_mod = _rnd((M, N), seed + 5), M
        if d["flag"] == 1:
            c.zero_rows = M // 2
            c.a = c.a.clone()
            c.a[: c.zero_rows] = 0
        cases.append(c)
    return tile, cases


@functools.lru_cache(maxsize=8)
def _weights(N, K, Npad, dev=None):
    return _pack_rows(_randn((N, K), N * 7 + K) / math.sqrt(K), Npad)


@functools.lru_cache(maxsize=4)
def _geglu_weights(D, K, dev=None):
    pg = ops.pack_geglu(_randn((2 * D, K), D + K).cpu() / math.sqrt(K), _randn((2 * D,), D).cpu(), _DEV)
    return pg.w, pg.bias


def _table_by_tile():
    by = {}
    for k, v in TABLE.items():
        by.setdefault(int(v[0]), []).append(k)
    return by


def _run_table(backend, keys):
    """GPU: the operands are drawn and the fp64 reference computed on the device (torch fp64 matmul) -- at the keys' own Npad and K that is
    ~3 TFLOP for the whole table, out of reach of a CPU within the budget; the arithmetic is the same fp64 sum over the bf16 operands"""
    global _DEV
    big = not backend.is_emu
    _DEV = backend.device
    _weights.cache_clear()
    _geglu_weights.cache_clear()
    try:
        _run_table_on(backend, keys, big)
    finally:
        _DEV = torch.device("cpu")
        _weights.cache_clear()
        _geglu_weights.cache_clear()


def _run_table_on(backend, keys, big):
    done, bad = {}, []
    for key in keys:
        tile, cases = table_cases(key, TABLE[key], big)
        ok_any, why = False, []
        for c in cases:
            sig = None if big else (tile, c.name.split(",")[0] == "ln", c.M, c.N, c.K, c.Npad, c.epi, c.split_k, c.ln_mode, c.rpb, c.vt_col0,
                                     bool(c.conv) and (c.conv["stride"], c.conv["upsample"], c.tap_group_n), c.a2 is not None,
                                     c.residual is not None, c.zero_rows > 0, c.dup_rows > 0)
            if sig is not None and sig in done:        # (the deduplicated proxy)
                res = done[sig]
            else:
                L = Launch(c, backend.device, tile)
                rc = L()
                backend.sync()
                if rc != 0:
                    res = f"rc {rc}" + (f" at {c.rpb} tokens" if c.epi == SPLIT_VT else "")
                else:
                    ref, scale = reference(c)
                    ref = {k: v.cpu() for k, v in ref.items()}
                    try:
                        _check(c, tile, L, ref, scale, "table")
                        res = None
                    except AssertionError as e:
                        res = str(e).splitlines()[0]
                if sig is not None:
                    done[sig] = res
            if res is None:
                ok_any = True
                break
            why.append(res)
        if not ok_any:
            bad.append(f"{key} -> {TABLE[key]}: {'; '.join(why)}")
    assert not bad, f"{len(bad)} tuning-table entries refused or wrong:\n" + "\n".join(bad)


@pytest.mark.parametrize("tile", sorted(_table_by_tile()))
def test_tuning_table_entries(backend, tile):
    """Every entry of gfx950.json names a configuration the library accepts for its key, and that configuration computes the right answer.
    Keys hold neither a row vector nor res_mod (a table-named A-in-registers tile is a preference the library demotes when one is present:
    test_table_named_rowgemm_tile_is_a_preference), so entries run without a row vector and with res_mod = M."""
    _run_table(backend, _table_by_tile()[tile])
