"""Norm conformance: every GroupNorm dispatch outcome and every LayerNorm instantiation against an fp64 reference of the same bf16 operands.

What the file checks, and how (the GEMM and attention suites do the same for their kernels):

* ``expected_path`` mirrors ``gn_launch`` (pcdms_amd/csrc/norm.hip).  The library has no entry that tells which kernel ran; the WORKSPACE tells:
  it is filled with a NaN pattern (the counters zero) before every launch, and afterwards the single-pass kernel has written nothing, the
  cluster kernel exactly ``nslab * S * 8`` floats at the head, the two-kernel path exactly ``B * nchunk * groups * 2`` floats behind the
  cluster area.  A case whose footprint is not the mirror's fails and names both.  The layout constants are in one place below
  (``WS``), next to a pointer to the comment that documents them (``pcdm_groupnorm_ws_floats``).
* The case tables reach every outcome at the smallest shape that does (``test_case_tables_cover_every_outcome``).
* Inputs are built so that a mistake is loud: every group its own mean and spread, every batch entry its own scale and offset, gamma / beta
  distinct per channel, and the rows at every boundary of the schedule (first / last row, chunk edges, the last row a thread holds)
  multiplied by ``max(4, sqrt(HW) / 2)``.  ``test_tolerance_bites`` proves on the CPU that the bound then refuses statistics that miss a
  row, count one twice, or belong to the neighbouring group / batch entry.
* ``out`` / ``pre_out`` are windows of sentinel-filled buffers: every element inside is written, nothing outside; on the GPU every accepted
  call runs twice and gives the same bits.

The bound
---------
Per element, with u = 2^-8 (bf16 unit roundoff: the final store), v = 2^-24 (fp32 unit roundoff) and
``s = (|x| + |mu|) * rstd * |gamma| + |beta|`` (the magnitude of the terms of ``x * sc + sh``, sc = rstd * gamma, sh = beta - mu * sc):

    |out - ref| <= u * |ref| + K * v * s

``u * |ref|`` is the correctly rounded store alone (a correctly rounded fp64 result sits at 0.99 of the bound).  K counts the fp32 rounding
steps of the longest chain in norm.hip, each taken at its worst case (an error of v times a quantity that s bounds):

* the group mean, ``gn_cluster_kernel<512, 16>`` / ``gn_fused_kernel<1024, 8>``: the serial adds of the rows a thread holds (16 / 8), the
  adds of the octet's 8 channels into the group sums (8), the xor-shuffle tree of ``wave_sum`` (6), the serial sum of the wave partials
  (8 / 16), the product ``(float)HW * (float)gs``, its reciprocal and the multiply (3): 41 in both kernels.  An error of the mean enters the
  output as ``d(mu) * rstd * gamma`` and ``|sum| <= n (|mu| + sigma)``, ``sigma * rstd <= 1``.
* rstd: the centred squares have the same tree, but their RELATIVE error enters ``rstd = var^-1/2`` at half weight and multiplies
  ``(x - mu) * rstd * gamma`` -- the same 41 steps halved would be 21; the squares are positive, sums of positives are perfectly conditioned,
  and a relative error of ``(x - mu)``-sized terms is covered by the mean's share where ``|x - mu| <= |x| + |mu|``.  Counted: ``* inv_cnt``,
  ``+ eps``, ``sqrtf``, the divide (4, half weight: 2).
* ``sc = rstd * gamma`` (1), ``sh = beta - mean * sc`` (2), ``x * sc + sh`` (2).
* SiLU: the product with -log2(e) (its error is an ABSOLUTE error |f| v of the exponent, i.e. a relative one of the exponential that the
  factor f e^-f <= 0.37 of the result damps), ``fast_exp2`` (v_exp_f32, 1 ulp = 2 v), ``1 + .`` (1), ``fast_rcp`` (v_rcp_f32, 1 ulp = 2 v), the
  final product (1): 7; SiLU's slope is at most 1.1, which the worst-case counting above absorbs.

41 + 2 + 5 + 7 = 55; the fp64 merges of the cluster kernel and the final ``(float)mean`` add 1; K = 64 is the next power of two, chosen before
the kernels were run (PyTorch's own fp32 ``group_norm`` needs K ~ 4.5 on these inputs: random signs make the typical error the root of the
count, not the count).  Two things the count does NOT cover, stated here so that a failure is read correctly: (a) the ``sigma`` in
``|sum| <= n (|mu| + sigma)`` has no counterpart in s -- an element with x ~ 0 in a group with mu ~ 0 and beta ~ 0 has only ``u |ref|`` to
cover it (the table's group means are >= 1 in magnitude before the batch transform); (b) the two-kernel path merges the ``gs`` channel
means of a group in a SERIAL chain of Chan updates (``gn_stats_kernel``), each of which rounds the running mean: gs = 1024 (C = 4096, 4
groups) is 1024 steps in the worst case, 0.4 sqrt(1024) ~ 13 v |mu| typically (39 at three standard deviations), which K = 64 admits and a
coherent error would not.

LayerNorm (exact two-pass, ``(x - mean) * rstd * gamma + beta``): the mean of ``layernorm_kernel<8>`` at C = 4096 takes 64 serial adds per lane,
6 shuffles and the divide (71); then ``x - mean``, ``* rstd`` (+ 2 for rstd's own steps at half weight), ``* gamma``, ``+ beta`` (6): K_LN = 80 with
the same s.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
import subprocess
import sys
from dataclasses import dataclass, replace
from pathlib import Path
from typing import Optional

import pytest
import torch

from pcdms_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent
BF16 = torch.bfloat16
U = 2.0 ** -8
V = 2.0 ** -24
K_GN = 64.0
K_LN = 80.0
WORST = {}                      # path -> largest err / bound seen in this process


# ------------------------------------------------------------------------------------------------ the library's constants, in one place
class WS:
    """Workspace layout of pcdm_groupnorm -- see the comment in ``pcdm_groupnorm_ws_floats`` (norm.hip) and ``gn_cluster_kernel``'s
    'ws layout' note: [kGnClusterMaxWgs][8] cluster partials | [kGnClusterMaxWgs][2] unsigned arrival counters | the time-out counter
    (+ 7 floats of padding) | [B][kGnMaxChunks][256][2] partial statistics of the two-kernel path."""
    MAX_CHUNKS = 64             # kGnMaxChunks
    UNROLL = 4                  # kGnUnroll
    MAX_C = 4096                # kGnMaxC
    THREADS = 256               # kThreads (stats / apply / LayerNorm)
    CLUSTER_THREADS = 512
    CLUSTER_MAX_WGS = 256       # kGnClusterMaxWgs
    COUNTERS = CLUSTER_MAX_WGS * 8                      # float offset of the counters
    TIMEOUT = COUNTERS + CLUSTER_MAX_WGS * 2            # float offset of the time-out counter
    CLUSTER_FLOATS = TIMEOUT + 8                        # kGnClusterFloats = 2568: where the two-kernel statistics start
    MAX_SLAB_KB = 352           # gn_launch: largest (batch, group set) slab of the single-pass kernel
    GUARD = 64                  # floats behind pcdm_groupnorm_ws_floats that nothing may touch
    NAN_BITS = 0x7FC0DEAD       # the sentinel


assert WS.CLUSTER_FLOATS == 2568


def _cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ 1. the mirror of gn_launch
@dataclass(frozen=True)
class GnPath:
    kind: str                   # "fused" | "cluster" | "two_kernel"
    gpb: int                    # groups per workgroup of the single-pass kernels (5: none)
    noct: int                   # octets of a group set (single-pass) -- two_kernel: octets of a ROW (C / 8)
    threads: int = 0            # fused
    maxr: int = 0               # fused / cluster
    S: int = 0                  # cluster
    rows_per_chunk: int = 0     # cluster / two_kernel
    nchunk: int = 0             # two_kernel
    rows_par: int = 0           # rows walked in parallel by one workgroup
    nslab: int = 0

    def outcome(self) -> str:
        if self.kind == "fused":
            return f"fused{self.threads}"
        if self.kind == "cluster":
            return f"cluster_s{self.S}_r{self.maxr}"
        return "two_kernel_" + ("lt256" if self.noct < 256 else "eq256" if self.noct == 256 else "gt256")


def gn_cluster_split(nslab: int, HW: int, noct: int) -> int:
    rows_par = WS.CLUSTER_THREADS // noct
    S = 2
    while S <= 8 and nslab * S <= WS.CLUSTER_MAX_WGS:
        if _cdiv(_cdiv(HW, S), rows_par) <= 16:
            return S
        S *= 2
    return 0


def expected_path(B: int, HW: int, C1: int, C2: int, groups: int, splitk: bool, cluster_ok: bool, is_emu: bool) -> GnPath:
    """``gn_launch`` in Python.  ``splitk`` does not move the dispatch (the split-K source takes every path; the two-kernel one behind a reduce
    launch of its own); ``cluster_ok``: what ``gn_cluster_enabled`` answers on the device; the emulator never takes the cluster path."""
    del splitk
    Cc = C1 + C2
    gs = Cc // groups
    gpb = 1
    while gpb <= 4 and (gpb * gs) % 8:
        gpb += 1
    noct = gpb * gs // 8
    cluster_ok = cluster_ok and not is_emu
    max_slab = int(os.environ.get("PCDM_GN_FUSED_MAX_KB", WS.MAX_SLAB_KB)) * 1024
    if gpb <= 4 and groups % gpb == 0 and noct <= 64:
        nslab = (groups // gpb) * B
        few_slabs = nslab <= 128 and HW >= 1024
        split = gn_cluster_split(nslab, HW, noct) if cluster_ok else 0
        if HW * noct * 16 <= max_slab and not (few_slabs and split > 0):
            for th in (256, 512, 1024):
                if _cdiv(HW, th // noct) <= 8:
                    return GnPath("fused", gpb, noct, threads=th, maxr=8, rows_par=th // noct, nslab=nslab)
        if split:
            rows_par = WS.CLUSTER_THREADS // noct
            rpc = _cdiv(HW, split)
            return GnPath("cluster", gpb, noct, maxr=8 if _cdiv(rpc, rows_par) <= 8 else 16, S=split, rows_per_chunk=rpc,
                          rows_par=rows_par, nslab=nslab)
    noct_row = Cc // 8
    rows_par = WS.THREADS // min(noct_row, WS.THREADS)
    nchunk = max(1, min(WS.MAX_CHUNKS, _cdiv(HW, rows_par * WS.UNROLL)))
    return GnPath("two_kernel", gpb, noct_row, rows_per_chunk=_cdiv(HW, nchunk), nchunk=nchunk, rows_par=rows_par)


def ws_footprint(p: GnPath, B: int, groups: int):
    """(first float, floats) that the path writes in the workspace, the counters apart"""
    if p.kind == "fused":
        return (0, 0)
    if p.kind == "cluster":
        return (0, p.nslab * p.S * 8)
    return (WS.CLUSTER_FLOATS, B * p.nchunk * groups * 2)


def boundary_rows(p: GnPath, HW: int) -> set:
    """rows at which the path's schedule has an edge: first / last row, chunk edges, the first row of the last pass of a thread"""
    rows = {0, HW - 1}
    if p.kind == "fused":
        rows.add(((HW - 1) // p.rows_par) * p.rows_par)
        return rows
    nch = p.S if p.kind == "cluster" else p.nchunk
    step = p.rows_par * (1 if p.kind == "cluster" else WS.UNROLL)
    for ch in range(nch):
        r0, r1 = ch * p.rows_per_chunk, min((ch + 1) * p.rows_per_chunk, HW)
        if r1 > r0:
            rows |= {r0, r1 - 1, r0 + ((r1 - r0 - 1) // step) * step}
    return rows


def device_cluster_ok(backend) -> bool:
    """what ``gn_cluster_enabled`` decides (norm.hip): the switch, no CU mask, a device with one CU per workgroup of the largest grid"""
    if backend.is_emu or os.environ.get("PCDM_GN_CLUSTER", "1")[:1] == "0":
        return False
    if any(m in os.environ for m in ("HSA_CU_MASK", "ROC_GLOBAL_CU_MASK", "HSA_CU_MASK_SKIP_INIT")):
        return False
    return torch.cuda.get_device_properties(backend.device).multi_processor_count >= WS.CLUSTER_MAX_WGS


# ------------------------------------------------------------------------------------------------ 2. the case tables
@dataclass(frozen=True)
class Case:
    name: str
    B: int
    HW: int
    C1: int
    C2: int
    G: int
    sk: int = 0                 # split-K form of x1: the number of fp32 slabs (0: plain bf16)
    flavour: str = "plain"      # "plain" | "large_mean" | "const" | "zeros"
    eps: float = 1e-5
    sk_ops: str = "brv"         # split-K form: which of bias / row vector / residual are present
    step: Optional[int] = None  # split-K form: the value of the device step counter (None: no counter); count = 3
    store_pre: int = 1

    @property
    def C(self):
        return self.C1 + self.C2

    @property
    def form(self):
        return "sk" if self.sk else "two" if self.C2 else "plain"

    def path(self, cluster_ok: bool, is_emu: bool) -> GnPath:
        return expected_path(self.B, self.HW, self.C1, self.C2, self.G, bool(self.sk), cluster_ok, is_emu)


def _forms(name, B, HW, Cc, G, c1, sk, **kw):
    """the plain, the two-source (split at c1, inside a group where the group size allows) and the split-K form of one shape"""
    return [Case(name + "-plain", B, HW, Cc, 0, G, **kw), Case(name + "-two", B, HW, c1, Cc - c1, G, **kw),
            Case(name + "-sk", B, HW, c1, Cc - c1, G, sk=sk, **kw)]


# Cases that run on both backends.  With noct = 64 (one group of 512 channels) the single-pass kernel
# holds HW <= 32 / 64 / 128 rows at 256 / 512 / 1024 threads, the cluster kernel (GPU) HW <= 256 / 512 / 1024 at S = 2 / 4 / 8.
SMALL = (
    _forms("f256-hw30", 2, 30, 512, 1, 200, 2)
    + _forms("f512-hw60", 2, 60, 512, 1, 200, 3, eps=1e-6)
    + _forms("f1024-hw100", 2, 100, 512, 1, 264, 4)
    # GPU: cluster S = 2 with 16 rows held; emulator: two-kernel at exactly 256 octets per row
    + _forms("c2048-hw130", 1, 130, 2048, 4, 1000, 5)
    # cluster refused on the emulator -> two-kernel, noct < 256; GPU: S = 2 / MAXR 16 with a ragged last chunk
    + _forms("n64-hw201", 2, 201, 512, 1, 200, 2, eps=1e-6)
    # C > 2048: the ocb loop of gn_stats_kernel takes a second trip (512 and 384 octets per row); ragged last chunk
    + _forms("c4096-hw70", 1, 70, 4096, 4, 2000, 8)
    + [Case("c3072-hw37", 2, 37, 3072, 0, 3), Case("c1024-g1-noct128", 2, 45, 1024, 0, 1)]
    # odd group sizes: always two-kernel
    + _forms("gs1", 2, 50, 32, 32, 16, 9)
    + [Case("gs3", 2, 50, 24, 0, 8), Case("gs5-two", 2, 50, 16, 24, 8, eps=1e-6), Case("gs3-hw600-3chunks", 1, 600, 24, 0, 8)]
    # octets that span two (four) groups: gpb 4 and 2
    + [Case("gs10", 2, 37, 80, 0, 8), Case("gs30-two", 2, 37, 64, 176, 8), Case("gs60-sk", 2, 37, 96, 144, 4, sk=3),
       Case("gs20", 2, 37, 160, 0, 8, eps=1e-6), Case("gs12-two", 2, 37, 40, 56, 8), Case("gs6", 2, 37, 48, 0, 8),
       Case("gs4-sk", 2, 37, 32, 0, 8, sk=2, sk_ops=""), Case("gs2", 3, 37, 16, 0, 8), Case("gs10-f512", 2, 700, 80, 0, 8)]
    # small B and HW
    + [Case("b1-hw1", 1, 1, 64, 0, 8), Case("hw1-two", 3, 1, 32, 32, 8), Case("hw3-below-rows-par", 2, 3, 16, 0, 2),
       Case("two-kernel-b1-hw1", 1, 1, 24, 0, 8), Case("two-kernel-hw3-below-rows-par", 2, 3, 24, 0, 8),
       Case("two-kernel-hw1-c4096", 1, 1, 4096, 0, 4)]
    # +50 sigma, a constant slab and a slab of zeros per path (the cluster path: LARGE)
    + [Case("f512-large-mean", 2, 60, 512, 0, 1, flavour="large_mean"), Case("f256-const", 2, 37, 64, 0, 8, flavour="const"),
       Case("f256-zeros", 2, 37, 64, 0, 8, flavour="zeros"), Case("two-kernel-large-mean", 2, 700, 24, 0, 8, flavour="large_mean"),
       Case("two-kernel-const", 2, 50, 24, 0, 8, flavour="const", eps=1e-6), Case("two-kernel-zeros-sk", 2, 50, 24, 0, 8, sk=2, flavour="zeros"),
       Case("c2048-hw130-large-mean", 1, 130, 2048, 0, 4, flavour="large_mean"), Case("c2048-hw130-const", 1, 130, 2048, 0, 4, flavour="const"),
       Case("c2048-hw130-zeros", 1, 130, 2048, 0, 4, flavour="zeros")]
    # ---- the shapes of the cluster kernel (GPU) and of its refusals; the emulator takes them on the other two paths
    + _forms("s2r8-b1-hw1024", 1, 1024, 64, 8, 24, 2)                    # the shared-CFG-prefix batch; 8 slabs -> cluster although it fits
    + _forms("s4r16-hw301", 2, 301, 512, 1, 200, 3)                    # ragged: chunks of 76, 76, 76, 73
    + _forms("s8r16-hw601", 2, 601, 512, 1, 264, 4, eps=1e-6)          # chunks of 76 ... 69
    + [Case("s8r16-hw600", 2, 600, 512, 0, 1), Case("s4r16-hw300", 2, 300, 512, 0, 1), Case("s2r16-hw200", 2, 200, 512, 0, 1)]
    + [Case("cluster-gs10-hw1031", 1, 1031, 80, 0, 8), Case("cluster-gs20-two", 1, 1030, 64, 96, 8)]
    # refused by the cluster kernel (S = 8 would hold 18 rows): two-kernel with 64 chunks of 18, the last two EMPTY
    + _forms("refused-hw1100", 2, 1100, 512, 1, 200, 2)
    + _forms("c2048-hw1147", 1, 1147, 2048, 4, 1000, 2)               # exactly 256 octets; 64 chunks of 18, the last of 13
    + [Case("c4096-hw1500", 1, 1500, 4096, 0, 4)]                      # 64 chunks of 24, the last EMPTY
    + [Case("cluster-large-mean", 2, 301, 512, 0, 1, flavour="large_mean"), Case("cluster-const", 2, 201, 512, 0, 1, flavour="const"),
       Case("cluster-zeros-sk", 2, 601, 512, 0, 1, sk=2, flavour="zeros")]
)

# GPU only (seconds apiece under the emulator): the largest and the first refused number of slabs at S = 8 (8 x 32 = 256 workgroups)
LARGE = [Case("s8r16-hw513-32slabs", 32, 513, 512, 0, 1), Case("refused-33slabs-hw513", 33, 513, 512, 0, 1)]
CASES = {c.name: c for c in tuple(SMALL) + tuple(LARGE)}
assert len(CASES) == len(SMALL) + len(LARGE)
CLUSTER_CASES = tuple(c.name for c in CASES.values() if c.path(True, False).kind == "cluster")

GPU_OUTCOMES = ("fused256", "fused512", "fused1024", "cluster_s2_r8", "cluster_s2_r16", "cluster_s4_r16", "cluster_s8_r16",
                "two_kernel_lt256", "two_kernel_eq256", "two_kernel_gt256")
EMU_OUTCOMES = ("fused256", "fused512", "fused1024", "two_kernel_lt256", "two_kernel_eq256", "two_kernel_gt256")
# S = 4 and S = 8 are tried only after S / 2 was refused, i.e. ceil(ceil(HW / (S/2)) / rows_par) >= 17, which makes
# ceil(ceil(HW / S) / rows_par) >= 9: the 8-row instantiation never runs with S > 2.  (The scan below checks that, not only this sentence.)
UNREACHABLE = {"cluster_s4_r8": "S = 4 follows a refused S = 2 (> 16 rows per thread): at S = 4 a thread then holds > 8",
               "cluster_s8_r8": "S = 8 follows a refused S = 4 (> 16 rows per thread): at S = 8 a thread then holds > 8"}


def test_case_tables_cover_every_outcome():
    """every dispatch outcome in the plain, the two-source and the split-K form: on the GPU (cluster path on), on the emulator, and -- for
    the shapes of the cluster path -- with the cluster path off; the outcomes that cannot occur are shown not to"""
    for what, cases, cluster_ok, is_emu, want in (("gpu", CASES.values(), True, False, GPU_OUTCOMES), ("emu", SMALL, False, True, EMU_OUTCOMES)):
        seen = {(c.path(cluster_ok, is_emu).outcome(), c.form) for c in cases}
        missing = [(o, f) for o in want for f in ("plain", "two", "sk") if (o, f) not in seen]
        assert not missing, f"{what}: no case for {missing}"
    off = {CASES[n].path(False, False).kind for n in CLUSTER_CASES}
    assert off == {"fused", "two_kernel"}, off           # PCDM_GN_CLUSTER=0: the cluster shapes fall to BOTH other paths
    for noct in range(1, 65):                            # every (noct, HW) the cluster kernel can take, nslab = 1
        rows_par = WS.CLUSTER_THREADS // noct
        for HW in range(1, 8 * 16 * rows_par + 2):
            S = gn_cluster_split(1, HW, noct)
            assert not (S > 2 and _cdiv(_cdiv(HW, S), rows_par) <= 8), (UNREACHABLE, noct, HW, S)
    # groups % gpb != 0 (a refusal of the single-pass kernels in gn_launch) cannot occur either: gpb = 2 needs gs = 4 mod 8 and gpb = 4
    # needs gs = 2 mod 4, and C = groups * gs is a multiple of 8 only with groups a multiple of 2 resp. 4; gpb = 3 would need 8 | gs
    for gs in range(1, 513):
        gpb = next((k for k in range(1, 5) if (k * gs) % 8 == 0), 5)
        assert gpb != 3 and all(G % gpb == 0 for G in range(1, 257) if gpb <= 4 and (G * gs) % 8 == 0 and G * gs <= WS.MAX_C)
    for c in CASES.values():
        assert c.B * c.HW * c.C <= 1536 * 4096 * 3 // 2, c.name    # (the largest: 32 / 33 slabs at the first HW that needs S = 8)
    # the dispatch arithmetic the tables were built from
    for (B, HW, Cc, G), want in (((1, 1024, 64, 8), "cluster_s2_r8"), ((2, 300, 512, 1), "cluster_s4_r16"), ((2, 600, 512, 1), "cluster_s8_r16"),
                                 ((32, 600, 512, 1), "cluster_s8_r16"), ((33, 600, 512, 1), "two_kernel_lt256"), ((2, 1100, 512, 1), "two_kernel_lt256"),
                                 ((2, 30, 512, 1), "fused256"), ((2, 60, 512, 1), "fused512"), ((2, 100, 512, 1), "fused1024"),
                                 ((2, 999, 32, 32), "two_kernel_lt256"), ((2, 7, 24, 8), "two_kernel_lt256"), ((1, 9, 4096, 4), "two_kernel_gt256"),
                                 ((1, 9, 2048, 2), "two_kernel_eq256")):
        assert expected_path(B, HW, Cc, 0, G, False, True, False).outcome() == want, (B, HW, Cc, G)
    p = expected_path(1, 9, 4096, 0, 4, False, True, False)
    assert (p.noct, 4096 // 4 // 8) == (512, 128)


# ------------------------------------------------------------------------------------------------ 3. inputs
def _frac(i: torch.Tensor, a: float) -> torch.Tensor:
    return torch.frac((i.double() + 1.0) * a)


def _schedule_rows(case: Case) -> set:
    rows = set()
    for cluster_ok, is_emu in ((True, False), (False, False), (False, True)):
        rows |= boundary_rows(case.path(cluster_ok, is_emu), case.HW)
    return rows


@functools.lru_cache(maxsize=3)
def gn_operands(case: Case):
    """(x [B, HW, C], gamma [C], beta [C]) as fp64 tensors holding bf16 values"""
    B, HW, Cc, G = case.B, case.HW, case.C, case.G
    gs = Cc // G
    gen = torch.Generator().manual_seed(1000 + sum(map(ord, case.name)))
    gi = torch.arange(G)
    mean_g = torch.where(gi % 2 == 0, 1.0, -1.0).double() * (1.0 + 8.0 * _frac(gi, 0.6180339887))        # +-(1 .. 9), neighbours far apart
    spread_g = 2.0 ** (-2.0 + 4.0 * _frac(gi, 0.7548776662))                                               # 1/4 .. 4
    if case.flavour == "large_mean":
        mean_g = mean_g + 50.0 * spread_g
    x = torch.randn(B, HW, G, gs, generator=gen, dtype=torch.float64) * spread_g.view(1, 1, G, 1) + mean_g.view(1, 1, G, 1)
    bi = torch.arange(B)
    scale_b = 2.0 ** (torch.remainder(bi * 2 + 1, 5).double() - 2.0) * (1.0 + 0.25 * _frac(bi, 0.6180339887))   # 1/4 .. 4, all different for B <= 5
    off_b = 6.0 * (_frac(bi, 0.7548776662) - 0.5) * (bi > 0)
    x = x * scale_b.view(B, 1, 1, 1) + off_b.view(B, 1, 1, 1)
    amp = max(4.0, math.sqrt(HW) / 2.0)
    x[:, sorted(_schedule_rows(case))] *= amp
    if case.flavour == "const":
        x[0, :, 0, :] = 3.140625
        if G > 1:                                       # (one group: the other batch entry keeps its rows, for the mutations to bite)
            x[B - 1, :, G - 1, :] = -0.0478515625
    if case.flavour == "zeros":
        x[0, :, 0, :] = 0.0
        if G > 1:
            x[B - 1, :, G - 1, :] = 0.0
    x = x.reshape(B, HW, Cc).to(BF16).double()
    ci = torch.arange(Cc)
    gamma = (0.5 + 1.5 * _frac(ci, 0.6180339887)) * torch.where(ci % 5 == 3, -1.0, 1.0).double()
    beta = 6.0 * (_frac(ci, 0.7548776662) - 0.5)
    return x, gamma.to(BF16).double(), beta.to(BF16).double()


# ------------------------------------------------------------------------------------------------ 4. reference and bound
def gn_stats(x: torch.Tensor, G: int, rows=None):
    """fp64 {mean, biased variance} [B, G] of x [B, HW, C] over the given rows (a list with repeats allowed; None: all)"""
    B, HW, Cc = x.shape
    xs = x if rows is None else x[:, rows]
    xs = xs.reshape(B, xs.shape[1], G, Cc // G)
    mu = xs.mean(dim=(1, 3))
    var = ((xs - mu.view(B, 1, G, 1)) ** 2).mean(dim=(1, 3))
    return mu, var


def gn_eval(x, gamma, beta, G, mu, var, eps, silu):
    """fp64 GroupNorm(+SiLU) of x with the given statistics, and the bound's magnitude s"""
    B, HW, Cc = x.shape
    gs = Cc // G
    mu_c = mu.repeat_interleave(gs, dim=1).view(B, 1, Cc)
    rstd_c = (1.0 / torch.sqrt(var + eps)).repeat_interleave(gs, dim=1).view(B, 1, Cc)
    y = (x - mu_c) * rstd_c * gamma + beta
    s = (x.abs() + mu_c.abs()) * rstd_c * gamma.abs() + beta.abs()
    if silu:
        y = y * torch.sigmoid(y)
    return y, s


@functools.lru_cache(maxsize=4)
def gn_reference(case: Case, silu: bool):
    x, gamma, beta = gn_operands(case)
    return _gn_reference_of(x, gamma, beta, case.G, case.eps, silu)


def _gn_reference_of(x, gamma, beta, G, eps, silu):
    mu, var = gn_stats(x, G)
    ref, s = gn_eval(x, gamma, beta, G, mu, var, eps, silu)
    return ref, U * ref.abs() + K_GN * V * s


def compare(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor):
    """(violations, largest err / bound, flat index of the worst element); a non-finite output is a violation"""
    out = out.double().cpu().reshape(ref.shape)
    bad = ~torch.isfinite(out)
    err = (torch.where(bad, torch.zeros_like(out), out) - ref).abs()
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    ratio = torch.where(bad, torch.full_like(ratio, float("inf")), ratio)
    worst = int(ratio.argmax())
    return int((ratio > 1.0).sum()), float(ratio.flatten()[worst]), worst


# ------------------------------------------------------------------------------------------------ 7. the split-K source without a GEMM
SK_STEP_COUNT = 3


@functools.lru_cache(maxsize=3)
def sk_source(case: Case):
    """Synthetic operands of ``pcdm_gn_splitk_src`` whose sum is (about) the structured x1 of the case, and ``pre``: the fp32 sum on the CPU in
    the documented order (slabs by index, bias, row vector, residual), rounded to nearest-even bf16 -- what ``pre_out`` must hold, bit for
    bit, and what the GroupNorm normalises."""
    x, gamma, beta = gn_operands(case)
    B, HW, C1, S = case.B, case.HW, case.C1, case.sk
    M = B * HW
    Npad, ldr, ldrv = C1 + 8 * (1 + case.B % 2), C1 + 16, C1 + 4 * 3
    gen = torch.Generator().manual_seed(77 + sum(map(ord, case.name)))
    x1 = x[:, :, :C1].reshape(M, C1).float()
    bias = torch.randn(Npad, generator=gen) if "b" in case.sk_ops else None
    rowvec = torch.randn(SK_STEP_COUNT if case.step is not None else 1, B, ldrv, generator=gen) * 2.0 if "r" in case.sk_ops else None
    residual = (torch.randn(M, ldr, generator=gen) * 1.5).to(BF16) if "v" in case.sk_ops else None
    block = 0 if case.step is None else min(max(case.step, 0), SK_STEP_COUNT - 1)      # the clamp the device applies
    rest = x1.clone()
    if bias is not None:
        rest -= bias[:C1]
    if rowvec is not None:
        rest -= rowvec[block, :, :C1].repeat_interleave(HW, dim=0)
    if residual is not None:
        rest -= residual[:, :C1].float()
    part = torch.randn(S, M, Npad, generator=gen) * 3.0                               # (the padding columns hold noise: never read)
    part[S - 1, :, :C1] = rest - part[:S - 1, :, :C1].sum(0)
    v = torch.zeros(M, C1)
    for k in range(S):
        v = v + part[k, :, :C1]
    v = v + (bias[:C1] if bias is not None else torch.zeros(C1))
    v = v + (rowvec[block, :, :C1].repeat_interleave(HW, dim=0) if rowvec is not None else torch.zeros(M, C1))
    pre = (v + (residual[:, :C1].float() if residual is not None else torch.zeros(M, C1))).to(BF16)
    xs = torch.cat([pre.double().view(B, HW, C1), x[:, :, C1:]], dim=2)
    return dict(part=part, bias=bias, rowvec=rowvec, residual=residual, pre=pre, x=xs, gamma=gamma, beta=beta, Npad=Npad, ldr=ldr, ldrv=ldrv)


@functools.lru_cache(maxsize=4)
def sk_reference(case: Case, silu: bool):
    src = sk_source(case)
    return _gn_reference_of(src["x"], src["gamma"], src["beta"], case.G, case.eps, silu)


# ------------------------------------------------------------------------------------------------ 6. launches behind guards
GUARD16 = 64                    # bf16 elements in front of and behind every output window (128 bytes: the windows stay 16-byte aligned)
SENT16 = 0x7FB5                 # a bf16 NaN no kernel produces


def _sent16(n: int, dev) -> torch.Tensor:
    t = torch.empty(n + 2 * GUARD16, dtype=BF16, device=dev)
    t.view(torch.int16).fill_(SENT16)
    return t


def _window_state(buf: torch.Tensor):
    """(guards intact, elements of the window still holding the sentinel)"""
    b = buf.view(torch.int16).cpu()
    n = b.numel() - 2 * GUARD16
    return bool((b[:GUARD16] == SENT16).all() and (b[GUARD16 + n:] == SENT16).all()), int((b[GUARD16:GUARD16 + n] == SENT16).sum())


class GnLaunch:
    """One case on one backend: device operands, sentinel-filled outputs and workspace, the call through the C ABI, the checks behind it."""

    def __init__(self, case: Case, backend):
        self.case, self.backend, dev = case, backend, backend.device
        self.dev = dev
        B, HW, C1, C2 = case.B, case.HW, case.C1, case.C2
        M = B * HW
        if case.sk:
            src = sk_source(case)
            x = src["x"]
            self.part = src["part"].to(dev)
            self.bias = None if src["bias"] is None else src["bias"].to(dev)
            self.rowvec = None if src["rowvec"] is None else src["rowvec"].to(dev)
            self.residual = None if src["residual"] is None else src["residual"].to(dev)
            self.step = None if case.step is None else torch.tensor([case.step], dtype=torch.int32, device=dev)
            self.step_error = torch.zeros(1, dtype=torch.int32, device=dev)
            self.Npad, self.ldr, self.ldrv = src["Npad"], src["ldr"], src["ldrv"]
            self.pre_expect = src["pre"]
            self.x1 = None
        else:
            x = gn_operands(case)[0]
            self.x1 = x[:, :, :C1].reshape(M, C1).to(BF16).contiguous().to(dev)
        gamma, beta = gn_operands(case)[1:]
        self.x2 = x[:, :, C1:].reshape(M, C2).to(BF16).contiguous().to(dev) if C2 else None
        self.gamma, self.beta = gamma.float().to(dev), beta.float().to(dev)
        self.n_ws = int(_lib.lib().pcdm_groupnorm_ws_floats(B, case.C))
        self.ws = torch.empty(self.n_ws + WS.GUARD, dtype=torch.float32, device=dev)
        self.reset()

    def reset(self):
        c = self.case
        self.obuf = _sent16(c.B * c.HW * c.C, self.dev)
        self.pbuf = _sent16(c.B * c.HW * c.C1, self.dev)
        self.ws.view(torch.int32).fill_(WS.NAN_BITS)
        self.ws[WS.COUNTERS:WS.TIMEOUT + 1] = 0.0          # the counters are zero on entry
        if self.case.sk:
            self.step_error.zero_()

    def sync(self):
        self.backend.sync()

    def call(self, silu: bool, **over) -> int:
        """the C call; ``over`` replaces arguments (the refusal tests)"""
        c, L = self.case, _lib.lib()
        a = dict(C1=c.C1, C2=c.C2, B=c.B, HW=c.HW, G=c.G, x2=ops._ptr(self.x2), y=self.obuf[GUARD16:].data_ptr(), ws=self.ws.data_ptr(),
                 gamma=self.gamma.data_ptr(), beta=self.beta.data_ptr())
        a.update({k: v for k, v in over.items() if k in a})
        st = ops._stream(self.obuf)
        if not c.sk:
            a["x1"] = over.get("x1", self.x1.data_ptr())
            return L.pcdm_groupnorm(a["x1"], a["C1"], a["x2"], a["C2"], a["B"], a["HW"], a["G"], c.eps, a["gamma"], a["beta"], int(silu),
                                    a["y"], a["ws"], st)
        sp = _lib.GnSplitKSrc()
        sp.part, sp.split_k, sp.M, sp.N, sp.Npad = self.part.data_ptr(), c.sk, c.B * c.HW, c.C1, self.Npad
        sp.bias, sp.rowvec, sp.ldrv = ops._ptr(self.bias), ops._ptr(self.rowvec), self.ldrv
        sp.rowvec_step, sp.rowvec_step_stride = ops._ptr(self.step), c.B * self.ldrv
        sp.rowvec_step_count, sp.step_error = (SK_STEP_COUNT if self.step is not None else 0), self.step_error.data_ptr()
        sp.residual, sp.ldr = ops._ptr(self.residual), self.ldr
        sp.pre_out, sp.store_pre = self.pbuf[GUARD16:].data_ptr(), c.store_pre
        for k, v in over.items():
            if k.startswith("sp_"):
                setattr(sp, k[3:], v)
        return L.pcdm_groupnorm_splitk(C.byref(sp) if not over.get("null_src") else None, a["x2"], a["C2"], a["B"], a["HW"], a["G"], c.eps,
                                       a["gamma"], a["beta"], int(silu), a["y"], a["ws"], st)

    def ws_written(self):
        """(first, count) of the floats that no longer hold the sentinel, the counter region apart -- and the problems seen"""
        w = self.ws.view(torch.int32).cpu()
        probs = []
        if not bool((w[self.n_ws:] == WS.NAN_BITS).all()):
            probs.append("the guard behind pcdm_groupnorm_ws_floats was written")
        cnt = w[WS.COUNTERS:WS.TIMEOUT]
        if int(cnt.abs().max()):
            probs.append(f"arrival counters not zero after the launch ({int((cnt != 0).sum())} of them)")
        if int(w[WS.TIMEOUT]):
            probs.append(f"time-out counter {int(w[WS.TIMEOUT])}")
        if not bool((w[WS.TIMEOUT + 1:WS.CLUSTER_FLOATS] == WS.NAN_BITS).all()):
            probs.append("the padding behind the time-out counter was written")
        touched = w != WS.NAN_BITS
        touched[WS.COUNTERS:WS.TIMEOUT + 1] = False
        idx = touched[:self.n_ws].nonzero().flatten()
        if idx.numel() == 0:
            return (0, 0), probs
        first, last = int(idx[0]), int(idx[-1])
        if last - first + 1 != idx.numel():
            probs.append(f"workspace written with holes: {idx.numel()} floats in [{first}, {last}]")
        return (first, idx.numel()), probs


def footprint_kind(fp) -> str:
    return "fused (nothing written)" if fp[1] == 0 else f"cluster ({fp[1]} floats at the head)" if fp[0] < WS.COUNTERS else \
        f"two_kernel ({fp[1]} floats from {fp[0]})"


def run_gn_case(case: Case, backend, cluster_ok: Optional[bool] = None, fails=None):
    """Both SiLU settings: launch (twice on the GPU: same bits), footprint against the mirror, guards, every element written, the bound."""
    own = []
    cluster_ok = device_cluster_ok(backend) if cluster_ok is None else cluster_ok
    p = case.path(cluster_ok, backend.is_emu)
    want = ws_footprint(p, case.B, case.G)
    L = GnLaunch(case, backend)
    for silu in (False, True):
        tag = f"{case.name}[{backend.name}, silu={int(silu)}] mirror {p.outcome()}"
        L.reset()
        assert expect_accept_gn(case), tag
        rc = L.call(silu)
        L.sync()
        if rc != 0:
            own.append(f"{tag}: refused ({rc})")
            continue
        got, probs = L.ws_written()
        own += [f"{tag}: {m}" for m in probs]
        if got != want:
            own.append(f"{tag}: the mirror expects {footprint_kind(want)}, the library's workspace footprint is {footprint_kind(got)}")
        ok, unwritten = _window_state(L.obuf)
        if not ok or unwritten:
            own.append(f"{tag}: out guards intact={ok}, {unwritten} elements never written")
        out = L.obuf[GUARD16:GUARD16 + case.B * case.HW * case.C].clone()
        ref, bound = (sk_reference if case.sk else gn_reference)(case, silu)
        nviol, worst, at = compare(out, ref, bound)
        WORST[p.kind] = max(WORST.get(p.kind, 0.0), worst if math.isfinite(worst) else 1e30)
        print(f"{tag}: err / bound {worst:.4f}")
        if nviol:
            b, r, ch = at // (case.HW * case.C), (at // case.C) % case.HW, at % case.C
            own.append(f"{tag}: {nviol} elements beyond the bound, worst err / bound {worst:.4g} at (b {b}, row {r}, channel {ch}): "
                       f"out {float(out.flatten()[at]):.6g} ref {float(ref.flatten()[at]):.6g}")
        if case.sk:
            ok, unwritten = _window_state(L.pbuf)
            n = case.B * case.HW * case.C1
            if not ok:
                own.append(f"{tag}: pre_out guards written")
            if case.store_pre or p.kind == "two_kernel":
                pre = L.pbuf[GUARD16:GUARD16 + n].cpu().view(torch.int16)
                diff = int((pre != L.pre_expect.reshape(-1).view(torch.int16)).sum())
                if diff:
                    own.append(f"{tag}: pre_out differs from the fp32 sum in the documented order in {diff} of {n} elements")
            elif unwritten != n:
                own.append(f"{tag}: store_pre = 0 on a single-pass path, yet {n - unwritten} elements of pre_out were written")
            want_err = int(case.step is not None and "r" in case.sk_ops and not 0 <= case.step < SK_STEP_COUNT)
            if int(L.step_error.cpu()[0]) != want_err:
                own.append(f"{tag}: step_error {int(L.step_error.cpu()[0])}, expected {want_err}")
        if not backend.is_emu:                            # the rerun: the same bits
            first = (L.obuf.clone(), L.pbuf.clone())
            L.reset()
            rc = L.call(silu)
            L.sync()
            if rc != 0 or not all(torch.equal(f.view(torch.int16), b.view(torch.int16)) for f, b in zip(first, (L.obuf, L.pbuf))):
                own.append(f"{tag}: the second run (rc {rc}) differs from the first")
    if fails is None:
        assert not own, "\n".join(own)
    else:
        fails += own


def _record(backend, suffix=""):
    """GPU: the largest err / bound per path so far, to the parity record (asserted <= 1)"""
    if backend.is_emu:
        return
    from tests import parity_record
    for path, w in WORST.items():
        parity_record.check(f"norm_conformance_{path}{suffix}_err_over_bound", w, 1.0)


@pytest.mark.parametrize("name", [c.name for c in SMALL])
def test_groupnorm_small(backend, name):
    run_gn_case(CASES[name], backend)
    _record(backend)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in LARGE])
def test_groupnorm_large(gpu_backend, name):
    run_gn_case(CASES[name], gpu_backend)
    _record(gpu_backend)


# split-K source: the four-way unrolled slab loop and its tail, every operand present and absent, the step counter inside and outside its range
SK_OPS = ("brv", "", "b", "r", "v", "rv")
SK_CASES = tuple(Case(f"sk{S}-{SK_OPS[i] or 'none'}", 2, 37, 48, 16 * (i % 2), 8, sk=S, sk_ops=SK_OPS[i], store_pre=int(i != 2),
                      step=(None, None, None, 1, None, 5)[i], eps=(1e-5, 1e-6)[i % 2])
                 for i, S in enumerate((2, 3, 4, 5, 8, 9))) + (
    Case("sk3-step-negative", 2, 37, 48, 0, 8, sk=3, sk_ops="br", step=-3),
    Case("sk5-step-last", 1, 60, 512, 0, 1, sk=5, sk_ops="r", step=2, store_pre=0),
    Case("sk4-two-kernel-store0", 2, 50, 24, 0, 8, sk=4, sk_ops="rv", step=0, store_pre=0),     # the two-kernel path writes pre_out regardless
)


@pytest.mark.parametrize("case", SK_CASES, ids=lambda c: c.name)
def test_splitk_source(backend, case):
    run_gn_case(case, backend)
    _record(backend)


# ------------------------------------------------------------------------------------------------ 5. the bound bites
def _interior_row(case: Case):
    """an interior row at an edge of the schedule (a chunk edge where the path has chunks); any interior row otherwise; None: HW < 3"""
    if case.HW < 3:
        return None
    edges = set()
    for cluster_ok, is_emu in ((True, False), (False, True)):
        p = case.path(cluster_ok, is_emu)
        if p.kind != "fused":
            edges |= {ch * p.rows_per_chunk for ch in range(1, p.S or p.nchunk) if ch * p.rows_per_chunk < case.HW - 1}
    edges = edges or (boundary_rows(case.path(True, False), case.HW) - {0, case.HW - 1})
    return min(edges) if edges else case.HW // 2


def gn_mutations(case: Case, x):
    """name -> (mean, var, eps) of the deliberately wrong statistics, or a str: why the mutation cannot apply to this case"""
    B, HW, G = case.B, case.HW, case.G
    mu, var = gn_stats(x, G)
    rows = list(range(HW))
    m = {}
    m["no_last_row"] = gn_stats(x, G, rows[:-1]) + (case.eps,) if HW > 1 else "HW = 1: no row would be left"
    m["no_first_row"] = gn_stats(x, G, rows[1:]) + (case.eps,) if HW > 1 else "HW = 1: no row would be left"
    r = _interior_row(case)
    m["row_twice"] = gn_stats(x, G, rows + [r]) + (case.eps,) if r is not None else "HW < 3: no interior row"
    m["next_group"] = (mu.roll(-1, 1), var.roll(-1, 1), case.eps) if G > 1 else "one group"
    m["next_batch"] = (mu.roll(-1, 0), var.roll(-1, 0), case.eps) if B > 1 else "B = 1"
    m["no_eps"] = (mu, var, 0.0) if case.flavour in ("const", "zeros") else "no slab of variance 0"
    return m


BITE_CASES = tuple(CASES.values()) + SK_CASES[:2]


@pytest.mark.parametrize("part", range(8))
def test_tolerance_bites(part):
    """CPU only, no kernel: for every case the correctly rounded fp64 result passes the comparison and the correctly rounded result of every
    wrong set of statistics FAILS it.  A mutation that cannot apply to a case says why; no case escapes all of them."""
    fails = []
    for case in BITE_CASES[part::8]:
        silu = len(case.name) % 2 == 1
        if case.sk:
            src = sk_source(case)
            x, gamma, beta = src["x"], src["gamma"], src["beta"]
        else:
            x, gamma, beta = gn_operands(case)
        ref, bound = _gn_reference_of(x, gamma, beta, case.G, case.eps, silu)
        nviol, worst, _ = compare(ref.to(BF16), ref, bound)
        if nviol:
            fails.append(f"{case.name}: the correctly rounded result has {nviol} violations (err / bound {worst:.4g})")
        applied = 0
        for name, mut in gn_mutations(case, x).items():
            if isinstance(mut, str):
                continue
            applied += 1
            y, _ = gn_eval(x, gamma, beta, case.G, mut[0], mut[1], mut[2], silu)
            nviol, worst, _ = compare(y.to(BF16), ref, bound)
            if nviol == 0:
                fails.append(f"{case.name}: '{name}' passes the comparison (err / bound {worst:.4g})")
        if applied == 0:
            fails.append(f"{case.name}: no mutation applies")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 8. return codes
def expect_accept_gn(case: Case, **o) -> bool:
    """the ``return -1`` lines of pcdm_groupnorm / pcdm_groupnorm_splitk; ``o`` as in ``GnLaunch.call``"""
    C1, C2, B, HW, G = (o.get(k, getattr(case, k)) for k in ("C1", "C2", "B", "HW", "G"))
    Cc = C1 + C2
    if B <= 0 or HW <= 0 or G <= 0 or G > 256 or o.get("y", 1) in (None, 0) or o.get("ws", 1) in (None, 0):
        return False
    if C1 % 8 or C2 % 8 or Cc % G or Cc > WS.MAX_C or (C2 > 0 and o.get("x2", 1 if case.C2 else None) is None):
        return False
    if not case.sk:
        return o.get("x1", 1) is not None
    if o.get("null_src") or o.get("sp_part", 1) is None or o.get("sp_pre_out", 1) is None or C1 <= 0:
        return False
    src = sk_source(case)
    S, Npad, M = o.get("sp_split_k", case.sk), o.get("sp_Npad", src["Npad"]), o.get("sp_M", case.B * case.HW)
    if S < 2 or S > 64 or Npad < C1 or Npad % 8 or M != B * HW:
        return False
    if src["rowvec"] is not None and (o.get("sp_ldrv", src["ldrv"]) % 4 or o.get("sp_rowvec", 0) & 15 or
                                      (case.step is not None and o.get("sp_rowvec_step_stride", 0) % 4)):
        return False
    if o.get("sp_bias", 0) & 15 or (src["residual"] is not None and (o.get("sp_ldr", src["ldr"]) < C1 or o.get("sp_ldr", src["ldr"]) % 8)):
        return False
    if case.step is not None and src["rowvec"] is not None and (o.get("sp_rowvec_step_count", SK_STEP_COUNT) < 0 or o.get("sp_step_error", 0) & 3):
        return False
    return True


def _assert_refused(L: GnLaunch, what: str, fails: list, **over):
    if expect_accept_gn(L.case, **over):
        fails.append(f"{what}: the predicate accepts it")
    L.reset()
    before = (L.obuf.clone(), L.pbuf.clone(), L.ws.clone())
    rc = L.call(True, **over)
    L.sync()
    if rc != -1:
        fails.append(f"{what}: rc {rc}, expected -1")
    for name, a, b in zip(("out", "pre_out", "ws"), before, (L.obuf, L.pbuf, L.ws)):
        if not torch.equal(a.view(torch.int16), b.view(torch.int16)):
            fails.append(f"{what}: the refused call wrote {name}")


def test_groupnorm_refusals(backend):
    fails = []
    L = GnLaunch(Case("refuse-plain", 2, 37, 48, 16, 8), backend)
    for what, over in (("C1 % 8", dict(C1=44, C2=16, G=4)), ("C2 % 8", dict(C1=48, C2=12, G=4)), ("C % groups", dict(G=7)), ("groups > 256", dict(G=512)),
                       ("x2 missing", dict(x2=None)), ("x1 missing", dict(x1=None)), ("y missing", dict(y=None)), ("ws missing", dict(ws=None)),
                       ("B = 0", dict(B=0)), ("HW = 0", dict(HW=0)), ("groups = 0", dict(G=0)), ("C > 4096", dict(C1=4096, C2=16, G=8))):
        _assert_refused(L, "pcdm_groupnorm, " + what, fails, **over)
    L = GnLaunch(Case("refuse-sk", 2, 37, 48, 16, 8, sk=3, step=1), backend)
    src = sk_source(L.case)
    for what, over in (("split_k = 1", dict(sp_split_k=1)), ("split_k = 65", dict(sp_split_k=65)), ("Npad < C1", dict(sp_Npad=40)),
                       ("Npad % 8", dict(sp_Npad=src["Npad"] + 4)), ("M != B * HW", dict(sp_M=2 * 37 - 1)), ("M != B * HW (HW)", dict(HW=36)),
                       ("row vector misaligned", dict(sp_rowvec=L.rowvec.data_ptr() + 4)), ("ldrv % 4", dict(sp_ldrv=src["ldrv"] + 2)),
                       ("step stride % 4", dict(sp_rowvec_step_stride=2 * src["ldrv"] + 2)), ("bias misaligned", dict(sp_bias=L.bias.data_ptr() + 4)),
                       ("ldr < C1", dict(sp_ldr=40)), ("ldr % 8", dict(sp_ldr=src["ldr"] + 4)), ("step count < 0", dict(sp_rowvec_step_count=-1)),
                       ("step_error misaligned", dict(sp_step_error=L.step_error.data_ptr() + 2)), ("part missing", dict(sp_part=None)),
                       ("pre_out missing", dict(sp_pre_out=None)), ("no source", dict(null_src=True)), ("C1 % 8", dict(sp_N=44)),
                       ("C % groups", dict(G=7)), ("groups > 256", dict(G=512)), ("x2 missing", dict(x2=None)), ("C > 4096", dict(sp_N=4088, sp_Npad=4096))):
        if "sp_N" in over:
            over["C1"] = over["sp_N"]
        _assert_refused(L, "pcdm_groupnorm_splitk, " + what, fails, **over)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 9. LayerNorm
LN_FIXED = {320: (8, 5), 640: (16, 5), 1280: (32, 5), 768: (32, 3), 1536: (64, 3), 2048: (64, 4)}     # C -> (lanes per row, octets per lane)
LN_WIDTHS = tuple(LN_FIXED) + (8, 64, 512, 520, 1528) + (1544, 2056, 4096)


def ln_instance(Cc: int):
    """the switch of pcdm_layernorm: (instantiation, rows per block)"""
    if Cc in LN_FIXED:
        lpr, opl = LN_FIXED[Cc]
        assert 8 * lpr * opl == Cc
        return f"rows<{lpr},{opl}>", (WS.THREADS // 64) * (64 // lpr)
    return ("generic<3>" if Cc <= 1536 else "generic<8>"), WS.THREADS // 64


def ln_rows(Cc: int):
    rpb = ln_instance(Cc)[1]
    return tuple(sorted({1, rpb - 1, rpb, rpb + 1, 2 * rpb + 3} - {0}))


def expect_accept_ln(rows: int, Cc: int, x=1, y=1) -> bool:
    return not (x is None or y is None or rows <= 0 or Cc % 8 or Cc > 4096 or Cc <= 0)


@functools.lru_cache(maxsize=None)
def ln_operands(rows: int, Cc: int):
    """every row its own mean and scale; the row before the last constant, the last at +50 sigma (where there are that many rows)"""
    gen = torch.Generator().manual_seed(5000 + 7 * rows + Cc)
    ri = torch.arange(rows)
    mean_r = torch.where(ri % 2 == 0, 1.0, -1.0).double() * (1.0 + 8.0 * _frac(ri, 0.6180339887))
    spread_r = 2.0 ** (-2.0 + 4.0 * _frac(ri, 0.7548776662))
    if rows >= 2:
        mean_r[rows - 1] += 50.0 * spread_r[rows - 1]
    x = torch.randn(rows, Cc, generator=gen, dtype=torch.float64) * spread_r.view(rows, 1) + mean_r.view(rows, 1)
    x[:, Cc - 8:] *= 4.0                                 # the last octet: the edge of every instantiation's column loop
    if rows >= 3:
        x[rows - 2] = -2.71875
    ci = torch.arange(Cc)
    gamma = (0.5 + 1.5 * _frac(ci, 0.6180339887)) * torch.where(ci % 5 == 3, -1.0, 1.0).double()
    beta = 6.0 * (_frac(ci, 0.7548776662) - 0.5)
    return x.to(BF16).double(), gamma.to(BF16).double(), beta.to(BF16).double()


def ln_eval(x, gamma, beta, mu, var, eps):
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mu) * rstd * gamma + beta
    return y, U * y.abs() + K_LN * V * ((x.abs() + mu.abs()) * rstd * gamma.abs() + beta.abs())


def ln_reference(rows, Cc, eps):
    x, gamma, beta = ln_operands(rows, Cc)
    return ln_eval(x, gamma, beta, x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True), eps)


@pytest.mark.parametrize("Cc", LN_WIDTHS)
def test_layernorm_widths(backend, Cc):
    """every fixed-width instantiation and both generic ones, at 1, rpb - 1, rpb, rpb + 1 and 2 rpb + 3 rows"""
    fails, dev = [], backend.device
    eps = 1e-5 if Cc % 16 else 1e-6
    for rows in ln_rows(Cc):
        tag = f"layernorm C {Cc} ({ln_instance(Cc)[0]}) rows {rows} [{backend.name}]"
        x, gamma, beta = ln_operands(rows, Cc)
        xd, gd, bd = x.to(BF16).to(dev), gamma.float().to(dev), beta.float().to(dev)
        ref, bound = ln_reference(rows, Cc, eps)
        assert expect_accept_ln(rows, Cc)
        prev = None
        for run in range(1 if backend.is_emu else 2):
            obuf = _sent16(rows * Cc, dev)
            rc = _lib.lib().pcdm_layernorm(xd.data_ptr(), obuf[GUARD16:].data_ptr(), rows, Cc, eps, gd.data_ptr(), bd.data_ptr(), ops._stream(obuf))
            backend.sync()
            if rc != 0:
                fails.append(f"{tag}: refused ({rc})")
                break
            ok, unwritten = _window_state(obuf)
            if not ok or unwritten:
                fails.append(f"{tag}: guards intact={ok}, {unwritten} elements never written")
            if prev is not None and not torch.equal(prev.view(torch.int16), obuf.view(torch.int16)):
                fails.append(f"{tag}: the second run differs from the first")
            prev = obuf
        if rc != 0:
            continue
        nviol, worst, at = compare(prev[GUARD16:GUARD16 + rows * Cc], ref, bound)
        WORST["layernorm"] = max(WORST.get("layernorm", 0.0), worst if math.isfinite(worst) else 1e30)
        print(f"{tag}: err / bound {worst:.4f}")
        if nviol:
            fails.append(f"{tag}: {nviol} elements beyond the bound, worst err / bound {worst:.4g} at (row {at // Cc}, channel {at % Cc})")
    try:
        _record(backend)
    except AssertionError as e:
        fails.append(str(e))
    assert not fails, "\n".join(fails)


def test_layernorm_tolerance_bites():
    """CPU only: the correctly rounded result passes; the statistics of the neighbouring row, or without the last octet, FAIL"""
    fails = []
    for Cc in LN_WIDTHS:
        for rows in ln_rows(Cc):
            x, gamma, beta = ln_operands(rows, Cc)
            ref, bound = ln_reference(rows, Cc, 1e-5)
            if compare(ref.to(BF16), ref, bound)[0]:
                fails.append(f"C {Cc} rows {rows}: the correctly rounded result fails")
            mu, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
            mu8 = x[:, :Cc - 8].mean(1, keepdim=True)
            muts = {"next_row": (mu.roll(-1, 0), var.roll(-1, 0)) if rows > 1 else None,
                    # (C = 8: no octet is left, the statistics are NaN -- which the comparison refuses as it must)
                    "no_last_octet": (mu8, ((x[:, :Cc - 8] - mu8) ** 2).mean(1, keepdim=True))}
            for name, mv in muts.items():
                if mv is None:
                    continue                             # one row: it has no neighbour ('no_last_octet' applies to every case)
                y, _ = ln_eval(x, gamma, beta, mv[0], mv[1], 1e-5)
                if compare(y.to(BF16), ref, bound)[0] == 0:
                    fails.append(f"C {Cc} rows {rows}: '{name}' passes the comparison")
    assert not fails, "\n".join(fails)


def test_layernorm_refusals(backend):
    dev, fails = backend.device, []
    x = torch.zeros(4 * 4104, dtype=BF16, device=dev)
    g = torch.ones(4104, dtype=torch.float32, device=dev)
    for rows, Cc, xo, yo in ((4, 60, 1, 1), (4, 4104, 1, 1), (0, 64, 1, 1), (-1, 64, 1, 1), (4, 0, 1, 1), (4, -8, 1, 1), (4, 64, None, 1), (4, 64, 1, None)):
        obuf = _sent16(4 * 4104, dev)
        before = obuf.clone()
        assert not expect_accept_ln(rows, Cc, xo, yo)
        rc = _lib.lib().pcdm_layernorm(xo and x.data_ptr(), yo and obuf[GUARD16:].data_ptr(), rows, Cc, 1e-5, g.data_ptr(), g.data_ptr(),
                                       ops._stream(obuf))
        backend.sync()
        if rc != -1 or not torch.equal(before.view(torch.int16), obuf.view(torch.int16)):
            fails.append(f"pcdm_layernorm(rows {rows}, C {Cc}, x {xo}, y {yo}): rc {rc}, out written: {not torch.equal(before.view(torch.int16), obuf.view(torch.int16))}")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 10. the cluster switch
def _child_main() -> int:
    """``python -m tests.test_norm_conformance``: the shapes of the cluster path in this (fresh) process, whose environment decides the path"""
    from tests.conftest import Backend
    _lib.load()
    assert torch.cuda.is_available() and not _lib.is_emulator()
    backend = Backend("gpu", torch.device("cuda:0"))
    fails = []
    for name in CLUSTER_CASES:
        run_gn_case(CASES[name], backend, fails=fails)
    print("\n".join(fails))
    print("WORST " + " ".join(f"{k}={v:.4g}" for k, v in sorted(WORST.items())), flush=True)
    return 1 if fails else 0


@pytest.mark.gpu
def test_cluster_switch_off(gpu_backend):
    """PCDM_GN_CLUSTER=0 (what a partitioned device gets) is read once per process: the cluster shapes in one fresh child process, where the
    mirror with the cluster path off must name the path taken (single-pass where the slab fits, two-kernel otherwise)."""
    env = dict(os.environ, PCDM_GN_CLUSTER="0")
    p = subprocess.run([sys.executable, "-m", "tests.test_norm_conformance"], cwd=str(ROOT), env=env, timeout=600,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-6000:]}"
    from tests import parity_record
    items = next(ln for ln in p.stdout.splitlines() if ln.startswith("WORST ")).split()[1:]
    assert {i.split("=")[0] for i in items} == {"fused", "two_kernel"}, items
    for item in items:
        path, w = item.split("=")
        parity_record.check(f"norm_conformance_{path}_cluster_off_err_over_bound", float(w), 1.0)


if __name__ == "__main__":
    sys.exit(_child_main())
