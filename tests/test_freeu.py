"""FreeU (arXiv 2309.11497; diffusers 0.24.0 ``apply_freeu`` / ``fourier_filter``) in the UNet schedules: the kernel, the Python and the C
schedule, the fused step and the public surface.

* **Reference.**  Always the literal ``fftn -> fftshift -> mask -> ifftshift -> ifftn(...).real`` with ``torch.fft`` in fp64 on the host
  (``_fourier``), never the closed form the kernel evaluates.
* **Kernel bounds** (derived).  The backbone is one fp32 product rounded to bf16: bit-equal to ``(x.float() * float32(b)).bfloat16()``, the upper
  half bit-equal to the input.  The skip: the kernel carries its sums and the correction in fp64, so its value before the single rounding is
  ~1e-15 from the fp64 FFT form; both round to bf16 and can differ only where the exact value sits on a rounding tie: every element within
  ONE bf16 ulp (ordinal distance <= 1) of the rounded fp64 result.  ``s`` is an fp32 argument: the reference uses the fp32-rounded value.
* **Schedule stages** are judged with the method of tests/test_schedule_conformance.py (teacher forcing, e_ref, 2 x e_ref; faults >= 4 x e_ref).

The counts of elements that are not bit-equal go to ``freeu_values.json`` in the scratch directory of a test run (next to the file of
tests/parity_record.py); ``python -m tests.test_freeu`` refreshes ``profiles/freeu_values.json`` from it.
"""
from __future__ import annotations

import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet as OU
from oracle.unet import UNetConfig, synth_state_dict, unet_forward
from pcdms_amd import _lib, ops
from pcdms_amd.unet import Stage2_InapintUNet2DConditionModel, UNet2DConditionModel
from pcdms_amd.unet_ctx import UNetContext
from tests import parity_record
from tests import test_schedule_conformance as SC
from tests import test_workspace_containment as WC
from tests.test_unet import REL_L2_TOL, _kwargs
from tests.test_workspace_containment import redzone  # noqa: F401  (fixture)

ROOT = Path(__file__).resolve().parent.parent
VALUES_OUT = parity_record.OUT.parent / "freeu_values.json"
BF = torch.bfloat16
FREEU = (0.9, 0.2, 1.2, 1.4)   # (s1, s2, b1, b2): the SD-2.1 values of the FreeU paper


def _f32(v: float) -> float:
    return float(np.float32(v))


def _fourier(x: torch.Tensor, s: float, threshold: int = 1) -> torch.Tensor:
    """diffusers 0.24.0 ``fourier_filter`` on NCHW ``x`` (fp64 or fp32), restated literally"""
    B, Cc, H, W = x.shape
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(B, Cc, H, W, dtype=x.dtype)
    cr, cc = H // 2, W // 2
    mask[..., cr - threshold:cr + threshold, cc - threshold:cc + threshold] = s
    return torch.fft.ifftn(torch.fft.ifftshift(f * mask, dim=(-2, -1)), dim=(-2, -1)).real


def _rows(x_nchw):
    B, Cc, H, W = x_nchw.shape
    return x_nchw.permute(0, 2, 3, 1).reshape(B * H * W, Cc)


def _nchw(rows, B, H, W):
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def _ordinal(t: torch.Tensor) -> torch.Tensor:
    """bf16 -> an integer that counts representable values (+0 and -0 coincide)"""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i >= 0, i, -(i & 0x7FFF))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _record(key, value):
    try:
        VALUES_OUT.parent.mkdir(exist_ok=True)
        cur = json.loads(VALUES_OUT.read_text()) if VALUES_OUT.exists() else {}
        cur[key] = value
        VALUES_OUT.write_text(json.dumps(cur, indent=0, sort_keys=True))
    except (OSError, ValueError):
        pass


# ================================================================================================ 1. the kernel against fp64
ONE_LAUNCH_MAX = 355          # pcdm.h: H * W <= 355 keeps the (image, 64-channel) slab in LDS
FALLBACK_SHAPE = (1, 4, 89, 16, 72)   # 356 pixels: the smallest plane the size rule sends to the two-launch form (4 x 89; 72 channels: a ragged chunk)
SHAPES = [(2, 8, 11, 1280, 1280), (2, 16, 22, 1280, 640), (3, 8, 8, 64, 64), (2, 3, 5, 48, 40), (1, 2, 3, 32, 32), (1, 2, 2, 32, 32),
          (2, 1, 4, 32, 32), (2, 4, 1, 32, 32), (1, 1, 1, 32, 32), FALLBACK_SHAPE]
PARAMS = [(1.4, 0.9), (1.2, 0.2), (1, 1)]


def _kernel_inputs(B, H, W, C1, C2, seed=1):
    g = torch.Generator().manual_seed(seed)
    h = (torch.randn(B * H * W, C1, generator=g) * 1.5 + 0.3).to(BF)
    k = (torch.randn(B * H * W, C2, generator=g) * 1.5 + 0.3).to(BF)
    return h, k


def _run_kernel(dev, h, k, B, H, W, b, s, inplace=False):
    nb = ops.freeu_ws_bytes(B, H, W, h.shape[1], k.shape[1])
    assert nb >= 0
    ws = torch.empty(nb, dtype=torch.uint8, device=dev) if nb else None
    hd, kd = h.to(dev).clone(), k.to(dev)
    ho, so = ops.freeu(hd, kd, torch.empty_like(kd), B, H, W, b, s, hidden_out=None if inplace else torch.empty_like(hd), ws=ws)
    assert torch.equal(_bits(kd), _bits(k)), "the skip input was written"
    return ho, so


def test_size_rule():
    """the smallest two-launch plane is the one named above"""
    from tests.emu import build_emu
    _lib.use_library(build_emu.load())
    B, H, W, C1, C2 = FALLBACK_SHAPE
    assert H * W == ONE_LAUNCH_MAX + 1 and ops.freeu_ws_bytes(B, H, W, C1, C2) > 0
    assert ops.freeu_ws_bytes(1, 5, 71, C1, C2) == 0 and ops.freeu_ws_bytes(8, 16, 22, 1280, 1280) == 0 and ops.freeu_ws_bytes(8, 8, 11, 2560, 1280) == 0


@pytest.mark.parametrize("b,s", PARAMS)
@pytest.mark.parametrize("B,H,W,C1,C2", SHAPES)
def test_kernel_vs_fp64(backend, B, H, W, C1, C2, b, s):
    dev = backend.device
    h, k = _kernel_inputs(B, H, W, C1, C2)
    ho, so = _run_kernel(dev, h, k, B, H, W, b, s)
    backend.sync()
    # backbone: exact
    want_h = h.clone()
    want_h[:, :C1 // 2] = (h[:, :C1 // 2].float() * torch.tensor(b, dtype=torch.float32)).to(BF)
    assert torch.equal(_bits(ho), _bits(want_h))
    assert torch.equal(_bits(ho[:, C1 // 2:]), _bits(h[:, C1 // 2:]))
    # skip: one bf16 ulp from the rounded fp64 FFT form
    ref = _rows(_fourier(_nchw(k.double(), B, H, W), _f32(s))).to(BF)
    dist = (_ordinal(so.cpu()) - _ordinal(ref)).abs()
    neq = int((dist != 0).sum())
    print(f"freeu B={B} {H}x{W} C1={C1} C2={C2} b={b} s={s}: {neq} of {ref.numel()} skip elements not bit-equal, worst distance {int(dist.max())} ulp")
    _record(f"{backend.name}/B={B}|H={H}|W={W}|C1={C1}|C2={C2}|b={b}|s={s}", dict(not_bit_equal=neq, elements=ref.numel(), worst_ulp=int(dist.max())))
    assert torch.isfinite(so.float()).all() and int(dist.max()) <= 1
    if (b, s) == (1, 1):
        assert torch.equal(_bits(ho), _bits(h)) and torch.equal(_bits(so), _bits(k))
    # rerun; in place; image 0 alone
    ho2, so2 = _run_kernel(dev, h, k, B, H, W, b, s, inplace=True)
    assert torch.equal(_bits(ho2), _bits(ho)) and torch.equal(_bits(so2), _bits(so))
    if B == 2:
        n = H * W
        ho1, so1 = _run_kernel(dev, h[:n].contiguous(), k[:n].contiguous(), 1, H, W, b, s)
        assert torch.equal(_bits(ho1), _bits(ho[:n])) and torch.equal(_bits(so1), _bits(so[:n]))


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,C1,C2", [SHAPES[0], SHAPES[3], FALLBACK_SHAPE])
def test_kernel_graph_replay(gpu_backend, B, H, W, C1, C2):
    dev = gpu_backend.device
    h, k = _kernel_inputs(B, H, W, C1, C2)
    b, s = 1.2, 0.2
    ho, so = _run_kernel(dev, h, k, B, H, W, b, s)
    nb = ops.freeu_ws_bytes(B, H, W, C1, C2)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev) if nb else None
    hd, kd = h.to(dev), k.to(dev)
    go, gs = torch.zeros_like(hd), torch.zeros_like(kd)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        ops.freeu(hd, kd, gs, B, H, W, b, s, hidden_out=go, ws=ws)
    for _ in range(2):
        go.zero_(), gs.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(go), _bits(ho)) and torch.equal(_bits(gs), _bits(so))


# ================================================================================================ 2. refusals
def test_refusals(backend):
    dev = backend.device
    lib = _lib.lib()
    B, H, W = 1, 2, 3
    for C1, C2 in ((12, 32), (32, 4)):
        h = torch.full((B * H * W, C1), 7.0, dtype=BF, device=dev)
        k = torch.full((B * H * W, max(C2, 8)), 7.0, dtype=BF, device=dev)
        ho, so = torch.full_like(h, 3.0), torch.full_like(k, 3.0)
        assert lib.pcdm_freeu(h.data_ptr(), ho.data_ptr(), k.data_ptr(), so.data_ptr(), B, H, W, C1, C2, 1.2, 0.9, None, ops._stream(h)) == -1
        assert lib.pcdm_freeu_ws_bytes(B, H, W, C1, C2) == -1
        backend.sync()
        assert bool((ho == 3.0).all()) and bool((so == 3.0).all()) and bool((h == 7.0).all()) and bool((k == 7.0).all())
    h = torch.zeros(B * H * W, 32, dtype=BF, device=dev)
    k = torch.zeros(B * H * W, 32, dtype=BF, device=dev)
    st = ops._stream(h)
    assert lib.pcdm_freeu(None, h.data_ptr(), k.data_ptr(), h.data_ptr(), B, H, W, 32, 32, 1.0, 1.0, None, st) == -1
    assert lib.pcdm_freeu(h.data_ptr(), h.data_ptr(), k.data_ptr(), k.data_ptr(), B, H, W, 32, 32, 1.0, 1.0, None, st) == -1    # skip_out == skip
    assert lib.pcdm_freeu(h.data_ptr(), h.data_ptr(), k.data_ptr(), torch.empty_like(k).data_ptr(), B, 0, W, 32, 32, 1.0, 1.0, None, st) == -1
    Bf, Hf, Wf, C1f, C2f = FALLBACK_SHAPE                                       # the two-launch form without its workspace
    hf, kf = (t.to(dev) for t in _kernel_inputs(*FALLBACK_SHAPE))
    assert lib.pcdm_freeu(hf.data_ptr(), hf.data_ptr(), kf.data_ptr(), torch.empty_like(kf).data_ptr(), Bf, Hf, Wf, C1f, C2f, 1.0, 0.5, None, st) == -1


# ================================================================================================ 3. the schedule stages, teacher-forced
def _level_sizes(h, w, n):
    out = [(h, w)]
    for _ in range(n - 1):
        out.append(((out[-1][0] - 1) // 2 + 1, (out[-1][1] - 1) // 2 + 1))
    return out


def freeu_plan(cfg, B, h, w, L, n0, fu, *, pose=True, phase=True) -> SC.Plan:
    """``SC.unet_plan`` with the two FreeU stages in front of every resnet of up blocks 0 and 1; that resnet's ``n1`` / ``out`` stages read them"""
    s1, s2, b1, b2 = fu
    pl = SC.unet_plan(cfg, B, h, w, L, n0, pose=pose, phase=phase)
    nlev = len(cfg.block_out_channels)
    sizes = _level_sizes(h, w, nlev)
    stages = []
    for st in pl.stages:
        m = re.fullmatch(r"(up_blocks\.([01])\.resnets\.(\d+)\.)(n1|out)", st.name)
        if m is None:
            stages.append(st)
            continue
        p, i, j, kind = m.group(1), int(m.group(2)), int(m.group(3)), m.group(4)
        hh, ww = sizes[nlev - 1 - i]
        if kind == "n1":
            x, skip = st.ins
            bs = ((b1, s1), (b2, s2))

            def f_h(P, I, q, ft, i=i, j=j):
                xx, b = I[0], bs[i][0]
                half = xx.shape[1] // 2
                if (ft == "blocks_1_2" and i == 0) or (ft == "only_j0" and j > 0):
                    return xx
                if ft == "blocks_1_2":
                    b = bs[0][0]
                y = xx.clone()
                if ft == "second_half":
                    y[:, half:] = xx[:, half:] * b
                elif ft == "all_channels":
                    y = xx * b
                else:
                    y[:, :half] = xx[:, :half] * b
                return y

            def f_s(P, I, q, ft, i=i, j=j):
                xx, (b, s) = I[0], bs[i]
                if (ft == "blocks_1_2" and i == 0) or (ft == "only_j0" and j > 0):
                    return xx
                if ft in ("s_swapped", "blocks_1_2"):
                    s = bs[1 - i][1]
                y = _fourier(xx, s, 2 if ft == "threshold_2" else 1)
                if ft == "no_dedup":       # the frequency along an axis of length 1 counted twice: twice the correction
                    y = 2 * y - xx
                if ft == "b_on_skip":
                    y[:, : y.shape[1] // 2] *= b
                return y
            fh = ["second_half", "all_channels", "only_j0"] if j > 0 else ["second_half", "all_channels"]
            fs = ["b_on_skip", "s_swapped", "threshold_2"] + (["only_j0"] if j > 0 else []) + (["no_dedup"] if 1 in (hh, ww) else [])
            fh.append("blocks_1_2"), fs.append("blocks_1_2")
            for nm, src, fn, faults in ((p + "fu_h", x, f_h, fh), (p + "fu_s", skip, f_s, fs)):
                stages.append(SC.Stage(nm, [src], fn, structural=faults))
                pl.layout[nm] = SC._rows_nchw(nm, B, hh, ww)
            st.ins = [p + "fu_h", p + "fu_s"]
        else:
            st.ins = [st.ins[0], p + "fu_h", p + "fu_s"]
        stages.append(st)
    pl.stages = stages
    return pl


def _model(backend, cfg, cls, sd):
    m = cls(**_kwargs(cfg), layers_per_block=cfg.layers_per_block)
    m.load_state_dict(sd)
    m.to(backend.device)
    return m


CASES = {"stage2": (Stage2_InapintUNet2DConditionModel, {}, True),
         "stage3": (UNet2DConditionModel, dict(in_channels=8, class_embed_type=None, projection_class_embeddings_input_dim=None), False)}


@pytest.mark.parametrize("case", list(CASES))
def test_schedule_stages(backend, case):
    """every ``fu_h`` / ``fu_s`` tap against the fp64 restatement of that stage on the product's own inputs, the resnets behind them fed the FreeU
    taps, tapped == untapped"""
    from pcdms_amd import unet as U
    cls, kw, pose = CASES[case]
    cfg = UNetConfig.tiny(**kw)
    B, h, w, L, n0 = (2, 16, 24, 5, 1) if backend.is_emu else (4, 16, 24, 10, 2)
    dev = backend.device
    sd = SC.round_weights(synth_state_dict(cfg, seed=0, random_affine=True))
    m = _model(backend, cfg, cls, sd).enable_freeu(*FREEU)
    s, e, c, p = SC._unet_inputs(cfg, B, h, w, L, n0, pose)
    tt = torch.tensor([981], dtype=torch.int64, device=dev)
    m._pack()
    x_in = ops.nchw_to_nhwc_bf16(s.to(dev), cpad=m._w["conv_in"].cin)

    def forward(taps):
        m._taps = taps
        try:
            cond = m.prepare_conditioning(B, h, w, e.to(dev), None if c is None else c.to(dev), None if p is None else p.to(dev), zero_ctx_batches=n0)
            out = m._forward_nhwc(x_in, B, h, w, tt, cond).clone()
        finally:
            m._taps = None
        backend.sync()
        return out
    plain = forward(None)
    taps: dict = {}
    out = forward(taps)
    assert torch.equal(out, plain), "the tap hook changed the result"
    pl = freeu_plan(cfg, B, h, w, L, n0, FREEU, pose=pose, phase=U.PHASE_UPSAMPLE)
    T = SC._unet_logical(pl, taps, sd, dict(sample=s, t=torch.tensor([981]), ehs=e, cl=c, pose=p))
    rows, fails = SC.compare(pl, sd, T)
    fu_rows = [r for r in rows if ".fu_" in r[0]]
    assert len(fu_rows) == 2 * 2 * (cfg.layers_per_block + 1)
    for n, a, b_, bound in fu_rows:
        print(f"{case:8s} {n:40s} e_ref {a:.3e} device {b_:.3e} bound {bound:.3e}")
    assert not fails, "\n".join(fails)


def test_faults_are_seen():
    """CPU only: each FreeU fault, applied to the reference side, moves its stage by >= 4 x e_ref.  Latents 8 x 24: the lowest level is 1 x 3, so
    the deduplication along an axis of length 1 is in the list.  (Scaling the +1 instead of the -1 frequencies is no fault: the same real part.)"""
    cfg = UNetConfig.tiny()
    B, h, w, L, n0 = 2, 8, 24, 5, 1
    sd = SC.round_weights(synth_state_dict(cfg, seed=0, random_affine=True))
    s, e, c, p = SC._unet_inputs(cfg, B, h, w, L, n0)
    pl = freeu_plan(cfg, B, h, w, L, n0, FREEU)
    raw = dict(sample=s, t=torch.tensor([981]), ehs=e, cl=c, pose=p)
    T = SC._chain(pl, sd, raw)
    seen, kinds = {}, set()
    for st in pl.stages:
        if ".fu_" not in st.name:
            continue
        ref = st.run(sd, T, torch.float64, SC.ident)
        e_ref = SC.rel(T[st.name], ref)
        for ft in st.structural:
            bad = st.run(sd, T, torch.float64, SC.ident, fault=ft)
            seen[f"{ft}@{st.name}"] = SC.rel(T[st.name], bad) / max(e_ref, 1e-300)
            kinds.add(ft)
    assert kinds == {"second_half", "all_channels", "b_on_skip", "s_swapped", "threshold_2", "blocks_1_2", "only_j0", "no_dedup"}
    low = {k: round(v, 3) for k, v in seen.items() if not v >= SC.BITE}
    print(json.dumps({k: round(v, 2) for k, v in seen.items()}, indent=0))
    assert not low, low


# ================================================================================================ 4. end to end against the oracle
def oracle_forward(sd, cfg, sample, timestep, ehs, class_labels=None, pose=None, freeu=None):
    """``oracle.unet.unet_forward`` restated from its own blocks, with the FreeU rule of diffusers 0.24.0 in the up loop (``freeu`` = (s1, s2, b1, b2))"""
    G, eps, boc, heads, L = cfg.norm_num_groups, cfg.norm_eps, cfg.block_out_channels, cfg.attention_head_dim, cfg.layers_per_block
    B = sample.shape[0]
    t = timestep if torch.is_tensor(timestep) else torch.tensor([timestep], dtype=torch.int64)
    t = (t[None] if t.dim() == 0 else t).expand(B)
    emb = OU.timestep_mlp(sd, "time_embedding.", OU._q(OU.timestep_embedding(t, boc[0], cfg.flip_sin_to_cos, cfg.freq_shift).to(sample.dtype)))
    if cfg.class_embed_type == "projection":
        emb = OU._q(emb + OU.timestep_mlp(sd, "class_embedding.", class_labels.squeeze(1)))
    x = OU._conv(sample, sd["conv_in.weight"], sd["conv_in.bias"], padding=1)
    if pose is not None:
        x = OU._q(x + pose)
    skips = [x]
    for i, typ in enumerate(cfg.down_block_types):
        for j in range(L):
            x = OU.resnet_block(sd, f"down_blocks.{i}.resnets.{j}.", x, emb, G, eps)
            if typ == "CrossAttnDownBlock2D":
                x = OU.transformer_2d(sd, f"down_blocks.{i}.attentions.{j}.", x, ehs, heads[i], G)
            skips.append(x)
        if i != len(boc) - 1:
            x = OU._conv(x, sd[f"down_blocks.{i}.downsamplers.0.conv.weight"], sd[f"down_blocks.{i}.downsamplers.0.conv.bias"], stride=2, padding=1)
            skips.append(x)
    x = OU.resnet_block(sd, "mid_block.resnets.0.", x, emb, G, eps)
    x = OU.transformer_2d(sd, "mid_block.attentions.0.", x, ehs, heads[-1], G)
    x = OU.resnet_block(sd, "mid_block.resnets.1.", x, emb, G, eps)
    rheads = list(reversed(heads))
    for i, typ in enumerate(cfg.up_block_types):
        for j in range(L + 1):
            sk = skips.pop()
            if freeu is not None and i < 2:
                s, b = freeu[i], freeu[2 + i]
                x = torch.cat([x[:, : x.shape[1] // 2] * b, x[:, x.shape[1] // 2:]], 1)
                sk = _fourier(sk, s)
            x = torch.cat([x, sk], dim=1)
            x = OU.resnet_block(sd, f"up_blocks.{i}.resnets.{j}.", x, emb, G, eps)
            if typ == "CrossAttnUpBlock2D":
                x = OU.transformer_2d(sd, f"up_blocks.{i}.attentions.{j}.", x, ehs, rheads[i], G)
        if i != len(boc) - 1:
            x = F.interpolate(x, size=tuple(skips[-1].shape[-2:]), mode="nearest")
            x = OU._conv(x, sd[f"up_blocks.{i}.upsamplers.0.conv.weight"], sd[f"up_blocks.{i}.upsamplers.0.conv.bias"], padding=1)
    x = OU._silu(OU._gn(x, G, sd["conv_norm_out.weight"], sd["conv_norm_out.bias"], eps))
    return OU._conv(x, sd["conv_out.weight"], sd["conv_out.bias"], padding=1)


# Chosen on the CPU: the random-weight tiny UNet renormalises after every convolution (61 norm layers), so the paper's (0.9, 0.2, 1.2, 1.4) moves
# the oracle's eps by 0.047 (16 x 24) / 0.071 (8 x 8) only, (6, 6, 3, 3) by 0.111 / 0.119, and these by 0.135 / 0.161: >= 4 x REL_L2_TOL = 0.1
E2E_FREEU = (-3.0, -3.0, 4.0, 4.0)


def test_end_to_end_vs_oracle(backend):
    from tests.test_unet import _inputs
    cfg = UNetConfig.tiny()
    B, h, w, L = (2, 8, 8, 5) if backend.is_emu else (4, 16, 24, 10)     # tests/test_unet.py::test_unet_tiny's configuration
    sd = synth_state_dict(cfg, seed=0, random_affine=True)
    s, e, c, p = _inputs(cfg, B, h, w, L)
    t = torch.tensor(981)
    off = unet_forward(sd, cfg, s, t, e, c, p)
    assert torch.equal(oracle_forward(sd, cfg, s, t, e, c, p), off), "the local restatement is not the oracle's forward"
    on = oracle_forward(sd, cfg, s, t, e, c, p, freeu=E2E_FREEU)
    moved = ((on - off).norm() / off.norm()).item()
    assert moved >= 4 * REL_L2_TOL, moved                                      # a no-op FreeU cannot pass below
    m = Stage2_InapintUNet2DConditionModel(**_kwargs(cfg))
    m.load_state_dict(sd)
    m.to(backend.device).enable_freeu(*E2E_FREEU)
    dev = backend.device
    out = m(s.to(dev), t.to(dev), e.to(dev), class_labels=c.to(dev), my_pose_cond=p.to(dev), return_dict=False)[0]
    backend.sync()
    rel = ((out.float().cpu() - on).norm() / on.norm()).item()
    print(f"FreeU on: product vs oracle rel-L2 {rel:.4f}; oracle on vs off {moved:.4f}")
    assert torch.isfinite(out).all() and rel <= REL_L2_TOL, rel


# ================================================================================================ 5. C schedule and fused step
def _both_schedules(backend, m, cfg, B, h, w, L, n0, pose):
    dev = backend.device
    s, e, c, p = SC._unet_inputs(cfg, B, h, w, L, n0, pose)
    t = torch.tensor([417], dtype=torch.int64, device=dev)
    cond = m.prepare_conditioning(B, h, w, e.to(dev), None if c is None else c.to(dev), None if p is None else p.to(dev), zero_ctx_batches=n0)
    x_in = ops.nchw_to_nhwc_bf16(s.to(dev), cpad=m._w["conv_in"].cin)
    py = m._forward_nhwc(x_in, B, h, w, t, cond).clone()
    ctx = UNetContext(m)
    pose_b = ctx.prepare_conditioning(B, h, w, e, c, p, zero_ctx_batches=n0)
    cs = ctx.forward(x_in, t, None, B, h, w, pose_b)
    backend.sync()
    return py, cs, ctx.workspace(B, h, w, L).numel()


@pytest.mark.parametrize("case", list(CASES))
def test_c_schedule_equals_python_schedule(backend, case):
    cls, kw, pose = CASES[case]
    topology = "two_level" if backend.is_emu else "tiny"                      # (the lane emulator: the two-level topology of the workspace tests)
    cfg = WC._unet_config(topology, **kw)
    B, h, w, L, n0 = (2, 8, 8, 5, 1) if backend.is_emu else (4, 16, 24, 9, 2)
    m = WC._unet_model(backend, cfg, cls)
    py0, cs0, ws0 = _both_schedules(backend, m, cfg, B, h, w, L, n0, pose)
    assert torch.equal(py0, cs0)
    # FreeU never enabled: the workspace total is what the parent commit's build answered (tests/golden/workspace_totals_parent.json)
    assert ws0 == WC._parent_total(f"unet_{topology}", B=B, h=h, w=w, L=L)
    m.enable_freeu(*FREEU)
    py1, cs1, ws1 = _both_schedules(backend, m, cfg, B, h, w, L, n0, pose)
    assert torch.equal(py1, cs1), (py1 - cs1).abs().max()
    assert not torch.equal(py1, py0) and ws1 > ws0
    m.enable_freeu(FREEU[0], FREEU[1], FREEU[2], 1.5)                          # one float
    py2, cs2, _ = _both_schedules(backend, m, cfg, B, h, w, L, n0, pose)
    assert torch.equal(py2, cs2) and not torch.equal(py2, py1)
    m.disable_freeu()
    py3, cs3, ws3 = _both_schedules(backend, m, cfg, B, h, w, L, n0, pose)
    assert torch.equal(py3, py0) and torch.equal(cs3, py0) and ws3 == ws0


@pytest.mark.gpu
def test_launch_count_without_freeu(gpu_backend):
    """FreeU never enabled, and enabled then disabled: the same launch list, without a FreeU launch; on: one launch per affected resnet more, plus
    the reduce launches that are no longer deferred"""
    cfg = UNetConfig.tiny()
    B, h, w, L, n0 = 4, 16, 24, 9, 2
    dev = gpu_backend.device
    m = _model(gpu_backend, cfg, Stage2_InapintUNet2DConditionModel, synth_state_dict(cfg, seed=3, random_affine=True))
    s, e, c, p = SC._unet_inputs(cfg, B, h, w, L, n0, True)
    t = torch.tensor([417], dtype=torch.int64, device=dev)
    x_in = None

    def names():
        nonlocal x_in
        cond = m.prepare_conditioning(B, h, w, e.to(dev), c.to(dev), p.to(dev), zero_ctx_batches=n0)
        if x_in is None:
            x_in = ops.nchw_to_nhwc_bf16(s.to(dev), cpad=m._w["conv_in"].cin)
        m._forward_nhwc(x_in, B, h, w, t, cond)          # (tunes unseen shapes)
        torch.cuda.synchronize()
        before = ops.LAUNCH_LOG
        ops.LAUNCH_LOG = []
        try:
            m._forward_nhwc(x_in, B, h, w, t, cond)
            torch.cuda.synchronize()
            return [r[0] for r in ops.LAUNCH_LOG]
        finally:
            ops.LAUNCH_LOG = before
    never = names()
    m.enable_freeu(*FREEU)
    on = names()
    m.disable_freeu()
    again = names()
    assert "freeu" not in never and again == never
    assert on.count("freeu") == 2 * (cfg.layers_per_block + 1) and len(on) >= len(never) + on.count("freeu")


def test_fused_step(backend, monkeypatch):
    """fused (graph-captured on the device) DDIM with FreeU on == the literal loop of the same calls under tests/test_pipeline.py's rule; toggling
    or changing one float changes the result and matches a fresh pipeline; disable_freeu() restores the bits"""
    import pcdms_amd.unet as U
    from oracle.pipeline import synth_inputs
    from pcdms_amd.pipeline import Stage2_InpaintDiffusionPipeline
    from pcdms_amd.schedulers import DDIMScheduler
    from tests.test_pipeline import _build, _call, _same_path
    from tests.test_schedulers import SD21
    monkeypatch.setattr(U, "SHARE_CFG_PREFIX", False)     # (the rule compares the two scheduler forms on identical UNet launches)
    cfg = UNetConfig.tiny()
    N, h, w, L, steps = (1, 8, 8, 4, 1) if backend.is_emu else (2, 16, 24, 9, 4)   # (the emulator captures no graph; ~10 s per forward there: one step, as tests/test_pipeline.py)
    dev = backend.device
    inp = synth_inputs(cfg, h, w, N, L_img=L)

    def fresh(fu):
        _, m = _build(backend, cfg)
        pipe = Stage2_InpaintDiffusionPipeline(m, DDIMScheduler.from_config(SD21))
        if fu is not None:
            pipe.enable_freeu(*fu)
        return pipe
    for c_schedule in ((False,) if backend.is_emu else (False, True)):
        pipe = fresh(None)
        pipe.c_schedule = c_schedule
        off = _call(pipe, inp, dev, N, steps, h, w, mode="fused")
        pipe.enable_freeu(*FREEU)
        on = _call(pipe, inp, dev, N, steps, h, w, mode="fused")
        lit = _call(pipe, inp, dev, N, steps, h, w, mode="reference")
        backend.sync()
        assert not torch.equal(on, off) and _same_path(on, lit, steps == 1)
        assert torch.equal(on, _call(fresh(FREEU), inp, dev, N, steps, h, w, mode="fused"))
        if not backend.is_emu:
            other = FREEU[:3] + (1.5,)
            pipe.enable_freeu(*other)
            on2 = _call(pipe, inp, dev, N, steps, h, w, mode="fused")
            assert not torch.equal(on2, on) and torch.equal(on2, _call(fresh(other), inp, dev, N, steps, h, w, mode="fused"))
        pipe.disable_freeu()
        assert torch.equal(_call(pipe, inp, dev, N, steps, h, w, mode="fused"), off)


# ================================================================================================ 6. the FreeU-on workspace plan
def test_workspace_plan(backend, redzone):  # noqa: F811
    lib = _lib.lib()
    topology = "two_level" if backend.is_emu else "tiny"
    B, h, w, L, n0, pose_b = 2, 7, 9, 5, 1, 1
    for rz in (0, WC.RZ):                       # the enumerator's invariants, FreeU on: aligned, dense, disjoint; "fu_s" is in the plan only then
        redzone(rz)
        with WC._unet_handle(topology) as hd:
            off_total = lib.pcdm_unet_workspace_bytes(hd, B, h, w, L)
            off_names = [n for n, _, _ in WC._entries("pcdm_unet_workspace_layout", hd, B, h, w, L)]
            assert lib.pcdm_unet_set_freeu(hd, 1, *FREEU) == 0
            total = lib.pcdm_unet_workspace_bytes(hd, B, h, w, L)
            ent = WC._entries("pcdm_unet_workspace_layout", hd, B, h, w, L)
            WC._check_layout(ent, total, rz)
            assert "fu_s" not in off_names and [n for n, _, _ in ent if n not in off_names] == ["fu_s"] and total > off_total
            assert lib.pcdm_unet_set_freeu(hd, 0, 1.0, 1.0, 1.0, 1.0) == 0
            assert lib.pcdm_unet_workspace_bytes(hd, B, h, w, L) == off_total
    redzone(0)
    # one red-zone run: every zone intact, the outputs those of the zone-0 run and of the Python schedule
    cfg = WC._unet_config(topology)
    m = WC._unet_model(backend, cfg).enable_freeu(*FREEU)
    inp = WC._unet_inputs(cfg, B, h, w, L, n0, pose_b)
    x_in, py_plain, py_table = WC._python_schedule(backend, m, inp, B, h, w, n0, False)
    c0 = WC._c_schedule(backend, UNetContext(m), x_in, inp, B, h, w, n0, False)
    redzone(WC.RZ)
    with WC.Allocs(backend.device, WC.FILL, guard=WC.RZ) as al:
        ctx = WC._ZonedContext(m)
        c1 = WC._c_schedule(backend, ctx, x_in, inp, B, h, w, n0, False)
    backend.sync()
    ws, ent, rz = ctx.zoned
    assert rz == WC.RZ and any(n == "fu_s" for n, _, _ in ent)
    WC._zones_intact(ws, ent, WC.RZ, "pcdm_unet_* with FreeU on")
    al.check()
    assert WC._same_bits(c1, c0) and WC._same_bits(c0, (py_plain, py_table))


# ================================================================================================ 7. the surface
def test_surface():
    from pcdms_amd.pipeline import PCDMsPipeline, Stage2_InpaintDiffusionPipeline, Stage3_RefinedDiffusionPipeline
    from pcdms_amd.schedulers import DDIMScheduler
    from tests.test_schedulers import SD21
    for pipe_cls, (cls, kw, _) in ((PCDMsPipeline, CASES["stage2"]), (Stage2_InpaintDiffusionPipeline, CASES["stage2"]),
                                   (Stage3_RefinedDiffusionPipeline, CASES["stage3"])):
        cfg = UNetConfig.tiny(**kw)
        unet = cls(**_kwargs(cfg))
        pipe = pipe_cls(unet, DDIMScheduler.from_config(SD21))
        assert unet._freeu is None
        pipe.enable_freeu(0.9, 0.2, 1.2, 1.4)
        assert unet._freeu == (0.9, 0.2, 1.2, 1.4)
        pipe.disable_freeu()
        assert unet._freeu is None
        gen = unet._pack_gen = getattr(unet, "_pack_gen", 0)
        unet.enable_freeu(s1=0.9, s2=0.2, b1=1.2, b2=1.4)
        assert unet._pack_gen == gen + 1                   # (captured graphs and C contexts are rebuilt)
        unet.enable_freeu(0.9, 0.2, 1.2, 1.4)
        assert unet._pack_gen == gen + 1
        unet.disable_freeu()


if __name__ == "__main__":   # refresh profiles/freeu_values.json from what the tests left in the scratch directory
    dst = ROOT / "profiles" / "freeu_values.json"
    cur = json.loads(dst.read_text()).get("cases", {}) if dst.exists() else {}
    cur.update(json.loads(VALUES_OUT.read_text()))
    dst.write_text(json.dumps(dict(note="pcdm_freeu against the fp64 FFT form rounded to bf16: skip elements that are not bit-equal and the worst "
                                        "ordinal distance (the bound is 1 ulp; recorded, not gated beyond it); emu/ = lane emulator, gpu/ = MI355X "
                                        "(tests/test_freeu.py)", cases=cur), indent=0, sort_keys=True) + "\n")
    print(dst, len(cur), "cases")
