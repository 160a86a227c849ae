"""The VAE at any latent size: the fused wide-head attention ``pcdm_attn_wide`` (one head, 64 <= d <= 512) against an fp64 reference,
its refusals, and ``AutoencoderKL`` / the pipelines that own one at latent sizes whose area is not a multiple of 64 or whose sides are odd.

Kernel tolerance as ``close(..., tol=1.5e-2)`` in tests/test_kernels.py (max error <= 1.5e-2 max|ref|) plus rel-L2 <= 1e-2.  VAE
tolerances as tests/test_vae.py states them: rel-L2 <= 3e-2 on the moments and the image; uint8 pixels: mean abs diff <= 1.5 levels,
<= 1 % of pixels off by more than 8.
"""
from __future__ import annotations

import pytest
import torch

from oracle import vae as O
from pcdms_amd import _lib, ops
from pcdms_amd.vae import AutoencoderKL

SENTINEL = 0x4B3C   # bf16 bit pattern written around the output window


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


def _attn_case(dev, B, Lq, Lk, d, seed, spike=False):
    """q, k as column views of [M, 2d] buffers (the VAE's EPI_SPLIT_VT output), vt [B, d, ldvt] with NaN in the columns >= Lk, and the
    fp64 reference.  spike: a few keys (first, middle, last) score ~30 above the rest, exercising the online rescale."""
    g = torch.Generator().manual_seed(seed)
    scale = d ** -0.5
    qbuf = torch.randn(B * Lq, 2 * d, generator=g)
    kbuf = qbuf if Lq == Lk else torch.randn(B * Lk, 2 * d, generator=g)
    v = torch.randn(B, Lk, d, generator=g)
    if spike:
        u = torch.randn(d, generator=g)
        u /= u.norm()
        qbuf[:, :d] += 3 * u
        for j in sorted({0, Lk // 2, Lk - 1}):
            kbuf.view(B, Lk, 2 * d)[:, j, d:] = u * (10 / scale)
    qbuf, kbuf, v = qbuf.bfloat16(), kbuf.bfloat16(), v.bfloat16()
    ldvt = (Lk + 7) // 8 * 8 + 8
    vt = torch.full((B, d, ldvt), float("nan"), dtype=torch.bfloat16)
    vt[:, :, :Lk] = v.transpose(1, 2)
    qd = qbuf[:, :d].double().to(dev).view(B, Lq, d)
    kd = kbuf[:, d:].double().to(dev).view(B, Lk, d)
    ref = torch.softmax(torch.einsum("bqd,bkd->bqk", qd, kd) * scale, -1) @ v.double().to(dev)
    qbuf_d = qbuf.to(dev)
    kbuf_d = qbuf_d if Lq == Lk else kbuf.to(dev)
    return qbuf_d[:, :d], kbuf_d[:, d:], vt.to(dev), ref.reshape(B * Lq, d), scale


def _window(dev, rows, d):
    """A sentinel-filled buffer and the [rows, d] window (rows 2.., columns 8..) the kernel writes; ldo = d + 24."""
    big = torch.full((rows + 5, d + 24), SENTINEL, dtype=torch.int16, device=dev).view(torch.bfloat16)
    return big, big[2:2 + rows, 8:8 + d]


def _outside_untouched(big, rows, d):
    keep = torch.ones(big.shape, dtype=torch.bool, device=big.device)
    keep[2:2 + rows, 8:8 + d] = False
    return bool((big.view(torch.int16)[keep] == SENTINEL).all())


def _check(out, ref, what):
    err, top = (out.double() - ref).abs().max().item(), ref.abs().max().item()
    assert err <= 1.5e-2 * top, (what, err, top)
    r = _rel(out, ref)
    assert r <= 1e-2, (what, r)


EMU_CASES = [  # d, B, Lq, Lk, spike
    (64, 1, 1, 1, False), (64, 2, 7, 63, False), (64, 1, 65, 65, True), (128, 1, 65, 64, False), (128, 2, 63, 130, True),
    (192, 1, 40, 100, False), (320, 1, 33, 129, True), (512, 1, 130, 7, False), (512, 1, 64, 65, True), (512, 2, 130, 130, False),
]
GPU_CASES = [  # d, B, Lq = Lk, spike
    (512, 1, 3750, False), (512, 3, 5632, True), (512, 1, 8192, False), (128, 3, 8192, True), (64, 3, 3750, False), (128, 1, 5632, False),
]


def test_attn_wide_vs_fp64(backend):
    dev = backend.device
    cases = EMU_CASES if backend.is_emu else [(d, B, L, L, sp) for d, B, L, sp in GPU_CASES]
    for i, (d, B, Lq, Lk, spike) in enumerate(cases):
        what = (d, B, Lq, Lk, spike)
        q, k, vt, ref, scale = _attn_case(dev, B, Lq, Lk, d, seed=10 + i, spike=spike)
        big, out = _window(dev, B * Lq, d)
        ops.attn_wide(q, k, vt, out, B, Lq, Lk, scale)
        backend.sync()
        assert _outside_untouched(big, B * Lq, d), what
        _check(out, ref, what)
        if not backend.is_emu:   # reruns are bit-identical
            first = out.clone()
            ops.attn_wide(q, k, vt, out, B, Lq, Lk, scale)
            backend.sync()
            assert torch.equal(first.view(torch.int16), out.view(torch.int16)), what


def test_attn_wide_refusals(backend):
    dev = backend.device
    d, B, L = 64, 1, 40
    q, k, vt, _, scale = _attn_case(dev, B, L, L, d, seed=3)
    big, out = _window(dev, B * L, d)
    lib = _lib.lib()
    strm = ops._stream(out)

    def call(d_=d, Lq=L, Lk=L, ldvt=vt.shape[-1], qp=q):
        return lib.pcdm_attn_wide(qp.data_ptr(), qp.stride(0), k.data_ptr(), k.stride(0), vt.data_ptr(), ldvt, out.data_ptr(),
                                  out.stride(0), B, Lq, Lk, d_, scale, strm)
    rcs = dict(d0=call(d_=0), d96=call(d_=96), d576=call(d_=576), lk0=call(Lk=0), lq0=call(Lq=0), ldvt_short=call(ldvt=L - 8),
               ldvt_odd=call(ldvt=L + 4), q_misaligned=call(qp=q[:, 4:]))
    backend.sync()
    assert all(rc != 0 for rc in rcs.values()), rcs
    assert _outside_untouched(big, 0, 0), "a refused call wrote to the output buffer"
    assert call() == 0   # the same arguments with nothing wrong do run
    backend.sync()


def _build(dev, cfg, seed):
    sd = O.synth_state_dict(cfg, seed)
    m = AutoencoderKL(block_out_channels=cfg.block_out_channels, layers_per_block=cfg.layers_per_block,
                      latent_channels=cfg.latent_channels, norm_num_groups=cfg.norm_num_groups)
    m.load_state_dict(sd)
    return sd, m.to(dev)


def _encode_decode_vs_oracle(backend, cfg, sd, m, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, 3, 8 * h, 8 * w, generator=g) * 2 - 1
    mom = m.encode(x.to(backend.device)).latent_dist.parameters
    backend.sync()
    assert mom.shape == (1, 8, h, w)
    r_enc = _rel(mom, O.encode_moments(sd, cfg, x))
    z = torch.randn(1, 4, h, w, generator=g)
    img = m.decode(z.to(backend.device), return_dict=False)[0]
    backend.sync()
    ref = O.decode(sd, cfg, z)
    assert img.shape == ref.shape
    r_dec = _rel(img, ref)
    u8 = m.decode_to_uint8(z.to(backend.device))
    backend.sync()
    dpx = (u8.cpu().int() - O.postprocess_uint8(ref).int()).abs().float()
    print(f"latent {h}x{w}: encode rel-L2 {r_enc:.4f}, decode rel-L2 {r_dec:.4f}, uint8 mean |diff| {dpx.mean():.3f}")
    assert r_enc <= 3e-2, (h, w, r_enc)
    assert r_dec <= 3e-2, (h, w, r_dec)
    assert dpx.mean() <= 1.5 and (dpx > 8).float().mean() <= 0.01, (h, w, dpx.mean(), (dpx > 8).float().mean())


def test_vae_tiny_ragged_latents(backend):
    """Latents whose area is not a multiple of 64 and whose sides are odd: encode moments, decoded image and uint8 pixels against
    oracle/vae.py (the mid-block attention used to refuse these with NotImplementedError)."""
    cfg = O.VAEConfig.tiny()
    sd, m = _build(backend.device, cfg, seed=7)
    sizes = [(5, 7), (11, 13)] if backend.is_emu else [(5, 7), (11, 13), (38, 25), (75, 50)]
    for i, (h, w) in enumerate(sizes):
        _encode_decode_vs_oracle(backend, cfg, sd, m, h, w, seed=20 + i)


@pytest.mark.gpu
def test_vae_no_quadratic_scratch(gpu_backend):
    """After a decode at latent 64x128 (HW = 8192, an area the old path accepted) no cached buffer is HW x HW."""
    cfg = O.VAEConfig.tiny()
    _, m = _build(gpu_backend.device, cfg, seed=1)
    img = m.decode(torch.randn(1, 4, 64, 128, generator=torch.Generator().manual_seed(0)).cuda(), return_dict=False)[0]
    torch.cuda.synchronize()
    assert img.shape == (1, 3, 512, 1024) and bool(torch.isfinite(img).all())
    HW = 64 * 128   # (every channel count of the model, x4 for the phase upsampling, is far below HW)
    quadratic = [k for k, t in m._bufs.items() if t.dim() >= 2 and t.shape[-1] >= HW and t.shape[-2] >= HW]
    assert not quadratic, quadratic


@pytest.mark.gpu
def test_vae_mid_block_peak_memory(gpu_backend):
    """A mid-block at latent 64x128 (HW = 8192, C = 512) with none of its buffers allocated yet allocates less than one fp32 HW x HW
    score matrix (256 MiB) in all.  (A first run beforehand settles what the process keeps across calls: the GEMM tile choices of unseen
    shapes and the shared split-K workspace.)"""
    cfg = O.VAEConfig()
    _, m = _build(gpu_backend.device, cfg, seed=2)
    m._pack()
    H, W, C = 64, 128, cfg.block_out_channels[-1]
    x = torch.randn(H * W, C, generator=torch.Generator().manual_seed(0)).bfloat16().cuda()
    m._mid(m._w["d.mid"], x, 1, H, W)
    m._bufs.clear()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = m._mid(m._w["d.mid"], x, 1, H, W)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"cold mid-block at HW = {H * W}: peak allocation +{grown / 2 ** 20:.1f} MiB")
    assert y.shape == (H * W, C) and bool(torch.isfinite(y.float()).all())
    assert grown < (H * W) ** 2 * 4, grown / 2 ** 20


@pytest.mark.gpu
def test_vae_full_ragged_latents(gpu_backend):
    """Full SD-2.1 VAE at latent 38x25 (canvas 304x200) and 75x50 (canvas 600x400): encode and decode against the oracle."""
    cfg = O.VAEConfig()
    sd, m = _build(gpu_backend.device, cfg, seed=3)
    for i, (h, w) in enumerate([(38, 25), (75, 50)]):
        _encode_decode_vs_oracle(gpu_backend, cfg, sd, m, h, w, seed=30 + i)


@pytest.mark.gpu
def test_vae_full_batch3_decode(gpu_backend):
    """One launch covers the whole batch: a batch-3 decode at 75x50 matches each sample's single decode, the last one the oracle."""
    cfg = O.VAEConfig()
    sd, m = _build(gpu_backend.device, cfg, seed=4)
    dev = gpu_backend.device
    z = torch.randn(3, 4, 75, 50, generator=torch.Generator().manual_seed(5))
    img3 = m.decode(z.to(dev), return_dict=False)[0]
    for b in range(3):
        one = m.decode(z[b:b + 1].to(dev), return_dict=False)[0]
        r = _rel(img3[b:b + 1], one)
        assert r <= 2e-2, (b, r)
    r_last = _rel(img3[2:], O.decode(sd, cfg, z[2:]))
    print(f"batch-3 decode at 75x50: last sample vs the oracle rel-L2 {r_last:.4f}")
    assert r_last <= 3e-2, r_last


class _FixedNoiseVAE:
    """The pipelines call vae.encode(...).latent_dist.sample(generator): inject the oracle's posterior noise."""

    def __init__(self, vae, noise):
        self.config, self._vae, self._noise = vae.config, vae, noise
        self.decode, self.decode_to_uint8 = vae.decode, vae.decode_to_uint8

    def encode(self, x):
        d = self._vae.encode(x).latent_dist
        noise = self._noise.to(x.device)
        return type("E", (), {"latent_dist": type("D", (), {"sample": staticmethod(lambda generator=None: d.sample(noise=noise))})})


@pytest.mark.gpu
def test_pipelines_with_vae_at_ragged_latents(gpu_backend):
    """vae_image -> encode -> sampling -> decode_to_uint8 at ragged latents (tiny UNets + tiny VAE) against the oracle chain, as
    tests/test_vae.py::test_pipeline_with_vae_pixels does at 16x16: stage 2 at 11x14 (154 positions), stage 3 at 9x13 (both odd)."""
    from oracle.pipeline import stage2_sample, stage3_sample, synth_inputs
    from oracle.schedulers import DDIMOracle
    from oracle.unet import UNetConfig, synth_state_dict
    from pcdms_amd import (DDIMScheduler, Stage2_InapintUNet2DConditionModel, Stage2_InpaintDiffusionPipeline,
                           Stage3_RefinedDiffusionPipeline, UNet2DConditionModel)
    from tests.test_schedulers import SD21
    from tests.test_unet import _kwargs
    dev = gpu_backend.device
    vcfg = O.VAEConfig.tiny()
    vsd, vae = _build(dev, vcfg, seed=5)
    g = torch.Generator().manual_seed(4)

    # ---- stage 2 (prior embedding), latent 11 x 14 (even width: the default mask covers it)
    ucfg = UNetConfig.tiny()
    usd = synth_state_dict(ucfg, seed=0, random_affine=True)
    unet = Stage2_InapintUNet2DConditionModel(**_kwargs(ucfg))
    unet.load_state_dict(usd)
    unet.to(dev)
    N, h, w, steps = 2, 11, 14, 4
    inp = synth_inputs(ucfg, h, w, N, L_img=7)
    vae_image = torch.rand(1, 3, h * 8, w * 8, generator=g) * 2 - 1
    post_noise = torch.randn(1, 4, h, w, generator=g)
    ml = O.sample_latents(O.encode_moments(vsd, vcfg, vae_image), post_noise) * vcfg.scaling_factor
    lat = stage2_sample(usd, ucfg, DDIMOracle(), num_images_per_prompt=N, guidance_scale=2.0, num_inference_steps=steps,
                        **dict(inp, masked_latents=ml))
    ref_u8 = O.postprocess_uint8(O.decode(vsd, vcfg, lat / vcfg.scaling_factor))
    pipe = Stage2_InpaintDiffusionPipeline(unet, DDIMScheduler.from_config(SD21), vae=_FixedNoiseVAE(vae, post_noise))
    out = pipe(height=h * 8, width=w * 8, vae_image=vae_image.to(dev), s_img_proj_f=inp["s_img_proj_f"].to(dev),
               st_pose_f=inp["st_pose_f"].to(dev), pred_t_img_embed=inp["pred_t_img_embed"].to(dev),
               latents=inp["latents"].to(dev), num_images_per_prompt=N, guidance_scale=2.0, num_inference_steps=steps,
               output_type="uint8")
    assert _rel(out.latents, lat) <= 3e-2, _rel(out.latents, lat)
    d = (out.images.cpu().int() - ref_u8.int()).abs().float()
    assert out.images.shape == (N, h * 8, w * 8, 3)
    assert d.mean() <= 2.0 and (d > 12).float().mean() <= 0.02, (d.mean(), (d > 12).float().mean())

    # ---- stage 3, latent 9 x 13
    c3 = UNetConfig.tiny(in_channels=8, class_embed_type=None, projection_class_embeddings_input_dim=None)
    sd3 = synth_state_dict(c3, seed=6, random_affine=True)
    m3 = UNet2DConditionModel(**_kwargs(c3))
    m3.load_state_dict(sd3)
    m3.to(dev)
    N3, h3, w3 = 1, 9, 13
    gen_t = torch.rand(1, 3, h3 * 8, w3 * 8, generator=g) * 2 - 1
    post3 = torch.randn(1, 4, h3, w3, generator=g)
    feat = torch.randn(1, 7, c3.cross_attention_dim, generator=g)
    lat3 = torch.randn(N3, 4, h3, w3, generator=g)
    gl = O.sample_latents(O.encode_moments(vsd, vcfg, gen_t), post3) * vcfg.scaling_factor
    o_lat3 = stage3_sample(sd3, c3, DDIMOracle(), gen_t_img_latents=gl, s_img_proj_f=feat, latents=lat3, num_images_per_prompt=N3,
                           guidance_scale=2.0, num_inference_steps=3)
    o_u8 = O.postprocess_uint8(O.decode(vsd, vcfg, o_lat3 / vcfg.scaling_factor))
    pipe3 = Stage3_RefinedDiffusionPipeline(m3, DDIMScheduler.from_config(SD21), vae=_FixedNoiseVAE(vae, post3))
    out3 = pipe3(height=h3 * 8, width=w3 * 8, vae_gen_t_image=gen_t.to(dev), s_img_proj_f=feat.to(dev), latents=lat3.to(dev),
                 num_images_per_prompt=N3, guidance_scale=2.0, num_inference_steps=3, output_type="uint8")
    assert _rel(out3.latents, o_lat3) <= 3e-2, _rel(out3.latents, o_lat3)
    d3 = (out3.images.cpu().int() - o_u8.int()).abs().float()
    assert out3.images.shape == (N3, h3 * 8, w3 * 8, 3)
    assert d3.mean() <= 2.0 and (d3 > 12).float().mean() <= 0.02, (d3.mean(), (d3 > 12).float().mean())
