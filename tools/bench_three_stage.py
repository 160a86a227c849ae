#!/usr/bin/env python3
"""BASELINE.json configs[3]: stage-1 prior + stage-2 + stage-3 refine, 352x512, 8 samples per pair, one MI355X -- every stage at its
full size with seeded random weights (no checkpoints offline), from pixels to pixels, timed per stage with HIP events.

Per pair, following the three drivers: CLIP ViT-H/14 embed of the source -> stage-1 prior (N = 1, 20 UnCLIP steps, guidance 0;
stage1_batchtest_prior_model.py:105-113) -> DINOv2-giant + ImageProjModel_p, pose canvas -> ControlNetConditioningEmbedding, VAE encode of
the [source | black] canvas -> stage-2 (N = 8 -> UNet batch 16, 50 DDIM steps, guidance 2; stage2_batchtest_inpaint_model.py:188-200) -> VAE
decode -> stage-3 on the target half of one sample (N = 4, 20 steps, guidance 2; stage3_batchtest_refined_model.py:161-171) -> uint8.

``--pick first`` (default) refines sample 0.  ``--pick best`` hands stage 3 the sample the evaluation driver would keep: stage 2 decodes to uint8 on
the device, pcdms_amd.metrics.pick_best scores the target half of every sample against a (synthetic) target image and writes the normalised best one
-- the whole hand-over stays on the device, the chosen index is read after the pair has finished.  It then times both modes, interleaved, and prints
the two per-pair times side by side.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import pcdms_amd as P  # noqa: E402
from oracle import cond as OC  # noqa: E402  (synthetic weights only)
from oracle import prior as OP  # noqa: E402
from oracle import vae as OV  # noqa: E402
from oracle.unet import UNetConfig, synth_state_dict  # noqa: E402
from tests.test_schedulers import SD21  # noqa: E402
from tests.test_unet import _kwargs  # noqa: E402


def _rand_sd(model, g):
    sd = {}
    for k, shp in model.expected_shapes().items():
        if len(shp) >= 2 and "position" not in k and "cls_token" not in k and "mask_token" not in k:
            fan = shp[1] * (shp[2] * shp[3] if len(shp) == 4 else 1)
            sd[k] = (torch.rand(shp, generator=g) * 2 - 1) / fan ** 0.5
        elif k.endswith("lambda1") or (k.endswith(".weight") and len(shp) == 1):
            sd[k] = torch.ones(shp)
        else:
            sd[k] = torch.randn(shp, generator=g) * 0.02
    return sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n2", type=int, default=8, help="stage-2 samples per pair")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--pick", choices=("first", "best"), default="first", help="which stage-2 sample stage 3 refines (best: device-side SSIM pick)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    t0 = time.time()
    clip = P.CLIPVisionModelWithProjection(); clip.load_state_dict(_rand_sd(clip, g)); clip.to(dev)
    dino = P.Dinov2Model(); dino.load_state_dict(_rand_sd(dino, g)); dino.to(dev)
    prior = P.Stage1_PriorTransformer(num_embeddings=2, embedding_dim=1024); prior.load_state_dict(OP.synth_state_dict(OP.PriorConfig(), 1)); prior.to(dev)
    iproj = P.ImageProjModel_p(1536, 768, 1024); iproj.load_state_dict(OC.synth(OC.image_proj_param_shapes(), 2, 1.0)); iproj.to(dev)
    pose_proj = P.ControlNetConditioningEmbedding(320, 3, (16, 32, 96, 256)); pose_proj.load_state_dict(OC.synth(OC.pose_param_shapes(), 3)); pose_proj.to(dev)
    vae = P.AutoencoderKL(); vae.load_state_dict(OV.synth_state_dict(OV.VAEConfig(), 4)); vae.to(dev)
    ucfg = UNetConfig()
    unet2 = P.Stage2_InapintUNet2DConditionModel(**_kwargs(ucfg)); unet2.load_state_dict(synth_state_dict(ucfg, seed=5)); unet2.to(dev)
    u3cfg = UNetConfig(in_channels=8, class_embed_type=None, projection_class_embeddings_input_dim=None)
    unet3 = P.UNet2DConditionModel(**_kwargs(u3cfg)); unet3.load_state_dict(synth_state_dict(u3cfg, seed=6)); unet3.to(dev)
    pipe1 = P.Stage1_PriorPipeline(prior).to(dev)
    pipe2 = P.Stage2_InpaintDiffusionPipeline(unet2, P.DDIMScheduler.from_config(SD21), vae=vae)
    pipe3 = P.Stage3_RefinedDiffusionPipeline(unet3, P.DDIMScheduler.from_config(SD21), vae=vae)
    load_s = time.time() - t0
    H, W = 512, 352
    s_img = (torch.rand(1, 3, H, W, generator=g) * 2 - 1).to(dev)
    pose = (torch.rand(1, 3, H, 2 * W, generator=g) * 2 - 1).to(dev)
    pix = torch.randn(1, 3, 224, 224, generator=g).to(dev)
    t_img = (torch.rand(1, H, W, 3, generator=g) * 255).to(torch.uint8).to(dev)      # the pair's target image (--pick best scores against it)
    kp_s, kp_t = torch.rand(1, 1, 36, generator=g).to(dev), torch.rand(1, 1, 36, generator=g).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

    picked = []

    def one_pair(timed, pick="first"):
        marks = [ev() for _ in range(6)]
        marks[0].record()
        s_embed = clip(pix).image_embeds.unsqueeze(1)
        pred = pipe1(s_embed=s_embed, s_pose=kp_s, t_pose=kp_t, num_images_per_prompt=1, num_inference_steps=20, generator=gen,
                     guidance_scale=0)[0].unsqueeze(1)
        marks[1].record()
        feat = iproj(dino(pix).last_hidden_state)
        st_pose_f = pose_proj(pose)
        canvas = torch.cat([s_img, -torch.ones_like(s_img)], dim=3)
        marks[2].record()
        out2 = pipe2(height=H, width=2 * W, vae_image=canvas, s_img_proj_f=feat, st_pose_f=st_pose_f, pred_t_img_embed=pred,
                     num_images_per_prompt=a.n2, guidance_scale=2.0, generator=gen, num_inference_steps=50,
                     output_type="uint8" if pick == "best" else "pt")
        marks[3].record()
        if pick == "best":    # the driver's best-SSIM sample, chosen and normalised on the device (no host copy between the stages)
            gen_t, index, _ = P.pick_best(out2.images, t_img, cand_window=(W, 0, W, H), out="normalized")
        else:
            gen_t, index = (out2.images[:1, :, :, W:] * 2 - 1).contiguous(), None          # target half of sample 0
        marks[4].record()
        out3 = pipe3(height=H, width=W, vae_gen_t_image=gen_t, s_img_proj_f=feat, num_images_per_prompt=4, guidance_scale=2.0, generator=gen,
                     num_inference_steps=20, output_type="uint8")
        marks[5].record()
        torch.cuda.synchronize()
        assert out3.images.shape == (4, H, W, 3) and torch.isfinite(out2.latents).all()
        assert out2.images.shape == ((a.n2, H, 2 * W, 3) if pick == "best" else (a.n2, 3, H, 2 * W))
        if timed and index is not None:
            picked.append(int(index.item()))
        names = ["stage1 (CLIP-H + prior, 20 steps)", "conditioning (DINOv2-g, image proj, pose embed)", f"stage2 (VAE enc, N={a.n2}, 50 DDIM, VAE dec)",
                 "glue", "stage3 (VAE enc, N=4, 20 steps, VAE dec + uint8)"]
        return {n: marks[i].elapsed_time(marks[i + 1]) for i, n in enumerate(names)}
    one_pair(False)   # packs weights, autotunes new shapes, captures the stage-2 graph
    one_pair(False)
    if a.pick == "best":
        one_pair(False, "best")
    acc, acc_best = {}, {}
    for _ in range(a.iters):
        for k, v in one_pair(True).items():
            acc[k] = acc.get(k, 0.0) + v / a.iters
        if a.pick == "best":
            for k, v in one_pair(True, "best").items():
                acc_best[k] = acc_best.get(k, 0.0) + v / a.iters
    total = sum(acc.values())
    if a.pick == "best":
        print(json.dumps(dict(metric="three-stage pair latency, stage 3 refines the best-SSIM stage-2 sample (device-side pick)",
                              refined_sample_per_pair=picked, total_ms_pick_best=round(sum(acc_best.values()), 1), total_ms_pick_first=round(total, 1),
                              per_stage_ms={k: round(v, 1) for k, v in acc_best.items()})))
    print(json.dumps(dict(metric="three-stage pair latency (BASELINE.json configs[3])", total_ms=round(total, 1),
                          stage2_images_per_s=round(a.n2 / (total * 1e-3), 3), per_stage_ms={k: round(v, 1) for k, v in acc.items()},
                          load_and_pack_s=round(load_s, 1), data="synthetic", weights="seeded random, full-size")))


if __name__ == "__main__":
    main()
