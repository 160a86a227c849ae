"""What FreeU costs: (1) per-step ms of the fused, graph-captured batch-4 352 x 512 stage-2 step with FreeU off and on, the two pipelines
called alternately on the same device; (2) ``pcdm_freeu`` alone at the two real levels (8 x 11 and 16 x 22 at UNet batch 8) against a
``torch.fft`` restatement on the same device.  Recorded (profiles/freeu_bench.json), not gated.

    python tools/bench_freeu.py [--rounds 3] [--ddim-steps 20] [--out profiles/freeu_bench.json] [--kernel-only]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FREEU = (0.9, 0.2, 1.2, 1.4)


def _events_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel_alone(dev, iters=200):
    from pcdms_amd import ops
    rows = []
    for B, H, W, C1, C2 in ((8, 8, 11, 1280, 1280), (8, 16, 22, 1280, 1280), (8, 16, 22, 1280, 640)):
        g = torch.Generator().manual_seed(0)
        h = (torch.randn(B * H * W, C1, generator=g) * 1.5 + 0.3).to(torch.bfloat16).to(dev)
        k = (torch.randn(B * H * W, C2, generator=g) * 1.5 + 0.3).to(torch.bfloat16).to(dev)
        ho, so = torch.empty_like(h), torch.empty_like(k)
        b, s = 1.2, 0.9

        def hip():
            ops.freeu(h, k, so, B, H, W, b, s, hidden_out=ho)

        def fft():   # diffusers' own form (fp32 FFT of the NCHW view) + the backbone scaling, in eager PyTorch
            x = k.view(B, H, W, C2).permute(0, 3, 1, 2).float()
            f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
            mask = torch.ones_like(x)
            mask[..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = s
            y = torch.fft.ifftn(torch.fft.ifftshift(f * mask, dim=(-2, -1)), dim=(-2, -1)).real
            so.copy_(y.permute(0, 2, 3, 1).reshape(B * H * W, C2))
            ho.copy_(h)
            ho[:, :C1 // 2] *= b
        for fn in (hip, fft):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t_hip = min(_events_ms(hip, iters) for _ in range(3))
        t_fft = min(_events_ms(fft, max(iters // 10, 5)) for _ in range(3))
        rows.append(dict(B=B, H=H, W=W, C1=C1, C2=C2, pcdm_freeu_us=round(t_hip * 1e3, 2), torch_fft_us=round(t_fft * 1e3, 2),
                         bytes_moved=int(B * H * W * (C1 + 2 * C2) * 2)))
        print(rows[-1], flush=True)
    return rows


def fused_step(dev, rounds, ddim_steps, batch):
    from bench import device_state_dict
    from oracle.pipeline import synth_inputs
    from oracle.unet import UNetConfig
    from pcdms_amd.pipeline import Stage2_InpaintDiffusionPipeline
    from pcdms_amd.schedulers import DDIMScheduler
    from pcdms_amd.unet import Stage2_InapintUNet2DConditionModel
    cfg = UNetConfig()
    height, width = 512, 352
    h, w = height // 8, 2 * width // 8
    sd = device_state_dict(cfg, 0, dev)
    pipes = {}
    for name in ("off", "on"):
        unet = Stage2_InapintUNet2DConditionModel(
            in_channels=9, block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.attention_head_dim,
            cross_attention_dim=cfg.cross_attention_dim, use_linear_projection=True, class_embed_type="projection",
            projection_class_embeddings_input_dim=cfg.projection_class_embeddings_input_dim, sample_size=64)
        unet.load_state_dict(sd)
        unet.to(dev)
        sched = DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                              clip_sample=False, set_alpha_to_one=False, steps_offset=1)
        pipes[name] = Stage2_InpaintDiffusionPipeline(unet, sched)
    pipes["on"].enable_freeu(*FREEU)
    dinp = {k: v.to(dev) for k, v in synth_inputs(cfg, h, w, batch).items()}

    def call(pipe):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lat = pipe(height=height, width=2 * width, masked_latents=dinp["masked_latents"], s_img_proj_f=dinp["s_img_proj_f"],
                   st_pose_f=dinp["st_pose_f"], pred_t_img_embed=dinp["pred_t_img_embed"], latents=dinp["latents"], num_images_per_prompt=batch,
                   guidance_scale=2.0, num_inference_steps=ddim_steps, output_type="latent").latents
        torch.cuda.synchronize()
        assert torch.isfinite(lat).all()
        return (time.perf_counter() - t0) * 1e3 / ddim_steps
    for name in ("off", "on"):          # warm-up: tuning of unseen shapes, capture
        call(pipes[name])
    ms = {"off": [], "on": []}
    for _ in range(rounds):
        for name in ("off", "on"):
            ms[name].append(call(pipes[name]))
    out = {k: dict(ms_per_step=[round(v, 4) for v in vs], median=round(statistics.median(vs), 4)) for k, vs in ms.items()}
    out["delta_ms_per_step"] = round(out["on"]["median"] - out["off"]["median"], 4)
    print(out, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ddim-steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "freeu_bench.json"))
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = dict(note="tools/bench_freeu.py on one MI355X: per-step ms = one sampling call (conditioning + captured steps) / steps, FreeU "
                    f"{FREEU} off and on called alternately; kernel: HIP-event time per call, best of 3 batches",
               device=torch.cuda.get_device_name(dev), kernel=kernel_alone(dev))
    if not args.kernel_only:
        res["fused_step"] = dict(batch=args.batch, height=512, width=352, ddim_steps=args.ddim_steps, **fused_step(dev, args.rounds, args.ddim_steps, args.batch))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(args.out)


if __name__ == "__main__":
    main()
