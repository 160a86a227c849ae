"""Stage-2 pose-conditioned inpainting sampler on the MI355X.

Mirrors ``Stage2_InpaintDiffusionPipeline.__call__``
(/root/reference/src/pipelines/stage2_inpaint_pipeline.py:389-541): same keyword arguments, same
conditioning assembly (:430-466), same loop body (:496-519).  Two execution modes over the same
kernels:

* ``mode="reference"`` -- literally the reference's loop: ``cat`` inputs, ``self.unet(...)``,
  CFG combine, ``self.scheduler.step(...)`` with any scheduler object (UniPC / DDIM / DDPM / DPM-Solver++ /
  Euler / Euler-ancestral / LMS / PNDM).
* ``mode="fused"`` (default for DDIM with eta = 0, for UniPC, the shipped driver's scheduler, for DPM-Solver++ in both its
  ODE ("DPM++ 2M") and SDE forms, and for Euler, Euler-ancestral, LMS and PNDM: all are per-step LINEAR updates with host-known
  coefficients; the noise of the stochastic ones is drawn up front into a per-step table) -- per step: ``pcdm_assemble_input``
  (``pcdm_assemble_input_ex`` with the step's ``scale_model_input`` factor for the sigma-space samplers) -> UNet schedule ->
  ``pcdm_cfg_step`` / ``pcdm_unipc_step`` / ``pcdm_dpmpp_step`` / ``pcdm_multistep_step`` (CFG + scheduler update from a device-side
  coefficient table; multistep history lives in static slots) -> ``pcdm_advance_step``; the step is captured once in a hipGraph and
  replayed ``len(scheduler.timesteps)`` times (PNDM: ``num_inference_steps + 1``; the step index lives in device memory), which
  removes ~700 host launches per step from the critical path.

VAE encode/decode are outside the hot path: pass ``masked_latents``
(= vae.encode(vae_image).sample * scaling_factor, ref :443-444) and read ``output.latents``.
"""
from __future__ import annotations

import inspect
from dataclasses import dataclass
from typing import Any, Callable, List, Optional, Union

import torch

from . import ops
from .schedulers import (DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler, _step_noise,
                         _TableStepScheduler)
from .unet import Stage2_InapintUNet2DConditionModel


@dataclass
class Stage2_InpaintDiffusionPipelineOutput:
    images: Any
    nsfw_content_detected: Optional[List[bool]] = None
    latents: Optional[torch.Tensor] = None


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    """ref :52-63 (inactive in the reference driver, which passes guidance_rescale=0.0,
    stage2_batchtest_inpaint_model.py:191).  One HIP kernel: per-sample std matching + mix."""
    a, b = noise_cfg.float().contiguous(), noise_pred_text.float().contiguous()
    return ops.rescale_noise_cfg(a, b, torch.empty_like(a), guidance_rescale).to(noise_cfg.dtype)


def retrieve_timesteps(scheduler, num_inference_steps: Optional[int] = None, device=None, timesteps: Optional[List[int]] = None,
                       **kwargs):
    """``retrieve_timesteps`` of the notebook pipeline (ref src/pipelines/PCDMs_pipeline.py:190-231): calls
    ``scheduler.set_timesteps`` and returns ``(scheduler.timesteps, num_inference_steps)``; a custom ``timesteps`` list is passed
    on only to schedulers whose ``set_timesteps`` has a ``timesteps`` parameter, anything else is a ``ValueError`` (same message)."""
    if timesteps is not None:
        if "timesteps" not in set(inspect.signature(scheduler.set_timesteps).parameters.keys()):
            raise ValueError(f"The current scheduler class {scheduler.__class__}'s `set_timesteps` does not support custom"
                             f" timestep schedules. Please check whether you are using the correct scheduler.")
        scheduler.set_timesteps(timesteps=timesteps, device=device, **kwargs)
        timesteps = scheduler.timesteps
        num_inference_steps = len(timesteps)
    else:
        scheduler.set_timesteps(num_inference_steps, device=device, **kwargs)
        timesteps = scheduler.timesteps
    return timesteps, num_inference_steps


class Stage2_InpaintDiffusionPipeline:
    #: False in ``Simple_Stage2_InpaintDiffusionPipeline`` (ref :544-887): no stage-1 embedding, i.e. no class_labels and
    #: only the 257 projected source-image tokens as context
    use_prior_embed = True

    def __init__(self, unet: Stage2_InapintUNet2DConditionModel, scheduler, vae=None, c_schedule: bool = False):
        self.unet = unet
        self.scheduler = scheduler
        self.vae = vae
        self.vae_scale_factor = 8
        #: run the UNet of the fused step through the single C entry ``pcdm_unet_forward`` (include/pcdm.h; pcdms_amd/unet_ctx.py)
        #: instead of the Python schedule of ctypes calls: bit-identical results, one call per step
        self.c_schedule = c_schedule
        self._ctx = None
        self._graph = None
        self._graph_key = None
        self._st = {}

    #: the stock UNet class a pipeline directory holds (the drivers replace ``pipe.unet`` right after ``from_pretrained``)
    _unet_kwargs: dict = {}

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, torch_dtype=None, **kwargs):
        """``Stage2_InpaintDiffusionPipeline.from_pretrained(sd21_dir, torch_dtype=...)`` as the drivers call it
        (/root/reference/stage2_batchtest_inpaint_model.py:123): loads ``vae/`` and ``unet/`` (stock SD UNet; the driver then
        assigns its own ``pipe.unet`` / ``pipe.scheduler``, :125-132) and builds a scheduler from
        ``scheduler/scheduler_config.json``, by class name.  SD-2.1 ships a PNDM config (``skip_prk_steps=True``): the pipeline
        then holds a ``PNDMScheduler``, as the reference's does.  A class name that ``pcdms_amd.schedulers`` does not have
        still becomes a ``DDIMScheduler`` with the shared keys.
        Text encoder / tokenizer / safety checker of the directory are not used by the stage-2 call and are not loaded."""
        import json
        from pathlib import Path

        from . import schedulers as S
        from .unet import UNet2DConditionModel
        from .vae import AutoencoderKL
        root = Path(str(pretrained_model_name_or_path))
        vae = AutoencoderKL.from_pretrained(root, subfolder="vae", torch_dtype=torch_dtype) if (root / "vae").is_dir() else None
        unet = UNet2DConditionModel.from_pretrained(root, subfolder="unet", torch_dtype=torch_dtype, **cls._unet_kwargs)
        scfg = {}
        sj = root / "scheduler" / "scheduler_config.json"
        if sj.exists():
            scfg = json.loads(sj.read_text())
        sched_cls = getattr(S, str(scfg.get("_class_name", "")), None)
        if not (isinstance(sched_cls, type) and issubclass(sched_cls, S._Base)):
            sched_cls = S.DDIMScheduler
        return cls(unet, sched_cls.from_config(scfg), vae=vae)

    @property
    def device(self):
        return self.unet.device

    _execution_device = device

    def to(self, device):
        self.unet.to(device)
        if self.vae is not None and hasattr(self.vae, "to"):
            self.vae.to(device)
        return self

    def enable_xformers_memory_efficient_attention(self, attention_op=None):
        self.unet.set_use_memory_efficient_attention_xformers(True, attention_op)

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """``pipe.enable_freeu(s1, s2, b1, b2)`` of the reference's pipelines (src/pipelines/PCDMs_pipeline.py:744-762): forwarded to ``self.unet``.
        The state is part of what a captured step depends on: changing it re-captures (``_run_fused``)."""
        if not hasattr(self.unet, "enable_freeu"):
            raise ValueError("The pipeline must have `unet` for using FreeU.")
        self.unet.enable_freeu(s1=s1, s2=s2, b1=b1, b2=b2)

    def disable_freeu(self):
        """ref src/pipelines/PCDMs_pipeline.py:765-768."""
        self.unet.disable_freeu()

    def prepare_extra_step_kwargs(self, generator, eta):
        """ref :307-322."""
        params = set(inspect.signature(self.scheduler.step).parameters.keys())
        kw = {}
        if "eta" in params:
            kw["eta"] = eta
        if "generator" in params:
            kw["generator"] = generator
        return kw

    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        """ref :371-387."""
        shape = (batch_size, num_channels_latents, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an "
                             f"effective batch size of {batch_size}.")
        if latents is None:
            gdev = generator.device if isinstance(generator, torch.Generator) else device
            latents = torch.randn(shape, generator=generator, device=gdev, dtype=torch.float32).to(device)
        else:
            latents = latents.to(device)
        return latents.to(dtype) * self.scheduler.init_noise_sigma

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, prompt=None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, negative_prompt=None,
                 num_images_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None,
                 latents: Optional[torch.Tensor] = None, prompt_embeds=None, negative_prompt_embeds=None,
                 output_type: Optional[str] = "pil", return_dict: bool = True,
                 callback: Optional[Callable[[int, int, torch.Tensor], None]] = None, callback_steps: int = 1,
                 cross_attention_kwargs=None, guidance_rescale: float = 0.0,
                 vae_image: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                 s_img_proj_f: Optional[torch.Tensor] = None, st_pose_f: Optional[torch.Tensor] = None,
                 pred_t_img_embed: Optional[torch.Tensor] = None,
                 # extensions
                 masked_latents: Optional[torch.Tensor] = None, mode: Optional[str] = None, use_graph: bool = True):
        if prompt is not None or prompt_embeds is not None or negative_prompt is not None:
            raise NotImplementedError("text prompts are not part of the stage-2 path (dead code in the reference, :245-291)")
        device = self.device
        if height % 8 or width % 8:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        bs, num, _ = s_img_proj_f.shape
        N = num_images_per_prompt
        h, w = height // 8, width // 8
        do_cfg = guidance_scale > 1.0
        rep = 2 if do_cfg else 1
        f32 = dict(device=device, dtype=torch.float32)

        # ---- conditioning (ref :430-466); sample index = pair*N + k, CFG layout [uncond(all); cond(all)]
        if masked_latents is None:
            if self.vae is None:
                raise ValueError("pass masked_latents=... (VAE encode is outside the hot path) or construct with vae=")
            masked_latents = self.vae.encode(vae_image.to(device)).latent_dist.sample(generator=generator)
            masked_latents = masked_latents * self.vae.config.scaling_factor
        masked = masked_latents.to(**f32).repeat_interleave(N, 0).repeat(rep, 1, 1, 1).contiguous() if bs > 1 \
            else masked_latents.to(**f32).contiguous()                      # bs == 1: batch-broadcast in the kernel
        if mask is None:
            mask = torch.cat([torch.ones(bs, 1, h, w // 2), torch.zeros(bs, 1, h, w // 2)], dim=3)
        mask = mask.to(**f32).repeat_interleave(N, 0).repeat(rep, 1, 1, 1).contiguous() if bs > 1 \
            else mask.to(**f32).contiguous()
        pose = st_pose_f.to(**f32)
        pose_cond = pose.repeat_interleave(N, 0).repeat(rep, 1, 1, 1).contiguous() if bs > 1 else pose.contiguous()
        if self.use_prior_embed:
            feature_f = torch.cat([s_img_proj_f.to(**f32), pred_t_img_embed.to(**f32)], dim=1).repeat_interleave(N, 0)
            prior_embed = pred_t_img_embed.to(**f32).repeat_interleave(N, 0)
        else:
            feature_f = s_img_proj_f.to(**f32).repeat_interleave(N, 0)
            prior_embed = None
        if do_cfg:
            feature_f = torch.cat([torch.zeros_like(feature_f), feature_f], dim=0)
            if prior_embed is not None:
                prior_embed = torch.cat([torch.zeros_like(prior_embed), prior_embed], dim=0)
        feature_f = feature_f.contiguous()
        if prior_embed is not None:
            prior_embed = prior_embed.contiguous()

        # ---- timesteps, latents (ref :472-487)
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        timesteps = self.scheduler.timesteps
        lat = self.prepare_latents(bs * N, 4, height, width, torch.float32, device, generator, latents).contiguous()
        extra = self.prepare_extra_step_kwargs(generator, eta)

        lat = self._sample(lat, mask, masked, pose_cond, feature_f, prior_embed, timesteps, do_cfg, guidance_scale, guidance_rescale,
                           eta, extra, mode, use_graph, callback, callback_steps, zero_uncond=do_cfg,   # uncond context = literal zeros (:457-458)
                           shared_halves=do_cfg)   # latents doubled (:499), one mask / masked latents / pose for both CFG halves (:430-459)

        images = self._postprocess(lat, output_type)
        if not return_dict:
            return (images, None)
        return Stage2_InpaintDiffusionPipelineOutput(images=images, nsfw_content_detected=None, latents=lat)

    def _sample(self, lat, mask, masked, pose_cond, feature_f, prior_embed, timesteps, do_cfg, guidance_scale, guidance_rescale, eta,
                extra, mode, use_graph, callback, callback_steps, zero_uncond=False, shared_halves=False):
        """The denoise loop on prepared (CFG-doubled) conditioning: fused + hipGraph for DDIM, the reference's literal loop otherwise.
        ``zero_uncond``: the unconditional half of ``feature_f`` is literal zeros (the UNet then skips that half of every cross-attention).
        ``shared_halves``: mask / masked latents / pose of the two CFG halves are the same tensors repeated (the UNet then runs conv_in,
        the first norm1 and the first conv1's contraction once for both: ``prepare_conditioning(shared_cfg_input=True)``)."""
        linear = isinstance(self.scheduler, (DDIMScheduler, DDPMScheduler)) and eta == 0.0 \
            and not isinstance(self.scheduler, DDPMScheduler)
        # UniPC (ref stage2_batchtest_inpaint_model.py:132): multistep, but still one linear map per step on static state slots
        linear = linear or (isinstance(self.scheduler, UniPCMultistepScheduler) and self.scheduler.config.solver_order <= 2)
        # DPM-Solver++ (ODE and SDE form): linear in (x, eps, m1, noise); the SDE noise comes from a per-call table of the same draws
        linear = linear or isinstance(self.scheduler, DPMSolverMultistepScheduler)
        # Euler / Euler-ancestral / LMS / PNDM: linear in (x, a saved sample, eps and its history, noise) on five static slots
        linear = linear or isinstance(self.scheduler, _TableStepScheduler)
        mode = mode or ("fused" if linear else "reference")
        if mode == "fused" and not linear:
            raise ValueError("mode='fused' needs a scheduler with one linear update per step (DDIM with eta=0, UniPC, DPM-Solver++, Euler, Euler-ancestral, LMS, PNDM)")

        if mode == "reference":
            # the literal loop: bare unet(...) calls.  The UNet recognises the step-invariant tensors by identity (it keeps
            # them alive while cached); drop whatever an earlier call left behind, and our references on the way out
            self.unet.invalidate_caches()
            for i, t in enumerate(timesteps):
                x = torch.cat([lat] * 2) if do_cfg else lat
                x = self.scheduler.scale_model_input(x, t)
                B = x.shape[0]
                inp = torch.cat([x] + ([] if mask is None else [mask.expand(B, -1, -1, -1)]) + [masked.expand(B, -1, -1, -1)], dim=1)
                eps = self.unet(inp, t, class_labels=prior_embed, encoder_hidden_states=feature_f,
                                my_pose_cond=pose_cond, return_dict=False)[0]
                if do_cfg:
                    g = torch.empty_like(lat)
                    eps = eps.float().contiguous()
                    ops.cfg_step(eps, True, float(guidance_scale), None, None, None, eps_out=g)
                    if guidance_rescale > 0.0:   # ref :514-516
                        g = rescale_noise_cfg(g, eps[eps.shape[0] // 2:], guidance_rescale)
                    eps = g
                lat = self.scheduler.step(eps, t, lat, **extra, return_dict=False)[0]
                if callback is not None and i % callback_steps == 0:
                    callback(i, t, lat)
            self.unet.invalidate_caches()
        else:
            lat = self._run_fused(lat, mask, masked, pose_cond, feature_f, prior_embed, timesteps, do_cfg,
                                  float(guidance_scale), eta, use_graph, callback, callback_steps,
                                  float(guidance_rescale) if do_cfg else 0.0, zero_uncond, shared_halves and do_cfg,
                                  generator=extra.get("generator"))

        return lat

    def _postprocess(self, lat, output_type):
        """ref :528-532: vae.decode(latents / scaling_factor) + VaeImageProcessor.postprocess."""
        if output_type == "latent" or self.vae is None:
            return lat
        z = lat / self.vae.config.scaling_factor
        if output_type == "pt":
            return (self.vae.decode(z, return_dict=False)[0] / 2 + 0.5).clamp(0, 1)
        u8 = self.vae.decode_to_uint8(z)            # uint8 [N, H, W, 3] on the device (HIP kernel)
        if output_type == "uint8":
            return u8
        arr = u8.cpu().numpy()
        if output_type == "np":
            return arr.astype("float32") / 255.0
        from PIL import Image                        # "pil" (the reference default)
        return [Image.fromarray(a) for a in arr]

    # ------------------------------------------------------------------------------------------
    def _step_eager(self, st):
        unet = self.unet
        B, h, w = st["B"], st["h"], st["w"]
        if st.get("scaled"):   # scale_model_input: the latent channels times this step's 1 / sqrt(sigma^2 + 1), read from the step table
            x_in = ops.assemble_input_ex(st["lat"], st["rep"], st["mask"], st["masked"], st["x_in"], st["coef"], ops.MS_IN_SCALE, st["step"],
                                         st["step_err"])
        else:
            x_in = ops.assemble_input(st["lat"], st["rep"], st["mask"], st["masked"], st["x_in"])
        if st.get("ctx") is not None:
            eps = st["ctx"].forward(x_in, st["timesteps"], st["step"], B, h, w, st["pose_b"], out=st["eps_c"], L=st["L"])
        else:
            eps = unet._forward_nhwc(x_in, B, h, w, st["timesteps"], st["cond"], step_dev=st["step"])
        cfg, g, e = st["rep"] == 2, st["g"], eps
        if st["gr"] > 0.0:   # CFG -> rescale_noise_cfg (ref :510-516) -> scheduler update
            n = eps.shape[0] // 2
            ops.cfg_step(eps, True, st["g"], None, None, None, eps_out=st["eps_g"])
            ops.rescale_noise_cfg(st["eps_g"], eps[n:], st["eps_g"], st["gr"])
            cfg, g, e = False, 1.0, st["eps_g"]
        if st["unipc"]:
            ops.unipc_step(e, cfg, g, st["lat"], st["m1"], st["m2"], st["last"], st["coef"], st["step"], st["step_err"])
        elif st["dpm"]:
            ops.dpmpp_step(e, cfg, g, st["lat"], st["m1"], st["noise"], st["coef"], st["step"], st["step_err"])
        elif st.get("ms"):
            ops.multistep_step(e, cfg, g, st["lat"], st["xs"], st["h1"], st["h2"], st["h3"], st["noise"], st["coef"], st["step"], st["step_err"])
        else:
            ops.cfg_step(e, cfg, g, st["lat"], st["lat"], st["coef"], st["step"], step_error=st["step_err"])
        ops.advance_step(st["step"])

    @staticmethod
    def _weights_generation(unet, dev):
        """What a captured step's weight and workspace pointers depend on: which model (its process-wide serial number), which packing
        of its weights, which split-K workspace."""
        return (unet._serial, getattr(unet, "_pack_gen", 0), ops.workspace_generation(dev))

    @staticmethod
    def _context_generation(ctx, w_gen):
        """What the one-off tuning step of the C schedule was made for: which context (its serial number), which weights and workspace."""
        return (ctx._serial, w_gen)

    @staticmethod
    def _zero_history(st):
        if st.get("unipc"):
            for k in ("m1", "m2", "last"):
                st[k].zero_()
        elif st.get("dpm"):
            st["m1"].zero_()
        elif st.get("ms"):
            for k in ("xs", "h1", "h2", "h3"):
                st[k].zero_()

    def _run_fused(self, lat, mask, masked, pose_cond, feature_f, prior_embed, timesteps, do_cfg, g, eta, use_graph,
                   callback, callback_steps, guidance_rescale=0.0, zero_uncond=False, shared_halves=False, generator=None):
        unet, dev = self.unet, self.device
        if unet._w is None:
            unet._pack()
        n = len(timesteps)
        N, _, h, w = lat.shape
        rep = 2 if do_cfg else 1
        B = rep * N
        n0 = N if (do_cfg and zero_uncond) else 0
        unipc = isinstance(self.scheduler, UniPCMultistepScheduler)
        dpm = isinstance(self.scheduler, DPMSolverMultistepScheduler)
        ms = isinstance(self.scheduler, _TableStepScheduler)     # Euler / Euler-ancestral / LMS / PNDM: pcdm_multistep_step
        sde = (dpm or ms) and self.scheduler.stochastic
        scaled = ms and self.scheduler.scales_input
        kind = "unipc" if unipc else ("dpm_sde" if sde else "dpm") if dpm else ("ms", sde, scaled) if ms else "linear"
        tdt = torch.float32 if timesteps.dtype.is_floating_point else torch.int64   # the scheduler's own: float32 tables keep fractional timesteps
        key = (B, h, w, n, rep, n0, tuple(feature_f.shape), None if mask is None else tuple(mask.shape), tuple(masked.shape),
               None if pose_cond is None else tuple(pose_cond.shape), prior_embed is None, kind, bool(shared_halves), tdt,
               bool(self.c_schedule))   # (the captured step calls either the Python schedule or the C context: each refreshes its own buffers)
        st = self._st if self._graph_key == key else {}
        if not st:
            st.update(B=B, h=h, w=w, rep=rep, unipc=unipc, dpm=dpm, ms=ms, scaled=scaled, noise=None,
                      lat=torch.empty_like(lat), mask=None if mask is None else torch.empty_like(mask), masked=torch.empty_like(masked),
                      eps_g=torch.empty_like(lat),
                      x_in=torch.empty(B, h, w, 64, dtype=ops.BF16, device=dev),
                      step=torch.zeros(1, dtype=torch.int32, device=dev),
                      step_err=torch.zeros(1, dtype=torch.int32, device=dev),   # raised by every table reader for a counter outside its table
                      timesteps=torch.empty(n, dtype=tdt, device=dev),
                      coef=torch.empty(n, 12 if (unipc or ms) else 8 if dpm else 4, dtype=torch.float32, device=dev))
            if unipc:   # UniPC history (two stored x0-predictions, last corrected sample): static slots, zeroed per call
                st.update(m1=torch.zeros_like(lat), m2=torch.zeros_like(lat), last=torch.zeros_like(lat))
            if dpm:     # DPM-Solver++ history (the previous x0-prediction) and, for the SDE form, the per-step noise table [n, numel]
                st.update(m1=torch.zeros_like(lat), noise=torch.empty(n, lat.numel(), dtype=torch.float32, device=dev) if sde else None)
            if ms:      # saved sample + three eps-history slots, zeroed per call
                st.update(xs=torch.zeros_like(lat), h1=torch.zeros_like(lat), h2=torch.zeros_like(lat), h3=torch.zeros_like(lat),
                          noise=torch.empty(n, lat.numel(), dtype=torch.float32, device=dev) if sde else None)
            self._graph = None
        # Per call: the static input slots the captured step reads are refilled, and the step-invariant conditioning (class
        # embedding, NHWC pose, the 16 cross-attention K / V^T) is recomputed EAGERLY into the UNet's shape-keyed buffers --
        # ~20 small launches against the 50 x ~400 of the loop.  No content comparison, no host sync: whatever another caller
        # (a reference-mode call, a bare unet(...)) left in those shared buffers is overwritten, and the graph only ever reads
        # the same addresses.
        st["lat"].copy_(lat)
        if mask is not None:
            st["mask"].copy_(mask)
        st["masked"].copy_(masked)
        st["timesteps"].copy_(timesteps.to(dev, tdt))
        st["step_err"].zero_()
        # (with the timestep table: the time / class embedding MLPs and every time_emb_proj for ALL steps, once per call)
        st["cond"] = unet.prepare_conditioning(B, h, w, feature_f, prior_embed, pose_cond, zero_ctx_batches=n0, shared_cfg_input=shared_halves,
                                               timesteps=st["timesteps"])
        st["coef"].copy_(self.scheduler.coefficient_table(device=dev) if (unipc or dpm or ms) else self.scheduler.coefficient_table(eta, device=dev))
        if sde:   # the draws the literal loop would make, one per step in step order, refilled per call outside the captured step
            for i in range(n):
                st["noise"][i].copy_(_step_noise(lat.shape, generator, dev).reshape(-1))
        st["g"] = g
        if st.get("gr", guidance_rescale) != guidance_rescale:
            self._graph = None
        st["gr"] = guidance_rescale
        freeu = getattr(unet, "_freeu", None)   # on / off and the four floats: another launch list, other kernel arguments
        if st.get("freeu", freeu) != freeu:
            self._graph = None
        st["freeu"] = freeu
        # pipe.unet replaced, weights re-packed (load_state_dict / .to), or a split-K workspace re-allocated: re-capture.  The model is named
        # by its serial number, never by id(): a model built after the old one was dropped may sit at the same address
        w_gen = self._weights_generation(unet, dev)
        if st.get("w_gen") != w_gen:
            self._graph = None
        st["ctx"] = None
        if self.c_schedule:
            from .unet_ctx import UNetContext
            if self._ctx is None or self._ctx._pack_gen != unet._pack_gen or self._ctx.unet is not unet:
                self._ctx = UNetContext(unet)
                self._graph = None
            # one Python-schedule step first, once per (context, weights, workspace): it tunes every GEMM shape of this batch size.  The
            # device step counter is reset BEFORE it (a reused `st` still holds the last run's count, one past the end of the
            # timestep / coefficient tables: ADVICE r3)
            if st.get("c_tuned") != self._context_generation(self._ctx, w_gen) and dev.type == "cuda":
                lat0 = lat.clone()
                st["step"].zero_()
                self._zero_history(st)
                self._step_eager(st)
                st["lat"].copy_(lat0)
                st["step"].zero_()
                self._zero_history(st)
                self._ctx.sync_tiles()
                # the eager step may have grown the split-K workspace (-> a new workspace generation): store the generation AFTER it, or
                # the next call would tune a second time
                w_gen2 = self._weights_generation(unet, dev)
                if w_gen2 != w_gen:
                    self._graph = None        # (a graph captured on the old workspace addresses must not be replayed)
                w_gen = w_gen2
                st["c_tuned"] = self._context_generation(self._ctx, w_gen)
            st["pose_b"] = self._ctx.prepare_conditioning(B, h, w, feature_f, prior_embed, pose_cond, zero_ctx_batches=n0,
                                                          shared_cfg_input=st["cond"].shared_halves)
            self._ctx.prepare_timesteps(st["timesteps"], B, h, w, L=feature_f.shape[1])
            st["L"] = feature_f.shape[1]   # (in `key` through feature_f.shape: the captured forward's context length)
            st["eps_c"] = st.get("eps_c") if st.get("eps_c") is not None and st["eps_c"].shape[0] == B else \
                torch.empty(B, unet.config.out_channels, h, w, dtype=torch.float32, device=dev)
            st["ctx"] = self._ctx
        st["step"].zero_()
        self._zero_history(st)
        self._st, self._graph_key = st, key
        if use_graph and dev.type == "cuda":
            if self._graph is None or self._st.get("g_captured") != g:
                # warm-up step (allocates every scratch buffer, autotunes unseen GEMM shapes), then capture
                lat0 = st["lat"].clone()
                self._step_eager(st)
                torch.cuda.synchronize()
                st["lat"].copy_(lat0)
                st["step"].zero_()
                self._zero_history(st)
                graph = torch.cuda.CUDAGraph()
                # thread_local: other threads (e.g. the RCCL watchdog) may touch the runtime while we capture
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    self._step_eager(st)
                st["lat"].copy_(lat0)
                st["step"].zero_()
                self._zero_history(st)
                self._graph = graph
                st["g_captured"] = g
                w_gen = self._weights_generation(unet, dev)   # (the warm-up may have grown it)
            st["w_gen"] = w_gen
            for i in range(n):
                self._graph.replay()
                if callback is not None and i % callback_steps == 0:   # (stream-ordered copy of the live latent buffer)
                    callback(i, timesteps[i], st["lat"].clone())
        else:
            st["w_gen"] = w_gen
            for i in range(n):
                self._step_eager(st)
                if callback is not None and i % callback_steps == 0:
                    callback(i, timesteps[i], st["lat"])
        out = st["lat"].clone()
        # the device step counter indexes the per-call time table inside the UNet's kernels: they bound it (a counter beyond the table is
        # clamped, never an out-of-bounds read of THAT table) and raise a flag -- read once per sampling call (one 4-byte copy behind the
        # loop).  Every sampler's step kernel bounds its coefficient / noise row and reports likewise (st["step_err"]: one more 4-byte read
        # per call, no launch in the step), so no step of any sampler kind reads past st["coef"] or st["noise"].  The UNet's flag lives where
        # the schedule that ran keeps it: in the context's workspace on the C schedule (no kernel of such a call writes the Python
        # schedule's), in the UNet's scratch otherwise -- one 4-byte read per call either way, no second synchronisation
        if st["ctx"] is not None:
            overflow = st["ctx"].step_overflow(B, h, w, L=feature_f.shape[1])
        else:
            overflow = hasattr(unet, "step_overflow") and unet.step_overflow()
        if overflow or int(st["step_err"].item()) != 0:
            raise RuntimeError("the device step counter left the time-embedding table of this sampling call (clamped on the device): "
                               "the schedule ran more steps than prepare_conditioning(timesteps=...) was given")
        return out


class Simple_Stage2_InpaintDiffusionPipeline(Stage2_InpaintDiffusionPipeline):
    """The reference's variant without the stage-1 prior embedding (stage2_inpaint_pipeline.py:544-887):
    ``self.unet(x, t, encoder_hidden_states=feature_f, my_pose_cond=pose_cond)`` (:860-862) with a UNet built
    without ``class_embed_type``; ``pred_t_img_embed`` is ignored."""

    use_prior_embed = False


class Stage3_RefinedDiffusionPipeline(Stage2_InpaintDiffusionPipeline):
    """Stage-3 refinement sampler: mirrors ``Stage3_RefinedDiffusionPipeline.__call__``
    (/root/reference/src/pipelines/stage3_refined_pipeline.py:441-578).  UNet = ``pcdms_amd.UNet2DConditionModel``
    with ``in_channels=8``; input ``cat([latents, gen_t_img_latents], 1)`` (:538); CFG uncond half = zero context and
    zero refine latents (:491-497).  The reference forgets to repeat the conditioning for
    ``num_images_per_prompt`` under CFG (a shape error for N > 1); here it is repeated.
    ``gen_t_img_latents`` = vae.encode(vae_gen_t_image).sample() * scaling_factor (:483-484; VAE outside the hot path)."""

    @torch.no_grad()
    def __call__(self, height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 50,
                 guidance_scale: float = 7.5, num_images_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None,
                 latents: Optional[torch.Tensor] = None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 callback=None, callback_steps: int = 1, guidance_rescale: float = 0.0,
                 vae_gen_t_image: Optional[torch.Tensor] = None, s_img_proj_f: Optional[torch.Tensor] = None,
                 gen_t_img_latents: Optional[torch.Tensor] = None, mode: Optional[str] = None, use_graph: bool = True):
        device = self.device
        N = num_images_per_prompt
        f32 = dict(device=device, dtype=torch.float32)
        if gen_t_img_latents is None:
            if self.vae is None:
                raise ValueError("pass gen_t_img_latents=... (VAE encode is outside the hot path) or construct with vae=")
            gen_t_img_latents = self.vae.encode(vae_gen_t_image.to(device)).latent_dist.sample(generator=generator)
            gen_t_img_latents = gen_t_img_latents * self.vae.config.scaling_factor
        do_cfg = guidance_scale > 1.0
        feat = s_img_proj_f.to(**f32).repeat_interleave(N, 0)
        gl = gen_t_img_latents.to(**f32).repeat_interleave(N, 0)
        if do_cfg:
            feat = torch.cat([torch.zeros_like(feat), feat])
            gl = torch.cat([torch.zeros_like(gl), gl])
        feat, gl = feat.contiguous(), gl.contiguous()
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        lat = self.prepare_latents(s_img_proj_f.shape[0] * N, 4, height, width, torch.float32, device, generator, latents).contiguous()
        extra = self.prepare_extra_step_kwargs(generator, eta)
        # the same loop machinery as stage 2 (ref :533-563): no mask channel, no pose, no class labels; DDIM / UniPC / DPM-Solver++ run as the
        # captured fused step, anything else through the literal loop
        lat = self._sample(lat, None, gl, None, feat, None, self.scheduler.timesteps, do_cfg, guidance_scale, guidance_rescale, eta, extra,
                           mode, use_graph, callback, callback_steps, zero_uncond=do_cfg)
        images = self._postprocess(lat, output_type)
        if not return_dict:
            return (images, None)
        return Stage2_InpaintDiffusionPipelineOutput(images=images, nsfw_content_detected=None, latents=lat)


class PCDMsPipeline(Simple_Stage2_InpaintDiffusionPipeline):
    """The notebook's "simplified PCDMs" caller of the same UNet: mirrors
    ``PCDMsPipeline.__call__`` (/root/reference/src/pipelines/PCDMs_pipeline.py:893-1184; pcdms_kaggle_demo.ipynb cell 38).
    Inputs arrive as tensors: ``simg_mask_latents`` (VAE latents of the [source | black] canvas, already scaled), ``mask``,
    ``cond_pose`` (the pose feature, un-doubled: it broadcasts over the batch, :1127), ``prompt_embeds`` = the projected
    DINOv2 tokens and ``negative_prompt_embeds`` = ``image_proj_model(zeros)`` (cell 37) -- a NON-zero unconditional
    context; no ``class_labels``.  The input is ``cat([latents, mask, simg_mask_latents], 1)`` doubled for CFG (:1117-1119),
    which is what ``pcdm_assemble_input`` builds.  Text prompts, IP-adapter images, LoRA scale, ``clip_skip`` and the safety
    checker are SD boilerplate the notebook never uses: ``NotImplementedError`` when given.  ``timesteps`` goes through
    ``retrieve_timesteps`` as in the reference (:1081): a ``ValueError`` unless the scheduler's ``set_timesteps`` accepts it."""

    @torch.no_grad()
    def __call__(self, simg_mask_latents=None, mask=None, cond_pose=None, prompt=None, height: Optional[int] = None,
                 width: Optional[int] = None, num_inference_steps: int = 50, timesteps=None, guidance_scale: float = 7.5,
                 negative_prompt=None, num_images_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None,
                 latents: Optional[torch.Tensor] = None, prompt_embeds=None, negative_prompt_embeds=None, ip_adapter_image=None,
                 output_type: Optional[str] = "pil", return_dict: bool = True, cross_attention_kwargs=None,
                 guidance_rescale: float = 0.0, clip_skip=None, callback_on_step_end=None,
                 callback_on_step_end_tensor_inputs=("latents",), mode: Optional[str] = None, use_graph: bool = True, **kwargs):
        if prompt is not None or negative_prompt is not None or ip_adapter_image is not None or cross_attention_kwargs is not None \
                or clip_skip is not None:
            raise NotImplementedError("text prompts / IP-adapter / LoRA / clip_skip are not part of the PCDMs path")
        if prompt_embeds is None or simg_mask_latents is None or mask is None or cond_pose is None:
            raise ValueError("simg_mask_latents, mask, cond_pose and prompt_embeds are required")
        device = self.device
        N = num_images_per_prompt
        h, w = simg_mask_latents.shape[-2:]
        height, width = height or h * self.vae_scale_factor, width or w * self.vae_scale_factor
        if (height // self.vae_scale_factor, width // self.vae_scale_factor) != (h, w):
            raise ValueError("height / width do not match simg_mask_latents")
        f32 = dict(device=device, dtype=torch.float32)
        do_cfg = guidance_scale > 1.0
        bs = prompt_embeds.shape[0]
        pe = prompt_embeds.to(**f32).repeat_interleave(N, 0)                    # encode_prompt: repeat per prompt (:404-406)
        if do_cfg:
            if negative_prompt_embeds is None:
                raise ValueError("negative_prompt_embeds is required with guidance_scale > 1 (the notebook passes image_proj_model(zeros))")
            feature_f = torch.cat([negative_prompt_embeds.to(**f32).repeat_interleave(N, 0), pe])
        else:
            feature_f = pe
        rep = 2 if do_cfg else 1

        def per_sample(x):   # [1 | bs*N, ...] as given -> broadcastable by the kernels (1) or the full CFG-doubled batch
            x = x.to(**f32)
            return x.contiguous() if x.shape[0] == 1 else torch.cat([x] * rep).contiguous()
        mask_t, masked, pose_cond = per_sample(mask), per_sample(simg_mask_latents), per_sample(cond_pose)
        for name, t in (("mask", mask_t), ("simg_mask_latents", masked), ("cond_pose", pose_cond)):
            if t.shape[0] not in (1, rep * bs * N):
                raise ValueError(f"{name}: batch {t.shape[0] // (rep if t.shape[0] != 1 else 1)} does not match {bs * N} samples")
        ts, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, device, timesteps)   # ref :1081
        lat = self.prepare_latents(bs * N, 4, height, width, torch.float32, device, generator, latents).contiguous()
        extra = self.prepare_extra_step_kwargs(generator, eta)
        cb = None
        if callback_on_step_end is not None:   # diffusers >= 0.22 callback protocol (:1150-1158), latents only
            def cb(i, t, cur):
                callback_on_step_end(self, i, t, {"latents": cur})
        lat = self._sample(lat, mask_t, masked, pose_cond, feature_f.contiguous(), None, ts, do_cfg, guidance_scale, guidance_rescale, eta,
                           extra, mode, use_graph, cb, 1, shared_halves=do_cfg)   # (per_sample above: the same tensors for both halves)
        images = self._postprocess(lat, output_type)
        if not return_dict:
            return (images, None)
        return Stage2_InpaintDiffusionPipelineOutput(images=images, nsfw_content_detected=None, latents=lat)
