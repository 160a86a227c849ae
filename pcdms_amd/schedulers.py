"""MI355X-native stand-ins for the reference's ``pipe.scheduler`` objects.

The reference uses three diffusers 0.24.0 schedulers at this boundary:
``UniPCMultistepScheduler`` (stage2_batchtest_inpaint_model.py:132), ``DDIMScheduler``
(pcdms_kaggle_demo.ipynb cell 15 -- the configuration BASELINE.json's metric names) and
``DDPMScheduler`` (stage2_train_inpaint_model.py:175,361).  The pipelines type the slot as any
``KarrasDiffusionSchedulers`` member; the six that ``Simple_Stage2_InpaintDiffusionPipeline.__init__`` names
(src/pipelines/stage2_inpaint_pipeline.py:547-558) are all here: DDIM, ``DPMSolverMultistepScheduler`` ("DPM++ 2M", with or without
Karras sigmas, and its SDE form), ``PNDMScheduler`` (PLMS, the SD-2.1 directory's own scheduler), ``LMSDiscreteScheduler``,
``EulerDiscreteScheduler`` and ``EulerAncestralDiscreteScheduler``.  Call sites:
src/pipelines/stage2_inpaint_pipeline.py:472-473 (set_timesteps / timesteps), :386
(init_noise_sigma), :494 (order), :500 (scale_model_input), :519 (step; ``eta`` / ``generator`` are
passed only if ``inspect.signature(step)`` has them, :313-321).

Coefficient math is scalar host code (float64, tables in fp32 where diffusers keeps them in fp32);
every tensor update is a hand-written HIP kernel from libpcdm.so (``pcdm_lincomb`` /
``pcdm_cfg_step`` / ``pcdm_dpmpp_step`` / ``pcdm_multistep_step``).  Tensors must be on the GPU: there is no CPU tensor path.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import ops


class SchedulerOutput:
    def __init__(self, prev_sample, pred_original_sample=None):
        self.prev_sample = prev_sample
        self.pred_original_sample = pred_original_sample

    def __getitem__(self, i):
        return (self.prev_sample,)[i]


class _Config(SimpleNamespace):
    def __getitem__(self, k):
        return getattr(self, k)

    def get(self, k, d=None):
        return getattr(self, k, d)

    def keys(self):
        return self.__dict__.keys()


def _betas(cfg) -> np.ndarray:
    T = cfg.num_train_timesteps
    if cfg.trained_betas is not None:
        return np.asarray(cfg.trained_betas, dtype=np.float32)
    if cfg.beta_schedule == "linear":
        return torch.linspace(cfg.beta_start, cfg.beta_end, T, dtype=torch.float32).numpy()
    if cfg.beta_schedule == "scaled_linear":
        return (torch.linspace(cfg.beta_start ** 0.5, cfg.beta_end ** 0.5, T, dtype=torch.float32) ** 2).numpy()
    if cfg.beta_schedule == "squaredcos_cap_v2":   # diffusers betas_for_alpha_bar (cosine), max_beta 0.999
        def alpha_bar(t):
            return math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
        return np.asarray([min(1 - alpha_bar((i + 1) / T) / alpha_bar(i / T), 0.999) for i in range(T)], dtype=np.float32)
    raise NotImplementedError(f"{cfg.beta_schedule} does is not implemented")


def _f32(t: torch.Tensor) -> torch.Tensor:
    if not t.is_cuda and not ops._lib.is_emulator():
        raise RuntimeError("scheduler.step needs GPU tensors (no CPU tensor path in pcdms_amd)")
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def _train_sigmas(ac: torch.Tensor) -> np.ndarray:
    """((1 - ac) / ac) ** 0.5 of the fp32 training table (fp32, as diffusers)."""
    a = ac.numpy()
    return ((1 - a) / a) ** 0.5


def _convert_to_karras(in_sigmas: np.ndarray, num_inference_steps: int, rho: float = 7.0) -> np.ndarray:
    """Karras et al. (2022) noise levels: rho-spaced from ``in_sigmas[0]`` (sigma_max) down to ``in_sigmas[-1]`` (sigma_min).
    ``in_sigmas`` is the training sigma table flipped (decreasing), as diffusers passes it; float64 result."""
    sigma_min, sigma_max = float(in_sigmas[-1]), float(in_sigmas[0])
    ramp = np.linspace(0, 1, num_inference_steps)
    min_inv_rho, max_inv_rho = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
    return (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** rho


def _sigma_to_t(sigma, log_sigmas: np.ndarray) -> np.ndarray:
    """Fractional training timestep of ``sigma``: linear interpolation in log-sigma between the two neighbouring training entries
    (``log_sigmas`` increasing with t), clamped to the table."""
    sigma = np.asarray(sigma)
    log_sigma = np.log(np.maximum(sigma, 1e-10))
    dists = log_sigma - log_sigmas[:, np.newaxis]
    low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
    high_idx = low_idx + 1
    low, high = log_sigmas[low_idx], log_sigmas[high_idx]
    w = np.clip((low - log_sigma) / (low - high), 0, 1)
    return ((1 - w) * low_idx + w * high_idx).reshape(sigma.shape)


def _karras_schedule(ac: torch.Tensor, num_inference_steps: int) -> Tuple[np.ndarray, np.ndarray]:
    """(int64 timesteps [n], fp32 sigmas [n + 1]) of ``use_karras_sigmas=True`` (diffusers 0.24 multistep schedulers): the Karras
    sigmas between the ends of the training table, timesteps from ``_sigma_to_t`` rounded to integers (the time-embedding ABI takes
    int64), and the last sigma repeated as the final one."""
    sig = _train_sigmas(ac)
    sigmas = _convert_to_karras(np.flip(sig).copy(), num_inference_steps)
    ts = np.round(_sigma_to_t(sigmas, np.log(sig))).astype(np.int64)
    return ts, np.concatenate([sigmas, sigmas[-1:]]).astype(np.float32)


def _step_noise(shape, generator: Optional[torch.Generator], dev) -> torch.Tensor:
    """The per-step Gaussian noise of the stochastic multistep samplers (literal loop and fused path alike): drawn on the generator's
    device (a CPU generator works), then moved to ``dev``."""
    z = torch.randn(shape, generator=generator, device=generator.device if generator is not None else dev, dtype=torch.float32)
    return z.to(dev)


def _alpha_sigma_lambda(sigma: float) -> Tuple[float, float, float]:
    """(alpha_t, sigma_t, lambda_t) of a noise level sigma = sigma_t / alpha_t, in float64."""
    alpha = 1.0 / math.sqrt(sigma * sigma + 1.0)
    sig = sigma * alpha
    return alpha, sig, math.log(alpha) - math.log(sig)


class _Base:
    order = 1
    init_noise_sigma = 1.0
    _defaults: dict = {}

    def __init__(self, **kwargs):
        cfg = dict(self._defaults)
        cfg.update(kwargs)   # from_config semantics (diffusers): keys of other, compatible schedulers do not act here but stay in
        self.config = _Config(**cfg)   # .config ("hidden" attributes), so that A.from_config(B.from_config(A.config).config) round-trips
        betas = _betas(self.config)
        self.betas = torch.from_numpy(betas.copy())
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)  # fp32, as diffusers
        self._ac = self.alphas_cumprod.numpy().astype(np.float64)
        self.num_inference_steps: Optional[int] = None
        self.timesteps = torch.arange(self.config.num_train_timesteps - 1, -1, -1, dtype=torch.int64)

    @classmethod
    def from_config(cls, config, **kwargs):
        cfg = dict(config.__dict__ if isinstance(config, SimpleNamespace) else config)
        cfg.update(kwargs)
        return cls(**cfg)

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def __len__(self):
        return self.config.num_train_timesteps

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        """sqrt(ac_t) x0 + sqrt(1-ac_t) noise with one coefficient pair per batch row."""
        x0, n = _f32(original_samples), _f32(noise)
        out = torch.empty_like(x0)
        ts = [int(v) for v in timesteps.reshape(-1).tolist()]
        if len(ts) == 1:
            ts = ts * x0.shape[0]
        for b, t in enumerate(ts):
            a = float(self._ac[t])
            ops.lincomb(out[b], [x0[b], n[b]], [math.sqrt(a), math.sqrt(1 - a)])
        return out.to(original_samples.dtype)


class DDIMScheduler(_Base):
    """SURVEY.md Appendix A-9.  ``DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
    beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False, steps_offset=1)`` is the
    notebook's (cell 15) configuration."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, clip_sample=True, set_alpha_to_one=True, steps_offset=0,
                     prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                     clip_sample_range=1.0, sample_max_value=1.0, timestep_spacing="leading", rescale_betas_zero_snr=False)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c.prediction_type != "epsilon" or c.thresholding or c.rescale_betas_zero_snr:
            raise NotImplementedError("only epsilon prediction without thresholding is on the stage-2 path")
        self.final_alpha_cumprod = 1.0 if c.set_alpha_to_one else float(self._ac[0])

    def set_timesteps(self, num_inference_steps: int, device=None):
        c = self.config
        if num_inference_steps > c.num_train_timesteps:
            raise ValueError("`num_inference_steps` cannot be larger than `num_train_timesteps`")
        self.num_inference_steps = num_inference_steps
        T = c.num_train_timesteps
        if c.timestep_spacing == "leading":
            ratio = T // num_inference_steps
            ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + c.steps_offset
        elif c.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        elif c.timestep_spacing == "trailing":
            ts = np.round(np.arange(T, 0, -T / num_inference_steps)).astype(np.int64) - 1
        else:
            raise ValueError(c.timestep_spacing)
        self.timesteps = torch.from_numpy(ts).to(device)

    def _alphas(self, t: int) -> Tuple[float, float]:
        tp = t - self.config.num_train_timesteps // self.num_inference_steps
        return float(self._ac[t]), (float(self._ac[tp]) if tp >= 0 else self.final_alpha_cumprod)

    def step_coefficients(self, t: int, eta: float = 0.0) -> Tuple[float, float, float, float, float]:
        """(cx, ce, cn, c0x, c0e): x_prev = cx*x + ce*eps + cn*noise ; x0 = c0x*x + c0e*eps."""
        a, ap = self._alphas(int(t))
        var = (1 - ap) / (1 - a) * (1 - a / ap)
        std = eta * math.sqrt(max(var, 0.0))
        c0x, c0e = 1.0 / math.sqrt(a), -math.sqrt(1 - a) / math.sqrt(a)
        if self.config.clip_sample:
            raise NotImplementedError("clip_sample=True is not linear; the stage-2 path uses clip_sample=False")
        dirc = math.sqrt(max(1 - ap - std * std, 0.0))
        return math.sqrt(ap) * c0x, math.sqrt(ap) * c0e + dirc, std, c0x, c0e

    def coefficient_table(self, eta: float = 0.0, device=None) -> torch.Tensor:
        """fp32 [n_steps, 4] rows {cx, ce, cn, 0} in timestep order, for the device-indexed fused step."""
        rows = [list(self.step_coefficients(int(t), eta)[:3]) + [0.0] for t in self.timesteps.tolist()]
        return torch.tensor(rows, dtype=torch.float32, device=device)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, eta: float = 0.0,
             use_clipped_model_output: bool = False, generator=None, variance_noise: Optional[torch.Tensor] = None,
             return_dict: bool = True):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        cx, ce, cn, c0x, c0e = self.step_coefficients(int(timestep), eta)
        e, x = _f32(model_output), _f32(sample)
        xs, cs = [x, e], [cx, ce]
        if cn > 0:
            if variance_noise is None:
                variance_noise = torch.randn(e.shape, generator=generator, device=e.device, dtype=torch.float32)
            xs.append(_f32(variance_noise))
            cs.append(cn)
        prev = ops.lincomb(torch.empty_like(x), xs, cs).to(sample.dtype)
        if not return_dict:
            return (prev,)
        x0 = ops.lincomb(torch.empty_like(x), [x, e], [c0x, c0e]).to(sample.dtype)
        return SchedulerOutput(prev, x0)


class DDPMScheduler(_Base):
    """SURVEY.md Appendix A-11 (variance_type fixed_small, epsilon prediction)."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, variance_type="fixed_small", clip_sample=True, prediction_type="epsilon",
                     thresholding=False, dynamic_thresholding_ratio=0.995, clip_sample_range=1.0,
                     sample_max_value=1.0, timestep_spacing="leading", steps_offset=0)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if self.config.prediction_type != "epsilon" or self.config.variance_type != "fixed_small":
            raise NotImplementedError

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.config.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.config.steps_offset
        self.timesteps = torch.from_numpy(ts).to(device)

    def step_coefficients(self, t: int) -> Tuple[float, float, float]:
        n = self.num_inference_steps or self.config.num_train_timesteps
        tp = t - self.config.num_train_timesteps // n
        a = float(self._ac[t])
        ap = float(self._ac[tp]) if tp >= 0 else 1.0
        cur_a = a / ap
        cur_b = 1 - cur_a
        c0x, c0e = 1 / math.sqrt(a), -math.sqrt(1 - a) / math.sqrt(a)
        k0, kx = math.sqrt(ap) * cur_b / (1 - a), math.sqrt(cur_a) * (1 - ap) / (1 - a)
        sigma = math.sqrt(max((1 - ap) / (1 - a) * cur_b, 1e-20)) if t > 0 else 0.0
        return k0 * c0x + kx, k0 * c0e, sigma

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, return_dict: bool = True):
        if self.config.clip_sample:
            raise NotImplementedError("clip_sample=True is outside the stage-2 path")
        cx, ce, cn = self.step_coefficients(int(timestep))
        e, x = _f32(model_output), _f32(sample)
        xs, cs = [x, e], [cx, ce]
        if cn > 0:
            if variance_noise is None:
                variance_noise = torch.randn(e.shape, generator=generator, device=e.device, dtype=torch.float32)
            xs.append(_f32(variance_noise))
            cs.append(cn)
        prev = ops.lincomb(torch.empty_like(x), xs, cs).to(sample.dtype)
        return (prev,) if not return_dict else SchedulerOutput(prev)


class UniPCMultistepScheduler(_Base):
    """UniPC, B(h) = e^h - 1 ("bh2"), order 2, predict_x0, lower_order_final.

    ``step`` has no ``eta`` / ``generator`` parameters (the pipeline inspects the signature).  Stateful:
    one instance per in-flight sampling run."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, solver_order=2, prediction_type="epsilon", thresholding=False,
                     dynamic_thresholding_ratio=0.995, sample_max_value=1.0, predict_x0=True, solver_type="bh2",
                     lower_order_final=True, disable_corrector=[], solver_p=None, use_karras_sigmas=False,
                     timestep_spacing="linspace", steps_offset=0)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c.solver_type in ("midpoint", "heun", "logrho"):   # a DPM-Solver config (from_config): diffusers maps it to bh2 as well
            c.solver_type = "bh2"
        if (c.prediction_type != "epsilon" or c.thresholding or not c.predict_x0
                or c.solver_p is not None or c.solver_type not in ("bh1", "bh2")):
            raise NotImplementedError("UniPC variant outside the stage-2 path")
        self.set_timesteps(c.num_train_timesteps)

    def set_timesteps(self, num_inference_steps: int, device=None):
        c, T = self.config, self.config.num_train_timesteps
        self.num_inference_steps = num_inference_steps
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif c.timestep_spacing == "leading":
            ratio = T // (num_inference_steps + 1)
            ts = (np.arange(0, num_inference_steps + 1) * ratio).round()[::-1][:-1].copy().astype(np.int64) + c.steps_offset
        else:
            raise NotImplementedError(c.timestep_spacing)
        if c.use_karras_sigmas:   # the coefficient math below reads self.sigmas only
            ts, self.sigmas = _karras_schedule(self.alphas_cumprod, num_inference_steps)
        else:
            ac = self.alphas_cumprod.numpy()
            sig = ((1 - ac) / ac) ** 0.5
            sigmas = np.interp(ts, np.arange(0, len(sig)), sig)
            self.sigmas = np.concatenate([sigmas, [((1 - ac[0]) / ac[0]) ** 0.5]]).astype(np.float32)
        self.timesteps = torch.from_numpy(ts).to(device)
        self.model_outputs: List[Optional[torch.Tensor]] = [None] * c.solver_order
        self.lower_order_nums = 0
        self.last_sample: Optional[torch.Tensor] = None
        self._step_index: Optional[int] = None
        self.this_order = 1
        self._ts_list = [int(v) for v in ts]

    @property
    def step_index(self):
        return self._step_index

    # ---- scalar pieces
    def _als(self, i: int) -> Tuple[np.float32, np.float32, np.float32]:
        s = np.float32(self.sigmas[i])
        alpha = np.float32(1.0) / np.sqrt(s * s + np.float32(1.0), dtype=np.float32)
        sig = s * alpha
        return np.log(alpha) - np.log(sig), alpha, sig

    def _rb(self, rks, hh, order):
        with np.errstate(divide="ignore", invalid="ignore"):   # hh == 0 on the repeated final Karras sigma: those terms go unused
            h_phi_1 = np.expm1(hh)
            h_phi_k = h_phi_1 / hh - 1
            B_h = hh if self.config.solver_type == "bh1" else np.expm1(hh)
            R, b, fact = [], [], 1
            for i in range(1, order + 1):
                R.append(np.power(rks, i - 1))
                b.append(h_phi_k * fact / B_h)
                fact *= i + 1
                h_phi_k = h_phi_k / hh - 1 / fact
        return np.stack(R), np.array(b), h_phi_1, B_h

    def predictor_coefficients(self, i: int, order: int):
        """x_next = cx*x + sum_k cm[k]*m_{-k}  (m_0 newest x0-prediction)."""
        lam_t, alpha_t, sigma_t = self._als(i + 1)
        lam_s, _, sigma_s = self._als(i)
        h = lam_t - lam_s
        rks = [(self._als(i - k)[0] - lam_s) / h for k in range(1, order)] + [1.0]
        R, b, h_phi_1, B_h = self._rb(np.array(rks, dtype=np.float32), -h, order)
        cm = [0.0] * order
        cm[0] = -float(alpha_t * h_phi_1)
        if order > 1:
            rhos = np.array([0.5]) if order == 2 else np.linalg.solve(R[:-1, :-1], b[:-1])
            for k in range(1, order):
                cf = -float(alpha_t * B_h) * float(rhos[k - 1]) / float(rks[k - 1])
                cm[k] += cf      # D1_k = (m_{-k} - m_0) / r_k
                cm[0] -= cf
        return float(sigma_t / sigma_s), cm

    def corrector_coefficients(self, i: int, order: int):
        """x_corrected = cl*last_sample + sum_k cm[k]*m_{-k} + ct*model_t (m_0 = newest stored, before model_t)."""
        lam_t, alpha_t, sigma_t = self._als(i)
        lam_s, _, sigma_s = self._als(i - 1)
        h = lam_t - lam_s
        rks = [(self._als(i - (k + 1))[0] - lam_s) / h for k in range(1, order)] + [1.0]
        R, b, h_phi_1, B_h = self._rb(np.array(rks, dtype=np.float32), -h, order)
        rhos = np.array([0.5]) if order == 1 else np.linalg.solve(R, b)
        cm = [0.0] * order
        cm[0] = -float(alpha_t * h_phi_1)
        for k in range(1, order):
            cf = -float(alpha_t * B_h) * float(rhos[k - 1]) / float(rks[k - 1])
            cm[k] += cf
            cm[0] -= cf
        ct = -float(alpha_t * B_h) * float(rhos[-1])
        cm[0] -= ct
        return float(sigma_t / sigma_s), cm, ct

    def coefficient_table(self, device=None) -> torch.Tensor:
        """fp32 [n, 12] rows for ``pcdm_unipc_step`` (include/pcdm.h): the scalars ``step`` would compute at step i of a fresh run --
        the order bookkeeping (``lower_order_nums``, ``this_order``, ``lower_order_final``) depends on i and n only, so the whole
        multistep update is a per-step linear map on (x, eps, m1, m2, last_sample) with host-known coefficients."""
        c, n = self.config, len(self._ts_list)
        if c.solver_order > 2:
            raise NotImplementedError("fused UniPC: solver_order <= 2")
        rows = np.zeros((n, 12), dtype=np.float64)
        lower, this_order = 0, 1
        for i in range(n):
            _, alpha_t, sigma_t = self._als(i)
            rows[i, 0], rows[i, 1] = 1.0 / float(alpha_t), -float(sigma_t) / float(alpha_t)
            if i > 0 and (i - 1) not in c.disable_corrector:
                cl, cm, ct = self.corrector_coefficients(i, this_order)
                rows[i, 2], rows[i, 3], rows[i, 6] = 1.0, cl, ct
                rows[i, 4:4 + len(cm)] = cm
            order = min(c.solver_order, n - i) if c.lower_order_final else c.solver_order
            this_order = min(order, lower + 1)
            cx, cm = self.predictor_coefficients(i, this_order)
            rows[i, 7] = cx
            rows[i, 8:8 + len(cm)] = cm
            if lower < c.solver_order:
                lower += 1
        return torch.from_numpy(rows.astype(np.float32)).to(device)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, return_dict: bool = True):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            self._step_index = self._ts_list.index(int(timestep))
        i = self._step_index
        c = self.config
        e, x = _f32(model_output), _f32(sample)
        _, alpha_t, sigma_t = self._als(i)
        m_t = ops.lincomb(torch.empty_like(x), [x, e], [1.0 / float(alpha_t), -float(sigma_t) / float(alpha_t)])
        use_corrector = i > 0 and (i - 1) not in c.disable_corrector and self.last_sample is not None
        if use_corrector:
            cl, cm, ct = self.corrector_coefficients(i, self.this_order)
            xs = [self.last_sample] + [self.model_outputs[-(k + 1)] for k in range(self.this_order)] + [m_t]
            x = ops.lincomb(torch.empty_like(x), xs, [cl] + cm + [ct])
        for k in range(c.solver_order - 1):
            self.model_outputs[k] = self.model_outputs[k + 1]
        self.model_outputs[-1] = m_t
        order = min(c.solver_order, len(self._ts_list) - i) if c.lower_order_final else c.solver_order
        self.this_order = min(order, self.lower_order_nums + 1)
        self.last_sample = x
        cx, cm = self.predictor_coefficients(i, self.this_order)
        xs = [x] + [self.model_outputs[-(k + 1)] for k in range(self.this_order)]
        prev = ops.lincomb(torch.empty_like(x), xs, [cx] + cm).to(sample.dtype)
        if self.lower_order_nums < c.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1
        return (prev,) if not return_dict else SchedulerOutput(prev)


class DPMSolverMultistepScheduler(_Base):
    """diffusers 0.24.0 ``DPMSolverMultistepScheduler`` (DPM-Solver++, Lu et al. 2022, arXiv:2211.01095): "DPM++ 2M"
    (``algorithm_type="dpmsolver++"``) and its SDE form (``"sde-dpmsolver++"``), solver order 1 or 2, midpoint or heun, with or
    without Karras sigmas, ``timestep_spacing`` linspace / leading / trailing, epsilon prediction.

    Every update is linear in (x, eps, the previous x0-prediction m1, noise) with scalars that depend on the step index and the step
    count only, so ``coefficient_table`` holds the whole sampler and ``pcdm_dpmpp_step`` runs it in one kernel per step (the fused
    pipeline replays it from a hipGraph); ``step`` runs the same kernel with one host-computed row.

    Choices where diffusers 0.24 could not be checked here (upstream parity unverified; tools/compare_with_diffusers.py pins it):

    * The final sigma is ``((1 - ac[0]) / ac[0]) ** 0.5`` without Karras sigmas and the last Karras sigma repeated with them --
      never 0.  The final Karras step then has h = 0: its coefficients are the h -> 0 limits (x' = x), finite for every variant.
    * Karras timesteps are ``_sigma_to_t`` rounded to int64 and are NOT deduplicated: every sigma keeps its step, so
      ``len(timesteps) == num_inference_steps`` and ``len(sigmas) == num_inference_steps + 1`` always.  A timestep that occurs
      twice is looked up as diffusers' ``_init_step_index`` does (the second occurrence) when ``step`` starts mid-schedule.
    * Coefficients are float64 host math on the fp32 sigma table (diffusers evaluates them in fp32 tensors; the two differ at fp32
      rounding), stored as fp32.
    * The SDE noise of a step is ``torch.randn(x.shape, generator=generator)`` on the generator's device, drawn at every step
      including the last; the fused pipeline draws the same sequence up front (``_step_noise``).

    ``step`` has no ``eta`` parameter (the pipeline inspects the signature).  Stateful: one instance per in-flight sampling run."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                     sample_max_value=1.0, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                     euler_at_final=False, use_karras_sigmas=False, use_lu_lambdas=False, lambda_min_clipped=-float("inf"),
                     variance_type=None, timestep_spacing="linspace", steps_offset=0)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c.solver_type in ("logrho", "bh1", "bh2"):   # a UniPC config (from_config): diffusers maps it to midpoint as well
            c.solver_type = "midpoint"
        why = None
        if c.algorithm_type not in ("dpmsolver++", "sde-dpmsolver++"):
            why = f"algorithm_type {c.algorithm_type!r} (dpmsolver++ and sde-dpmsolver++ only)"
        elif c.solver_type not in ("midpoint", "heun"):
            why = f"solver_type {c.solver_type!r}"
        elif c.solver_order not in (1, 2):
            why = f"solver_order {c.solver_order} (1 or 2 only)"
        elif c.prediction_type != "epsilon":
            why = f"prediction_type {c.prediction_type!r} (epsilon only)"
        elif c.thresholding:
            why = "thresholding (not a linear update)"
        elif c.use_lu_lambdas:
            why = "use_lu_lambdas"
        elif c.lambda_min_clipped is not None and math.isfinite(float(c.lambda_min_clipped)):
            why = "a finite lambda_min_clipped"
        elif c.variance_type is not None:
            why = f"variance_type {c.variance_type!r} (learned variance)"
        elif c.timestep_spacing not in ("linspace", "leading", "trailing"):
            why = f"timestep_spacing {c.timestep_spacing!r}"
        if why is not None:
            raise NotImplementedError(f"DPMSolverMultistepScheduler: {why} is not implemented")
        self.set_timesteps(c.num_train_timesteps)

    def set_timesteps(self, num_inference_steps: int, device=None):
        c, T, n = self.config, self.config.num_train_timesteps, num_inference_steps
        if c.use_karras_sigmas:
            ts, self.sigmas = _karras_schedule(self.alphas_cumprod, n)
        else:
            if c.timestep_spacing == "linspace":
                ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
            elif c.timestep_spacing == "leading":
                ratio = T // (n + 1)
                ts = (np.arange(0, n + 1) * ratio).round()[::-1][:-1].copy().astype(np.int64) + c.steps_offset
            else:   # trailing
                ts = np.arange(T, 0, -T / n).round().copy().astype(np.int64) - 1
            ac = self.alphas_cumprod.numpy()
            sig = _train_sigmas(self.alphas_cumprod)
            sigmas = np.interp(ts, np.arange(0, len(sig)), sig)
            self.sigmas = np.concatenate([sigmas, [((1 - ac[0]) / ac[0]) ** 0.5]]).astype(np.float32)
        self.num_inference_steps = len(ts)
        self.timesteps = torch.from_numpy(ts).to(device)
        self._ts_list = [int(v) for v in ts]
        self.model_outputs: List[Optional[torch.Tensor]] = [None] * c.solver_order
        self.lower_order_nums = 0
        self._step_index: Optional[int] = None

    @property
    def step_index(self):
        return self._step_index

    def _order(self, i: int, lower_order_nums: int) -> int:
        """Solver order of step i (0.24: ``lower_order_nums`` and ``lower_order_final``)."""
        c, n = self.config, len(self._ts_list)
        final = i == n - 1 and (c.euler_at_final or (c.lower_order_final and n < 15))
        return 1 if (c.solver_order == 1 or lower_order_nums < 1 or final) else 2

    def step_row(self, i: int, order: Optional[int] = None) -> List[float]:
        """{a_x, a_e, p_x, p_m0, p_m1, p_z, 0, 0} of step i (``pcdm_dpmpp_step``): m0 = a_x x + a_e eps;
        x' = p_x x + p_m0 m0 + p_m1 m1 + p_z z.  ``order`` defaults to that of step i in a fresh run."""
        c = self.config
        if order is None:
            order = self._order(i, min(i, c.solver_order))
        alpha_s, sigma_s, lam_s = _alpha_sigma_lambda(float(self.sigmas[i]))
        alpha_t, sigma_t, lam_t = _alpha_sigma_lambda(float(self.sigmas[i + 1]))
        h = lam_t - lam_s
        a_x, a_e = 1.0 / alpha_s, -sigma_s / alpha_s
        sde = c.algorithm_type == "sde-dpmsolver++"
        em1 = math.expm1(-h)           # e^-h - 1
        e2m1 = math.expm1(-2.0 * h)    # e^-2h - 1
        if sde:
            p_x, p_m0, p_z = sigma_t / sigma_s * math.exp(-h), -alpha_t * e2m1, sigma_t * math.sqrt(max(-e2m1, 0.0))
        else:
            p_x, p_m0, p_z = sigma_t / sigma_s, -alpha_t * em1, 0.0
        p_m1 = 0.0
        if order == 2:
            h0 = lam_s - _alpha_sigma_lambda(float(self.sigmas[i - 1]))[2]
            # D1 = (m0 - m1) / r0 with r0 = h0 / h; the weight of D1 is multiplied by h / h0 in closed form, so h == 0 (the repeated
            # final Karras sigma) gives the finite limit 0 instead of 0 / 0
            if sde and c.solver_type == "midpoint":
                w = -0.5 * alpha_t * e2m1 * h / h0
            elif sde:   # heun: alpha_t ((1 - e^-2h) / (-2h) + 1) h / h0
                w = alpha_t * (0.5 * e2m1 + h) / h0
            elif c.solver_type == "midpoint":
                w = -0.5 * alpha_t * em1 * h / h0
            else:       # heun: alpha_t ((e^-h - 1) / h + 1) h / h0
                w = alpha_t * (em1 + h) / h0
            p_m0, p_m1 = p_m0 + w, -w
        return [a_x, a_e, p_x, p_m0, p_m1, p_z, 0.0, 0.0]

    def coefficient_table(self, device=None) -> torch.Tensor:
        """fp32 [n, 8] rows for ``pcdm_dpmpp_step`` (include/pcdm.h): the rows ``step`` would use at each step of a fresh run."""
        rows = [self.step_row(i) for i in range(len(self._ts_list))]
        return torch.tensor(rows, dtype=torch.float64).to(torch.float32).to(device)

    @property
    def stochastic(self) -> bool:
        return self.config.algorithm_type == "sde-dpmsolver++"

    def _init_step_index(self, timestep) -> int:
        idx = [k for k, v in enumerate(self._ts_list) if v == int(timestep)]
        if not idx:
            raise ValueError(f"timestep {int(timestep)} is not in this schedule")
        return idx[1] if len(idx) > 1 else idx[0]

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None,
             variance_noise: Optional[torch.Tensor] = None, return_dict: bool = True):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            self._step_index = self._init_step_index(timestep)
        i = self._step_index
        e, x = _f32(model_output), _f32(sample)
        noise = None
        if self.stochastic:
            if variance_noise is None:
                variance_noise = _step_noise(x.shape, generator, x.device)
            noise = _f32(variance_noise.to(x.device)).reshape(1, -1)
        coef = torch.tensor([self.step_row(i, self._order(i, self.lower_order_nums))], dtype=torch.float32, device=x.device)
        prev = x.clone()
        m = self.model_outputs[-1].clone() if self.model_outputs[-1] is not None else torch.zeros_like(x)
        ops.dpmpp_step(e, False, 1.0, prev, m, noise, coef)      # prev <- x', m <- this step's x0-prediction
        for k in range(self.config.solver_order - 1):
            self.model_outputs[k] = self.model_outputs[k + 1]
        self.model_outputs[-1] = m
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1
        prev = prev.to(sample.dtype)
        return (prev,) if not return_dict else SchedulerOutput(prev)


class _TableStepScheduler(_Base):
    """Shared machinery of the four samplers that run on ``pcdm_multistep_step`` (include/pcdm.h): each is, at every step of a fresh run, a
    linear map on (x, a saved sample xs, eps, three older eps h1..h3, noise) whose scalars depend on the step index and the step count only.
    ``_rows()`` holds them (float64 [len(timesteps), 12]); ``coefficient_table`` is the fused pipeline's device table, ``step`` runs the same
    kernel on one row with the history in slots this object owns.  The step index is a counter that ``set_timesteps`` resets.  Stateful: one
    instance per in-flight sampling run."""

    #: does ``scale_model_input`` change the sample (the row's ``in_scale`` is then not 1)?
    scales_input = False
    stochastic = False

    def _reset_state(self):
        self._step_index: Optional[int] = None
        self._slots: Optional[List[torch.Tensor]] = None     # [xs, h1, h2, h3]
        self._table: Optional[torch.Tensor] = None

    @property
    def step_index(self):
        return self._step_index

    def _rows(self) -> np.ndarray:
        raise NotImplementedError

    def coefficient_table(self, device=None) -> torch.Tensor:
        """fp32 [len(timesteps), 12] rows {c_x, c_s, c_0, c_1, c_2, c_3, c_z, in_scale, save, push, 0, 0} for ``pcdm_multistep_step`` and
        ``pcdm_assemble_input_ex`` (include/pcdm.h): the rows ``step`` uses at each step of a fresh run; float64 host math, stored as fp32."""
        return torch.from_numpy(self._rows().astype(np.float32)).to(device)

    def _init_step_index(self, timestep) -> int:
        return 0

    def _index(self, timestep) -> int:
        if self._step_index is None:
            self._step_index = self._init_step_index(timestep)
        return self._step_index

    def _run_step(self, model_output: torch.Tensor, sample: torch.Tensor, timestep, noise: Optional[torch.Tensor], return_dict: bool):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        i = self._index(timestep)
        if i >= len(self.timesteps):
            raise IndexError(f"step {i} of a schedule of {len(self.timesteps)} steps: call set_timesteps before another run")
        e, x = _f32(model_output), _f32(sample)
        if self._table is None or self._table.device != x.device:
            self._table = self.coefficient_table(device=x.device)
        if self._slots is None or self._slots[0].shape != x.shape or self._slots[0].device != x.device:
            self._slots = [torch.zeros_like(x) for _ in range(4)]
        prev = x.clone()
        z = None if noise is None else _f32(noise.to(x.device)).reshape(1, -1)
        ops.multistep_step(e, False, 1.0, prev, *self._slots, z, self._table[i:i + 1])
        self._step_index = i + 1
        prev = prev.to(sample.dtype)
        return (prev,) if not return_dict else SchedulerOutput(prev)


class _SigmaScheduler(_TableStepScheduler):
    """The sigma-space ("k-diffusion") schedule shared by Euler, Euler-ancestral and LMS in diffusers 0.24.0: float32 timesteps (fractional
    with ``timestep_spacing="linspace"``), ``sigma = sqrt((1 - ac) / ac)`` interpolated at them (fp32, as diffusers keeps the table) with a
    final 0, the sample held at scale ``sigma`` (``init_noise_sigma``) and divided by ``sqrt(sigma^2 + 1)`` in front of the UNet."""

    scales_input = True
    _has_karras = False

    def _check(self, name: str):
        c = self.config
        why = None
        if c.prediction_type != "epsilon":
            why = f"prediction_type {c.prediction_type!r} (epsilon only)"
        elif c.timestep_spacing not in ("linspace", "leading", "trailing"):
            why = f"timestep_spacing {c.timestep_spacing!r}"
        elif c.get("interpolation_type", "linear") != "linear" and name == "EulerDiscreteScheduler":
            why = f"interpolation_type {c.interpolation_type!r} (linear only)"
        elif c.get("timestep_type", "discrete") != "discrete" and name == "EulerDiscreteScheduler":
            why = f"timestep_type {c.timestep_type!r} (discrete only)"
        elif c.get("rescale_betas_zero_snr", False):
            why = "rescale_betas_zero_snr"
        if why is not None:
            raise NotImplementedError(f"{name}: {why} is not implemented")

    def set_timesteps(self, num_inference_steps: int, device=None):
        c, T, n = self.config, self.config.num_train_timesteps, num_inference_steps
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n, dtype=np.float32)[::-1].copy()
        elif c.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float32) + c.steps_offset
        else:   # trailing
            ts = (np.arange(T, 0, -T / n)).round().copy().astype(np.float32) - 1
        sig = _train_sigmas(self.alphas_cumprod)
        sigmas = np.interp(ts, np.arange(0, len(sig)), sig)
        if self._has_karras and c.get("use_karras_sigmas", False):   # timesteps of the Karras sigmas stay fractional (not rounded)
            sigmas = _convert_to_karras(sigmas, n)
            ts = _sigma_to_t(sigmas, np.log(sig)).astype(np.float32)
        self.sigmas = np.concatenate([sigmas, [0.0]]).astype(np.float32)
        self.num_inference_steps = n
        self.timesteps = torch.from_numpy(ts).to(device)
        self._ts_list = [float(v) for v in ts]
        self._reset_state()

    @property
    def init_noise_sigma(self) -> float:
        smax = float(np.max(self.sigmas))
        return smax if self.config.timestep_spacing in ("linspace", "trailing") else math.sqrt(smax * smax + 1.0)

    def _in_scale(self, i: int) -> float:
        s = float(self.sigmas[i])
        return 1.0 / math.sqrt(s * s + 1.0)

    def _init_step_index(self, timestep) -> int:
        if timestep is None:
            return 0
        t = float(timestep)
        idx = [k for k, v in enumerate(self._ts_list) if v == t]
        if not idx:
            raise ValueError(f"timestep {t} is not in this schedule")
        return idx[1] if len(idx) > 1 else idx[0]     # (as diffusers: a repeated timestep means the second occurrence when a run starts there)

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        """sample / sqrt(sigma_i^2 + 1) at the current step (one ``pcdm_lincomb`` launch; the fused pipeline folds the same fp32 scalar
        into ``pcdm_assemble_input_ex``)."""
        i = self._index(timestep)
        x = _f32(sample)
        return ops.lincomb(torch.empty_like(x), [x], [self._in_scale(i)]).to(sample.dtype)

    def _blank_rows(self) -> np.ndarray:
        n = len(self._ts_list)
        rows = np.zeros((n, ops.MS_ROW), dtype=np.float64)
        rows[:, ops.MS_CX] = 1.0
        rows[:, ops.MS_IN_SCALE] = [self._in_scale(i) for i in range(n)]
        return rows


class EulerDiscreteScheduler(_SigmaScheduler):
    """diffusers 0.24.0 ``EulerDiscreteScheduler`` restated (that source could not be read here: parity is against the float64 restatement
    in tests/test_karras_samplers.py, upstream parity is unpinned; tools/compare_with_diffusers.py checks it where diffusers is installed).
    Epsilon prediction, ``interpolation_type="linear"``, with or without Karras sigmas, ``timestep_spacing`` linspace / leading / trailing;
    the step is the deterministic one, ``s_churn = 0``:  x' = x + (sigma_{i+1} - sigma_i) eps."""

    _has_karras = True
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     prediction_type="epsilon", interpolation_type="linear", use_karras_sigmas=False, timestep_spacing="linspace",
                     steps_offset=0)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self._check("EulerDiscreteScheduler")
        self.set_timesteps(self.config.num_train_timesteps)

    def _rows(self) -> np.ndarray:
        rows = self._blank_rows()
        s = self.sigmas.astype(np.float64)
        rows[:, ops.MS_C0] = s[1:] - s[:-1]
        return rows

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, s_churn: float = 0.0, s_tmin: float = 0.0,
             s_tmax: float = float("inf"), s_noise: float = 1.0, generator=None, return_dict: bool = True):
        if s_churn != 0.0:
            raise NotImplementedError("EulerDiscreteScheduler.step: s_churn != 0 (stochastic churn) is not implemented")
        return self._run_step(model_output, sample, timestep, None, return_dict)


class EulerAncestralDiscreteScheduler(_SigmaScheduler):
    """diffusers 0.24.0 ``EulerAncestralDiscreteScheduler`` restated (parity as for ``EulerDiscreteScheduler``), epsilon prediction:
    sigma_up = sqrt(sigma_to^2 (sigma_from^2 - sigma_to^2) / sigma_from^2), sigma_down = sqrt(sigma_to^2 - sigma_up^2),
    x' = x + (sigma_down - sigma_from) eps + sigma_up z.  z is ``_step_noise``: one draw per step in step order (the last step draws too,
    with weight 0), which the fused pipeline makes up front into its per-step table."""

    stochastic = True
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self._check("EulerAncestralDiscreteScheduler")
        self.set_timesteps(self.config.num_train_timesteps)

    def _rows(self) -> np.ndarray:
        rows = self._blank_rows()
        s = self.sigmas.astype(np.float64)
        s_from, s_to = s[:-1], s[1:]
        up = np.sqrt(s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2)
        down = np.sqrt(s_to ** 2 - up ** 2)
        rows[:, ops.MS_C0] = down - s_from
        rows[:, ops.MS_CZ] = up
        return rows

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None,
             variance_noise: Optional[torch.Tensor] = None, return_dict: bool = True):
        if variance_noise is None:
            variance_noise = _step_noise(sample.shape, generator, sample.device)
        return self._run_step(model_output, sample, timestep, variance_noise, return_dict)


def _lms_coefficients(sigmas: np.ndarray, i: int, order: int) -> List[float]:
    """c_k, k < order: the integral from sigma_i to sigma_{i+1} of the Lagrange basis polynomial of node sigma_{i-k} over the nodes
    sigma_i .. sigma_{i-order+1}.  Closed form in float64: the polynomial is expanded in u = tau - sigma_i (small numbers near the
    interval), integrated term by term and evaluated at u = sigma_{i+1} - sigma_i."""
    s = np.asarray(sigmas, dtype=np.float64)
    d = s[i + 1] - s[i]
    out = []
    for k in range(order):
        roots = [s[i - j] - s[i] for j in range(order) if j != k]
        den = float(np.prod([s[i - k] - s[i - j] for j in range(order) if j != k])) if roots else 1.0
        poly = np.poly(roots) if roots else np.array([1.0])      # highest power first
        out.append(float(np.polyval(np.polyint(poly), d)) / den)
    return out


class LMSDiscreteScheduler(_SigmaScheduler):
    """diffusers 0.24.0 ``LMSDiscreteScheduler`` restated (parity as for ``EulerDiscreteScheduler``), epsilon prediction, order 4:
    x' = x + sum_k c_k eps_{i-k} over the last min(i + 1, 4) model outputs, c_k the integral of the Lagrange basis polynomial over
    [sigma_i, sigma_{i+1}].  diffusers integrates with adaptive quadrature (scipy, 1e-4 relative); here the polynomial is integrated in
    CLOSED FORM in float64 (``_lms_coefficients``), which is the exact value that quadrature approximates.  scipy is not a dependency."""

    _has_karras = True
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     use_karras_sigmas=False, prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0)
    lms_order = 4

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self._check("LMSDiscreteScheduler")
        self.set_timesteps(self.config.num_train_timesteps)

    def _rows(self) -> np.ndarray:
        rows = self._blank_rows()
        for i in range(rows.shape[0]):
            order = min(i + 1, self.lms_order)
            rows[i, ops.MS_C0:ops.MS_C0 + order] = _lms_coefficients(self.sigmas, i, order)
        rows[:, ops.MS_PUSH] = 1.0
        return rows

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, order: int = 4, return_dict: bool = True):
        if order != self.lms_order:
            raise NotImplementedError("LMSDiscreteScheduler.step: order 4 only")
        return self._run_step(model_output, sample, timestep, None, return_dict)


class PNDMScheduler(_TableStepScheduler):
    """diffusers 0.24.0 ``PNDMScheduler`` restated (parity as for ``EulerDiscreteScheduler``) in its ``skip_prk_steps=True`` form, the
    PLMS sampler of the SD-2.1 ``scheduler_config.json``; epsilon prediction.  The Runge-Kutta warm-up is not built: ``skip_prk_steps``
    defaults to True HERE (diffusers: False) and an explicit False is refused.

    ``timesteps`` repeats the second entry, so n steps are n + 1 UNet calls.  Call 0 steps with eps and saves the sample; call 1 redoes
    that step from the SAVED sample with (eps + e_1) / 2 and pushes no history; from then on the 2-, 3- and 4-term Adams-Bashforth weights.
    x' = sqrt(a_p / a_t) x - (a_p - a_t) e' / (a_t sqrt(1 - a_p) + sqrt(a_t (1 - a_t) a_p))."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     skip_prk_steps=True, set_alpha_to_one=False, prediction_type="epsilon", timestep_spacing="leading", steps_offset=0)
    _AB = {1: (1.0,), 2: (3 / 2, -1 / 2), 3: (23 / 12, -16 / 12, 5 / 12), 4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        why = None
        if not c.skip_prk_steps:
            why = "skip_prk_steps=False (the Runge-Kutta warm-up steps)"
        elif c.prediction_type != "epsilon":
            why = f"prediction_type {c.prediction_type!r} (epsilon only)"
        elif c.timestep_spacing not in ("linspace", "leading", "trailing"):
            why = f"timestep_spacing {c.timestep_spacing!r}"
        if why is not None:
            raise NotImplementedError(f"PNDMScheduler: {why} is not implemented")
        self.final_alpha_cumprod = 1.0 if c.set_alpha_to_one else float(self._ac[0])
        self._reset_state()

    def set_timesteps(self, num_inference_steps: int, device=None):
        c, T, n = self.config, self.config.num_train_timesteps, num_inference_steps
        if n > T:
            raise ValueError("`num_inference_steps` cannot be larger than `num_train_timesteps`")
        if c.timestep_spacing == "leading":
            t = (np.arange(0, n) * (T // n)).round() + c.steps_offset
        elif c.timestep_spacing == "linspace":
            t = np.linspace(0, T - 1, n).round()
        else:   # trailing
            t = np.round(np.arange(T, 0, -T / n))[::-1] - 1
        t = t.astype(np.int64)
        ts = np.concatenate([t[:-1], t[-2:-1], t[-1:]])[::-1].copy()
        self.num_inference_steps = n
        self.timesteps = torch.from_numpy(ts).to(device)
        self._ts_list = [int(v) for v in ts]
        self._reset_state()

    def _transfer(self, t: int, tp: int) -> Tuple[float, float]:
        """(c_x, c_e) of ``_get_prev_sample``: x' = c_x x + c_e e'."""
        a_t = float(self._ac[t])
        a_p = float(self._ac[tp]) if tp >= 0 else self.final_alpha_cumprod
        den = a_t * math.sqrt(1 - a_p) + math.sqrt(a_t * (1 - a_t) * a_p)
        return math.sqrt(a_p / a_t), -(a_p - a_t) / den

    def _rows(self) -> np.ndarray:
        m = len(self._ts_list)
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        rows = np.zeros((m, ops.MS_ROW), dtype=np.float64)
        rows[:, ops.MS_IN_SCALE] = 1.0
        for k, t in enumerate(self._ts_list):
            if k == 1:       # the repeated timestep: from the saved sample, over the same interval as call 0, with the averaged eps
                cx, ce = self._transfer(t + ratio, t)
                rows[k, ops.MS_CS], rows[k, ops.MS_C0], rows[k, ops.MS_C1] = cx, 0.5 * ce, 0.5 * ce
                continue
            cx, ce = self._transfer(t, t - ratio)
            w = self._AB[1 if k == 0 else min(k, 4)]
            rows[k, ops.MS_CX] = cx
            rows[k, ops.MS_C0:ops.MS_C0 + len(w)] = [ce * v for v in w]
            rows[k, ops.MS_PUSH] = 1.0
            rows[k, ops.MS_SAVE] = 1.0 if k == 0 else 0.0
        return rows

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, return_dict: bool = True):
        return self._run_step(model_output, sample, timestep, None, return_dict)


class UnCLIPScheduler(_Base):
    """Stand-in for diffusers 0.24.0 ``UnCLIPScheduler`` at the stage-1 prior's call sites
    (/root/reference/src/pipelines/stage1_prior_pipeline.py:439-440 ``set_timesteps`` / ``timesteps``, :279
    ``init_noise_sigma``, :478-483 ``step(pred, timestep=t, sample=latents, prev_timestep=...)``).
    Class defaults are diffusers'; the Kandinsky-2.2 prior's ``scheduler_config.json`` (prediction_type "sample",
    clip_sample_range 10, "fixed_small_log") arrives through ``from_config`` / ``from_pretrained``.
    Scalar coefficient math on the host (float64), the tensor update is one HIP kernel (``pcdm_unclip_step``)."""

    _defaults = dict(num_train_timesteps=1000, variance_type="fixed_small_log", clip_sample=True, clip_sample_range=1.0,
                     prediction_type="epsilon", beta_schedule="squaredcos_cap_v2", trained_betas=None)
    KANDINSKY22_PRIOR = dict(num_train_timesteps=1000, variance_type="fixed_small_log", clip_sample=True,
                             clip_sample_range=10.0, prediction_type="sample", beta_schedule="squaredcos_cap_v2")

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c.variance_type != "fixed_small_log" or c.prediction_type not in ("epsilon", "sample"):
            raise NotImplementedError("UnCLIP variant outside the stage-1 path (learned_range variance / v-prediction)")
        self._betas64 = self.betas.numpy().astype(np.float64)

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = (self.config.num_train_timesteps - 1) / (num_inference_steps - 1)
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
        self.timesteps = torch.from_numpy(ts).to(device)

    def step_coefficients(self, t: int, prev_t: Optional[int] = None):
        """(p_x, p_e, clip, c_x0, c_x, c_noise): x0 = clamp(p_x x + p_e pred, +-clip); prev = c_x0 x0 + c_x x + c_noise z."""
        c = self.config
        if prev_t is None:
            prev_t = t - 1
        a_t = float(self._ac[t])
        a_prev = float(self._ac[prev_t]) if prev_t >= 0 else 1.0
        b_t, b_prev = 1 - a_t, 1 - a_prev
        if prev_t == t - 1:
            beta = float(self._betas64[t])
            alpha = 1 - beta
        else:
            beta = 1 - a_t / a_prev
            alpha = 1 - beta
        if c.prediction_type == "epsilon":
            p_x, p_e = 1 / math.sqrt(a_t), -math.sqrt(1 - a_t) / math.sqrt(a_t)
        else:
            p_x, p_e = 0.0, 1.0
        clip = float(c.clip_sample_range) if c.clip_sample else 0.0
        std = math.exp(0.5 * math.log(max(b_prev / b_t * beta, 1e-20))) if t > 0 else 0.0
        return p_x, p_e, clip, math.sqrt(a_prev) * beta / b_t, math.sqrt(alpha) * b_prev / b_t, std

    def step(self, model_output, timestep, sample, prev_timestep=None, generator=None, variance_noise=None,
             return_dict: bool = True):
        t = int(timestep)
        co = self.step_coefficients(t, None if prev_timestep is None else int(prev_timestep))
        e, x = _f32(model_output), _f32(sample)
        noise = None
        if co[5] > 0:
            if variance_noise is None:
                variance_noise = torch.randn(e.shape, generator=generator, dtype=torch.float32,
                                             device=generator.device if generator is not None else e.device)
            noise = _f32(variance_noise.to(e.device))
        prev = ops.unclip_step(e, False, 0.0, x, noise, torch.empty_like(x), (*co, 1.0, 0.0)).to(sample.dtype)
        return (prev,) if not return_dict else SchedulerOutput(prev)
