"""MI355X-native stand-ins for the reference's ``pipe.scheduler`` objects.

The reference uses three diffusers 0.24.0 schedulers at this boundary:
``UniPCMultistepScheduler`` (stage2_batchtest_inpaint_model.py:132), ``DDIMScheduler``
(pcdms_kaggle_demo.ipynb cell 15 -- the configuration BASELINE.json's metric names) and
``DDPMScheduler`` (stage2_train_inpaint_model.py:175,361).  The pipelines type the slot as any
``KarrasDiffusionSchedulers`` member; of those, ``DPMSolverMultistepScheduler`` ("DPM++ 2M", with or without
Karras sigmas, and its SDE form) is here too.  Call sites:
src/pipelines/stage2_inpaint_pipeline.py:472-473 (set_timesteps / timesteps), :386
(init_noise_sigma), :494 (order), :500 (scale_model_input), :519 (step; ``eta`` / ``generator`` are
passed only if ``inspect.signature(step)`` has them, :313-321).

Coefficient math is scalar host code (float64, tables in fp32 where diffusers keeps them in fp32);
every tensor update is a hand-written HIP kernel from libpcdm.so (``pcdm_lincomb`` /
``pcdm_cfg_step`` / ``pcdm_dpmpp_step``).  Tensors must be on the GPU: there is no CPU tensor path.
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
