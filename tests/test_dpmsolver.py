"""DPM-Solver++ multistep sampling ("DPM++ 2M", Karras sigmas, SDE form): ``pcdms_amd.DPMSolverMultistepScheduler``, the
``pcdm_dpmpp_step`` kernel and the fused (graph-captured) pipeline path.

Yardstick: ``DPMRef`` below, a float64 restatement of the DPM-Solver++ update formulas (Lu et al. 2022, arXiv:2211.01095) with the
diffusers 0.24 order bookkeeping and final-sigma rules.  Parity is vs this in-repo restatement; upstream is unverified
(tools/compare_with_diffusers.py pins it where diffusers is installed)."""
from __future__ import annotations

import json
import math

import numpy as np
import pytest
import torch

from oracle.pipeline import stage2_sample, synth_inputs
from oracle.unet import UNetConfig, synth_state_dict
from pcdms_amd import ops
from pcdms_amd.pipeline import Stage2_InpaintDiffusionPipeline
from pcdms_amd.schedulers import DPMSolverMultistepScheduler, UniPCMultistepScheduler, _karras_schedule
from pcdms_amd.unet import Stage2_InapintUNet2DConditionModel
from tests.test_schedulers import SD21
from tests.test_unet import _kwargs


@pytest.fixture(autouse=True)
def _modes_compared_on_identical_launches(request, monkeypatch):
    """As in tests/test_pipeline.py: the fused sampler is held to the reference-semantics loop of the same library, a comparison of
    the two SCHEDULER formulations on identical UNet launches.  The CFG-shared prefix (which only the fused sampler can promise) puts
    other tile configurations, i.e. other fp32 summation orders, under the first two convolutions of one side: switched off here."""
    import pcdms_amd.unet as U
    monkeypatch.setattr(U, "SHARE_CFG_PREFIX", False)


# ---------------------------------------------------------------------------------------------------------------------------------
class DPMRef:
    """float64 DPM-Solver++ (dpmsolver++ / sde-dpmsolver++, order <= 2, midpoint / heun) on the SD-2.1 training table.  Sigmas are
    kept as an fp32 table (as diffusers keeps them); everything after that is float64.  ``step`` returns the input dtype."""

    order = 1
    init_noise_sigma = 1.0

    def __init__(self, algorithm_type="dpmsolver++", solver_type="midpoint", solver_order=2, use_karras_sigmas=False,
                 lower_order_final=True, euler_at_final=False):
        betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
        self.ac = torch.cumprod(1.0 - betas, dim=0).numpy()
        self.sde = algorithm_type == "sde-dpmsolver++"
        self.heun = solver_type == "heun"
        self.solver_order, self.karras = solver_order, use_karras_sigmas
        self.lower_order_final, self.euler_at_final = lower_order_final, euler_at_final
        self.noises = None   # optional list of per-step noise tensors (SDE)

    def set_timesteps(self, n, device=None):
        sig = ((1 - self.ac) / self.ac) ** 0.5                                  # fp32, increasing with t
        if self.karras:
            lo, hi = float(sig[0]), float(sig[-1])
            ramp = np.linspace(0, 1, n)
            s = (hi ** (1 / 7) + ramp * (lo ** (1 / 7) - hi ** (1 / 7))) ** 7
            ts = np.round(np.interp(np.log(s), np.log(sig.astype(np.float64)), np.arange(1000))).astype(np.int64)
            self.sigmas = np.concatenate([s, s[-1:]]).astype(np.float32)
        else:
            ts = np.linspace(0, 999, n + 1).round()[::-1][:-1].astype(np.int64)
            s = np.interp(ts, np.arange(1000), sig)
            self.sigmas = np.concatenate([s, [sig[0]]]).astype(np.float32)
        self.timesteps = torch.from_numpy(ts.copy())
        self.n, self.i, self.m1 = n, 0, None

    def scale_model_input(self, x, t=None):
        return x

    def _als(self, i):
        s = float(self.sigmas[i])
        a = 1 / math.sqrt(s * s + 1)
        return a, s * a, math.log(a) - math.log(s * a)

    def order_of(self, i):
        final = i == self.n - 1 and (self.euler_at_final or (self.lower_order_final and self.n < 15))
        return 1 if (self.solver_order == 1 or i == 0 or final) else 2

    def update(self, i, order, x, e, m1, z):
        """(x', m0) of step i in float64."""
        alpha_s, sigma_s, lam_s = self._als(i)
        alpha_t, sigma_t, lam_t = self._als(i + 1)
        h = lam_t - lam_s
        m0 = (x - sigma_s * e) / alpha_s
        if self.sde:
            xn = (sigma_t / sigma_s * math.exp(-h)) * x + alpha_t * (1 - math.exp(-2 * h)) * m0 \
                + sigma_t * math.sqrt(1 - math.exp(-2 * h)) * z
        else:
            xn = (sigma_t / sigma_s) * x - alpha_t * (math.exp(-h) - 1) * m0
        if order == 2:
            h0 = lam_s - self._als(i - 1)[2]
            d1 = (m0 - m1) * (h / h0)                                               # D1 = (m0 - m1) / r0, r0 = h0 / h
            if self.sde:
                wgt = 0.5 * alpha_t * (1 - math.exp(-2 * h)) if not self.heun else \
                    (alpha_t * ((1 - math.exp(-2 * h)) / (-2 * h) + 1) if h != 0 else 0.0)
            else:
                wgt = -0.5 * alpha_t * (math.exp(-h) - 1) if not self.heun else \
                    (alpha_t * ((math.exp(-h) - 1) / h + 1) if h != 0 else 0.0)   # (h -> 0 limit: 0)
            xn = xn + wgt * d1
        return xn, m0

    def step(self, eps, t, x, variance_noise=None):
        i = self.i
        if self.sde and variance_noise is None:
            variance_noise = self.noises[i]
        z = None if variance_noise is None else variance_noise.double().cpu()
        xn, m0 = self.update(i, self.order_of(i), x.double().cpu(), eps.double().cpu(), self.m1, z)
        self.m1, self.i = m0, i + 1
        return xn.to(x.dtype)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: schedule known answers, coefficient table, configuration surface
def test_known_answers_sd21():
    d = DPMSolverMultistepScheduler.from_config(SD21)
    d.set_timesteps(20)
    u = UniPCMultistepScheduler.from_config(SD21)
    u.set_timesteps(20)
    assert d.timesteps.dtype == torch.int64 and d.timesteps.tolist() == u.timesteps.tolist()
    assert d.timesteps.tolist() == [999, 949, 899, 849, 799, 749, 699, 649, 599, 549, 500, 450, 400, 350, 300, 250, 200, 150, 100, 50]
    assert np.allclose(d.sigmas[:3], [14.614647, 10.90424, 8.302806], rtol=1e-6)
    assert float(d.sigmas[-1]) == pytest.approx(0.02916753, rel=1e-6)          # final sigma of 0.24: sigma of ac[0], not 0
    assert d.step_index is None and d.order == 1 and d.init_noise_sigma == 1.0
    k = DPMSolverMultistepScheduler.from_config(SD21, use_karras_sigmas=True)
    k.set_timesteps(20)
    s = np.asarray(k.sigmas, dtype=np.float64)
    assert len(s) == 21 and s[0] == pytest.approx(14.614647, rel=1e-6) and s[-2] == pytest.approx(0.02916753, rel=1e-6)
    assert s[-1] == s[-2]                                                       # last Karras sigma repeated
    r = s[:-1] ** (1 / 7)
    assert np.allclose(np.diff(r), (r[-1] - r[0]) / 19, rtol=0, atol=1e-6)     # rho = 7 spacing
    ts = k.timesteps
    assert ts.dtype == torch.int64 and ts[0] == 999 and ts[-1] == 0 and bool((ts[1:] <= ts[:-1]).all())
    uk = UniPCMultistepScheduler.from_config(SD21, use_karras_sigmas=True)
    uk.set_timesteps(20)
    assert uk.timesteps.tolist() == _karras_schedule(uk.alphas_cumprod, 20)[0].tolist() == ts.tolist()
    assert np.array_equal(uk.sigmas, k.sigmas) and torch.isfinite(uk.coefficient_table()).all()


def test_karras_timesteps_are_not_deduplicated():
    """Pinned choice (docstring): repeated rounded Karras timesteps stay, so every sigma keeps its step."""
    k = DPMSolverMultistepScheduler.from_config(SD21, use_karras_sigmas=True)
    k.set_timesteps(50)
    ts = k.timesteps.tolist()
    assert len(ts) == 50 and len(set(ts)) < 50 and len(k.sigmas) == 51 and k.num_inference_steps == 50
    ref = DPMRef(use_karras_sigmas=True)
    ref.set_timesteps(50)
    assert ts == ref.timesteps.tolist() and np.allclose(k.sigmas, ref.sigmas, rtol=1e-6)


@pytest.mark.parametrize("n", [5, 14, 15, 20, 50])
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("solver_type", ["midpoint", "heun"])
@pytest.mark.parametrize("algo", ["dpmsolver++", "sde-dpmsolver++"])
def test_coefficient_table_vs_reference(algo, solver_type, order, karras, n):
    """Row i of the table, applied in float64 to random (x, eps, m1, z), equals the reference's step i of a fresh run."""
    kw = dict(algorithm_type=algo, solver_type=solver_type, solver_order=order, use_karras_sigmas=karras)
    d = DPMSolverMultistepScheduler.from_config(SD21, **kw)
    d.set_timesteps(n)
    ref = DPMRef(**kw)
    ref.set_timesteps(n)
    assert d.timesteps.tolist() == ref.timesteps.tolist() and np.allclose(d.sigmas, ref.sigmas, rtol=1e-6)
    tab = d.coefficient_table()
    assert tab.shape == (n, 8) and tab.dtype == torch.float32 and torch.isfinite(tab).all()
    assert (tab[:, 6:] == 0).all() and ((tab[:, 5] != 0).any() if algo.startswith("sde") else (tab[:, 5] == 0).all())
    g = torch.Generator().manual_seed(n)
    for i in range(n):
        x, e, m1, z = (torch.randn(64, generator=g, dtype=torch.float64) for _ in range(4))
        c = tab[i].double()
        m0 = c[0] * x + c[1] * e
        xn = c[2] * x + c[3] * m0 + c[4] * m1 + c[5] * z
        want, want_m0 = ref.update(i, ref.order_of(i), x, e, m1, z if ref.sde else None)
        assert _rel(m0, want_m0) <= 1e-6 and _rel(xn, want) <= 1e-6, (i, _rel(m0, want_m0), _rel(xn, want))
        if ref.order_of(i) == 1:
            assert c[4] == 0


def test_final_karras_step_is_finite_and_identity():
    """h == 0 on the repeated final Karras sigma: every variant's coefficients are the finite h -> 0 limits (x' = x)."""
    for algo in ("dpmsolver++", "sde-dpmsolver++"):
        for st in ("midpoint", "heun"):
            d = DPMSolverMultistepScheduler.from_config(SD21, algorithm_type=algo, solver_type=st, use_karras_sigmas=True)
            d.set_timesteps(20)                                                 # n >= 15: the last step stays second order
            row = d.coefficient_table()[-1]
            assert torch.isfinite(row).all()
            assert row[2] == pytest.approx(1.0, abs=1e-6) and abs(float(row[3])) < 1e-6 and abs(float(row[4])) < 1e-6
            assert abs(float(row[5])) < 1e-6


def test_euler_at_final_and_lower_order_final():
    def orders(n, **kw):
        d = DPMSolverMultistepScheduler.from_config(SD21, **kw)
        d.set_timesteps(n)
        return [int(r[4] != 0) + 1 for r in d.coefficient_table()]
    assert orders(n=10) == [1] + [2] * 8 + [1]
    assert orders(n=20) == [1] + [2] * 19
    assert orders(n=20, euler_at_final=True) == [1] + [2] * 18 + [1]
    assert orders(n=10, lower_order_final=False) == [1] + [2] * 9
    assert orders(n=10, solver_order=1) == [1] * 10


@pytest.mark.parametrize("bad", [dict(solver_order=3), dict(algorithm_type="dpmsolver"), dict(algorithm_type="sde-dpmsolver"),
                                 dict(thresholding=True), dict(prediction_type="v_prediction"), dict(use_lu_lambdas=True),
                                 dict(lambda_min_clipped=-5.1), dict(variance_type="learned_range"), dict(solver_type="other"),
                                 dict(timestep_spacing="karras")])
def test_unsupported_configs_are_refused(bad):
    with pytest.raises(NotImplementedError):
        DPMSolverMultistepScheduler.from_config(SD21, **bad)


def test_spacings_and_config_round_trip(tmp_path):
    for sp in ("linspace", "leading", "trailing"):
        d = DPMSolverMultistepScheduler.from_config(SD21, timestep_spacing=sp)
        d.set_timesteps(10)
        assert d.timesteps.dtype == torch.int64 and len(d.timesteps) == 10 and len(d.sigmas) == 11
        assert torch.isfinite(d.coefficient_table()).all()
    assert DPMSolverMultistepScheduler.from_config(SD21, timestep_spacing="trailing", num_train_timesteps=1000).timesteps[0] == 999
    u = UniPCMultistepScheduler.from_config(SD21)
    d = DPMSolverMultistepScheduler.from_config(u.config)
    assert d.config.beta_schedule == "scaled_linear" and d.config.algorithm_type == "dpmsolver++" and d.config.solver_type == "midpoint"
    assert d.config.skip_prk_steps is True and d.config.solver_order == 2
    u2 = UniPCMultistepScheduler.from_config(d.config)
    assert u2.config.solver_type == "bh2" and u2.config.steps_offset == 1 and u2.config.beta_end == 0.012
    import inspect
    params = inspect.signature(d.step).parameters
    assert "eta" not in params and "generator" in params and "variance_noise" in params


def test_pipeline_from_pretrained_resolves_dpm(tmp_path):
    from safetensors.torch import save_file

    from tests.test_from_pretrained import SD21_UNET_JSON
    root = tmp_path / "sd21"
    for sub in ("unet", "scheduler"):
        (root / sub).mkdir(parents=True)
    (root / "unet" / "config.json").write_text(json.dumps(SD21_UNET_JSON))
    stock = UNetConfig.tiny(in_channels=4, class_embed_type=None, projection_class_embeddings_input_dim=None)
    save_file({k: v.contiguous() for k, v in synth_state_dict(stock, seed=1).items()}, str(root / "unet" / "diffusion_pytorch_model.safetensors"))
    (root / "scheduler" / "scheduler_config.json").write_text(json.dumps({
        "_class_name": "DPMSolverMultistepScheduler", "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085,
        "num_train_timesteps": 1000, "algorithm_type": "sde-dpmsolver++", "use_karras_sigmas": True, "steps_offset": 1}))
    pipe = Stage2_InpaintDiffusionPipeline.from_pretrained(root)
    assert type(pipe.scheduler) is DPMSolverMultistepScheduler
    assert pipe.scheduler.config.algorithm_type == "sde-dpmsolver++" and pipe.scheduler.config.use_karras_sigmas


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel and scheduler.step: lane emulator in the CPU suite, MI355X under -m gpu
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("with_noise", [False, True])
def test_dpmpp_step_kernel(backend, cfg, with_noise):
    dev = backend.device
    g = torch.Generator().manual_seed(5)
    steps, n = 4, 3 * 257                                                        # (not a multiple of the block size)
    coef = torch.randn(steps, 8, generator=g, dtype=torch.float64)
    coef[:, 6:] = 0
    x, m1 = torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64)
    eps = torch.randn((2 if cfg else 1) * n, generator=g, dtype=torch.float64)
    noise = torch.randn(steps, n, generator=g, dtype=torch.float64)
    gs, st = 3.5, 2
    e = eps[:n] + gs * (eps[n:] - eps[:n]) if cfg else eps
    c = coef.float().double()[st]
    m0 = c[0] * x + c[1] * e
    want = c[2] * x + c[3] * m0 + c[4] * m1 + (c[5] * noise[st] if with_noise else 0)
    xd, m1d = x.float().to(dev), m1.float().to(dev)
    step = torch.tensor([st], dtype=torch.int32, device=dev)
    ops.dpmpp_step(eps.float().to(dev), cfg, gs, xd, m1d, noise.float().to(dev) if with_noise else None, coef.float().to(dev), step)
    backend.sync()
    assert _rel(xd, want) <= 1e-6 and _rel(m1d, m0) <= 1e-6                     # x and the history slot updated in place
    from pcdms_amd import _lib
    assert _lib.lib().pcdm_dpmpp_step(eps.data_ptr(), 0, 1.0, xd.data_ptr(), m1d.data_ptr(), None, None, steps, None, None, n, None) == -1
    assert _lib.lib().pcdm_dpmpp_step(eps.data_ptr(), 0, 1.0, xd.data_ptr(), m1d.data_ptr(), None, coef.data_ptr(), steps, None, None, 0, None) == -1


@pytest.mark.parametrize("variant", ["2m", "2m_heun_karras", "sde", "sde_heun_karras"])
def test_step_trajectory_vs_reference(backend, variant):
    """20 steps of ``scheduler.step`` with eps a fixed affine function of x (SDE: injected ``variance_noise``) vs ``DPMRef``."""
    dev = backend.device
    kw = dict(algorithm_type="sde-dpmsolver++" if variant.startswith("sde") else "dpmsolver++",
              solver_type="heun" if "heun" in variant else "midpoint", use_karras_sigmas="karras" in variant)
    g = torch.Generator().manual_seed(11)
    shape = (2, 4, 6, 10)
    x0, c = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    noises = [torch.randn(shape, generator=g) for _ in range(20)]
    d = DPMSolverMultistepScheduler.from_config(SD21, **kw)
    d.set_timesteps(20, device=dev)
    ref = DPMRef(**kw)
    ref.set_timesteps(20)
    x, xr = x0.to(dev), x0.double()
    for i, t in enumerate(d.timesteps):
        extra = dict(variance_noise=noises[i].to(dev)) if ref.sde else {}
        x = d.step(0.3 * x + c.to(dev), t, x, **extra).prev_sample
        xr = ref.update(i, ref.order_of(i), xr, 0.3 * xr + c.double(), ref.m1, noises[i].double() if ref.sde else None)
        ref.m1, xr = xr[1], xr[0]
        assert d.step_index == i + 1
    backend.sync()
    assert torch.isfinite(x).all() and _rel(x, xr) <= 1e-5, _rel(x, xr)


def test_sde_step_draws_from_a_cpu_generator(backend):
    """No ``variance_noise``: the step draws ``torch.randn`` from the caller's (CPU) generator; the same draw injected gives the same step."""
    dev = backend.device
    shape = (1, 4, 4, 6)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(dev)
    e = torch.randn(shape, generator=torch.Generator().manual_seed(2)).to(dev)
    outs = []
    for inject in (False, True):
        d = DPMSolverMultistepScheduler.from_config(SD21, algorithm_type="sde-dpmsolver++")
        d.set_timesteps(10, device=dev)
        kw = dict(variance_noise=torch.randn(shape, generator=torch.Generator().manual_seed(7))) if inject else \
            dict(generator=torch.Generator().manual_seed(7))
        outs.append(d.step(e, d.timesteps[0], x, **kw)[0])
    backend.sync()
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# pipeline: literal loop vs the fp64 reference scheduler, fused vs literal
def _build(backend, cfg, seed=0):
    sd = synth_state_dict(cfg, seed=seed, random_affine=True)
    m = Stage2_InapintUNet2DConditionModel(**_kwargs(cfg))
    m.load_state_dict(sd)
    m.to(backend.device)
    return sd, m


def _call(pipe, inp, dev, N, steps, h, w, **kw):
    return pipe(height=h * 8, width=w * 8, masked_latents=inp["masked_latents"].to(dev),
                s_img_proj_f=inp["s_img_proj_f"].to(dev), st_pose_f=inp["st_pose_f"].to(dev),
                pred_t_img_embed=inp["pred_t_img_embed"].to(dev), latents=inp["latents"].to(dev),
                num_images_per_prompt=N, guidance_scale=kw.pop("guidance_scale", 2.0), num_inference_steps=steps, output_type="latent",
                **kw).latents


def _same_path(a, b):
    """tests/test_pipeline.py::_same_path standard for several steps."""
    return _rel(a, b) <= 1e-3


def _sizes(backend):
    # emulator: 3 steps (the middle one is second order), one image; GPU: 8 steps, two images
    return (1, 8, 8, 4, 3) if backend.is_emu else (2, 16, 24, 9, 8)


@pytest.mark.parametrize("karras", [False, True])
def test_pipeline_dpmpp_2m(backend, karras):
    cfg = UNetConfig.tiny()
    N, h, w, L, steps = _sizes(backend)
    sd, m = _build(backend, cfg, seed=4)
    inp = synth_inputs(cfg, h, w, N, L_img=L)
    ref = stage2_sample(sd, cfg, DPMRef(use_karras_sigmas=karras), num_images_per_prompt=N, guidance_scale=2.0,
                        num_inference_steps=steps, **inp)
    pipe = Stage2_InpaintDiffusionPipeline(m, DPMSolverMultistepScheduler.from_config(SD21, use_karras_sigmas=karras))
    lit = _call(pipe, inp, backend.device, N, steps, h, w, mode="reference")
    fused = _call(pipe, inp, backend.device, N, steps, h, w)                   # the default mode for DPM-Solver++
    backend.sync()
    assert pipe._st["dpm"] and pipe._st["noise"] is None
    assert torch.isfinite(lit).all() and _rel(lit, ref) <= 3e-2, _rel(lit, ref)
    assert _same_path(fused, lit), _rel(fused, lit)


def test_pipeline_dpmpp_2m_sde(backend):
    cfg = UNetConfig.tiny()
    N, h, w, L, steps = _sizes(backend)
    if backend.is_emu:
        steps = 2   # (CPU-suite budget: four sampling runs; the second-order update is covered by the ODE test above)
    sd, m = _build(backend, cfg, seed=6)
    inp = synth_inputs(cfg, h, w, N, L_img=L)
    pipe = Stage2_InpaintDiffusionPipeline(m, DPMSolverMultistepScheduler.from_config(SD21, algorithm_type="sde-dpmsolver++"))

    def run(seed, **kw):
        return _call(pipe, inp, backend.device, N, steps, h, w, generator=torch.Generator().manual_seed(seed), **kw)
    lit = run(3, mode="reference")
    fused = run(3)
    assert pipe._st["noise"] is not None and pipe._st["noise"].shape == (steps, N * 4 * h * w)
    again = run(3)
    other = run(4)
    backend.sync()
    assert torch.isfinite(fused).all() and _same_path(fused, lit), _rel(fused, lit)
    assert torch.equal(again, fused)
    assert _rel(other, fused) > 1e-2
    # the literal loop with these draws is the reference scheduler with the same noise
    g = torch.Generator().manual_seed(3)
    r = DPMRef(algorithm_type="sde-dpmsolver++")
    r.noises = [torch.randn((N, 4, h, w), generator=g) for _ in range(steps)]
    ref = stage2_sample(sd, cfg, r, num_images_per_prompt=N, guidance_scale=2.0, num_inference_steps=steps, **inp)
    assert _rel(lit, ref) <= 3e-2, _rel(lit, ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU only
@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["dpmsolver++", "sde-dpmsolver++"])
def test_fused_dpm_graph_replay_and_c_schedule(gpu_backend, algo):
    cfg = UNetConfig.tiny()
    dev = gpu_backend.device
    N, h, w, L, steps = 2, 16, 24, 9, 8
    sd, m = _build(gpu_backend, cfg, seed=7)
    inp = synth_inputs(cfg, h, w, N, L_img=L)
    outs = {}
    for c_sched in (False, True):
        pipe = Stage2_InpaintDiffusionPipeline(m, DPMSolverMultistepScheduler.from_config(SD21, algorithm_type=algo, use_karras_sigmas=True),
                                               c_schedule=c_sched)
        kw = lambda: dict(generator=torch.Generator().manual_seed(1))        # noqa: E731
        a = _call(pipe, inp, dev, N, steps, h, w, **kw())
        assert pipe._graph is not None
        b = _call(pipe, inp, dev, N, steps, h, w, **kw())
        torch.cuda.synchronize()
        assert torch.isfinite(a).all() and torch.equal(a, b)
        outs[c_sched] = a
        if not c_sched:   # guidance_rescale: guided eps first, then the step with cfg = 0
            gr_f = _call(pipe, inp, dev, N, steps, h, w, guidance_rescale=0.7, **kw())
            gr_l = _call(pipe, inp, dev, N, steps, h, w, guidance_rescale=0.7, mode="reference", **kw())
            assert _same_path(gr_f, gr_l) and _rel(gr_f, a) > 1e-4
    assert _same_path(outs[True], outs[False]), _rel(outs[True], outs[False])


@pytest.mark.gpu
def test_full_size_dpmpp_2m_karras_config1(gpu_backend):
    """configs[1] shape (4 images of 352 x 512, latent 64 x 88, CFG => UNet batch 8), synthetic full-size weights, DPM++ 2M Karras, 20 steps:
    finite, deterministic, fused within 1e-3 of the literal loop."""
    dev = gpu_backend.device
    cfg = UNetConfig()
    sd = synth_state_dict(cfg, seed=0)
    N, h, w, steps = 4, 64, 88, 20
    inp = synth_inputs(cfg, h, w, N)
    m = Stage2_InapintUNet2DConditionModel(**_kwargs(cfg))
    m.load_state_dict(sd)
    m.to(dev)
    pipe = Stage2_InpaintDiffusionPipeline(m, DPMSolverMultistepScheduler.from_config(SD21, use_karras_sigmas=True))
    a = _call(pipe, inp, dev, N, steps, h, w)
    b = _call(pipe, inp, dev, N, steps, h, w)
    lit = _call(pipe, inp, dev, N, steps, h, w, mode="reference")
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert _same_path(a, lit), _rel(a, lit)
