"""Euler, Euler-ancestral, LMS and PNDM (PLMS) sampling: the four scheduler classes of ``pcdms_amd.schedulers``, the ``pcdm_multistep_step``
kernel, the scaled input assembly (``pcdm_assemble_input_ex``), float32 timesteps down to the time embedding, and the fused (graph-captured)
pipeline path.

Yardstick: ``SigmaRef`` and ``PNDMRef`` below, float64 restatements of the four diffusers 0.24 schedulers written here and sharing no code
with the classes under test (LMS integrates with Gauss-Legendre quadrature, PNDM keeps the literal ``ets`` list).  Sigmas are kept as fp32
tables, as diffusers keeps them; everything after that is float64.  Parity is against THIS restatement: upstream parity is unpinned
(tools/compare_with_diffusers.py checks it where diffusers is installed).  The point-mass tests anchor the restatement itself on the exact
solution of the probability-flow ODE, which rests on nobody's memory of diffusers.

Measured worst errors: profiles/karras_sampler_values.json (``python -m tests.test_karras_samplers`` refreshes it from a run's scratch file)."""
from __future__ import annotations

import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle.pipeline import stage2_sample, synth_inputs
from oracle.unet import UNetConfig, synth_state_dict
from pcdms_amd import ops
from pcdms_amd.pipeline import Stage2_InpaintDiffusionPipeline
from pcdms_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler,
                                  LMSDiscreteScheduler, PNDMScheduler, UniPCMultistepScheduler)
from pcdms_amd.unet import Stage2_InapintUNet2DConditionModel
from tests import parity_record
from tests.test_schedulers import SD21
from tests.test_unet import _kwargs

ROOT = Path(__file__).resolve().parent.parent
VALUES_OUT = parity_record.OUT.parent / "karras_sampler_values.json"   # the scratch directory of a test run (tests/parity_record.py)
CLASSES = dict(euler=EulerDiscreteScheduler, euler_a=EulerAncestralDiscreteScheduler, lms=LMSDiscreteScheduler, pndm=PNDMScheduler)
CX, CS, C0, C1, C2, C3, CZ, IN_SCALE, SAVE, PUSH = range(10)       # row layout of include/pcdm.h (PCDM_MS_*), restated


@pytest.fixture(autouse=True)
def _modes_compared_on_identical_launches(monkeypatch):
    """As in tests/test_dpmsolver.py: fused and literal loop are compared on identical UNet launches (no CFG-shared prefix)."""
    import pcdms_amd.unet as U
    monkeypatch.setattr(U, "SHARE_CFG_PREFIX", False)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


def _record(name: str, value: float, tol: float) -> None:
    """The measured value goes to the run's scratch files (the shared parity record and this file's own) and is held to ``tol``."""
    try:
        VALUES_OUT.parent.mkdir(exist_ok=True)
        try:
            cur = json.loads(VALUES_OUT.read_text())
        except (OSError, ValueError):
            cur = {}
        cur[name] = max(float(value), float(cur.get(name, 0.0)))
        VALUES_OUT.write_text(json.dumps(cur, indent=1, sort_keys=True))
    except OSError:
        pass
    print(f"{name}: {float(value):.4g} (bound {tol:.4g})")
    parity_record.check(f"karras_samplers/{name}", value, tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 restatements
def _sd21_alphas_cumprod() -> np.ndarray:
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).numpy()                            # fp32, as diffusers


class SigmaRef:
    """float64 Euler (s_churn = 0) / Euler-ancestral / LMS (order 4) in sigma space on the SD-2.1 training table.  ``update`` is one step on
    explicit state; ``step`` / ``scale_model_input`` give the stateful interface ``oracle.pipeline.stage2_sample`` drives."""

    order = 1

    def __init__(self, kind="euler", spacing="linspace", karras=False, steps_offset=1):
        assert kind in ("euler", "euler_a", "lms")
        self.kind, self.spacing, self.karras, self.steps_offset = kind, spacing, karras, steps_offset
        self.ac = _sd21_alphas_cumprod()
        self.noises = None                                                       # optional per-step noise tensors (euler_a)

    def set_timesteps(self, n, device=None):
        sig = ((1 - self.ac) / self.ac) ** 0.5                                   # fp32, increasing with t
        if self.spacing == "linspace":
            ts = np.linspace(0, 999, n, dtype=np.float32)[::-1].copy()
        elif self.spacing == "leading":
            ts = (np.arange(n) * (1000 // n)).round()[::-1].astype(np.float32) + self.steps_offset
        else:
            ts = np.arange(1000, 0, -1000 / n).round().astype(np.float32) - 1
        s = np.interp(ts, np.arange(1000), sig)
        if self.karras:
            lo, hi = float(s[-1]), float(s[0])
            s = (hi ** (1 / 7) + np.linspace(0, 1, n) * (lo ** (1 / 7) - hi ** (1 / 7))) ** 7
            ts = np.interp(np.log(s), np.log(sig.astype(np.float64)), np.arange(1000)).astype(np.float32)   # fractional, not rounded
        self.sigmas = np.concatenate([s, [0.0]]).astype(np.float32)
        self.timesteps = torch.from_numpy(ts.copy())
        self.n, self.i, self.hist = n, 0, []

    @property
    def init_noise_sigma(self):
        smax = float(self.sigmas.max())
        return smax if self.spacing in ("linspace", "trailing") else math.sqrt(smax ** 2 + 1)

    def in_scale(self, i):
        return 1.0 / math.sqrt(float(self.sigmas[i]) ** 2 + 1.0)

    def scale_model_input(self, x, t=None):
        return (x.double() * self.in_scale(self.i)).to(x.dtype)

    def lms_coefficients(self, i, order):
        """Gauss-Legendre (4 nodes: exact to degree 7) integral of each Lagrange basis polynomial over [sigma_i, sigma_{i+1}]."""
        s = self.sigmas.astype(np.float64)
        nodes, weights = np.polynomial.legendre.leggauss(4)
        a, b = s[i], s[i + 1]
        tau = 0.5 * (b - a) * nodes + 0.5 * (b + a)
        out = []
        for k in range(order):
            f = np.ones_like(tau)
            for j in range(order):
                if j != k:
                    f = f * (tau - s[i - j]) / (s[i - k] - s[i - j])
            out.append(0.5 * (b - a) * float(np.sum(weights * f)))
        return out

    def update(self, i, x, e, xs=None, hist=(), z=None):
        """x' of step i in float64; ``hist`` = older eps, newest first."""
        s0, s1 = float(self.sigmas[i]), float(self.sigmas[i + 1])
        if self.kind == "euler":
            return x + (s1 - s0) * e
        if self.kind == "euler_a":
            up = math.sqrt(s1 ** 2 * (s0 ** 2 - s1 ** 2) / s0 ** 2)
            down = math.sqrt(s1 ** 2 - up ** 2)
            return x + (down - s0) * e + (up * z if z is not None else 0.0)
        order = min(i + 1, 4)
        ds = [e] + list(hist)
        return x + sum(c * d for c, d in zip(self.lms_coefficients(i, order), ds[:order]))

    def step(self, eps, t, x, variance_noise=None):
        i = self.i
        z = None
        if self.kind == "euler_a":
            z = (variance_noise if variance_noise is not None else self.noises[i]).double().cpu()
        e = eps.double().cpu()
        xn = self.update(i, x.double().cpu(), e, None, self.hist, z)
        self.hist = ([e] + self.hist)[:3]
        self.i = i + 1
        return xn.to(x.dtype)


class PNDMRef:
    """float64 PLMS (``PNDMScheduler`` with ``skip_prk_steps=True``, leading spacing, SD-2.1 table), the literal bookkeeping: an ``ets`` list,
    the saved ``cur_sample`` and a call counter."""

    order = 1
    init_noise_sigma = 1.0
    kind = "pndm"

    def __init__(self, steps_offset=1, set_alpha_to_one=False):
        self.ac = _sd21_alphas_cumprod().astype(np.float64)
        self.steps_offset = steps_offset
        self.final = 1.0 if set_alpha_to_one else float(self.ac[0])

    def set_timesteps(self, n, device=None):
        self.ratio = 1000 // n
        t = np.arange(n) * self.ratio + self.steps_offset
        ts = np.concatenate([t[:-1], t[-2:-1], t[-1:]])[::-1].astype(np.int64)
        self.timesteps = torch.from_numpy(ts.copy())
        self.n, self.counter, self.ets, self.cur_sample = n, 0, [], None

    def scale_model_input(self, x, t=None):
        return x

    def in_scale(self, i):
        return 1.0

    def prev_sample(self, x, t, tp, e):
        a_t = self.ac[t]
        a_p = self.ac[tp] if tp >= 0 else self.final
        den = a_t * math.sqrt(1 - a_p) + math.sqrt(a_t * (1 - a_t) * a_p)
        return math.sqrt(a_p / a_t) * x - (a_p - a_t) * e / den

    def step(self, eps, t, x, variance_noise=None):
        t = int(t)
        e, xd = eps.double().cpu(), x.double().cpu()
        tp = t - self.ratio
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(e)
        else:
            tp, t = t, t + self.ratio
        if len(self.ets) == 1 and self.counter == 0:
            self.cur_sample = xd
        elif len(self.ets) == 1 and self.counter == 1:
            e = (e + self.ets[-1]) / 2
            xd, self.cur_sample = self.cur_sample, None
        elif len(self.ets) == 2:
            e = (3 * self.ets[-1] - self.ets[-2]) / 2
        elif len(self.ets) == 3:
            e = (23 * self.ets[-1] - 16 * self.ets[-2] + 5 * self.ets[-3]) / 12
        else:
            e = (55 * self.ets[-1] - 59 * self.ets[-2] + 37 * self.ets[-3] - 9 * self.ets[-4]) / 24
        self.counter += 1
        return self.prev_sample(xd, t, tp, e).to(x.dtype)

    def update(self, i, x, e, xs=None, hist=(), z=None):
        """Call i on explicit state: ``xs`` the saved sample, ``hist`` the eps pushed so far (newest first)."""
        pushed = 0 if i == 0 else 1 if i <= 2 else min(i - 1, 3)                  # entries of ets in front of call i (after its [-3:] cut)
        self.counter, self.cur_sample = i, xs
        self.ets = [h for h in reversed(list(hist)[:pushed])]
        return self.step(e, self.timesteps[i], x)


def _ref(kind, **kw):
    return PNDMRef(**kw) if kind == "pndm" else SigmaRef(kind, **kw)


def _apply_row(row, x, xs, e, h, z):
    """Row of the coefficient table applied in float64 (the update include/pcdm.h states)."""
    c = row.double()
    return c[CX] * x + c[CS] * xs + c[C0] * e + c[C1] * h[0] + c[C2] * h[1] + c[C3] * h[2] + c[CZ] * z


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU, no library: schedules, tables, anchors, configuration
def test_known_answers_sd21():
    p = PNDMScheduler.from_config(SD21)
    for n, want in ((5, [801, 601, 601, 401, 201, 1]), (2, [501, 1, 1]), (1, [1])):
        p.set_timesteps(n)
        assert p.timesteps.dtype == torch.int64 and p.timesteps.tolist() == want
    assert p.init_noise_sigma == 1 and p.order == 1
    e = EulerDiscreteScheduler.from_config(SD21, timestep_spacing="linspace")
    e.set_timesteps(5)
    assert e.timesteps.dtype == torch.float32 and e.timesteps.tolist() == [999, 749.25, 499.5, 249.75, 0]
    assert e.sigmas.dtype == np.float32 and len(e.sigmas) == 6 and e.sigmas[-1] == 0
    smax = 14.614647                                                             # sigma of the last SD-2.1 training step (tests/test_dpmsolver.py)
    assert e.init_noise_sigma == pytest.approx(smax, rel=1e-6)
    for cls in (EulerAncestralDiscreteScheduler, LMSDiscreteScheduler):
        s = cls.from_config(SD21, timestep_spacing="linspace")
        s.set_timesteps(5)
        assert s.timesteps.tolist() == e.timesteps.tolist() and np.array_equal(s.sigmas, e.sigmas) and s.order == 1
    t = EulerDiscreteScheduler.from_config(SD21, timestep_spacing="trailing")
    t.set_timesteps(5)
    assert t.timesteps.tolist() == [999, 799, 599, 399, 199] and t.init_noise_sigma == pytest.approx(smax, rel=1e-6)
    ld = EulerDiscreteScheduler.from_config(SD21, timestep_spacing="leading")
    ld.set_timesteps(5)
    assert ld.timesteps.tolist() == [801, 601, 401, 201, 1] and ld.sigmas[-1] == 0
    assert ld.init_noise_sigma == pytest.approx(math.sqrt(float(ld.sigmas[0]) ** 2 + 1), rel=1e-7) and ld.init_noise_sigma < smax
    k = EulerDiscreteScheduler.from_config(SD21, use_karras_sigmas=True)
    k.set_timesteps(10)
    r = np.asarray(k.sigmas[:-1], dtype=np.float64) ** (1 / 7)
    assert np.allclose(np.diff(r), (r[-1] - r[0]) / 9, rtol=0, atol=1e-6) and k.sigmas[-1] == 0      # rho = 7 spacing, then 0
    assert k.timesteps.dtype == torch.float32 and float(k.timesteps[0]) == 999 and float(k.timesteps[-1]) == 0
    assert any(float(v) != round(float(v)) for v in k.timesteps)                 # not rounded


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 20, 50])
@pytest.mark.parametrize("case", ["euler-linspace", "euler-leading", "euler-trailing", "euler-linspace-karras", "euler-leading-karras",
                                  "euler-trailing-karras", "euler_a-linspace", "euler_a-leading", "euler_a-trailing", "lms-linspace",
                                  "lms-leading", "lms-trailing", "lms-linspace-karras", "pndm-leading"])
def test_coefficient_table_vs_reference(case, n):
    """Row i of the table, applied in float64 to random (x, xs, eps, history, z), equals the restatement's step i; the bound is that of
    tests/test_dpmsolver.py::test_coefficient_table_vs_reference (fp32 storage of float64 coefficients)."""
    kind, spacing, *rest = case.split("-")
    karras = bool(rest)
    kw = dict(timestep_spacing=spacing)
    if karras:
        kw["use_karras_sigmas"] = True
    d = CLASSES[kind].from_config(SD21, **kw)
    d.set_timesteps(n)
    ref = _ref(kind) if kind == "pndm" else _ref(kind, spacing=spacing, karras=karras)
    ref.set_timesteps(n)
    m = n + 1 if (kind == "pndm" and n > 1) else n
    assert len(d.timesteps) == m == len(ref.timesteps)
    if kind == "pndm":
        assert d.timesteps.tolist() == ref.timesteps.tolist()
    else:
        assert d.timesteps.dtype == torch.float32 and np.allclose(d.timesteps.numpy(), ref.timesteps.numpy(), rtol=1e-6, atol=1e-4)
        assert np.allclose(d.sigmas, ref.sigmas, rtol=1e-6) and d.init_noise_sigma == pytest.approx(ref.init_noise_sigma, rel=1e-6)
    tab = d.coefficient_table()
    assert tab.shape == (m, 12) and tab.dtype == torch.float32 and torch.isfinite(tab).all() and (tab[:, 10:] == 0).all()
    g = torch.Generator().manual_seed(n)
    worst = 0.0
    for i in range(m):
        x, xs, e, h1, h2, h3, z = (torch.randn(64, generator=g, dtype=torch.float64) for _ in range(7))
        got = _apply_row(tab[i], x, xs, e, (h1, h2, h3), z)
        want = ref.update(i, x, e, xs, (h1, h2, h3), z)
        worst = max(worst, _rel(got, want))
        assert _rel(got, want) <= 1e-6, (i, _rel(got, want))
        assert float(tab[i, IN_SCALE]) == pytest.approx(ref.in_scale(i), rel=1e-6)
        if kind == "pndm":
            assert bool(tab[i, SAVE]) == (i == 0) and bool(tab[i, PUSH]) == (i != 1) and tab[i, CZ] == 0
        else:
            assert tab[i, SAVE] == 0 and tab[i, CS] == 0 and tab[i, CX] == 1 and bool(tab[i, PUSH]) == (kind == "lms")
            assert (tab[i, CZ] != 0) == (kind == "euler_a" and i < m - 1)
    _record(f"table/{case}", worst, 1e-6)


@pytest.mark.parametrize("karras", [False, True])
def test_lms_coefficients_closed_form_vs_gauss_legendre(karras):
    from pcdms_amd.schedulers import _lms_coefficients
    d = LMSDiscreteScheduler.from_config(SD21, use_karras_sigmas=karras)
    ref = SigmaRef("lms", karras=karras)
    worst = 0.0
    for n in (2, 3, 4, 5, 20, 50):
        d.set_timesteps(n)
        ref.set_timesteps(n)
        for i in range(n):
            for order in range(1, min(i + 1, 4) + 1):
                got, want = np.array(_lms_coefficients(ref.sigmas, i, order)), np.array(ref.lms_coefficients(i, order))
                worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
                # the basis polynomials sum to 1: the coefficients sum to the length of the interval
                assert sum(got) == pytest.approx(float(ref.sigmas[i + 1]) - float(ref.sigmas[i]), rel=1e-10)
        assert d.coefficient_table()[0, C0] == pytest.approx(float(d.sigmas[1]) - float(d.sigmas[0]), rel=1e-6)    # order 1 = Euler
    assert worst <= 1e-10, worst                                                 # both are exact up to float64 rounding


def _point_mass_run(kind, n, stepper):
    """Drive ``stepper(i, t, x, eps) -> x'`` along the exact eps of a point mass at x0; returns (final x, expected final x)."""
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(32, generator=g, dtype=torch.float64)
    ref = _ref(kind)
    ref.set_timesteps(n)
    x = 3.0 * torch.randn(32, generator=g, dtype=torch.float64) * ref.init_noise_sigma        # any start
    ac = _sd21_alphas_cumprod().astype(np.float64)
    c = None
    for i, t in enumerate(ref.timesteps.tolist()):
        if kind == "pndm":
            a = ac[int(t)]
            eps = (x - math.sqrt(a) * x0) / math.sqrt(1 - a)
            c = eps if c is None else c
        else:
            eps = (x - x0) / float(ref.sigmas[i])
        x = stepper(ref, i, t, x, eps)
    if kind == "pndm":
        a_f = ac[0]                                                               # final_alpha_cumprod (set_alpha_to_one=False)
        return x, math.sqrt(a_f) * x0 + math.sqrt(1 - a_f) * c
    return x, x0


@pytest.mark.parametrize("n", [1, 2, 3, 5, 20])
@pytest.mark.parametrize("kind", ["euler", "euler_a", "lms", "pndm"])
def test_point_mass_anchor(kind, n):
    """eps* of a point-mass data distribution is constant along the exact trajectory, so every consistent linear multistep method is exact
    on it: Euler, LMS and Euler-ancestral with zero noise land on x0 at sigma = 0, PLMS on sqrt(a_f) x0 + sqrt(1 - a_f) eps*."""
    zero = torch.zeros(32, dtype=torch.float64)
    got, want = _point_mass_run(kind, n, lambda ref, i, t, x, e: ref.step(e, t, x, variance_noise=zero))
    assert _rel(got, want) <= 1e-12, _rel(got, want)                             # the restatement: float64 rounding
    d = CLASSES[kind].from_config(SD21, **({} if kind == "pndm" else dict(timestep_spacing="linspace")))
    d.set_timesteps(n)
    tab = d.coefficient_table()
    state = dict(xs=zero, h=[zero, zero, zero])

    def table_step(ref, i, t, x, e):
        row = tab[i]
        xn = _apply_row(row, x, state["xs"], e, state["h"], zero)
        if row[SAVE] != 0:
            state["xs"] = x
        if row[PUSH] != 0:
            state["h"] = [e] + state["h"][:2]
        return xn
    got, want = _point_mass_run(kind, n, table_step)
    _record(f"point_mass/{kind}/n{n}", _rel(got, want), 1e-5)


@pytest.mark.parametrize("cls,bad", [
    (EulerDiscreteScheduler, dict(prediction_type="v_prediction")), (EulerDiscreteScheduler, dict(interpolation_type="log_linear")),
    (EulerDiscreteScheduler, dict(timestep_spacing="karras")), (EulerDiscreteScheduler, dict(timestep_type="continuous")),
    (EulerAncestralDiscreteScheduler, dict(prediction_type="sample")), (EulerAncestralDiscreteScheduler, dict(timestep_spacing="x")),
    (LMSDiscreteScheduler, dict(prediction_type="v_prediction")), (LMSDiscreteScheduler, dict(timestep_spacing="x")),
    (PNDMScheduler, dict(skip_prk_steps=False)), (PNDMScheduler, dict(prediction_type="v_prediction")), (PNDMScheduler, dict(timestep_spacing="x"))])
def test_unsupported_configs_are_refused(cls, bad):
    with pytest.raises(NotImplementedError):
        cls.from_config(SD21, **bad)


def test_config_round_trips_and_step_signatures():
    import inspect
    every = (DDIMScheduler, UniPCMultistepScheduler, DPMSolverMultistepScheduler, *CLASSES.values())
    for a in every:
        for b in every:
            sb = b.from_config(a.from_config(SD21).config)
            assert sb.config.beta_schedule == "scaled_linear" and sb.config.beta_end == 0.012 and sb.config.steps_offset == 1
            assert sb.config.skip_prk_steps is True
            sa = a.from_config(sb.config)
            assert type(sa) is a and sa.config.num_train_timesteps == 1000
    assert EulerDiscreteScheduler().config.timestep_spacing == "linspace" and PNDMScheduler().config.timestep_spacing == "leading"
    assert LMSDiscreteScheduler().config.beta_schedule == "linear" and EulerAncestralDiscreteScheduler().config.steps_offset == 0
    params = {k: set(inspect.signature(c.step).parameters) for k, c in CLASSES.items()}
    assert "generator" in params["euler_a"] and "generator" in params["euler"] and "s_churn" in params["euler"] and "order" in params["lms"]
    assert all("eta" not in p and "return_dict" in p for p in params.values()) and "generator" not in params["pndm"]
    import pcdms_amd
    assert all(getattr(pcdms_amd, c.__name__) is c for c in CLASSES.values())


def test_pipeline_from_pretrained_resolves_pndm(tmp_path):
    from safetensors.torch import save_file

    from tests.test_from_pretrained import SD21_UNET_JSON
    root = tmp_path / "sd21"
    for sub in ("unet", "scheduler"):
        (root / sub).mkdir(parents=True)
    (root / "unet" / "config.json").write_text(json.dumps(SD21_UNET_JSON))
    stock = UNetConfig.tiny(in_channels=4, class_embed_type=None, projection_class_embeddings_input_dim=None)
    save_file({k: v.contiguous() for k, v in synth_state_dict(stock, seed=1).items()}, str(root / "unet" / "diffusion_pytorch_model.safetensors"))
    (root / "scheduler" / "scheduler_config.json").write_text(json.dumps({
        "_class_name": "PNDMScheduler", "_diffusers_version": "0.8.0", "beta_end": 0.012, "beta_schedule": "scaled_linear",
        "beta_start": 0.00085, "clip_sample": False, "num_train_timesteps": 1000, "prediction_type": "epsilon", "set_alpha_to_one": False,
        "skip_prk_steps": True, "steps_offset": 1, "trained_betas": None}))
    pipe = Stage2_InpaintDiffusionPipeline.from_pretrained(root)
    assert type(pipe.scheduler) is PNDMScheduler and pipe.scheduler.config.steps_offset == 1
    pipe.scheduler.set_timesteps(5)
    assert pipe.scheduler.timesteps.tolist() == [801, 601, 601, 401, 201, 1]
    u = UniPCMultistepScheduler.from_config(pipe.scheduler.config)
    assert u.config.beta_schedule == "scaled_linear" and u.config.steps_offset == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels: lane emulator in the CPU suite, MI355X under -m gpu
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4 * 16 * 24 + 3])
def test_multistep_step_kernel(backend, n, cfg):
    """Random rows with every slot non-zero; each save / push combination, noise table NULL and given, step counter NULL and given.  Result
    and the five state slots vs float64 of the fp32 inputs; in place; a second identical call is bit-identical.

    Conditioning: a relative bound on a seven-term fp32 sum means something only where the terms do not cancel, and at n = 1 there is no
    vector norm to average a cancelling element away.  So magnitudes are random in [0.25, 1.25) and the sign of each coefficient column is
    flipped TOGETHER with the sign of its operand: the kernel sees mixed signs, every product of a row's sum is positive, and 1e-6 asks the
    same of one element as of 1539 (seven fused roundings and the CFG combine are at most ~10 ulp = 6e-7 of such a sum)."""
    from pcdms_amd import _lib
    dev = backend.device
    g = torch.Generator().manual_seed(1000 + n)
    rows = 5

    def mag(*shape):
        return (0.25 + torch.rand(*shape, generator=g)).float()
    sign = torch.where(torch.rand(7, generator=g) < 0.5, -1.0, 1.0)           # per operand: x, xs, eps, h1, h2, h3, noise
    coef = mag(rows, 12)
    coef[:, :7] *= sign
    coef[:, 10:] = 0
    f = [mag(n) * sign[k] for k in (0, 1, 3, 4, 5)]                              # x, xs, h1, h2, h3
    eps = mag(n)
    if cfg:
        eps = torch.cat([eps, eps + mag(n)])                                     # (cond - uncond > 0: the guided eps does not cancel either)
    eps = eps * sign[2]
    noise = mag(rows, n) * sign[6]
    gs = 3.5
    e = (eps[:n].double() + gs * (eps[n:].double() - eps[:n].double())) if cfg else eps.double()
    worst = 0.0
    for save in (0.0, 1.0):
        for push in (0.0, 2.0):
            for with_noise in (False, True):
                for st in (None, 3):
                    c = coef.clone()
                    c[:, SAVE], c[:, PUSH] = save, push
                    r = c[0 if st is None else st].double()
                    x, xs, h1, h2, h3 = (t.double() for t in f)
                    z = noise[0 if st is None else st].double() if with_noise else torch.zeros(n, dtype=torch.float64)
                    want = [r[CX] * x + r[CS] * xs + r[C0] * e + r[C1] * h1 + r[C2] * h2 + r[C3] * h3 + r[CZ] * z,
                            x if save else xs, e if push else h1, h1 if push else h2, h2 if push else h3]
                    outs = []
                    for _ in range(2):
                        state = [t.clone().to(dev) for t in f]
                        step = None if st is None else torch.tensor([st], dtype=torch.int32, device=dev)
                        err = torch.zeros(1, dtype=torch.int32, device=dev)
                        ops.multistep_step(eps.to(dev), cfg, gs, *state, noise.to(dev) if with_noise else None, c.to(dev), step, err)
                        backend.sync()
                        assert int(err.item()) == 0
                        outs.append(state)
                    for a, b, w in zip(outs[0], outs[1], want):
                        assert torch.equal(a, b)
                        worst = max(worst, _rel(a, w))
                        assert _rel(a, w) <= 1e-6, (save, push, with_noise, st, _rel(a, w))
    _record(f"multistep_step/{backend.name}/n{n}/cfg{int(cfg)}", worst, 1e-6)
    # a step counter outside the table is clamped to the nearest row and reported; refusals launch nothing
    state = [t.clone().to(dev) for t in f]
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.multistep_step(eps.to(dev), cfg, gs, *state, None, coef.to(dev), torch.tensor([rows + 7], dtype=torch.int32, device=dev), err)
    backend.sync()
    last = [t.clone().to(dev) for t in f]
    ops.multistep_step(eps.to(dev), cfg, gs, *last, None, coef.to(dev), torch.tensor([rows - 1], dtype=torch.int32, device=dev))
    backend.sync()
    assert int(err.item()) == 1 and all(torch.equal(a, b) for a, b in zip(state, last))
    L, p = _lib.lib(), [t.data_ptr() for t in state]
    cd, ed = coef.to(dev), eps.to(dev)
    before = [t.clone() for t in state]
    assert L.pcdm_multistep_step(None, 0, 1.0, *p, None, cd.data_ptr(), rows, None, None, n, None) == -1
    assert L.pcdm_multistep_step(ed.data_ptr(), 0, 1.0, *p, None, None, rows, None, None, n, None) == -1
    assert L.pcdm_multistep_step(ed.data_ptr(), 0, 1.0, p[0], None, *p[2:], None, cd.data_ptr(), rows, None, None, n, None) == -1
    assert L.pcdm_multistep_step(ed.data_ptr(), 0, 1.0, *p, None, cd.data_ptr(), rows, None, None, 0, None) == -1
    assert L.pcdm_multistep_step(ed.data_ptr(), 0, 1.0, *p, None, cd.data_ptr(), 0, None, None, n, None) == -1
    backend.sync()
    assert all(torch.equal(a, b) for a, b in zip(state, before))


@pytest.mark.parametrize("with_mask", [True, False])
def test_assemble_input_scaled(backend, with_mask):
    dev = backend.device
    N, h, w = (2, 4, 6) if backend.is_emu else (3, 16, 24)
    g = torch.Generator().manual_seed(90)
    lat = torch.randn(N, 4, h, w, generator=g) * 9
    mask = torch.cat([torch.ones(1, 1, h, w // 2), torch.zeros(1, 1, h, w // 2)], 3) if with_mask else None
    masked = torch.randn(2 * N, 4, h, w, generator=g)
    tab = torch.rand(4, 12, generator=g) + 0.05
    plain = torch.empty(2 * N, h, w, 64, dtype=ops.BF16, device=dev)
    md = None if mask is None else mask.to(dev)
    ops.assemble_input(lat.to(dev), 2, md, masked.to(dev), plain)
    same = torch.full_like(plain, 7.0)
    ops.assemble_input_ex(lat.to(dev), 2, md, masked.to(dev), same)            # no scale pointer
    backend.sync()
    assert torch.equal(same.view(torch.int16), plain.view(torch.int16))
    nl = 9 if with_mask else 8
    for st in (None, 2):
        out = torch.full_like(plain, 7.0)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        step = None if st is None else torch.tensor([st], dtype=torch.int32, device=dev)
        ops.assemble_input_ex(lat.to(dev), 2, md, masked.to(dev), out, tab.to(dev), 7, step, err)
        backend.sync()
        scale = tab[0 if st is None else st, 7]                                   # fp32 scalar: fp32 multiply, one rounding to bf16
        want = (torch.cat([lat] * 2) * scale).to(ops.BF16).permute(0, 2, 3, 1)
        assert torch.equal(out[..., :4].cpu().view(torch.int16), want.contiguous().view(torch.int16))
        assert torch.equal(out[..., 4:].cpu().view(torch.int16), plain[..., 4:].cpu().view(torch.int16))    # mask, masked latents, zero padding
        assert (out[..., nl:] == 0).all() and int(err.item()) == 0
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    clamped = torch.empty_like(plain)
    ops.assemble_input_ex(lat.to(dev), 2, md, masked.to(dev), clamped, tab.to(dev), 7, torch.tensor([-3], dtype=torch.int32, device=dev), err)
    first = torch.empty_like(plain)
    ops.assemble_input_ex(lat.to(dev), 2, md, masked.to(dev), first, tab.to(dev), 7, None, None)
    backend.sync()
    assert int(err.item()) == 1 and torch.equal(clamped.view(torch.int16), first.view(torch.int16))


@pytest.mark.parametrize("dim", (64, 320))
def test_float_timestep_embedding(backend, dim):
    """Integer-valued float timesteps give the bits of the int64 entry points; fractional ones meet the bound that
    tests/test_small_ops_conformance.py::test_timestep_embedding derives for the int64 kernel, against float64."""
    from tests.test_small_ops_conformance import timestep_ref
    dev, B = backend.device, 3
    ints = torch.tensor([0, 1, 500, 981, 999], dtype=torch.int64)
    fracs = torch.tensor([749.25, 499.5, 0.75, 998.99, 123.456, 249.75], dtype=torch.float32)
    worst = 0.0
    for flip in (False, True):
        for shift in (0.0, 1.0):
            a = ops.timestep_embedding_rows(ints.to(dev), torch.empty(5, dim, device=dev), flip, shift)
            b = ops.timestep_embedding_rows(ints.float().to(dev), torch.empty(5, dim, device=dev), flip, shift)
            backend.sync()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            for i in (None, 3):
                step = None if i is None else torch.tensor([i], dtype=torch.int32, device=dev)
                a1 = ops.timestep_embedding(ints.to(dev), step, torch.empty(B, dim, device=dev), flip, shift)
                b1 = ops.timestep_embedding(ints.float().to(dev), step, torch.empty(B, dim, device=dev), flip, shift)
                backend.sync()
                assert torch.equal(a1.view(torch.int32), b1.view(torch.int32)) and torch.equal(b1[0], b[0 if i is None else i])
            ref, bound = timestep_ref(fracs.double().tolist(), dim, flip, shift)
            rows = ops.timestep_embedding_rows(fracs.to(dev), torch.empty(len(fracs), dim, device=dev), flip, shift)
            one = ops.timestep_embedding(fracs.to(dev), torch.tensor([4], dtype=torch.int32, device=dev), torch.empty(B, dim, device=dev), flip, shift)
            backend.sync()
            ratio = ((rows.double().cpu() - ref).abs() / bound).max().item()
            worst = max(worst, ratio)
            assert ratio <= 1.0, (flip, shift, ratio)
            assert all(torch.equal(one[k], rows[4]) for k in range(B))
    _record(f"float_timestep_embedding/{backend.name}/dim{dim}", worst, 1.0)


def _build(backend, cfg, seed=0):
    sd = synth_state_dict(cfg, seed=seed, random_affine=True)
    m = Stage2_InapintUNet2DConditionModel(**_kwargs(cfg))
    m.load_state_dict(sd)
    m.to(backend.device)
    return sd, m


def test_float_timesteps_through_the_unet(backend):
    """The Python schedule's time table and per-step embedding, and the C context's table, with an integer-valued float32 timestep table:
    the bits of the int64 table.  A Python float passed to ``unet(...)`` is no longer truncated."""
    from pcdms_amd.unet_ctx import UNetContext
    cfg = UNetConfig.tiny()
    dev = backend.device
    B, h, w, L = 2, 8, 8, 5
    _, m = _build(backend, cfg, seed=3)
    g = torch.Generator().manual_seed(0)
    s = torch.randn(B, cfg.in_channels, h, w, generator=g)
    e = torch.randn(B, L, cfg.cross_attention_dim, generator=g)
    c = torch.randn(B, 1, cfg.projection_class_embeddings_input_dim, generator=g) * 0.4
    p = torch.randn(1, cfg.block_out_channels[0], h, w, generator=g) * 0.1
    ti = torch.tensor([981, 417, 1], dtype=torch.int64, device=dev)
    tf = ti.float()
    step = torch.tensor([1], dtype=torch.int32, device=dev)
    m.prepare_conditioning(B, h, w, e.to(dev), c.to(dev), p.to(dev), zero_ctx_batches=0)      # (packs the weights)
    x_in = ops.nchw_to_nhwc_bf16(s.to(dev), cpad=m._w["conv_in"].cin)
    outs = {}
    for name, ts in (("i", ti), ("f", tf)):
        cond = m.prepare_conditioning(B, h, w, e.to(dev), c.to(dev), p.to(dev), zero_ctx_batches=0, timesteps=ts)
        assert cond.temb_steps.dtype == ts.dtype and cond.temb_steps.data_ptr() == ts.data_ptr()
        outs[name, "table"] = cond.temb_all.clone()
        outs[name, "py"] = m._forward_nhwc(x_in, B, h, w, ts, cond, step_dev=step).clone()
        backend.sync()
    assert torch.equal(outs["i", "table"], outs["f", "table"]) and torch.equal(outs["i", "py"], outs["f", "py"])
    # the C context on the float table: the bits of the Python schedule on the int64 table (which the C schedule on int64 equals:
    # tests/test_unet_ctx.py)
    ctx = UNetContext(m)
    pose_b = ctx.prepare_conditioning(B, h, w, e, c, p, zero_ctx_batches=0)
    ctx.prepare_timesteps(tf, B, h, w)
    out_c = ctx.forward(x_in, tf, step, B, h, w, pose_b)
    backend.sync()
    assert torch.equal(out_c, outs["i", "py"])
    # scalars at the public boundary: 417.0 is 417, 417.5 is not truncated to it
    kw = dict(encoder_hidden_states=e.to(dev), class_labels=c.to(dev), my_pose_cond=p.to(dev), return_dict=False)
    b = m(s.to(dev), 417.0, **kw)[0]
    d = m(s.to(dev), 417.5, **kw)[0]
    backend.sync()
    assert torch.equal(b, outs["i", "py"]) and torch.isfinite(d).all() and not torch.equal(b, d)


@pytest.mark.parametrize("n", [5, 20])
@pytest.mark.parametrize("kind", ["euler", "euler_a", "lms", "pndm"])
def test_step_trajectory_vs_reference(backend, kind, n):
    """The class's ``scale_model_input`` / ``step`` loop with eps a fixed affine function of the scaled sample vs the restatement; the bound of
    tests/test_dpmsolver.py::test_step_trajectory_vs_reference.  Euler-ancestral draws from a CPU generator."""
    dev = backend.device
    g = torch.Generator().manual_seed(11)
    shape = (2, 4, 6, 10)
    x0, c = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    d = CLASSES[kind].from_config(SD21, **({} if kind == "pndm" else dict(timestep_spacing="linspace")))
    d.set_timesteps(n, device=dev)
    ref = _ref(kind)
    ref.set_timesteps(n)
    extra = dict(generator=torch.Generator().manual_seed(7)) if kind == "euler_a" else {}
    g2 = torch.Generator().manual_seed(7)
    x, xr = (x0 * d.init_noise_sigma).to(dev), x0.double() * ref.init_noise_sigma
    assert len(d.timesteps) == (n + 1 if kind == "pndm" else n)
    for i, t in enumerate(d.timesteps):
        x = d.step(0.3 * d.scale_model_input(x, t) + c.to(dev), t, x, **extra).prev_sample
        z = torch.randn(shape, generator=g2) if kind == "euler_a" else None
        xr = ref.step(0.3 * ref.scale_model_input(xr, t) + c.double(), ref.timesteps[i], xr, variance_noise=z)
        assert d.step_index == i + 1
    backend.sync()
    assert torch.isfinite(x).all()
    _record(f"trajectory/{backend.name}/{kind}/n{n}", _rel(x, xr), 1e-5)
    d.set_timesteps(n, device=dev)                                               # the counter and the history are reset
    assert d.step_index is None and d._slots is None


# ---------------------------------------------------------------------------------------------------------------------------------
# pipeline: literal loop vs the fp64 restatement, fused vs literal
def _call(pipe, inp, dev, N, steps, h, w, **kw):
    return pipe(height=h * 8, width=w * 8, masked_latents=inp["masked_latents"].to(dev),
                s_img_proj_f=inp["s_img_proj_f"].to(dev), st_pose_f=inp["st_pose_f"].to(dev),
                pred_t_img_embed=inp["pred_t_img_embed"].to(dev), latents=inp["latents"].to(dev),
                num_images_per_prompt=N, guidance_scale=kw.pop("guidance_scale", 2.0), num_inference_steps=steps, output_type="latent",
                **kw).latents


def _same_path(a, b):
    """tests/test_pipeline.py::_same_path standard for several steps."""
    return _rel(a, b) <= 1e-3


def _make(kind, **kw):
    return CLASSES[kind].from_config(SD21, **({} if kind == "pndm" else dict(timestep_spacing="linspace")), **kw)


@pytest.mark.parametrize("kind", ["euler", "euler_a", "lms", "pndm"])
def test_pipeline_fused_vs_literal_vs_reference(backend, kind):
    cfg = UNetConfig.tiny()
    # emulator (CPU-suite budget): one image, two steps -- the second-order LMS step, the averaged and the two-term PLMS call; GPU: two
    # images and every warm-up branch
    N, h, w, L, steps = (1, 8, 8, 4, 2) if backend.is_emu else (2, 16, 24, 9, 6)
    sd, m = _build(backend, cfg, seed=4)
    inp = synth_inputs(cfg, h, w, N, L_img=L)
    pipe = Stage2_InpaintDiffusionPipeline(m, _make(kind))
    calls = []
    inner = m._forward_nhwc
    m._forward_nhwc = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    gen = (lambda: dict(generator=torch.Generator().manual_seed(3))) if kind == "euler_a" else dict
    lit = _call(pipe, inp, backend.device, N, steps, h, w, mode="reference", **gen())
    n_calls = steps + 1 if kind == "pndm" else steps
    assert len(calls) == n_calls                                                 # PNDM: n + 1 UNet calls for n steps
    fused = _call(pipe, inp, backend.device, N, steps, h, w, use_graph=False, **gen())      # fused is the default mode for the four
    assert len(calls) == 2 * n_calls
    m._forward_nhwc = inner
    again = fused if backend.is_emu else _call(pipe, inp, backend.device, N, steps, h, w, **gen())      # (graph replay)
    backend.sync()
    st = pipe._st
    assert st["ms"] and st["coef"].shape == (n_calls, 12) and int(st["step"].item()) == n_calls and int(st["step_err"].item()) == 0
    assert st["timesteps"].dtype == (torch.int64 if kind == "pndm" else torch.float32) and st["scaled"] == (kind != "pndm")
    assert (st["noise"] is not None) == (kind == "euler_a")
    assert torch.equal(again, fused)
    ref_s = _ref(kind)
    if kind == "euler_a":                                                        # the literal loop's draws: one per step, in step order
        g = torch.Generator().manual_seed(3)
        ref_s.noises = [torch.randn((N, 4, h, w), generator=g) for _ in range(steps)]
    ref = stage2_sample(sd, cfg, ref_s, num_images_per_prompt=N, guidance_scale=2.0, num_inference_steps=steps, **inp)
    assert torch.isfinite(lit).all()
    _record(f"pipeline_literal_vs_fp64/{backend.name}/{kind}", _rel(lit, ref), 3e-2)
    _record(f"pipeline_fused_vs_literal/{backend.name}/{kind}", _rel(fused, lit), 3e-2)
    assert _same_path(fused, lit), _rel(fused, lit)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU only
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["euler", "pndm"])
def test_fused_repeatability_graph_eager_c_schedule(gpu_backend, kind):
    """Fused eager == fused graph replay == a second call == ``c_schedule=True``, bit for bit; Euler runs its fractional linspace timesteps
    through ``UNetContext``.  No step overflow after PNDM's n + 1 steps; guidance_rescale goes through the same code."""
    cfg = UNetConfig.tiny()
    dev = gpu_backend.device
    N, h, w, L, steps = 2, 16, 24, 9, 7
    _, m = _build(gpu_backend, cfg, seed=7)
    inp = synth_inputs(cfg, h, w, N, L_img=L)
    pipe = Stage2_InpaintDiffusionPipeline(m, _make(kind))
    eager = _call(pipe, inp, dev, N, steps, h, w, use_graph=False)
    a = _call(pipe, inp, dev, N, steps, h, w)
    assert pipe._graph is not None
    b = _call(pipe, inp, dev, N, steps, h, w)
    torch.cuda.synchronize()
    assert not m.step_overflow() and int(pipe._st["step_err"].item()) == 0
    assert int(pipe._st["step"].item()) == (steps + 1 if kind == "pndm" else steps)
    if kind == "euler":
        assert pipe._st["timesteps"].dtype == torch.float32 and any(float(v) != round(float(v)) for v in pipe._st["timesteps"])
    assert torch.isfinite(a).all() and torch.equal(a, eager) and torch.equal(a, b)
    gr_f = _call(pipe, inp, dev, N, steps, h, w, guidance_rescale=0.7)
    gr_l = _call(pipe, inp, dev, N, steps, h, w, guidance_rescale=0.7, mode="reference")
    assert _same_path(gr_f, gr_l) and _rel(gr_f, a) > 1e-4
    pc = Stage2_InpaintDiffusionPipeline(m, _make(kind), c_schedule=True)
    c1 = _call(pc, inp, dev, N, steps, h, w)
    c2 = _call(pc, inp, dev, N, steps, h, w)
    torch.cuda.synchronize()
    assert pc._ctx is not None and not pc._ctx.step_overflow(2 * N, h, w)
    assert torch.equal(c1, c2) and torch.equal(c1, a), _rel(c1, a)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["euler", "pndm"])
def test_full_size_config1(gpu_backend, kind):
    """Full-size synthetic weights, one image at latent 32 x 64 with CFG (UNet batch 2): finite, deterministic, fused within the bound of
    tests/test_dpmsolver.py::test_full_size_dpmpp_2m_karras_config1 of the literal loop."""
    dev = gpu_backend.device
    cfg = UNetConfig()
    sd = synth_state_dict(cfg, seed=0)
    N, h, w, steps = 1, 32, 64, 10
    inp = synth_inputs(cfg, h, w, N)
    m = Stage2_InapintUNet2DConditionModel(**_kwargs(cfg))
    m.load_state_dict(sd)
    m.to(dev)
    pipe = Stage2_InpaintDiffusionPipeline(m, _make(kind))
    a = _call(pipe, inp, dev, N, steps, h, w)
    b = _call(pipe, inp, dev, N, steps, h, w)
    lit = _call(pipe, inp, dev, N, steps, h, w, mode="reference")
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    _record(f"full_size_fused_vs_literal/{kind}", _rel(a, lit), 1e-3)


if __name__ == "__main__":   # refresh profiles/karras_sampler_values.json from the file a test run left in the scratch directory
    import sys
    src = Path(sys.argv[1]) if len(sys.argv) > 1 else VALUES_OUT
    dst = ROOT / "profiles" / "karras_sampler_values.json"
    old = json.loads(dst.read_text()) if dst.exists() else {}
    vals = dict(old.get("values", {}))
    vals.update(json.loads(src.read_text()))
    old["note"] = "worst relative errors measured by tests/test_karras_samplers.py (emu: the lane emulator; gpu: MI355X) against its float64 restatements"
    old["values"] = vals
    dst.write_text(json.dumps(old, indent=1, sort_keys=True) + "\n")
    print(f"{dst}: {len(vals)} values")
