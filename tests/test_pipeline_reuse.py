"""A long-lived sampling pipeline held to a fresh one across every state its captured step bakes in.

``Stage2_InpaintDiffusionPipeline._run_fused`` keeps static buffers, a hipGraph, a C context and tuning state between calls and decides from a
hand-written key and a few generation tuples whether the old graph may be replayed.  A wrong decision gives plausible, wrong images and no
error, and no kernel test can see it.  Method: ONE pipeline object per schedule (Python schedule, C schedule) walks a fixed list of calls
(``_rows``); after each call its latents are compared, bit for bit, with those of a FRESH pipeline making the same call -- a new UNet object
from the same state dict, a new scheduler object, a new pipeline object.  Successive calls alternate between two conditioning sets (other
latents, masked latents, pose feature, image tokens, prior embedding), so a buffer that was not refreshed always shows.

Two rules make the bit-for-bit comparison legitimate:

1. the GEMM tile choices come from the process-global ``ops._TUNED``, filled by a first-use autotuner whose choice depends on timing.  So every
   distinct call of a walk is first made once on a throw-away pipeline with the result discarded (``_warm``: its tiles are then decided);
   ``len(ops._TUNED)`` must not change over the recorded walk, or the walk fails and says so.
2. only equal launches are compared: a reference-mode call with a fresh pipeline's reference-mode call, a fused call with a fresh fused call
   of the same ``use_graph`` and ``c_schedule``.  Between the modes there is only the ``_same_path`` standard of tests/test_karras_samplers.py,
   under the same ``SHARE_CFG_PREFIX`` switch.

Rows on the lane emulator (the CPU suite).  Measured: one tiny-UNet sampling call (N = 1, latent 8 x 8, L = 4, 2 steps) costs about 35 s
there, and the four ``test_pipeline_fused_vs_literal_vs_reference[emu-*]`` cases take 374 s together; rows 1, 2, 4, 10a and 10 back on both
schedules took 660 s, rows 1, 2 and 4 on the Python schedule with rows 1 and 2 on the C schedule 366 s.  So the emulator keeps rows 1 and 2
(static buffers refilled with new conditioning) on both schedules: eight calls, fresh ones included, ~300 s.  Rows 4-10, 12, 14 and 16 of the
eager subset were moved to the GPU (``test_eager_subset[gpu-*]``, where the whole subset takes seconds).  Rows 3, 11 and 15 (and the stale-graph side of row 16) can only
fail with a graph; row 16 stays in the eager subset on the GPU because the flip also swaps which schedule's buffers a call refreshes.  There is no throw-away walk on the emulator: the autotuner runs on the GPU only.

Row 9: ``DDIMScheduler`` refuses ``prediction_type="v_prediction"`` at construction; the row asserts that refusal and makes its point (a new
scheduler object of the same class and ``kind`` with other coefficients) with ``timestep_spacing="trailing"``.

Step overflow: a callback of the step BEFORE the last pushes the device step counter past the tables, so exactly one step runs there (after
the last step no kernel reads a table any more).  Every reader of a step-indexed table bounds the counter on the device (include/pcdm.h, ABI 6;
tests/test_step_counter.py holds each of them to it on guarded and windowed tables first), so the test runs on the pipeline's own ``[n, width]``
coefficient table and ``[n, numel]`` noise table, for every sampler kind; the stage-1 prior's captured step is replayed once too often likewise.
"""
from __future__ import annotations

import gc
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import pytest
import torch

from oracle.pipeline import synth_inputs
from oracle.unet import UNetConfig, synth_state_dict
from pcdms_amd import ops
from pcdms_amd.pipeline import Stage2_InpaintDiffusionPipeline, Stage3_RefinedDiffusionPipeline
from pcdms_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler
from pcdms_amd.unet import Stage2_InapintUNet2DConditionModel
from tests.test_karras_samplers import _make, _rel, _same_path
from tests.test_schedulers import SD21
from tests.test_unet import _kwargs

CFG = UNetConfig.tiny()
W1, W2 = 4, 9                                                                    # seeds of the two state dicts


@pytest.fixture(autouse=True)
def _modes_compared_on_identical_launches(monkeypatch):
    """As in tests/test_karras_samplers.py: fused and literal loop are compared on identical UNet launches (no CFG-shared prefix)."""
    import pcdms_amd.unet as U
    monkeypatch.setattr(U, "SHARE_CFG_PREFIX", False)


# ---------------------------------------------------------------------------------------------------------------------------------
# calls
@dataclass(frozen=True)
class Call:
    """Everything a sampling call's result depends on: the key of the fresh-result cache."""
    shape: Tuple[int, int, int, int]                                             # N, h, w, L
    steps: int
    inp: str = "A"                                                               # conditioning set
    sched: str = "ddim"
    g: float = 2.0
    gr: float = 0.0
    mode: str = "fused"
    use_graph: bool = True
    c_schedule: bool = False
    weights: int = W1
    freeu: Optional[Tuple[float, float, float, float]] = None
    attn: str = "bf16"


_SD, _INPUTS, _FRESH = {}, {}, {}


def _sd(seed):
    if seed not in _SD:
        _SD[seed] = synth_state_dict(CFG, seed=seed, random_affine=True)
    return _SD[seed]


def _inputs(which, shape):
    """Set A: ``oracle.pipeline.synth_inputs`` (seeds 1..5).  Set B: the same recipe on seeds 11..15 -- every tensor differs."""
    N, h, w, L = shape
    if (which, shape) not in _INPUTS:
        inp = synth_inputs(CFG, h, w, N, L_img=L)
        if which == "B":
            g = [torch.Generator().manual_seed(10 + k) for k in range(6)]
            ml = torch.zeros(1, 4, h, w)
            ml[..., : w // 2] = torch.randn(1, 4, h, w // 2, generator=g[2]) * 0.18215 * 5
            inp = dict(latents=torch.randn(N, 4, h, w, generator=g[1]), masked_latents=ml,
                       st_pose_f=torch.randn(1, CFG.block_out_channels[0], h, w, generator=g[3]) * 0.1,
                       s_img_proj_f=torch.randn(1, L, CFG.cross_attention_dim, generator=g[4]),
                       pred_t_img_embed=torch.randn(1, 1, CFG.projection_class_embeddings_input_dim, generator=g[5]) * 0.4)
            assert all(v.shape == inp[k].shape for k, v in synth_inputs(CFG, h, w, N, L_img=L).items())
        _INPUTS[which, shape] = inp
    return _INPUTS[which, shape]


def _scheduler(name):
    if name == "ddim":
        return DDIMScheduler.from_config(SD21)
    if name == "ddim_trailing":                                                  # same class, same `kind`, other timesteps and coefficients
        return DDIMScheduler.from_config(SD21, timestep_spacing="trailing")
    if name == "unipc":
        return UniPCMultistepScheduler.from_config(SD21)
    if name == "dpm":
        return DPMSolverMultistepScheduler.from_config(SD21)
    if name == "dpm_sde":
        return DPMSolverMultistepScheduler.from_config(SD21, algorithm_type="sde-dpmsolver++")
    return _make(name)                                                           # euler (float timestep table), pndm (n + 1 UNet calls)


def _unet(dev, seed, freeu=None, attn="bf16"):
    m = Stage2_InapintUNet2DConditionModel(**_kwargs(CFG))
    m.load_state_dict(_sd(seed))
    m.to(dev)
    if freeu is not None:
        m.enable_freeu(*freeu)
    m.set_attention_precision(attn)
    return m


def _run(pipe, c: Call, dev, **kw):
    N, h, w, _ = c.shape
    inp = _inputs(c.inp, c.shape)
    if c.sched == "dpm_sde":
        kw["generator"] = torch.Generator().manual_seed(3)
    out = pipe(height=h * 8, width=w * 8, masked_latents=inp["masked_latents"].to(dev), s_img_proj_f=inp["s_img_proj_f"].to(dev),
               st_pose_f=inp["st_pose_f"].to(dev), pred_t_img_embed=inp["pred_t_img_embed"].to(dev), latents=inp["latents"].to(dev),
               num_images_per_prompt=N, guidance_scale=c.g, guidance_rescale=c.gr, num_inference_steps=c.steps, output_type="latent",
               mode=c.mode, use_graph=c.use_graph, **kw).latents
    return out.clone()


def _fresh(c: Call, dev, cache=_FRESH):
    """The call on a fresh UNet / scheduler / pipeline: once per process and distinct call."""
    key = (c, dev.type)
    if key not in cache:
        pipe = Stage2_InpaintDiffusionPipeline(_unet(dev, c.weights, c.freeu, c.attn), _scheduler(c.sched), c_schedule=c.c_schedule)
        cache[key] = _run(pipe, c, dev)
        del pipe
        gc.collect()
    return cache[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# the walk
def _rows(base: Call, shapes, graph: bool):
    """The fixed walk: (row, what to do to the pipeline before the call, the call).  An action is a callable on the walker, or None.
    ``shapes`` = (latent variant, L variant, N variant).  Inputs alternate A / B over the whole list (assigned by ``_walk``)."""
    fu1, fu2 = (0.9, 0.2, 1.2, 1.4), (0.9, 0.2, 1.2, 1.5)
    b = base
    rows = [("01", None, b), ("02", None, b), ("03 guidance scale", None, replace(b, g=3.5)), ("04 no CFG", None, replace(b, g=1.0)),
            ("05 back", None, b), ("06 guidance_rescale", None, replace(b, gr=0.7)), ("06 back", None, b),
            ("07 fewer steps", None, replace(b, steps=b.steps - 1)), ("07 back", None, b)]
    for s in ("unipc", "dpm", "dpm_sde", "euler", "pndm", "ddim"):
        rows.append((f"08 {s}", None, replace(b, sched=s)))
    rows += [("09 v-prediction refused, trailing spacing", "v_refused", replace(b, sched="ddim_trailing")), ("09 back", None, b),
             ("10 reference mode", None, replace(b, mode="reference")), ("10 back", None, b),
             ("10 after a bare forward", "bare_forward", b)]
    if graph:
        rows += [("11 eager", None, replace(b, use_graph=False)), ("11 graph", None, b)]
    for what, shp in zip(("latent", "L", "N"), shapes):
        rows += [(f"12 {what} {shp}", None, replace(b, shape=shp)), (f"12 {what} back", None, b)]
    if graph:
        rows += [("13 FreeU", None, replace(b, freeu=fu1)), ("13 FreeU, one float changed", None, replace(b, freeu=fu2)), ("13 FreeU off", None, b),
                 ("13 fp8 attention", None, replace(b, attn="fp8")), ("13 bf16 attention", None, b)]
    rows += [("14 load_state_dict", "load", replace(b, weights=W2)), ("14 back", "load", b)]
    if graph:
        rows += [("15 pipe.unet replaced", "replace", replace(b, weights=W2)), ("15 back", "replace", b)]
    rows += [("16 c_schedule flipped", None, replace(b, c_schedule=not b.c_schedule)), ("16 back", None, b)]
    if graph:
        rows += [("17 second pipeline, same UNet", "second", b), ("17 first pipeline", "first", b), ("17 second pipeline again", "second", b)]
    return rows


class _Walker:
    """One long-lived pipeline (and a second one sharing its UNet for row 17) brought into the state each call names."""

    def __init__(self, dev, base: Call, cls=Stage2_InpaintDiffusionPipeline):
        self.dev, self.state = dev, base
        self.pipe = cls(_unet(dev, base.weights), _scheduler(base.sched), c_schedule=base.c_schedule)
        self.second = None
        self.active = self.pipe

    def apply(self, action, c: Call):
        pipe, s = self.pipe, self.state
        if action == "v_refused":
            with pytest.raises(NotImplementedError):
                DDIMScheduler.from_config(SD21, prediction_type="v_prediction")
        if action == "bare_forward":   # overwrites the UNet's shared shape-keyed conditioning buffers with the OTHER set's conditioning
            N, h, w, _ = c.shape
            o = _inputs("B" if c.inp == "A" else "A", c.shape)
            B = 2 * N
            x = torch.cat([o["latents"], torch.ones(N, 1, h, w), o["masked_latents"].expand(N, -1, -1, -1)], 1).repeat(2, 1, 1, 1)
            ehs = torch.cat([o["s_img_proj_f"], o["pred_t_img_embed"]], 1).repeat(N, 1, 1)
            ehs = torch.cat([torch.zeros_like(ehs), ehs])                        # (the launches of a reference-mode step: zero uncond context)
            eps = pipe.unet(x.to(self.dev), 417, class_labels=o["pred_t_img_embed"].repeat(B, 1, 1).to(self.dev),
                            encoder_hidden_states=ehs.to(self.dev), my_pose_cond=o["st_pose_f"].to(self.dev), return_dict=False)[0]
            assert bool(torch.isfinite(eps).all())
        if action == "replace":        # the old model is dropped BEFORE the new one is built: CPython may hand out its address again
            for p in (self.pipe, self.second):
                if p is not None:
                    p.unet = None
            gc.collect()
            new = _unet(self.dev, c.weights, s.freeu, s.attn)
            for p in (self.pipe, self.second):
                if p is not None:
                    p.unet = new
        elif c.weights != s.weights:
            assert action == "load"
            pipe.unet.load_state_dict(_sd(c.weights))
        if c.sched != s.sched:
            for p in (self.pipe, self.second):
                if p is not None:
                    p.scheduler = _scheduler(c.sched)
        if c.freeu != s.freeu:
            pipe.enable_freeu(*c.freeu) if c.freeu is not None else pipe.disable_freeu()
        if c.attn != s.attn:
            pipe.unet.set_attention_precision(c.attn)
        if c.c_schedule != s.c_schedule:
            pipe.c_schedule = c.c_schedule
        if action == "second":
            if self.second is None:
                self.second = type(pipe)(pipe.unet, _scheduler(c.sched), c_schedule=c.c_schedule)
            self.active = self.second
        elif action == "first":
            self.active = self.pipe
        self.state = c


_WARM = set()


def _warm(dev, calls):
    """Rule 1: every distinct call, once per process, on a throw-away pipeline whose result is discarded.  What the tuner sees of a call is its
    GEMM shapes, and those do not depend on the conditioning set, on graph replay (the capture's warm-up step tunes eagerly) or on the C
    schedule (its context is handed the tiles that one Python-schedule step of the same batch decided): calls that differ only in these are
    one call here.  Were that wrong, ``len(ops._TUNED)`` would change over the record and the walk would fail.  (GPU only: under the emulator
    every launch takes the library's heuristic tile.)"""
    for c in calls if dev.type == "cuda" else ():
        k = replace(c, inp="A", use_graph=True, c_schedule=False)
        if k not in _WARM:
            _fresh(k, dev, {})
            _WARM.add(k)


def _walk(dev, base: Call, shapes, graph: bool, only=None, fresh_cache=_FRESH):
    """The walk, after the throw-away calls.  Returns ({row: failure text or None}, tuned entries before, after)."""
    rows = _rows(base if graph else replace(base, use_graph=False), shapes, graph)
    if not graph:
        rows = [(r, a, replace(c, use_graph=False)) for r, a, c in rows]
    if only is not None:
        rows = [x for x in rows if x[0] in only]
    rows = [(r, a, replace(c, inp="AB"[i % 2])) for i, (r, a, c) in enumerate(rows)]
    out = {}
    _warm(dev, [c for _, _, c in rows])
    tuned = len(ops._TUNED)
    wk = _Walker(dev, rows[0][2])
    prev_fused = None
    for r, action, c in rows:
        wk.apply(action, c)
        got = _run(wk.active, c, dev)
        want = _fresh(c, dev, fresh_cache)
        why = None
        if not torch.equal(got, want):
            why = f"row {r}: the reused pipeline differs from a fresh one (rel {_rel(got, want):.3g}) in {c}"
        elif c.mode == "reference" and prev_fused is not None:   # rule 2: between the modes only the _same_path standard
            fused = _fresh(replace(c, mode="fused", use_graph=graph), dev, fresh_cache)
            if not _same_path(got, fused):
                why = f"row {r}: reference mode is off the fused result by {_rel(got, fused):.3g}"
        prev_fused = got if c.mode == "fused" else prev_fused
        assert r not in out
        out[r] = why
    del wk
    gc.collect()
    return out, tuned, len(ops._TUNED)


_WALKS = {}
GPU_BASE = Call(shape=(2, 16, 24, 9), steps=3)
GPU_SHAPES = ((2, 16, 16, 9), (2, 16, 24, 5), (1, 16, 24, 9))
EMU_BASE = Call(shape=(1, 8, 8, 4), steps=2, use_graph=False)
EMU_SHAPES = ((1, 8, 4, 4), (1, 8, 8, 3), (2, 8, 8, 4))
EMU_ROWS = ("01", "02")                                                          # (module docstring)
ROW_IDS = [r for r, _, _ in _rows(GPU_BASE, GPU_SHAPES, True)]


def _graph_walk(dev, c_schedule):
    if c_schedule not in _WALKS:
        try:
            _WALKS[c_schedule] = _walk(dev, replace(GPU_BASE, c_schedule=c_schedule), GPU_SHAPES, graph=True)
        except Exception as e:   # (a walk that raises is not made again for each of the row ids)
            _WALKS[c_schedule] = e
    if isinstance(_WALKS[c_schedule], Exception):
        raise RuntimeError("the walk (made once per process) raised") from _WALKS[c_schedule]
    return _WALKS[c_schedule]


@pytest.mark.parametrize("c_schedule", [False, True], ids=["py", "c"])
def test_eager_subset(backend, c_schedule):
    """Rows 1-10, 12, 14 and 16 without a graph (the emulator keeps rows 1 and 2: module docstring)."""
    if backend.is_emu:
        only = EMU_ROWS
        res, t0, t1 = _walk(backend.device, replace(EMU_BASE, c_schedule=c_schedule), EMU_SHAPES, graph=False, only=only, fresh_cache={})
        assert len(res) == len(only)
    else:
        res, t0, t1 = _walk(backend.device, replace(GPU_BASE, c_schedule=c_schedule), GPU_SHAPES, graph=False)
    assert t0 == t1, f"the autotuner decided {t1 - t0} GEMM shapes during the recorded walk: the bit-for-bit comparison was not valid"
    bad = [w for w in res.values() if w]
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("c_schedule", [False, True], ids=["py", "c"])
def test_walk_tuner_was_warm(gpu_backend, c_schedule):
    _, t0, t1 = _graph_walk(gpu_backend.device, c_schedule)
    assert t0 == t1, f"the autotuner decided {t1 - t0} GEMM shapes during the recorded walk: the bit-for-bit comparison was not valid"


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROW_IDS)
@pytest.mark.parametrize("c_schedule", [False, True], ids=["py", "c"])
def test_walk_row(gpu_backend, c_schedule, row):
    """The whole walk with graphs (made once per schedule and process); one test id per row."""
    res, _, _ = _graph_walk(gpu_backend.device, c_schedule)
    assert res[row] is None, f"{res[row]}\n(rows of this walk that differ: {[r for r, why in res.items() if why]})"


# ---------------------------------------------------------------------------------------------------------------------------------
# that the tests bite
@pytest.mark.gpu
@pytest.mark.parametrize("fault", ["guidance scale", "weights re-packed", "c_schedule"])
def test_walk_sees_a_stale_graph(gpu_backend, monkeypatch, fault):
    """One named invalidation is skipped; the row it guards must then differ from the fresh pipeline.  The faults are wrong RESULTS: every
    pointer the stale graph replays stays inside allocations that ``st``, the UNet's ``_bufs`` / packed weights (still referenced by the stale
    graph's owner below) and the context's ``_keep`` hold.  (The dropped-UNet row is not injected: there a stale graph would read freed memory.)"""
    dev = gpu_backend.device
    base = replace(GPU_BASE, c_schedule=fault == "c_schedule")
    a, b = replace(base, inp="A"), replace(base, inp="B")
    warm = [a, replace(b, g=3.5), replace(b, weights=W2), replace(b, c_schedule=False)]
    _warm(dev, warm)                                                             # rule 1
    t0 = len(ops._TUNED)
    wk = _Walker(dev, a)
    assert torch.equal(_run(wk.pipe, a, dev), _fresh(a, dev))
    graph, keep = wk.pipe._graph, None
    assert graph is not None
    if fault == "guidance scale":
        nxt = replace(b, g=3.5)

        class Forgetful(dict):                                                   # st["g_captured"] always "equals" the new g
            def get(self, k, d=None):
                return wk.pipe._st["g"] if k == "g_captured" else dict.get(self, k, d)
        wk.pipe._st = Forgetful(wk.pipe._st)
    elif fault == "weights re-packed":
        nxt = replace(b, weights=W2)
        keep = wk.pipe.unet._w                                                   # the old packed weights stay alive: the stale graph reads live memory
        monkeypatch.setattr(Stage2_InpaintDiffusionPipeline, "_weights_generation", staticmethod(lambda unet, d: 0))
        wk.pipe._st["w_gen"] = 0
    else:
        nxt = replace(b, c_schedule=False)
        assert wk.pipe._graph_key[-1] is True                                    # `key` as before the fix: the same on both sides of the flip
        wk.pipe._graph_key = wk.pipe._graph_key[:-1] + (False,)
    wk.apply("load" if fault == "weights re-packed" else None, nxt)
    got = _run(wk.pipe, nxt, dev)
    assert wk.pipe._graph is graph, "the injected fault did not keep the stale graph"
    want = _fresh(nxt, dev)
    assert not torch.equal(got, want) and _rel(got, want) > 1e-3, f"a stale graph ({fault}) went unseen: rel {_rel(got, want):.3g}"
    del keep
    assert len(ops._TUNED) == t0, "the autotuner decided GEMM shapes between the compared calls: the comparison was not valid"
    del wk
    gc.collect()


# ---------------------------------------------------------------------------------------------------------------------------------
# stage 3 (shares _run_fused) and the stage-1 prior (its own captured step): short walks, same method
def _short_walk(dev, rows, fresh, run, make):
    """``rows``: call descriptions (any hashable); ``make()`` the long-lived object, ``run(obj, row)`` a call, ``fresh(row)`` the same call on
    fresh objects.  Twice (rule 1); returns the rows that differ."""
    bad = []
    for record in (False, True):
        t0, obj, cache = len(ops._TUNED), make(), {}
        for i, row in enumerate(rows):
            got = run(obj, row)
            if row not in cache:
                cache[row] = fresh(row)
            if record and not torch.equal(got, cache[row]):
                bad.append(f"call {i} {row}: rel {_rel(got, cache[row]):.3g}")
        del obj
        gc.collect()
    assert len(ops._TUNED) == t0, "the autotuner decided GEMM shapes during the recorded walk: the bit-for-bit comparison was not valid"
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("c_schedule", [False, True], ids=["py", "c"])
def test_stage3_walk(gpu_backend, c_schedule):
    """Rows 1-5 on ``Stage3_RefinedDiffusionPipeline`` (8 input channels, no mask channel, no pose, no class embedding)."""
    from pcdms_amd import UNet2DConditionModel
    dev = gpu_backend.device
    cfg = UNetConfig.tiny(in_channels=8, class_embed_type=None, projection_class_embeddings_input_dim=None)
    sd = synth_state_dict(cfg, seed=W1, random_affine=True)
    N, h, w, L, steps = 2, 16, 24, 9, 3
    inputs = {}
    for which, seed in (("A", 8), ("B", 18)):
        g = torch.Generator().manual_seed(seed)
        inputs[which] = dict(s_img_proj_f=torch.randn(1, L, cfg.cross_attention_dim, generator=g).to(dev),
                             gen_t_img_latents=(torch.randn(1, 4, h, w, generator=g) * 0.9).to(dev), latents=torch.randn(N, 4, h, w, generator=g).to(dev))

    def make():
        m = UNet2DConditionModel(**_kwargs(cfg))
        m.load_state_dict(sd)
        return Stage3_RefinedDiffusionPipeline(m.to(dev), DDIMScheduler.from_config(SD21), c_schedule=c_schedule)

    def run(pipe, row):
        which, g = row
        return pipe(height=h * 8, width=w * 8, num_images_per_prompt=N, guidance_scale=g, num_inference_steps=steps, output_type="latent",
                    **inputs[which]).latents.clone()
    rows = [("A", 2.0), ("B", 2.0), ("A", 3.5), ("B", 1.0), ("A", 2.0)]
    bad = _short_walk(dev, rows, lambda row: run(make(), row), run, make)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_prior_walk(gpu_backend):
    """``Stage1_PriorPipeline``: the same call twice with new conditioning, another guidance scale, another step count, ``pipe.prior`` replaced
    by a newly built prior with other weights after the old one was dropped, back to the first call."""
    from oracle import prior as O
    from pcdms_amd import Stage1_PriorPipeline, Stage1_PriorTransformer
    from tests.test_prior import _kwargs as prior_kwargs
    dev = gpu_backend.device
    cfg = O.PriorConfig.tiny()
    N = 2
    inputs = {}
    for which, seed in (("A", 21), ("B", 22)):
        g = torch.Generator().manual_seed(seed)
        inputs[which] = dict(s_embed=torch.randn(1, 1, cfg.embedding_dim, generator=g), s_pose=torch.randn(1, cfg.pose_dim, generator=g),
                             t_pose=torch.randn(1, cfg.pose_dim, generator=g), latents=torch.randn(N, cfg.embedding_dim, generator=g),
                             variance_noises=[torch.randn(N, cfg.embedding_dim, generator=g) for _ in range(4)])

    def prior(seed):
        m = Stage1_PriorTransformer(**prior_kwargs(cfg))
        m.load_state_dict(O.synth_state_dict(cfg, seed))
        return m.to(dev)

    def run(pipe, row):
        which, g, steps, seed = row
        if pipe.seed != seed:                                                    # dropped first, then built: the address may be handed out again
            pipe.prior = None
            gc.collect()
            pipe.prior, pipe.seed = prior(seed), seed
        return pipe(num_images_per_prompt=N, num_inference_steps=steps, guidance_scale=g, **inputs[which]).image_embeds.clone()

    def make(seed=1):
        pipe = Stage1_PriorPipeline(prior(seed)).to(dev)
        pipe.seed = seed
        return pipe
    rows = [("A", 2.5, 3, 1), ("B", 2.5, 3, 1), ("A", 4.0, 3, 1), ("B", 2.5, 4, 1), ("A", 2.5, 3, 2), ("B", 2.5, 3, 1), ("A", 2.5, 3, 1)]
    bad = _short_walk(dev, rows, lambda row: run(make(row[3]), row), run, make)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# identity, step overflow, one context at two context lengths
def test_identity_is_a_serial_number_not_an_address(monkeypatch):
    """Two models built one after the other with equal ``_pack_gen`` -- the case in which ``id()`` may coincide once the first is dropped --
    give different generation tuples, also when ``id`` is made to collide outright; so do two contexts and two priors."""
    from types import SimpleNamespace

    import pcdms_amd.pipeline as P
    import pcdms_amd.prior as PR
    from pcdms_amd import Stage1_PriorPipeline
    from oracle import prior as O
    from pcdms_amd import Stage1_PriorTransformer
    from tests.test_prior import _kwargs as prior_kwargs
    for mod in (P, PR):
        monkeypatch.setattr(mod, "id", lambda obj: 7, raising=False)             # every object at "the same address"
    dev = torch.device("cpu")
    a, b = (Stage2_InapintUNet2DConditionModel(**_kwargs(CFG)) for _ in range(2))
    a._pack_gen = b._pack_gen = 1
    ga, gb = (Stage2_InpaintDiffusionPipeline._weights_generation(m, dev) for m in (a, b))
    assert ga != gb and ga[1:] == gb[1:] and ga == Stage2_InpaintDiffusionPipeline._weights_generation(a, dev)
    serials = [a._serial, b._serial]
    del a
    gc.collect()
    c = Stage2_InapintUNet2DConditionModel(**_kwargs(CFG))                       # may sit where `a` sat
    p, q = (Stage1_PriorTransformer(**prior_kwargs(O.PriorConfig.tiny())) for _ in range(2))
    serials += [c._serial, p._serial, q._serial]
    assert len(set(serials)) == len(serials) and serials == sorted(serials)
    p._pack_gen = q._pack_gen = 1                                                # the prior's graph key and the C schedule's tuning key
    kp, kq = Stage1_PriorPipeline._prior_generation(p), Stage1_PriorPipeline._prior_generation(q)
    assert kp != kq and kp[1:] == kq[1:] and kp == Stage1_PriorPipeline._prior_generation(p)
    x, y = SimpleNamespace(_serial=serials[-1] + 1), SimpleNamespace(_serial=serials[-1] + 2)
    assert Stage2_InpaintDiffusionPipeline._context_generation(x, gb) != Stage2_InpaintDiffusionPipeline._context_generation(y, gb)
    assert Stage2_InpaintDiffusionPipeline._context_generation(x, ga) != Stage2_InpaintDiffusionPipeline._context_generation(x, gb)


def test_context_at_two_context_lengths(backend):
    """One ``UNetContext`` prepared at L = 9 and L = 5 for the same (B, h, w): ``forward`` and ``step_overflow`` at either length use the
    workspace prepared at that length, whichever was prepared last -- the bits and flags of two single-length contexts.  (Emulator: one
    sample and the order (9, 5) only, in which the default length is the wrong one for L = 9.)"""
    from pcdms_amd.unet_ctx import UNetContext
    dev = backend.device
    B, h, w = (1, 8, 8) if backend.is_emu else (4, 16, 24)
    m = _unet(dev, W1)
    g = torch.Generator().manual_seed(0)
    s = torch.randn(B, CFG.in_channels, h, w, generator=g)
    p = torch.randn(1, CFG.block_out_channels[0], h, w, generator=g) * 0.1
    ehs = {L: torch.randn(B, L, CFG.cross_attention_dim, generator=g) for L in (9, 5)}
    # each length has its own class labels and its own timestep table of the SAME step count: a time table shared between the two
    # workspaces (it is filled from the workspace's class embedding) would show as the other length's embeddings
    c = {L: torch.randn(B, 1, CFG.projection_class_embeddings_input_dim, generator=g) * 0.4 for L in (9, 5)}
    ts = {9: torch.tensor([801, 401, 1], dtype=torch.int64, device=dev), 5: torch.tensor([961, 517, 83], dtype=torch.int64, device=dev)}
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    sv = {9: 1, 5: 7}                                                            # L = 5 is driven past its table, L = 9 is not

    def prepare(ctx, L):
        pose_b = ctx.prepare_conditioning(B, h, w, ehs[L], c[L], p, zero_ctx_batches=0)
        ctx.prepare_timesteps(ts[L], B, h, w, L=L)
        return pose_b
    single, serials = {}, [m._serial]
    for L in (9, 5):
        ctx = UNetContext(m)
        serials.append(ctx._serial)
        pose_b = prepare(ctx, L)
        if not single:
            x_in = ops.nchw_to_nhwc_bf16(s.to(dev), cpad=m._w["conv_in"].cin)
        step.fill_(sv[L])
        single[L] = (ctx.forward(x_in, ts[L], step, B, h, w, pose_b).clone(), ctx.step_overflow(B, h, w))
    assert single[9][1] is False and single[5][1] is True and not torch.equal(single[9][0], single[5][0])
    for order in ((9, 5),) if backend.is_emu else ((9, 5), (5, 9)):              # (emulator: four forwards in all, ~60 s)
        ctx = UNetContext(m)
        serials.append(ctx._serial)
        pose_b = {L: prepare(ctx, L) for L in order}
        for L in (9, 5):
            step.fill_(sv[L])
            out = ctx.forward(x_in, ts[L], step, B, h, w, pose_b[L], L=L)
            backend.sync()
            assert torch.equal(out, single[L][0]), (order, L)
        assert ctx.step_overflow(B, h, w, L=9) is False and ctx.step_overflow(B, h, w, L=5) is True, order
        assert ctx.step_overflow(B, h, w) is single[order[-1]][1], order          # without L: the length last prepared at this (B, h, w)
    assert serials == sorted(set(serials))                                       # one process-wide count over models and contexts
    with pytest.raises(RuntimeError):
        ctx.forward(x_in, ts[9], step, B + 1, h, w, 1)                              # nothing prepared at this shape: refused before any launch


OVERFLOW_KINDS = {"linear": ("ddim", 4), "unipc": ("unipc", 12), "dpm": ("dpm", 8), "dpm_sde": ("dpm_sde", 8), "table_step": ("euler", 12)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(OVERFLOW_KINDS))
@pytest.mark.parametrize("c_schedule", [False, True], ids=["py", "c"])
def test_step_overflow_is_reported_on_both_schedules(gpu_backend, c_schedule, kind):
    """A callback pushes the device step counter past the tables before the last step: the pipeline raises on the Python schedule AND on the C
    schedule (whose flag lives in the context's workspace), for every sampler kind, and the next call on the same pipeline succeeds and equals
    a fresh one.  The tables are the pipeline's own allocations of exactly n rows: the step that runs with the counter at 2n - 1 is bounded by
    the kernels (tests/test_step_counter.py)."""
    dev = gpu_backend.device
    sched, width = OVERFLOW_KINDS[kind]
    a, b = replace(GPU_BASE, c_schedule=c_schedule, inp="A", sched=sched), replace(GPU_BASE, c_schedule=c_schedule, inp="B", sched=sched)
    n = a.steps
    _warm(dev, (a, b))                                                           # rule 1
    t0 = len(ops._TUNED)
    wk = _Walker(dev, a)
    pipe = wk.pipe
    if kind == "linear":
        assert torch.equal(_run(pipe, replace(a, use_graph=False), dev), _fresh(a, dev))   # (eager == graph: tests/test_karras_samplers.py)
    assert torch.equal(_run(pipe, a, dev), _fresh(a, dev))                       # captures the graph
    coef = pipe._st["coef"]
    assert tuple(coef.shape) == (n, width) and coef.is_contiguous() and coef.untyped_storage().nbytes() == n * width * 4   # production layout: no slack
    assert pipe._st["noise"] is None or tuple(pipe._st["noise"].shape) == (n, a.shape[0] * 4 * a.shape[1] * a.shape[2])
    assert int(pipe._st["step_err"].item()) == 0

    def push(i, t, lat):
        if i == n - 2:
            pipe._st["step"] += n
    with pytest.raises(RuntimeError, match="step counter left the time-embedding table"):
        _run(pipe, b, dev, callback=push)
    assert int(pipe._st["step_err"].item()) == 1                                 # the sampler's own step kernel clamped and said so
    assert pipe._st["coef"].data_ptr() == coef.data_ptr()
    assert torch.equal(_run(pipe, b, dev), _fresh(b, dev))
    assert torch.equal(_run(pipe, a, dev), _fresh(a, dev))
    assert len(ops._TUNED) == t0


@pytest.mark.gpu
def test_prior_step_overflow_is_reported(gpu_backend):
    """Stage 1: after a normal graph call the captured step is replayed once more -- the counter is then n, one past the timestep, coefficient and
    noise tables.  The kernels clamp it and raise the flag, the check behind the replays raises, and a following normal call succeeds and
    equals a fresh pipeline's output bit for bit."""
    from oracle import prior as O
    from pcdms_amd import Stage1_PriorPipeline, Stage1_PriorTransformer
    from tests.test_prior import _kwargs as prior_kwargs
    dev = gpu_backend.device
    cfg = O.PriorConfig.tiny()
    N, steps = 2, 3
    g = torch.Generator().manual_seed(21)
    inp = dict(s_embed=torch.randn(1, 1, cfg.embedding_dim, generator=g), s_pose=torch.randn(1, cfg.pose_dim, generator=g),
               t_pose=torch.randn(1, cfg.pose_dim, generator=g), latents=torch.randn(N, cfg.embedding_dim, generator=g),
               variance_noises=[torch.randn(N, cfg.embedding_dim, generator=g) for _ in range(steps)])

    def make():
        m = Stage1_PriorTransformer(**prior_kwargs(cfg))
        m.load_state_dict(O.synth_state_dict(cfg, 1))
        return Stage1_PriorPipeline(m.to(dev)).to(dev)

    def run(pipe):
        return pipe(num_images_per_prompt=N, num_inference_steps=steps, guidance_scale=2.5, **inp).image_embeds.clone()
    run(make())                                                                  # rule 1: the tiles of this call are decided
    t0 = len(ops._TUNED)
    want = run(make())
    pipe = make()
    assert torch.equal(run(pipe), want)
    st = pipe._gst
    assert tuple(st["coef"].shape) == (steps, 8) and tuple(st["noise"].shape) == (steps, N * cfg.embedding_dim) and st["ts"].numel() == steps
    assert int(st["step"].item()) == steps and int(st["step_err"].item()) == 0
    pipe._check_step_counter()                                                   # nothing to report yet
    st["graph"].replay()                                                         # one replay too many: the counter is n
    torch.cuda.synchronize()
    assert int(st["step"].item()) == steps + 1 and int(st["step_err"].item()) == 1
    with pytest.raises(RuntimeError, match="step counter left the step tables"):
        pipe._check_step_counter()
    assert torch.equal(run(pipe), want)                                          # the flag is zeroed per call; the result is a fresh pipeline's
    assert len(ops._TUNED) == t0
