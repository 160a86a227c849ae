"""Conformance of the sampler-step and elementwise kernels (pcdms_amd/csrc/misc.hip) against fp64 references of the same operands.

The form is that of the GEMM, attention and norm suites: an fp64 reference of exactly the operands the kernel reads, a per-element bound derived
from the kernel's arithmetic BEFORE it ran, outputs that are windows of sentinel-filled buffers (``Win``: nothing outside the window changes,
nothing inside stays unwritten), table rows and noise slabs the kernel must not read filled with NaN, every GPU call twice from the same
state with the same bits, and the largest ``err / bound`` per family in the parity record (``small_ops/<family>``, asserted <= 1).
``test_*_bites`` show per family that the bound refuses a slightly wrong result.

Notation: u = u32 = 2^-24 (fp32 unit roundoff), u16 = 2^-8 (bf16), gamma(k) = k u / (1 - k u).  hipcc contracts ``a * b + c`` into one FMA
(-ffp-contract=fast), the emulator build does not: every count below takes the uncontracted chain, contraction only removes roundings.

(a) Linear step kernels
-----------------------
Each output is a sum of products of fp32 operands; by the standard forward analysis of such an expression ``|out - ref| <= gamma(k) * A``
where A is the same expression with every operand and coefficient replaced by its magnitude (a subtraction becomes a sum) and k the number
of fp32 operations on the longest path from an operand to the output.  Counted from misc.hip:

* guided eps      e  = e0 + g * (e1 - e0)                                   sub, mul, add                          k = 3  (cfg off: exact)
* cfg_step        v  = c0 x + c1 e + c2 noise                               e (3), mul, add, add                   k = 6; eps_out = e: 3
* unipc_step      mt = c0 x + c1 e                                          e (3), mul, add                        k = 5
                  xc = c3 last + c4 m1 + c5 m2 + c6 mt                      mt (5), mul, add                       k = 7  (c2 == 0: xc = x, exact)
                  x' = c7 xc + c8 mt + c9 m1                                xc (7), mul, add, add                  k = 10
                  m2' = m1 (exact), m1' = mt (5), last' = xc (7)
* dpmpp_step      m0 = c0 x + c1 e (5);  x' = c2 x + c3 m0 + c4 m1 + c5 z   m0 (5), mul, add, add, add             k = 9;  m1' = m0: 5
* unclip_step     x0 = clamp(c0 x + c1 e) (5; the clamp is exact and 1-Lipschitz: an error in front of it is not enlarged)
  (and _dev)      v  = (c3 x0 + c4 x + c5 z) c6 + c7                         x0 (5), mul, add, add, mul, add        k = 10
* lincomb         v  = 0 + c0 x0 + ... : the first product passes every add                                        k = nin + 1
* advance chain   three unipc steps on the kernel's own state: the error of the state enters the next step through the same magnitude
                  expression (it is linear in the state), so E' = gamma(k) A + (1 + gamma(k)) A(E) with A(E) the expression evaluated on the
                  incoming error bounds and a zero eps.
* rescale_noise_cfg: both variances in fp64 (single pass: at mean 100 / std 0.01 the cancellation costs 1e8 * 2^-53 ~ 1e-8 relative, far
  below u), then ``factor = (float)sqrt`` (1), ``gr * factor`` (1), ``1 - gr`` (1), the add (1), ``a * f`` (1): 5 roundings, each of a term
  that ``|a| (|gr| factor + |1 - gr|)`` bounds; the bound is 6 u of that.

(b) softmax_rows
----------------
With t = scale * log2(e) * s (exact), M = max |t| over the row, D_i = t_max - t_i >= 0 and Z = sum 2^-D_j >= 1 (p_i = 2^-D_i / Z):

* the kernel's exponent is ``fl(fl(fl(scale * LOG2E) * s_i) - mx)``: the two roundings of the constant are a common factor (1 + eps), |eps| <= 2u,
  on every t; the product rounds once (delta_i), the subtraction once (eta_i; exact by Sterbenz where D_i <= t_max).  The error of the
  exponent of element i relative to element j is ``delta_i t_i - delta_j t_j`` (<= 2 u M) plus ``(eps + eta)``-terms proportional to D:
  at most 3 u D_i for the element and, averaged over the row with weights p_j, 3 u sum p_j D_j <= 3 u log2(cols) <= 3 u 13 (D_j <=
  log2(1 / p_j) and the entropy of 8192 outcomes is at most 13 bits).  2^x has the derivative ln 2: the M part is 1.39 u M -- the bound's
  4 u M has a factor 2.9 over it --, the D part 2.08 u (D_i + 13).
* An element with D_i > 126 has a subnormal (or flushed: v_exp_f32 has no denormal results) numerator and p_i < 2^-126: no relative bound
  exists there; the tests hold such elements only as -inf (exactly 0 on both sides) and in the one-hot row, whose other entries are below
  the floor on both sides.  So D_i <= 126 and the D part is at most 2.08 * 139 u = 290 u.
* exp2 (v_exp_f32: 1 ulp = 2 u) for the element and, averaged, for the sum: 4 u; the sum of positives: 32 serial adds per thread, 6 shuffle
  adds, 3 adds of the wave partials: 41 u; the reciprocal (an IEEE division): u; the product: u.
* 290 + 4 + 41 + 2 = 337 u = 4 u * 84.3: **c = 96** (the next multiple of 32), fixed before any run.  Against u16 = 65536 u it is 0.6 % of the
  bound: the bf16 store dominates everywhere but in the shifted rows, where 4 u M is a quarter of it.
* the store rounds to bf16: u16 p; 2^-133 is the smallest bf16 subnormal (a result below it may round either way).

(c) small_linear
----------------
A lane accumulates K / 64 products (8 per trip of 512 columns) in K / 64 adds, the wave sums in 6, bias and ``add`` take one each, each
product one: K / 64 + 9 <= K / 64 + 16 operations on the longest path, over the magnitude ``sum_k |act(x)| |w| + |bias| + |add|`` (bias and add
belong to the expression that is rounded, so they belong to its magnitude).  SiLU: ``silu_f(x) = x / (1 + __expf(-x))`` has no derivable
error on the GPU (__expf is v_exp_f32 behind a product with log2 e, whose rounding error grows with |x|), so it is MEASURED through this very
entry (``test_measure_silu``: a one-hot weight of 1.0 makes y = silu_f(x) exactly) over [-100, 100] and recorded as ``small_ops/silu_rel``;
the constant of the bound, C_SILU, is twice the recorded value rounded up to a power of two.  Where |silu| < 1e-30 (x < -73.4) both sides are
below 1e-30 in magnitude with the same sign: SILU_FLOOR = 2^-98 (3.2e-30) covers it.  act_in adds C_SILU sum |silu(x)| |w| + SILU_FLOOR sum |w|;
act_out adds C_SILU |silu(v)| + SILU_FLOOR and carries the error of v through SiLU's slope (at most 1.1).

(d) timestep embedding
----------------------
``f = expf(-ln(1e4) k / (half - shift))``: the product and the quotient round the argument (|arg| <= ln 1e4 = 9.21) twice: 2 u * 9.21 absolute in
the exponent = relative in f; expf is 1 ulp (2 u); ``t * f`` rounds once: the angle a = t f has the relative error u (2 * 9.21 + 3) <= 4 u (1 +
ln 1e4) = 40.8 u -- a factor 1.9.  sin / cos have slope <= 1 and are good to 1 ulp of a value <= 1, with another for slack: 2 u.
``|out - ref| <= |t f| * 4 u (1 + ln 1e4) + 2 u``: a bound on fp32 evaluation of the formula, which the oracle's own fp32 evaluation is asserted
to meet as well.

(e) exact kernels: bit for bit; time_class_combine: one fp32 add in front of SiLU (u (|emb| + |cls|) through a slope <= 1.1), C_SILU |silu| +
SILU_FLOOR, the bf16 store u16 |silu|.  gaussian_sample: ``0.5 * lv`` is exact, __expf is measured as SiLU's is (``test_measure_expf``,
``small_ops/expf_rel``, over the clamp range [-30, 20]: C_EXPF); e * z, the add, the product with scale: 3 u of (|mean| + e |z|) |scale|.

(f) quantize_fp8: no bound -- the decoded bytes equal torch's float8_e4m3fn cast (round to nearest even) of clamp(fp32(bf16 * scale), +-448).
"""
from __future__ import annotations

import ctypes as C
import math

import pytest
import torch

from pcdms_amd import _lib, ops

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
U32 = 2.0 ** -24
U16 = 2.0 ** -8
LOG2E = 1.4426950408889634
C_SOFTMAX = 96.0            # derived in (b)
# Measured on the MI355X through the entries themselves and kept in profiles/r6_parity_values.json: small_ops/silu_rel = 3.659e-6 (61.4 u32,
# at x = -72.125: the product with log2 e in front of v_exp_f32 costs |x| u32) and small_ops/expf_rel = 8.839e-7 (14.8 u32, at lv = -27.56).
# The constants are twice the recorded value, rounded up to a power of two.  (The emulator's libm expf: 1.27e-7 and 5.9e-8.)
SILU_REL_RECORDED = 3.659e-6
EXPF_REL_RECORDED = 8.839e-7
C_SILU = 2.0 ** -17         # _pow2_ceil(2 * SILU_REL_RECORDED) = 7.63e-6
C_EXPF = 2.0 ** -19         # _pow2_ceil(2 * EXPF_REL_RECORDED) = 1.91e-6
assert C_SILU == 2.0 ** math.ceil(math.log2(2.0 * SILU_REL_RECORDED)) and C_EXPF == 2.0 ** math.ceil(math.log2(2.0 * EXPF_REL_RECORDED))
SILU_FLOOR = 2.0 ** -98
NS = (1, 255, 256, 257, 1000)
N_GPU = 4 * 64 * 88
GUARD = 64                  # elements in front of and behind every window (the windows stay 16-byte aligned for every element size)
SENT = {F32: (torch.int32, 0x7FA5A5A5), BF16: (torch.int16, 0x7FA5), U8: (torch.uint8, 0x55), torch.int32: (torch.int32, 0x7FA5A5A5)}
WORST = {}                  # family -> largest err / bound seen in this process


def gamma(k: int) -> float:
    return k * U32 / (1.0 - k * U32)


def ns_for(backend):
    return NS + (() if backend.is_emu else (N_GPU,))


# ------------------------------------------------------------------------------------------------ windows, launches, comparison
class Win:
    """``n`` elements inside a sentinel-filled buffer with GUARD elements on either side; ``init``: an in-place state (the window starts as it)"""

    def __init__(self, n: int, dtype, dev, init=None):
        self.n, self.dtype, self.itype, self.pat = n, dtype, *SENT[dtype]
        self.buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
        self.buf.view(self.itype).fill_(self.pat)
        self.t = self.buf[GUARD:GUARD + n]
        self.state = init is not None
        if init is not None:
            self.t.copy_(init.reshape(-1).to(dtype))

    @property
    def ptr(self) -> int:
        return self.t.data_ptr()

    def bits(self) -> torch.Tensor:
        return self.buf.view(self.itype).cpu().clone()

    def get(self) -> torch.Tensor:
        return self.t.cpu().clone()

    def problems(self, name: str, keep=None) -> list:
        """guards intact; no element of an output window still the sentinel -- except where ``keep`` (a bool mask over the window) says the
        kernel must NOT write: there every element must still be the sentinel"""
        b = self.buf.view(self.itype).cpu()
        out = []
        if not bool((b[:GUARD] == self.pat).all() and (b[GUARD + self.n:] == self.pat).all()):
            out.append(f"{name}: written outside its window")
        w = b[GUARD:GUARD + self.n] == self.pat
        if keep is not None:
            if not bool(w[keep.reshape(-1)].all()):
                out.append(f"{name}: {int((~w[keep.reshape(-1)]).sum())} elements written that must keep their content")
            w = w[~keep.reshape(-1)]
        if not self.state and int(w.sum()):
            out.append(f"{name}: {int(w.sum())} elements never written")
        return out

    def untouched(self) -> bool:
        return bool((self.buf.view(self.itype).cpu() == self.pat).all())


def launch(backend, go):
    """``go()`` builds its state afresh, calls the library and returns (rc, [Win, ...]).  GPU: twice, the same bits."""
    rc, wins = go()
    backend.sync()
    if not backend.is_emu:
        rc2, wins2 = go()
        backend.sync()
        assert rc2 == rc, (rc, rc2)
        for i, (a, b) in enumerate(zip(wins, wins2)):
            assert torch.equal(a.bits(), b.bits()), f"window {i}: the second run differs from the first"
    return rc, wins


def compare(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor):
    """(violations, largest err / bound, flat index of the worst element); a non-finite output where the reference is finite is a violation"""
    out = out.double().cpu().reshape(ref.shape)
    bad = ~torch.isfinite(out)
    err = (torch.where(bad, torch.zeros_like(out), out) - ref).abs()
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    ratio = torch.where(bad, torch.full_like(ratio, float("inf")), ratio)
    worst = int(ratio.argmax())
    return int((ratio > 1.0).sum()), float(ratio.flatten()[worst]), worst


def judge(family: str, tag: str, out, ref, bound, fails: list):
    nviol, worst, at = compare(out, ref, bound)
    WORST[family] = max(WORST.get(family, 0.0), worst if math.isfinite(worst) else 1e30)
    if nviol:
        fails.append(f"{tag}: {nviol} elements beyond the bound, worst err / bound {worst:.4g} at {at}: out "
                     f"{float(out.double().flatten()[at]):.9g} ref {float(ref.flatten()[at]):.9g}")


def record(backend, *families):
    """GPU: the largest err / bound of the families so far, to the parity record (asserted <= 1)"""
    for f in families:
        print(f"small_ops/{f}: err / bound {WORST.get(f, 0.0):.4f} [{backend.name}]")
        if not backend.is_emu:
            from tests import parity_record
            parity_record.check(f"small_ops/{f}", WORST.get(f, 0.0), 1.0)


def rnd(seed: int, *shape, scale: float = 1.0, mean: float = 0.0) -> torch.Tensor:
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).mul(scale).add(mean).float()


def dev_f32(t: torch.Tensor, dev) -> torch.Tensor:
    return t.to(F32).contiguous().to(dev)


def nan_table(rows: int, width: int, sel: int, row: torch.Tensor, dev) -> torch.Tensor:
    """[rows, width] fp32, NaN except row ``sel``"""
    t = torch.full((rows, width), float("nan"), dtype=F32)
    t[sel] = row
    return t.contiguous().to(dev)


def step_tensor(step, dev):
    return None if step is None else torch.tensor([step], dtype=torch.int32, device=dev)


def lib():
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ (a) references: value and magnitude
def guided(e0, e1, g, cfg, mag=False):
    """e = e0 + g (e1 - e0); ``mag``: operands are magnitudes, the subtraction becomes a sum.  -> (e, roundings)"""
    if not cfg:
        return e0, 0
    return e0 + g * ((e1 + e0) if mag else (e1 - e0)), 3


def split_eps(eps: torch.Tensor, n: int, cfg):
    e = eps.double()
    return e[:n], (e[n:2 * n] if cfg else None)


def eval_both(fn, tensors: dict, coef):
    """fn(tensors, coef, mag) evaluated on the fp64 operands and on their magnitudes"""
    val = fn({k: (None if v is None else v.double()) for k, v in tensors.items()}, [float(c) for c in coef], False)
    mag = fn({k: (None if v is None else v.double().abs()) for k, v in tensors.items()}, [abs(float(c)) for c in coef], True)
    return val, mag


def cfg_step_ref(t, c, mag):
    e, _ = guided(t["e0"], t["e1"], c[4], t["e1"] is not None, mag)
    v = c[0] * t["x"] + c[1] * e
    if t["noise"] is not None:
        v = v + c[2] * t["noise"]
    return {"eps_out": e, "x_prev": v}


def unipc_ref(t, c, mag):
    """c = the 12 table floats + [g]"""
    e, _ = guided(t["e0"], t["e1"], c[12], t["e1"] is not None, mag)
    mt = c[0] * t["x"] + c[1] * e
    xc = t["x"] if c[2] == 0 else c[3] * t["last"] + c[4] * t["m1"] + c[5] * t["m2"] + c[6] * mt
    return {"x": c[7] * xc + c[8] * mt + c[9] * t["m1"], "m1": mt, "m2": t["m1"], "last": xc}


def dpmpp_ref(t, c, mag):
    """c = the 8 table floats + [g]"""
    e, _ = guided(t["e0"], t["e1"], c[8], t["e1"] is not None, mag)
    m0 = c[0] * t["x"] + c[1] * e
    v = c[2] * t["x"] + c[3] * m0 + c[4] * t["m1"]
    if t["noise"] is not None:
        v = v + c[5] * t["noise"]
    return {"x": v, "m1": m0}


def unclip_ref(t, c, mag):
    """c = the 8 coefficients + [g]; the magnitude passes through the clamp unclamped (an upper bound of it)"""
    e, _ = guided(t["e0"], t["e1"], c[8], t["e1"] is not None, mag)
    x0 = c[0] * t["x"] + c[1] * e
    if c[2] > 0 and not mag:
        x0 = x0.clamp(-c[2], c[2])
    v = c[3] * x0 + c[4] * t["x"]
    if t["noise"] is not None:
        v = v + c[5] * t["noise"]
    return {"x": v * c[6] + c[7]}


K_CFG = {"eps_out": 3, "x_prev": 6}
K_UNIPC = {"x": 10, "m1": 5, "m2": 0, "last": 7}
K_DPMPP = {"x": 9, "m1": 5}
K_UNCLIP = {"x": 10}


def eps_pair(seed: int, n: int, cfg: bool, dev):
    """(host eps [2n]: the second half NaN when cfg is off -- it must not be read --, device copy)"""
    eps = torch.cat([rnd(seed, n), rnd(seed + 1, n, scale=1.5, mean=0.25)])
    if not cfg:
        eps[n:] = float("nan")
    return eps, eps.to(dev)


# ------------------------------------------------------------------------------------------------ (a) cfg_step
CFG_COEF = (0.98828125, -0.15625, 0.0625, float("nan"))     # {cx, ce, cn, unused}: the unused slot must not matter


def run_cfg_step(backend, n, cfg, step, with_noise, outs, fails, g=7.5, swap_check=False):
    dev = backend.device
    eps, eps_d = eps_pair(10 + n, n, cfg, dev)
    x, noise = rnd(20 + n, n, scale=2.0), (rnd(30 + n, n) if with_noise else None)
    coef = torch.tensor(CFG_COEF, dtype=F32)
    tab = nan_table(4, 4, step or 0, coef, dev)
    x_d, noise_d, st = x.to(dev), (None if noise is None else noise.to(dev)), step_tensor(step, dev)

    def go():
        xp = Win(n, F32, dev) if "x_prev" in outs else None
        eo = Win(n, F32, dev) if "eps_out" in outs else None
        rc = lib().pcdm_cfg_step(eps_d.data_ptr(), int(cfg), g, x_d.data_ptr(), ops._ptr(noise_d), xp.ptr if xp else None, eo.ptr if eo else None,
                                 tab.data_ptr(), 4, ops._ptr(st), None, n, ops._stream(eps_d))
        return rc, [w for w in (xp, eo) if w is not None]

    rc, wins = launch(backend, go)
    tag = f"cfg_step[n={n} cfg={int(cfg)} step={step} noise={int(with_noise)} outs={'+'.join(outs)}]"
    if rc != 0:
        fails.append(f"{tag}: refused ({rc})")
        return
    e0, e1 = split_eps(eps, n, cfg)
    val, mag = eval_both(cfg_step_ref, {"e0": e0, "e1": e1, "x": x, "noise": noise}, list(coef[:3]) + [0.0, g])
    names = [k for k in ("x_prev", "eps_out") if k in outs]
    for name, w in zip(names, wins):
        fails += w.problems(f"{tag} {name}")
        judge("steps", f"{tag} {name}", w.get(), val[name], gamma(K_CFG[name]) * mag[name], fails)
    if swap_check and cfg:       # the second half is read at exactly eps[n + i]: the halves swapped is another result
        sw, _ = eval_both(cfg_step_ref, {"e0": e1, "e1": e0, "x": x, "noise": noise}, list(coef[:3]) + [0.0, g])
        assert compare(wins[0].get(), sw[names[0]], gamma(K_CFG[names[0]]) * mag[names[0]])[0] > 0, f"{tag}: passes with the halves swapped"


def test_cfg_step(backend):
    fails = []
    for n in ns_for(backend):
        for i, (cfg, step, noise, outs) in enumerate((c, s, z, o) for c in (False, True) for s in (None, 0, 3) for z in (False, True)
                                                     for o in (("eps_out",), ("x_prev",), ("x_prev", "eps_out"))):
            if n in (257, N_GPU) or i % 5 == n % 5:      # every combination at two sizes, a fifth of them at the others
                run_cfg_step(backend, n, cfg, step, noise, outs, fails, swap_check=True)
    assert not fails, "\n".join(fails)
    record(backend, "steps")


# ------------------------------------------------------------------------------------------------ (a) unipc_step, the advance chain
def unipc_row(i: int, corrector: bool) -> torch.Tensor:
    r = torch.tensor([1.015625 + 0.01 * i, -0.21875 - 0.01 * i, 1.0 if corrector else 0.0, 0.6875, -0.40625 + 0.02 * i, 0.109375, 0.59375,
                      0.9375 - 0.01 * i, 0.28125, -0.171875, float("nan"), float("nan")], dtype=F32)     # the two unused slots must not matter
    if not corrector:
        r[3:7] = float("nan")            # a first step must not touch the corrector's coefficients either
    return r


def unipc_state(seed, n, corrector):
    st = {"x": rnd(seed, n, scale=2.0), "m1": rnd(seed + 1, n), "m2": rnd(seed + 2, n), "last": rnd(seed + 3, n, scale=2.0)}
    if not corrector:
        st["last"] = torch.full((n,), float("nan"))     # uninitialised history
    return st


def run_unipc(backend, n, cfg, step, corrector, fails, g=2.0):
    dev = backend.device
    eps, eps_d = eps_pair(40 + n, n, cfg, dev)
    st0 = unipc_state(50 + n, n, corrector)
    row = unipc_row(1, corrector)
    tab = nan_table(4, 12, step or 0, row, dev)
    st = step_tensor(step, dev)

    def go():
        w = {k: Win(n, F32, dev, init=v) for k, v in st0.items()}
        rc = lib().pcdm_unipc_step(eps_d.data_ptr(), int(cfg), g, w["x"].ptr, w["m1"].ptr, w["m2"].ptr, w["last"].ptr, tab.data_ptr(), 4, ops._ptr(st),
                                   None, n, ops._stream(eps_d))
        return rc, [w[k] for k in ("x", "m1", "m2", "last")]

    rc, wins = launch(backend, go)
    tag = f"unipc_step[n={n} cfg={int(cfg)} step={step} corrector={int(corrector)}]"
    if rc != 0:
        fails.append(f"{tag}: refused ({rc})")
        return
    e0, e1 = split_eps(eps, n, cfg)
    c = [0.0 if math.isnan(float(v)) else float(v) for v in row] + [g]
    tens = dict(st0, e0=e0, e1=e1)
    if not corrector:
        tens["last"] = torch.zeros(n)
    val, mag = eval_both(unipc_ref, tens, c)
    for name, w in zip(("x", "m1", "m2", "last"), wins):
        fails += w.problems(f"{tag} {name}")
        k = 0 if name == "m2" or (name == "last" and not corrector) else K_UNIPC[name]
        if k == 0:
            want = st0["m1"] if name == "m2" else st0["x"]
            if not torch.equal(w.get().view(torch.int32), want.view(torch.int32)):
                fails.append(f"{tag}: {name} is not the old {'m1' if name == 'm2' else 'x'} bit for bit")
        else:
            judge("steps", f"{tag} {name}", w.get(), val[name], gamma(k) * mag[name], fails)


def test_unipc_step(backend):
    fails = []
    for n in ns_for(backend):
        for cfg in (False, True):
            for step in (None, 0, 3):
                for corrector in (False, True):
                    run_unipc(backend, n, cfg, step, corrector, fails)
    assert not fails, "\n".join(fails)
    record(backend, "steps")


def test_unipc_three_chained_steps(backend):
    """three steps on the kernel's own state with pcdm_advance_step between them, against the fp64 recurrence with the bound accumulated; the
    exact parts of the advance (m2 <- m1, m1 <- m_t, last <- x_c) are compared bit for bit with what the step before left"""
    dev, fails, g = backend.device, [], 3.0
    for n in ns_for(backend):
        rows = [unipc_row(0, False), unipc_row(1, True), unipc_row(2, True), torch.full((12,), float("nan"))]
        tab = torch.stack(rows).contiguous().to(dev)
        eps = [eps_pair(60 + 7 * s + n, n, True, dev) for s in range(3)]
        st0 = unipc_state(70 + n, n, False)
        st0["m1"], st0["m2"] = torch.zeros(n), torch.zeros(n)        # pcdm.h: zero m1 / m2 / last before step 0 (last: NaN here, never read)

        def go():
            w = {k: Win(n, F32, dev, init=v) for k, v in st0.items()}
            step = Win(1, torch.int32, dev, init=torch.zeros(1, dtype=torch.int32))
            snaps, rc = [], 0
            for s in range(3):
                rc |= lib().pcdm_unipc_step(eps[s][1].data_ptr(), 1, g, w["x"].ptr, w["m1"].ptr, w["m2"].ptr, w["last"].ptr, tab.data_ptr(),
                                            4, step.ptr, None, n, ops._stream(tab))
                rc |= lib().pcdm_advance_step(step.ptr, ops._stream(tab))
                snaps.append({k: Win(n, F32, dev, init=v.t) for k, v in w.items()})
            go.snaps, go.step = snaps, step
            return rc, [w[k] for k in ("x", "m1", "m2", "last")] + [step] + [sn[k] for sn in snaps for k in ("x", "m1", "m2", "last")]

        rc, wins = launch(backend, go)
        tag = f"unipc chain[n={n}]"
        assert rc == 0, tag
        for w in wins[:5]:
            fails += w.problems(tag)
        if int(go.step.get()[0]) != 3:
            fails.append(f"{tag}: the step counter is {int(go.step.get()[0])} after three advances")
        ref = {k: v.double() for k, v in st0.items()}
        ref["last"] = torch.zeros(n, dtype=torch.float64)
        err = {k: torch.zeros(n, dtype=torch.float64) for k in ref}
        prev = {k: v for k, v in st0.items()}
        for s in range(3):
            corrector = s > 0
            c = [0.0 if math.isnan(float(v)) else float(v) for v in rows[s]] + [g]
            e0, e1 = split_eps(eps[s][0], n, True)
            val, mag = eval_both(unipc_ref, dict(ref, e0=e0, e1=e1), c)
            zero = torch.zeros(n)
            _, prop = eval_both(unipc_ref, dict(err, e0=zero, e1=zero), c)
            got = {k: go.snaps[s][k].get() for k in ref}
            new_err = {}
            for name in ("x", "m1", "m2", "last"):
                k = 0 if name == "m2" or (name == "last" and not corrector) else K_UNIPC[name]
                new_err[name] = gamma(k) * mag[name] + (1.0 + gamma(k)) * prop[name]
                if k:
                    judge("steps", f"{tag} step {s} {name}", got[name], val[name], new_err[name], fails)
            if not torch.equal(got["m2"].view(torch.int32), prev["m1"].view(torch.int32)):
                fails.append(f"{tag} step {s}: m2 is not the old m1 bit for bit")
            if not corrector and not torch.equal(got["last"].view(torch.int32), prev["x"].view(torch.int32)):
                fails.append(f"{tag} step {s}: last is not the old x bit for bit (no corrector: x_c = x)")
            ref, err, prev = val, new_err, got
    assert not fails, "\n".join(fails)
    record(backend, "steps")


# ------------------------------------------------------------------------------------------------ (a) dpmpp_step, unclip_step, unclip_step_dev, lincomb
DPMPP_ROW = (0.9921875, -0.1328125, 0.71875, 0.3046875, -0.0859375, 0.15625, float("nan"), float("nan"))


def run_dpmpp(backend, n, cfg, step, with_noise, fails, g=2.0):
    dev = backend.device
    eps, eps_d = eps_pair(80 + n, n, cfg, dev)
    x, m1 = rnd(81 + n, n, scale=2.0), rnd(82 + n, n)
    noise = rnd(83 + n, n) if with_noise else None
    row = torch.tensor(DPMPP_ROW, dtype=F32)
    tab, st = nan_table(4, 8, step or 0, row, dev), step_tensor(step, dev)
    nz = None if noise is None else nan_table(4, n, step or 0, noise, dev)

    def go():
        wx, wm = Win(n, F32, dev, init=x), Win(n, F32, dev, init=m1)
        rc = lib().pcdm_dpmpp_step(eps_d.data_ptr(), int(cfg), g, wx.ptr, wm.ptr, ops._ptr(nz), tab.data_ptr(), 4, ops._ptr(st), None, n, ops._stream(eps_d))
        return rc, [wx, wm]

    rc, wins = launch(backend, go)
    tag = f"dpmpp_step[n={n} cfg={int(cfg)} step={step} noise={int(with_noise)}]"
    if rc != 0:
        fails.append(f"{tag}: refused ({rc})")
        return
    e0, e1 = split_eps(eps, n, cfg)
    val, mag = eval_both(dpmpp_ref, {"e0": e0, "e1": e1, "x": x, "m1": m1, "noise": noise}, list(row[:6]) + [0.0, 0.0, g])
    for name, w in zip(("x", "m1"), wins):
        fails += w.problems(f"{tag} {name}")
        judge("steps", f"{tag} {name}", w.get(), val[name], gamma(K_DPMPP[name]) * mag[name], fails)


def test_dpmpp_step(backend):
    fails = []
    for n in ns_for(backend):
        for cfg in (False, True):
            for step in (None, 0, 3):
                for noise in (False, True):
                    run_dpmpp(backend, n, cfg, step, noise, fails)
    assert not fails, "\n".join(fails)
    record(backend, "steps")


UNCLIP_C = (1.1875, -0.640625, 1.5, 0.4375, 0.5625, 0.21875, 1.25, -0.09375)   # {p_x, p_e, clip, c_x0, c_x, c_noise, out_scale, out_shift}


def unclip_inputs(n, c):
    """x with entries whose x0 lands exactly on +-clip and one ulp to either side of it (p_x = 1, p_e = 0 rows use them)"""
    x = rnd(91 + n, n, scale=2.0)
    clip = float(c[2])
    if clip > 0 and float(c[0]) == 1.0 and float(c[1]) == 0.0:
        edge = torch.tensor([clip, -clip, clip, -clip, clip, -clip], dtype=F32).view(torch.int32) + torch.tensor([0, 0, 1, 1, -1, -1], dtype=torch.int32)
        x[:min(n, 6)] = edge.view(F32)[:min(n, 6)]
    return x


def run_unclip(backend, n, cfg, c, with_noise, dev_step, fails, g=4.0, alias=False):
    """``dev_step`` None: pcdm_unclip_step (host coefficients); an int: pcdm_unclip_step_dev with that *step_dev"""
    dev = backend.device
    eps, eps_d = eps_pair(90 + n, n, cfg, dev)
    c = torch.tensor(c, dtype=F32)
    x = unclip_inputs(n, c)
    noise = rnd(92 + n, n) if with_noise else None
    final = dev_step is not None and float(c[5]) == 0.0      # the final step: its slab must not be read
    if dev_step is not None:
        tab, st = nan_table(4, 8, dev_step, c, dev), step_tensor(dev_step, dev)
        nz = None if noise is None else nan_table(4, n, dev_step, torch.full((n,), float("nan")) if final else noise, dev)
    else:
        c8 = (C.c_float * 8)(*[float(v) for v in c])
        x_d, nz = x.to(dev), (None if noise is None else noise.to(dev))

    def go():
        if dev_step is not None:
            wx = Win(n, F32, dev, init=x)
            rc = lib().pcdm_unclip_step_dev(eps_d.data_ptr(), int(cfg), g, wx.ptr, ops._ptr(nz), tab.data_ptr(), 4, st.data_ptr(), None, n,
                                              ops._stream(eps_d))
        else:
            wx = Win(n, F32, dev, init=x) if alias else Win(n, F32, dev)
            rc = lib().pcdm_unclip_step(eps_d.data_ptr(), int(cfg), g, wx.ptr if alias else x_d.data_ptr(), ops._ptr(nz), wx.ptr, c8, n,
                                        ops._stream(eps_d))
        return rc, [wx]

    rc, wins = launch(backend, go)
    tag = f"unclip_step{'_dev' if dev_step is not None else ''}[n={n} cfg={int(cfg)} c={[float(v) for v in c]} noise={int(with_noise)} step={dev_step} alias={int(alias)}]"
    if rc != 0:
        fails.append(f"{tag}: refused ({rc})")
        return
    e0, e1 = split_eps(eps, n, cfg)
    val, mag = eval_both(unclip_ref, {"e0": e0, "e1": e1, "x": x, "noise": None if final else noise}, list(c) + [g])
    fails += wins[0].problems(tag)
    judge("steps", tag, wins[0].get(), val["x"], gamma(K_UNCLIP["x"]) * mag["x"], fails)


def unclip_variants():
    on = UNCLIP_C
    off = on[:2] + (0.0,) + on[3:]
    edge = (1.0, 0.0, 1.5) + on[3:]                              # x0 = x exactly: values at +-clip and one ulp beside it
    nonoise = on[:5] + (0.0,) + on[6:]                           # c_noise == 0: the final step
    return on, off, edge, nonoise


def test_unclip_step(backend):
    fails = []
    on, off, edge, nonoise = unclip_variants()
    for n in ns_for(backend):
        for cfg in (False, True):
            for c in (on, off, edge):
                for noise in (False, True):
                    run_unclip(backend, n, cfg, c, noise, None, fails)
        run_unclip(backend, n, True, on, True, None, fails, alias=True)     # pcdm.h: x_prev may alias x
    assert not fails, "\n".join(fails)
    record(backend, "steps")


def test_unclip_step_dev(backend):
    fails = []
    on, off, edge, nonoise = unclip_variants()
    for n in ns_for(backend):
        for cfg in (False, True):
            for step in (0, 3):
                for c in (on, off, edge):
                    for noise in (False, True):
                        run_unclip(backend, n, cfg, c, noise, step, fails)
                run_unclip(backend, n, cfg, nonoise, True, step, fails)    # c[5] == 0 while the slab holds NaN
    assert not fails, "\n".join(fails)
    record(backend, "steps")


LIN_C = (0.75, -1.3125, 0.40625, 2.5, -0.15625, 0.9375)


def run_lincomb(backend, n, nin, fails, expect=0):
    dev = backend.device
    xs = [rnd(100 + 3 * j + n, n, scale=1.0 + j) for j in range(max(nin, 1))]
    xs_d = [t.to(dev) for t in xs]
    ptrs = (C.c_void_p * max(nin, 1))(*[t.data_ptr() for t in xs_d])
    cs = (C.c_float * 7)(*(LIN_C + (1.0,)))

    def go():
        y = Win(n, F32, dev)
        return lib().pcdm_lincomb(y.ptr, nin, ptrs, cs, n, ops._stream(xs_d[0])), [y]

    rc, wins = launch(backend, go)
    tag = f"lincomb[n={n} nin={nin}]"
    if expect:
        if rc != expect or not wins[0].untouched():
            fails.append(f"{tag}: rc {rc} (expected {expect}), output untouched: {wins[0].untouched()}")
        return
    if rc != 0:
        fails.append(f"{tag}: refused ({rc})")
        return
    val = sum(float(torch.tensor(LIN_C[j], dtype=F32)) * xs[j].double() for j in range(nin))
    mag = sum(abs(LIN_C[j]) * xs[j].double().abs() for j in range(nin))
    fails += wins[0].problems(tag)
    judge("steps", tag, wins[0].get(), val, gamma(nin + 1) * mag, fails)


def test_lincomb(backend):
    fails = []
    for n in ns_for(backend):
        for nin in range(1, 7):
            run_lincomb(backend, n, nin, fails)
    run_lincomb(backend, 257, 0, fails, expect=-1)
    run_lincomb(backend, 257, 7, fails, expect=-1)
    assert not fails, "\n".join(fails)
    record(backend, "steps")


# ------------------------------------------------------------------------------------------------ (a) rescale_noise_cfg
def rescale_ref(a: torch.Tensor, b: torch.Tensor, gr: float):
    a, b = a.double(), b.double()
    factor = (b.std(dim=1, unbiased=True) / a.std(dim=1, unbiased=True)).view(-1, 1)
    grf = float(torch.tensor(gr, dtype=F32))
    return a * (grf * factor + (1.0 - grf)), 6.0 * U32 * a.abs() * (abs(grf) * factor + abs(1.0 - grf))


def run_rescale(backend, N, n, gr, fails, alias=False, mean=0.0, std=1.0):
    dev = backend.device
    a, b = rnd(110 + n + N, N, n, scale=std, mean=mean), rnd(111 + n + N, N, n, scale=0.7 * std, mean=-mean)
    a_d, b_d = a.to(dev), b.to(dev)

    def go():
        o = Win(N * n, F32, dev, init=a if alias else None)
        rc = lib().pcdm_rescale_noise_cfg(o.ptr if alias else a_d.data_ptr(), b_d.data_ptr(), o.ptr, N, n, gr, ops._stream(a_d))
        return rc, [o]

    rc, wins = launch(backend, go)
    tag = f"rescale_noise_cfg[N={N} n={n} gr={gr} alias={int(alias)} mean={mean}]"
    if rc != 0:
        fails.append(f"{tag}: refused ({rc})")
        return
    ref, bound = rescale_ref(a, b, gr)
    fails += wins[0].problems(tag)
    judge("rescale", tag, wins[0].get(), ref, bound, fails)


def test_rescale_noise_cfg(backend):
    fails = []
    for n in (2, 63, 352, 1023, 1024, 1025):
        for N in (1, 3):
            for gr in (0.0, 0.7, 1.0):
                run_rescale(backend, N, n, gr, fails)
        run_rescale(backend, 3, n, 0.7, fails, alias=True)
        if n > 2:
            run_rescale(backend, 3, n, 0.7, fails, mean=100.0, std=0.01)       # the single-pass fp64 variance under cancellation
    assert not fails, "\n".join(fails)
    record(backend, "rescale")


# ------------------------------------------------------------------------------------------------ (b) softmax_rows
SOFTMAX_COLS = (1, 2, 63, 64, 255, 256, 257, 300, 4097, 8191, 8192)
SM_SCALE = 0.09375               # with the rows shifted by 3e4: 4 u32 M = 0.25 u16


def softmax_ref(s: torch.Tensor, scale: float, c: float = C_SOFTMAX):
    z = s.double() * scale
    p = torch.softmax(z, dim=1)
    fin = torch.where(torch.isfinite(z), z.abs(), torch.zeros_like(z))
    M = fin.max(dim=1, keepdim=True).values * LOG2E
    return p, p * (U16 + 4.0 * U32 * (M + c)) + 2.0 ** -133


def softmax_rows_data(cols: int, seed: int = 0) -> torch.Tensor:
    """row 0: scores whose scaled spread is 3 (natural units); rows 1 / 2: the same law shifted by +-3e4"""
    s = rnd(120 + cols + seed, 3, cols, scale=3.0 / SM_SCALE)
    s[1] += 3e4
    s[2] -= 3e4
    return s


def run_softmax(backend, s: torch.Tensor, scale: float, ld_s: int, ld_p: int, fails, tag, exact=None):
    dev = backend.device
    rows, cols = s.shape
    sbuf = torch.full((rows, ld_s), float("nan"), dtype=F32)       # the padding of S must not be read
    sbuf[:, :cols] = s
    s_d = sbuf.to(dev)
    keep = torch.zeros(rows, ld_p, dtype=torch.bool)
    keep[:, cols:] = True

    def go():
        p = Win(rows * ld_p, BF16, dev)
        return lib().pcdm_softmax_rows(s_d.data_ptr(), p.ptr, rows, cols, ld_s, ld_p, scale, ops._stream(s_d)), [p]

    rc, wins = launch(backend, go)
    tag = f"softmax_rows[{tag} cols={cols} ld_s={ld_s} ld_p={ld_p}]"
    if rc != 0:
        fails.append(f"{tag}: refused ({rc})")
        return None
    fails += wins[0].problems(tag, keep=keep)
    out = wins[0].get().view(rows, ld_p)[:, :cols]
    ref, bound = softmax_ref(s, scale)
    judge("softmax", tag, out, ref, bound, fails)
    if exact is not None:
        exact(out, tag, fails)
    return out


@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_rows(backend, cols):
    fails = []
    run_softmax(backend, softmax_rows_data(cols), SM_SCALE, cols, cols, fails, "contiguous")
    run_softmax(backend, softmax_rows_data(cols, 1), SM_SCALE, cols + 5, cols + 3, fails, "padded")
    assert not fails, "\n".join(fails)
    record(backend, "softmax")


def test_softmax_rows_special_rows(backend):
    fails = []
    # one-hot: every other score 1000 natural units below
    s = torch.zeros(2, 300)
    s[0, 17], s[1, 299] = 1000.0, 1000.0

    def one_hot(out, tag, fails):
        want = torch.zeros(2, 300)
        want[0, 17], want[1, 299] = 1.0, 1.0
        if not torch.equal(out.float(), want):
            fails.append(f"{tag}: not exactly one-hot")
    run_softmax(backend, s, 1.0, 300, 300, fails, "one-hot", exact=one_hot)

    # a constant row of 256 columns: exp2(0) = 1 summed 256 times, the reciprocal and the store are exact
    def const(out, tag, fails):
        if not bool((out.float() == 2.0 ** -8).all()):
            fails.append(f"{tag}: a constant row of 256 is not exactly 2^-8 everywhere")
    run_softmax(backend, torch.full((2, 256), -3.25), 0.5, 256, 264, fails, "constant", exact=const)

    # -inf entries: exactly 0, the rest of the row inside the bound
    s = softmax_rows_data(257)
    holes = torch.zeros(3, 257, dtype=torch.bool)
    holes[:, ::3] = True
    holes[1, :200] = True
    s[holes] = float("-inf")

    def zeros(out, tag, fails):
        if not bool((out.float()[holes] == 0).all()):
            fails.append(f"{tag}: a -inf score did not give exactly 0")
    run_softmax(backend, s, SM_SCALE, 260, 257, fails, "-inf entries", exact=zeros)
    assert not fails, "\n".join(fails)
    record(backend, "softmax")


def test_softmax_rows_refusals(backend):
    dev = backend.device
    s_d = torch.zeros(2 * 8200, dtype=F32, device=dev)
    for cols, ld_s, ld_p, rows, what in ((8193, 8200, 8200, 2, "cols > 8192"), (300, 299, 300, 2, "ld_s < cols"), (300, 300, 299, 2, "ld_p < cols"),
                                         (0, 8, 8, 2, "cols < 1"), (8, 8, 8, 0, "rows < 1")):
        p = Win(2 * 8200, BF16, dev)
        rc = lib().pcdm_softmax_rows(s_d.data_ptr(), p.ptr, rows, cols, ld_s, ld_p, 1.0, ops._stream(s_d))
        backend.sync()
        assert rc == -1 and p.untouched(), f"softmax_rows {what}: rc {rc}, output untouched {p.untouched()}"
    p = Win(64, BF16, dev)
    assert lib().pcdm_softmax_rows(None, p.ptr, 2, 8, 8, 8, 1.0, ops._stream(s_d)) == -1 and p.untouched()
    assert lib().pcdm_softmax_rows(s_d.data_ptr(), None, 2, 8, 8, 8, 1.0, ops._stream(s_d)) == -1


# ------------------------------------------------------------------------------------------------ (c) small_linear
def silu64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    return x / (1.0 + torch.exp(-x))


def measure_unary(backend, xs: torch.Tensor, kind: str) -> torch.Tensor:
    """the device's silu_f (through pcdm_small_linear with one-hot weights of 1.0: y[b, n] = silu_f(x[b, n]) exactly -- every other product
    is a finite number times zero) or __expf(0.5 lv) (through pcdm_gaussian_sample with mean 0, noise 1, scale 1) of every element of xs"""
    dev = backend.device
    if kind == "expf":
        n = xs.numel()
        mom = torch.cat([torch.zeros(n), xs.float()]).to(dev)
        noise, out = torch.ones(n, device=dev), Win(n, F32, dev)
        assert lib().pcdm_gaussian_sample(mom.data_ptr(), noise.data_ptr(), out.ptr, 1, 1, n, 1.0, ops._stream(mom)) == 0
        backend.sync()
        assert not out.problems("expf sweep")
        return out.get()
    pad = (-xs.numel()) % 256
    x = torch.cat([xs.float(), torch.zeros(pad)]).view(-1, 32, 8)
    w = torch.eye(8).to(BF16).to(dev)
    got = []
    for blk in x:
        x_d, y = blk.contiguous().to(dev), Win(256, F32, dev)
        assert lib().pcdm_small_linear(x_d.data_ptr(), w.data_ptr(), None, None, y.ptr, 32, 8, 8, 1, 0, ops._stream(x_d)) == 0
        backend.sync()
        assert not y.problems("silu sweep")
        got.append(y.get())
    return torch.cat(got)[:xs.numel()]


def silu_sweep() -> torch.Tensor:
    g = torch.Generator().manual_seed(5)
    return torch.cat([torch.linspace(-100.0, 100.0, 6401), torch.linspace(-2.0, 2.0, 1025), (torch.rand(2048, generator=g) - 0.5) * 200.0,
                      torch.tensor([88.0, -88.0, -100.0, 100.0, 87.5, -87.5, 0.0, -0.0, 1e-20, -1e-20])]).float()


def test_measure_silu(backend):
    """the relative error of silu_f where |silu| >= 1e-30, measured through pcdm_small_linear; below that the floor holds; C_SILU covers it twice"""
    xs = silu_sweep()
    got, ref = measure_unary(backend, xs, "silu").double(), silu64(xs)
    assert bool(torch.isfinite(got).all())
    big = ref.abs() >= 1e-30
    rel = float(((got - ref).abs()[big] / ref.abs()[big]).max())
    floor = float((got - ref).abs()[~big].max())
    print(f"silu_f: largest relative error {rel:.4g} ({rel / U32:.2f} u32) at x = {float(xs[big][((got - ref).abs()[big] / ref.abs()[big]).argmax()]):.6g}; "
          f"below 1e-30: {floor:.3g} absolute [{backend.name}]")
    assert floor <= SILU_FLOOR, floor
    assert 2.0 * rel <= C_SILU, f"C_SILU = {C_SILU:.3g} is not twice the measurement {rel:.4g}"
    if not backend.is_emu:
        from tests import parity_record
        parity_record.check("small_ops/silu_rel", rel, C_SILU / 2.0)


LIN_B, LIN_K, LIN_N = (1, 7, 8, 9, 17, 32), (8, 504, 512, 520, 1280), (1, 3, 4, 5, 40)
LIN_VARIANTS = tuple((ai, ao, hb, ha) for ai in (0, 1) for ao in (0, 1, 2) for hb in (False, True) for ha in (False, True))   # 24


def small_linear_ref(x, w, bias, add, act_in, act_out):
    """fp64 value and bound of y [B, N] from fp32 x [B, K], bf16 w [N, K], fp32 bias [N] / add [B, N]"""
    K = x.shape[1]
    a = silu64(x) if act_in else x.double()
    wd = w.double()
    v = a @ wd.t()
    mag = a.abs() @ wd.abs().t()
    err = torch.zeros_like(v)
    if act_in:
        err = C_SILU * mag + SILU_FLOOR * wd.abs().sum(dim=1).view(1, -1)
    if bias is not None:
        v, mag = v + bias.double().view(1, -1), mag + bias.double().abs().view(1, -1)
    if add is not None and act_out != 1:
        v, mag = v + add.double(), mag + add.double().abs()
    err = err + (K / 64 + 16) * U32 * mag
    if act_out:
        err = 1.1 * err + C_SILU * silu64(v).abs() + SILU_FLOOR
        v = silu64(v)
        if add is not None and act_out == 1:       # the add behind the activation: one rounding of the sum
            err = err + U32 * (v.abs() + add.double().abs())
            v = v + add.double()
    return v, err


def small_linear_operands(B, K, N, seed=0):
    x = rnd(130 + B + K + N + seed, B, K, scale=2.0)
    x[0, 0] = -90.0                                   # a SiLU argument where __expf is large (act_in) -- |silu| ~ 7e-38, the floor's range
    w = rnd(131 + B + K + N + seed, N, K, scale=0.5).to(BF16)
    return x, w, rnd(132 + N + seed, N), rnd(133 + B + N + seed, B, N, scale=1.5)


def run_small_linear(backend, B, K, N, variant, fails):
    dev = backend.device
    act_in, act_out, has_bias, has_add = variant
    x, w, bias, add = small_linear_operands(B, K, N)
    bias, add = (bias if has_bias else None), (add if has_add else None)
    x_d, w_d = x.to(dev), w.to(dev)
    b_d, a_d = (None if bias is None else bias.to(dev)), (None if add is None else add.to(dev))

    def go():
        y = Win(B * N, F32, dev)
        rc = lib().pcdm_small_linear(x_d.data_ptr(), w_d.data_ptr(), ops._ptr(b_d), ops._ptr(a_d), y.ptr, B, K, N, act_in, act_out, ops._stream(x_d))
        return rc, [y]

    rc, wins = launch(backend, go)
    tag = f"small_linear[B={B} K={K} N={N} act_in={act_in} act_out={act_out} bias={int(has_bias)} add={int(has_add)}]"
    if rc != 0:
        fails.append(f"{tag}: refused ({rc})")
        return
    ref, bound = small_linear_ref(x, w, bias, add, act_in, act_out)
    fails += wins[0].problems(tag)
    judge("small_linear", tag, wins[0].get(), ref, bound, fails)


@pytest.mark.parametrize("B", LIN_B)
def test_small_linear(backend, B):
    """every (B, K, N) of the grid, the 24 (act_in, act_out, bias, add) variants dealt over them in turn -- and all 24 at one K per B"""
    fails, i = [], LIN_B.index(B) * 5
    for K in LIN_K:
        for N in LIN_N:
            run_small_linear(backend, B, K, N, LIN_VARIANTS[i % 24], fails)
            i += 7                                    # (7 is coprime to 24: the 25 shapes of a B meet every variant)
    K = LIN_K[LIN_B.index(B) % len(LIN_K)]
    for v in LIN_VARIANTS:
        run_small_linear(backend, B, K, 5, v, fails)
    assert not fails, "\n".join(fails)
    record(backend, "small_linear")


def test_small_linear_refusals(backend):
    dev = backend.device
    x, w = torch.zeros(33 * 16, device=dev), torch.zeros(8 * 16, dtype=BF16, device=dev)
    for B, K, N, what in ((33, 8, 4, "B > 32"), (0, 8, 4, "B < 1"), (4, 12, 4, "K % 8"), (4, 4, 4, "K % 8 (K < 8)"), (4, 0, 4, "K < 1"), (4, 8, 0, "N < 1")):
        y = Win(33 * 8, F32, dev)
        rc = lib().pcdm_small_linear(x.data_ptr(), w.data_ptr(), None, None, y.ptr, B, K, N, 0, 0, ops._stream(x))
        backend.sync()
        assert rc == -1 and y.untouched(), f"small_linear {what}: rc {rc}"
    y = Win(64, F32, dev)
    assert lib().pcdm_small_linear(None, w.data_ptr(), None, None, y.ptr, 4, 8, 4, 0, 0, ops._stream(x)) == -1
    assert lib().pcdm_small_linear(x.data_ptr(), None, None, None, y.ptr, 4, 8, 4, 0, 0, ops._stream(x)) == -1
    assert lib().pcdm_small_linear(x.data_ptr(), w.data_ptr(), None, None, None, 4, 8, 4, 0, 0, ops._stream(x)) == -1
    backend.sync()
    assert y.untouched()


# ------------------------------------------------------------------------------------------------ (d) timestep embedding
T_VALUES = (0, 1, 500, 981, 999)
LN1E4 = math.log(10000.0)


def timestep_ref(t, dim: int, flip: bool, shift: float, wrong_half: bool = False):
    """fp64 [len(t), dim] and the bound"""
    half = dim // 2
    k = torch.arange(half, dtype=torch.float64)
    f = torch.exp(-LN1E4 * k / (half - (0.0 if wrong_half else shift)))
    a = torch.tensor(t, dtype=torch.float64).view(-1, 1) * f.view(1, -1)
    s, c = torch.sin(a), torch.cos(a)
    bound = a.abs() * 4.0 * U32 * (1.0 + LN1E4) + 2.0 * U32
    return (torch.cat([c, s], 1) if flip else torch.cat([s, c], 1)), torch.cat([bound, bound], 1)


@pytest.mark.parametrize("dim", (64, 320))
def test_timestep_embedding(backend, dim):
    from oracle.unet import timestep_embedding as oracle_embedding
    dev, fails, B = backend.device, [], 3
    table = torch.tensor(T_VALUES, dtype=torch.int64)
    for flip in (0, 1):
        for shift in (0.0, 1.0):
            ref, bound = timestep_ref(list(T_VALUES), dim, bool(flip), shift)
            # (the bound is one on fp32 evaluation of the formula: torch's own meets it)
            nviol, worst, _ = compare(oracle_embedding(table, dim, bool(flip), shift), ref, bound)
            assert nviol == 0, f"the oracle's fp32 timestep_embedding misses the bound: err / bound {worst:.3g}"
            for idx, t in enumerate(T_VALUES):
                for use_step in (False, True):
                    # step_dev NULL reads t_dev[0]; an index reads that entry of a table whose other entries are far away
                    tt = torch.full((5,), 123456, dtype=torch.int64)
                    tt[idx if use_step else 0] = t
                    t_d, st = tt.to(dev), (step_tensor(idx, dev) if use_step else None)

                    def go():
                        o = Win(B * dim, F32, dev)
                        return lib().pcdm_timestep_embedding(t_d.data_ptr(), 5, ops._ptr(st), None, o.ptr, B, dim, flip, shift, ops._stream(t_d)), [o]

                    rc, wins = launch(backend, go)
                    tag = f"timestep_embedding[t={t} dim={dim} flip={flip} shift={shift} step={'index' if use_step else 'NULL'}]"
                    assert rc == 0, tag
                    fails += wins[0].problems(tag)
                    out = wins[0].get().view(B, dim)
                    if not all(torch.equal(out[0].view(torch.int32), out[b].view(torch.int32)) for b in range(1, B)):
                        fails.append(f"{tag}: the B rows differ")
                    judge("timestep", tag, out[0], ref[idx], bound[idx], fails)
            # the table form: row i <- t_dev[i]
            t_d = table.to(dev)

            def go_rows():
                o = Win(5 * dim, F32, dev)
                return lib().pcdm_timestep_embedding_rows(t_d.data_ptr(), 5, o.ptr, dim, flip, shift, ops._stream(t_d)), [o]

            rc, wins = launch(backend, go_rows)
            tag = f"timestep_embedding_rows[dim={dim} flip={flip} shift={shift}]"
            assert rc == 0, tag
            fails += wins[0].problems(tag)
            judge("timestep", tag, wins[0].get().view(5, dim), ref, bound, fails)
    assert not fails, "\n".join(fails)
    record(backend, "timestep")


# ------------------------------------------------------------------------------------------------ (e) exact kernels
def bits16(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def test_layout_kernels_exact(backend):
    dev, fails = backend.device, []
    B, HW = 2, 37
    for Cc, Cpad in ((3, 8), (9, 16)):
        x = rnd(140 + Cc, B, Cc, HW, scale=3.0)
        x_d = x.to(dev)

        def go():
            y = Win(B * HW * Cpad, BF16, dev)
            return lib().pcdm_nchw_f32_to_nhwc_bf16(x_d.data_ptr(), y.ptr, B, Cc, Cpad, HW, ops._stream(x_d)), [y]

        rc, wins = launch(backend, go)
        tag = f"nchw_f32_to_nhwc_bf16[C={Cc} Cpad={Cpad}]"
        assert rc == 0, tag
        fails += wins[0].problems(tag)
        want = torch.zeros(B, HW, Cpad, dtype=BF16)
        want[:, :, :Cc] = x.permute(0, 2, 1).to(BF16)
        if not torch.equal(bits16(wins[0].get()), bits16(want).reshape(-1)):       # (bits: the padding is +0, not -0)
            fails.append(f"{tag}: differs from the RNE cast / the padded channels are not exactly zero")
        # and back, from a source whose every element is its own value
        src = (torch.arange(B * HW * Cc, dtype=F32) * 0.25 - 40.0).to(BF16).view(B, HW, Cc)
        s_d = src.to(dev)

        def go_back():
            y = Win(B * Cc * HW, F32, dev)
            return lib().pcdm_nhwc_bf16_to_nchw_f32(s_d.data_ptr(), y.ptr, B, Cc, HW, ops._stream(s_d)), [y]

        rc, wins = launch(backend, go_back)
        tag = f"nhwc_bf16_to_nchw_f32[C={Cc}]"
        assert rc == 0, tag
        fails += wins[0].problems(tag)
        if not torch.equal(wins[0].get().view(B, Cc, HW), src.float().permute(0, 2, 1)):
            fails.append(f"{tag}: not the transposed widening")
    assert not fails, "\n".join(fails)


def _from_bits(bits) -> torch.Tensor:
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(F32)


def bf16_specials() -> torch.Tensor:
    bits = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000,      # ties (to even: down, up), just above, just below
            0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0xFF7FFFFF,                              # overflow to inf by rounding, the largest that does not
            0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00800000, 0x80800000,      # inf, zeros, the smallest normals
            0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FA5A5A5]                              # NaNs (quiet, payload, signalling)
    return _from_bits(bits)


def bf16_subnormals() -> torch.Tensor:
    bits = [0x00000001, 0x00008000, 0x00010000, 0x00018000, 0x007FFFFF, 0x007F8000, 0x80010000, 0x807FFFFF, 0x00400000, 0x80400000]
    return _from_bits(bits)


def test_f32_to_bf16_exact(backend):
    dev, fails = backend.device, []
    for n in ns_for(backend):
        spec, sub = bf16_specials(), bf16_subnormals()
        x = rnd(150 + n, n, scale=100.0)
        k = min(n, spec.numel())
        x[:k] = spec[:k]
        if n >= 256:
            x[100:100 + sub.numel()] = sub
        x_d = x.to(dev)

        def go():
            y = Win(n, BF16, dev)
            return lib().pcdm_f32_to_bf16(x_d.data_ptr(), y.ptr, n, ops._stream(x_d)), [y]

        rc, wins = launch(backend, go)
        tag = f"f32_to_bf16[n={n}]"
        assert rc == 0, tag
        fails += wins[0].problems(tag)
        got, want = wins[0].get(), x.to(BF16)
        nan = torch.isnan(x)
        if not torch.equal(torch.isnan(got.float()), nan):
            fails.append(f"{tag}: NaN in does not give NaN out (or the reverse)")
        subn = (x != 0) & (x.abs() < 2.0 ** -126)
        same = bits16(got) == bits16(want)
        signed_zero = (got.float() == 0) & (torch.signbit(got.float()) == torch.signbit(x))
        ok = nan | same | (subn & signed_zero)
        if not bool(ok.all()):
            i = int((~ok).nonzero()[0])
            fails.append(f"{tag}: {int((~ok).sum())} elements differ from the RNE cast, first x = {float(x[i])!r} ({int(x.view(torch.int32)[i]) & 0xFFFFFFFF:#010x}): "
                         f"{int(bits16(got)[i]) & 0xFFFF:#06x} for {int(bits16(want)[i]) & 0xFFFF:#06x}")
        if n >= 256:
            flushed = bool((subn & ~same).any())
            print(f"{tag}: fp32 subnormals are {'flushed to a signed zero' if flushed else 'converted as torch converts them (RNE, bf16 subnormals)'} [{backend.name}]")
            if not backend.is_emu and n == 256:       # (recorded on the MI355X: 0 -- v_cvt_pk_bf16_f32 rounds them as torch does)
                from tests import parity_record
                parity_record.check("small_ops/f32_to_bf16_subnormals_flushed", 1.0 if flushed else 0.0, 1.0)
    assert not fails, "\n".join(fails)


def test_assemble_input_exact(backend):
    dev, fails = backend.device, []
    N, rep, h, w = 2, 2, 3, 5
    HW, Bout = h * w, N * rep
    lat = rnd(160, N, 4, HW, scale=2.0)
    for with_mask in (True, False):
        for mb in (1, Bout):
            for cpad in (16, 64):
                mask, masked = rnd(161 + mb, mb, 1, HW), rnd(162 + mb, mb, 4, HW, scale=1.5)
                l_d, m_d, k_d = lat.to(dev), mask.to(dev), masked.to(dev)

                def go():
                    o = Win(Bout * HW * cpad, BF16, dev)
                    rc = lib().pcdm_assemble_input(l_d.data_ptr(), N, rep, m_d.data_ptr() if with_mask else None, mb, k_d.data_ptr(), mb, o.ptr, h, w, cpad,
                                                   ops._stream(l_d))
                    return rc, [o]

                rc, wins = launch(backend, go)
                tag = f"assemble_input[mask={int(with_mask)} mask_b=masked_b={mb} cpad={cpad}]"
                assert rc == 0, tag
                fails += wins[0].problems(tag)
                parts = [lat.repeat(rep, 1, 1)] + ([mask.expand(Bout, 1, HW)] if with_mask else []) + [masked.expand(Bout, 4, HW)]
                cat = torch.cat(parts, 1)
                want = torch.zeros(Bout, HW, cpad, dtype=BF16)
                want[:, :, :cat.shape[1]] = cat.permute(0, 2, 1).to(BF16)
                if not torch.equal(bits16(wins[0].get()), bits16(want).reshape(-1)):
                    fails.append(f"{tag}: differs from the concatenation / the padding is not exactly zero")
    assert not fails, "\n".join(fails)


def test_pixel_shuffle2_exact(backend):
    dev, fails = backend.device, []
    B, H, W = 2, 3, 5
    for Cc in (8, 24):
        n = B * H * W * 4 * Cc
        src = torch.arange(n, dtype=torch.int32).to(torch.int16)          # every element names its own index (n < 2^15)
        assert n < 2 ** 15
        s_d = src.to(dev)

        def go():
            o = Win(n, BF16, dev)
            return lib().pcdm_pixel_shuffle2(s_d.data_ptr(), o.ptr, B, H, W, Cc, ops._stream(s_d)), [o]

        rc, wins = launch(backend, go)
        tag = f"pixel_shuffle2[C={Cc}]"
        assert rc == 0, tag
        fails += wins[0].problems(tag)
        # out[b, 2y + a, 2x + bb, c] = in[(b, y, x), (2a + bb) C + c]
        want = src.view(B, H, W, 2, 2, Cc).permute(0, 1, 3, 2, 4, 5).reshape(-1)
        if not torch.equal(bits16(wins[0].get()), want):
            fails.append(f"{tag}: not the documented permutation")
    assert not fails, "\n".join(fails)


def test_time_class_combine(backend):
    dev, fails = backend.device, []
    n, B = 3, 2
    for D in (5, 64):
        for with_cls in (False, True):
            emb, cls = rnd(170 + D, n, D, scale=3.0), rnd(171 + D, B, D, scale=2.0)
            emb[0, 0] = -80.0
            e_d, c_d = emb.to(dev), cls.to(dev)

            def go():
                o = Win(n * B * D, BF16, dev)
                return lib().pcdm_time_class_combine(e_d.data_ptr(), c_d.data_ptr() if with_cls else None, o.ptr, n, B, D, ops._stream(e_d)), [o]

            rc, wins = launch(backend, go)
            tag = f"time_class_combine[D={D} cls={int(with_cls)}]"
            assert rc == 0, tag
            fails += wins[0].problems(tag)
            v = emb.double().view(n, 1, D) + (cls.double().view(1, B, D) if with_cls else torch.zeros(1, B, D, dtype=torch.float64))
            mag = emb.double().abs().view(n, 1, D) + (cls.double().abs().view(1, B, D) if with_cls else 0.0)
            ref = silu64(v)
            bound = U16 * ref.abs() + C_SILU * ref.abs() + SILU_FLOOR + 1.1 * U32 * mag * (1.0 if with_cls else 0.0) + 2.0 ** -133
            judge("time_class_combine", tag, wins[0].get().view(n, B, D), ref, bound, fails)
    assert not fails, "\n".join(fails)
    record(backend, "time_class_combine")


def test_image_to_uint8_exact(backend):
    dev, fails = backend.device, []
    sweep = torch.cat([torch.linspace(-1.2, 1.2, 4001), torch.tensor([float("inf"), float("-inf"), 1.0, -1.0, 0.0])]).float()
    HW = sweep.numel()
    for cstride in (3, 4):
        B = 2
        x = torch.full((B, cstride, HW), float("nan"))                  # a fourth channel must not be read
        for b in range(B):
            for c in range(3):
                x[b, c] = sweep.roll(37 * (3 * b + c))
        x_d = x.to(dev)

        def go():
            o = Win(B * HW * 3, U8, dev)
            return lib().pcdm_image_to_uint8(x_d.data_ptr(), o.ptr, B, cstride, HW, ops._stream(x_d)), [o]

        rc, wins = launch(backend, go)
        tag = f"image_to_uint8[cstride={cstride}]"
        assert rc == 0, tag
        got = wins[0].get().view(B, HW, 3)
        want = (x[:, :3] * 0.5 + 0.5).clamp(0, 1).mul(255).round().permute(0, 2, 1).to(U8)
        # (0x55 = 85 is a legitimate pixel: the never-written check is the comparison itself)
        b = wins[0].bits()
        if not bool((b[:GUARD] == 0x55).all() and (b[GUARD + wins[0].n:] == 0x55).all()):
            fails.append(f"{tag}: written outside its window")
        if not torch.equal(got, want):
            fails.append(f"{tag}: {int((got != want).sum())} of {want.numel()} bytes differ from fp32 (x * 0.5 + 0.5).clamp(0, 1).mul(255).round()")
    assert not fails, "\n".join(fails)


def test_measure_expf(backend):
    """the relative error of __expf(0.5 lv) over the clamp range, measured through pcdm_gaussian_sample; C_EXPF covers it twice"""
    lv = torch.cat([torch.linspace(-30.0, 20.0, 16385), torch.tensor([-30.0, -29.99, 0.0, 19.99, 20.0])]).float()
    got, ref = measure_unary(backend, lv, "expf").double(), torch.exp(0.5 * lv.double())
    rel = float(((got - ref).abs() / ref).max())
    print(f"__expf(0.5 lv): largest relative error {rel:.4g} ({rel / U32:.2f} u32) at lv = {float(lv[((got - ref).abs() / ref).argmax()]):.6g} [{backend.name}]")
    assert 2.0 * rel <= C_EXPF, f"C_EXPF = {C_EXPF:.3g} is not twice the measurement {rel:.4g}"
    if not backend.is_emu:
        from tests import parity_record
        parity_record.check("small_ops/expf_rel", rel, C_EXPF / 2.0)


def test_gaussian_sample(backend):
    dev, fails = backend.device, []
    B, zc, HW, scale = 2, 4, 37, 0.18215
    scale32 = float(torch.tensor(scale, dtype=F32))
    mean, lv, z = rnd(180, B, zc, HW, scale=2.0), rnd(181, B, zc, HW, scale=6.0), rnd(182, B, zc, HW)
    edges = torch.tensor([-40.0, -30.0, -29.99, 0.0, 19.99, 20.0, 25.0])
    lv[0, 0, :7], lv[1, 3, -7:] = edges, edges
    mom = torch.cat([mean, lv], 1).contiguous()
    m_d, z_d = mom.to(dev), z.to(dev)
    for with_noise in (True, False):
        def go():
            o = Win(B * zc * HW, F32, dev)
            return lib().pcdm_gaussian_sample(m_d.data_ptr(), z_d.data_ptr() if with_noise else None, o.ptr, B, zc, HW, scale, ops._stream(m_d)), [o]

        rc, wins = launch(backend, go)
        tag = f"gaussian_sample[noise={int(with_noise)}]"
        assert rc == 0, tag
        fails += wins[0].problems(tag)
        got = wins[0].get().view(B, zc, HW)
        if not with_noise:                              # mean * scale exactly (one fp32 product; e * 0 = 0 is exact)
            if not torch.equal(got, mean * torch.tensor(scale, dtype=F32)):
                fails.append(f"{tag}: not mean * scale bit for bit")
            continue
        e = torch.exp(0.5 * lv.double().clamp(-30.0, 20.0))
        ref = (mean.double() + e * z.double()) * scale32
        bound = (3.0 * U32 * (mean.double().abs() + e * z.double().abs()) + C_EXPF * e * z.double().abs()) * abs(scale32)
        judge("gaussian_sample", tag, got, ref, bound, fails)
    assert not fails, "\n".join(fails)
    record(backend, "gaussian_sample")


# ------------------------------------------------------------------------------------------------ (f) quantize_fp8
def fp8_decode(b: torch.Tensor) -> torch.Tensor:
    return b.cpu().contiguous().view(torch.float8_e4m3fn).float()


def fp8_ref(x: torch.Tensor, scale: float) -> torch.Tensor:
    """torch's RNE cast of clamp(fp32(bf16 * scale), +-448), decoded; NaN stays NaN"""
    return (x.float() * torch.tensor(scale, dtype=F32)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()


def fp8_specials() -> torch.Tensor:
    v = [0.0, -0.0, 2.0 ** -10, -(2.0 ** -10), 2.0 ** -10 * 1.0078125, 2.0 ** -10 * 0.9921875, 2.0 ** -9, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -11, 2.0 ** -6,
         2.0 ** -6 * 0.9375, 2.0 ** -6 * 0.96875, 1.0, 1.0625, 1.1875, 1.0703125, 1.0546875, -1.0625, -1.1875, 240.0, 416.0, 432.0, 448.0, 464.0, 480.0, -464.0,
         1e5, -1e5, float("inf"), float("-inf"), 3.0e38, 17.0, 18.0, 19.0, 0.3, -0.7]
    return torch.tensor(v, dtype=F32).to(BF16)


def run_quantize(backend, x2d: torch.Tensor, cols, cols_pad, ldy, scale, fails, tag, x_offset=0):
    """x2d: a bf16 [rows, ldx] host tensor (the kernel reads columns < cols); ``x_offset``: the device copy starts that many ELEMENTS behind a
    16-byte aligned address"""
    dev = backend.device
    rows, ldx = x2d.shape
    x2d = x2d.clone()
    x2d[:, cols:] = float("nan")                      # columns the kernel must not read: a NaN would show in the padding bytes
    flat = torch.full((rows * ldx + x_offset + 8,), float("nan"), dtype=BF16)
    flat[x_offset:x_offset + rows * ldx] = x2d.reshape(-1)
    x_d = flat.to(dev)
    assert x_d.data_ptr() % 16 == 0
    keep = torch.zeros(rows, ldy, dtype=torch.bool)
    keep[:, cols_pad:] = True

    def go():
        y = Win(rows * ldy, U8, dev)
        rc = lib().pcdm_quantize_fp8(x_d.data_ptr() + 2 * x_offset, y.ptr, rows, cols, cols_pad, ldx, ldy, scale, ops._stream(x_d))
        return rc, [y]

    rc, wins = launch(backend, go)
    tag = f"quantize_fp8[{tag} rows={rows} cols={cols} cols_pad={cols_pad} ldx={ldx} ldy={ldy} x offset={x_offset}]"
    if rc != 0:
        fails.append(f"{tag}: refused ({rc})")
        return None
    y = wins[0]
    b = y.bits()
    if not bool((b[:GUARD] == 0x55).all() and (b[GUARD + y.n:] == 0x55).all()):
        fails.append(f"{tag}: written outside its window")
    got = y.get().view(rows, ldy)
    if not bool((got[:, cols_pad:] == 0x55).all()):
        fails.append(f"{tag}: bytes behind cols_pad written")
    if not bool((got[:, cols:cols_pad] == 0).all()):
        fails.append(f"{tag}: the padding bytes [cols, cols_pad) are not exactly 0")
    dec, ref = fp8_decode(got[:, :cols]), fp8_ref(x2d[:, :cols], scale)
    nan = torch.isnan(ref)
    if not torch.equal(torch.isnan(dec), nan):
        fails.append(f"{tag}: NaN in must give an e4m3 NaN byte (0x7f / 0xff) and nothing else may: bytes {sorted(set(got[:, :cols][nan].tolist()))} at the NaNs")
    diff = (dec != ref) & ~nan
    if bool(diff.any()):
        i = diff.nonzero()[0]
        fails.append(f"{tag}: {int(diff.sum())} decoded values differ from torch's float8_e4m3fn cast, first at {i.tolist()}: x = "
                     f"{float(x2d[i[0], i[1]])!r} -> {float(dec[i[0], i[1]])!r} for {float(ref[i[0], i[1]])!r}")
    return got


def fp8_matrix(rows: int, ldx: int, seed: int) -> torch.Tensor:
    x = rnd(190 + seed, rows, ldx, scale=40.0)
    x[:, ::7] *= 0.001                                # the subnormal range of e4m3
    x[:, 3::11] *= 20.0                               # saturation
    return x.to(BF16)


def test_quantize_fp8(backend):
    fails = []
    # cols % 8 != 0 with cols_pad, more than one block (rows * cols_pad / 8 > 256), ldy > cols_pad, a scale that is no power of two
    for cols, cols_pad, ldx, ldy, rows in ((61, 64, 64, 64, 5), (61, 64, 61, 72, 5), (77, 80, 88, 96, 40), (8, 8, 8, 8, 1), (3, 16, 3, 16, 7), (64, 64, 64, 64, 33)):
        run_quantize(backend, fp8_matrix(rows, ldx, cols), cols, cols_pad, ldy, 0.7421875, fails, "random")
    # the vector path (ldx % 8 == 0) and the element path (odd ldx) give the same bytes
    x = fp8_matrix(9, 64, 1)
    a = run_quantize(backend, x, 61, 64, 64, 1.5, fails, "ldx 64")
    b = run_quantize(backend, x[:, :61].contiguous(), 61, 64, 64, 1.5, fails, "ldx 61")
    if a is not None and b is not None and not torch.equal(a, b):
        fails.append("quantize_fp8: ldx = 64 and ldx = 61 give different bytes for the same values")
    # specials, at scale 1 (and 0.5 / 2: exact scalings that move every value to another binade)
    sp = fp8_specials()
    xs = torch.zeros(2, 40, dtype=BF16)
    xs[0, :sp.numel()], xs[1, :sp.numel()] = sp, -sp
    for scale in (1.0, 0.5, 2.0):
        run_quantize(backend, xs, 37, 40, 40, scale, fails, f"specials scale={scale}")
    assert not fails, "\n".join(fails)


def test_quantize_fp8_nan(backend):
    """a NaN in K or V must stay a NaN in the fp8 operand (0x7f / 0xff), on the vector and on the element path"""
    fails = []
    for ldx in (64, 61):
        x = fp8_matrix(4, ldx, 2)
        x[0, 0], x[1, 13], x[2, 60], x[3, 31] = float("nan"), float("nan"), -float("nan"), float("nan")
        x.view(torch.int16)[3, 32] = 0xFFA5 - 0x10000      # a negative NaN with a payload
        run_quantize(backend, x, 61, 64, 64, 1.0, fails, "NaN")
    assert not fails, "\n".join(fails)


def test_quantize_fp8_unaligned_x(backend):
    """x three elements behind a 16-byte boundary: with ldx = 64 the rows look aligned by their stride alone -- the kernel must take the element
    path (pcdm.h: x needs only its natural alignment); the bytes equal those of the aligned copy"""
    fails = []
    for ldx in (64, 61):
        x = fp8_matrix(6, ldx, 3)
        a = run_quantize(backend, x, 61, 64, 64, 1.25, fails, "aligned", x_offset=0)
        b = run_quantize(backend, x, 61, 64, 64, 1.25, fails, "offset 3", x_offset=3)
        if a is not None and b is not None and not torch.equal(a, b):
            fails.append(f"quantize_fp8 ldx={ldx}: the view at element offset 3 gives other bytes than the aligned copy")
    assert not fails, "\n".join(fails)


def test_quantize_fp8_refusals(backend):
    dev = backend.device
    x = torch.zeros(4096, dtype=BF16, device=dev)
    good = dict(rows=4, cols=61, cols_pad=64, ldx=64, ldy=64, yoff=0)
    for over, what in ((dict(yoff=4), "y not 8-byte aligned"), (dict(yoff=1), "y odd"), (dict(rows=0), "rows < 1"), (dict(cols=0), "cols < 1"),
                       (dict(cols_pad=56), "cols_pad < cols"), (dict(cols_pad=68, ldy=72), "cols_pad % 8"), (dict(ldy=68), "ldy % 8"),
                       (dict(ldy=56), "ldy < cols_pad"), (dict(ldx=60), "ldx < cols"), (dict(x=None), "x NULL"), (dict(y=None), "y NULL")):
        a = dict(good, **over)
        y = Win(1024, U8, dev)
        rc = lib().pcdm_quantize_fp8(a.get("x", x.data_ptr()), a.get("y", y.ptr + a["yoff"]), a["rows"], a["cols"], a["cols_pad"], a["ldx"], a["ldy"], 1.0,
                                     ops._stream(x))
        backend.sync()
        assert rc == -1 and y.untouched(), f"quantize_fp8 {what}: rc {rc}, output untouched {y.untouched()}"
    y = Win(1024, U8, dev)
    assert lib().pcdm_quantize_fp8(x.data_ptr(), y.ptr, 4, 61, 64, 64, 64, 1.0, ops._stream(x)) == 0


# ------------------------------------------------------------------------------------------------ the bounds bite (CPU only, no kernel)
def _rounded(v: torch.Tensor, dtype=F32) -> torch.Tensor:
    return v.to(dtype)


def test_step_bounds_bite():
    """per step kernel: the correctly rounded fp64 result passes, the result with ONE coefficient scaled by 1 + 2^-17 fails; cfg: the halves swapped fail"""
    n, g = 1000, 2.0
    eps, _ = eps_pair(200, n, True, torch.device("cpu"))
    e0, e1 = split_eps(eps, n, True)
    x, m1, m2, last, z = rnd(201, n, scale=2.0), rnd(202, n), rnd(203, n), rnd(204, n, scale=2.0), rnd(205, n)
    tens = {"e0": e0, "e1": e1, "x": x, "m1": m1, "m2": m2, "last": last, "noise": z}
    cases = (("cfg_step", cfg_step_ref, list(CFG_COEF[:3]) + [0.0, g], "x_prev", 6, 0),
             ("unipc_step", unipc_ref, [float(v) for v in unipc_row(1, True)[:10]] + [0.0, 0.0, g], "x", 10, 7),
             ("dpmpp_step", dpmpp_ref, list(DPMPP_ROW[:6]) + [0.0, 0.0, g], "x", 9, 2),
             ("unclip_step", unclip_ref, list(unclip_variants()[1]) + [g], "x", 10, 4),
             ("lincomb", lambda t, c, mag: {"y": c[0] * t["x"] + c[1] * t["m1"] + c[2] * t["m2"]}, list(LIN_C[:3]), "y", 4, 0))
    for name, fn, c, out, k, which in cases:
        c = [float(torch.tensor(v, dtype=F32)) for v in c]
        val, mag = eval_both(fn, tens, c)
        bound = gamma(k) * mag[out]
        assert compare(_rounded(val[out]), val[out], bound)[0] == 0, name
        c2 = list(c)
        c2[which] *= 1.0 + 2.0 ** -17
        wrong, _ = eval_both(fn, tens, c2)
        assert compare(_rounded(wrong[out]), val[out], bound)[0] > 0, f"{name}: coefficient {which} scaled by 1 + 2^-17 passes the bound"
    val, mag = eval_both(cfg_step_ref, tens, list(CFG_COEF[:3]) + [0.0, g])
    sw, _ = eval_both(cfg_step_ref, dict(tens, e0=e1, e1=e0), list(CFG_COEF[:3]) + [0.0, g])
    for out in ("eps_out", "x_prev"):
        assert compare(_rounded(sw[out]), val[out], gamma(K_CFG[out]) * mag[out])[0] > 0, f"cfg_step {out}: the halves swapped pass the bound"
    a, b = rnd(206, 3, 352), rnd(207, 3, 352, scale=0.7)
    ref, bound = rescale_ref(a, b, 0.7)
    assert compare(_rounded(ref), ref, bound)[0] == 0
    assert compare(_rounded(ref * (1.0 + 2.0 ** -17)), ref, bound)[0] > 0, "rescale_noise_cfg: a factor scaled by 1 + 2^-17 passes the bound"


def test_softmax_bound_bites():
    """the correctly rounded softmax passes; the softmax of the row without its last column and the softmax at scale * (1 + 2^-10) of a shifted row fail"""
    for cols in (64, 300, 8192):
        s = softmax_rows_data(cols)
        ref, bound = softmax_ref(s, SM_SCALE)
        nviol, worst, _ = compare(ref.to(BF16), ref, bound)
        assert nviol == 0 and (cols < 8192 or worst > 0.9), (cols, nviol, worst)   # (the bf16 store alone nearly fills the bound: it is no looser than that)
        short = torch.cat([torch.softmax(s[:, :-1].double() * SM_SCALE, 1), torch.zeros(3, 1, dtype=torch.float64)], 1)
        for r in range(3):
            assert compare(short[r].to(BF16), ref[r], bound[r])[0] > 0, f"cols {cols} row {r}: the softmax without the last column passes"
        warm = torch.softmax(s.double() * (SM_SCALE * (1.0 + 2.0 ** -10)), 1)
        for r in (1, 2):
            assert compare(warm[r].to(BF16), ref[r], bound[r])[0] > 0, f"cols {cols} row {r}: scale * (1 + 2^-10) passes on a shifted row"


def test_small_linear_bound_bites():
    """the correctly rounded result passes; with ONE weight row moved by one bf16 ulp that row's outputs fail"""
    for B, K, N, variant in ((9, 512, 5, (0, 0, True, True)), (7, 1280, 4, (1, 1, True, False)), (8, 8, 3, (0, 2, False, True))):
        act_in, act_out, hb, ha = variant
        x, w, bias, add = small_linear_operands(B, K, N)
        bias, add = (bias if hb else None), (add if ha else None)
        ref, bound = small_linear_ref(x, w, bias, add, act_in, act_out)
        assert compare(ref.float(), ref, bound)[0] == 0
        w2 = w.clone()
        w2.view(torch.int16)[N - 1] += 1                                 # one ulp up in magnitude, every element of the row
        wrong, _ = small_linear_ref(x, w2, bias, add, act_in, act_out)
        nviol = compare(wrong[:, N - 1].float(), ref[:, N - 1], bound[:, N - 1])[0]
        assert nviol > 0, f"B {B} K {K} N {N}: a weight row one bf16 ulp off passes the bound"
        assert compare(wrong[:, :N - 1].float(), ref[:, :N - 1], bound[:, :N - 1])[0] == 0 if N > 1 else True


def test_timestep_bound_bites():
    """the fp32-rounded reference passes; ``half`` in place of ``half - shift`` fails"""
    for dim in (64, 320):
        ref, bound = timestep_ref(list(T_VALUES), dim, True, 1.0)
        assert compare(ref.float(), ref, bound)[0] == 0
        wrong, _ = timestep_ref(list(T_VALUES), dim, True, 1.0, wrong_half=True)
        for i, t in enumerate(T_VALUES):
            if t:
                assert compare(wrong[i].float(), ref[i], bound[i])[0] > 0, f"dim {dim} t {t}: half in place of half - shift passes the bound"


# ------------------------------------------------------------------------------------------------ return codes of the remaining entries
def test_refusals(backend):
    """every ``return -1`` of the entries not covered above: the call is refused and the output keeps its bytes (for the step-indexed table
    readers also rows < 1 and a misaligned step_error; their step_dev may be NULL -- row 0 -- so that is no refusal)"""
    dev = backend.device
    L, st = lib(), None
    f = torch.zeros(4096, dtype=F32, device=dev)
    h = torch.zeros(4096, dtype=BF16, device=dev)
    t64 = torch.zeros(8, dtype=torch.int64, device=dev)
    i32 = torch.zeros(1, dtype=torch.int32, device=dev)
    F, H, T, I = f.data_ptr(), h.data_ptr(), t64.data_ptr(), i32.data_ptr()
    c8 = (C.c_float * 8)(*UNCLIP_C)
    ptrs = (C.c_void_p * 6)(*([F] * 6))
    cs = (C.c_float * 6)(*LIN_C)
    o32, o16, o8 = Win(2048, F32, dev), Win(2048, BF16, dev), Win(2048, U8, dev)
    O, Q, B8 = o32.ptr, o16.ptr, o8.ptr
    calls = {
        "timestep_embedding": (L.pcdm_timestep_embedding, [T, 8, None, None, O, 2, 64, 1, 0.0, st],
                               {0: None, 4: None, 5: 0, 6: (0, 63, -2), 1: (0, -1), 3: I + 2}),
        "timestep_embedding_rows": (L.pcdm_timestep_embedding_rows, [T, 2, O, 64, 1, 0.0, st], {0: None, 1: 0, 2: None, 3: (0, 63)}),
        "time_class_combine": (L.pcdm_time_class_combine, [F, F, Q, 2, 2, 8, st], {0: None, 2: None, 3: 0, 4: 0, 5: 0}),
        "assemble_input": (L.pcdm_assemble_input, [F, 2, 2, F, 1, F, 1, Q, 2, 2, 16, st], {0: None, 5: None, 7: None, 1: 0, 2: 0, 10: (8, 20, 0)}),
        "nchw_f32_to_nhwc_bf16": (L.pcdm_nchw_f32_to_nhwc_bf16, [F, Q, 2, 3, 8, 5, st], {0: None, 1: None, 2: (0, -1), 3: (0, -1), 5: (0, -1), 4: (12, 0)}),
        "nhwc_bf16_to_nchw_f32": (L.pcdm_nhwc_bf16_to_nchw_f32, [H, O, 2, 3, 5, st], {0: None, 1: None, 2: (0, -1), 3: (0, -1), 4: (0, -1)}),
        "f32_to_bf16": (L.pcdm_f32_to_bf16, [F, Q, 100, st], {0: None, 1: None, 2: (0, -5)}),
        "cfg_step": (L.pcdm_cfg_step, [F, 1, 2.0, F, None, O, None, F, 4, None, None, 100, st],
                     {0: None, 11: (0, -1), 3: None, 7: None, 8: (0, -1), 10: I + 2}),
        "unipc_step": (L.pcdm_unipc_step, [F, 1, 2.0, O, O + 1024, O + 2048, O + 3072, F, 4, None, None, 100, st],
                       {0: None, 3: None, 4: None, 5: None, 6: None, 7: None, 8: (0, -1), 10: I + 2, 11: (0, -1)}),
        "dpmpp_step": (L.pcdm_dpmpp_step, [F, 1, 2.0, O, O + 1024, None, F, 4, None, None, 100, st],
                       {0: None, 3: None, 4: None, 6: None, 7: (0, -1), 9: I + 2, 10: (0, -1)}),
        "unclip_step": (L.pcdm_unclip_step, [F, 1, 2.0, F, None, O, c8, 100, st], {0: None, 3: None, 5: None, 6: None, 7: (0, -1)}),
        "unclip_step_dev": (L.pcdm_unclip_step_dev, [F, 1, 2.0, O, None, F, 4, I, None, 100, st],
                            {0: None, 3: None, 5: None, 6: (0, -1), 8: I + 2, 9: (0, -1)}),
        "lincomb": (L.pcdm_lincomb, [O, 3, ptrs, cs, 100, st], {0: None, 1: (0, 7, -1), 2: None, 3: None, 4: (0, -1)}),
        "rescale_noise_cfg": (L.pcdm_rescale_noise_cfg, [F, F, O, 2, 100, 0.7, st], {0: None, 1: None, 2: None, 3: (0, -1), 4: (1, 0)}),
        "gaussian_sample": (L.pcdm_gaussian_sample, [F, F, O, 2, 4, 5, 1.0, st], {0: None, 2: None, 3: 0, 4: 0, 5: 0}),
        "image_to_uint8": (L.pcdm_image_to_uint8, [F, B8, 2, 3, 5, st], {0: None, 1: None, 2: 0, 3: (2, 0), 4: 0}),
        "pixel_shuffle2": (L.pcdm_pixel_shuffle2, [H, Q, 1, 2, 2, 8, st], {0: (None, H + 2, H + 8), 1: (None, Q + 2, Q + 8), 2: 0, 3: 0, 4: 0, 5: (0, 4, 12)}),
        "advance_step": (L.pcdm_advance_step, [I, st], {0: None}),
    }
    stream = ops._stream(f)
    fails = []
    for name, (fn, good, overrides) in calls.items():
        for pos, values in overrides.items():
            for v in (values if isinstance(values, tuple) else (values,)):
                args = list(good)
                args[pos] = v
                args[-1] = stream
                rc = fn(*args)
                backend.sync()
                if rc != -1:
                    fails.append(f"pcdm_{name}: argument {pos} = {v!r} gives rc {rc}, expected -1")
        if not (o32.untouched() and o16.untouched() and o8.untouched()) or int(i32.cpu()[0]) != 0:
            fails.append(f"pcdm_{name}: a refused call wrote to its output")
            break
    # and every good call of the table is accepted (the refusals above are refusals of the one argument)
    for name, (fn, good, _) in calls.items():
        args = list(good)
        args[-1] = stream
        rc = fn(*args)
        backend.sync()
        if rc != 0:
            fails.append(f"pcdm_{name}: the accepted form of the call gives rc {rc}")
    assert not fails, "\n".join(fails)
