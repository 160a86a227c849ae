"""The device step counter: every kernel that indexes a DEVICE table by it bounds it on the device (include/pcdm.h, ABI 6).

One captured graph serves every denoise step because the step kernels index device tables (coefficients, per-step noise, timesteps, the time
table) by a device counter the host cannot see at launch.  A counter one past a table -- a reused state holds exactly that -- must read the
nearest valid row and raise ``*step_error``, never foreign memory.  The conformance suites judge values at valid rows; this file judges the
counter:

(a) ``READERS`` names every entry point (or struct) of include/pcdm.h that takes a device counter; a host-only test parses the header, so a
    reader added later without a row count and an error flag fails by name.
(b) the clamp matrix: for every reader, shape and counter value ``c``, every output and in-place state is BIT-IDENTICAL to the same call with
    the counter at ``min(max(c, 0), rows - 1)`` (a property, not a tolerance); the flag is raised exactly when ``c`` is outside ``[0, rows)`` and
    never cleared; ``step_error = NULL`` and ``step_dev = NULL`` are accepted.  The in-range call is what tests/test_small_ops_conformance.py
    holds to fp64; where its reference functions exist the clamped call is also judged against them with that file's own bound, and the
    references of different rows are shown to differ (so "the nearest row" cannot be confused with another).
(c) refusals (``rows < 1``, a misaligned ``step_error``, a ``pcdm_gn_splitk_src`` of another size) return -1 and write nothing.

Counter values.  Lane emulator: INT32_MIN, -1, 0, rows - 1, rows, rows + 7, INT32_MAX (the extremes catch arithmetic in front of the clamp:
``4 * st`` overflows there).  GPU: -1, 0, rows - 1, rows ONLY, and every table sits inside a larger buffer with ``WindowPlace.MARGIN`` (4096)
bytes on either side while no table row is longer than that: a kernel whose clamp were missing on the product build would still read only
memory this test owns.  Both conditions are asserted.

profiles/step_counter_values.json records, per reader and counter value, the row used and the flag: recorded, not gated."""
from __future__ import annotations

import ctypes as C
import fcntl
import json
import re
import tempfile
from pathlib import Path

import pytest
import torch

from pcdms_amd import _lib, ops
from tests import guarded as G
from tests import test_small_ops_conformance as S

ROOT = Path(__file__).resolve().parent.parent
VALUES = ROOT / "profiles" / "step_counter_values.json"
F32, BF16, I32, I64 = torch.float32, torch.bfloat16, torch.int32, torch.int64
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
ROWS = 3
NS = (1, 63, 260)                      # the scalar tail, a full vector body with a tail, more than one workgroup of 256 lanes
MAX_ROW_BYTES = 260 * 4                # the widest table row of this file: a noise row of 260 floats
G_SCALE = 2.0


def counters(backend):
    """in the order they are tried: the near ones first, so that a missing clamp shows as a wrong result before an extreme can fault"""
    if backend.is_emu:
        return (0, ROWS - 1, -1, ROWS, ROWS + 7, INT32_MAX, INT32_MIN)
    return (0, ROWS - 1, -1, ROWS)


def clamp(c: int) -> int:
    return min(max(c, 0), ROWS - 1)


def rn(seed: int, *shape, scale: float = 1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).float()


def lib():
    return _lib.lib()


def ptr(t):
    return None if t is None else t.data_ptr()


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None


class Tables:
    """the tables of one case, each at its exact extent inside a larger buffer of NaN bytes (``WindowPlace``), and the counter / flag cells"""

    def __init__(self, backend):
        self.backend, self.dev = backend, backend.device
        self.P = G.WindowPlace(self.dev, 0xFF)
        self.step = torch.zeros(1, dtype=I32, device=self.dev)
        self.err = torch.zeros(1, dtype=I32, device=self.dev)

    def table(self, t: torch.Tensor) -> torch.Tensor:
        """a [ROWS, width] table: a row is at most MARGIN bytes, so the rows -1 and ROWS of an UNBOUNDED read lie inside the window's margins"""
        assert t.shape[0] == ROWS and t[0].numel() * t.element_size() <= MAX_ROW_BYTES <= G.WindowPlace.MARGIN, t.shape
        return self.P(t, 16)

    def cells(self, c, preset, use_err=True):
        """(step pointer, flag pointer) for counter ``c`` (None: step_dev NULL) and a flag preset"""
        if c is not None:
            assert self.backend.is_emu or -1 <= c <= ROWS, "GPU: no counter whose unbounded read could leave the test's own buffers"
            self.step.fill_(c)
        self.err.fill_(preset)
        return (None if c is None else self.step.data_ptr()), (self.err.data_ptr() if use_err else None)

    def flag(self) -> int:
        self.backend.sync()
        return int(self.err.cpu()[0])


# ================================================================================================ the readers
# Each ``make_*(T, p)`` places the tables of one case and returns (call, reference): ``call(step_ptr, err_ptr) -> (rc, {name: tensor})`` builds
# the state afresh from fixed seeds, launches once and returns every output and in-place state; ``reference(row) -> {name: (fp64 value, bound)}``
# or None where tests/test_small_ops_conformance.py has no reference function for the reader.
def _eps(n, cfg, dev, seed=1):
    e = torch.cat([rn(seed, n), rn(seed + 1, n, scale=1.5) + 0.25])
    return e[: (2 * n if cfg else n)].contiguous(), e[: (2 * n if cfg else n)].contiguous().to(dev)


def _coef(width, seed):
    """[ROWS, width]: random rows that differ in every column (magnitudes around 1)"""
    t = rn(seed, ROWS, width) * 0.5 + torch.tensor([[1.0], [-0.75], [0.5]])
    return t.contiguous()


def make_cfg_step(T, p):
    n, cfg, noise, dev = p["n"], p["cfg"], p["noise"], T.dev
    eps, eps_d = _eps(n, cfg, dev)
    x, z = rn(3, n, scale=2.0), (rn(4, n) if noise else None)
    coef = _coef(4, 5)
    x_d, z_d, tab = x.to(dev), (None if z is None else z.to(dev)), T.table(coef)

    def call(sp, ep, rows=ROWS):
        xp, eo = S.Win(n, F32, dev), S.Win(n, F32, dev)
        rc = lib().pcdm_cfg_step(ptr(eps_d), int(cfg), G_SCALE, ptr(x_d), ptr(z_d), xp.ptr, eo.ptr, ptr(tab), rows, sp, ep, n, stream(dev))
        return rc, {"x_prev": xp, "eps_out": eo}

    def reference(row):
        e0, e1 = S.split_eps(eps, n, cfg)
        val, mag = S.eval_both(S.cfg_step_ref, {"e0": e0, "e1": e1, "x": x, "noise": z}, list(coef[row][:3]) + [0.0, G_SCALE])
        return {k: (val[k], S.gamma(S.K_CFG[k]) * mag[k]) for k in ("x_prev", "eps_out")}
    return call, reference, ("x_prev",)


def make_unipc_step(T, p):
    n, cfg, dev = p["n"], p["cfg"], T.dev
    eps, eps_d = _eps(n, cfg, dev)
    st0 = {"x": rn(3, n, scale=2.0), "m1": rn(4, n), "m2": rn(5, n), "last": rn(6, n, scale=2.0)}
    coef = _coef(12, 7)
    coef[:, 2] = torch.tensor([0.0, 1.0, 1.0])          # row 0: no corrector
    tab = T.table(coef)

    def call(sp, ep, rows=ROWS):
        w = {k: S.Win(n, F32, dev, init=v) for k, v in st0.items()}
        rc = lib().pcdm_unipc_step(ptr(eps_d), int(cfg), G_SCALE, w["x"].ptr, w["m1"].ptr, w["m2"].ptr, w["last"].ptr, ptr(tab), rows, sp, ep, n,
                                   stream(dev))
        return rc, w

    def reference(row):
        e0, e1 = S.split_eps(eps, n, cfg)
        corrector = float(coef[row][2]) != 0.0
        val, mag = S.eval_both(S.unipc_ref, dict(st0, e0=e0, e1=e1), [float(v) for v in coef[row]] + [G_SCALE])
        k = dict(S.K_UNIPC, last=S.K_UNIPC["last"] if corrector else 0)
        return {name: (val[name], S.gamma(k[name]) * mag[name] if k[name] else torch.zeros(n, dtype=torch.float64)) for name in st0}
    return call, reference, ("x", "m1")


def make_dpmpp_step(T, p):
    n, cfg, noise, dev = p["n"], p["cfg"], p["noise"], T.dev
    eps, eps_d = _eps(n, cfg, dev)
    st0 = {"x": rn(3, n, scale=2.0), "m1": rn(4, n)}
    coef, z = _coef(8, 8), (rn(9, ROWS, n) if noise else None)
    tab, z_d = T.table(coef), (None if z is None else T.table(z))

    def call(sp, ep, rows=ROWS):
        w = {k: S.Win(n, F32, dev, init=v) for k, v in st0.items()}
        rc = lib().pcdm_dpmpp_step(ptr(eps_d), int(cfg), G_SCALE, w["x"].ptr, w["m1"].ptr, ptr(z_d), ptr(tab), rows, sp, ep, n, stream(dev))
        return rc, w

    def reference(row):
        e0, e1 = S.split_eps(eps, n, cfg)
        val, mag = S.eval_both(S.dpmpp_ref, dict(st0, e0=e0, e1=e1, noise=None if z is None else z[row]), [float(v) for v in coef[row]] + [G_SCALE])
        return {k: (val[k], S.gamma(S.K_DPMPP[k]) * mag[k]) for k in st0}
    return call, reference, ("x", "m1")


def make_unclip_step_dev(T, p):
    n, cfg, noise, dev = p["n"], p["cfg"], p["noise"], T.dev
    eps, eps_d = _eps(n, cfg, dev)
    x = rn(3, n, scale=2.0)
    coef, z = _coef(8, 10), (rn(11, ROWS, n) if noise else None)
    coef[:, 2] = torch.tensor([1.5, 0.0, 2.5])          # clip: on, off, on
    tab, z_d = T.table(coef), (None if z is None else T.table(z))

    def call(sp, ep, rows=ROWS):
        w = {"x": S.Win(n, F32, dev, init=x)}
        rc = lib().pcdm_unclip_step_dev(ptr(eps_d), int(cfg), 4.0, w["x"].ptr, ptr(z_d), ptr(tab), rows, sp, ep, n, stream(dev))
        return rc, w

    def reference(row):
        e0, e1 = S.split_eps(eps, n, cfg)
        val, mag = S.eval_both(S.unclip_ref, {"e0": e0, "e1": e1, "x": x, "noise": None if z is None else z[row]}, [float(v) for v in coef[row]] + [4.0])
        return {"x": (val["x"], S.gamma(S.K_UNCLIP["x"]) * mag["x"])}
    return call, reference, ("x",)


def make_multistep_step(T, p):
    n, cfg, noise, dev = p["n"], p["cfg"], p["noise"], T.dev
    _, eps_d = _eps(n, cfg, dev)
    st0 = {k: rn(3 + i, n) for i, k in enumerate(("x", "xs", "h1", "h2", "h3"))}
    coef = _coef(ops.MS_ROW, 12)
    coef[:, ops.MS_SAVE] = torch.tensor([1.0, 0.0, 1.0])
    coef[:, ops.MS_PUSH] = torch.tensor([1.0, 1.0, 0.0])
    z = rn(13, ROWS, n) if noise else None
    tab, z_d = T.table(coef), (None if z is None else T.table(z))

    def call(sp, ep, rows=ROWS):
        w = {k: S.Win(n, F32, dev, init=v) for k, v in st0.items()}
        rc = lib().pcdm_multistep_step(ptr(eps_d), int(cfg), G_SCALE, w["x"].ptr, w["xs"].ptr, w["h1"].ptr, w["h2"].ptr, w["h3"].ptr, ptr(z_d),
                                       ptr(tab), rows, sp, ep, n, stream(dev))
        return rc, w
    return call, None, ("x",)


def make_assemble_input_ex(T, p):
    dev, rep = T.dev, 2 if p["cfg"] else 1
    N, h, w, cpad = 2, 3, 5, 16
    lat, mask, masked = rn(1, N, 4, h, w).to(dev), rn(2, 1, 1, h, w).to(dev), rn(3, 1, 4, h, w).to(dev)
    coef = _coef(ops.MS_ROW, 14)
    tab = T.table(coef)

    def call(sp, ep, rows=ROWS):
        out = S.Win(rep * N * h * w * cpad, BF16, dev)
        rc = lib().pcdm_assemble_input_ex(ptr(lat), N, rep, ptr(mask), 1, ptr(masked), 1, out.ptr, h, w, cpad, ptr(tab), ops.MS_ROW, ops.MS_IN_SCALE,
                                          rows, sp, ep, stream(dev))
        return rc, {"out": out}
    return call, None, ("out",)


def make_timestep_embedding(T, p):
    dev, (B, dim), f32 = T.dev, p["shape"], p["f32"]
    tv = [801.0, 400.25, 1.0] if f32 else [801, 401, 1]
    tab = T.table(torch.tensor(tv, dtype=F32 if f32 else I64))
    fn = lib().pcdm_timestep_embedding_f32 if f32 else lib().pcdm_timestep_embedding
    flip, shift = (1, 0.0) if dim == 64 else (0, 1.0)

    def call(sp, ep, rows=ROWS):
        out = S.Win(B * dim, F32, dev)
        return fn(ptr(tab), rows, sp, ep, out.ptr, B, dim, flip, shift, stream(dev)), {"out": out}

    def reference(row):
        ref, bound = S.timestep_ref([tv[row]], dim, bool(flip), shift)
        return {"out": (ref.expand(B, dim).contiguous(), bound.expand(B, dim).contiguous())}
    return call, reference, ("out",)


def _rowvec_table(T, B, N, seed):
    """the per-step row-vector blocks of pcdm_gemm_params.rowvec / pcdm_gn_splitk_src.rowvec: [ROWS, B * N] fp32 (a block is one table row)"""
    return T.table(_coef(B * N, seed))


def make_gemm_rowvec_step(T, p):
    dev, M, N, K = T.dev, 64, 64, 64
    a = rn(1, M, K).to(BF16).to(dev)
    pw = ops.pack_linear(rn(2, N, K, scale=0.125), rn(3, N), dev)
    rv = _rowvec_table(T, 1, N, 15)

    def call(sp, ep, rows=ROWS):
        out = S.Win(M * N, BF16, dev)
        ops.gemm(a, pw, out.t.view(M, N), rowvec=rv, rows_per_batch=M, tile=2, rowvec_step=None if sp is None else T.step, rowvec_step_stride=N,
                 rowvec_step_count=rows, step_error=None if ep is None else T.err)
        return 0, {"out": out}
    return call, None, ("out",)


def make_groupnorm_splitk_rowvec_step(T, p):
    dev, B, HW, C1, groups, sk = T.dev, 1, 5, 56, 8, 2
    M, Npad = B * HW, 64
    part, bias = (rn(7, sk * M * Npad, scale=0.5)).to(dev), rn(8, Npad).to(dev)
    rv = _rowvec_table(T, B, C1, 16)
    res = rn(10, M, C1).to(BF16).to(dev)
    gam, bet = rn(5, C1).to(dev), rn(6, C1).to(dev)
    ws = torch.zeros(lib().pcdm_groupnorm_ws_floats(B, C1), dtype=F32, device=dev)

    def call(sp, ep, rows=ROWS, struct_size=None):
        y, pre = S.Win(M * C1, BF16, dev), S.Win(M * C1, BF16, dev)
        s = _lib.GnSplitKSrc()
        if struct_size is not None:
            s.struct_size = struct_size
        s.part, s.split_k, s.M, s.N, s.Npad = ptr(part), sk, M, C1, Npad
        s.bias, s.rowvec, s.ldrv, s.residual, s.ldr = ptr(bias), ptr(rv), C1, ptr(res), C1
        s.rowvec_step, s.rowvec_step_stride, s.rowvec_step_count, s.step_error = sp, B * C1, rows, ep
        s.pre_out, s.store_pre = pre.ptr, 1
        rc = lib().pcdm_groupnorm_splitk(C.byref(s), None, 0, B, HW, groups, 1e-5, ptr(gam), ptr(bet), 1, y.ptr, ptr(ws), stream(dev))
        return rc, {"y": y, "pre": pre}
    return call, None, ("y", "pre")


def _step_params(noise_options=(False, True)):
    return [dict(n=n, cfg=cfg, noise=z) for n in NS for cfg in (False, True) for z in noise_options]


# name (a prototype of include/pcdm.h with a ``step_dev`` parameter, or ``struct.rowvec_step``) -> (maker, cases)
READERS = {
    "pcdm_cfg_step": (make_cfg_step, _step_params()),
    "pcdm_unipc_step": (make_unipc_step, _step_params((False,))),
    "pcdm_dpmpp_step": (make_dpmpp_step, _step_params()),
    "pcdm_unclip_step_dev": (make_unclip_step_dev, _step_params()),
    "pcdm_timestep_embedding": (make_timestep_embedding, [dict(shape=s, f32=False) for s in ((3, 64), (1, 6))]),
    "pcdm_timestep_embedding_f32": (make_timestep_embedding, [dict(shape=s, f32=True) for s in ((3, 64), (1, 6))]),
    "pcdm_multistep_step": (make_multistep_step, _step_params()),
    "pcdm_assemble_input_ex": (make_assemble_input_ex, [dict(cfg=False), dict(cfg=True)]),
    "pcdm_gemm_params.rowvec_step": (make_gemm_rowvec_step, [dict()]),
    "pcdm_gn_splitk_src.rowvec_step": (make_groupnorm_splitk_rowvec_step, [dict()]),
}
SIX = ("pcdm_cfg_step", "pcdm_unipc_step", "pcdm_dpmpp_step", "pcdm_unclip_step_dev", "pcdm_timestep_embedding", "pcdm_timestep_embedding_f32")
# Prototypes with a ``step_dev`` parameter that index no table by it, or whose table length the library is not told -- each with its reason.
EXEMPT = {
    "pcdm_advance_step": "increments the counter; reads no table",
    "pcdm_unet_forward": "no length argument for t_dev (include/pcdm.h, KNOWN REMAINDER): step_dev NULL reads t_dev[0]; with the table of "
                         "pcdm_unet_prepare_timesteps the counter is bounded into its n rows (pcdm_unet_step_overflow; tests/test_unet_ctx.py); "
                         "with a counter and no prepared table the length of t_dev stays the caller's contract.  Both pipelines prepare the table.",
    "pcdm_unet_forward_f32": "as pcdm_unet_forward",
}


# ================================================================================================ (a) the header and the table agree
def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pcdm.h").read_text(), flags=re.S)


def test_every_reader_of_the_header_is_in_the_table():
    hdr = _header()
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(pcdm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)}
    structs = {m.group(1): m.group(2) for m in re.finditer(r"typedef struct (pcdm_\w+) \{(.*?)\}\s*\1;", hdr, flags=re.S)}
    assert len(protos) > 100 and "pcdm_gemm_params" in structs and "pcdm_gn_splitk_src" in structs, "the header was not parsed"
    found = [n for n, args in protos.items() if re.search(r"\bstep_dev\b", args)]
    found += [f"{n}.rowvec_step" for n, body in structs.items() if re.search(r"\browvec_step\s*;", body)]
    assert len(found) >= 13, found
    for name in found:
        assert name in READERS or name in EXEMPT, f"{name} takes a device step counter and is neither in READERS nor in EXEMPT (with a reason)"
    assert set(READERS) | set(EXEMPT) == set(found), sorted((set(READERS) | set(EXEMPT)) ^ set(found))
    assert not set(READERS) & set(EXEMPT) and all(len(why) > 10 for why in EXEMPT.values())
    # every reader takes what the bound needs: a row count and the flag
    for name in READERS:
        if "." in name:
            body = structs[name.split(".")[0]]
            assert re.search(r"\browvec_step_count\s*;", body) and re.search(r"\bstep_error\s*;", body) and re.search(r"\bstruct_size\s*;", body), name
        else:
            args = protos[name]
            assert re.search(r"\bint (scale_)?rows\b", args) and re.search(r"\bint32_t\s*\*\s*step_error\b", args), f"{name}: no rows / step_error argument"
    assert set(SIX) <= set(READERS)


# ================================================================================================ (b) the clamp matrix
def _record(backend, reader, rows_used):
    try:
        with open(Path(tempfile.gettempdir()) / "pcdm_step_counter_values.lock", "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)                                   # (the CPU suite runs under pytest-xdist: one writer at a time)
            values = json.loads(VALUES.read_text()) if VALUES.exists() else {}
            values.setdefault(backend.name, {})[reader] = {str(c): dict(row=r, flag=f) for c, (r, f) in rows_used.items()}
            VALUES.write_text(json.dumps(values, indent=1, sort_keys=True) + "\n")
    except OSError:
        pass                                                                   # a read-only checkout still runs the assertions


def _same(a: dict, b: dict):
    """names of the windows (guards included) whose bits differ"""
    return [k for k in a if not torch.equal(a[k].bits(), b[k].bits())]


def _run(T, call, c, preset, use_err=True):
    sp, ep = T.cells(c, preset, use_err)
    rc, wins = call(sp, ep)
    return rc, wins, T.flag()


@pytest.mark.parametrize("reader", list(READERS))
def test_clamp_matrix(backend, reader):
    maker, cases = READERS[reader]
    assert MAX_ROW_BYTES <= G.WindowPlace.MARGIN == 4096
    used = {}
    for p in cases:
        T = Tables(backend)
        call, reference, distinct = maker(T, p)
        tag = f"{reader}{p}"
        # in range: one result per row, left exactly as it was for a preset of 0 and of 5
        base = {}
        for r in range(ROWS):
            rc, wins, flag = _run(T, call, r, 0)
            assert rc == 0 and flag == 0, f"{tag}: counter {r} in range: rc {rc}, flag {flag}"
            for k, w in wins.items():
                bad = w.problems(f"{tag} counter {r} {k}")
                assert not bad, bad
            base[r] = wins
        for r in range(1, ROWS):                                                # the rows differ, so "the nearest valid row" is no other row
            for k in distinct:
                assert not torch.equal(base[r][k].bits(), base[0][k].bits()), f"{tag}: rows 0 and {r} give the same {k}: the table does not bite"
        assert not any(torch.equal(base[1][k].bits(), base[2][k].bits()) for k in distinct), f"{tag}: rows 1 and 2 give the same result"
        if reference is not None:
            refs = {r: reference(r) for r in range(ROWS)}
            for r in range(ROWS):                                               # the clamped call against fp64, tests/test_small_ops_conformance.py's bound
                for k, (val, bound) in refs[r].items():
                    nviol, worst, at = S.compare(base[r][k].get(), val, bound)
                    assert nviol == 0, f"{tag} row {r} {k}: {nviol} elements beyond the fp64 bound, worst err / bound {worst:.4g} at {at}"
                for r2 in range(ROWS):                                          # on the reference alone: another row is another result
                    if r2 != r:
                        assert any(not torch.equal(refs[r][k][0].float(), refs[r2][k][0].float()) for k in distinct), (tag, r, r2)
                        assert any(S.compare(refs[r2][k][0].float(), refs[r][k][0], refs[r][k][1])[0] > 0 for k in distinct), \
                            f"{tag}: the reference of row {r2} passes the bound of row {r}"
        for c in counters(backend):
            want, out_of_range = base[clamp(c)], not 0 <= c < ROWS
            for preset in (0, 5):
                rc, wins, flag = _run(T, call, c, preset)
                assert rc == 0, f"{tag}: counter {c}: rc {rc}"
                diff = _same(wins, want)
                assert not diff, f"{tag}: counter {c} is not bit-identical to counter {clamp(c)} in {diff}"
                assert flag == (1 if out_of_range else preset), f"{tag}: counter {c}, flag preset {preset}: the flag is {flag}"
            rc, wins, flag = _run(T, call, c, 5, use_err=False)                 # step_error NULL: accepted, nothing raised anywhere
            assert rc == 0 and not _same(wins, want) and flag == 5, f"{tag}: counter {c} with step_error NULL: rc {rc}, flag cell {flag}"
            hit = [r for r in range(ROWS) if not _same(wins, base[r])]
            used.setdefault(c, (hit[0] if hit else None, 1 if out_of_range else 0))
            assert used[c] == (clamp(c), 1 if out_of_range else 0), (tag, c, used[c])
        rc, wins, flag = _run(T, call, None, 5)                                 # step_dev NULL: row 0, the flag is not touched
        assert rc == 0 and not _same(wins, base[0]) and flag == 5, f"{tag}: step_dev NULL: rc {rc}, flag {flag}, differs in {_same(wins, base[0])}"
    _record(backend, reader, used)


# ================================================================================================ (c) refusals write nothing
@pytest.mark.parametrize("reader", SIX)
def test_refusals_write_nothing(backend, reader):
    """rows < 1 and a step_error that is not 4-byte aligned: -1, and the sentinel-filled outputs, the in-place state and the flag keep their bytes"""
    maker, cases = READERS[reader]
    p = cases[-1]
    T = Tables(backend)
    call, _, _ = maker(T, p)
    _, fresh = call(*T.cells(None, 5), rows=0)                                   # (refused: the windows as they are built)
    pristine = {k: w.bits() for k, w in fresh.items()}
    for what, kw, misalign in (("rows = 0", dict(rows=0), 0), ("rows = -1", dict(rows=-1), 0), ("rows = INT32_MIN", dict(rows=INT32_MIN), 0),
                               ("step_error + 1", {}, 1), ("step_error + 2", {}, 2), ("step_error + 3", {}, 3)):
        for c in (0, ROWS):
            sp, ep = T.cells(c, 5)
            rc, wins = call(sp, ep + misalign, **kw)
            backend.sync()
            assert rc == -1, f"{reader} {what}: rc {rc}"
            assert all(torch.equal(w.bits(), pristine[k]) for k, w in wins.items()), f"{reader} {what}: a refused call wrote to its outputs or state"
            assert T.flag() == 5, f"{reader} {what}: a refused call wrote the flag"
    rc, _ = call(*T.cells(ROWS - 1, 0))
    assert rc == 0, "the accepted form of the call"


def test_cfg_combine_alone_ignores_rows(backend):
    """pcdm_cfg_step with coef == NULL (the CFG combine alone) reads no table: rows and step_error are neither used nor checked"""
    dev, n = backend.device, 63
    _, eps_d = _eps(n, True, dev)
    T = Tables(backend)
    got = []
    for rows, mis, c in ((ROWS, 0, 0), (0, 0, ROWS), (-1, 2, INT32_MAX if backend.is_emu else ROWS)):
        sp, ep = T.cells(c, 5)
        eo = S.Win(n, F32, dev)
        rc = lib().pcdm_cfg_step(ptr(eps_d), 1, G_SCALE, None, None, None, eo.ptr, None, rows, sp, ep + mis, n, stream(dev))
        assert rc == 0 and T.flag() == 5 and not eo.problems("eps_out"), (rows, mis, c, rc)
        got.append(eo.bits())
    assert all(torch.equal(g, got[0]) for g in got[1:])


def test_gn_splitk_src_of_another_size_is_refused(backend):
    """ABI 6: ``pcdm_gn_splitk_src.struct_size`` is the first field; a host compiled against the older header (no struct_size, so the field holds the
    low half of ``part``) or any other size is refused before another field is read: nothing is written, the flag included"""
    size = C.sizeof(_lib.GnSplitKSrc)
    assert _lib.GnSplitKSrc.struct_size.offset == 0 and _lib.GnSplitKSrc().struct_size == size
    T = Tables(backend)
    call, _, _ = make_groupnorm_splitk_rowvec_step(T, {})
    _, fresh = call(*T.cells(0, 5), struct_size=0)
    pristine = {k: w.bits() for k, w in fresh.items()}
    for bad in (0, size - 4, size + 8, size - 8, 0x7F000000):
        rc, wins = call(*T.cells(ROWS, 5), struct_size=bad)
        backend.sync()
        assert rc == -1, f"struct_size {bad}: rc {rc}"
        assert all(torch.equal(w.bits(), pristine[k]) for k, w in wins.items()) and T.flag() == 5, f"struct_size {bad}: a refused call wrote"
    rc, wins = call(*T.cells(ROWS, 5), struct_size=size)
    assert rc == 0 and T.flag() == 1 and not any(w.untouched() for w in wins.values())
