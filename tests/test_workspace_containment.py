"""Workspace containment: WHERE the library reads and writes, not what it computes (the conformance suites judge values).

Five entry points carve many buffers out of one caller-owned workspace by hand-counted sizes -- ``pcdm_unet_forward`` (the plan of
csrc/unet_ctx.hip), ``pcdm_dwpose_forward``, ``pcdm_detect_forward``, ``pcdm_lpips`` and ``pcdm_inception_features`` --, and every call takes
scratch memory it does not initialise.  Two instruments, over every entry point, at the smallest shapes that move each size formula off its
easy case:

* RED ZONES (B2).  The test hook ``pcdm_set_workspace_redzone`` (include/pcdm.h) makes every layout leave RZ = 64 KiB unused behind each
  buffer; ``pcdm_*_layout`` enumerates the buffers.  64 KiB is a condition, not a measurement: it exceeds any single padded row, ``Npad - N``
  column strip or cache-line round-up the kernels can emit, and it moves every offset by more than any tile, so a dependence on two buffers
  being adjacent shows as well.  Zones and outer guards hold 0xFF bytes (NaN in fp32, bf16 and e4m3, -1 in the integer tables); after the
  calls every such byte must still be 0xFF and every output must be BIT-identical to the same call without red zones.
* DIRTY MEMORY (B3).  ``torch.empty`` and its kin are wrapped so that fresh buffers arrive filled with 0x00, with 0xFF, or untouched; the
  user-visible outputs of fresh objects must be bit-identical across the three runs.  Code that depends on "fresh memory happens to be zero"
  differs between the first two.

B1 holds the five layouts to their invariants on a wider grid (host only); B4 shows that each instrument bites.  The per-buffer high-water
marks of the red-zone runs go to profiles/workspace_layout_values.json: recorded, not gated."""
from __future__ import annotations

import contextlib
import ctypes as C
import fcntl
import functools
import itertools
import json
import math
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle.unet import UNetConfig, synth_state_dict
from pcdms_amd import _lib, ops
from pcdms_amd.unet import Stage2_InapintUNet2DConditionModel, UNet2DConditionModel
from pcdms_amd.unet_ctx import UNetContext

ROOT = Path(__file__).resolve().parent.parent
RZ = 64 * 1024                                             # red zone and outer guard, bytes
FILL = 0xFF
VALUES = ROOT / "profiles" / "workspace_layout_values.json"
PARENT_TOTALS = Path(__file__).resolve().parent / "golden" / "workspace_totals_parent.json"   # recorded from a build of the parent commit


# ================================================================================================ the hooks, seen from Python
@pytest.fixture
def redzone(backend):
    """``set(bytes)`` on the library the ``backend`` fixture installed; whatever a test does, the process-wide value is 0 again afterwards."""
    lib = _lib.lib()

    def set_(nbytes):
        assert lib.pcdm_set_workspace_redzone(nbytes) == 0 and lib.pcdm_get_workspace_redzone() == nbytes

    assert lib.pcdm_get_workspace_redzone() == 0
    try:
        yield set_
    finally:
        lib.pcdm_set_workspace_redzone(0)


def _entries(fn, *args):
    """the enumerated layout ``[(name, offset, bytes)]`` of one sub-allocator, or None where it refuses the arguments"""
    f = getattr(_lib.lib(), fn)
    n = f(*args, -1, None, None, None)
    if n < 0:
        return None
    out = []
    for i in range(n):
        name, off, nb = C.c_char_p(), C.c_int64(-1), C.c_int64(-1)
        assert f(*args, i, C.byref(name), C.byref(off), C.byref(nb)) == n
        out.append((name.value.decode(), off.value, nb.value))
    assert f(*args, n, None, None, None) == -1 and f(*args, -2, None, None, None) == -1
    return out


def _check_layout(entries, total, rz):
    """B1: 256-aligned, in offset order, pairwise disjoint, inside the total, a gap of at least ``rz`` behind every entry -- and DENSE: each
    layout hands out its workspace without holes, so the next entry starts exactly ``rz`` behind the previous one and the total ends ``rz``
    behind the last (an entry that lost bytes, or a total that does not count the zones, breaks this)."""
    assert entries and total > 0 and total % 256 == 0
    at = 0
    names = [e[0] for e in entries]
    assert len(set(names)) == len(names), names
    for name, off, nb in entries:
        assert off % 256 == 0 and nb % 256 == 0 and nb >= 0, (name, off, nb)
        assert off >= at, f"'{name}' at {off} overlaps the entry before it (which ends at {at - rz}, red zone to {at})"
        assert off == at, f"'{name}' at {off}: a hole of {off - at} bytes in front of it"
        at = off + nb + rz
    assert at <= total, f"the last entry and its red zone end at {at}, beyond the reported total {total}"
    assert at == total, f"the reported total {total} is not the end of the last entry plus the red zone ({at})"


def _unet_cfg(boc, heads, cross, layers, ctx_dim=64, class_embed=1, out_channels=4):
    cfg = _lib.UNetConfig()
    cfg.out_channels, cfg.n_levels, cfg.layers_per_block, cfg.cross_attention_dim = out_channels, len(boc), layers, ctx_dim
    cfg.norm_groups, cfg.norm_eps, cfg.class_embed, cfg.flip_sin_to_cos, cfg.freq_shift = 32, 1e-5, class_embed, 1, 0.0
    for i, (c, hd, x) in enumerate(zip(boc, heads, cross)):
        cfg.block_out_channels[i], cfg.heads[i], cfg.cross_attn[i] = c, hd, x
    return cfg


UNET_TOPOLOGIES = {"two_level": ((64, 128), (1, 2), (1, 0), 1), "tiny": ((64, 128, 256, 256), (1, 2, 4, 4), (1, 1, 1, 0), 2)}


@contextlib.contextmanager
def _unet_handle(topology):
    lib = _lib.lib()
    h = lib.pcdm_unet_create(C.byref(_unet_cfg(*UNET_TOPOLOGIES[topology])))
    assert h
    try:
        yield h
    finally:
        lib.pcdm_unet_destroy(h)


def _dwpose_cfg(Hin, Win, K, spp=(0, 0, 0, 1)):
    """the tiny estimator of tests/test_dwpose.py (widen 0.125, deepen 0.34) as the C struct"""
    cfg = _lib.DWPoseConfig(Hin=Hin, Win=Win, K=K, stem=8, n_stages=4)
    for i, (co, nb, ident) in enumerate(((16, 1, 1), (32, 2, 1), (64, 2, 1), (128, 1, 0))):
        cfg.out[i], cfg.blocks[i], cfg.identity[i], cfg.spp[i] = co, nb, ident, spp[i]
    return cfg


def _detect_cfg(S, num_classes=5):
    """the tiny detector of tests/test_person_detector.py (widen 0.125, deepen 1/3) as the C struct"""
    cfg = _lib.DetectConfig(S=S, num_classes=num_classes, class_id=0, stem=8, head=32, neck_blocks=1, max_candidates=512, max_det=32, score_thr=0.5,
                            nms_thr=0.65, pose_nms_thr=0.7)
    for i, (co, nb) in enumerate(((16, 1), (32, 3), (64, 3), (128, 1))):
        cfg.out[i], cfg.blocks[i] = co, nb
    return cfg


# Each layout: name -> (total(args), entries(args), the argument grid as {argument: values}, which arguments must not shrink the total).
# ``args`` is a dict; the UNet's carry the open context under "handle".
def _lay_unet(topology):
    def total(a):
        return _lib.lib().pcdm_unet_workspace_bytes(a["handle"], a["B"], a["h"], a["w"], a["L"])

    def entries(a):
        return _entries("pcdm_unet_workspace_layout", a["handle"], a["B"], a["h"], a["w"], a["L"])
    grid = dict(B=(1, 2, 3, 4, 8), h=(7, 8, 10, 15, 16), w=(6, 8, 9, 11, 12, 24), L=(1, 5, 7, 9, 17, 77))
    return total, entries, grid


def _lay_dwpose():
    def cfg(a):
        return C.byref(_dwpose_cfg(a["Hin"], a["Win"], a["K"], a["spp"]))
    total = lambda a: _lib.lib().pcdm_dwpose_ws_bytes(cfg(a), a["R"], a["flip"])                                # noqa: E731
    entries = lambda a: _entries("pcdm_dwpose_ws_layout", cfg(a), a["R"], a["flip"])                             # noqa: E731
    return total, entries, dict(Hin=(32, 64, 96), Win=(32, 64), K=(1, 7, 133, 256), R=(1, 2, 3, 8), flip=(0, 1), spp=((0, 0, 0, 1), (0, 0, 0, 0), (1, 0, 0, 1)))


def _lay_detect():
    cfg = lambda a: C.byref(_detect_cfg(a["S"], a["classes"]))                                                   # noqa: E731
    total = lambda a: _lib.lib().pcdm_detect_ws_bytes(cfg(a), a["N"])                                            # noqa: E731
    entries = lambda a: _entries("pcdm_detect_ws_layout", cfg(a), a["N"])                                        # noqa: E731
    return total, entries, dict(S=(32, 64, 96, 128), N=(1, 2, 3, 5), classes=(1, 5, 80))


def _lay_lpips():
    refn = lambda a: a["N"] if a["ref_all"] else 1                                                               # noqa: E731
    total = lambda a: _lib.lib().pcdm_lpips_ws_bytes(a["N"], refn(a), a["H"], a["W"])                            # noqa: E731
    entries = lambda a: _entries("pcdm_lpips_ws_layout", a["N"], refn(a), a["H"], a["W"])                        # noqa: E731
    return total, entries, dict(N=(1, 2, 3, 5), ref_all=(0, 1), H=(31, 37, 64, 100), W=(31, 41, 48, 90))


def _lay_inception():
    total = lambda a: _lib.lib().pcdm_inception_ws_bytes(a["B"], a["H"], a["W"], a["dims"])                      # noqa: E731
    entries = lambda a: _entries("pcdm_inception_ws_layout", a["B"], a["H"], a["W"], a["dims"])                  # noqa: E731
    return total, entries, dict(B=(1, 2, 3), H=(35, 75, 100, 299), W=(35, 75, 80, 299), dims=(64, 192, 768, 2048))


LAYOUTS = {"unet_two_level": functools.partial(_lay_unet, "two_level"), "unet_tiny": functools.partial(_lay_unet, "tiny"), "dwpose": _lay_dwpose,
           "detect": _lay_detect, "lpips": _lay_lpips, "inception": _lay_inception}
ORDERED = {"B", "h", "w", "L", "Hin", "Win", "K", "R", "flip", "S", "N", "classes", "ref_all", "H"}   # arguments a larger value of which never shrinks the total
# (the inception trunk's W and dims are ordered too; "spp" is a tuple and is compared through its own case below)
ORDERED |= {"W", "dims"}


def _key(args):
    return "|".join(f"{k}={'.'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in args.items() if k != "handle")


@contextlib.contextmanager
def _grid(name):
    """-> (total, entries, [args]) of a layout over its whole grid"""
    total, entries, grid = LAYOUTS[name]()
    with (_unet_handle(name[len("unet_"):]) if name.startswith("unet_") else contextlib.nullcontext()) as handle:
        points = []
        for values in itertools.product(*grid.values()):
            a = dict(zip(grid, values))
            if handle is not None:
                a["handle"] = handle
            points.append(a)
        yield total, entries, grid, points


def parent_totals_of_this_library():
    """{layout: {arguments: total}} at red zone 0 over every grid: run once against a build of the PARENT commit to record
    tests/golden/workspace_totals_parent.json (the parent has no enumerators and no red zone: only the ``*_ws_bytes`` queries are used)."""
    out = {}
    for name in LAYOUTS:
        with _grid(name) as (total, _, _, points):
            out[name] = {_key(a): int(total(a)) for a in points}
    return out


# ================================================================================================ B1. layout invariants (host only)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layout_invariants(backend, redzone, name):
    parent = json.loads(PARENT_TOTALS.read_text())[name]
    with _grid(name) as (total, entries, grid, points):
        assert len(parent) == len(points)
        seen, refused = {}, 0
        for a in points:
            redzone(0)
            t0, e0 = total(a), entries(a)
            assert t0 == parent[_key(a)], f"{name} {_key(a)}: the total at red zone 0 is {t0}, the parent commit computed {parent[_key(a)]}"
            if t0 < 0:                                                         # refused: the documented error value from both, with and without zones
                refused += 1
                assert t0 == -1 and e0 is None
                redzone(RZ)
                assert total(a) == -1 and entries(a) is None
                continue
            _check_layout(e0, t0, 0)
            redzone(RZ)
            t1, e1 = total(a), entries(a)
            _check_layout(e1, t1, RZ)
            assert [(n, b) for n, _, b in e1] == [(n, b) for n, _, b in e0] and t1 == t0 + RZ * len(e0), _key(a)   # the zones move buffers, never resize them
            redzone(0)
            assert total(a) == t0 and entries(a) == e0                         # ... and switching back re-plans (the cached UNet plan is keyed on it)
            seen[tuple(a[k] for k in grid)] = t0
        assert len(seen) >= len(points) // 2, (len(seen), refused)
        # a larger argument never gives a smaller total
        keys = list(grid)
        for i, k in enumerate(keys):
            if k not in ORDERED:
                continue
            for point, t in seen.items():
                for bigger in grid[k]:
                    other = point[:i] + (bigger,) + point[i + 1:]
                    if bigger > point[i] and other in seen:
                        assert seen[other] >= t, f"{name}: {k} {point[i]} -> {bigger} shrinks the workspace ({t} -> {seen[other]}) at {dict(zip(keys, point))}"


def test_layout_refusals(backend, redzone):
    """bad arguments: the documented error value (-1) from every size query and every enumerator, and from the red-zone setter"""
    lib = _lib.lib()
    for bad in (-256, 1, 255, 64 * 1024 + 8):
        assert lib.pcdm_set_workspace_redzone(bad) == -1 and lib.pcdm_get_workspace_redzone() == 0
    none3 = (None, None, None)
    with _unet_handle("two_level") as h:
        for B, hh, w, L in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, -1, 1), (1, 8, 8, 0)):
            assert lib.pcdm_unet_workspace_bytes(h, B, hh, w, L) == -1 and lib.pcdm_unet_workspace_layout(h, B, hh, w, L, -1, *none3) == -1
        assert lib.pcdm_unet_workspace_bytes(None, 1, 8, 8, 1) == -1 and lib.pcdm_unet_workspace_layout(None, 1, 8, 8, 1, 0, *none3) == -1
        n = lib.pcdm_unet_workspace_layout(h, 1, 8, 8, 1, -1, *none3)
        assert n > 40 and lib.pcdm_unet_workspace_layout(h, 1, 8, 8, 1, n, *none3) == -1
    for cfg, R in ((_dwpose_cfg(32, 32, 7), 0), (_dwpose_cfg(32, 32, 257), 1), (_dwpose_cfg(40, 32, 7), 1), (_dwpose_cfg(32, 32, 7), 4097)):
        assert lib.pcdm_dwpose_ws_bytes(C.byref(cfg), R, 1) == -1 and lib.pcdm_dwpose_ws_layout(C.byref(cfg), R, 1, -1, *none3) == -1
    assert lib.pcdm_dwpose_ws_bytes(None, 1, 1) == -1 and lib.pcdm_dwpose_ws_layout(None, 1, 1, 0, *none3) == -1
    for cfg, N in ((_detect_cfg(32), 0), (_detect_cfg(40), 1), (_detect_cfg(32, num_classes=0), 1), (_detect_cfg(32), 4097)):
        assert lib.pcdm_detect_ws_bytes(C.byref(cfg), N) == -1 and lib.pcdm_detect_ws_layout(C.byref(cfg), N, -1, *none3) == -1
    assert lib.pcdm_detect_ws_bytes(None, 1) == -1 and lib.pcdm_detect_ws_layout(None, 1, 0, *none3) == -1
    for N, ref_n, H, W in ((0, 1, 31, 31), (3, 2, 31, 31), (1, 1, 30, 31), (1, 1, 31, 30), (65536, 1, 31, 31)):
        assert lib.pcdm_lpips_ws_bytes(N, ref_n, H, W) == -1 and lib.pcdm_lpips_ws_layout(N, ref_n, H, W, -1, *none3) == -1
    for B, H, W, dims in ((0, 35, 35, 64), (1, 2, 35, 64), (1, 35, 35, 100), (1, 35, 35, 2048), (65536, 35, 35, 64)):
        assert lib.pcdm_inception_ws_bytes(B, H, W, dims) == -1 and lib.pcdm_inception_ws_layout(B, H, W, dims, -1, *none3) == -1


def test_unet_plan_alternating_shapes(backend, redzone):
    """two shapes in turn on ONE context (a host may alternate batch shapes): each gets the same layout every time, with and without zones"""
    lib = _lib.lib()
    with _unet_handle("tiny") as h:
        first = {}
        for rz in (0, RZ, 0):
            redzone(rz)
            for _ in range(3):
                for shape in ((2, 7, 9, 5), (4, 16, 24, 77)):
                    got = (lib.pcdm_unet_workspace_bytes(h, *shape), _entries("pcdm_unet_workspace_layout", h, *shape))
                    assert first.setdefault((rz, shape), got) == got
        assert first[(0, (2, 7, 9, 5))] != first[(0, (4, 16, 24, 77))] and first[(RZ, (2, 7, 9, 5))][0] > first[(0, (2, 7, 9, 5))][0]


# ================================================================================================ the two instruments
class Allocs:
    """While active, ``torch.empty``, ``torch.empty_like``, ``torch.empty_strided`` and ``Tensor.new_empty`` hand out tensors on ``device`` whose
    bytes are ``fill`` -- and, with ``guard`` > 0, that lie between two guards of that many 0xFF bytes inside a larger allocation (``check``).
    ``torch.zeros`` is untouched.  ``count``: how many allocations were filled (a case in which the patch filled none has tested nothing).
    During a stream capture tensors are handed out untouched (a captured fill would be replayed over buffers that carry state between replays)."""

    def __init__(self, device, fill, guard=0):
        self.device, self.fill, self.guard = torch.device(device), fill, guard
        self.count, self.owned = 0, []

    def _mine(self, device):
        dev = torch.device(device) if device is not None else torch.device("cpu")
        return dev.type == self.device.type and not (dev.type == "cuda" and torch.cuda.is_current_stream_capturing())

    def _dirty(self, t):
        """an allocation of torch's own shape and strides: fill its whole storage"""
        if t.untyped_storage().nbytes():
            self._orig["empty"](0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage()).fill_(self.fill)
            self.count += 1
        return t

    def _make(self, shape, dtype, device):
        shape = tuple(int(v) for v in shape)
        n = math.prod(shape) * dtype.itemsize
        if n == 0 or dtype == torch.bool:
            return self._orig["empty"](shape, dtype=dtype, device=device)
        g, body = self.guard, (n + 255) // 256 * 256
        raw = self._orig["empty"](2 * g + body, dtype=torch.uint8, device=device)
        raw.fill_(FILL if g else self.fill)
        if g:
            raw[g:g + n].fill_(self.fill)
            self.owned.append((raw, n, f"{str(dtype).replace('torch.', '')}{list(shape)}"))
        self.count += 1
        return raw[g:g + n].view(dtype).view(shape)

    def __enter__(self):
        self._orig = {"empty": torch.empty, "empty_like": torch.empty_like, "empty_strided": torch.empty_strided, "new_empty": torch.Tensor.new_empty}
        o = self._orig
        plain = {"dtype", "device"}

        def empty(*size, **kw):
            if not self._mine(kw.get("device")) or set(kw) - plain:
                t = o["empty"](*size, **kw)
                return self._dirty(t) if self._mine(t.device) and "out" not in kw else t
            shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
            return self._make(shape, kw.get("dtype") or torch.get_default_dtype(), kw.get("device") or "cpu")

        def empty_like(t, **kw):
            device = kw.get("device") or t.device
            if not self._mine(device):
                return o["empty_like"](t, **kw)
            if set(kw) - plain or not t.is_contiguous() or t.layout != torch.strided:
                return self._dirty(o["empty_like"](t, **kw))
            return self._make(t.shape, kw.get("dtype") or t.dtype, device)

        def empty_strided(*a, **kw):
            t = o["empty_strided"](*a, **kw)
            return self._dirty(t) if self._mine(t.device) else t

        def new_empty(t, *size, **kw):
            device = kw.get("device") or t.device
            if not self._mine(device) or set(kw) - plain:
                r = o["new_empty"](t, *size, **kw)
                return self._dirty(r) if self._mine(r.device) else r
            shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
            return self._make(shape, kw.get("dtype") or t.dtype, device)

        torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty = empty, empty_like, empty_strided, new_empty
        return self

    def __exit__(self, *exc):
        o = self._orig
        torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty = o["empty"], o["empty_like"], o["empty_strided"], o["new_empty"]
        return False

    def check(self):
        """every guard byte is still 0xFF"""
        for raw, n, label in self.owned:
            for side, zone, base in (("in front of", raw[:self.guard], -self.guard), ("behind", raw[self.guard + n:], n)):
                bad = (zone != FILL).nonzero()
                assert bad.numel() == 0, (f"the guard {side} a separately owned {label} buffer of {n} bytes is damaged: first at byte "
                                          f"{base + int(bad[0])} of the buffer, {bad.numel()} bytes")


def _zones_intact(ws, entries, rz, what):
    """every red-zone byte inside a carved workspace is still 0xFF"""
    for name, off, nb in entries:
        bad = (ws[off + nb:off + nb + rz] != FILL).nonzero()
        assert bad.numel() == 0, (f"{what}: the red zone behind buffer '{name}' ({nb} bytes at {off}) is damaged: first at workspace byte "
                                  f"{off + nb + int(bad[0])}, {int(bad[0])} bytes past the buffer's end, {bad.numel()} bytes")


def _high_water(ws, entries, fill):
    """per buffer: ``used`` = 1 + the last byte that no longer holds ``fill`` (0: never touched -- or only ever written with the fill byte)"""
    out = {}
    for name, off, nb in entries:
        touched = (ws[off:off + nb] != fill).flip(0).to(torch.uint8)
        used = nb - int(touched.argmax()) if nb and bool(touched.any()) else 0
        out[name] = {"used": used, "bytes": nb}
    return out


def _parent_total(layout, **args):
    """what a build of the parent commit answered for this point of the layout's grid (tests/golden/workspace_totals_parent.json)"""
    return json.loads(PARENT_TOTALS.read_text())[layout][_key(args)]


def _record(layout, shape, backend, buffers, total, parent):
    """profiles/workspace_layout_values.json: per layout, shape and backend ``used / bytes`` of every buffer; the totals at red zone 0 of this
    build and of the parent commit's (which must agree)"""
    assert total == parent, (layout, shape, total, parent)
    try:
        with open(Path(tempfile.gettempdir()) / "pcdm_workspace_layout_values.lock", "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)                                   # (the CPU suite runs under pytest-xdist: one writer at a time)
            values = json.loads(VALUES.read_text()) if VALUES.exists() else {}
            row = values.setdefault(layout, {}).setdefault(shape, {})
            row["total_red_zone_0"], row["total_red_zone_0_parent"] = total, parent
            row[backend.name] = {"buffers": buffers, "tightest": max(buffers, key=lambda n: buffers[n]["used"] / max(buffers[n]["bytes"], 1))}
            VALUES.write_text(json.dumps(values, indent=1, sort_keys=True) + "\n")
    except OSError:
        pass                                                                   # a read-only checkout still runs the assertions


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8) if t.numel() else t.detach().reshape(-1)


def _same_bits(a, b):
    """bit-identical (NaNs included), for tensors and nests of tensors"""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))
    return a == b


# ================================================================================================ B2. red-zone runs: the UNet context
def _unet_config(topology, **kw):
    if topology == "two_level":   # small enough for the lane emulator: two levels, one layer per block, cross-attention on the first level and in the mid block
        return UNetConfig.tiny(block_out_channels=(64, 128), attention_head_dim=(1, 2), layers_per_block=1,
                               down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), **kw)
    return UNetConfig.tiny(**kw)


def _unet_kwargs(cfg):
    from tests.test_unet import _kwargs
    return dict(_kwargs(cfg), layers_per_block=cfg.layers_per_block, down_block_types=cfg.down_block_types, up_block_types=cfg.up_block_types)


def _unet_model(backend, cfg, cls=Stage2_InapintUNet2DConditionModel, fp8=False):
    """a FRESH model on the synthetic weights the UNet tests use (tests/test_unet_ctx._run_both: seed 3, random affine)"""
    m = cls(**_unet_kwargs(cfg))
    m.load_state_dict(synth_state_dict(cfg, seed=3, random_affine=True))
    m.to(backend.device)
    if fp8:
        m.set_attention_precision("fp8")
    return m


def _unet_inputs(cfg, B, h, w, L, n0, pose_b, shared=False):
    g = torch.Generator().manual_seed(0)
    s = torch.randn(B, cfg.in_channels, h, w, generator=g)
    if shared:
        s = torch.cat([s[:B // 2], s[:B // 2]])                                # both CFG halves: the same sample
    e = torch.randn(B, L, cfg.cross_attention_dim, generator=g)
    e[:n0] = 0
    c = None if cfg.projection_class_embeddings_input_dim is None else torch.randn(B, 1, cfg.projection_class_embeddings_input_dim, generator=g) * 0.4
    p = torch.randn(pose_b, cfg.block_out_channels[0], h, w, generator=g) * 0.1 if pose_b else None
    return s, e, c, p


TS3 = (801, 401, 1)                                                           # the 3-entry timestep table; the forwards with a device step counter read entry 1


def _python_schedule(backend, m, inp, B, h, w, n0, shared):
    """-> (x_in, eps of a plain forward at t = 417, eps of a forward that picks its timestep from the table by a device step counter)"""
    dev = backend.device
    s, e, c, p = inp
    to = lambda t: None if t is None else t.to(dev)                                                              # noqa: E731
    ts = torch.tensor(TS3, dtype=torch.int64, device=dev)
    step = torch.ones(1, dtype=torch.int32, device=dev)
    cond = m.prepare_conditioning(B, h, w, to(e), to(c), to(p), zero_ctx_batches=n0, shared_cfg_input=shared)
    x_in = ops.nchw_to_nhwc_bf16(s.to(dev), cpad=m._w["conv_in"].cin)
    plain = m._forward_nhwc(x_in, B, h, w, torch.tensor([417], dtype=torch.int64, device=dev), cond).clone()
    cond = m.prepare_conditioning(B, h, w, to(e), to(c), to(p), zero_ctx_batches=n0, shared_cfg_input=shared, timesteps=ts)
    table = m._forward_nhwc(x_in, B, h, w, ts, cond, step_dev=step).clone()
    backend.sync()
    assert not m.step_overflow()
    return x_in, plain, table


class _ZonedContext(UNetContext):
    """a UNetContext that paints the red zones of every workspace it allocates, AFTER ``pcdm_unet_workspace_init`` (which zeroes all of it)"""

    def workspace(self, B, h, w, L):
        fresh = (B, h, w, L) not in self._ws
        ws = super().workspace(B, h, w, L)
        if fresh:
            rz = _lib.lib().pcdm_get_workspace_redzone()
            ent = _entries("pcdm_unet_workspace_layout", self._h, B, h, w, L)
            assert ws.numel() == ent[-1][1] + ent[-1][2] + rz
            for _, off, nb in ent:
                ws[off + nb:off + nb + rz].fill_(FILL)
            self.zoned = (ws, ent, rz)
        return ws


def _c_schedule(backend, ctx, x_in, inp, B, h, w, n0, shared):
    dev = backend.device
    _, e, c, p = inp
    ts = torch.tensor(TS3, dtype=torch.int64, device=dev)
    step = torch.ones(1, dtype=torch.int32, device=dev)
    pose_b = ctx.prepare_conditioning(B, h, w, e, c, p, zero_ctx_batches=n0, shared_cfg_input=shared)
    plain = ctx.forward(x_in, torch.tensor([417], dtype=torch.int64, device=dev), None, B, h, w, pose_b)
    ctx.prepare_timesteps(ts, B, h, w)
    table = ctx.forward(x_in, ts, step, B, h, w, pose_b)
    backend.sync()
    assert not ctx.step_overflow(B, h, w)
    return plain, table


def _unet_red_zone_case(backend, redzone, topology, B, h, w, L, n0, pose_b, fp8, shared=False, cls=None, **cfg_kw):
    if cls is None:   # (the stage-2 class adds the pose feature unconditionally: a case without pose runs the class that does not require one)
        cls = Stage2_InapintUNet2DConditionModel if pose_b else UNet2DConditionModel
    cfg = _unet_config(topology, **cfg_kw)
    m = _unet_model(backend, cfg, cls, fp8)
    inp = _unet_inputs(cfg, B, h, w, L, n0, pose_b, shared)
    x_in, py_plain, py_table = _python_schedule(backend, m, inp, B, h, w, n0, shared)
    assert not torch.equal(py_plain, py_table) and bool(torch.isfinite(py_plain).all())
    c0_plain, c0_table = _c_schedule(backend, UNetContext(m), x_in, inp, B, h, w, n0, shared)       # red zone 0, an ordinary workspace
    redzone(RZ)
    with Allocs(backend.device, FILL, guard=RZ) as al:   # the workspace, the time table and the outputs are separately owned: outer guards
        ctx = _ZonedContext(m)
        c1_plain, c1_table = _c_schedule(backend, ctx, x_in, inp, B, h, w, n0, shared)
    backend.sync()
    ws, ent, rz = ctx.zoned
    what = f"pcdm_unet_* {topology} B={B} {h}x{w} L={L} n0={n0} pose_b={pose_b} fp8={int(fp8)} shared={int(shared)}"
    assert rz == RZ and al.count >= 4
    _zones_intact(ws, ent, RZ, what)
    al.check()
    assert _same_bits((c1_plain, c1_table), (c0_plain, c0_table)), what                      # the zones change no bit
    assert _same_bits((c0_plain, c0_table), (py_plain, py_table)), what                      # ... and the C schedule is the fp64-judged Python schedule
    redzone(0)
    with _unet_handle(topology) as hd:
        total0 = _lib.lib().pcdm_unet_workspace_bytes(hd, B, h, w, L)
    _record(f"unet_{topology}", f"B={B}|h={h}|w={w}|L={L}|n0={n0}|pose_b={pose_b}|fp8={int(fp8)}|shared={int(shared)}|class_embed={int(bool(cfg.class_embed_type))}",
            backend, _high_water(ws, ent, 0), total0, _parent_total(f"unet_{topology}", B=B, h=h, w=w, L=L))


# (B, h, w, L, n0, pose_b, fp8): batch 1 and one context token | 63 pixels, every (x - 1) / 2 + 1 level odd | n0 == B, L one past a multiple of
# 16, a pose per batch entry, fp8 | 77 tokens, fp8
UNET_CASES = [(1, 8, 8, 1, 0, 0, False), (2, 7, 9, 5, 1, 1, False), (3, 10, 6, 17, 3, 3, True), (2, 16, 12, 77, 0, 1, True)]


@pytest.mark.parametrize("B,h,w,L,n0,pose_b,fp8", UNET_CASES)
def test_unet_red_zones(backend, redzone, B, h, w, L, n0, pose_b, fp8):
    _unet_red_zone_case(backend, redzone, "two_level" if backend.is_emu else "tiny", B, h, w, L, n0, pose_b, fp8)


def test_unet_red_zones_shared_cfg_input(backend, redzone):
    _unet_red_zone_case(backend, redzone, "two_level" if backend.is_emu else "tiny", 4, 8, 8, 5, 2, 1, False, shared=True)


@pytest.mark.gpu
def test_unet_red_zones_odd_sides_gpu(gpu_backend, redzone_gpu):
    _unet_red_zone_case(gpu_backend, redzone_gpu, "tiny", 4, 15, 11, 9, 2, 1, False)


@pytest.mark.gpu
def test_unet_red_zones_stage3_topology_gpu(gpu_backend, redzone_gpu):
    """no class embedding, no pose (the stage-3 refinement UNet, in_channels 8)"""
    _unet_red_zone_case(gpu_backend, redzone_gpu, "tiny", 2, 16, 12, 7, 1, 0, False, cls=UNet2DConditionModel, in_channels=8, class_embed_type=None,
                        projection_class_embeddings_input_dim=None)


@pytest.fixture
def redzone_gpu(gpu_backend):
    lib = _lib.lib()

    def set_(nbytes):
        assert lib.pcdm_set_workspace_redzone(nbytes) == 0 and lib.pcdm_get_workspace_redzone() == nbytes

    try:
        yield set_
    finally:
        lib.pcdm_set_workspace_redzone(0)


# ================================================================================================ B2. red-zone runs: the four one-call networks
def _carved_call(backend, redzone, layout, shape, total, entries, call, parent):
    """``call(ws)`` on an ordinary workspace at red zone 0, then at RZ on a workspace that is 0xFF everywhere (these calls promise nothing about
    the workspace's prior contents) between two outer guards: zones and guards intact, outputs bit-identical; the high-water marks are recorded"""
    dev = backend.device
    redzone(0)
    total0 = total()
    assert total0 > 0
    ref = call(torch.empty(total0, dtype=torch.uint8, device=dev))
    backend.sync()
    redzone(RZ)
    ent = entries()
    with Allocs(dev, FILL, guard=RZ) as al:                                    # (the outputs the wrappers allocate get outer guards too)
        ws = torch.empty(total(), dtype=torch.uint8, device=dev)
        assert ws.numel() == total0 + RZ * len(ent) and ws.data_ptr() % 16 == 0
        out = call(ws)
    backend.sync()
    what = f"{layout} {shape}"
    _zones_intact(ws, ent, RZ, what)
    al.check()
    assert _same_bits(out, ref), what
    redzone(0)
    _record(layout, shape, backend, _high_water(ws, ent, FILL), total0, parent)
    return ws, ent, out


@functools.lru_cache(maxsize=None)
def _dw_weights(Win, Hin, K):
    """the tiny estimator of tests/test_dwpose.py at another input size / keypoint count: (constructor arguments, synthetic state dict)"""
    from tests import test_dwpose as D
    kw = dict(input_size=(Win, Hin), widen_factor=0.125, deepen_factor=0.34, num_keypoints=K)
    sd = D.synth_state_dict(kw, D.SEED)
    if K != 133:
        kw["flip_indices"] = tuple(reversed(range(K)))
    return kw, sd


def _dw_estimator(Win, Hin, K):
    from pcdms_amd import pose
    kw, sd = _dw_weights(Win, Hin, K)
    return pose.DWPoseEstimator(sd, **kw)


def _dw_inputs(backend, R):
    from tests import test_dwpose as D
    img = D._dev(D._images(2, 70, 50, 11), backend)
    boxes = torch.tensor([[4.0, 3.0, 40.0, 60.0], [-8.0, 10.0, 45.0, 66.0], [20.0, 30.0, 49.5, 69.0]][:R]).to(backend.device)
    index = torch.tensor([0, 1, 1][:R], dtype=torch.int32).to(backend.device)
    return img, boxes, index


# Hin x Win 32 x 32 and 64 x 32; R = 1 and 3; flip off and on; 7 keypoints and 133 (neither a multiple of 4: the token matrix pads its rows);
# every network has stages without SPP (1-3) and one with it (4)
@pytest.mark.parametrize("Hin,Win,K,R,flip", [(32, 32, 7, 1, False), (32, 32, 133, 3, True), (64, 32, 7, 3, True), (64, 32, 133, 1, False)])
def test_dwpose_red_zones(backend, redzone, Hin, Win, K, R, flip):
    est = _dw_estimator(Win, Hin, K)
    cfg, wt = est._c_args(backend.device)
    img, boxes, index = _dw_inputs(backend, R)
    _, _, (kp, sc) = _carved_call(backend, redzone, "dwpose", f"Hin={Hin}|Win={Win}|K={K}|R={R}|flip={int(flip)}",
                                  lambda: ops.dwpose_ws_bytes(cfg, R, flip), lambda: _entries("pcdm_dwpose_ws_layout", C.byref(cfg), R, int(flip)),
                                  lambda ws: ops.dwpose_forward(img, boxes, index, flip, cfg, wt, ws),
                                  _parent_total("dwpose", Hin=Hin, Win=Win, K=K, R=R, flip=int(flip), spp=(0, 0, 0, 1)))
    assert bool(torch.isfinite(kp).all()) and bool(torch.isfinite(sc).all())
    assert _same_bits((kp, sc), tuple(est(img, boxes, index, flip_test=flip)))                     # ... and it is what the public call returns


def _detector(S):
    from pcdms_amd import pose
    from tests import test_person_detector as P
    return pose.PersonDetector(P._tiny()[0], **dict(P.TINY, size=S))


def _det_images(backend, N, portrait):
    from tests import test_person_detector as P
    H, W = (45, 29) if portrait else (30, 52)
    return P._dev(P._images(N, H, W, 11), backend)


@pytest.mark.parametrize("S,N,portrait", [(32, 1, True), (32, 3, False), (64, 3, True), (64, 1, False)])
def test_detector_red_zones(backend, redzone, S, N, portrait):
    det = _detector(S)
    cfg, wt = det._c_args(backend.device)
    img = _det_images(backend, N, portrait)
    _, _, out = _carved_call(backend, redzone, "detect", f"S={S}|N={N}|{'portrait' if portrait else 'landscape'}",
                             lambda: ops.detect_ws_bytes(cfg, N), lambda: _entries("pcdm_detect_ws_layout", C.byref(cfg), N),
                             lambda ws: ops.detect_forward(img, cfg, wt, ws), _parent_total("detect", S=S, N=N, classes=5))
    assert _same_bits(out, tuple(det(img)))


def _lpips_model():
    from pcdms_amd import metrics
    from tests import test_lpips as L
    return metrics.LPIPS("alex").load_state_dict(L._state_dict())


def _lpips_images(backend, N, ref_n, kind, H, W):
    from tests import test_lpips as L
    a, b = L._family("noise", H, W, N)
    return L._dev(L._as_input(a, kind), backend), L._dev(L._as_input(b[:ref_n], kind), backend)


# N = 1 / 3, ref_n = 1 / N, uint8 and fp32, the smallest size (31 x 31: conv3-5 on one pixel) and an odd one
@pytest.mark.parametrize("N,ref_n,kind,H,W", [(1, 1, "u8", 31, 31), (3, 1, "f32", 37, 41), (3, 3, "u8", 37, 41), (3, 3, "f32", 31, 31)])
def test_lpips_red_zones(backend, redzone, N, ref_n, kind, H, W):
    m = _lpips_model()
    a, b = _lpips_images(backend, N, ref_n, kind, H, W)
    dev, win = backend.device, (0, 0, W, H)
    wt = m._weights(dev)

    def call(ws):
        out, layers = torch.empty(N, dtype=torch.float32, device=dev), torch.empty((5, N), dtype=torch.float32, device=dev)
        argmin = torch.empty(1, dtype=torch.int32, device=dev)
        ops.lpips(a, b, win, win, wt, out, layers, argmin, ws, normalize=True)
        return out, layers, argmin
    _, _, (out, layers, _) = _carved_call(backend, redzone, "lpips", f"N={N}|ref_n={ref_n}|{kind}|H={H}|W={W}", lambda: ops.lpips_ws_bytes(N, ref_n, H, W),
                                          lambda: _entries("pcdm_lpips_ws_layout", N, ref_n, H, W), call,
                                          _parent_total("lpips", N=N, ref_all=int(ref_n == N and N > 1), H=H, W=W))
    got, got_layers = m(a, b, normalize=True, return_layers=True)
    assert _same_bits((out, layers), (got.view(-1), got_layers)) and bool((out > 1e-3).all())


def _inception_model(dims, resize):
    from pcdms_amd import metrics
    from tests import test_fid as F
    return metrics.InceptionV3Features(dims, resize_input=resize).load_state_dict(F._state_dict())


def _inception_case(backend, redzone, dims, H, W, resize, N=2):
    from tests import test_fid as F
    m = _inception_model(dims, resize)
    x = F._dev(F._images(N, H, W, 11, "f32"), backend)
    dev, win = backend.device, (0, 0, W, H)
    wt = m._weights(dev)
    h, w = (299, 299) if resize else (H, W)

    def call(ws):
        out = torch.empty((N, dims), dtype=torch.float32, device=dev)
        return ops.inception_features(x, win, wt, out, ws, dims=dims, resize=resize, normalize=True)
    _, _, out = _carved_call(backend, redzone, "inception", f"dims={dims}|N={N}|H={H}|W={W}|resize={int(resize)}", lambda: ops.inception_ws_bytes(N, h, w, dims),
                             lambda: _entries("pcdm_inception_ws_layout", N, h, w, dims), call, _parent_total("inception", B=N, H=h, W=w, dims=dims))
    assert _same_bits(out, m(x)) and bool(torch.isfinite(out).all()) and (N == 1 or not torch.equal(out[0], out[1]))


# the stem depths of tests/test_fid.py::test_trunk_stem (35 x 35, own size), and the bilinear resize to 299 x 299 in front of them (one image)
@pytest.mark.parametrize("dims,resize", [(64, False), (192, False), (64, True), (192, True)])
def test_inception_red_zones(backend, redzone, dims, resize):
    _inception_case(backend, redzone, dims, 35, 35, resize, N=1 if resize and backend.is_emu else 2)   # (299 x 299 under the lane emulator: 20-45 s an image)


@pytest.mark.gpu
@pytest.mark.parametrize("dims,resize", [(768, False), (2048, False), (768, True), (2048, True)])
def test_inception_red_zones_blocks_gpu(gpu_backend, redzone_gpu, dims, resize):
    _inception_case(gpu_backend, redzone_gpu, dims, 75, 75, resize)


# ================================================================================================ B2. separately owned buffers: outer guards
def _metric_images(backend, N=3, H=37, W=41, ref_n=1):
    rng = np.random.default_rng(5)
    cand = torch.from_numpy(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)).to(backend.device)
    ref = torch.from_numpy(rng.integers(0, 256, (ref_n, H, W, 3), dtype=np.uint8)).to(backend.device)
    return cand, ref


def _pose_people(backend, M=2, P=2, H=48, W=40):
    g = torch.Generator().manual_seed(3)
    kp = torch.rand(M, P, 134, 2, generator=g) * torch.tensor([W + 8.0, H + 8.0]) - 4.0       # some joints outside the frame
    sc = torch.rand(M, P, 134, generator=g)
    return kp.to(backend.device), sc.to(backend.device)


def _single_region_calls(backend):
    """name -> a call through the public wrapper, which allocates the call's single-region workspace and its outputs with ``torch.empty``"""
    from pcdms_amd import metrics, pose, preprocess
    cand, ref = _metric_images(backend)
    cand_f, ref_f = cand.float() / 255, ref.float() / 255
    src = _metric_images(backend, 1, 50, 44)[0][0]
    kp, sc = _pose_people(backend)
    return {
        "ssim": lambda: metrics.ssim(cand, ref), "ssim_f32_window": lambda: metrics.ssim(cand_f, ref_f, cand_window=(3, 2, 33, 31), ref_window=(8, 6, 33, 31)),
        "psnr": lambda: (metrics.psnr(cand, ref), metrics.mse(cand_f, ref_f)),
        "absdiff": lambda: (metrics.l1(cand, ref), metrics.mae(cand, ref), metrics.l1(cand_f, ref_f)),
        "ssim_box": lambda: (metrics.ssim_box(cand, ref, win_size=7), metrics.ssim_box(cand_f, ref_f, win_size=11, data_range=1.0)),
        "resample_u8": lambda: (preprocess.resize(src, (23, 17)), preprocess.resize(src, (61, 70)), preprocess.resize(src, (44, 21))),
        "resize_cv_cubic": lambda: (preprocess.resize_cv_cubic(src, (23, 17)), preprocess.resize_cv_cubic(src.float(), (61, 70), divisor=255.0, layout="nchw")),
        "pose_draw": lambda: (pose.draw_pose(kp, sc, (48, 40)), pose.draw_pose(kp, sc, (48, 40), image_size=(31, 27), faces=True)),
    }


SINGLE_REGION = ("ssim", "ssim_f32_window", "psnr", "absdiff", "ssim_box", "resample_u8", "resize_cv_cubic", "pose_draw")


@pytest.mark.parametrize("name", SINGLE_REGION)
def test_single_region_workspaces_are_contained(backend, name):
    """``pcdm_ssim``, ``pcdm_psnr``, ``pcdm_absdiff``, ``pcdm_ssim_box``, ``pcdm_resample_u8`` and ``pcdm_pose_draw`` take ONE region each: the
    workspace and every output tensor between outer guards, 0xFF inside; guards intact, results those of an ordinary call"""
    call = _single_region_calls(backend)[name]
    ref = call()
    backend.sync()
    with Allocs(backend.device, FILL, guard=RZ) as al:
        out = call()
    backend.sync()
    assert al.count >= 2, al.count
    al.check()
    assert _same_bits(out, ref), name


# ================================================================================================ B3. dirty-memory runs
def _three_fills(backend, run):
    """``run()`` builds FRESH objects and returns the user-visible outputs: once on fresh buffers full of 0x00, once full of 0xFF, once unpatched;
    bit-identical results, the patch must have filled something, and no separately owned buffer is overrun (256-byte guards)"""
    outs = {}
    for fill in (None, 0x00, FILL):
        if fill is None:
            outs[fill] = run()
            backend.sync()
            continue
        with Allocs(backend.device, fill, guard=256) as al:
            outs[fill] = run()
            backend.sync()
        assert al.count > 0, "the allocation patch filled nothing: the case tests nothing"
        al.check()
    assert _same_bits(outs[0x00], outs[FILL]), "fresh buffers full of 0x00 and full of 0xFF give different results: uninitialised memory is read"
    assert _same_bits(outs[None], outs[FILL]), "an unpatched run differs from the runs on filled buffers"
    return outs[None]


def _unet_shape(backend):
    return ("two_level", 2, 7, 9, 5, 1, 1) if backend.is_emu else ("tiny", 4, 15, 11, 9, 2, 1)


@pytest.mark.parametrize("fp8", [False, True])
def test_dirty_memory_unet_python_schedule(backend, fp8):
    topology, B, h, w, L, n0, pose_b = _unet_shape(backend)
    cfg = _unet_config(topology)
    inp = _unet_inputs(cfg, B, h, w, L, n0, pose_b)
    _three_fills(backend, lambda: _python_schedule(backend, _unet_model(backend, cfg, fp8=fp8), inp, B, h, w, n0, False)[1:])


@pytest.mark.parametrize("fp8", [False, True])
def test_dirty_memory_unet_context(backend, fp8):
    topology, B, h, w, L, n0, pose_b = _unet_shape(backend)
    cfg = _unet_config(topology)
    inp = _unet_inputs(cfg, B, h, w, L, n0, pose_b)

    def run():
        m = _unet_model(backend, cfg, fp8=fp8)
        ctx = UNetContext(m)
        x_in = ops.nchw_to_nhwc_bf16(inp[0].to(backend.device), cpad=m._w["conv_in"].cin)
        return _c_schedule(backend, ctx, x_in, inp, B, h, w, n0, False)
    _three_fills(backend, run)


def test_used_unet_workspace_equals_a_fresh_one(backend):
    """one workspace: fp8 attention with n0 = 1 and a shared pose, then ``prepare_conditioning`` again with fp8 off, another n0 and a pose per
    batch entry -- what the first use left (e4m3 copies, K / V^T of entries that are now skipped, LayerNorm partials) must not reach the result"""
    topology, B, h, w, L, _, _ = _unet_shape(backend)
    cfg = _unet_config(topology)
    m = _unet_model(backend, cfg)
    first, second = _unet_inputs(cfg, B, h, w, L, 1, 1), _unet_inputs(cfg, B, h, w, L, B // 2 + 1, B)
    lib = _lib.lib()

    def forwards(ctx, inp, n0):
        return _c_schedule(backend, ctx, ops.nchw_to_nhwc_bf16(inp[0].to(backend.device), cpad=m._w["conv_in"].cin), inp, B, h, w, n0, False)
    used = UNetContext(m)
    assert lib.pcdm_unet_set_attention_fp8(used._h, 1) == 0
    dirty = forwards(used, first, 1)
    assert lib.pcdm_unet_set_attention_fp8(used._h, 0) == 0
    again = forwards(used, second, B // 2 + 1)
    fresh = forwards(UNetContext(m), second, B // 2 + 1)
    assert not _same_bits(dirty, again)
    assert _same_bits(again, fresh)


def test_dirty_memory_vae(backend):
    """tiny VAE, encode and decode at a ragged latent (3 x 5: an area that is no multiple of 64, odd sides)"""
    from oracle import vae as O
    from tests.test_vae_any_size import _build
    cfg = O.VAEConfig.tiny()
    g = torch.Generator().manual_seed(20)
    x, z = torch.rand(1, 3, 24, 40, generator=g) * 2 - 1, torch.randn(1, 4, 3, 5, generator=g)

    def run():
        _, m = _build(backend.device, cfg, seed=7)
        return (m.encode(x.to(backend.device)).latent_dist.parameters, m.decode(z.to(backend.device), return_dict=False)[0],
                m.decode_to_uint8(z.to(backend.device)))
    _three_fills(backend, run)


def _cond_stack_cases(backend):
    """name -> (build a fresh model, inputs, call): the existing tiny configurations of tests/test_cond_stack_conformance.py and tests/test_cond.py"""
    from oracle import prior as OP
    from pcdms_amd import CLIPVisionModelWithProjection, ControlNetConditioningEmbedding, Dinov2Model, ImageProjModel_p, Stage1_PriorTransformer
    from pcdms_amd.cond import ImageProjection
    from tests import test_cond_stack_conformance as S
    dev = backend.device
    rnd = lambda *shape, seed=4: torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)     # noqa: E731
    dino_cfg = S.DINO_CASES["swiglu_28x42"][0]
    pcfg = OP.PriorConfig.tiny()
    px, ppe, psp, ptp = rnd(2, 1, 1024, seed=8), rnd(2, 1, 1024, seed=9) * 0.5, rnd(2, 1, 36, seed=10).abs(), rnd(2, 1, 36, seed=11).abs()
    return {
        "dinov2_swiglu": (lambda: Dinov2Model(dino_cfg), 1, lambda m, x=rnd(2, 3, 28, 42, seed=5): (lambda o: (o.last_hidden_state, o.pooler_output))(m(x))),
        "dinov2_gelu": (lambda: Dinov2Model(S.DINO_CASES["gelu_native28"][0]), 1, lambda m, x=rnd(1, 3, 28, 28, seed=5): (m(x).last_hidden_state,)),
        "clip_dh80": (lambda: CLIPVisionModelWithProjection(S._clip_cfg(80)), 2, lambda m, x=rnd(2, 3, 28, 28, seed=12): tuple(m(x, return_dict=False))),
        "clip_dh64": (lambda: CLIPVisionModelWithProjection(S._clip_cfg(64)), 2, lambda m, x=rnd(2, 3, 28, 28, seed=12): tuple(m(x, return_dict=False))),
        "prior": (lambda: Stage1_PriorTransformer(num_attention_heads=pcfg.num_attention_heads, attention_head_dim=64, num_layers=pcfg.num_layers,
                                                  embedding_dim=1024, num_embeddings=2, additional_embeddings=4), 3,
                  lambda m: (m(px, 457, ppe, psp, ptp).predicted_image_embedding, m(px * 0.5, 12, ppe, psp, ptp).predicted_image_embedding)),
        "pose_embedding": (lambda: ControlNetConditioningEmbedding(320, 3, (16, 32, 96, 256)), 4, lambda m, x=rnd(1, 3, 16, 24, seed=2).tanh(): (m(x),)),
        "image_proj_model_p": (lambda: ImageProjModel_p(128, 64, 64), 5, lambda m, x=rnd(1, 9, 128): (m(x),)),
        "image_projection": (lambda: ImageProjection(128, 64, 4), 6, lambda m, x=rnd(3, 64, seed=7): (m(x),)),
    }


COND_STACK = ("dinov2_swiglu", "dinov2_gelu", "clip_dh80", "clip_dh64", "prior", "pose_embedding", "image_proj_model_p", "image_projection")


@pytest.mark.parametrize("name", COND_STACK)
def test_dirty_memory_cond_stack(backend, name):
    from tests.test_cond_stack_conformance import synth_sd
    build, seed, call = _cond_stack_cases(backend)[name]
    sd = synth_sd(build(), seed=seed)

    def run():
        m = build()
        m.load_state_dict(sd)
        m.to(backend.device)
        return call(m)
    out = _three_fills(backend, run)
    assert all(bool(torch.isfinite(t.float()).all()) for t in out)


def test_dirty_memory_dwpose(backend):
    for R, flip in ((3, True), (1, False)):
        img, boxes, index = _dw_inputs(backend, R)
        _three_fills(backend, lambda: tuple(_dw_estimator(32, 32, 133)(img, boxes, index, flip_test=flip)))


def test_dirty_memory_detector(backend):
    img = _det_images(backend, 3, True)
    _three_fills(backend, lambda: tuple(_detector(64)(img)))


@pytest.mark.parametrize("sched", ["ddim", "unipc"])
def test_dirty_memory_pipeline_one_step(backend, sched):
    """a one-step sampling call of the fused pipeline, classifier-free guidance on (UNet batch 2 N)"""
    from oracle.pipeline import synth_inputs
    from pcdms_amd.pipeline import Stage2_InpaintDiffusionPipeline
    from pcdms_amd.schedulers import DDIMScheduler, UniPCMultistepScheduler
    from tests.test_pipeline import _call
    from tests.test_schedulers import SD21
    topology = "two_level" if backend.is_emu else "tiny"
    cfg = _unet_config(topology)
    N, h, w, L = (1, 8, 8, 4) if backend.is_emu else (2, 16, 24, 9)
    inp = synth_inputs(cfg, h, w, N, L_img=L)
    cls = DDIMScheduler if sched == "ddim" else UniPCMultistepScheduler

    def run():
        pipe = Stage2_InpaintDiffusionPipeline(_unet_model(backend, cfg), cls.from_config(SD21))
        return (_call(pipe, inp, backend.device, N, 1, h, w),)
    out = _three_fills(backend, run)
    assert bool(torch.isfinite(out[0]).all())


def test_dirty_memory_lpips_and_inception(backend):
    a, b = _lpips_images(backend, 3, 1, "u8", 37, 41)
    _three_fills(backend, lambda: tuple(_lpips_model()(a, b, normalize=True, return_layers=True)))
    from tests import test_fid as F
    x = F._dev(F._images(2, 35, 35, 11, "f32"), backend)
    for dims in (64, 192):
        _three_fills(backend, lambda: (_inception_model(dims, False)(x),))


@pytest.mark.parametrize("name", SINGLE_REGION)
def test_dirty_memory_calls(backend, name):
    """``ssim``, ``psnr``, ``absdiff``, ``ssim_box``, ``preprocess.resize``, ``resize_cv_cubic``, ``draw_pose``"""
    _three_fills(backend, _single_region_calls(backend)[name])


# ================================================================================================ B4. the instruments bite (emulator only)
@pytest.fixture
def emu():
    from tests.conftest import Backend
    from tests.emu import build_emu
    _lib.use_library(build_emu.load())
    try:
        yield Backend("emu", torch.device("cpu"))
    finally:
        _lib.lib().pcdm_set_workspace_redzone(0)


def test_a_byte_in_a_red_zone_is_reported(emu):
    """one byte written by the test into a red zone between two calls: reported with the buffer in front of the zone, its offset and the count;
    likewise one byte in an outer guard of a separately owned buffer"""
    lib = _lib.lib()
    m = _lpips_model()
    a, b = _lpips_images(emu, 1, 1, "u8", 31, 31)
    win, wt = (0, 0, 31, 31), m._weights(emu.device)
    assert lib.pcdm_set_workspace_redzone(RZ) == 0
    ent = _entries("pcdm_lpips_ws_layout", 1, 1, 31, 31)
    with Allocs(emu.device, FILL, guard=RZ) as al:
        ws = torch.empty(ops.lpips_ws_bytes(1, 1, 31, 31), dtype=torch.uint8)
        out = torch.empty(1)
        ops.lpips(a, b, win, win, wt, out, None, None, ws, normalize=True)
        _zones_intact(ws, ent, RZ, "lpips")
        name, off, nb = next(e for e in ent if e[0] == "tap2")
        ws[off + nb + 5] = 0x3C                                                # <- the "overrun": 6 bytes past tap2
        ops.lpips(a, b, win, win, wt, out, None, None, ws, normalize=True)
    with pytest.raises(AssertionError, match=rf"behind buffer 'tap2' .* first at workspace byte {off + nb + 5}, 5 bytes past the buffer's end, 1 bytes"):
        _zones_intact(ws, ent, RZ, "lpips")
    al.check()
    al.owned[-1][0][RZ + al.owned[-1][1] + 2] = 0                              # 3 bytes behind the 4-byte output
    with pytest.raises(AssertionError, match=r"guard behind a separately owned float32\[1\] buffer of 4 bytes is damaged: first at byte 6 of the buffer, 1 bytes"):
        al.check()


def test_a_read_of_uninitialised_memory_is_caught(emu):
    def reads_empty():
        return (torch.empty(8, device=emu.device) + 1.0,)

    def writes_first():
        return (torch.empty(8, device=emu.device).fill_(2.0) + 1.0,)

    def allocates_nothing():
        return (torch.zeros(8, device=emu.device) + 1.0,)
    with pytest.raises(AssertionError, match="uninitialised memory is read"):
        _three_fills(emu, reads_empty)
    _three_fills(emu, writes_first)
    with pytest.raises(AssertionError, match="filled nothing"):
        _three_fills(emu, allocates_nothing)
    before = torch.empty
    with Allocs(emu.device, 0xFF) as al:
        assert bool(torch.isnan(torch.empty(3)).all()) and bool(torch.isnan(torch.empty_like(torch.ones(2, 2))).all())
        assert bool(torch.isnan(torch.ones(2).new_empty((2, 3))).all()) and bool(torch.isnan(torch.empty_strided((2, 2), (1, 2))).all())
        assert bool((torch.zeros(4) == 0).all()) and al.count == 4
    assert torch.empty is before


def test_a_shrunk_layout_entry_fails_the_invariants(emu):
    lib = _lib.lib()
    for rz in (0, RZ):
        assert lib.pcdm_set_workspace_redzone(rz) == 0
        cfg = _dwpose_cfg(32, 32, 7)
        total, ent = lib.pcdm_dwpose_ws_bytes(C.byref(cfg), 3, 1), _entries("pcdm_dwpose_ws_layout", C.byref(cfg), 3, 1)
        _check_layout(ent, total, rz)
        i = next(k for k, e in enumerate(ent) if e[0] == "cat")
        shrunk = list(ent)
        shrunk[i] = (ent[i][0], ent[i][1], ent[i][2] - 256)                    # the entry lost one aligned row
        with pytest.raises(AssertionError, match="a hole of 256 bytes"):
            _check_layout(shrunk, total, rz)
        moved = [(n, off - (256 if k > i else 0), nb) for k, (n, off, nb) in enumerate(ent)]   # ... or its neighbours moved up into it
        with pytest.raises(AssertionError, match="overlaps the entry before it"):
            _check_layout(moved, total, rz)
        with pytest.raises(AssertionError, match="beyond the reported total"):
            _check_layout(ent, total - 256, rz)
