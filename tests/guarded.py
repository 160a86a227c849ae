"""Guard pages for operands: tensors that end (or start) where a mapping ends (CPU only; the lane-emulator build reads them like any memory).

``guarded(t, side, align)`` copies a contiguous tensor into anonymous ``mmap`` memory next to a page that ``mprotect`` made ``PROT_NONE``:

* ``side="end"``  : the tensor starts on a multiple of ``align`` bytes and its last byte lies at most ``align - 1`` bytes in front of the
  protected page (exactly in front of it when its size is a multiple of ``align``);
* ``side="start"``: its first byte is the first byte behind the protected page.

``align`` is the smallest alignment include/pcdm.h allows for that pointer.  The gap is a condition, not a measurement: an aligned access of
``align`` bytes cannot cross a page, so a gap below the alignment hides no access that could fault.  A read or write of one byte beyond the
extent on the guarded side ends the process with SIGSEGV (``faulthandler`` prints the Python stack).

``Place`` is the interface the case table of tests/test_operand_containment.py is written against; ``GuardedPlace`` implements it with guard
pages, ``WindowPlace`` (the GPU half) with windows inside larger device buffers whose surroundings hold a chosen byte.  ``GuardedAllocs`` makes
``torch.empty`` and its kin hand out guarded tensors (the outputs the wrappers allocate themselves; every buffer of a whole schedule)."""
from __future__ import annotations

import ctypes
import math
import mmap

import torch

PAGE = mmap.PAGESIZE
PROT_NONE = 0                   # <sys/mman.h>
FILL = 0xFF                     # uninitialised guarded memory: NaN in fp32 / bf16 / e4m3, -1 in the integer tables
_libc = ctypes.CDLL(None, use_errno=True)
_libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
_libc.mprotect.restype = ctypes.c_int


def _up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def guarded_bytes(nbytes: int, side: str = "end", align: int = 16, fill=None) -> tuple:
    """-> (uint8 tensor of ``nbytes`` bytes next to a PROT_NONE page, the gap in bytes between the tensor and that page)"""
    assert side in ("end", "start") and nbytes > 0 and align >= 1 and PAGE % align == 0, (side, nbytes, align)
    body = _up(_up(nbytes, align), PAGE)
    mm = mmap.mmap(-1, body + PAGE, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS, prot=mmap.PROT_READ | mmap.PROT_WRITE)
    base = ctypes.addressof(ctypes.c_char.from_buffer(mm))
    assert base % PAGE == 0
    if side == "end":
        offset, guard, gap = body - _up(nbytes, align), base + body, _up(nbytes, align) - nbytes
    else:
        offset, guard, gap = PAGE, base, 0
    if _libc.mprotect(guard, PAGE, PROT_NONE) != 0:
        raise OSError(ctypes.get_errno(), "mprotect")
    t = torch.frombuffer(mm, dtype=torch.uint8, count=nbytes, offset=offset)   # (keeps ``mm`` alive; the mapping goes when the tensor goes)
    assert t.data_ptr() == base + offset and t.data_ptr() % align == 0
    assert (guard - (t.data_ptr() + nbytes) == gap) if side == "end" else (t.data_ptr() == guard + PAGE)
    if fill is not None:
        t.fill_(fill)
    return t, gap


class Place:
    """Where the operands of one case lie.  ``__call__(t, align)``: a placed copy of contiguous ``t``; ``rows(t, ld, align)``: a placed copy of
    the 2-D ``t`` with row stride ``ld`` whose extent is ``(rows - 1) ld + cols`` elements (the last row is not padded out to ``ld``);
    ``out`` / ``out_rows``: the same for outputs (bytes ``FILL``).  ``count``: operands placed; ``max_gap``: the largest alignment gap."""

    device = torch.device("cpu")

    def __init__(self):
        self.count, self.max_gap = 0, 0

    def _raw(self, nbytes: int, align: int) -> torch.Tensor:
        raise NotImplementedError

    def __call__(self, t, align: int = 16):
        if t is None:
            return None
        t = t.detach().cpu().contiguous()
        if t.numel() == 0:
            return t.to(self.device)
        raw = self._raw(t.numel() * t.element_size(), align)
        raw.copy_(t.reshape(-1).view(torch.uint8))
        return raw.view(t.dtype).view(t.shape)

    def rows(self, t, ld: int, align: int = 16):
        if t is None:
            return None
        R, Cn = t.shape
        assert ld >= Cn
        n = (R - 1) * ld + Cn
        flat = _ORIG["zeros"](n, dtype=t.dtype)
        torch.as_strided(flat, (R, Cn), (ld, 1)).copy_(t)
        return torch.as_strided(self(flat, align), (R, Cn), (ld, 1))

    def out(self, shape, dtype, align: int = 16):
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        return self(torch.full((math.prod(shape) * dtype.itemsize,), FILL, dtype=torch.uint8).view(dtype).view(shape), align)

    def out_rows(self, R: int, Cn: int, ld: int, dtype, align: int = 16):
        n = (R - 1) * ld + Cn
        return torch.as_strided(self.out((n,), dtype, align), (R, Cn), (ld, 1))


class GuardedPlace(Place):
    def __init__(self, side: str):
        super().__init__()
        self.side = side

    def _raw(self, nbytes, align):
        t, gap = guarded_bytes(nbytes, self.side, align)
        self.count += 1
        self.max_gap = max(self.max_gap, gap)
        return t


def guarded(t: torch.Tensor, side: str = "end", align: int = 16) -> torch.Tensor:
    """a copy of contiguous ``t`` in guarded memory (see the module docstring)"""
    assert t.is_contiguous()
    return GuardedPlace(side)(t, align)


class WindowPlace(Place):
    """The GPU half: every operand ends at its exact extent inside a larger device buffer with ``MARGIN`` bytes in front of it and at least
    ``MARGIN`` behind it, all holding ``fill``.  Everything a kernel can reach by a bounded over-read is mapped memory."""

    MARGIN = 4096

    def __init__(self, device, fill: int):
        super().__init__()
        self.device, self.fill = torch.device(device), fill

    def _raw(self, nbytes, align):
        raw = _ORIG["empty"](2 * self.MARGIN + _up(nbytes, 256), dtype=torch.uint8, device=self.device)
        raw.fill_(self.fill)
        self.count += 1
        return raw[self.MARGIN:self.MARGIN + nbytes]

    def __call__(self, t, align: int = 16):
        if t is None:
            return None
        t = t.detach().cpu().contiguous()
        if t.numel() == 0:
            return t.to(self.device)
        raw = self._raw(t.numel() * t.element_size(), align)
        raw.copy_(t.reshape(-1).view(torch.uint8).to(self.device))
        return raw.view(t.dtype).view(t.shape)


_ORIG = {"empty": torch.empty, "zeros": torch.zeros, "empty_like": torch.empty_like, "new_empty": torch.Tensor.new_empty}


class GuardedAllocs:
    """While active, ``torch.empty``, ``torch.zeros``, ``torch.empty_like`` and ``Tensor.new_empty`` on ``place.device`` hand out tensors placed by
    ``place`` (uninitialised ones hold ``FILL`` bytes) -- the pattern of ``Allocs`` in tests/test_workspace_containment.py.  Calls with keyword
    arguments other than ``dtype`` / ``device``, bool tensors and empty shapes go to torch unchanged."""

    def __init__(self, place: Place, align: int = 16):
        self.place, self.align = place, align
        self.count = 0                         # allocations intercepted (``place.count`` holds the operands placed explicitly)

    def _mine(self, device):
        dev = torch.device(device) if device is not None else torch.device("cpu")
        return dev.type == self.place.device.type and not (dev.type == "cuda" and torch.cuda.is_current_stream_capturing())

    def _make(self, shape, dtype, zero):
        shape = tuple(int(v) for v in shape)
        n = math.prod(shape) * dtype.itemsize
        if n == 0 or dtype == torch.bool:
            return (_ORIG["zeros"] if zero else _ORIG["empty"])(shape, dtype=dtype, device=self.place.device)
        raw = self.place._raw(n, self.align)
        self.place.count -= 1                  # (an allocation, not an operand of the case)
        self.count += 1
        raw.fill_(0 if zero else FILL)
        return raw.view(dtype).view(shape)

    @staticmethod
    def _shape(size):
        return size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size

    def __enter__(self):
        plain = {"dtype", "device"}

        def alloc(name, zero):
            def f(*size, **kw):
                if not self._mine(kw.get("device")) or set(kw) - plain:
                    return _ORIG[name](*size, **kw)
                return self._make(self._shape(size), kw.get("dtype") or torch.get_default_dtype(), zero)
            return f

        def empty_like(t, **kw):
            if not self._mine(kw.get("device") or t.device) or set(kw) - plain or not t.is_contiguous() or t.layout != torch.strided:
                return _ORIG["empty_like"](t, **kw)
            return self._make(t.shape, kw.get("dtype") or t.dtype, False)

        def new_empty(t, *size, **kw):
            if not self._mine(kw.get("device") or t.device) or set(kw) - plain:
                return _ORIG["new_empty"](t, *size, **kw)
            return self._make(self._shape(size), kw.get("dtype") or t.dtype, False)

        self._saved = (torch.empty, torch.zeros, torch.empty_like, torch.Tensor.new_empty)
        torch.empty, torch.zeros, torch.empty_like, torch.Tensor.new_empty = alloc("empty", False), alloc("zeros", True), empty_like, new_empty
        return self

    def __exit__(self, *exc):
        torch.empty, torch.zeros, torch.empty_like, torch.Tensor.new_empty = self._saved
        return False


class unpatched:
    """inside ``GuardedAllocs``: torch's own allocators for the duration (host-side preparation of a case: cached case builders, scratch)"""

    def __enter__(self):
        self._saved = (torch.empty, torch.zeros, torch.empty_like, torch.Tensor.new_empty)
        torch.empty, torch.zeros, torch.empty_like, torch.Tensor.new_empty = _ORIG["empty"], _ORIG["zeros"], _ORIG["empty_like"], _ORIG["new_empty"]
        return self

    def __exit__(self, *exc):
        torch.empty, torch.zeros, torch.empty_like, torch.Tensor.new_empty = self._saved
        return False
