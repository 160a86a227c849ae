"""The host side every model class shares: ``HipModel`` owns the fp32 master weights, the packed device weights, the scratch buffers and
the slice of the ``torch.nn.Module`` surface the reference's drivers / pipelines touch on their model objects (``.to()``, ``.eval()``,
``.half()``, ``.cuda()``, ``.requires_grad_(False)``, ``.parameters()``, ``.modules()``, ``state_dict`` / ``load_state_dict`` ...), for
classes whose weights live as packed bf16 device buffers rather than ``nn.Parameter``s.  Inference only: ``train(True)`` raises.
Plus the three things every ``from_pretrained`` does: read ``config.json``, read the checkpoint file, PyTorch-default fresh init."""
from __future__ import annotations

import itertools
import json
import math
from pathlib import Path
from types import SimpleNamespace
from typing import Any, Dict, Optional, Sequence, Tuple

import torch

from . import _lib
from .ops import BF16

#: process-wide serial numbers of model and context objects.  A long-lived caller (a pipeline's captured graph) that has to tell "the same
#: model" from "another model" compares these, never ``id()``: CPython hands the address of a dropped object to the next one built.
_SERIAL = itertools.count(1)


def next_serial() -> int:
    return next(_SERIAL)


class Config(SimpleNamespace):
    """``model.config``: attribute, item and ``get`` access, ``keys()`` (so ``dict(config)`` works)."""

    def __getitem__(self, k):
        return getattr(self, k)

    def get(self, k, d=None):
        return getattr(self, k, d)

    def keys(self):
        return self.__dict__.keys()


def read_config(d, defaults: Dict[str, Any], known=None) -> Dict[str, Any]:
    """``defaults`` overlaid with the entries of ``d/config.json`` (when there is one) whose key is in ``known`` (default: in
    ``defaults``) or starts with "_" (``_class_name``, ``_diffusers_version``)."""
    cfg = dict(defaults)
    path = Path(d) / "config.json"
    if path.exists():
        known = cfg if known is None else known
        cfg.update({k: v for k, v in json.loads(path.read_text()).items() if k in known or k.startswith("_")})
    return cfg


def read_checkpoint(d, stems: Sequence[str]) -> Optional[Dict[str, torch.Tensor]]:
    """The state dict in the first of ``d/<stem>.safetensors``, ``d/<stem>.bin`` (stems in order) that exists, else ``None``."""
    for stem in stems:
        if (Path(d) / f"{stem}.safetensors").exists():
            from safetensors.torch import load_file
            return load_file(str(Path(d) / f"{stem}.safetensors"))
        if (Path(d) / f"{stem}.bin").exists():
            return torch.load(str(Path(d) / f"{stem}.bin"), map_location="cpu")
    return None


def default_init(expected_shapes: Dict[str, Tuple[int, ...]], seed: int = 0, zeros: Sequence[str] = (), divide: bool = False):
    """PyTorch-default fresh initialisation (what ``from_pretrained`` leaves in tensors the checkpoint does not supply): U(-b, b) with
    b = 1 / sqrt(fan_in) for a multi-dimensional weight and its bias, ones / zeros for a norm's weight / bias, zeros for ``zeros``.  One
    generator, consumed in the iteration order of ``expected_shapes``.  ``divide``: scale as ``u / sqrt(fan_in)`` instead of
    ``u * (1 / sqrt(fan_in))`` -- the two round differently, and each model's fresh values are pinned bit for bit
    (tests/golden/fresh_init_sha256.json): the prior has always divided."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in expected_shapes.items():
        wshape = () if k in zeros else expected_shapes[k[: k.rfind(".") + 1] + "weight"]
        if k in zeros:
            sd[k] = torch.zeros(shp)
        elif len(wshape) == 1:
            sd[k] = torch.ones(shp) if k.endswith("weight") else torch.zeros(shp)
        else:
            u, s = torch.rand(shp, generator=g) * 2 - 1, math.sqrt(math.prod(wshape[1:]))
            sd[k] = u / s if divide else u * (1.0 / s)
    return sd


class HipModel:
    training = False
    _reshape_same_numel = False   # load_state_dict: accept a tensor of another shape with the expected number of elements (reshaped)

    def __init__(self):
        self._serial = next_serial()
        self._device = torch.device("cpu")
        self._dtype = torch.float32                              # I/O dtype only; arithmetic is bf16 x bf16 -> fp32 on MFMA
        self._sd: Optional[Dict[str, torch.Tensor]] = None       # fp32 CPU master copy (the checkpoint's key names)
        self._w: Optional[Dict[str, Any]] = None                 # packed device weights (``_pack``)
        self._bufs: Dict[Tuple, torch.Tensor] = {}               # scratch, keyed (name, shape, dtype): static addresses per input shape

    def expected_shapes(self) -> Dict[str, Tuple[int, ...]]:
        raise NotImplementedError

    def _invalidate(self):
        """Hook: drop whatever a subclass derived from the weights or the device (called when either changes)."""

    def _remap_keys(self, sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Hook: rename / drop keys of an incoming state dict (older checkpoint layouts)."""
        return sd

    # ---------------------------------------------------------------- nn.Module-like surface
    @property
    def device(self):
        return self._device

    @property
    def dtype(self):
        return self._dtype

    def to(self, *args, **kwargs):
        device, dtype = kwargs.get("device"), kwargs.get("dtype")
        for a in args:
            if isinstance(a, torch.dtype):
                dtype = a
            elif a is not None:
                device = a
        if dtype is not None:
            self._dtype = dtype
        if device is not None and torch.device(device) != self._device:
            self._device = torch.device(device)
            if self._device.type == "cuda" and self._device.index is None:
                self._device = torch.device("cuda", torch.cuda.current_device())
            self._w = None
            self._bufs.clear()
            self._invalidate()
        return self

    def eval(self):
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("pcdms_amd models are inference-only (training is out of scope: SURVEY.md §2 rows 6, 14)")
        return self

    def requires_grad_(self, requires_grad: bool = False):
        if requires_grad:
            raise NotImplementedError("pcdms_amd models are inference-only")
        return self

    def half(self):
        return self.to(torch.float16)

    def float(self):
        return self.to(torch.float32)

    def cuda(self, device=None):
        return self.to(torch.device("cuda", torch.cuda.current_device() if device is None else device))

    def modules(self):
        yield self

    def named_parameters(self):
        """(name, fp32 host tensor) of the loaded state dict -- what ``sum(p.numel() for p in m.parameters())`` needs."""
        yield from self.state_dict().items()

    def parameters(self):
        for _, v in self.named_parameters():
            yield v

    # ---------------------------------------------------------------- weights
    def state_dict(self) -> Dict[str, torch.Tensor]:
        return dict(self._sd or {})

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        """Keys absent from a non-strict load keep their current value."""
        exp = self.expected_shapes()
        sd = self._remap_keys(dict(state_dict))
        missing = [k for k in exp if k not in sd]
        unexpected = [k for k in sd if k not in exp]
        bad = [f"{k}: {tuple(sd[k].shape)} vs {tuple(exp[k])}" for k in exp if k in sd and tuple(sd[k].shape) != tuple(exp[k])
               and not (self._reshape_same_numel and sd[k].numel() == math.prod(exp[k]))]
        if bad or (strict and (missing or unexpected)):
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}:\n"
                               f"  Missing key(s): {missing[:8]}{'...' if len(missing) > 8 else ''}\n"
                               f"  Unexpected key(s): {unexpected[:8]}{'...' if len(unexpected) > 8 else ''}\n"
                               f"  size mismatch: {bad[:8]}")
        old = self._sd or {}
        self._sd = {k: sd[k].detach().to("cpu", torch.float32).reshape(exp[k]) if k in sd else old[k] for k in exp if k in sd or k in old}
        self._w = None
        self._invalidate()
        return SimpleNamespace(missing_keys=missing, unexpected_keys=unexpected)

    def _ready(self):
        """First line of every ``_pack``."""
        if self._sd is None:
            raise RuntimeError("weights not loaded: call load_state_dict / from_pretrained first")
        if self._device.type != "cuda" and not _lib.is_emulator():
            raise RuntimeError(f"{type(self).__name__} runs on the MI355X only: call .to('cuda') (there is no CPU implementation)")

    def _tap(self, name: str, t: torch.Tensor) -> torch.Tensor:
        """Test hook (tests/test_cond_stack_conformance.py): with ``self._taps`` set to a dict, a clone of ``t`` -- a tensor a later launch
        reads -- is recorded under ``name``.  ``None`` (always, outside that test): nothing is cloned, nothing is launched."""
        taps = getattr(self, "_taps", None)
        if taps is not None:
            taps[name] = t.clone()
        return t

    def _buf(self, name: str, shape, dtype=BF16, zero: bool = False) -> torch.Tensor:
        key = (name, tuple(shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            t = self._bufs[key] = (torch.zeros if zero else torch.empty)(tuple(shape), dtype=dtype, device=self._device)
        return t
