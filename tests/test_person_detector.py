"""The person detector on the device (pcdms_amd/pose.py: PersonDetector, detect_people, estimate_pose_map(detector=...); csrc/detect.hip).

The yardstick is an fp64 restatement of the network with ``torch.nn.functional`` on the CPU (``Ref`` below), written from the definition in
include/pcdm.h (mmdet's CSPDarknet, YOLOXPAFPN, YOLOXHead, ``predict_by_feat``; mmcv's and mmpose's ``nms``) on SYNTHETIC seeded state dicts
under mmdet's key names: He-scaled weights, BatchNorm gamma in U(0.5, 1.5), beta in U(-0.1, 0.1), running statistics calibrated on a seeded batch
(as tests/test_dwpose.py does), and head biases chosen so that the selection case's condition holds (some priors pass the thresholds, some do
not, some boxes overlap enough to be suppressed).  mmdet and the published checkpoint are not available: parity with mmdet on its weights is a
dormant pin at the end of this file.

Method and bounds are tests/test_dwpose.py's: e = max |got - want| / max |want| against the fp64 restatement must satisfy e_dev <= 16 e_ref, e_ref
the same error of the restatement run in fp32 on the CPU (convolution, then unfused BatchNorm); a restatement whose operands are rounded to bf16
must EXCEED that bound; named faults must move their stage beyond 32 e_ref.  The network is checked stage by stage with teacher forcing through
the ``_taps`` hook.  The decode's e is normalised by S and its e_ref floored at one fp32 ulp.  The GPU tests write their figures to
profiles/yolox_values.json.  Measured on the MI355X: device / e_ref is at most 3.0 over the stages of the tiny network (neck.p5.csp.in), 3.9 for the
decoded boxes, and 1.1 / 6.9 / 7.2 for the full-width stem, head and stage-4 3 x 3 layers.
"""
from __future__ import annotations

import functools
import json
import math
import os
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
FACTOR = 16.0
BITE = 2.0 * FACTOR
ULP = 2.0 ** -23
BF = torch.bfloat16
BN = ("weight", "bias", "running_mean", "running_var")
# CSPDarknet's P5 arch_settings (in, out, blocks, identity, spp), spelled out here and not read from the product
ARCH_P5 = ((64, 128, 3, True, False), (128, 256, 9, True, False), (256, 512, 9, True, False), (512, 1024, 3, False, True))


def _dev(a, backend):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(backend.device)


def _err(got, want):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return ((got - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


def _q(operand):
    return (lambda t: t) if operand is None else (lambda t: t.to(operand).to(t.dtype))


def _record(key, value):
    path = ROOT / "profiles" / "yolox_values.json"
    try:
        values = json.loads(path.read_text()) if path.exists() else {}
        values[key] = value
        path.write_text(json.dumps(values, indent=1, sort_keys=True) + "\n")
    except OSError:
        pass                                                                   # a read-only checkout still runs the assertions


def _images(N, H, W, seed, noise=0.12):
    """smooth structure + noise, uint8 NHWC"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    imgs = []
    for n in range(N):
        ph = rng.uniform(0, 6.28, 3)
        base = np.stack([0.5 + 0.35 * np.sin(x / (9.0 + n) + p) * np.cos(y / (7.0 + c) + 2 * p) for c, p in enumerate(ph)], -1)
        imgs.append(np.clip(base + rng.normal(0, noise, base.shape), 0, 1))
    return np.ascontiguousarray(np.rint(np.stack(imgs) * 255).astype(np.uint8))


# ------------------------------------------------------------------------------------------------ the restatement: input
def resized(H, W, S):
    f = float(S) / float(max(H, W))
    return int(H * f + 0.5), int(W * f + 0.5)


def _lin_coeff(n_out, n_in, clamp_frac):
    """the stated rule of pcdm_resize_linear_u8 for one axis -> (s0, s1, w0, w1) per output index"""
    scale = 1.0 / (float(n_out) / float(n_in))
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    fl = np.floor(f)
    s, t = fl.astype(np.int64), (f - fl).astype(np.float32)
    if clamp_frac:
        lo, hi = s < 0, s >= n_in - 1
        t[lo | hi] = 0
        s[lo], s[hi] = 0, n_in - 1
    w0, w1 = np.rint((np.float32(1) - t) * np.float32(2048)).astype(np.int64), np.rint(t * np.float32(2048)).astype(np.int64)
    return np.clip(s, 0, n_in - 1), np.clip(s + 1, 0, n_in - 1), w0, w1


def prep_ref(img, S, faults=()):
    """uint8 RGB [N, H, W, 3] -> the Focus tensor fp32 [N, S/2, S/2, 12]: OpenCV's 8-bit INTER_LINEAR into (Wr, Hr), top-left in a 114 canvas, B G R,
    patches (top-left, bottom-left, top-right, bottom-right)"""
    N, H, W, _ = img.shape
    Hr, Wr = resized(H, W, S)
    xa, xb, a0, a1 = _lin_coeff(Wr, W, True)
    ya, yb, b0, b1 = _lin_coeff(Hr, H, False)
    src = img.astype(np.int64)
    S0 = src[:, ya][:, :, xa] * a0[None, None, :, None] + src[:, ya][:, :, xb] * a1[None, None, :, None]
    S1 = src[:, yb][:, :, xa] * a0[None, None, :, None] + src[:, yb][:, :, xb] * a1[None, None, :, None]
    small = (((b0[None, :, None, None] * (S0 >> 4)) >> 16) + ((b1[None, :, None, None] * (S1 >> 4)) >> 16) + 2) >> 2
    canvas = np.full((N, S, S, 3), 0 if "border_0" in faults else 114, np.int64)
    canvas[:, :Hr, :Wr] = np.clip(small, 0, 255)
    if "rgb" not in faults:
        canvas = canvas[..., ::-1]                                             # B, G, R
    order = ((0, 0), (0, 1), (1, 0), (1, 1)) if "focus_order" in faults else ((0, 0), (1, 0), (0, 1), (1, 1))
    return np.concatenate([canvas[:, dy::2, dx::2] for dy, dx in order], -1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the restatement: network
class Ref:
    """The network as a list of stages over LOGICAL NCHW tensors: ``stages()`` yields (name, input names, fn(dtype, q, faults, *inputs)), the names
    those of the product's taps; ``chain`` runs them from the Focus tensor.  A level's head tensor is cat [reg 4, obj 1, classes C]."""

    def __init__(self, sd, *, size, widen, deepen, classes, bn_eps=1e-3):
        self.sd, self.S, self.C, self.eps = sd, size, classes, bn_eps
        self.stem, self.head = int(64 * widen), int(256 * widen)
        self.arch = [(int(ci * widen), int(co * widen), max(round(nb * deepen), 1), ident, spp) for ci, co, nb, ident, spp in ARCH_P5]
        self.neck_blocks = max(round(3 * deepen), 1)
        self.calib = None

    def cm(self, name, x, dt, q, faults, stride=1, pad=0):
        sd = self.sd
        h = F.conv2d(q(x), q(sd[f"{name}.conv.weight"].to(dt)), None, stride=stride, padding=pad)
        if self.calib is not None:                                             # (once, while the weights are made: see the module docstring)
            co, var = h.shape[1], h.var((0, 2, 3))
            sd[f"{name}.bn.running_var"] = (var * (torch.rand(co, generator=self.calib) + 0.5)).float().clamp_min(1e-12)
            sd[f"{name}.bn.running_mean"] = (h.mean((0, 2, 3)) + (torch.rand(co, generator=self.calib) * 2 - 1) * 0.3 * var.sqrt()).float()
        m, v, g, b = (sd[f"{name}.bn.{k}"].to(dt) for k in ("running_mean", "running_var", "weight", "bias"))
        return F.silu(F.batch_norm(h, m, v, g, b, False, 0.0, 1e-5 if "bn_eps" in faults else self.eps))

    def plain(self, name, x, dt, q):
        return F.conv2d(q(x), q(self.sd[f"{name}.weight"].to(dt)), self.sd[f"{name}.bias"].to(dt))

    def _csp(self, add, tag, n, src, cout, nb, ident):
        cm, mid = self.cm, cout // 2

        def csp_in(dt, q, f, x, n=n):
            a, b = cm(f"{n}.main_conv", x, dt, q, f), cm(f"{n}.short_conv", x, dt, q, f)
            return torch.cat([b, a] if "concat_swapped" in f else [a, b], 1)
        add(f"{tag}.csp.in", (src,), csp_in)
        cat = f"{tag}.csp.in"
        for b in range(nb):
            add(f"{tag}.blocks.{b}.conv1", (cat,), lambda dt, q, f, x, n=n, b=b: cm(f"{n}.blocks.{b}.conv1", x[:, :mid], dt, q, f))

            def block(dt, q, f, t, c, n=n, b=b):
                y = cm(f"{n}.blocks.{b}.conv2", t, dt, q, f, pad=1)
                if ident or "identity_everywhere" in f:
                    y = y + c[:, :mid]
                return torch.cat([y, c[:, mid:]], 1)
            add(f"{tag}.blocks.{b}", (f"{tag}.blocks.{b}.conv1", cat), block)
            cat = f"{tag}.blocks.{b}"
        add(tag, (cat,), lambda dt, q, f, x, n=n: cm(f"{n}.final_conv", x, dt, q, f))

    def stages(self):
        cm, nb = self.cm, self.neck_blocks
        out = []
        add = lambda name, ins, fn: out.append((name, ins, fn))   # noqa: E731
        add("stem", ("focus",), lambda dt, q, f, x: cm("backbone.stem.conv", x, dt, q, f, pad=1))
        prev = "stem"
        for s, (_, co, blocks, ident, spp) in enumerate(self.arch, 1):
            add(f"stage{s}.down", (prev,), lambda dt, q, f, x, s=s: cm(f"backbone.stage{s}.0", x, dt, q, f, stride=2, pad=1))
            prev = f"stage{s}.down"
            if spp:
                def spp_cat(dt, q, f, x, s=s):
                    h = cm(f"backbone.stage{s}.1.conv1", x, dt, q, f)
                    return torch.cat([h] + [F.max_pool2d(h, k, 1, k // 2) for k in (5, 9, 13)], 1)
                add(f"stage{s}.spp.cat", (prev,), spp_cat)
                add(f"stage{s}.spp", (f"stage{s}.spp.cat",), lambda dt, q, f, x, s=s: cm(f"backbone.stage{s}.1.conv2", x, dt, q, f))
                prev = f"stage{s}.spp"
            self._csp(add, f"stage{s}", f"backbone.stage{s}.{2 if spp else 1}", prev, co, blocks, ident)
            prev = f"stage{s}"
        o1, o2, o3 = self.arch[1][1], self.arch[2][1], self.arch[3][1]
        up2 = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")   # noqa: E731
        add("neck.td0.cat", ("stage4", "stage3"), lambda dt, q, f, c5, c4: torch.cat([up2(cm("neck.reduce_layers.0", c5, dt, q, f)), c4], 1))
        self._csp(add, "neck.t4", "neck.top_down_blocks.0", "neck.td0.cat", o2, nb, False)
        add("neck.td1.cat", ("neck.t4", "stage2"), lambda dt, q, f, t4, c3: torch.cat([up2(cm("neck.reduce_layers.1", t4, dt, q, f)), c3], 1))
        self._csp(add, "neck.p3", "neck.top_down_blocks.1", "neck.td1.cat", o1, nb, False)

        def bottom_up(i, lateral_src):
            def fn(dt, q, f, p, lat):
                parts = [cm(f"neck.downsamples.{i}", p, dt, q, f, stride=2, pad=1), cm(f"neck.reduce_layers.{1 - i}", lat, dt, q, f)]
                return torch.cat(parts[::-1] if "lateral_first" in f else parts, 1)
            return fn
        add("neck.bu0.cat", ("neck.p3", "neck.t4"), bottom_up(0, "neck.t4"))           # [down(p3), r4]
        self._csp(add, "neck.p4", "neck.bottom_up_blocks.0", "neck.bu0.cat", o2, nb, False)
        add("neck.bu1.cat", ("neck.p4", "stage4"), bottom_up(1, "stage4"))             # [down(p4), r5]
        self._csp(add, "neck.p5", "neck.bottom_up_blocks.1", "neck.bu1.cat", o3, nb, False)
        for i in range(3):
            add(f"head.{i}.f", (f"neck.p{3 + i}",), lambda dt, q, f, x, i=i: cm(f"neck.out_convs.{i}", x, dt, q, f))
            for t in ("cls", "reg"):
                add(f"head.{i}.{t}.0", (f"head.{i}.f",), lambda dt, q, f, x, i=i, t=t: cm(f"bbox_head.multi_level_{t}_convs.{i}.0", x, dt, q, f, pad=1))
                add(f"head.{i}.{t}.1", (f"head.{i}.{t}.0",), lambda dt, q, f, x, i=i, t=t: cm(f"bbox_head.multi_level_{t}_convs.{i}.1", x, dt, q, f, pad=1))

            def head(dt, q, f, c, r, i=i):
                pre = "bbox_head.multi_level_conv_"
                if self.calib is not None:   # biases: class 0 mostly wins and its score straddles 0.5; boxes a few strides wide, so neighbours overlap
                    sd = self.sd
                    sd[f"{pre}cls.{i}.bias"] = torch.cat([torch.tensor([0.5]), torch.full((self.C - 1,), -1.0)]) + torch.randn(self.C, generator=self.calib) * 0.1
                    sd[f"{pre}obj.{i}.bias"] = torch.tensor([0.5])
                    sd[f"{pre}reg.{i}.bias"] = torch.tensor([0.0, 0.0, 1.9, 1.9]) + torch.randn(4, generator=self.calib) * 0.1
                    for t, x in (("cls", c), ("reg", r), ("obj", r)):             # logits within +-2.5 of the biases (the features are heavy-tailed)
                        sd[f"{pre}{t}.{i}.weight"] = (sd[f"{pre}{t}.{i}.weight"].to(dt) * 2.5 / F.conv2d(x, sd[f"{pre}{t}.{i}.weight"].to(dt)).abs().max()).float()
                obj = self.plain(f"{pre}obj.{i}", c if "obj_from_cls" in f else r, dt, q)
                return torch.cat([self.plain(f"{pre}reg.{i}", r, dt, q), obj, self.plain(f"{pre}cls.{i}", c, dt, q)], 1)
            add(f"head.{i}", (f"head.{i}.cls.1", f"head.{i}.reg.1"), head)
        return out

    def chain(self, focus, dt=torch.float64, operand=None, faults=()):
        """focus: logical [N, 12, S/2, S/2] -> {name: logical tensor}"""
        T = {"focus": focus.to(dt)}
        for name, ins, fn in self.stages():
            T[name] = fn(dt, _q(operand), faults, *[T[i] for i in ins])
        return T


# ------------------------------------------------------------------------------------------------ the restatement: decode and selection
def decode_ref(heads, S, H, W, class_id, score_thr, dt, faults=()):
    """logical head tensors [N, 5 + C, h, w] (numpy) -> (boxes [N, P, 4], scores [N, P], labels [N, P], candidates [N, P]) computed in ``dt``, every
    operation its own"""
    Hr, Wr = resized(H, W, S)
    sfx, sfy = dt(np.float32(Wr / W)), dt(np.float32(Hr / H))
    if "scale_swapped" in faults:
        sfx, sfy = sfy, sfx
    boxes, scores, labels = [], [], []
    for h, stride in zip(heads, (8, 16, 32)):
        N, hw = h.shape[0], h.shape[2]
        v = np.asarray(h, dt).transpose(0, 2, 3, 1).reshape(N, hw * hw, -1)
        st = dt(stride)
        ys, xs = np.divmod(np.arange(hw * hw), hw)
        off = dt(0.5) if "prior_offset" in faults else dt(0)
        px, py = (xs.astype(dt) + off) * st, (ys.astype(dt) + off) * st
        cx, cy = v[..., 0] * st + px, v[..., 1] * st + py
        w, hh = (v[..., 2:4] if "no_exp" in faults else np.exp(v[..., 2:4])).transpose(2, 0, 1) * st
        sig = lambda t: dt(1) / (dt(1) + np.exp(-t))   # noqa: E731
        cls = sig(v[..., 5:])
        labels.append(np.argmax(cls, -1))
        scores.append((np.max(cls, -1) * sig(v[..., 4])).astype(dt))
        half = dt(0.5)
        b = np.stack([cx - w * half, cy - hh * half, cx + w * half, cy + hh * half], -1).astype(dt)
        boxes.append(b if "rescale_late" in faults else b / np.array([sfx, sfy, sfx, sfy], dt))
    boxes, scores, labels = np.concatenate(boxes, 1), np.concatenate(scores, 1), np.concatenate(labels, 1)
    cand = (labels == class_id) & (scores >= dt(0.01)) & (scores > dt(score_thr))
    return boxes, scores, labels, cand


def iou_matrix(b, off):
    b = np.asarray(b, np.float64)
    area = (b[:, 2] - b[:, 0] + off) * (b[:, 3] - b[:, 1] + off)
    w = np.clip(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]) + off, 0, None)
    h = np.clip(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]) + off, 0, None)
    with np.errstate(invalid="ignore", divide="ignore"):
        return w * h / (area[:, None] + area[None, :] - w * h)


def greedy_ref(boxes, scores, flags, thr, off, max_cand=10 ** 9, ge=False, used=None):
    """one greedy pass over the flagged boxes of ONE image in (score descending, index ascending) order -> the kept indices in that order; ``used``
    (a list): every IoU that was compared with ``thr`` is appended"""
    order = sorted(np.flatnonzero(flags), key=lambda i: (-float(scores[i]), int(i)))[:max_cand]
    iou = iou_matrix(np.asarray(boxes)[order], off)
    kept = []
    for a in range(len(order)):
        hit = False
        for k in kept:
            if used is not None:
                used.append(iou[k, a])
            if iou[k, a] >= thr if ge else iou[k, a] > thr:
                hit = True
                break
        if not hit:
            kept.append(a)
    return [int(order[a]) for a in kept]


def select_ref(boxes, scores, cand, nms_thr=0.65, pose_thr=0.7, faults=(), used=None):
    """mmcv's nms (offset 0), then mmpose's over the survivors (+1) -> the kept indices of one image in score order"""
    first = greedy_ref(boxes, scores, cand, nms_thr, 1.0 if "first_offset_1" in faults else 0.0, used=used)
    flags = np.zeros(len(scores), bool)
    flags[first] = True
    return greedy_ref(boxes, scores, flags, pose_thr, 1.0, ge="ge" in faults, used=used)


# ------------------------------------------------------------------------------------------------ synthetic weights
def _shapes(kw):
    """every key of mmdet's state dict for the configuration -> shape; written out here, and test_state_dict holds the product's own list to it"""
    wf, df, C = kw.get("widen_factor", 1.0), kw.get("deepen_factor", 1.0), kw.get("num_classes", 80)
    sh = {}

    def conv_module(name, co, ci, k):
        sh[f"{name}.conv.weight"] = (co, ci, k, k)
        sh.update({f"{name}.bn.{b}": (co,) for b in BN})

    def csp(name, ci, co, nb):
        mid = co // 2
        conv_module(f"{name}.main_conv", mid, ci, 1)
        conv_module(f"{name}.short_conv", mid, ci, 1)
        conv_module(f"{name}.final_conv", co, 2 * mid, 1)
        for b in range(nb):
            conv_module(f"{name}.blocks.{b}.conv1", mid, mid, 1)
            conv_module(f"{name}.blocks.{b}.conv2", mid, mid, 3)
    conv_module("backbone.stem.conv", int(64 * wf), 12, 3)
    outs = []
    for s, (ci, co, nb, _, spp) in enumerate(ARCH_P5, 1):
        ci, co, nb = int(ci * wf), int(co * wf), max(round(nb * df), 1)
        outs.append(co)
        conv_module(f"backbone.stage{s}.0", co, ci, 3)
        if spp:
            conv_module(f"backbone.stage{s}.1.conv1", co // 2, co, 1)
            conv_module(f"backbone.stage{s}.1.conv2", co, 2 * co, 1)
        csp(f"backbone.stage{s}.{2 if spp else 1}", co, co, nb)
    _, o1, o2, o3 = outs
    nb, hc = max(round(3 * df), 1), int(256 * wf)
    conv_module("neck.reduce_layers.0", o2, o3, 1)
    conv_module("neck.reduce_layers.1", o1, o2, 1)
    csp("neck.top_down_blocks.0", 2 * o2, o2, nb)
    csp("neck.top_down_blocks.1", 2 * o1, o1, nb)
    conv_module("neck.downsamples.0", o1, o1, 3)
    conv_module("neck.downsamples.1", o2, o2, 3)
    csp("neck.bottom_up_blocks.0", 2 * o1, o2, nb)
    csp("neck.bottom_up_blocks.1", 2 * o2, o3, nb)
    for i, c in enumerate((o1, o2, o3)):
        conv_module(f"neck.out_convs.{i}", hc, c, 1)
        for j in range(2):
            conv_module(f"bbox_head.multi_level_cls_convs.{i}.{j}", hc, hc, 3)
            conv_module(f"bbox_head.multi_level_reg_convs.{i}.{j}", hc, hc, 3)
        for t, co in (("cls", C), ("reg", 4), ("obj", 1)):
            sh[f"bbox_head.multi_level_conv_{t}.{i}.weight"], sh[f"bbox_head.multi_level_conv_{t}.{i}.bias"] = (co, hc, 1, 1), (co,)
    return sh


def _ref(sd, kw):
    return Ref(sd, size=kw["size"], widen=kw.get("widen_factor", 1.0), deepen=kw.get("deepen_factor", 1.0), classes=kw.get("num_classes", 80))


def synth_state_dict(kw, seed, calib_size=None, calib_images=32, calib_dt=torch.float64, calib_noise=0.12, calib_shape=None):
    """a seeded state dict under mmdet's key names, its BatchNorm statistics and head layers calibrated on ``calib_images`` seeded images at the
    detector size ``calib_size`` (default: the configuration's own)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in _shapes(kw).items():
        if k.endswith("weight") and len(shp) == 4:
            sd[k] = torch.randn(shp, generator=g) * math.sqrt(2.0 / math.prod(shp[1:]))
        elif k.endswith("bn.weight") or k.endswith("running_var"):
            sd[k] = torch.rand(shp, generator=g) + 0.5
        else:                                                                  # biases, bn.bias, running_mean
            sd[k] = (torch.rand(shp, generator=g) * 2 - 1) * 0.1
    S = calib_size or kw["size"]
    ref = _ref(sd, kw)
    H, W = calib_shape or (S - 13, S // 2 + 2)                                # (the share of the 114 border is part of the statistics)
    focus = prep_ref(_images(calib_images, H, W, seed + 1, calib_noise), S)   # (the deep maps are 3 x 3: many images, or their statistics are noise)
    ref.calib = g
    ref.chain(torch.from_numpy(focus).permute(0, 3, 1, 2), dt=calib_dt)
    ref.calib = None
    for k in list(sd):
        if k.endswith("running_var"):
            sd[k[:-len("running_var")] + "num_batches_tracked"] = torch.tensor(7)
    return sd


TINY = dict(size=96, widen_factor=0.125, deepen_factor=1.0 / 3.0, num_classes=5)   # channels 8 .. 128, blocks 1, 3, 3, 1; levels 12^2, 6^2, 3^2
SRC_H, SRC_W = 83, 50                                                              # a non-square source: Wr = 58 != Hr = 96, a 114 border
SEED = 9


@functools.lru_cache(maxsize=None)
def _tiny():
    sd = synth_state_dict(TINY, SEED)
    return sd, _ref(sd, TINY)


@functools.lru_cache(maxsize=None)
def _detector(**over):
    from pcdms_amd import pose
    return pose.PersonDetector(_tiny()[0], **{**TINY, **dict(over)})


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """-> (the two test images, the fp64 chain's tensors from the stated rule's Focus tensor)"""
    _, ref = _tiny()
    img = _images(2, SRC_H, SRC_W, 11)
    return img, ref.chain(torch.from_numpy(prep_ref(img, TINY["size"])).permute(0, 3, 1, 2))


def _heads_np(T, dt=np.float64):
    return [T[f"head.{i}"].numpy().astype(dt) for i in range(3)]


# ------------------------------------------------------------------------------------------------ 1. per-kernel tests
@pytest.mark.parametrize("H,W,S", [(SRC_H, SRC_W, 96), (96, 40, 96), (37, 64, 64), (21, 30, 64)])
def test_prep(backend, H, W, S):
    """byte-exact against the stated rule: the non-square source, sources that are already S on their long side, an upscaled one"""
    from pcdms_amd import ops
    img = _images(2, H, W, H + W)
    want = prep_ref(img, S)
    got = ops.detect_prep(_dev(img, backend), S)
    backend.sync()
    Hr, Wr = resized(H, W, S)
    assert ops.detect_resized(H, W, S) == (Hr, Wr) and max(Hr, Wr) == S
    assert np.array_equal(got.cpu().numpy(), want)
    if max(H, W) == S:                                                         # nothing to resize: the canvas holds the pixels themselves
        assert np.array_equal(want[:, :, :, 0:3][:, :H // 2, :W // 2], img[:, 0:2 * (H // 2):2, 0:2 * (W // 2):2, ::-1].astype(np.float32))
    if Wr < S:
        assert (want[:, :, (Wr + 1) // 2:] == 114).all()
    for fault in ("focus_order", "rgb", "border_0"):                           # each named fault changes bytes, so the exact comparison sees it
        assert not np.array_equal(prep_ref(img, S, (fault,)), want), fault
    with pytest.raises(RuntimeError, match="code -1"):
        ops.detect_prep(_dev(img, backend), S + 8)
    with pytest.raises(ValueError):
        ops.detect_resized(4096, 1, 64)                                        # a side that would vanish


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (12, 9)])
def test_upsample_to_slice(backend, H, W):
    from pcdms_amd import ops
    C = 8
    x = torch.randn(2, H, W, C + 4, generator=torch.Generator().manual_seed(H))
    out = torch.full((2, 2 * H, 2 * W, C + 8), -5.5)
    d = _dev(out, backend)
    ops.upsample2_nearest_f32(_dev(x, backend), C, d, in_offset=4, offset=4)
    backend.sync()
    got = d.cpu()
    want = F.interpolate(x[..., 4:].permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(got[..., 4:4 + C], want) and (got[..., :4] == -5.5).all() and (got[..., 4 + C:] == -5.5).all()
    # an input and an output slice of ONE tensor (one base address, one pitch) that overlap are refused, and nothing is written; so is an offset
    # that is no multiple of 4
    from pcdms_amd import _lib
    t = _dev(torch.full((1, 4, 4, 16), 2.5), backend)
    assert _lib.lib().pcdm_upsample2_nearest_f32(t.data_ptr(), 1, 2, 2, 8, 16, 0, t.data_ptr(), 16, 4, None) == -1
    backend.sync()
    assert (t.cpu() == 2.5).all()
    with pytest.raises(RuntimeError, match="code -1"):
        ops.upsample2_nearest_f32(_dev(x, backend), C, d, in_offset=2, offset=4)


# hand-made candidate sets: (boxes, scores, flags) of one image
def _nms_run(backend, boxes, scores, flags, thr, off, max_cand=64, max_det=64):
    from pcdms_amd import ops
    b = torch.tensor(boxes, dtype=torch.float32).reshape(1, -1, 4)
    r = ops.nms_f32(_dev(b, backend), _dev(torch.tensor(scores, dtype=torch.float32).reshape(1, -1), backend),
                    _dev(torch.tensor(flags, dtype=torch.int32).reshape(1, -1), backend), thr=thr, offset=off, max_candidates=max_cand, max_det=max_det)
    backend.sync()
    return {k: v.cpu().numpy()[0] for k, v in r.items()}


def _nms_check(backend, boxes, scores, flags, thr, off, max_cand=64, max_det=64):
    r = _nms_run(backend, boxes, scores, flags, thr, off, max_cand, max_det)
    kept = greedy_ref(boxes, scores, flags, thr, off, max_cand)
    n = min(len(kept), max_det)
    assert r["count"] == n
    assert np.array_equal(r["boxes"][:n], np.asarray(boxes, np.float32).reshape(-1, 4)[kept[:n]]) and (r["boxes"][n:] == 0).all()
    assert np.array_equal(r["scores"][:n], np.asarray(scores, np.float32)[kept[:n]]) and (r["scores"][n:] == 0).all()
    assert sorted(np.flatnonzero(r["keep"])) == sorted(kept[:n])
    assert r["overflow"] == int(int(np.sum(flags)) > max_cand or len(kept) > max_det)
    return kept, r


def test_nms_hand_made(backend):
    A, B = [0.0, 0.0, 4.0, 4.0], [0.0, 0.0, 4.0, 2.0]
    far = [[100.0 + 10 * i, 0.0, 104.0 + 10 * i, 4.0] for i in range(4)]
    assert _nms_check(backend, [A, B], [0.9, 0.8], [0, 0], 0.5, 0.0)[0] == []                         # no candidate
    assert _nms_check(backend, [A, B], [0.9, 0.8], [0, 1], 0.5, 0.0)[0] == [1]                        # one
    assert _nms_check(backend, [A, A, A], [0.5, 0.9, 0.7], [1, 1, 1], 0.5, 0.0)[0] == [1]             # identical boxes: the best stays
    assert _nms_check(backend, far[:3] + [far[0]], [0.6, 0.6, 0.6, 0.6], [1, 1, 1, 1], 0.5, 0.0)[0] == [0, 1, 2]     # equal scores: the index decides
    # IoU exactly at the threshold is KEPT: 8 / (16 + 8 - 8) = 0.5 exactly; under offset 1 the pair has 15 / 25 = 0.6
    assert iou_matrix([A, B], 0.0)[0, 1] == 0.5 and _nms_check(backend, [A, B], [0.9, 0.8], [1, 1], 0.5, 0.0)[0] == [0, 1]
    assert greedy_ref([A, B], [0.9, 0.8], [1, 1], 0.5, 0.0, ge=True) == [0]                             # the fault `>=` would drop it
    assert iou_matrix([A, B], 1.0)[0, 1] == 0.6 and _nms_check(backend, [A, B], [0.9, 0.8], [1, 1], 0.6, 1.0)[0] == [0, 1]
    assert _nms_check(backend, [A, B], [0.9, 0.8], [1, 1], 0.59, 1.0)[0] == [0] and _nms_check(backend, [A, B], [0.9, 0.8], [1, 1], 0.55, 0.0)[0] == [0, 1]
    # a chain: A suppresses B, B would suppress C, A does not touch C -> C stays
    chain = [[0.0, 0.0, 10.0, 10.0], [3.0, 0.0, 13.0, 10.0], [6.0, 0.0, 16.0, 10.0]]
    m = iou_matrix(chain, 0.0)
    assert m[0, 1] > 0.5 and m[1, 2] > 0.5 and m[0, 2] < 0.5 and _nms_check(backend, chain, [0.9, 0.8, 0.7], [1, 1, 1], 0.5, 0.0)[0] == [0, 2]
    # offset 1 in a pass that should have offset 0 changes the set: IoU 6.2 / 9.8 = 0.633 keeps at 0.65, (7.2 / 10.8 = 0.667 would not)
    pair = [[0.0, 0.0, 8.0, 8.0], [1.8, 0.0, 9.8, 8.0]]
    assert _nms_check(backend, pair, [0.9, 0.8], [1, 1], 0.65, 0.0)[0] == [0, 1] and greedy_ref(pair, [0.9, 0.8], [1, 1], 0.65, 1.0) == [0]
    rng = np.random.default_rng(0)
    for n in (63, 64, 65, 300):                                                # boxes (about 90 % flagged) around the wave size, several strides of the block
        xy = rng.uniform(0, 60, (n, 2))
        wh = rng.uniform(4, 30, (n, 2))
        boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        scores = rng.permutation(n).astype(np.float32) / n
        flags = (rng.uniform(size=n) < 0.9).astype(np.int32)
        for thr, off in ((0.65, 0.0), (0.7, 1.0)):
            kept, r = _nms_check(backend, boxes, scores, flags, thr, off, max_cand=64, max_det=64)
            assert len(kept) >= 2
        if n == 65:                                                            # one above max_candidates: the flag, and the best are used
            flags[:] = 1
            kept, r = _nms_check(backend, boxes, scores, flags, 0.65, 0.0, max_cand=64, max_det=64)
            assert r["overflow"] == 1 and int(np.argmin(scores)) not in kept
    # candidate counts 63, 64, 65 at max_candidates 64, every box flagged: one below, exactly at (no overflow, every candidate used) and one above
    # the limit (the flag, and the best 64 are used: the worst score, kept if it were seen because it overlaps nothing, is not)
    for n, over in ((63, 0), (64, 0), (65, 1)):
        xy = rng.uniform(0, 60, (n, 2))
        boxes = np.concatenate([xy, xy + rng.uniform(4, 30, (n, 2))], 1).astype(np.float32)
        scores = (rng.permutation(n).astype(np.float32) + 1) / (n + 1)
        last = int(np.argmin(scores))
        boxes[last] = [500.0, 500.0, 510.0, 510.0]
        for thr, off in ((0.65, 0.0), (0.7, 1.0)):
            kept, r = _nms_check(backend, boxes, scores, np.ones(n, np.int32), thr, off, max_cand=64, max_det=64)
            assert r["overflow"] == over and (last in kept) == (not over) and len(kept) >= 2, (n, thr)
    kept, r = _nms_check(backend, far, [0.9, 0.8, 0.7, 0.6], [1, 1, 1, 1], 0.5, 0.0, max_cand=8, max_det=3)   # survivors above max_det
    assert kept == [0, 1, 2, 3] and r["count"] == 3 and r["overflow"] == 1
    nan = _nms_run(backend, [A, far[0]], [float("nan"), 0.5], [1, 1], 0.5, 0.0)                       # a NaN score is no candidate
    assert nan["count"] == 1 and np.array_equal(nan["boxes"][0], np.float32(far[0]))


def test_nms_refusals(backend):
    from pcdms_amd import _lib, ops
    b, s, f = _dev(torch.zeros(1, 4, 4), backend), _dev(torch.zeros(1, 4), backend), _dev(torch.ones(1, 4, dtype=torch.int32), backend)
    for kw in (dict(max_candidates=1025, max_det=4), dict(max_candidates=4, max_det=5), dict(max_candidates=4, max_det=0)):
        with pytest.raises((RuntimeError, ValueError)):
            ops.nms_f32(b, s, f, thr=0.5, offset=0.0, **kw)
    lib = _lib.lib()
    keep = _dev(torch.full((1, 4), 7, dtype=torch.int32), backend)
    assert lib.pcdm_nms_f32(b.data_ptr(), s.data_ptr(), f.data_ptr(), 1, 4, 4, 4, 0.5, 0.0, None, f.data_ptr(), None, None, None, None, None) == -1   # keep = flags
    assert lib.pcdm_nms_f32(b.data_ptr(), s.data_ptr(), f.data_ptr(), 1, 4, 4, 4, 0.5, 0.0, None, None, None, None, None, None, None) == -1           # no output
    assert lib.pcdm_nms_f32(b.data_ptr(), s.data_ptr(), f.data_ptr(), 1, 4, 4, 4, float("nan"), 0.0, None, keep.data_ptr(), None, None, None, None, None) == -1
    backend.sync()
    assert (keep.cpu() == 7).all()


def test_prep_and_decode_refusals(backend):
    """pcdm_detect_prep and pcdm_detect_decode: every -1 path writes nothing (direct calls on pre-filled buffers)"""
    from pcdms_amd import _lib
    lib = _lib.lib()
    S, C, N = 64, 5, 1
    ldh, P = 8 + 8, 21 * (S // 32) ** 2
    img = _dev(_images(N, 40, 64, 1), backend)
    focus = _dev(torch.full((N * (S // 2) ** 2 * 12 + 4,), 2.5), backend)
    prep = lambda H=40, W=64, size=S, n=N, out=focus.data_ptr(), src=img.data_ptr(): lib.pcdm_detect_prep(src, n, H, W, size, out, None)   # noqa: E731
    for kw in (dict(size=S + 8), dict(size=0), dict(size=8192), dict(H=0), dict(W=-1), dict(n=0), dict(src=None), dict(out=None),
               dict(out=focus.data_ptr() + 4), dict(H=1, W=4096)):
        assert prep(**kw) == -1, kw
    heads = [_dev(torch.zeros(N, S // st, S // st, ldh), backend) for st in (8, 16, 32)]
    boxes, scores = _dev(torch.full((N * P * 4 + 4,), 2.5), backend), _dev(torch.full((N, P), 2.5), backend)
    labels, cand = _dev(torch.full((N, P), 7, dtype=torch.int32), backend), _dev(torch.full((N, P), 7, dtype=torch.int32), backend)

    def decode(h8=heads[0].data_ptr(), n=N, size=S, classes=C, class_id=0, thr=0.5, H=40, W=64, b=boxes.data_ptr(), lab=labels.data_ptr()):
        return lib.pcdm_detect_decode(h8, heads[1].data_ptr(), heads[2].data_ptr(), n, size, classes, class_id, thr, H, W, b, scores.data_ptr(), lab,
                                      cand.data_ptr(), None)
    for kw in (dict(class_id=C), dict(class_id=-1), dict(classes=0), dict(classes=1025), dict(thr=float("nan")), dict(size=S + 8), dict(size=16),
               dict(n=0), dict(H=0), dict(h8=None), dict(h8=heads[0].data_ptr() + 4), dict(b=boxes.data_ptr() + 4), dict(b=None), dict(lab=None)):
        assert decode(**kw) == -1, kw
    backend.sync()
    assert (focus.cpu() == 2.5).all() and (boxes.cpu() == 2.5).all() and (scores.cpu() == 2.5).all()
    assert (labels.cpu() == 7).all() and (cand.cpu() == 7).all()
    assert prep() == 0 and decode() == 0                                       # the same calls with good arguments run
    backend.sync()
    assert (focus.cpu()[-4:] == 2.5).all() and (focus.cpu()[:-4] != 2.5).all() and (cand.cpu() != 7).all()


# ------------------------------------------------------------------------------------------------ 2. the whole network
def _logical(name, t, det):
    """a tapped device tensor -> the restatement's logical layout (and the padding channels, which must be 0)"""
    t = t.cpu()
    if name.startswith("head.") and name.count(".") == 1:
        return torch.cat([t[..., :5], t[..., 8:8 + det.C]], -1).permute(0, 3, 1, 2), torch.cat([t[..., 5:8], t[..., 8 + det.C:]], -1)
    return t.permute(0, 3, 1, 2), None


def _run_tapped(det, x):
    taps = {}
    det._taps = taps
    try:
        out = det(x)
    finally:
        det._taps = None
    return taps, out


def test_network(backend):
    """every tensor a later launch reads, stage by stage with teacher forcing; tapped = untapped; the one C call = the per-kernel path bit for bit;
    reruns, another N in between and the place in the batch change nothing"""
    _, ref = _tiny()
    det = _detector()
    img, T64 = _yardsticks()
    x = _dev(img, backend)
    taps, out_t = _run_tapped(det, x)
    out = det(x)
    single = det(x[1:])
    again = det(x)
    swapped = det(x.flip(0).contiguous())
    backend.sync()
    for a, b, c, d in zip(out, out_t, again, swapped):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d.flip(0))
    for a, b in zip(out, single):
        assert torch.equal(a[1:], b)
    assert tuple(out[0].shape) == (2, det.max_det, 4) and out[2].dtype == torch.int32 and out[0].device.type == backend.device.type
    assert np.array_equal(taps["focus"].cpu().numpy(), prep_ref(img, det.S))
    L, rows = {}, {}
    for name, t in taps.items():
        if name.startswith("decode.") or name.startswith("nms"):
            continue
        L[name], padc = _logical(name, t, det)
        assert padc is None or (padc == 0).all(), name                         # padding channels are exactly zero
    names = [n for n, _, _ in ref.stages()]
    assert set(names) == set(L) - {"focus"}, set(names) ^ (set(L) - {"focus"})
    for name, ins, fn in ref.stages():
        want = fn(torch.float64, _q(None), (), *[L[i].double() for i in ins])
        e_ref = _err(fn(torch.float32, _q(None), (), *[L[i].float() for i in ins]), want)
        e_bf = _err(fn(torch.float32, _q(BF), (), *[L[i].float() for i in ins]), want)
        e_dev = _err(L[name], want)
        rows[name] = {"e_ref_fp32_cpu": e_ref, "device": e_dev, "bf16_operands": e_bf}
        print(f"{name:28s} e_ref {e_ref:.3e} device {e_dev:.3e} bf16 {e_bf:.3e}")
        assert e_dev <= FACTOR * e_ref, (name, e_dev, e_ref)
        assert e_bf > FACTOR * e_ref, (name, e_bf, e_ref)
    if not backend.is_emu:
        worst = max(rows, key=lambda n: rows[n]["device"] / max(rows[n]["e_ref_fp32_cpu"], 1e-300))
        _record("network_tiny", {"stages": rows, "worst_stage": worst, "bound": "device <= 16 e_ref per stage; bf16 operands must exceed it"})


def test_decode(backend):
    """the product's own head tensors through pcdm_detect_decode against the fp64 restatement: boxes (normalised by S) and scores within 16
    max(e_ref, one ulp), e_ref the fp32 numpy restatement; labels and candidates exact"""
    det = _detector()
    img, _ = _yardsticks()
    taps, _ = _run_tapped(det, _dev(img, backend))
    backend.sync()
    heads = [_logical(f"head.{i}", taps[f"head.{i}"], det)[0].numpy() for i in range(3)]
    S = det.S
    b64, s64, l64, c64 = decode_ref(heads, S, SRC_H, SRC_W, 0, 0.5, np.float64)
    b32, s32, _, _ = decode_ref(heads, S, SRC_H, SRC_W, 0, 0.5, np.float32)
    got_b, got_s = taps["decode.boxes"].cpu().numpy().astype(np.float64), taps["decode.scores"].cpu().numpy().astype(np.float64)
    e_ref_b, e_dev_b = max(np.abs(b32 - b64).max() / S, ULP), np.abs(got_b - b64).max() / S
    e_ref_s, e_dev_s = max(_err(s32, s64), ULP), _err(got_s, s64)
    print(f"decode boxes e_ref {e_ref_b:.3e} device {e_dev_b:.3e}; scores e_ref {e_ref_s:.3e} device {e_dev_s:.3e}")
    assert e_dev_b <= FACTOR * e_ref_b and e_dev_s <= FACTOR * e_ref_s
    assert b64.shape == (2, 189, 4) and np.abs(s64 - 0.5).min() > 1e-5         # no score sits on the threshold, so membership is decidable
    assert np.array_equal(taps["decode.labels"].cpu().numpy(), l64) and np.array_equal(taps["decode.candidates"].cpu().numpy().astype(bool), c64)
    assert c64.any() and not c64.all() and (l64 != 0).any()
    for fault in ("no_exp", "prior_offset", "scale_swapped"):
        moved = np.abs(decode_ref(heads, S, SRC_H, SRC_W, 0, 0.5, np.float64, (fault,))[0] - b64).max() / S
        assert moved >= BITE * e_ref_b, (fault, moved)
    if not backend.is_emu:
        _record("decode_tiny", {"boxes_e_ref": e_ref_b, "boxes_device": e_dev_b, "scores_e_ref": e_ref_s, "scores_device": e_dev_s})


def _selection_condition():
    """the fp64 chain's decode and selection, and the condition under which fp32 cannot change the outcome: no score within 1e-5 of a threshold, no
    compared IoU within 1e-5 of its threshold, no two distinct candidate scores closer than 1e-5; enough happens: >= 8 candidates, >= 1 suppressed
    and >= 2 kept in some image"""
    _, T64 = _yardsticks()
    b, s, _, c = decode_ref(_heads_np(T64), TINY["size"], SRC_H, SRC_W, 0, 0.5, np.float64)
    kept, busy = [], False
    assert np.abs(s - 0.5).min() > 1e-5 and np.abs(s - 0.01).min() > 1e-5
    for n in range(b.shape[0]):
        used = []
        kept.append(select_ref(b[n], s[n], c[n], used=used))
        sc = np.sort(s[n][c[n]])
        assert len(sc) < 2 or np.diff(sc).min() > 1e-5
        u = np.asarray(used)
        assert len(u) == 0 or min(np.abs(u - 0.65).min(), np.abs(u - 0.7).min()) > 1e-5
        busy |= c[n].sum() >= 8 and len(kept[n]) >= 2 and len(kept[n]) < c[n].sum()
    assert busy
    return b, s, c, kept


def test_selection_on_the_network_output(backend):
    det = _detector()
    b64, s64, c64, kept = _selection_condition()
    img, _ = _yardsticks()
    taps, (boxes, scores, count, overflow) = _run_tapped(det, _dev(img, backend))
    backend.sync()
    dec_b, dec_s = taps["decode.boxes"].cpu().numpy(), taps["decode.scores"].cpu().numpy()
    for n in range(2):
        k = kept[n]
        assert int(count[n]) == len(k) and int(overflow[n]) == 0
        assert sorted(np.flatnonzero(taps["nms2.keep"][n].cpu().numpy())) == sorted(k)
        assert np.array_equal(boxes[n].cpu().numpy()[:len(k)], dec_b[n][k]) and np.array_equal(scores[n].cpu().numpy()[:len(k)], dec_s[n][k])   # the same indices in the same order
        assert (boxes[n].cpu().numpy()[len(k):] == 0).all() and (scores[n].cpu().numpy()[len(k):] == 0).all()
        assert np.abs(boxes[n].cpu().numpy()[:len(k)] - b64[n][k]).max() / det.S <= 1e-4


def test_selection_faults_are_seen(backend):
    """rescale after the NMS: two 8 x 8 boxes 1.6 pixels apart on the canvas have IoU(+1) 0.698 there and 0.703 in image pixels (the source is
    magnified 1.16 times), so mmpose's pass at 0.7 keeps both only if the boxes were NOT rescaled first.  The head tensors are made by hand; the
    first pass is disarmed (threshold 0.9)."""
    from pcdms_amd import ops
    det = _detector(nms_thr=0.9)
    S, C = det.S, det.C
    heads = [np.full((1, 5 + C, S // st, S // st), -12.0) for st in (8, 16, 32)]
    for h in heads:
        h[:, :4] = 0.0
    for (row, col), tx, sc in (((2, 2), 0.0, 6.0), ((2, 2 + 1), -0.8, 5.0), ((8, 8), 0.0, 4.0)):   # prior (x, y) = 8 (col, row); centre = 8 tx + x; w = h = 8
        heads[0][0, 0, row, col], heads[0][0, 4, row, col], heads[0][0, 5, row, col] = tx, sc, sc
    b, s, _, c = decode_ref(heads, S, SRC_H, SRC_W, 0, 0.5, np.float64)
    right = select_ref(b[0], s[0], c[0], nms_thr=0.9)
    b_late = decode_ref(heads, S, SRC_H, SRC_W, 0, 0.5, np.float64, ("rescale_late",))[0]
    assert c[0].sum() == 3 and len(right) == 2 and len(select_ref(b_late[0], s[0], c[0], nms_thr=0.9)) == 3
    dev = []
    for h in heads:
        t = np.zeros((1, h.shape[2], h.shape[3], 8 + det.C4), np.float32)
        t[..., :5], t[..., 8:8 + C] = h[:, :5].transpose(0, 2, 3, 1), h[:, 5:].transpose(0, 2, 3, 1)
        dev.append(_dev(t, backend))
    db, ds, _, dc = ops.detect_decode(dev, S, C, 0, 0.5, (SRC_H, SRC_W))
    boxes, scores, count, _ = det.select(db, ds, dc)
    backend.sync()
    assert int(count[0]) == 2 and np.abs(boxes[0, :2].cpu().numpy() - b[0][right]).max() <= 1e-4
    # `>=` in the NMS and offset 1 in the first pass: tests/test_nms_hand_made holds the device to the right answer on the deciding pairs


FAULTS = {"concat_swapped": "stage2.csp.in", "identity_everywhere": "stage4.blocks.0", "bn_eps": "stage3.down", "lateral_first": "neck.bu0.cat",
          "obj_from_cls": "head.1"}


def test_faults_are_seen(backend):
    """every named fault, applied to the fp64 restatement of its stage on the clean fp64 inputs, moves the stage by >= 32 e_ref (twice the bound).
    ``lateral_first`` stands for the roles of r4 and r5 confused in the bottom-up path: the two differ in size, so the observable form of that
    fault is the lateral tensor taking the downsampled one's place in the concatenation.  ``identity_everywhere`` is also run in the neck.  Every
    stage a fault is judged on is one the product records and test_network holds to 16 e_ref."""
    _, ref = _tiny()
    img, T = _yardsticks()
    taps, _ = _run_tapped(_detector(), _dev(img, backend))
    stages = {n: (ins, fn) for n, ins, fn in ref.stages()}
    for fault, name in list(FAULTS.items()) + [("identity_everywhere", "neck.p3.blocks.0"), ("concat_swapped", "neck.t4.csp.in")]:
        assert name in taps and all(i in taps for i in stages[name][0]), name
        ins, fn = stages[name]
        args = [T[i] for i in ins]
        e_ref = _err(fn(torch.float32, _q(None), (), *[a.float() for a in args]), T[name])
        moved = _err(fn(torch.float64, _q(None), (fault,), *args), T[name])
        print(f"{fault:20s} {name:20s} moved {moved:.3e} e_ref {e_ref:.3e}")
        assert moved >= BITE * e_ref and moved >= 4 * e_ref, (fault, moved, e_ref)


# ------------------------------------------------------------------------------------------------ 3. refusals, state dict, struct layout
def test_state_dict(tmp_path):
    from pcdms_amd import pose
    sd, _ = _tiny()
    for k in ("backbone.stem.conv.conv.weight", "backbone.stage4.1.conv1.bn.running_var", "backbone.stage4.2.blocks.0.conv2.conv.weight",
              "neck.top_down_blocks.1.short_conv.conv.weight", "neck.downsamples.1.bn.bias", "bbox_head.multi_level_conv_obj.2.bias",
              "bbox_head.multi_level_reg_convs.0.1.conv.weight"):
        assert k in sd, k                                                      # mmdet's names
        with pytest.raises(KeyError, match=k.replace(".", r"\.")):
            pose.PersonDetector({a: b for a, b in sd.items() if a != k}, **TINY)
    with pytest.raises(KeyError, match="neck.extra"):
        pose.PersonDetector({**sd, "neck.extra.weight": torch.zeros(1)}, **TINY)
    with pytest.raises(KeyError, match="multi_level_conv_cls.0.weight"):
        pose.PersonDetector({**sd, "bbox_head.multi_level_conv_cls.0.weight": torch.zeros(6, 32, 1, 1)}, **TINY)
    a = pose.PersonDetector({**sd, "ema_backbone_stem_conv_conv_weight": torch.zeros(3), "ema_anything": torch.zeros(1)}, **TINY)   # ignored
    torch.save({"meta": {"epoch": 1}, "state_dict": sd}, tmp_path / "yolox.pth")
    b = pose.PersonDetector.from_checkpoint(tmp_path / "yolox.pth", **TINY)
    for n, p in a._host.items():
        assert torch.equal(p["w"], b._host[n]["w"]) and torch.equal(p["bias"], b._host[n]["bias"]), n
    for bad in (dict(size=100), dict(widen_factor=0.1), dict(class_id=5), dict(max_det=0), dict(max_candidates=2000)):
        with pytest.raises(ValueError):
            pose.PersonDetector(sd, **{**TINY, **bad})
    for kw in (TINY, dict(size=640)):
        d = pose.PersonDetector.__new__(pose.PersonDetector)
        wf, df = kw.get("widen_factor", 1.0), kw.get("deepen_factor", 1.0)
        d.C, d.stem, d.head, d.neck_blocks = kw.get("num_classes", 80), int(64 * wf), int(256 * wf), max(round(3 * df), 1)
        d.stages = [(int(ci * wf), int(co * wf), max(round(nb * df), 1), i, s) for ci, co, nb, i, s in ARCH_P5]
        assert d.expected_shapes() == _shapes(kw), kw
    full = _shapes(dict(size=640))
    n_modules = 1 + 4 + 2 + 4 * 3 + 2 * (3 + 9 + 9 + 3) + 2 + 2 + 3 + 4 * (3 + 6) + 12
    assert len(full) == 5 * n_modules + 18 and full["backbone.stage3.1.blocks.8.conv2.conv.weight"] == (256, 256, 3, 3)
    assert [b for _, _, b, _, _ in _detector().stages] == [1, 3, 3, 1] and _detector().neck_blocks == 1


def test_forward_refusals_and_struct_layout(backend, tmp_path):
    """pcdm_detect_forward / pcdm_detect_ws_bytes: arguments outside the stated ranges return -1 and write nothing; the ctypes mirrors of the two
    structs against the header as gcc lays it out"""
    import ctypes
    import shutil
    import subprocess
    from pcdms_amd import _lib, ops
    det = _detector()
    cfg, wt = det._c_args(backend.device)
    img = _dev(_images(1, 40, 64, 3), backend)
    n = ops.detect_ws_bytes(cfg, 1)
    assert n > 0 and n % 256 == 0 and ops.detect_ws_bytes(cfg, 2) > n and ops.detect_ws_bytes(cfg, 0) == -1
    ws = torch.empty(n // 4, dtype=torch.float32, device=backend.device)
    lib = _lib.lib()
    outs = [torch.full((1, cfg.max_det, 4), 3.5, device=backend.device), torch.full((1, cfg.max_det), 3.5, device=backend.device),
            torch.full((1,), 77, dtype=torch.int32, device=backend.device), torch.full((1,), 77, dtype=torch.int32, device=backend.device)]

    def forward(c=cfg, w=wt, H=40, W=64, nbytes=n):
        return lib.pcdm_detect_forward(img.data_ptr(), 1, H, W, ctypes.byref(c), ctypes.byref(w), *[o.data_ptr() for o in outs], ws.data_ptr(), nbytes, None)
    assert forward(nbytes=n - 256) == -1 and forward(H=0) == -1 and forward(H=40000) == -1
    for field, value in (("S", 100), ("num_classes", 0), ("class_id", 5), ("stem", 12), ("head", 4), ("neck_blocks", 0), ("max_candidates", 1025),
                         ("max_det", cfg.max_candidates + 1), ("score_thr", float("nan"))):
        bad = _lib.DetectConfig.from_buffer_copy(cfg)
        setattr(bad, field, value)
        assert ops.detect_ws_bytes(bad, 1) == -1 and forward(c=bad) == -1, field
    for field, value in (("n_conv", wt.n_conv - 1), ("conv_w", None)):
        bad = _lib.DetectWeights.from_buffer_copy(wt)
        setattr(bad, field, value)
        assert forward(w=bad) == -1, field
    backend.sync()
    assert all((o.cpu() == (3.5 if o.dtype == torch.float32 else 77)).all() for o in outs)    # every -1 wrote nothing
    assert forward() == 0
    backend.sync()
    for a, b in zip(outs, det(img)):
        assert torch.equal(a, b)
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc: the struct layouts were not compared with the header (the refusals above were checked)")
    structs = {"pcdm_detect_config": _lib.DetectConfig, "pcdm_detect_weights": _lib.DetectWeights}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT / "include" / "pcdm.h"}"', "int main(void) {"]
    for cname, ct in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in ct._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["  return 0;", "}"]))
    subprocess.check_call([gcc, "-std=c11", "-Wall", "-Werror", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    got = dict(ln.split() for ln in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    for cname, ct in structs.items():
        assert int(got[cname]) == ctypes.sizeof(ct), cname
        for f, _ in ct._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(ct, f).offset, (cname, f)


# ------------------------------------------------------------------------------------------------ 4. composition
@functools.lru_cache(maxsize=None)
def _sparse_sd(shift):
    """the tiny state dict with the objectness biases lowered: a few detections a frame, so that the pose estimator (slow under the emulator) runs
    on a few boxes"""
    sd = dict(_tiny()[0])
    for i in range(3):
        sd[f"bbox_head.multi_level_conv_obj.{i}.bias"] = sd[f"bbox_head.multi_level_conv_obj.{i}.bias"] - shift
    return sd


@functools.lru_cache(maxsize=None)
def _pose_estimator():
    from pcdms_amd import pose
    from tests import test_dwpose
    kw, sd, _ = test_dwpose._tiny(True)
    return pose.DWPoseEstimator(sd, **kw)


def test_detect_people_and_pose_map(backend):
    """detect_people: every image's boxes in order, the whole frame at count 0; estimate_pose_map(detector=...) = the chained calls; without a
    detector the output is byte for byte what the parent gave (the whole frame as the one box)"""
    from pcdms_amd import pose, preprocess
    det, blind, est = _detector(), _detector(score_thr=0.9999), _pose_estimator()
    img, _ = _yardsticks()
    x = _dev(img, backend)
    boxes, index = pose.detect_people(det, x)
    b, _, count, _ = det(x)
    backend.sync()
    cnt = count.tolist()
    assert min(cnt) >= 2 and tuple(boxes.shape) == (sum(cnt), 4) and index.tolist() == [0] * cnt[0] + [1] * cnt[1] and index.dtype == torch.int32
    assert torch.equal(boxes, torch.cat([b[0, :cnt[0]], b[1, :cnt[1]]]))
    none, idx = pose.detect_people(blind, x)                                   # nothing passes 0.9999: the reference's fallback
    assert blind(x)[2].tolist() == [0, 0] and none.tolist() == [[0.0, 0.0, float(SRC_W), float(SRC_H)]] * 2 and idx.tolist() == [0, 1]
    det = pose.PersonDetector(_sparse_sd(0.7), **TINY)
    one = _dev(_images(1, 90, 60, 8)[0], backend)
    Hd, Wd = pose.detect_size(90, 60, 128)
    frame = preprocess.resize(one, (Wd, Hd))
    fb, _ = pose.detect_people(det, frame)
    assert fb.shape[0] == 2                                                    # two people, two skeletons
    kp, sc = est(frame, fb)
    want = pose.draw_pose(*pose.wholebody_to_openpose(kp, sc), (Hd, Wd), image_size=pose.detect_size(90, 60, 64))[0]
    got = pose.estimate_pose_map(est, one, detect_resolution=128, image_resolution=64, detector=det)
    plain = pose.estimate_pose_map(est, one, detect_resolution=128, image_resolution=64)
    kp0, sc0 = est(frame)
    want0 = pose.draw_pose(*pose.wholebody_to_openpose(kp0, sc0), (Hd, Wd), image_size=pose.detect_size(90, 60, 64))[0]
    given = pose.estimate_pose_map(est, one, detect_resolution=128, image_resolution=64, boxes=fb[:1], detector=blind)   # given boxes win
    backend.sync()
    assert torch.equal(got, want) and torch.equal(plain, want0) and got.dtype == torch.uint8
    kp1, sc1 = est(frame, fb[:1])
    assert torch.equal(given, pose.draw_pose(*pose.wholebody_to_openpose(kp1, sc1), (Hd, Wd), image_size=pose.detect_size(90, 60, 64))[0])


def _load_tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, ROOT / "tools" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_flags_load_a_checkpoint(backend, tmp_path):
    """tools/extract_pose.py --det_weights and the stage-2 driver's --pose_det_weights load a synthetic checkpoint and use its boxes; without the
    flags there is no detector"""
    from PIL import Image
    from pcdms_amd import pose
    from tests import test_dwpose
    sd = _sparse_sd(0.5)
    torch.save({"state_dict": sd}, tmp_path / "yolox.pth")
    size, widen, deepen = test_dwpose._write_checkpoint(tmp_path / "dw.pth", True)
    img = _images(1, 75, 50, 13)[0]
    Image.fromarray(img).save(tmp_path / "a.png")
    det_flags = ["--det_size", "96", "--det_widen_factor", "0.125", "--det_deepen_factor", str(1.0 / 3.0), "--det_num_classes", "5"]
    tool = _load_tool("extract_pose")
    common = [str(tmp_path / "a.png"), "--weights", str(tmp_path / "dw.pth"), "--image_size", "96", "128", "--input_size", *size, "--widen_factor", widen,
              "--deepen_factor", deepen, "--detect_resolution", "64", "--device", str(backend.device)]
    assert tool.main(common + ["--out", str(tmp_path / "det"), "--det_weights", str(tmp_path / "yolox.pth"), *det_flags]) == 0
    det, est = pose.PersonDetector(sd, **TINY), _pose_estimator()
    frame = pose.preprocess.resize(pose.preprocess.resize(_dev(img, backend), (96, 128)), (64, 64))
    boxes, _ = pose.detect_people(det, frame)
    assert boxes.shape[0] == 3                                                 # the detector's boxes, not the whole-frame fallback
    with np.load(tmp_path / "det" / "a_pose.npz") as f:
        assert f["keypoints"].shape == (boxes.shape[0], 133, 2) and np.array_equal(f["keypoints"], est(frame, boxes)[0].cpu().numpy())
    drv = _load_tool("stage2_batchtest_inpaint_model")
    args = drv.build_parser().parse_args([])
    assert args.pose_det_weights is None and drv.load_detector(args) is None    # the default is unchanged
    args = drv.build_parser().parse_args(["--pose_det_weights", str(tmp_path / "yolox.pth")] + [a.replace("--det_", "--pose_det_") for a in det_flags])
    loaded = drv.load_detector(args)
    want = pose.estimate_pose_map(est, _dev(img, backend), detector=det)
    got = drv.load_pose("unused", "estimator", backend.device, True, str(tmp_path / "a.png"), est, loaded)
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 5. GPU only
@pytest.mark.gpu
def test_graph_capture_gpu(gpu_backend):
    det = _detector()
    img, _ = _yardsticks()
    x = _dev(img, gpu_backend)
    eager = det(x)                                                             # (also uploads the weights: not capturable)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = det(x)
    torch.cuda.current_stream().wait_stream(side)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, eager))
    x.copy_(x.flip(2))                                                         # new pixels, the same addresses
    graph.replay()
    torch.cuda.synchronize()
    fresh = det(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, fresh)) and not torch.equal(fresh[0], eager[0])


FULL = dict(size=640)
FULL_NOISE = 0.3             # noisy pictures: their statistics do not depend on the size, so a calibration at 128 x 128 holds at 640 x 640


@functools.lru_cache(maxsize=None)
def _full_sd():
    return synth_state_dict(FULL, 17, calib_size=128, calib_images=48, calib_dt=torch.float32, calib_noise=FULL_NOISE,
                            calib_shape=(96, 128))   # (small and in fp32: full width is slow on the CPU)


@functools.lru_cache(maxsize=None)
def _full_det():
    from pcdms_amd import pose
    return pose.PersonDetector(_full_sd(), **FULL)


@pytest.mark.gpu
@pytest.mark.parametrize("name,module,cin,hw,stride", [("stem", "backbone.stem.conv", 12, 320, 1),
                                                       ("head_cls_conv", "bbox_head.multi_level_cls_convs.0.0", 256, 80, 1),
                                                       ("stage4_block_conv2", "backbone.stage4.2.blocks.0.conv2", 512, 20, 1)])
def test_full_width_layer_gpu(gpu_backend, name, module, cin, hw, stride):
    """full-width single layers at B = 1 against the fp64 restatement of the layer (convolution, BatchNorm eps 1e-3, SiLU)"""
    from pcdms_amd import ops
    ref, det = _ref(_full_sd(), FULL), _full_det()
    g = torch.Generator().manual_seed(hw)
    x = torch.rand(1, cin, hw, hw, generator=g) * (255.0 if name == "stem" else 1.0) - (0.0 if name == "stem" else 0.5)
    w = det._weights(gpu_backend.device)[module]
    got = ops.conv2d_f32_act(_dev(x.permute(0, 2, 3, 1).contiguous(), gpu_backend), w, stride=stride, pad=(1, 1), act=ops.CONV_ACT_SILU)
    torch.cuda.synchronize()
    fn = lambda dt, q: ref.cm(module, x.to(dt), dt, q, (), stride=stride, pad=1)   # noqa: E731
    want = fn(torch.float64, _q(None))
    e_ref, e_bf, e_dev = _err(fn(torch.float32, _q(None)), want), _err(fn(torch.float32, _q(BF)), want), _err(got.cpu().permute(0, 3, 1, 2), want)
    print(f"{name}: e_ref {e_ref:.3e} device {e_dev:.3e} bf16 {e_bf:.3e}")
    _record(f"full_width_{name}", {"e_ref_fp32_cpu": e_ref, "device": e_dev, "bf16_operands": e_bf, "bound_16_e_ref": FACTOR * e_ref})
    assert e_dev <= FACTOR * e_ref and e_bf > FACTOR * e_ref


@pytest.mark.gpu
def test_full_width_call_gpu(gpu_backend):
    """one full-width 640 x 640 call on synthetic weights: finite, count <= max_det, and the one C call = the kernel-by-kernel path"""
    det = _full_det()
    x = _dev(_images(1, 480, 640, 2, FULL_NOISE), gpu_backend)
    out = det(x)
    _, out_t = _run_tapped(det, x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, out_t))
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all() and 0 <= int(out[2][0]) <= det.max_det


# ------------------------------------------------------------------------------------------------ 6. a dormant pin
def _have_mmdet():
    try:
        import mmdet  # noqa: F401
        return True
    except Exception:
        return False


@pytest.mark.gpu
@pytest.mark.skipif(not (_have_mmdet() and os.environ.get("PCDM_YOLOX_CKPT") and os.environ.get("PCDM_YOLOX_CONFIG")),
                    reason="needs mmdet, PCDM_YOLOX_CKPT = the published yolox_l_8x8_300e_coco checkpoint and PCDM_YOLOX_CONFIG = its yolox_l_8xb8-300e_coco.py")
def test_pin_against_mmdet(gpu_backend):
    """the published checkpoint through mmdet's inference_detector against PersonDetector before mmpose's pass: the same person boxes to a tenth of
    a pixel wherever mmdet's score is above 0.5"""
    from mmdet.apis import inference_detector, init_detector
    from pcdms_amd import pose
    ckpt = os.environ["PCDM_YOLOX_CKPT"]
    model = init_detector(os.environ["PCDM_YOLOX_CONFIG"], ckpt, device="cuda:0")
    img = _images(1, 480, 360, 21)[0]
    res = inference_detector(model, np.ascontiguousarray(img[..., ::-1])).pred_instances     # the reference hands mmdet a BGR array
    keep = ((res.labels == 0) & (res.scores > 0.5)).cpu().numpy()
    want = res.bboxes.cpu().numpy()[keep]
    det = pose.PersonDetector.from_checkpoint(ckpt, pose_nms_thr=1.0)
    boxes, _, count, _ = det(_dev(img, gpu_backend))
    got = boxes[0, :int(count[0])].cpu().numpy()
    assert got.shape == want.shape and np.abs(got - want).max() <= 0.1
