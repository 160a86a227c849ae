"""The whole-body pose estimator on the device (pcdms_amd/pose.py: DWPoseEstimator, estimate_pose_map; csrc/pose_net.hip; pcdm_conv2d_f32_act).

The yardstick is an fp64 restatement of the network with ``torch.nn.functional`` on the CPU (``Ref`` below), written from the definition in
include/pcdm.h (mmdet's CSPNeXt, mmpose's RTMCCHead, SimCC decoding) on SYNTHETIC seeded state dicts under mmpose's key names: He-scaled weights,
BatchNorm gamma in U(0.5, 1.5), beta in U(-0.1, 0.1), running statistics calibrated on a seeded batch (as tests/test_fid.py does, so that no layer
is dead or saturated), the head's first layer scaled to unit-variance maps, and ``g``, gamma, beta, ``res_scale`` drawn away from their initial values.  mmpose, mmdet and the published checkpoint are
not available: parity with mmpose on its weights is a dormant pin at the end of this file.

Method (tests/test_fid.py): a result is compared with the fp64 restatement as e = max |got - want| / max |want| and must satisfy e_dev <= 16 e_ref,
e_ref = the same error of the restatement run in fp32 on the CPU (convolution, then unfused BatchNorm, as mmcv computes it); a restatement whose
operands are rounded to bf16 must EXCEED that bound, so the bound discriminates.  The whole network is checked stage by stage with teacher
forcing (tests/test_schedule_conformance.py): a stage's inputs are the product's own recorded tensors of the stage before (the ``_taps`` hook).
``test_faults_are_seen``: named faults of the restatement must each move their stage beyond the bound (32 e_ref: twice the bound, which is more
than the 4 e_ref a fault has to reach to be a fault at all).  The GPU tests write their figures to profiles/dwpose_values.json.  Measured on the
MI355X: device / e_ref is at most 2.3 over the stages of the tiny network and 1.6 over the full-width layers, except the full-width 7 x 7
``final_layer`` at 10.8 -- one sequential chain of 50176 fmaf per output where the CPU library adds in blocks, the case the factor 16 is there for.
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
MFMA_F32_ERR = 3.5e-7            # per output, times sum |a b| (tests/test_fid.py)
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
BF = torch.bfloat16


def _dev(a, backend):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(backend.device)


def _err(got, want):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return ((got - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


def _q(operand):
    return (lambda t: t) if operand is None else (lambda t: t.to(operand).to(t.dtype))


def _record(key, value):
    path = ROOT / "profiles" / "dwpose_values.json"
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


# ------------------------------------------------------------------------------------------------ the restatement
def box_f32(boxes, Hin, Win):
    """GetBBoxCenterScale + the aspect fix in fp32, every operation its own -> (cx, cy, w, h) float32 arrays"""
    b = np.asarray(boxes, np.float32)
    half, pad, ar = np.float32(0.5), np.float32(1.25), np.float32(Win) / np.float32(Hin)
    cx, cy = (b[:, 0] + b[:, 2]) * half, (b[:, 1] + b[:, 3]) * half
    w, h = (b[:, 2] - b[:, 0]) * pad, (b[:, 3] - b[:, 1]) * pad
    wide = w > h * ar
    return cx, cy, np.where(wide, w, h * ar).astype(np.float32), np.where(wide, w / ar, h).astype(np.float32)


def _sat_rint(v):
    return np.rint(np.clip(np.nan_to_num(v, nan=-2147483648.0), -2147483648.0, 2147483647.0)).astype(np.int64)


def crop_ref(img, boxes, index, Hin, Win, flip):
    """the stated fixed-point rule (include/pcdm.h: pcdm_pose_crop) in numpy -> (fp32 [R or 2 R, Hin, Win, 4], the uint8 levels [R, Hin, Win, 3])"""
    N, H, W, _ = img.shape
    cx, cy, w, _ = box_f32(boxes, Hin, Win)
    out, lev = [], []
    for r in range(len(cx)):
        inv = np.float64(w[r]) / np.float64(Win)
        bx, by = np.float64(cx[r]) - 0.5 * Win * inv, np.float64(cy[r]) - 0.5 * Hin * inv
        X = (_sat_rint(bx * 1024.0) + 16 + _sat_rint(inv * np.arange(Win, dtype=np.float64) * 1024.0)) >> 5
        Y = (_sat_rint(by * 1024.0) + 16 + _sat_rint(inv * np.arange(Hin, dtype=np.float64) * 1024.0)) >> 5
        sx, fx, sy, fy = (X >> 5)[None, :], (X & 31)[None, :], (Y >> 5)[:, None], (Y & 31)[:, None]
        acc = np.zeros((Hin, Win, 3), np.int64)
        ok_img = 0 <= index[r] < N
        for dy, dx, wt in ((0, 0, (32 - fx) * (32 - fy) * 32), (0, 1, fx * (32 - fy) * 32), (1, 0, (32 - fx) * fy * 32), (1, 1, fx * fy * 32)):
            px, py = np.broadcast_to(sx + dx, (Hin, Win)), np.broadcast_to(sy + dy, (Hin, Win))
            ok = (px >= 0) & (px < W) & (py >= 0) & (py < H) & ok_img
            v = img[index[r] if ok_img else 0][np.clip(py, 0, H - 1), np.clip(px, 0, W - 1)].astype(np.int64)
            acc += np.where(ok[..., None], v, 0) * wt[..., None]
        val = (acc + 16384) >> 15
        lev.append(val.astype(np.uint8))
        o = np.zeros((Hin, Win, 4), np.float32)
        o[..., :3] = (val.astype(np.float32) - np.array(MEAN, np.float32)) / np.array(STD, np.float32)
        out.append(o)
    out = np.stack(out)
    return (np.concatenate([out, out[:, :, ::-1]]) if flip else out), np.stack(lev)


def decode_ref(logits, nx, R, flip_idx, boxes, Hin, Win, faults=()):
    """logits [R2, K, nx + ny] (numpy, any float type) -> (keypoints fp32 [R, K, 2], scores [R, K] in the logits' type, merged x, merged y)"""
    x, y = logits[..., :nx], logits[..., nx:]
    if flip_idx is not None:
        fi = np.asarray(flip_idx)
        xf, yf = x[R:][:, fi], y[R:][:, fi]
        if "bins_not_reversed" not in faults:
            xf = xf[..., ::-1]
        x, y = 0.5 * (x[:R] + xf), 0.5 * (y[:R] + yf)
    lx, ly, mx, my = np.argmax(x, -1), np.argmax(y, -1), np.max(x, -1), np.max(y, -1)
    sc = np.where(mx > my, mx if "score_max" in faults else my, my if "score_max" in faults else mx)
    drop = sc <= 0
    loc = np.stack([np.where(drop, -1, lx), np.where(drop, -1, ly)], -1).astype(np.float32) / np.float32(2.0)
    cx, cy, w, h = box_f32(boxes, Hin, Win)
    size, scale, c = np.array([Win, Hin], np.float32), np.stack([w, h], -1)[:, None, :], np.stack([cx, cy], -1)[:, None, :]
    kp = loc / size * scale + c - np.float32(0.5) * scale
    return kp.astype(np.float32), sc, x, y


# The tables of the definition, spelled out here and not read from the product: CSPNeXt's P5 arch_settings (in, out, blocks, identity, spp), the
# COCO-WholeBody flip_indices (mmpose configs/_base_/datasets/coco_wholebody.py: entry k = the keypoint that k becomes in the mirrored image), and
# below, in ``_shapes``, every key of mmpose's state dict with its shape.
ARCH_P5 = ((64, 128, 3, True, False), (128, 256, 6, True, False), (256, 512, 6, True, False), (512, 1024, 3, False, True))
FLIP_133 = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15,                                                    # body
            20, 21, 22, 17, 18, 19,                                                                                      # feet
            39, 38, 37, 36, 35, 34, 33, 32, 31, 30, 29, 28, 27, 26, 25, 24, 23,                                          # face contour
            49, 48, 47, 46, 45, 44, 43, 42, 41, 40,                                                                      # eyebrows
            50, 51, 52, 53, 58, 57, 56, 55, 54,                                                                          # nose
            68, 67, 66, 65, 70, 69, 62, 61, 60, 59, 64, 63,                                                              # eyes
            77, 76, 75, 74, 73, 72, 71, 82, 81, 80, 79, 78, 87, 86, 85, 84, 83, 90, 89, 88,                              # mouth
            112, 113, 114, 115, 116, 117, 118, 119, 120, 121, 122, 123, 124, 125, 126, 127, 128, 129, 130, 131, 132,     # left hand -> right
            91, 92, 93, 94, 95, 96, 97, 98, 99, 100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111]              # right hand -> left


class Ref:
    """The network as a list of stages over LOGICAL tensors (NCHW feature maps, [rows, C] token matrices): ``stages()`` yields (name, input names,
    fn(dtype, q, faults, *inputs)); ``chain`` runs them from the crops."""

    def __init__(self, sd, *, Win, Hin, widen, deepen, K=133, bn_eps=1e-5, flip_idx=None):
        self.sd, self.Win, self.Hin, self.K, self.eps = sd, Win, Hin, K, bn_eps
        self.stem = int(64 * widen)
        self.arch = [(int(ci * widen), int(co * widen), max(round(nb * deepen), 1), ident, spp) for ci, co, nb, ident, spp in ARCH_P5]
        self.flip_idx = list(FLIP_133) if flip_idx is None else list(flip_idx)
        self.calib = None

    def cm(self, name, x, dt, q, faults, stride=1, pad=0, groups=1):
        sd = self.sd
        h = F.conv2d(q(x), q(sd[f"{name}.conv.weight"].to(dt)), None, stride=stride, padding=pad, groups=groups)
        if self.calib is not None:                                             # (once, while the weights are made: see the module docstring)
            co, var = h.shape[1], h.var((0, 2, 3))
            sd[f"{name}.bn.running_var"] = (var * (torch.rand(co, generator=self.calib) + 0.5)).float().clamp_min(1e-12)
            sd[f"{name}.bn.running_mean"] = (h.mean((0, 2, 3)) + (torch.rand(co, generator=self.calib) * 2 - 1) * 0.3 * var.sqrt()).float()
        m, v, g, b = (sd[f"{name}.bn.{k}"].to(dt) for k in ("running_mean", "running_var", "weight", "bias"))
        return F.silu(F.batch_norm(h, m, v, g, b, False, 0.0, 1e-3 if "bn_eps" in faults else self.eps))

    @staticmethod
    def scalenorm(x, g, faults):
        scale = 1.0 if "scalenorm_scale" in faults else x.shape[-1] ** -0.5
        return x / (torch.linalg.vector_norm(x, dim=-1, keepdim=True) * scale).clamp(min=1e-5) * g

    def stages(self):
        sd, cm, K = self.sd, self.cm, self.K
        out = []
        add = lambda name, ins, fn: out.append((name, ins, fn))   # noqa: E731
        prev = "crop"
        for i in range(3):
            add(f"stem.{i}", (prev,), lambda dt, q, f, x, i=i: cm(f"backbone.stem.{i}", x, dt, q, f, stride=2 if i == 0 else 1, pad=1))
            prev = f"stem.{i}"
        for s, (_, co, nb, ident, spp) in enumerate(self.arch, 1):
            mid = co // 2
            add(f"stage{s}.down", (prev,), lambda dt, q, f, x, s=s: cm(f"backbone.stage{s}.0", x, dt, q, f, stride=2, pad=1))
            prev = f"stage{s}.down"
            if spp:
                def spp_cat(dt, q, f, x, s=s):
                    h = cm(f"backbone.stage{s}.1.conv1", x, dt, q, f)
                    return torch.cat([h] + [F.max_pool2d(h, k, 1, k // 2) for k in (5, 9, 13)], 1)
                add(f"stage{s}.spp.cat", (prev,), spp_cat)
                add(f"stage{s}.spp", (f"stage{s}.spp.cat",), lambda dt, q, f, x, s=s: cm(f"backbone.stage{s}.1.conv2", x, dt, q, f))
                prev = f"stage{s}.spp"
            n = f"backbone.stage{s}.{2 if spp else 1}"

            def csp_in(dt, q, f, x, n=n):
                a, b = cm(f"{n}.main_conv", x, dt, q, f), cm(f"{n}.short_conv", x, dt, q, f)
                return torch.cat([b, a] if "concat_swapped" in f else [a, b], 1)
            add(f"stage{s}.csp.in", (prev,), csp_in)
            cat = f"stage{s}.csp.in"
            for b in range(nb):
                add(f"stage{s}.blocks.{b}.conv1", (cat,), lambda dt, q, f, x, n=n, b=b, mid=mid: cm(f"{n}.blocks.{b}.conv1", x[:, :mid], dt, q, f, pad=1))
                add(f"stage{s}.blocks.{b}.dw", (f"stage{s}.blocks.{b}.conv1",),
                    lambda dt, q, f, x, n=n, b=b, mid=mid: cm(f"{n}.blocks.{b}.conv2.depthwise_conv", x, dt, q, f, pad=2, groups=mid))

                def block(dt, q, f, u, c, n=n, b=b, mid=mid, ident=ident):
                    y = cm(f"{n}.blocks.{b}.conv2.pointwise_conv", u, dt, q, f)
                    if ident and "no_identity" not in f:
                        y = y + c[:, :mid]
                    return torch.cat([y, c[:, mid:]], 1)
                add(f"stage{s}.blocks.{b}", (f"stage{s}.blocks.{b}.dw", cat), block)
                cat = f"stage{s}.blocks.{b}"
            add(f"stage{s}.pool", (cat,), lambda dt, q, f, x: q(x).mean((2, 3)))

            def att(dt, q, f, p, n=n):
                v = F.linear(q(p), q(sd[f"{n}.attention.fc.weight"].to(dt).flatten(1)), sd[f"{n}.attention.fc.bias"].to(dt))
                return torch.sigmoid(v) if "sigmoid" in f else F.hardsigmoid(v)
            add(f"stage{s}.att", (f"stage{s}.pool",), att)

            def final(dt, q, f, c, a, n=n):
                if "attention_after" in f:
                    return cm(f"{n}.final_conv", c, dt, q, f) * a[:, :, None, None]
                return cm(f"{n}.final_conv", c * a[:, :, None, None], dt, q, f)
            add(f"stage{s}", (cat, f"stage{s}.att"), final)
            prev = f"stage{s}"

        def final_layer(dt, q, f, x):
            if self.calib is not None:   # unit-variance maps around a bias of magnitude 1 .. 2: no token's h w values are all near 0, where ScaleNorm
                h0 = F.conv2d(x, sd["head.final_layer.weight"].to(dt), None, padding=3)           # over the tiny nets' 2 .. 6 positions is ill-conditioned
                sd["head.final_layer.weight"] = (sd["head.final_layer.weight"].to(dt) / h0.std()).float()
                sign = (torch.rand(K, generator=self.calib) < 0.5).float() * 2 - 1
                sd["head.final_layer.bias"] = sign * (torch.rand(K, generator=self.calib) + 1.0)
            h = F.conv2d(q(x), q(sd["head.final_layer.weight"].to(dt)), sd["head.final_layer.bias"].to(dt), padding=3)
            return h.flatten(2).reshape(-1, h.shape[2] * h.shape[3])               # [B K, P]
        add("head.final_layer", (prev,), final_layer)
        add("head.mlp.0", ("head.final_layer",), lambda dt, q, f, x: self.scalenorm(q(x), sd["head.mlp.0.g"].to(dt), f))
        add("head.mlp.1", ("head.mlp.0",), lambda dt, q, f, x: F.linear(q(x), q(sd["head.mlp.1.weight"].to(dt))))
        add("head.gau.ln", ("head.mlp.1",), lambda dt, q, f, x: self.scalenorm(q(x), sd["head.gau.ln.g"].to(dt), f))
        add("head.gau.shortcut", ("head.mlp.1",), lambda dt, q, f, x: q(x) * sd["head.gau.res_scale.scale"].to(dt))
        add("head.gau.uv", ("head.gau.ln",), lambda dt, q, f, x: F.silu(F.linear(q(x), q(sd["head.gau.uv.weight"].to(dt)))))
        add("head.gau.core", ("head.gau.uv",), lambda dt, q, f, x: gau_core_ref(q(x), K, sd["head.gau.gamma"].to(dt), sd["head.gau.beta"].to(dt), f))
        add("head.gau", ("head.gau.core", "head.gau.shortcut"), lambda dt, q, f, x, sh: sh + F.linear(q(x), q(sd["head.gau.o.weight"].to(dt))))
        add("head.cls", ("head.gau",), lambda dt, q, f, x: F.linear(q(x), q(torch.cat([sd["head.cls_x.weight"], sd["head.cls_y.weight"]], 0).to(dt))))
        return out

    def chain(self, crops, dt=torch.float64, operand=None, faults=()):
        """crops: logical [B, 3, Hin, Win] -> {name: logical tensor}"""
        T = {"crop": crops.to(dt)}
        for name, ins, fn in self.stages():
            T[name] = fn(dt, _q(operand), faults, *[T[i] for i in ins])
        return T


def gau_core_ref(uv, T, gamma, beta, faults=()):
    """uv [B T, 2 e + s] -> [B T, e]"""
    s = gamma.shape[1]
    e = (uv.shape[1] - s) // 2
    u, v, base = (t.reshape(-1, T, t.shape[1]) for t in torch.split(uv, [e, e, s], 1))
    g0, g1 = (1, 0) if "gamma_swapped" in faults else (0, 1)
    qq, kk = base * gamma[g0] + beta[g0], base * gamma[g1] + beta[g1]
    qk = torch.bmm(qq, kk.transpose(1, 2))
    if "no_sqrt_s" not in faults:
        qk = qk / math.sqrt(s)
    a = F.relu(qk)
    if "no_square" not in faults:
        a = a * a
    return (u * torch.bmm(a, v)).reshape(-1, e)


def synth_state_dict(est_kwargs, seed):
    """a seeded state dict under mmpose's key names for DWPoseEstimator(**est_kwargs), its BatchNorm statistics calibrated on a seeded batch"""
    shapes = _shapes(est_kwargs)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in shapes.items():
        if k.endswith("conv.weight") or k in ("head.final_layer.weight", "head.mlp.1.weight", "head.gau.uv.weight", "head.gau.o.weight",
                                              "head.cls_x.weight", "head.cls_y.weight") or k.endswith("fc.weight"):
            sd[k] = torch.randn(shp, generator=g) * math.sqrt(2.0 / math.prod(shp[1:]))
        elif k.endswith("bn.weight") or k.endswith("running_var"):
            sd[k] = torch.rand(shp, generator=g) + 0.5
        elif k.endswith(".g"):
            sd[k] = torch.rand(shp, generator=g) + 0.7
        elif k == "head.gau.gamma":
            sd[k] = torch.randn(shp, generator=g) * 0.5 + 1.0
        elif k == "head.gau.res_scale.scale":
            sd[k] = torch.rand(shp, generator=g) + 0.5
        elif k == "head.gau.beta":
            sd[k] = torch.randn(shp, generator=g) * 0.3
        else:                                                                  # biases, bn.bias, running_mean
            sd[k] = (torch.rand(shp, generator=g) * 2 - 1) * 0.1
    ref = _ref(sd, est_kwargs)
    W, H = est_kwargs["input_size"]
    img = _images(16, H + 8, W + 8, seed + 1)
    crops, _ = crop_ref(img, [[0, 0, W + 8, H + 8]] * 16, list(range(16)), H, W, False)
    ref.calib = g
    ref.chain(torch.from_numpy(crops[..., :3]).permute(0, 3, 1, 2))
    ref.calib = None
    for k in list(sd):
        if k.endswith("running_var"):
            sd[k[:-len("running_var")] + "num_batches_tracked"] = torch.tensor(7)
    return sd


def _shapes(est_kwargs):
    """every key of mmpose's state dict for the configuration (mmdet CSPNeXt, mmpose RTMCCHead module names) -> shape; written out here, and
    test_state_dict_keys_are_checked holds the product's own list to it"""
    W, H = est_kwargs["input_size"]
    K, wf, df = est_kwargs.get("num_keypoints", 133), est_kwargs.get("widen_factor", 1.0), est_kwargs.get("deepen_factor", 1.0)
    sh = {}

    def conv_module(name, co, ci, k):
        sh[f"{name}.conv.weight"] = (co, ci, k, k)
        sh.update({f"{name}.bn.weight": (co,), f"{name}.bn.bias": (co,), f"{name}.bn.running_mean": (co,), f"{name}.bn.running_var": (co,)})
    c = int(64 * wf)
    conv_module("backbone.stem.0", c // 2, 3, 3)
    conv_module("backbone.stem.1", c // 2, c // 2, 3)
    conv_module("backbone.stem.2", c, c // 2, 3)
    for s, (ci, co, nb, _, spp) in enumerate(ARCH_P5, 1):
        ci, co, nb, mid = int(ci * wf), int(co * wf), max(round(nb * df), 1), int(co * wf) // 2
        conv_module(f"backbone.stage{s}.0", co, ci, 3)
        csp = f"backbone.stage{s}.1"
        if spp:
            conv_module(f"backbone.stage{s}.1.conv1", co // 2, co, 1)
            conv_module(f"backbone.stage{s}.1.conv2", co, 2 * co, 1)
            csp = f"backbone.stage{s}.2"
        conv_module(f"{csp}.main_conv", mid, co, 1)
        conv_module(f"{csp}.short_conv", mid, co, 1)
        conv_module(f"{csp}.final_conv", co, 2 * mid, 1)
        for b in range(nb):
            conv_module(f"{csp}.blocks.{b}.conv1", mid, mid, 3)
            conv_module(f"{csp}.blocks.{b}.conv2.depthwise_conv", mid, 1, 5)
            conv_module(f"{csp}.blocks.{b}.conv2.pointwise_conv", mid, mid, 1)
        sh[f"{csp}.attention.fc.weight"], sh[f"{csp}.attention.fc.bias"] = (2 * mid, 2 * mid, 1, 1), (2 * mid,)
    sh["head.final_layer.weight"], sh["head.final_layer.bias"] = (K, int(1024 * wf), 7, 7), (K,)
    sh["head.mlp.0.g"], sh["head.mlp.1.weight"] = (1,), (256, (H // 32) * (W // 32))
    sh["head.gau.ln.g"], sh["head.gau.uv.weight"], sh["head.gau.o.weight"] = (1,), (1152, 256), (256, 512)
    sh["head.gau.gamma"], sh["head.gau.beta"], sh["head.gau.res_scale.scale"] = (2, 128), (2, 128), (256,)
    sh["head.cls_x.weight"], sh["head.cls_y.weight"] = (2 * W, 256), (2 * H, 256)
    return sh


def _ref(sd, est_kwargs):
    W, H = est_kwargs["input_size"]
    return Ref(sd, Win=W, Hin=H, widen=est_kwargs.get("widen_factor", 1.0), deepen=est_kwargs.get("deepen_factor", 1.0),
               K=est_kwargs.get("num_keypoints", 133), bn_eps=est_kwargs.get("bn_eps", 1e-5))


TINY = dict(input_size=(64, 96), widen_factor=0.125, deepen_factor=0.34)      # blocks (1, 2, 2, 1)
TINY_EMU = dict(input_size=(32, 64), widen_factor=0.125, deepen_factor=0.34)  # (the lane emulator runs the 64 x 96 network too slowly)
SEED = 3


@functools.lru_cache(maxsize=None)
def _tiny(emu):
    kw = TINY_EMU if emu else TINY
    sd = synth_state_dict(kw, SEED)
    return kw, sd, _ref(sd, kw)


# ------------------------------------------------------------------------------------------------ 1. per-kernel tests
CROP_BOXES = [[10.0, 6.0, 50.0, 70.0],           # inside
              [-20.5, 30.25, 40.0, 100.0],       # partly outside
              [-30.0, -40.0, 120.0, 130.0],      # larger than the image
              [33.3, 20.1, 47.9, 36.6]]          # small: magnified


def test_crop(backend):
    from pcdms_amd import ops
    Hin, Win = 48, 32
    img = _images(2, 80, 64, 5)
    index = [0, 1, 1, 0]
    want, _ = crop_ref(img, CROP_BOXES, index, Hin, Win, True)
    got = ops.pose_crop(_dev(img, backend), _dev(torch.tensor(CROP_BOXES), backend), _dev(torch.tensor(index, dtype=torch.int32), backend), (Hin, Win),
                        flip=True)
    backend.sync()
    got = got.cpu().numpy()
    assert got.shape == (8, Hin, Win, 4) and (got[..., 3] == 0).all()
    assert np.array_equal(got, want)                                           # byte-equal to the stated rule
    assert np.array_equal(got[4:], got[:4, :, ::-1])                           # the mirror is taken from the crop
    assert (want[2, 0, 0, :3] == ((0 - np.array(MEAN, np.float32)) / np.array(STD, np.float32))).all()   # outside the image: level 0
    plain = ops.pose_crop(_dev(img, backend), _dev(torch.tensor(CROP_BOXES), backend), _dev(torch.tensor(index, dtype=torch.int32), backend), (Hin, Win),
                          flip=False)
    assert torch.equal(plain.cpu(), torch.from_numpy(want[:4]))
    with pytest.raises(RuntimeError, match="code -1"):
        ops.pose_crop(_dev(img, backend), _dev(torch.tensor(CROP_BOXES), backend), None, (0, Win), flip=False)


def test_crop_within_one_level_of_bilinear(backend):
    """Against an fp64 bilinear (zeros outside the image).  (a) At the rule's own 1/32-pixel sampling positions, everywhere: the integer arithmetic
    adds the final rounding only, half a level.  (b) At the exact positions xs = (xd - 0.5 Win) / s + cx: the position is quantised by up to 1/64
    pixel per axis, which costs 1/64 of the local gradient -- below half a level on a smooth image wherever the four taps lie inside the image
    (one level in all), but not across the image border, where the constant-0 border is a step of up to 255 levels in one pixel (measured there:
    2.4 levels); that is a property of the stated rule, so the one-level bound of (b) is asserted for samples whose taps are inside, and samples
    that touch the border are held to the rule's own worst case instead: a bilinear surface of 8-bit data has a slope of at most 255 levels per
    pixel along each axis, so 1/64 pixel per axis and the final rounding give 2 x 255 / 64 + 0.5 = 8.5 levels."""
    from pcdms_amd import ops
    Hin, Win, H, W = 48, 32, 80, 64
    img = _images(1, H, W, 6, noise=0.0)
    got = ops.pose_crop(_dev(img, backend), _dev(torch.tensor(CROP_BOXES), backend), None, (Hin, Win), flip=True)
    backend.sync()
    lev = got.cpu().double().numpy()[..., :3] * np.array(STD) + np.array(MEAN)
    cx, cy, w, _ = (a.astype(np.float64) for a in box_f32(CROP_BOXES, Hin, Win))
    pad = np.zeros((H + 2, W + 2, 3))
    pad[1:-1, 1:-1] = img[0]

    def bilinear(xs, ys):
        x0, y0 = np.floor(xs), np.floor(ys)
        tx, ty = (xs - x0)[None, :, None], (ys - y0)[:, None, None]
        px = lambda yy, xx: pad[np.clip(yy + 1, 0, H + 1).astype(int)[:, None], np.clip(xx + 1, 0, W + 1).astype(int)[None, :]]   # noqa: E731
        inside = ((y0 >= 0) & (y0 + 1 < H))[:, None] & ((x0 >= 0) & (x0 + 1 < W))[None, :]
        return (1 - ty) * ((1 - tx) * px(y0, x0) + tx * px(y0, x0 + 1)) + ty * ((1 - tx) * px(y0 + 1, x0) + tx * px(y0 + 1, x0 + 1)), inside
    BORDER = 2 * 255.0 / 64.0 + 0.5                                            # 1/64 pixel per axis x the steepest slope of 8-bit data, + the rounding
    seen_outside = False
    for r in range(len(CROP_BOXES)):
        inv = w[r] / Win
        bx, by = cx[r] - 0.5 * Win * inv, cy[r] - 0.5 * Hin * inv
        X = (_sat_rint(bx * 1024.0) + 16 + _sat_rint(inv * np.arange(Win) * 1024.0)) >> 5
        Y = (_sat_rint(by * 1024.0) + 16 + _sat_rint(inv * np.arange(Hin) * 1024.0)) >> 5
        at_rule, _ = bilinear(X / 32.0, Y / 32.0)
        exact, inside = bilinear((np.arange(Win) - 0.5 * Win) * inv + cx[r], (np.arange(Hin) - 0.5 * Hin) * inv + cy[r])
        for half, flipped in ((lev[r], False), (lev[len(CROP_BOXES) + r][:, ::-1], True)):       # the mirrored copy too
            assert np.abs(half - at_rule).max() <= 0.5 + 1e-4, (r, flipped, np.abs(half - at_rule).max())
            assert np.abs(half - exact)[inside].max() <= 1.0, (r, flipped, np.abs(half - exact)[inside].max())
            assert np.abs(half - exact).max() <= BORDER, (r, flipped, np.abs(half - exact).max())
        seen_outside |= bool((~inside).any())
        print(f"box {r}: at the rule's positions {np.abs(lev[r] - at_rule).max():.3f}, exact positions inside {np.abs(lev[r] - exact)[inside].max():.3f}, "
              f"everywhere {np.abs(lev[r] - exact).max():.3f} levels")
    assert seen_outside


def _conv_case(seed, B, Hi, Wi, pitch, Cin, Cout, kh, kw):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, Hi, Wi, pitch, generator=g) * 2 - 1
    w = torch.randn(Cout, Cin, kh, kw, generator=g) * math.sqrt(2.0 / (Cin * kh * kw))
    bias = (torch.rand(Cout, generator=g) * 2 - 1) * 0.1
    return g, x, w, bias


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("kh,kw,stride,pad,Cin", [(1, 1, 1, (0, 0), 12), (3, 3, 2, (1, 1), 8), (7, 7, 1, (3, 3), 4)])
def test_conv_act(backend, act, kh, kw, stride, pad, Cin):
    """channel slices in and out, Cout = 133 (a tail of 5), K = kh kw Cin no multiple of 16 (12, 72, 196), each activation, residual, A-scale"""
    from pcdms_amd import ops
    B, Hi, Wi, Cout, pitch_in, in_off, pitch, off, sentinel = 2, 5, 6, 133, 24, 8, 144, 8, -77.25
    g, x, w, bias = _conv_case(100 * kh + 10 * act + Cin, B, Hi, Wi, pitch_in, Cin, Cout, kh, kw)
    pw = ops.pack_lpips_conv(w, bias, backend.device)
    xs = x[..., in_off:in_off + Cin].permute(0, 3, 1, 2).double()
    scale = torch.rand(B, Cin, generator=g) + 0.25
    Ho, Wo = (Hi + 2 * pad[0] - kh) // stride + 1, (Wi + 2 * pad[1] - kw) // stride + 1
    res = torch.randn(B, Ho, Wo, 140, generator=g)
    fn = (lambda t: t, F.relu, F.silu)[act]

    def want_of(dt, operand=None):
        q = _q(operand)
        a = (x[..., in_off:in_off + Cin].to(dt) * scale.to(dt)[:, None, None, :]).permute(0, 3, 1, 2)
        return fn(F.conv2d(q(a), q(w.to(dt)), bias.to(dt), stride=stride, padding=pad)) + res[..., 4:4 + Cout].to(dt).permute(0, 3, 1, 2)
    want = want_of(torch.float64)
    e_ref, e_bf = _err(want_of(torch.float32), want), _err(want_of(torch.float32, BF), want)
    out = torch.full((B, Ho, Wo, pitch), sentinel, dtype=torch.float32, device=backend.device)
    ops.conv2d_f32_act(_dev(x, backend), pw, stride=stride, pad=pad, act=act, in_offset=in_off, residual=_dev(res, backend), res_offset=4,
                       a_scale=_dev(scale, backend), out=out, offset=off)
    backend.sync()
    o = out.cpu()
    assert (o[..., :off] == sentinel).all() and (o[..., off + Cout:] == sentinel).all()      # nothing outside the slice was written
    e_dev = _err(o[..., off:off + Cout].permute(0, 3, 1, 2), want)
    print(f"conv_act {kh}x{kw} s{stride} act {act}: e_ref {e_ref:.3e} device {e_dev:.3e} bf16 {e_bf:.3e}")
    assert e_dev <= FACTOR * e_ref and e_bf > FACTOR * e_ref
    # every extra off: bit-equal to pcdm_conv2d_f32_ex (values of the same run), ReLU or none
    if act <= 1:
        xt = _dev(x[..., in_off:in_off + Cin].contiguous(), backend)
        a = ops.conv2d_f32_act(xt, pw, stride=stride, pad=pad, act=act)
        b = ops.conv2d_f32_ex(xt, pw, stride=stride, pad=pad, relu=bool(act))
        sliced = ops.conv2d_f32_act(_dev(x, backend), pw, stride=stride, pad=pad, act=act, in_offset=in_off)
        backend.sync()
        assert torch.equal(a, b) and torch.equal(sliced, b)
        if pad[0] == pad[1]:
            assert torch.equal(ops.conv2d_f32(xt, pw, stride=stride, pad=pad[0], relu=bool(act)), b)
        mag = F.conv2d(xs.abs(), w.double().abs(), None, stride=stride, padding=pad) + bias.abs().view(1, -1, 1, 1)
        plain = fn(F.conv2d(xs, w.double(), bias.double(), stride=stride, padding=pad))
        assert ((b.cpu().double().permute(0, 3, 1, 2) - plain).abs() <= MFMA_F32_ERR * mag).all()


def test_conv_act_in_place_residual_and_refusals(backend):
    """the CSP block's last convolution: reads another tensor, adds the output slice's old values and rewrites it"""
    from pcdms_amd import ops
    g, x, w, bias = _conv_case(7, 2, 4, 5, 8, 8, 8, 1, 1)
    pw = ops.pack_lpips_conv(w, bias, backend.device)
    cat = torch.randn(2, 4, 5, 16, generator=g)
    want = cat.clone().double()
    want[..., :8] += F.silu(F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), bias.double())).permute(0, 2, 3, 1)
    d = _dev(cat.clone(), backend)
    ops.conv2d_f32_act(_dev(x, backend), pw, act=2, residual=d, out=d)
    backend.sync()
    assert torch.equal(d.cpu()[..., 8:], cat[..., 8:]) and _err(d.cpu(), want) <= 1e-6
    xd = _dev(x, backend)
    for kw in (dict(act=3), dict(in_offset=2), dict(in_offset=4), dict(offset=1, out=torch.empty(2, 4, 5, 8, device=backend.device))):
        with pytest.raises(RuntimeError, match="code -1"):
            ops.conv2d_f32_act(xd, pw, **kw)
    # an output slice that overlaps the input slice of the same tensor would race: refused, by the convolution and by the depthwise kernel
    with pytest.raises(RuntimeError, match="code -1"):
        ops.conv2d_f32_act(d, pw, out=d, offset=4)                              # reads channels 0 .. 7, writes 4 .. 11
    ops.conv2d_f32_act(d, pw, out=d, offset=8)                                  # disjoint slices of one tensor: fine
    dw_w, dw_b = _dev(torch.zeros(25, 8), backend), _dev(torch.zeros(8), backend)
    with pytest.raises(RuntimeError, match="code -1"):
        ops.dwconv5_silu_f32(d, dw_w, dw_b, d)
    ops.dwconv5_silu_f32(d, dw_w, dw_b, d, offset=8)


DW_CASES = [(4, 1, 1), (4, 2, 3), (36, 2, 3), (36, 9, 12), (4, 9, 12)]


def _dw_check(backend, C, H, W, B=2):
    from pcdms_amd import ops
    g = torch.Generator().manual_seed(C * 100 + H)
    x = torch.randn(B, H, W, C + 8, generator=g)
    w = torch.randn(C, 1, 5, 5, generator=g) * 0.3
    bias = torch.randn(C, generator=g) * 0.2

    def want_of(dt, operand=None):
        q = _q(operand)
        return F.silu(F.conv2d(q(x[..., 4:4 + C].to(dt).permute(0, 3, 1, 2)), q(w.to(dt)), bias.to(dt), padding=2, groups=C))
    want = want_of(torch.float64)
    e_ref, e_bf = _err(want_of(torch.float32), want), _err(want_of(torch.float32, BF), want)
    out = torch.full((B, H, W, C + 4), 9.5, dtype=torch.float32, device=backend.device)
    ops.dwconv5_silu_f32(_dev(x, backend), _dev(w.view(C, 25).t().contiguous(), backend), _dev(bias, backend), out, in_offset=4, offset=4)
    backend.sync()
    o = out.cpu()
    e_dev = _err(o[..., 4:].permute(0, 3, 1, 2), want)
    print(f"dw C {C} {H}x{W}: e_ref {e_ref:.3e} device {e_dev:.3e} bf16 {e_bf:.3e}")
    assert (o[..., :4] == 9.5).all() and e_dev <= FACTOR * e_ref and e_bf > FACTOR * e_ref
    return e_ref, e_dev, e_bf


@pytest.mark.parametrize("C,H,W", DW_CASES)
def test_depthwise(backend, C, H, W):
    _dw_check(backend, C, H, W)


@pytest.mark.gpu
def test_depthwise_wide_gpu(gpu_backend):
    e_ref, e_dev, e_bf = _dw_check(gpu_backend, 512, 24, 18)
    _record("depthwise_C512_24x18", {"e_ref_fp32_cpu": e_ref, "device": e_dev, "bf16_operands": e_bf, "bound_16_e_ref": FACTOR * e_ref})


@pytest.mark.parametrize("H,W", [(2, 3), (12, 9)])
def test_spp_pools(backend, H, W):
    """the 5 / 9 / 13 pools as the 5 x 5 maximum cascaded into the concat slices: exactly max_pool2d, NaN included"""
    from pcdms_amd import ops
    C = 8
    x = torch.randn(2, H, W, C, generator=torch.Generator().manual_seed(H))
    x[1, H // 2, W // 2, 3] = float("nan")
    cat = torch.full((2, H, W, 4 * C), -5.5)
    cat[..., :C] = x
    d = _dev(cat, backend)
    for j in range(3):
        ops.maxpool5_f32(d, C, d, in_offset=j * C, offset=(j + 1) * C)
    backend.sync()
    got = d.cpu()
    assert torch.equal(got[..., :C].nan_to_num(nan=9e9), x.nan_to_num(nan=9e9))
    for j, k in enumerate((5, 9, 13), 1):
        want = F.max_pool2d(x.permute(0, 3, 1, 2), k, 1, k // 2).permute(0, 2, 3, 1)
        assert torch.equal(got[..., j * C:(j + 1) * C].nan_to_num(nan=9e9), want.nan_to_num(nan=9e9)), k
    with pytest.raises(RuntimeError, match="code -1"):
        ops.maxpool5_f32(d, C, d, in_offset=0, offset=4)                        # overlapping slices


def test_fc_hardsigmoid(backend):
    from pcdms_amd import ops
    g = torch.Generator().manual_seed(2)
    x, w, b = torch.randn(3, 72, generator=g), torch.randn(72, 72, generator=g) * 0.4, torch.randn(72, generator=g)
    want = F.hardsigmoid(F.linear(x.double(), w.double(), b.double()))
    e_ref = _err(F.hardsigmoid(F.linear(x, w, b)), want)
    e_bf = _err(F.hardsigmoid(F.linear(x.to(BF).float(), w.to(BF).float(), b)), want)
    got = ops.fc_hsigmoid_f32(_dev(x, backend), _dev(w, backend), _dev(b, backend))
    backend.sync()
    assert (want == 0).any() and (want == 1).any()                             # both clamps are reached
    assert _err(got.cpu(), want) <= FACTOR * e_ref < e_bf


@pytest.mark.parametrize("T", [133, 5])
def test_gau_core(backend, T):
    from pcdms_amd import ops
    B, e, s = 2, 512 if T == 133 else 8, 128
    g = torch.Generator().manual_seed(T)
    uv = F.silu(torch.randn(B * T, 2 * e + s, generator=g))
    gamma, beta = torch.randn(2, s, generator=g) * 0.5 + 1.0, torch.randn(2, s, generator=g) * 0.3
    want = gau_core_ref(uv.double(), T, gamma.double(), beta.double())
    e_ref = _err(gau_core_ref(uv, T, gamma, beta), want)
    e_bf = _err(gau_core_ref(uv.to(BF).float(), T, gamma.to(BF).float(), beta.to(BF).float()), want)
    got = ops.gau_core_f32(_dev(uv, backend), B, _dev(gamma, backend), _dev(beta, backend))
    backend.sync()
    e_dev = _err(got.cpu(), want)
    print(f"gau core T {T}: e_ref {e_ref:.3e} device {e_dev:.3e} bf16 {e_bf:.3e}")
    assert tuple(got.shape) == (B * T, e) and e_dev <= FACTOR * e_ref and e_bf > FACTOR * e_ref
    swapped = ops.gau_core_f32(_dev(torch.cat([uv[T:], uv[:T]]), backend), B, _dev(gamma, backend), _dev(beta, backend))
    assert torch.equal(torch.cat([swapped[T:], swapped[:T]]), got)              # a crop does not depend on its place in the batch
    with pytest.raises(RuntimeError, match="code -1"):
        ops.gau_core_f32(_dev(torch.zeros(257, 2 * 8 + s), backend), 1, _dev(gamma, backend), _dev(beta, backend))   # more than 256 tokens


def test_scalenorm(backend):
    """the head's two uses: a transposed read of the NHWC map with a dim that is no multiple of 4, and rows with the scaled shortcut; an all-zero
    row meets the 1e-5 clamp and stays 0"""
    from pcdms_amd import ops
    B, K, P = 2, 7, 6
    gen = torch.Generator().manual_seed(1)
    f = torch.randn(B, P, K, generator=gen)                                    # [B, h w, K]: token k = channel k
    f[1, :, 3] = 0.0
    f[0, :, 2] = 1e-7                                                          # below the clamp: divided by 1e-5, not by its norm
    g = torch.tensor([1.3])
    rows = f.permute(0, 2, 1).reshape(B * K, P)
    want = Ref.scalenorm(rows.double(), g.double(), ())
    e_ref = _err(Ref.scalenorm(rows, g, ()), want)
    got = ops.scalenorm_f32(_dev(f, backend), B, K, P, (P * K, 1, K), _dev(g, backend))
    backend.sync()
    got = got.cpu()
    assert tuple(got.shape) == (B * K, 8) and (got[:, P:] == 0).all() and (got[K + 3] == 0).all()
    assert _err(got[:, :P], want) <= FACTOR * e_ref and _err(Ref.scalenorm(rows.to(BF).float(), g, ()), want) > FACTOR * e_ref
    assert abs(got[2, 0].item() - 1e-7 / 1e-5 * 1.3) <= 1e-6
    x = torch.randn(5, 256, generator=gen)
    rs = torch.rand(256, generator=gen) + 0.5
    hn, side = ops.scalenorm_f32(_dev(x, backend), 1, 5, 256, (0, 256, 1), _dev(g, backend), side_scale=_dev(rs, backend))
    backend.sync()
    want = Ref.scalenorm(x.double(), g.double(), ())
    assert _err(hn.cpu(), want) <= FACTOR * _err(Ref.scalenorm(x, g, ()), want)
    assert torch.equal(side.cpu(), x * rs)


def test_decode(backend):
    """ties (the first index wins), scores <= 0 -> -1, the flip pairs and reversed bins, a NaN logit"""
    from pcdms_amd import ops
    R, K, Hin, Win = 2, 5, 16, 96                                              # 192 x bins: three per lane; 32 y bins: half a wave
    nx, ny = 2 * Win, 2 * Hin
    g = torch.Generator().manual_seed(0)
    lg = torch.randn(2 * R, K, nx + ny, generator=g)
    flip_idx = [1, 0, 2, 4, 3]
    lg[0, 0, 70], lg[0, 0, 7], lg[0, 0, 135] = 9.0, 9.0, 9.0                    # a tie within one lane (7, 135) and across lanes (70)
    lg[R + 0, 1, nx - 1 - 70], lg[R + 0, 1, nx - 1 - 7], lg[R + 0, 1, nx - 1 - 135] = 9.0, 9.0, 9.0      # (keypoint 0's flipped row is row 1, reversed)
    lg[0, 2, :nx] = -1.0 - torch.rand(nx, generator=g)                         # score <= 0
    lg[R + 0, 2, :nx] = -1.0 - torch.rand(nx, generator=g)
    lg[1, 3, nx + 5] = float("nan")                                            # a NaN y logit: argmax there; the score keeps max_x (max_x > NaN is false)
    lg[1, 4, 100] = float("nan")                                               # a NaN x logit: the score is NaN, the location stays
    boxes = [[3.0, 4.0, 40.0, 90.0], [-5.0, 2.5, 20.0, 30.0]]
    for fi in (flip_idx, None):
        lgs = lg if fi is not None else lg[:R]
        kp_w, sc_w, _, _ = decode_ref(lgs.numpy(), nx, R, fi, boxes, Hin, Win)
        kp, sc = ops.simcc_decode(_dev(lgs.reshape(-1, nx + ny).contiguous(), backend), nx, R, K,
                                  None if fi is None else _dev(torch.tensor(fi, dtype=torch.int32), backend), _dev(torch.tensor(boxes), backend), (Hin, Win))
        backend.sync()
        assert np.array_equal(kp.cpu().numpy(), kp_w, equal_nan=True) and np.array_equal(sc.cpu().numpy(), sc_w, equal_nan=True)
    cx, cy, w, h = box_f32(boxes, Hin, Win)
    kp_f, sc_f, _, _ = decode_ref(lg.numpy(), nx, R, flip_idx, boxes, Hin, Win)
    assert kp_f[0, 0, 0] == np.float32(np.float32(3.5) / np.float32(Win) * w[0] + cx[0] - np.float32(0.5) * w[0])       # bin 7: the first of the tie
    assert sc_f[0, 2] <= 0 and kp_f[0, 2, 0] == np.float32(np.float32(-0.5) / np.float32(Win) * w[0] + cx[0] - np.float32(0.5) * w[0])
    assert np.isnan(sc_f[1, 4]) and not np.isnan(sc_f[1, 3])


# ------------------------------------------------------------------------------------------------ 2. the whole network
NET_BOXES = [[4.0, 3.0, 60.0, 100.0], [-8.0, 10.0, 50.0, 90.0], [20.0, 30.0, 70.0, 118.0]]
NET_INDEX = [0, 1, 1]


@functools.lru_cache(maxsize=None)
def _estimator(emu):
    from pcdms_amd import pose
    kw, sd, _ = _tiny(emu)
    return pose.DWPoseEstimator(sd, **kw)


def _logical(name, t, est, B):
    """a tapped device tensor -> the restatement's logical layout (and the padding columns, which must be 0)"""
    t = t.cpu()
    if name == "head.final_layer":
        return t.permute(0, 3, 1, 2).reshape(B * est.K, -1), None
    if name == "head.mlp.0":
        P = (est.Hin // 32) * (est.Win // 32)
        return t[:, :P], t[:, P:]
    if name == "crop":
        return t[..., :3].permute(0, 3, 1, 2), t[..., 3:]
    if name.startswith("head."):                                               # token matrices (the linears see them as [1, 1, rows, C])
        return t.reshape(B * est.K, -1), None
    return (t.permute(0, 3, 1, 2), None) if t.dim() == 4 else (t, None)


@functools.lru_cache(maxsize=None)
def _stage_yardsticks(emu, flip):
    """-> (the two test images, the fp64 chain's tensors on the stated rule's crops of NET_BOXES)"""
    kw, sd, ref = _tiny(emu)
    W, H = kw["input_size"]
    img = _images(2, 128, 80, 11)
    crops, _ = crop_ref(img, NET_BOXES, NET_INDEX, H, W, flip)
    T = ref.chain(torch.from_numpy(crops[..., :3]).permute(0, 3, 1, 2))
    return img, T


def _network_check(backend, flip):
    emu = backend.is_emu
    kw, sd, ref = _tiny(emu)
    est = _estimator(emu)
    W, H = kw["input_size"]
    img, T64 = _stage_yardsticks(emu, flip)
    R, B = len(NET_BOXES), len(NET_BOXES) * (2 if flip else 1)
    x, boxes, index = _dev(img, backend), _dev(torch.tensor(NET_BOXES), backend), _dev(torch.tensor(NET_INDEX, dtype=torch.int32), backend)
    taps = {}
    est._taps = taps
    try:
        kp_t, sc_t = est(x, boxes, index, flip_test=flip)
    finally:
        est._taps = None
    kp, sc = est(x, boxes, index, flip_test=flip)
    perm = [2, 0, 1]
    kp_p, sc_p = est(x, boxes[perm].contiguous(), index[perm].contiguous(), flip_test=flip)
    backend.sync()
    assert torch.equal(kp, kp_t) and torch.equal(sc, sc_t)                     # tapped = untapped, and a rerun is bit-identical
    assert torch.equal(kp_p, kp[perm]) and torch.equal(sc_p, sc[perm])         # a crop does not depend on its place in the batch
    assert tuple(kp.shape) == (R, est.K, 2) and tuple(sc.shape) == (R, est.K) and kp.device.type == backend.device.type
    want_crop, _ = crop_ref(img, NET_BOXES, NET_INDEX, H, W, flip)
    assert np.array_equal(taps["crop"].cpu().numpy(), want_crop)
    # every tapped tensor against the fp64 restatement of the ONE stage that wrote it, from the product's own recorded inputs
    L, rows = {}, {}                                                           # logical tensors; the measured figures per stage
    for name, t in taps.items():
        if name in ("keypoints", "scores"):
            continue
        L[name], padc = _logical(name, t, est, B)
        assert padc is None or (padc == 0).all(), name                         # padding channels are exactly zero
    names = [n for n, _, _ in ref.stages()]
    assert set(names) == set(L) - {"crop"}, set(names) ^ (set(L) - {"crop"})
    for name, ins, fn in ref.stages():
        args64 = [L[i].double() for i in ins]
        want = fn(torch.float64, _q(None), (), *args64)
        e_ref = _err(fn(torch.float32, _q(None), (), *[L[i].float() for i in ins]), want)
        e_bf = _err(fn(torch.float32, _q(BF), (), *[L[i].float() for i in ins]), want)
        e_dev = _err(L[name], want)
        rows[name] = {"e_ref_fp32_cpu": e_ref, "device": e_dev, "bf16_operands": e_bf}
        print(f"{name:28s} e_ref {e_ref:.3e} device {e_dev:.3e} bf16 {e_bf:.3e}")
        assert e_dev <= FACTOR * e_ref, (name, e_dev, e_ref)
        assert e_bf > FACTOR * e_ref, (name, e_bf, e_ref)
    # keypoints: equal to the fp64 chain's wherever its decision is wider than twice the measured logit error
    nx = 2 * W
    lg64 = T64["head.cls"].reshape(B, est.K, -1).numpy()
    kp_w, sc_w, mx, my = decode_ref(lg64, nx, R, ref.flip_idx if flip else None, NET_BOXES, H, W)
    lg_dev = L["head.cls"].double().reshape(B, est.K, -1).numpy()
    _, _, dx, dy = decode_ref(lg_dev, nx, R, ref.flip_idx if flip else None, NET_BOXES, H, W)
    e_logit = max(np.abs(dx - mx).max(), np.abs(dy - my).max())
    gap = lambda m: np.diff(np.sort(m, -1)[..., -2:], axis=-1)[..., 0]   # noqa: E731
    excused = (gap(mx) <= 2 * e_logit) | (gap(my) <= 2 * e_logit) | (np.abs(sc_w) <= 2 * e_logit)
    share = float(excused.mean())
    print(f"logit error {e_logit:.3e} (max |logit| {np.abs(mx).max():.3e}); excused keypoints {share:.4f}")
    assert share <= 0.02, share
    got_kp, got_sc = kp.cpu().numpy(), sc.cpu().numpy()
    assert np.abs(got_kp - kp_w)[~excused].max() <= 1e-3
    assert np.abs(got_sc - sc_w)[~excused].max() <= 2 * e_logit
    assert (np.ptp(kp_w.reshape(-1, 2), 0) > 4).all()                          # the synthetic network does not answer one point for everything
    return rows, e_logit, share


@pytest.mark.parametrize("flip", [True, False])
def test_network(backend, flip):
    rows, e_logit, share = _network_check(backend, flip)
    if not backend.is_emu:
        worst = max(rows, key=lambda n: rows[n]["device"] / max(rows[n]["e_ref_fp32_cpu"], 1e-300))
        _record(f"network_tiny_flip{int(flip)}", {"stages": rows, "worst_stage": worst, "logit_error": e_logit, "excused_keypoint_share": share,
                                                  "bound": "device <= 16 e_ref per stage; bf16 operands must exceed it"})


def test_forward_refusals_and_struct_layout(backend, tmp_path):
    """pcdm_dwpose_forward / pcdm_dwpose_ws_bytes: arguments outside the stated ranges return -1 and write nothing; the ctypes mirrors of the two
    structs against the header as gcc lays it out"""
    import ctypes
    import shutil
    import subprocess
    from pcdms_amd import _lib, ops
    est = _estimator(backend.is_emu)
    cfg, wt = est._c_args(backend.device)
    img = _dev(_images(1, 70, 50, 3), backend)
    boxes, index = _dev(torch.tensor([[0.0, 0.0, 50.0, 70.0]]), backend), _dev(torch.zeros(1, dtype=torch.int32), backend)
    n = ops.dwpose_ws_bytes(cfg, 1, True)
    assert n > 0 and n % 256 == 0 and ops.dwpose_ws_bytes(cfg, 2, True) > n > ops.dwpose_ws_bytes(cfg, 1, False)
    assert ops.dwpose_ws_bytes(cfg, 0, True) == -1
    ws = torch.empty(n // 4, dtype=torch.float32, device=backend.device)
    kp, sc = ops.dwpose_forward(img, boxes, index, True, cfg, wt, ws)
    backend.sync()
    assert torch.equal(kp, est(img, boxes, index)[0])
    with pytest.raises(RuntimeError, match="code -1"):
        ops.dwpose_forward(img, boxes, index, True, cfg, wt, ws[:-64])                    # a workspace that is too small
    for field, value in (("K", 257), ("Hin", cfg.Hin + 8), ("stem", 12), ("n_stages", 3)):
        bad = _lib.DWPoseConfig.from_buffer_copy(cfg)
        setattr(bad, field, value)
        assert ops.dwpose_ws_bytes(bad, 1, True) == -1, field
        with pytest.raises(RuntimeError, match="code -1"):
            ops.dwpose_forward(img, boxes, index, True, bad, wt, ws)
    for field, value in (("n_conv", wt.n_conv - 1), ("n_dw", wt.n_dw + 1), ("mlp_g", None), ("flip_idx", None)):
        bad = _lib.DWPoseWeights.from_buffer_copy(wt)
        setattr(bad, field, value)
        with pytest.raises(RuntimeError, match="code -1"):
            ops.dwpose_forward(img, boxes, index, True, cfg, bad, ws)
    gcc = shutil.which("gcc")
    if gcc is None:
        return
    structs = {"pcdm_dwpose_config": _lib.DWPoseConfig, "pcdm_dwpose_weights": _lib.DWPoseWeights}
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


@pytest.mark.gpu
def test_graph_capture_gpu(gpu_backend):
    est = _estimator(False)
    img, _ = _stage_yardsticks(False, True)
    x, boxes = _dev(img, gpu_backend), _dev(torch.tensor(NET_BOXES), gpu_backend)
    index = _dev(torch.tensor(NET_INDEX, dtype=torch.int32), gpu_backend)
    kp, sc = est(x, boxes, index)                                              # (also uploads the weights: not capturable)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            kp_g, sc_g = est(x, boxes, index)
    torch.cuda.current_stream().wait_stream(side)
    kp_g.zero_(); sc_g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(kp_g, kp) and torch.equal(sc_g, sc)
    x.copy_(x.flip(2))                                                         # new pixels, the same addresses
    graph.replay()
    torch.cuda.synchronize()
    kp_n, sc_n = est(x, boxes, index)
    torch.cuda.synchronize()
    assert torch.equal(kp_g, kp_n) and torch.equal(sc_g, sc_n) and not torch.equal(kp_n, kp)


# ------------------------------------------------------------------------------------------------ 3. full widths on the GPU, one layer each
def _full_stage(gpu_backend, which, B, hw):
    """one layer of the full-width network (``which``: "csp" = the stage-4 CSP layer, "head") on synthetic weights and a synthetic 1024-channel
    input: the schedule's own code, every tapped tensor teacher forced against the fp64 restatement of its stage"""
    ref, est = _ref(_full_sd(), FULL), _full_est()
    w = est._weights(gpu_backend.device)
    x = torch.randn(B, 1024, *hw, generator=torch.Generator().manual_seed(5)) * 0.5
    xd = _dev(x.permute(0, 2, 3, 1).contiguous(), gpu_backend)
    taps, rows = {}, {}
    est._taps = taps
    try:
        est._csp_layer(xd, w, 4) if which == "csp" else est._head(xd, w)
    finally:
        est._taps = None
    torch.cuda.synchronize()
    L = {n: _logical(n, t, est, B)[0] for n, t in taps.items()}
    L["stage4.spp" if which == "csp" else "stage4"] = x
    for name, ins, fn in ref.stages():
        if name not in taps:
            continue
        want = fn(torch.float64, _q(None), (), *[L[i].double() for i in ins])
        e_ref = _err(fn(torch.float32, _q(None), (), *[L[i].float() for i in ins]), want)
        e_bf = _err(fn(torch.float32, _q(BF), (), *[L[i].float() for i in ins]), want)
        e_dev = _err(L[name], want)
        rows[name] = {"e_ref_fp32_cpu": e_ref, "device": e_dev, "bf16_operands": e_bf}
        print(f"{name:28s} e_ref {e_ref:.3e} device {e_dev:.3e} bf16 {e_bf:.3e}")
        assert e_dev <= FACTOR * e_ref, (name, e_dev, e_ref)
        assert e_bf > FACTOR * e_ref, (name, e_bf, e_ref)
    assert set(rows) == set(taps)
    return rows


FULL = dict(input_size=(288, 384))


@functools.lru_cache(maxsize=None)
def _full_sd():
    """full-width synthetic weights for the two layers test 3 runs (the rest of the state dict is zeros: never run)"""
    shapes = _shapes(FULL)
    g = torch.Generator().manual_seed(17)
    sd = {}
    for k, shp in shapes.items():
        live = k.startswith("backbone.stage4.2.") or k.startswith("head.")
        if not live:
            sd[k] = torch.ones(shp) if k.endswith("running_var") else torch.zeros(shp)
        elif k.endswith("weight") and len(shp) >= 2:
            sd[k] = torch.randn(shp, generator=g) * math.sqrt(2.0 / math.prod(shp[1:]))
        elif k.endswith("bn.weight") or k.endswith("running_var") or k.endswith(".g") or k.endswith("scale"):
            sd[k] = torch.rand(shp, generator=g) + 0.5
        elif k == "head.gau.gamma":
            sd[k] = torch.randn(shp, generator=g) * 0.5 + 1.0
        else:
            sd[k] = (torch.rand(shp, generator=g) * 2 - 1) * 0.2
    return sd


@functools.lru_cache(maxsize=None)
def _full_est():
    from pcdms_amd import pose
    return pose.DWPoseEstimator(_full_sd(), **FULL)


@pytest.mark.gpu
def test_full_width_stage4_csp_gpu(gpu_backend):
    rows = _full_stage(gpu_backend, "csp", 2, (12, 9))
    assert {"stage4.csp.in", "stage4.blocks.2", "stage4.att", "stage4"} <= set(rows)
    _record("full_width_stage4_csp", rows)


@pytest.mark.gpu
def test_full_width_head_gpu(gpu_backend):
    rows = _full_stage(gpu_backend, "head", 2, (12, 9))
    assert {"head.final_layer", "head.gau.core", "head.cls"} <= set(rows)
    _record("full_width_head", rows)


# ------------------------------------------------------------------------------------------------ 4. the bound bites
FAULTS = {"no_identity": "stage1.blocks.0", "sigmoid": "stage2.att", "attention_after": "stage2", "gamma_swapped": "head.gau.core",
          "no_square": "head.gau.core", "no_sqrt_s": "head.gau.core", "scalenorm_scale": "head.mlp.0", "bn_eps": "stage3.down",
          "concat_swapped": "stage3.csp.in"}


def test_faults_are_seen():
    """every named fault, applied to the fp64 restatement of its stage on the clean fp64 inputs, moves the stage by >= 32 e_ref (twice the bound)"""
    kw, sd, ref = _tiny(False)
    W, H = kw["input_size"]
    _, T = _stage_yardsticks(False, True)
    stages = {n: (ins, fn) for n, ins, fn in ref.stages()}
    for fault, name in FAULTS.items():
        ins, fn = stages[name]
        args = [T[i] for i in ins]
        e_ref = _err(fn(torch.float32, _q(None), (), *[a.float() for a in args]), T[name])
        moved = _err(fn(torch.float64, _q(None), (fault,), *args), T[name])
        print(f"{fault:18s} {name:20s} moved {moved:.3e} e_ref {e_ref:.3e}")
        assert moved >= BITE * e_ref and moved >= 4 * e_ref, (fault, moved, e_ref)
    # the decode: the merged logits and the scores
    R, nx = len(NET_BOXES), 2 * W
    lg = T["head.cls"].reshape(2 * R, ref.K, -1).numpy()
    kp, sc, mx, _ = decode_ref(lg, nx, R, ref.flip_idx, NET_BOXES, H, W)
    kp_f, _, mx_f, _ = decode_ref(lg, nx, R, ref.flip_idx, NET_BOXES, H, W, faults=("bins_not_reversed",))
    e_ref = _err(decode_ref(lg.astype(np.float32), nx, R, ref.flip_idx, NET_BOXES, H, W)[2], mx)
    assert _err(mx_f, mx) >= BITE * max(e_ref, 2.0 ** -24) and (np.abs(kp_f - kp).max(-1) > 0.25).mean() > 0.02
    _, sc_f, _, _ = decode_ref(lg, nx, R, ref.flip_idx, NET_BOXES, H, W, faults=("score_max",))
    assert _err(sc_f, sc) >= BITE * 2.0 ** -24 and (sc_f >= sc).all() and (sc_f > sc).any()


# ------------------------------------------------------------------------------------------------ 5. the host layer
def _product_shapes(est_kwargs):
    """the product's own key list for a configuration, without weights"""
    from pcdms_amd import pose
    e = pose.DWPoseEstimator.__new__(pose.DWPoseEstimator)
    W, H = est_kwargs["input_size"]
    e.Win, e.Hin, e.K = W, H, est_kwargs.get("num_keypoints", 133)
    wf, df = est_kwargs.get("widen_factor", 1.0), est_kwargs.get("deepen_factor", 1.0)
    e.stem = int(64 * wf)
    e.stages = [(int(ci * wf), int(co * wf), max(round(nb * df), 1), i, s) for ci, co, nb, i, s in pose._ARCH_P5]
    return e.expected_shapes()


def test_state_dict_keys_are_checked():
    from pcdms_amd import pose
    kw, sd, _ = _tiny(True)
    for k in ("backbone.stage4.1.conv1.conv.weight", "backbone.stage2.1.blocks.1.conv2.depthwise_conv.bn.running_var", "backbone.stage3.1.attention.fc.bias",
              "head.mlp.0.g", "head.gau.res_scale.scale", "head.cls_y.weight"):
        assert k in sd, k                                                      # mmpose's names
        with pytest.raises(KeyError, match=k.replace(".", r"\.")):
            pose.DWPoseEstimator({a: b for a, b in sd.items() if a != k}, **kw)
    with pytest.raises(KeyError, match="neck.reduce"):
        pose.DWPoseEstimator({**sd, "neck.reduce.weight": torch.zeros(1)}, **kw)
    with pytest.raises(KeyError, match="head.gau.gamma"):
        pose.DWPoseEstimator({**sd, "head.gau.gamma": torch.zeros(3, 128)}, **kw)
    with pytest.raises(ValueError):
        pose.DWPoseEstimator(sd, **{**kw, "input_size": (40, 64)})
    with pytest.raises(ValueError):
        pose.DWPoseEstimator(sd, **kw, flip_indices=[0] * 133)
    assert list(pose.COCO_WHOLEBODY_FLIP) == FLIP_133 and all(FLIP_133[FLIP_133[k]] == k for k in range(133))      # the tables spelled out above
    for cfg in (kw, TINY, FULL):
        assert _product_shapes(cfg) == _shapes(cfg), cfg
    full = _shapes(FULL)
    assert len(full) == 5 * (3 + 4 + 2 + 3 * 4 + 3 * (3 + 6 + 6 + 3)) + 8 + 12 and full["backbone.stage4.2.blocks.2.conv1.conv.weight"] == (512, 512, 3, 3)


def test_checkpoint_round_trip_and_refusals(backend, tmp_path):
    from pcdms_amd import pose
    kw, sd, _ = _tiny(True)
    torch.save({"meta": {"epoch": 1}, "state_dict": sd}, tmp_path / "dw.pth")
    a, b = pose.DWPoseEstimator.from_checkpoint(tmp_path / "dw.pth", **kw), pose.DWPoseEstimator(sd, **kw)
    img = _dev(_images(1, 70, 50, 3), backend)
    (kp_a, sc_a), (kp_b, sc_b) = a(img[0]), b(img)                              # one [H, W, 3] image; no boxes: the whole image
    whole = b(img, torch.tensor([[0.0, 0.0, 50.0, 70.0]]))
    backend.sync()
    assert torch.equal(kp_a, kp_b) and torch.equal(sc_a, sc_b) and torch.equal(whole[0], kp_b) and tuple(kp_a.shape) == (1, 133, 2)
    for bad in (dict(images_u8=img.float()), dict(images_u8=img, boxes=torch.zeros(0, 4)), dict(images_u8=img, boxes=torch.zeros(2, 3)),
                dict(images_u8=img, image_index=torch.tensor([0])), dict(images_u8=img, boxes=torch.zeros(2, 4), image_index=torch.tensor([0, 1])),
                dict(images_u8=torch.cat([img, img]), boxes=torch.zeros(3, 4))):
        with pytest.raises(ValueError):
            b(**bad)


def test_estimate_pose_map_is_the_chained_calls(backend):
    from pcdms_amd import pose, preprocess
    est = _estimator(True)
    img = _dev(_images(1, 90, 60, 4)[0], backend)
    got = pose.estimate_pose_map(est, img, detect_resolution=128, image_resolution=64)
    Hd, Wd = pose.detect_size(90, 60, 128)
    kp, sc = est(preprocess.resize(img, (Wd, Hd)))
    want = pose.draw_pose(*pose.wholebody_to_openpose(kp, sc), (Hd, Wd), image_size=pose.detect_size(90, 60, 64))[0]
    backend.sync()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (*pose.detect_size(90, 60, 64), 3) and torch.equal(got, want)
    assert (Hd, Wd) == (192, 128) and got.any()                                # something was drawn


def _load_tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, ROOT / "tools" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_checkpoint(path, emu):
    """a synthetic checkpoint of the tiny configuration in mmpose's layout -> the command-line flags that name that configuration"""
    kw, sd, _ = _tiny(emu)
    torch.save({"meta": {"epoch": 1}, "state_dict": sd}, path)
    return [str(kw["input_size"][0]), str(kw["input_size"][1])], str(kw["widen_factor"]), str(kw["deepen_factor"])


def test_extract_pose_tool_and_driver_loader(backend, tmp_path):
    """tools/extract_pose.py writes the map and a keypoint file tools/render_pose.py renders to the same map; the stage-2 driver's pose loader with
    ``--pose_source estimator`` returns ``estimate_pose_map`` of the picture"""
    from PIL import Image
    from pcdms_amd import pose
    size, widen, deepen = _write_checkpoint(tmp_path / "dw.pth", backend.is_emu)
    img = _images(1, 75, 50, 8)[0]
    Image.fromarray(img).save(tmp_path / "a.png")
    tool = _load_tool("extract_pose")
    assert tool.main([str(tmp_path / "a.png"), "--weights", str(tmp_path / "dw.pth"), "--out", str(tmp_path / "out"), "--image_size", "96", "128",
                      "--input_size", *size, "--widen_factor", widen, "--deepen_factor", deepen,
                      "--detect_resolution", "64", "--device", str(backend.device)]) == 0
    png = np.asarray(Image.open(tmp_path / "out" / "a_pose.png").convert("RGB"))
    with np.load(tmp_path / "out" / "a_pose.npz") as f:
        assert f["keypoints"].shape == (1, 133, 2) and f["scores"].shape == (1, 133) and list(f["size"]) == [64, 64]     # detect_size(128, 96, 64)
    assert png.shape == (192, 128, 3)                                          # detect_size(128, 96, 128)
    kp, sc, (Hd, Wd) = _load_tool("render_pose").load_keypoints(tmp_path / "out" / "a_pose.npz", backend.device)
    assert np.array_equal(pose.draw_pose(kp, sc, (Hd, Wd), image_size=(192, 128))[0].cpu().numpy(), png)    # the file holds what the map was drawn from
    est = pose.DWPoseEstimator.from_checkpoint(tmp_path / "dw.pth", **_tiny(backend.is_emu)[0])
    drv = _load_tool("stage2_batchtest_inpaint_model")
    want = pose.estimate_pose_map(est, _dev(img, backend))
    for on_device in (False, True):
        got = drv.load_pose("unused", "estimator", backend.device, on_device, str(tmp_path / "a.png"), est)
        assert np.array_equal(got.cpu().numpy() if on_device else np.asarray(got), want.cpu().numpy())
    args = drv.build_parser().parse_args([])
    assert args.pose_source == "image" and args.pose_weights is None            # the default is unchanged


@pytest.mark.gpu
def test_stage2_driver_pose_source_estimator_gpu(gpu_backend, tmp_path):
    """The stage-2 driver on the fabricated tiny checkpoints of tests/test_preprocess.py with ``--pose_source estimator``: the same output files as
    ``--pose_source image`` reading the maps ``estimate_pose_map`` gives for the pictures (written losslessly under the driver's file names)."""
    pytest.importorskip("transformers")
    from PIL import Image
    from pcdms_amd import pose
    from tests.test_preprocess import _fabricate_stage2
    drv, common, pairs, W, H = _fabricate_stage2(tmp_path)
    size, widen, deepen = _write_checkpoint(tmp_path / "dw.pth", False)
    est = pose.DWPoseEstimator.from_checkpoint(tmp_path / "dw.pth", **_tiny(False)[0])
    for n in ("a", "b", "c"):
        img = torch.from_numpy(np.array(Image.open(tmp_path / "img" / f"{n}.png").convert("RGB"))).to(gpu_backend.device)
        Image.fromarray(pose.estimate_pose_map(est, img).cpu().numpy()).save(tmp_path / "pose" / f"{n}_pose.png")
        (tmp_path / "pose" / f"{n}_pose.jpg").write_bytes((tmp_path / "pose" / f"{n}_pose.png").read_bytes())       # Pillow goes by content
    (tmp_path / "test_data.json").write_text(json.dumps(pairs))
    files = {}
    for source in ("image", "estimator"):
        args = drv.build_parser().parse_args(common + ["--save_path", str(tmp_path / f"out_{source}"), "--json_path", str(tmp_path / "test_data.json"),
                                                       "--preprocess_device", "gpu", "--pose_source", source, "--pose_weights", str(tmp_path / "dw.pth"), "--pose_input_size", *size,
                                                       "--pose_widen_factor", widen, "--pose_deepen_factor", deepen])
        drv.inference(args, 0, pairs)
        out = tmp_path / f"out_{source}" / "guidancescale2.0_seed42_numsteps3"
        files[source] = {f.name: f.read_bytes() for f in sorted(out.glob("*.png"))}
    assert sorted(files["image"]) == ["a_to_b.png", "b_to_c.png"]
    assert files["estimator"] == files["image"]


# ------------------------------------------------------------------------------------------------ 6. a dormant pin
def _have_mmpose():
    try:
        import mmpose  # noqa: F401
        return True
    except Exception:
        return False


@pytest.mark.gpu
@pytest.mark.skipif(not (_have_mmpose() and os.environ.get("PCDM_DWPOSE_CKPT") and os.environ.get("PCDM_DWPOSE_CONFIG")),
                    reason="needs mmpose, PCDM_DWPOSE_CKPT = the published dw-ll_ucoco_384.pth and PCDM_DWPOSE_CONFIG = its dwpose-l_384x288.py")
def test_pin_against_mmpose(gpu_backend):
    """the published checkpoint through mmpose's inference_topdown (PCDM_DWPOSE_CONFIG = its dwpose-l_384x288.py) against DWPoseEstimator: the same
    keypoints to a quarter of a SimCC bin wherever mmpose's score is confident"""
    from mmpose.apis import inference_topdown, init_model
    from pcdms_amd import pose
    ckpt = os.environ["PCDM_DWPOSE_CKPT"]
    model = init_model(os.environ["PCDM_DWPOSE_CONFIG"], ckpt, device="cuda:0")
    img = _images(1, 384, 288, 21)[0]
    box = np.array([[20.0, 10.0, 260.0, 370.0]], np.float32)
    res = inference_topdown(model, np.ascontiguousarray(img[..., ::-1]), box)[0].pred_instances     # mmpose reads BGR
    kp, sc = pose.DWPoseEstimator.from_checkpoint(ckpt)(_dev(img, gpu_backend), torch.from_numpy(box))
    sure = res.keypoint_scores[0] > 0.5
    assert np.abs(kp.cpu().numpy()[0] - res.keypoints[0])[sure].max() <= 0.25 * 1.25 * 360 / 384 / 2
