"""Pose maps from keypoints on the device (pcdms_amd/pose.py, csrc/pose_draw.hip).

1. Whole maps, byte for byte, against a numpy / Python restatement (below) of the reference's arithmetic from keypoints to integers
   (controlnet_aux dwpose: ``DWposeDetector.__call__`` after the networks, ``util.draw_bodypose`` / ``draw_handpose`` / ``draw_facepose``) and of the
   raster rules of include/pcdm.h.  The restatement paints the primitives one after another and applies ``(canvas * 0.6).astype(uint8)`` after the limb
   layer, as the reference does; the device takes, per pixel, the last primitive that covers it.
2. The raster rules against an independent rasteriser, Pillow's: discs and lines exactly, limbs within the stated shares of the polygon OpenCV
   would fill.  Measured here (Pillow 12.2): discs 0, lines 0 mismatches; limbs 3.8 % of the union overall, 9.4 % for the worst limb
   (profiles/pose_values.json).
3. The bilinear resize against a numpy restatement of OpenCV's fixed-point form (bytes) and an fp64 bilinear (within one level).
4. The host-side functions against numpy restatements.
5. Graph capture and run-to-run identity on the GPU.
6. The stage-2 driver with ``--pose_source keypoints`` against ``--pose_source image`` on the PNGs ``tools/render_pose.py`` writes.
7. A dormant pin against OpenCV itself, skipped unless ``cv2`` is installed and ``PCDM_REFERENCE_SRC`` names the ``src`` directory of
   a PCDMs checkout.
"""
from __future__ import annotations

import importlib.util
import json
import math
import os
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
COORD = 1 << 20

LIMB_SEQ = [[2, 3], [2, 6], [3, 4], [4, 5], [6, 7], [7, 8], [2, 9], [9, 10], [10, 11], [2, 12], [12, 13], [13, 14], [2, 1], [1, 15], [15, 17], [1, 16],
            [16, 18], [3, 17], [6, 18]]
BODY_COLORS = [[255, 0, 0], [255, 85, 0], [255, 170, 0], [255, 255, 0], [170, 255, 0], [85, 255, 0], [0, 255, 0], [0, 255, 85], [0, 255, 170],
               [0, 255, 255], [0, 170, 255], [0, 85, 255], [0, 0, 255], [85, 0, 255], [170, 0, 255], [255, 0, 255], [255, 0, 170], [255, 0, 85]]
HAND_EDGES = [[0, 1], [1, 2], [2, 3], [3, 4], [0, 5], [5, 6], [6, 7], [7, 8], [0, 9], [9, 10], [10, 11], [11, 12], [0, 13], [13, 14], [14, 15], [15, 16],
              [0, 17], [17, 18], [18, 19], [19, 20]]


# ------------------------------------------------------------------------------------------------ the yardstick
def hsv_to_rgb(h: float, s: float, v: float):
    """matplotlib.colors.hsv_to_rgb for one colour, in float64."""
    i = int(h * 6.0)
    f = h * 6.0 - i
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    return [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)][i % 6]


HAND_COLORS = [[int(np.rint(c * 255.0)) for c in hsv_to_rgb(e / 20.0, 1.0, 1.0)] for e in range(20)]


def lround(v: float) -> int:
    """C's lround: halves away from zero."""
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


COS = [lround(math.cos(math.radians(t)) * 16384) for t in range(360)]
SIN = [lround(math.sin(math.radians(t)) * 16384) for t in range(360)]


def trunc(v) -> int:
    """int(v), clamped to +-2^20 (include/pcdm.h); NaN: the lower bound."""
    v = float(v)
    if not v > -COORD:
        return -COORD
    return COORD if v > COORD else int(v)


def ref_prims(kp: np.ndarray, sc: np.ndarray, H: int, W: int, hands: bool, faces: bool) -> list:
    """The reference's arithmetic, in its order and precision, from one map's keypoints [P, 134, 2] / scores [P, 134] (fp32) to the integer
    primitives in draw order: ("limb", cx, cy, a, theta, rgb) / ("disc", x, y, r, rgb) / ("line", x0, y0, x1, y1, rgb)."""
    kp, sc = kp.astype(F32), sc.astype(F32)
    P = kp.shape[0]
    cand = kp.copy()
    cand[..., 0] /= float(W)
    cand[..., 1] /= float(H)
    body = cand[:, :18].copy()
    visible = sc[:, :18] > F32(0.3)
    cand[sc < F32(0.3)] = -1
    out = []
    for i in range(17):
        for n in range(P):
            j = np.array(LIMB_SEQ[i]) - 1
            if not visible[n, j].all():
                continue
            Y = body[n, j, 0] * float(W)
            X = body[n, j, 1] * float(H)
            assert Y.dtype == F32 and X.dtype == F32
            with np.errstate(all="ignore"):
                mX, mY = np.mean(X), np.mean(Y)
                length = np.sqrt((X[0] - X[1]) ** 2 + (Y[0] - Y[1]) ** 2)
                a = trunc(length / F32(2))
            if a < 0:
                continue
            dy, dx = float(X[0] - X[1]), float(Y[0] - Y[1])
            theta = 0 if (math.isnan(dy) or math.isnan(dx)) else int(math.degrees(math.atan2(dy, dx)))
            out.append(("limb", trunc(mY), trunc(mX), a, theta, BODY_COLORS[i]))
    for i in range(18):
        for n in range(P):
            if visible[n, i]:
                out.append(("disc", trunc(body[n, i, 0] * F32(W)), trunc(body[n, i, 1] * F32(H)), 4, BODY_COLORS[i]))
    if hands:
        for peaks in list(cand[:, 92:113]) + list(cand[:, 113:134]):
            pts = [(trunc(p[0] * F32(W)), trunc(p[1] * F32(H))) for p in peaks]
            for e, (i0, i1) in enumerate(HAND_EDGES):
                if min(pts[i0] + pts[i1]) >= 1:
                    out.append(("line", *pts[i0], *pts[i1], HAND_COLORS[e]))
            out += [("disc", x, y, 1, [0, 0, 255]) for x, y in pts if x >= 1 and y >= 1]
    if faces:
        for lm in cand[:, 24:92]:
            for p in lm:
                x, y = trunc(p[0] * F32(W)), trunc(p[1] * F32(H))
                if x >= 1 and y >= 1:
                    out.append(("disc", x, y, 3, [255, 255, 255]))
    return out


def limb_mask(H, W, cx, cy, a, theta):
    """The limb rule of include/pcdm.h on an H x W canvas, in Python integers (no overflow at any size)."""
    C, S = COS[theta % 360], SIN[theta % 360]
    y, x = np.mgrid[0:H, 0:W]
    dx, dy = (x - cx).astype(object), (y - cy).astype(object)
    u, v = 2 * (dx * C + dy * S), 2 * (dy * C - dx * S)
    A, B = 2 * a + 1, 9
    m = (abs(u) <= A * 16384) & (abs(v) <= B * 16384) & (B * B * u * u + A * A * v * v <= A * A * B * B * (1 << 28))
    return m.astype(bool)


def limb_mask_fast(H, W, cx, cy, a, theta):
    """``limb_mask`` evaluated only where the limb can be (int64 pre-tests, Python integers for the ellipse test)."""
    C, S = COS[theta % 360], SIN[theta % 360]
    R = max(a, 4) + 8 + a // 4096
    x0, x1, y0, y1 = max(cx - R, 0), min(cx + R, W - 1), max(cy - R, 0), min(cy + R, H - 1)
    m = np.zeros((H, W), bool)
    if x0 > x1 or y0 > y1:
        return m
    y, x = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    dx, dy = x - cx, y - cy
    u, v = 2 * (dx * C + dy * S), 2 * (dy * C - dx * S)
    A, B = 2 * a + 1, 9
    pre = (np.abs(u) <= A * 16384) & (np.abs(v) <= B * 16384)
    uo, vo = u[pre].astype(object), v[pre].astype(object)
    sub = m[y0:y1 + 1, x0:x1 + 1]
    sub[pre] = (B * B * uo * uo + A * A * vo * vo <= A * A * B * B * (1 << 28)).astype(bool)
    return m


def disc_mask(H, W, cx, cy, r):
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    return (x - cx) ** 2 + (y - cy) ** 2 <= r * r + r // 2


def line_pixels(x0, y0, x1, y1):
    """The line rule, walked: the pixel of every step k = 0 .. n along the major axis."""
    ddx, ddy = x1 - x0, y1 - y0
    adx, ady = abs(ddx), abs(ddy)
    sx, sy = (ddx > 0) - (ddx < 0), (ddy > 0) - (ddy < 0)
    n = max(adx, ady)
    if n == 0:
        return [(x0, y0)]
    if adx >= ady:
        return [(x0 + sx * k, y0 + sy * ((2 * k * ady + adx) // (2 * adx))) for k in range(n + 1)]
    return [(x0 + sx * ((2 * k * adx + ady) // (2 * ady)), y0 + sy * k) for k in range(n + 1)]


def line_mask(H, W, x0, y0, x1, y1):
    m = np.zeros((H, W), bool)
    for x, y in line_pixels(x0, y0, x1, y1):
        if 0 <= x < W and 0 <= y < H:
            m[y, x] = True
    return m


def ref_draw(kp, sc, H, W, hands=True, faces=False) -> np.ndarray:
    """One map as the reference draws it: limbs, ``(canvas * 0.6).astype(uint8)``, joints, hands, faces, each primitive over what is there."""
    canvas = np.zeros((H, W, 3), np.uint8)
    prims = ref_prims(kp, sc, H, W, hands, faces)
    for p in prims:
        if p[0] == "limb":
            canvas[limb_mask_fast(H, W, *p[1:5])] = p[5]
    canvas = (canvas * 0.6).astype(np.uint8)
    for p in prims:
        if p[0] == "disc":
            x, y, r = p[1:4]
            if -r <= x < W + r and -r <= y < H + r:
                x0, y0 = max(x - r, 0), max(y - r, 0)
                sub = canvas[y0:y + r + 1, x0:x + r + 1]
                sub[disc_mask(sub.shape[0], sub.shape[1], x - x0, y - y0, r)] = p[4]
        elif p[0] == "line":
            canvas[line_mask(H, W, *p[1:5])] = p[5]
    return canvas


# ------------------------------------------------------------------------------------------------ cases
def blank(P):
    return np.zeros((P, 134, 2), F32), np.zeros((P, 134), F32)


def person(seed, H, W, cx=0.5, cy=0.5, spread=0.22):
    """One fully visible person scattered about (cx, cy) (fractions of the frame), non-integer coordinates."""
    rng = np.random.default_rng(seed)
    kp = (np.array([cx * W, cy * H]) + rng.normal(0, 1, (1, 134, 2)) * np.array([spread * W, spread * H])).astype(F32)
    for base in (92, 113):      # hands: short edges around a wrist
        kp[0, base:base + 21] = kp[0, base] + rng.normal(0, 0.04 * min(H, W), (21, 2)).astype(F32)
    return kp, np.full((1, 134), 0.9, F32)


def limb_person(p0, p1, joints=(1, 2)):
    """A person of which only the two joints of one limb (default neck - right shoulder: limb 0) are visible."""
    kp, sc = blank(1)
    kp[0, joints[0]], kp[0, joints[1]] = p0, p1
    sc[0, list(joints)] = 0.9
    return kp, sc


def stack(people):
    return np.concatenate([p[0] for p in people]), np.concatenate([p[1] for p in people])


def case_maps(name, H, W):
    """-> (list of (keypoints [P, J, 2], scores [P, J]) per map, draw_pose keywords)."""
    s = min(H, W) / 64.0      # the emulator canvases are the unit
    kw = {}
    if name == "multi_person":
        return [person(1, H, W), stack([person(2, H, W), person(3, H, W, 0.55, 0.5), person(4, H, W, 0.45, 0.55)])], kw
    if name == "layering":      # person 0: the nose alone; person 1: limb 0 (red) across it
        kp0, sc0 = blank(1)
        kp0[0, 0] = (0.5 * W + 0.25, 0.5 * H + 0.25)
        sc0[0, 0] = 0.9
        return [stack([(kp0, sc0), limb_person((0.5 * W - 20 * s, 0.5 * H - 3 * s), (0.5 * W + 20 * s, 0.5 * H + 3 * s))])], kw
    if name == "body_threshold":      # the two ends of limb 0 and the nose: exactly 0.3f, the next float, 0.3f
        kp, sc = person(5, H, W, spread=0.1)
        sc[0, :18] = [F32(0.3), np.nextafter(F32(0.3), F32(1)), np.nextafter(F32(0.3), F32(1))] + [F32(0.3)] * 5 + [np.nextafter(F32(0.3), F32(1))] * 10
        return [(kp, sc)], kw
    if name == "hand_threshold":
        kp, sc = person(6, H, W, spread=0.1)
        sc[0, 92:113] = F32(0.3)
        sc[0, 113:134] = np.nextafter(F32(0.3), F32(0))
        sc[0, 24:92] = F32(0.3)
        return [(kp, sc)], dict(faces=True)
    if name == "neck":      # 133-joint input, the left shoulder (mmpose 5) below the threshold: the neck, the shoulder and their six limbs go
        kp, sc = person(7, H, W, spread=0.1)
        kp, sc = np.delete(kp, 17, axis=1), np.delete(sc, 17, axis=1)
        sc[0, 5] = 0.1
        return [(kp, sc)], kw
    if name == "short_limbs":      # a = 0 (ends one pixel apart, and coincident) and a = 1
        c = np.array([0.5 * W, 0.5 * H], F32)
        ends = [((0, 0), (1, 0)), ((0, 0), (0, 0)), ((0, 0), (2, 1)), ((0, 0), (0, 3)), ((0, 0), (-1, -1)), ((0, 0), (2.9, 0))]
        return [stack([limb_person(c + np.array(o, F32) * F32(s) + np.array(a, F32), c + np.array(o, F32) * F32(s) + np.array(b, F32),
                                   joints=(1, 2 if i % 2 == 0 else 5))
                       for i, ((a, b), o) in enumerate(zip(ends, [(-24, -12), (-12, -12), (0, -12), (12, -12), (-12, 8), (8, 8)]))])], kw
    if name == "angles":      # 0, +-90, 180, +-45, +-135 degrees, and a few in between
        c = np.array([0.5 * W, 0.5 * H], F32)
        L = 6 * s
        dirs = [(1, 0), (0, 1), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1), (2, 1), (-1, 3), (3, -2), (-5, -1)]
        people = []
        for i, d in enumerate(dirs):
            o = c + np.array([(i % 4 - 1.5) * 14 * s * W / min(H, W), (i // 4 - 1) * 16 * s], F32)
            people.append(limb_person(o, o + np.array(d, F32) * F32(L), joints=[(1, 2), (1, 5), (2, 3), (5, 6)][i % 4]))
        return [stack(people)], kw
    if name == "limb_outside":      # partly outside, wholly outside, a negative centre, ends far outside the frame (a above 7281)
        return [stack([limb_person((-30 * s, 10 * s), (20 * s, 30 * s)), limb_person((-50 * s, -50 * s), (-20 * s, -30 * s), joints=(1, 5)),
                       limb_person((-9 * s, -2 * s), (-2 * s, -7 * s), joints=(2, 3)), limb_person((W - 5 * s, H + 2 * s), (W + 30 * s, H - 20 * s), joints=(5, 6)),
                       limb_person((-20000.5, 0.4 * H), (30000.25, 0.7 * H), joints=(1, 8)),
                       limb_person((0.3 * W, -900000.0), (0.6 * W, 800000.0), joints=(8, 9))])], kw
    if name == "zero_coordinate":      # x = 0.4 -> int 0: the two edges at that hand point and the point itself go, the body joint stays
        kp, sc = person(8, H, W, spread=0.1)
        kp[0, 92 + 5, 0] = 0.4
        kp[0, 113, 1] = 0.9
        kp[0, 3] = (0.4, 0.5 * H)
        kp[0, 4] = (0.25 * W, 0.0)
        return [(kp, sc)], kw
    if name == "hand_octants":      # the finger chains of both hands walk through all eight octants, plus the axes and diagonals
        steps = [[(10, 3), (3, 10), (-3, 10), (-10, 3)], [(-10, -3), (-3, -10), (3, -10), (10, -3)], [(7, 0), (0, 7), (-7, 0), (0, -7)],
                 [(5, 5), (-5, 5), (-5, -5), (5, -5)], [(9, 1), (1, 9), (-9, -1), (-1, -9)]]
        kp, sc = blank(1)
        for base, wrist in ((92, (0.3 * W, 0.5 * H)), (113, (0.7 * W, 0.5 * H))):
            kp[0, base] = wrist
            for f, chain in enumerate(steps):
                pt = np.array(wrist, F32)
                for k, d in enumerate(chain):
                    pt = pt + np.array(d, F32) * F32(0.5 * s if base == 92 else 0.8 * s)
                    kp[0, base + 1 + 4 * f + k] = pt
            sc[0, base:base + 21] = 0.9
        return [(kp, sc)], kw
    if name == "no_persons":
        return [blank(0)], kw
    if name == "ragged_batch":
        return [stack([person(9, H, W), person(10, H, W, 0.4, 0.6)]), person(11, H, W, 0.6, 0.4)], kw
    if name == "faces":
        return [person(12, H, W)], dict(faces=True)
    if name == "hands":
        return [person(13, H, W)], dict(hands=False)
    raise KeyError(name)


CASES = ["multi_person", "layering", "body_threshold", "hand_threshold", "neck", "short_limbs", "angles", "limb_outside", "zero_coordinate", "hand_octants",
         "no_persons", "ragged_batch", "faces", "hands"]


def canvas_sizes(backend):
    """(H, W): under the emulator 64 x 96 and 53 x 75 (no multiple of the 32 x 8 tile), on the GPU 512 x 512 and 768 x 1024."""
    return [(64, 96), (53, 75)] if backend.is_emu else [(512, 512), (768, 1024)]


def to134(kp, sc):
    from pcdms_amd import pose
    if kp.shape[1] == 134:
        return kp, sc
    k, s = pose.wholebody_to_openpose(kp, sc)
    return k.numpy(), s.numpy()


def device_draw(backend, maps, size, **kw):
    from pcdms_amd import pose
    out = pose.draw_pose([torch.from_numpy(k).to(backend.device) for k, _ in maps], [torch.from_numpy(s).to(backend.device) for _, s in maps], size, **kw)
    backend.sync()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. whole maps
@pytest.mark.parametrize("name", CASES)
def test_map_bytes(backend, name):
    for H, W in canvas_sizes(backend):
        maps, kw = case_maps(name, H, W)
        got = device_draw(backend, maps, (H, W), **kw)
        assert got.shape == (len(maps), H, W, 3) and got.dtype == np.uint8
        for m, (kp, sc) in enumerate(maps):
            want = ref_draw(*to134(kp, sc), H, W, **kw)
            bad = int((got[m] != want).any(axis=2).sum())
            assert bad == 0, f"{name} {W} x {H} map {m}: {bad} pixels differ, first at (y, x) = {np.argwhere((got[m] != want).any(axis=2))[0]}"
            # what each case is about, said outright
            prims = ref_prims(*to134(kp, sc), H, W, kw.get("hands", True), kw.get("faces", False))
            kinds = [p[0] for p in prims]
            if name == "layering":
                x, y = prims[1][1:3]
                assert kinds == ["limb", "disc", "disc", "disc"] and tuple(got[m, y, x]) == (255, 0, 0)      # the nose, over the limb, at full colour
                assert tuple(got[m, y, x + 6]) == (153, 0, 0)                                              # the limb beside it: 255 * 3 / 5
            elif name == "body_threshold":
                assert sum(p[0] == "disc" and p[3] == 4 for p in prims) == 12 and kinds.count("limb") == 9
            elif name == "hand_threshold":
                assert kinds.count("line") == 20 and sum(p[0] == "disc" and p[3] == 1 for p in prims) == 21 and sum(p[0] == "disc" and p[3] == 3 for p in prims) == 68
            elif name == "neck":
                assert kinds.count("limb") == 11 and sum(p[0] == "disc" and p[3] == 4 for p in prims) == 16
            elif name == "short_limbs":
                assert sorted(p[3] for p in prims if p[0] == "limb") == [0, 0, 0, 1, 1, 1]
            elif name == "angles":
                # (the diagonals are exact where k / W * W returns k for every coordinate: the power-of-two canvas)
                exact = {0, 90, -90, 180} | ({45, -45, 135, -135} if (H & (H - 1)) == 0 and (W & (W - 1)) == 0 else set())
                assert {p[4] for p in prims if p[0] == "limb"} >= exact
            elif name == "limb_outside":
                assert max(p[3] for p in prims if p[0] == "limb") > 7281 and min(p[1] for p in prims if p[0] == "limb") < 0
            elif name == "zero_coordinate":
                assert kinds.count("line") == 40 - 7 and sum(p[0] == "disc" and p[3] == 1 for p in prims) == 40 and sum(p[0] == "disc" and p[3] == 4 for p in prims) == 18
            elif name == "no_persons":
                assert not got.any()
            elif name == "faces":
                assert np.array_equal(device_draw(backend, maps, (H, W))[m], ref_draw(kp, sc, H, W)) and (got[m] != ref_draw(kp, sc, H, W)).any()
            elif name == "hands":
                assert "line" not in kinds


def test_hand_octants_cover_all_eight(backend):
    H, W = canvas_sizes(backend)[0]
    (kp, sc), = case_maps("hand_octants", H, W)[0]
    octs = set()
    for p in ref_prims(kp, sc, H, W, True, False):
        if p[0] == "line":
            dx, dy = p[3] - p[1], p[4] - p[2]
            if dx and dy and abs(dx) != abs(dy):
                octs.add((dx > 0, dy > 0, abs(dx) > abs(dy)))
    assert len(octs) == 8


def test_limits_are_refused(backend):
    from pcdms_amd import ops, pose
    dev = backend.device
    kp, sc = torch.zeros((1, 33, 134, 2), device=dev), torch.zeros((1, 33, 134), device=dev)
    with pytest.raises(ValueError, match="32 persons"):
        pose.draw_pose(kp, sc, (64, 64))
    with pytest.raises(ValueError, match="4096"):
        pose.draw_pose(kp[:, :1], sc[:, :1], (8, 4097))
    assert ops.pose_ws_bytes(1, 33) == -1 and ops.pose_ws_bytes(1, 32) == 32 * 185 * 32
    tables = pose._tables(dev)
    sentinel = torch.full((1, 2, 4097, 3), 7, dtype=torch.uint8, device=dev)
    ws = torch.zeros(33 * 185 * 32, dtype=torch.uint8, device=dev)
    for k, s, out in ((kp[:, :1], sc[:, :1], sentinel), (kp[:, :1], sc[:, :1], sentinel.view(1, 4097, 2, 3)), (kp, sc, sentinel[:, :, :64])):
        with pytest.raises(RuntimeError, match="code -1"):
            ops.pose_draw(k.contiguous(), s.contiguous(), tables, out.contiguous(), ws, hands=True, faces=False)
    backend.sync()
    assert bool((sentinel == 7).all())      # a refusal writes nothing
    big = pose.draw_pose(kp[:, :32], sc[:, :32], (16, 40))      # 32 persons are taken
    backend.sync()
    assert not big.any()


# ------------------------------------------------------------------------------------------------ 2. the rules against Pillow
def test_discs_against_pillow():
    for r in (1, 3, 4):
        for cx, cy in ((12, 11), (0, 0), (2, 19), (23, 1)):
            img = Image.new("L", (24, 20))
            ImageDraw.Draw(img).ellipse([cx - r, cy - r, cx + r, cy + r], fill=255)
            assert np.array_equal(np.asarray(img) > 0, disc_mask(20, 24, cx, cy, r)), (r, cx, cy)


def test_lines_against_pillow():
    rng = np.random.default_rng(20)
    H, W = 90, 120
    for i in range(300):
        x0, x1 = (int(v) for v in rng.integers(-20, W + 20, 2))
        y0, y1 = (int(v) for v in rng.integers(-20, H + 20, 2))
        if i % 10 == 0:
            x1 = x0          # vertical, horizontal and single-pixel segments among them
        if i % 15 == 0:
            y1 = y0
        img = Image.new("L", (W, H))
        ImageDraw.Draw(img).line([(x0, y0), (x1, y1)], fill=255, width=1)
        assert np.array_equal(np.asarray(img) > 0, line_mask(H, W, x0, y0, x1, y1)), (x0, y0, x1, y1)


def ellipse2poly(cx, cy, a, b, theta):
    """The 361 vertices of cv2.ellipse2Poly((cx, cy), (a, b), theta, 0, 360, 1), rounded half to even as cvRound does."""
    al, be = math.cos(math.radians(theta)), math.sin(math.radians(theta))
    pts = []
    for i in range(361):
        x, y = a * math.cos(math.radians(i)), b * math.sin(math.radians(i))
        pts.append((int(np.rint(cx + x * al - y * be)), int(np.rint(cy + x * be + y * al))))
    return pts


def limb_shares(limbs, H, W, polygon):
    """(overall share, worst share) of the pixels that differ between the limb rule and ``polygon(limb) -> mask``, relative to the union."""
    diff = union = 0
    worst = 0.0
    for cx, cy, a, theta in limbs:
        rule, poly = limb_mask_fast(H, W, cx, cy, a, theta), polygon(cx, cy, a, theta)
        d, u = int((rule != poly).sum()), int((rule | poly).sum())
        diff, union, worst = diff + d, union + u, max(worst, d / u)
    return diff / union, worst


def seeded_limbs():
    rng = np.random.default_rng(2024)
    return [(int(rng.integers(80, 120)), int(rng.integers(80, 120)), int(rng.integers(4, 70)), int(rng.integers(-180, 181))) for _ in range(400)]


def test_limbs_against_pillow_polygon():
    H = W = 200

    def polygon(cx, cy, a, theta):
        img = Image.new("L", (W, H))
        ImageDraw.Draw(img).polygon(ellipse2poly(cx, cy, a, 4, theta), fill=255, outline=255)
        return np.asarray(img) > 0

    overall, worst = limb_shares(seeded_limbs(), H, W, polygon)
    print(f"limb rule vs Pillow polygon of the ellipse2Poly vertices: {overall:.4f} of the union overall, {worst:.4f} worst limb")
    assert overall <= 0.06 and worst <= 0.12, (overall, worst)


def test_fast_limb_mask_is_the_rule():
    """The yardstick's bounding-box evaluation against the rule evaluated on every pixel in Python integers."""
    for cx, cy, a, theta in [(20, 15, 0, 0), (20, 15, 1, 45), (-5, 3, 9, -30), (20, 15, 30, 77), (40, 30, 9000, 3), (10, 10, 600000, -91)]:
        assert np.array_equal(limb_mask(40, 50, cx, cy, a, theta), limb_mask_fast(40, 50, cx, cy, a, theta)), (cx, cy, a, theta)


def test_device_map_against_pillow(backend):
    """Hands (lines, discs of radius 1), joints (radius 4) and face points (radius 3) drawn by the device against the same primitives drawn
    by Pillow, no limb in the map: 0 mismatching pixels."""
    H, W = canvas_sizes(backend)[1]
    maps = []
    for seed in (31, 32, 33):
        kp, sc = person(seed, H, W)
        sc[0, 1:18] = 0.0                        # the nose is the only body joint: no limb
        maps.append((kp, sc))
    got = device_draw(backend, maps, (H, W), faces=True)
    for m, (kp, sc) in enumerate(maps):
        img = Image.new("RGB", (W, H))
        d = ImageDraw.Draw(img)
        for p in ref_prims(kp, sc, H, W, True, True):
            if p[0] == "disc":
                d.ellipse([p[1] - p[3], p[2] - p[3], p[1] + p[3], p[2] + p[3]], fill=tuple(p[4]))
            else:
                d.line([(p[1], p[2]), (p[3], p[4])], fill=tuple(p[5]), width=1)
        assert np.array_equal(got[m], np.asarray(img)), int((got[m] != np.asarray(img)).any(axis=2).sum())


# ------------------------------------------------------------------------------------------------ 3. bilinear resize
def lin_coeffs(n_in, n_out, clamp_frac):
    scale = 1.0 / (n_out / n_in)
    s0, s1, w0, w1 = [], [], [], []
    for d in range(n_out):
        f = F32((d + 0.5) * scale - 0.5)
        fl = np.floor(f)
        s, t = int(fl), F32(f - fl)
        if clamp_frac:
            if s < 0:
                s, t = 0, F32(0)
            if s >= n_in - 1:
                s, t = n_in - 1, F32(0)
        w0.append(int(np.rint(F32(F32(1) - t) * F32(2048))))
        w1.append(int(np.rint(F32(t * F32(2048)))))
        s0.append(min(max(s, 0), n_in - 1))
        s1.append(min(max(s + 1, 0), n_in - 1))
    return np.array(s0), np.array(s1), np.array(w0), np.array(w1)


def ref_resize_linear(img: np.ndarray, Hd: int, Wd: int) -> np.ndarray:
    """OpenCV's 8-bit INTER_LINEAR in its fixed-point form (include/pcdm.h: pcdm_resize_linear_u8), int32 numpy."""
    xa, xb, a0, a1 = lin_coeffs(img.shape[1], Wd, True)
    ya, yb, b0, b1 = lin_coeffs(img.shape[0], Hd, False)
    src = img.astype(np.int32)
    rows = src[:, xa] * a0[None, :, None] + src[:, xb] * a1[None, :, None]
    S0, S1 = rows[ya], rows[yb]
    return ((((b0[:, None, None] * (S0 >> 4)) >> 16) + ((b1[:, None, None] * (S1 >> 4)) >> 16) + 2) >> 2).astype(np.uint8)


def ref_bilinear_f64(img: np.ndarray, Hd: int, Wd: int) -> np.ndarray:
    def axis(n_in, n_out):
        f = np.clip((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0, n_in - 1)
        s = np.minimum(np.floor(f).astype(int), max(n_in - 2, 0))
        return s, np.minimum(s + 1, n_in - 1), f - s
    ya, yb, ty = axis(img.shape[0], Hd)
    xa, xb, tx = axis(img.shape[1], Wd)
    src = img.astype(np.float64)
    rows = src[:, xa] * (1 - tx)[None, :, None] + src[:, xb] * tx[None, :, None]
    return rows[ya] * (1 - ty)[:, None, None] + rows[yb] * ty[:, None, None]


@pytest.mark.parametrize("src_hw,dst_hw", [((32, 32), (64, 64)), ((40, 24), (77, 61)), ((30, 30), (23, 19)), ((21, 35), (21, 35))])
def test_resize_linear(backend, src_hw, dst_hw):
    from pcdms_amd import ops
    rng = np.random.default_rng(sum(src_hw) + dst_hw[0])
    imgs = rng.integers(0, 256, (2, *src_hw, 3), dtype=np.uint8)
    imgs[1, ::2] = 255 - imgs[1, ::2] // 8      # hard edges and saturated values
    dst = torch.empty((2, *dst_hw, 3), dtype=torch.uint8, device=backend.device)
    ops.resize_linear_u8(torch.from_numpy(imgs).to(backend.device), dst)
    backend.sync()
    got = dst.cpu().numpy()
    worst = 0.0
    for m in range(2):
        assert np.array_equal(got[m], ref_resize_linear(imgs[m], *dst_hw))
        worst = max(worst, float(np.abs(got[m].astype(np.float64) - ref_bilinear_f64(imgs[m], *dst_hw)).max()))
    print(f"resize_linear {src_hw} -> {dst_hw}: max |fixed point - fp64 bilinear| = {worst:.3f} levels")
    assert worst <= 1.0
    if src_hw == dst_hw:
        assert np.array_equal(got, imgs)


def test_draw_pose_image_size(backend):
    """``image_size``: the map drawn at the detection size, then the bilinear step; ``out=`` is filled and returned."""
    from pcdms_amd import pose
    H, W = canvas_sizes(backend)[1]
    kp, sc = person(40, H, W)
    k, s = torch.from_numpy(kp).to(backend.device), torch.from_numpy(sc).to(backend.device)
    Hi, Wi = (H * 3) // 2 + 1, (W * 3) // 2 - 2
    out = torch.empty((1, Hi, Wi, 3), dtype=torch.uint8, device=backend.device)
    assert pose.draw_pose(k, s, (H, W), image_size=(Hi, Wi), out=out) is out
    backend.sync()
    assert np.array_equal(out.cpu().numpy()[0], ref_resize_linear(ref_draw(kp, sc, H, W), Hi, Wi))
    with pytest.raises(ValueError, match="out must be"):
        pose.draw_pose(k, s, (H, W), out=out)


# ------------------------------------------------------------------------------------------------ 4. host-side functions
def test_wholebody_to_openpose():
    from pcdms_amd import pose
    rng = np.random.default_rng(3)
    kp = rng.uniform(0, 500, (4, 133, 2)).astype(F32)
    sc = rng.uniform(0, 1, (4, 133)).astype(F32)
    sc[0, 5], sc[1, 6], sc[2, 5], sc[2, 6] = F32(0.3), F32(0.3), np.nextafter(F32(0.3), F32(1)), np.nextafter(F32(0.3), F32(1))
    # dwpose/wholebody.py:97-119 on fp32 arrays
    info = np.concatenate((kp, sc[..., None]), axis=-1)
    neck = np.mean(info[:, [5, 6]], axis=1)
    neck[:, 2] = np.logical_and(info[:, 5, 2] > F32(0.3), info[:, 6, 2] > F32(0.3)).astype(int)
    new = np.insert(info, 17, neck, axis=1)
    mmpose_idx = [17, 6, 8, 10, 7, 9, 12, 14, 16, 13, 15, 2, 1, 4, 3]
    openpose_idx = [1, 2, 3, 4, 6, 7, 8, 9, 10, 12, 13, 14, 15, 16, 17]
    new[:, openpose_idx] = new[:, mmpose_idx]
    assert info.dtype == F32
    k, s = pose.wholebody_to_openpose(kp, sc)
    assert k.dtype == torch.float32 and tuple(k.shape) == (4, 134, 2) and tuple(s.shape) == (4, 134)
    assert np.array_equal(k.numpy(), new[..., :2]) and np.array_equal(s.numpy(), new[..., 2])
    assert s[:, 1].tolist() == [0.0, 0.0, 1.0, float(sc[3, 5] > F32(0.3) and sc[3, 6] > F32(0.3))]
    k1, s1 = pose.wholebody_to_openpose(torch.from_numpy(kp[0]), torch.from_numpy(sc[0]))      # one person, no leading axis
    assert torch.equal(k1, k[0]) and torch.equal(s1, s[0])
    with pytest.raises(ValueError):
        pose.wholebody_to_openpose(kp[:, :132], sc[:, :132])


def test_detect_size():
    from pcdms_amd import pose

    def restated(H, W, resolution):      # controlnet_aux/util.py:87-95
        H, W = float(H), float(W)
        k = float(resolution) / min(H, W)
        H *= k
        W *= k
        return int(np.round(H / 64.0)) * 64, int(np.round(W / 64.0)) * 64

    rng = np.random.default_rng(4)
    shapes = [(512, 512), (1101, 750), (256, 176), (96, 160), (480, 640), (100, 300)] + [tuple(int(v) for v in rng.integers(40, 2000, 2)) for _ in range(200)]
    for H, W in shapes:
        for res in (512, 256, 96, 160, 1024):
            assert pose.detect_size(H, W, res) == restated(H, W, res), (H, W, res)
    assert pose.detect_size(96, 160, 96) == (128, 128)      # 1.5 and 2.5 both round to 2: half to even
    assert pose.detect_size(1101, 750, 512) == (768, 512)


def test_constant_tables(backend):
    from pcdms_amd import ops
    t = ops.pose_tables()
    assert len(t) == 740 and t[0:720:2] == COS and t[1:720:2] == SIN
    assert [[c & 255, (c >> 8) & 255, (c >> 16) & 255] for c in t[720:]] == HAND_COLORS


def test_hand_colours_are_matplotlibs():
    colors = pytest.importorskip("matplotlib.colors")
    for e in range(20):
        assert np.array_equal(np.rint(colors.hsv_to_rgb([e / 20.0, 1.0, 1.0]) * 255), HAND_COLORS[e]), e


# ------------------------------------------------------------------------------------------------ 5. GPU only
@pytest.mark.gpu
def test_graph_replay_and_reruns(gpu_backend):
    from pcdms_amd import pose
    dev = gpu_backend.device
    H, W = 512, 512
    maps, _ = case_maps("ragged_batch", H, W)
    P = max(k.shape[0] for k, _ in maps)
    kp, sc = torch.zeros((2, P, 134, 2), device=dev), torch.zeros((2, P, 134), device=dev)
    for m, (k, s) in enumerate(maps):
        kp[m, :k.shape[0]], sc[m, :k.shape[0]] = torch.from_numpy(k).to(dev), torch.from_numpy(s).to(dev)
    eager = pose.draw_pose(kp, sc, (H, W), image_size=(640, 576), faces=True).clone()
    again = pose.draw_pose(kp, sc, (H, W), image_size=(640, 576), faces=True)
    torch.cuda.synchronize()
    assert torch.equal(eager, again) and bool(eager.any())
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pose.draw_pose(kp, sc, (H, W), image_size=(640, 576), faces=True, out=out)      # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pose.draw_pose(kp, sc, (H, W), image_size=(640, 576), faces=True, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ------------------------------------------------------------------------------------------------ 6. callers
def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name, ROOT / "tools" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_keypoints(path, seed, H, W):
    kp, sc = stack([person(seed, H, W), person(seed + 50, H, W, 0.45, 0.55)])
    np.savez(path, keypoints=kp, scores=sc, size=np.array([W, H]))
    return kp, sc


def test_render_pose_tool_and_driver_loader(backend, tmp_path):
    """tools/render_pose.py writes the map of a keypoint file as a PNG; the stage-2 driver's pose loader returns the same pixels from the PNG
    (``--pose_source image``) and from the keypoint file (``keypoints``), on the host path and on the ``--preprocess_device gpu`` path."""
    H, W = 96, 64
    kp, sc = _write_keypoints(tmp_path / "a_pose.npz", 60, H, W)
    tool = _load_tool("render_pose")
    assert tool.main([str(tmp_path / "a_pose.npz"), str(tmp_path / "a_pose.png"), "--device", str(backend.device)]) == 0
    png = np.asarray(Image.open(tmp_path / "a_pose.png").convert("RGB"))
    assert np.array_equal(png, ref_draw(kp, sc, H, W))
    (tmp_path / "a_pose.jpg").write_bytes((tmp_path / "a_pose.png").read_bytes())      # the driver's file name; Pillow goes by content
    drv = _load_tool("stage2_batchtest_inpaint_model")
    path = str(tmp_path / "a_pose.jpg")
    for on_device in (False, True):
        a, b = drv.load_pose(path, "image", backend.device, on_device), drv.load_pose(path, "keypoints", backend.device, on_device)
        if on_device:
            assert a.device == b.device == backend.device and torch.equal(a, b) and np.array_equal(a.cpu().numpy(), png)
        else:
            assert isinstance(b, Image.Image) and a.mode == b.mode == "RGB" and np.array_equal(np.asarray(a), np.asarray(b))
    assert drv.build_parser().parse_args([]).pose_source == "image"
    # 133-joint files and the resize to an image resolution
    np.savez(tmp_path / "b.npz", keypoints=np.delete(kp, 17, axis=1), scores=np.delete(sc, 17, axis=1), size=np.array([W, H]))
    assert tool.main([str(tmp_path / "b.npz"), str(tmp_path / "b.png"), "--device", str(backend.device), "--image_resolution", "128"]) == 0
    from pcdms_amd import pose
    k134, s134 = to134(np.delete(kp, 17, axis=1), np.delete(sc, 17, axis=1))
    Hi, Wi = pose.detect_size(H, W, 128)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "b.png")), ref_resize_linear(ref_draw(k134, s134, H, W), Hi, Wi))


@pytest.mark.gpu
def test_stage2_driver_pose_source_keypoints_writes_the_same_files(gpu_backend, tmp_path):
    """The stage-2 driver on the fabricated tiny checkpoints of tests/test_preprocess.py: the pose maps rendered to PNG by tools/render_pose.py and
    read with ``--pose_source image``, against ``--pose_source keypoints`` rendering them on the device: identical output files."""
    pytest.importorskip("transformers")
    from tests.test_preprocess import _fabricate_stage2
    drv, common, pairs, W, H = _fabricate_stage2(tmp_path)
    tool = _load_tool("render_pose")
    for i, n in enumerate(("a", "b", "c")):
        _write_keypoints(tmp_path / "pose" / f"{n}_pose.npz", 70 + i, 150, 90)
        assert tool.main([str(tmp_path / "pose" / f"{n}_pose.npz"), str(tmp_path / "pose" / f"{n}_pose.png")]) == 0
        (tmp_path / "pose" / f"{n}_pose.jpg").write_bytes((tmp_path / "pose" / f"{n}_pose.png").read_bytes())      # the driver's file name; Pillow goes by content
    (tmp_path / "test_data.json").write_text(json.dumps(pairs))
    files = {}
    for source in ("image", "keypoints"):
        args = drv.build_parser().parse_args(common + ["--save_path", str(tmp_path / f"out_{source}"), "--json_path", str(tmp_path / "test_data.json"),
                                                       "--preprocess_device", "gpu", "--pose_source", source])
        drv.inference(args, 0, pairs)
        out = tmp_path / f"out_{source}" / "guidancescale2.0_seed42_numsteps3"
        files[source] = {f.name: f.read_bytes() for f in sorted(out.glob("*.png"))}
    assert sorted(files["image"]) == ["a_to_b.png", "b_to_c.png"]
    assert files["keypoints"] == files["image"]


# ------------------------------------------------------------------------------------------------ 7. dormant pin against OpenCV
def test_limbs_against_opencv_and_reference_draw():
    """Skipped unless OpenCV is installed and PCDM_REFERENCE_SRC names the reference's src directory: the limb rule against cv2.ellipse2Poly + fillConvexPoly with the caps of
    test_limbs_against_pillow_polygon, and whole maps against the reference's own draw_pose (the shares are printed)."""
    cv2 = pytest.importorskip("cv2")
    ref = Path(os.environ.get("PCDM_REFERENCE_SRC", ""))      # the src directory of a PCDMs checkout
    if not os.environ.get("PCDM_REFERENCE_SRC") or not (ref / "controlnet_aux" / "dwpose" / "util.py").exists():
        pytest.skip("no reference tree (PCDM_REFERENCE_SRC)")
    H = W = 200

    def polygon(cx, cy, a, theta):
        img = np.zeros((H, W), np.uint8)
        cv2.fillConvexPoly(img, cv2.ellipse2Poly((cx, cy), (a, 4), theta, 0, 360, 1), 255)
        return img > 0

    overall, worst = limb_shares(seeded_limbs(), H, W, polygon)
    print(f"limb rule vs cv2.fillConvexPoly: {overall:.4f} of the union overall, {worst:.4f} worst limb")
    assert overall <= 0.06 and worst <= 0.12, (overall, worst)
    spec = importlib.util.spec_from_file_location("ref_dwpose_util", ref / "controlnet_aux" / "dwpose" / "util.py")
    util = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(util)
    Hc, Wc = 256, 192
    kp, sc = person(90, Hc, Wc)
    cand = kp.copy()
    cand[..., 0] /= float(Wc)
    cand[..., 1] /= float(Hc)
    subset = np.where(sc[:, :18] > 0.3, np.arange(18, dtype=np.float32)[None], -1)
    canvas = util.draw_bodypose(np.zeros((Hc, Wc, 3), np.uint8), cand[:, :18].reshape(18, 2), subset)
    canvas = util.draw_handpose(canvas, np.vstack([cand[:, 92:113], cand[:, 113:]]))
    want = ref_draw(kp, sc, Hc, Wc)
    share = float((canvas != want).any(axis=2).sum()) / float(((canvas != 0) | (want != 0)).any(axis=2).sum())
    print(f"whole map vs the reference's draw_pose: {share:.4f} of the drawn pixels differ")
    assert share <= 0.06, share
