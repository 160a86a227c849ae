"""OpenCV's 8-bit Lanczos4 and area resampling on the device (pcdms_amd/preprocess.py: resize_cv; pcdms_amd/pose.py: resize_image; csrc/resize_cv.hip;
include/pcdm.h: pcdm_resize_cv_u8) -- the frame ``controlnet_aux.util.resize_image`` gives both pose networks.

1. BYTES.  An independent numpy restatement of the four arithmetic forms, written here from the header's definitions (int64 and ``np.float32``
   step by step; it shares no table with ``preprocess``): every case must be byte-equal to it, under the lane emulator and on the GPU.
2. DEFINITIONS.  Anchors that do not share the restatement's rounding, each bound computed per output from the coefficients, not chosen: Lanczos4
   against fp64 ``sinc(x) sinc(x / 4)`` resampling, true area against the exact fp64 box integral, integer-ratio area against Pillow's
   ``Image.BOX``.  profiles/resize_cv_values.json records the measured worst cases.
3. PROPERTIES.  Bit-identical reruns, independence of the place in the batch, hipGraph capture and replay.
4. ``estimate_pose_map(frame_resize=...)``, the wrapper's operand checks, operand containment (the cases register in the table of
   tests/test_operand_containment.py at import and run here: on guard pages in a child, with three fills on the GPU), and a dormant comparison
   with the ``cv2`` package.  OpenCV is not a dependency; parity with the package is not pinned by a test that runs by default."""
from __future__ import annotations

import json
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import test_operand_containment as OC

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
PI = math.pi
R45 = 0.70710678118654752440
AB = ((1.0, 0.0), (-R45, -R45), (0.0, 1.0), (R45, -R45), (-1.0, 0.0), (R45, R45), (0.0, -1.0), (-R45, R45))


def _record(key, value):
    path = ROOT / "profiles" / "resize_cv_values.json"
    try:
        values = json.loads(path.read_text()) if path.exists() else {}
        values[key] = value
        path.write_text(json.dumps(values, indent=1, sort_keys=True) + "\n")
    except OSError:
        pass                                                                   # a read-only checkout still runs the assertions


def _images(M, H, W, seed):
    """noise, with hard edges and saturated values in the second image"""
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (M, H, W, 3), dtype=np.uint8)
    if M > 1:
        imgs[1, ::2] = 255 - imgs[1, ::2] // 8
    return imgs


def _dev(a, backend):
    return torch.from_numpy(np.ascontiguousarray(a)).to(backend.device)


# ================================================================================================ the restatement
def axis_scale(n_in, n_out):
    return 1.0 / (float(n_out) / float(n_in))


def lanczos_position(n_in, n_out):
    """-> (s int64 [n_out], t fp32 [n_out])"""
    d = np.arange(n_out, dtype=np.float64)
    f = ((d + 0.5) * axis_scale(n_in, n_out) - 0.5).astype(F32)
    s = np.floor(f)
    return s.astype(np.int64), (f - s).astype(F32)


def lanczos_real(t):
    """the eight fp32 coefficients of one fraction, as the header states them"""
    if t < np.finfo(F32).eps:
        return np.array([0, 0, 0, 1, 0, 0, 0, 0], F32)
    y0 = -(float(t) + 3) * PI / 4
    s0, c0 = math.sin(y0), math.cos(y0)
    c = np.zeros(8, F32)
    total = F32(0)
    for i in range(8):
        y = -(float(t) + 3 - i) * PI / 4
        c[i] = F32((AB[i][0] * s0 + AB[i][1] * c0) / (y * y))
        total = F32(total + c[i])
    r = F32(F32(1) / total)
    return (c * r).astype(F32)


def lanczos_axis(n_in, n_out):
    """-> (source index [n_out, 8] clamped, int64 coefficient [n_out, 8], fp32 coefficient [n_out, 8], t)"""
    s, t = lanczos_position(n_in, n_out)
    real = np.stack([lanczos_real(v) for v in t])
    fixed = np.clip(np.rint((real * F32(2048)).astype(F32)), -32768, 32767).astype(np.int64)
    idx = np.clip(s[:, None] + np.arange(-3, 5)[None, :], 0, n_in - 1)
    return idx, fixed, real, t


def ref_lanczos4(img, Hd, Wd):
    xi, xa, _, _ = lanczos_axis(img.shape[1], Wd)
    yi, yb, _, _ = lanczos_axis(img.shape[0], Hd)
    src = img.astype(np.int64)
    S = (src[:, xi, :] * xa[None, :, :, None]).sum(2)                          # [Hs, Wd, 3], not rounded
    acc = (S[yi] * yb[:, :, None, None]).sum(1)                                # [Hd, Wd, 3]
    return np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def ref_area_box(img, Hd, Wd):
    Hs, Ws = img.shape[:2]
    sy, sx = Hs // Hd, Ws // Wd
    assert sy * Hd == Hs and sx * Wd == Ws
    total = img.astype(np.int64).reshape(Hd, sy, Wd, sx, 3).sum((1, 3))
    if (sx, sy) == (2, 2):
        return ((total + 2) >> 2).astype(np.uint8)
    inv = F32(F32(1) / F32(sx * sy))
    return np.clip(np.rint(total.astype(F32) * inv), 0, 255).astype(np.uint8)


def area_entries(n_in, n_out):
    """per output: [(source, fp32 weight), ...] in the header's order"""
    scale = axis_scale(n_in, n_out)
    out = []
    for d in range(n_out):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, n_in - f1)
        s2 = min(int(math.floor(f2)), n_in - 1)
        s1 = min(int(math.ceil(f1)), s2)
        e = []
        if s1 - f1 > 1e-3:
            e.append((s1 - 1, F32((s1 - f1) / cell)))
        for j in range(s1, s2):
            e.append((j, F32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            e.append((s2, F32(min(min(f2 - s2, 1.0), cell) / cell)))
        out.append(e)
    return out


def ref_area_true(img, Hd, Wd):
    xe, ye = area_entries(img.shape[1], Wd), area_entries(img.shape[0], Hd)
    kx = max(len(e) for e in xe)
    cnt = np.array([len(e) for e in xe])
    xs = np.array([[e[k][0] if k < len(e) else 0 for k in range(kx)] for e in xe])
    xw = np.array([[e[k][1] if k < len(e) else 0 for k in range(kx)] for e in xe], F32)
    src = img.astype(F32)
    out = np.zeros((Hd, Wd, 3), np.uint8)
    for y, rows in enumerate(ye):
        total = None
        for r, beta in rows:
            buf = np.zeros((Wd, 3), F32)
            for k in range(kx):
                m = cnt > k
                buf[m] = buf[m] + src[r, xs[m, k]] * xw[m, k][:, None]         # fp32 product, then fp32 sum: two roundings
            total = beta * buf if total is None else total + beta * buf
        assert total.dtype == F32
        out[y] = np.clip(np.rint(total), 0, 255).astype(np.uint8)
    return out


def area_linear_axis(n_in, n_out, is_x):
    scale = axis_scale(n_in, n_out)
    s0, s1, w0, w1 = [], [], [], []
    for d in range(n_out):
        s = int(math.floor(d * scale))
        t = F32((d + 1) - (s + 1) * (1 / scale))
        t = F32(0) if t <= 0 else F32(t - np.floor(t))
        if is_x and s >= n_in - 1:
            s, t = n_in - 1, F32(0)
        w0.append(int(np.rint(F32(F32(1) - t) * F32(2048))))
        w1.append(int(np.rint(F32(t * F32(2048)))))
        s0.append(min(max(s, 0), n_in - 1))
        s1.append(min(max(s + 1, 0), n_in - 1))
    return np.array(s0), np.array(s1), np.array(w0, np.int64), np.array(w1, np.int64)


def ref_area_linear(img, Hd, Wd):
    xa, xb, a0, a1 = area_linear_axis(img.shape[1], Wd, True)
    ya, yb, b0, b1 = area_linear_axis(img.shape[0], Hd, False)
    src = img.astype(np.int64)
    rows = src[:, xa] * a0[None, :, None] + src[:, xb] * a1[None, :, None]
    S0, S1 = rows[ya], rows[yb]
    v = (((b0[:, None, None] * (S0 >> 4)) >> 16) + ((b1[:, None, None] * (S1 >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def area_rule(Hs, Ws, Hd, Wd):
    sx, sy = axis_scale(Ws, Wd), axis_scale(Hs, Hd)
    eps = np.finfo(np.float64).eps
    if sx >= 1 and sy >= 1:
        return "box" if abs(sx - round(sx)) < eps and abs(sy - round(sy)) < eps else "true"
    return "linear"


def ref_resize_cv(img, Hd, Wd, interpolation):
    """one image uint8 [H, W, 3] -> uint8 [Hd, Wd, 3]"""
    Hs, Ws = img.shape[:2]
    if (Hs, Ws) == (Hd, Wd):
        return img.copy()
    if interpolation == "lanczos4":
        return ref_lanczos4(img, Hd, Wd)
    return {"box": ref_area_box, "true": ref_area_true, "linear": ref_area_linear}[area_rule(Hs, Ws, Hd, Wd)](img, Hd, Wd)


def ref_resize_image(img, resolution):
    H, W = float(img.shape[0]), float(img.shape[1])
    k = float(resolution) / min(H, W)
    Hd, Wd = int(np.round(H * k / 64.0)) * 64, int(np.round(W * k / 64.0)) * 64
    return ref_resize_cv(img, Hd, Wd, "lanczos4" if k > 1 else "area")


# ================================================================================================ 1. bytes
# (interpolation, (Hs, Ws), (Hd, Wd), the arithmetic it must take, M)
CASES = [
    ("lanczos4", (5, 7), (64, 128), "lanczos4", 1),        # fewer than eight source pixels: every tap clamps
    ("lanczos4", (23, 19), (31, 52), "lanczos4", 2),
    ("lanczos4", (41, 29), (17, 11), "lanczos4", 1),       # reduction, no antialiasing
    ("lanczos4", (24, 20), (24, 35), "lanczos4", 1),       # one axis equal
    ("lanczos4", (21, 35), (21, 35), "copy", 2),
    ("area", (24, 36), (12, 18), "box", 2),                # 2 x 2
    ("area", (24, 36), (8, 18), "box", 1),                 # 3 rows x 2 columns
    ("area", (41, 29), (17, 11), "true", 1),
    ("area", (6, 30), (4, 11), "true", 1),                 # 6 -> 4: cell edges on integers, the 1e-3 tests
    ("area", (34, 21), (20, 21), "true", 1),               # scale_x = 1 with scale_y = 1.7
    ("area", (40, 30), (20, 64), "linear", 1),             # one axis enlarged, one reduced
    ("area", (9, 6), (64, 64), "linear", 1),               # both enlarged
    ("area", (41, 29), (17, 11), "true", 2),               # M = 2 with different images
    ("area", (40, 30), (20, 64), "linear", 2),
    ("area", (13, 17), (13, 17), "copy", 1),
]


def _case_id(c):
    return f"{c[0]}-{c[1][0]}x{c[1][1]}-{c[2][0]}x{c[2][1]}-M{c[4]}"


def test_cases_take_the_paths_they_name():
    from pcdms_amd import ops, preprocess
    names = {ops.RESIZE_CV_AREA_INT: "box", ops.RESIZE_CV_AREA: "true", ops.RESIZE_CV_AREA_LINEAR: "linear"}
    for interp, (Hs, Ws), (Hd, Wd), path, _ in CASES:
        if path == "copy":
            assert (Hs, Ws) == (Hd, Wd)
        elif interp == "area":
            assert area_rule(Hs, Ws, Hd, Wd) == path == names[preprocess.cv_area_rule(Hs, Ws, Hd, Wd)], (Hs, Ws, Hd, Wd)
    assert abs(axis_scale(34, 20) - 1.7) < 1e-12 and axis_scale(21, 21) == 1.0
    # 6 -> 4: cells [0, 1.5], [1.5, 3], [3, 4.5], [4.5, 6]: an edge on an integer gives no sliver entry
    assert [[s for s, _ in e] for e in area_entries(6, 4)] == [[0, 1], [1, 2], [3, 4], [4, 5]]
    # 49 : 1 tiles exactly, yet 1 / (1 / 49) is not 49 in fp64: OpenCV takes true area there, and so does the rule picker
    assert axis_scale(49, 1) != 49.0 and preprocess.cv_area_rule(49, 49, 1, 1) == ops.RESIZE_CV_AREA


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_bytes_equal_the_restatement(backend, case):
    from pcdms_amd import preprocess
    interp, (Hs, Ws), (Hd, Wd), path, M = case
    imgs = _images(M, Hs, Ws, Hs * 131 + Wd)
    got = preprocess.resize_cv(_dev(imgs, backend), (Wd, Hd), interp)
    again = preprocess.resize_cv(_dev(imgs, backend), (Wd, Hd), interp)
    backend.sync()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (M, Hd, Wd, 3)
    g = got.cpu().numpy()
    for m in range(M):
        want = ref_resize_cv(imgs[m], Hd, Wd, interp)
        bad = np.argwhere(g[m] != want)
        assert not len(bad), (f"{_case_id(case)} image {m}: {len(bad)} bytes differ, first at {bad[0].tolist()}: "
                              f"{int(g[m][tuple(bad[0])])} vs {int(want[tuple(bad[0])])}")
    assert torch.equal(got, again)                                             # reruns are bit-identical
    if path == "copy":
        assert np.array_equal(g, imgs)
    one = preprocess.resize_cv(_dev(imgs[M - 1], backend), (Wd, Hd), interp)   # rank 3 in, rank 3 out; the image alone = the image in the batch
    backend.sync()
    assert tuple(one.shape) == (Hd, Wd, 3) and torch.equal(one, got[M - 1])


def test_place_in_the_batch(backend):
    """an image's bytes do not depend on where in the batch it lies, nor on its neighbours"""
    from pcdms_amd import preprocess
    imgs = _images(3, 23, 19, 7)
    for interp, (Hd, Wd) in (("lanczos4", (31, 52)), ("area", (10, 8)), ("area", (40, 8))):
        a = preprocess.resize_cv(_dev(imgs, backend), (Wd, Hd), interp)
        b = preprocess.resize_cv(_dev(imgs[::-1], backend), (Wd, Hd), interp)
        backend.sync()
        assert torch.equal(a, b.flip(0))


@pytest.mark.parametrize("hw", [(50, 37), (100, 210), (64, 64)])
@pytest.mark.parametrize("resolution", [64, 128])
def test_resize_image(backend, hw, resolution):
    from pcdms_amd import pose
    img = _images(1, *hw, hw[0] + resolution)[0]
    got = pose.resize_image(_dev(img, backend), resolution)
    backend.sync()
    want = ref_resize_image(img, resolution)
    assert tuple(got.shape) == want.shape == (*pose.detect_size(*hw, resolution), 3)
    assert np.array_equal(got.cpu().numpy(), want)


def test_refusals(backend):
    from pcdms_amd import _lib, ops, preprocess
    img = _dev(_images(1, 9, 6, 1), backend)
    with pytest.raises(ValueError, match="interpolation"):
        preprocess.resize_cv(img, (8, 8), "cubic")
    with pytest.raises(ValueError, match="uint8"):
        preprocess.resize_cv(img.float(), (8, 8))
    with pytest.raises(ValueError, match="positive"):
        preprocess.resize_cv(img, (0, 8))
    # the library itself: -1 and nothing written
    lib, dst = _lib.lib(), torch.full((1, 4, 3, 3), 7, dtype=torch.uint8, device=backend.device)
    s = ops._stream(img)
    tab = torch.zeros(64, dtype=torch.int32, device=backend.device)
    call = lambda src, M, Hs, Ws, d, Hd, Wd, rule, xt, yt: lib.pcdm_resize_cv_u8(src, M, Hs, Ws, d, Hd, Wd, rule, xt, yt, s)   # noqa: E731
    p, d, t = img.data_ptr(), dst.data_ptr(), tab.data_ptr()
    assert call(None, 1, 9, 6, d, 4, 3, 0, t, t) == -1 and call(p, 1, 9, 6, None, 4, 3, 0, t, t) == -1
    assert call(p, 1, 0, 6, d, 4, 3, 0, t, t) == -1 and call(p, 1, 9, 6, d, 4, -3, 0, t, t) == -1 and call(p, -1, 9, 6, d, 4, 3, 0, t, t) == -1
    assert call(p, 1, 9, 6, d, 4, 3, 4, t, t) == -1 and call(p, 1, 9, 6, d, 4, 3, -1, t, t) == -1                  # unknown rule
    for rule in (0, 2, 3):
        assert call(p, 1, 9, 6, d, 4, 3, rule, None, t) == -1 and call(p, 1, 9, 6, d, 4, 3, rule, t, None) == -1   # a table the rule needs
    assert call(p, 1, 9, 6, d, 4, 3, 1, None, None) == -1                                                          # 9 / 4: no integer ratio
    assert call(p, 1, 9, 6, d, 18, 3, 2, t, t) == -1                                                               # true area cannot enlarge
    assert call(p, 1, 1 << 15, 1 << 15, d, 4, 3, 0, t, t) == -1 and call(p, 1, 9, 6, d, 1 << 15, 1 << 15, 0, t, t) == -1   # 2^31 bytes and more
    backend.sync()
    assert bool((dst == 7).all())


def test_wrong_tables_stay_inside(backend):
    """every table entry is clamped on the device: tables of extreme values give some picture, deterministically, and touch nothing else (the guard
    pages and fills below check the same with right tables)"""
    from pcdms_amd import ops
    src = _dev(_images(1, 9, 6, 2), backend)
    for rule in (ops.RESIZE_CV_LANCZOS4, ops.RESIZE_CV_AREA, ops.RESIZE_CV_AREA_LINEAR):
        Hd, Wd = (4, 3) if rule == ops.RESIZE_CV_AREA else (12, 11)
        outs = []
        for fill in (-(1 << 31), (1 << 31) - 1, 0x7FC00000):                   # (the last: NaN as a weight)
            xt = torch.full((ops.resize_cv_table_ints(6, Wd, rule),), fill, dtype=torch.int64).to(torch.int32).to(backend.device)
            yt = torch.full((ops.resize_cv_table_ints(9, Hd, rule),), fill, dtype=torch.int64).to(torch.int32).to(backend.device)
            dst = torch.empty((1, Hd, Wd, 3), dtype=torch.uint8, device=backend.device)
            outs.append((ops.resize_cv_u8(src, dst, rule, xt, yt).clone(), ops.resize_cv_u8(src, dst, rule, xt, yt).clone()))
        backend.sync()
        assert all(torch.equal(a, b) for a, b in outs)


# ================================================================================================ 2. definitions
def _sinc(x):
    x = np.asarray(x, np.float64)
    return np.where(x == 0, 1.0, np.sin(PI * x) / np.where(x == 0, 1.0, PI * x))


def lanczos_f64(t):
    """sinc(x) sinc(x / 4) at the eight taps of fraction t, x = t + 3 - i: fp64, not normalised"""
    x = float(t) + 3 - np.arange(8)
    return _sinc(x) * _sinc(x / 4)


def test_stated_coefficients_are_the_lanczos_kernel():
    """the header's closed form (one sine and one cosine per output; it leaves out the factor sin(pi t) / pi^2 * 4 that all eight taps share, which
    the normalisation removes) IS sinc(x) sinc(x / 4) normalised to sum 1: within 5e-8 per coefficient when evaluated in fp64.  In fp32 as
    stated -- eight roundings, seven sums, a reciprocal and a product, each 2^-24 relative, with sum |c| / |sum c| < 1.8 -- within 16 * 2^-24."""
    worst64 = worst32 = 0.0
    for t in np.concatenate([np.linspace(2e-7, 1, 997, endpoint=False), [1e-3, 0.5, 1 - 2.0 ** -24]]).astype(F32):
        want = lanczos_f64(t)
        want = want / want.sum()
        y0 = -(float(t) + 3) * PI / 4
        c = np.array([(a * math.sin(y0) + b * math.cos(y0)) / (-(float(t) + 3 - i) * PI / 4) ** 2 for i, (a, b) in enumerate(AB)])
        worst64 = max(worst64, float(np.abs(c / c.sum() - want).max()))
        worst32 = max(worst32, float(np.abs(lanczos_real(t).astype(np.float64) - want).max()))
        assert np.abs(want).sum() < 1.8
    print(f"Lanczos4 closed form vs normalised sinc sinc: fp64 {worst64:.3g}, fp32 as stated {worst32:.3g}")
    _record("lanczos4_closed_form_vs_sinc", {"fp64": worst64, "fp32_as_stated": worst32})
    assert worst64 <= 5e-8 and worst32 <= 16 * 2.0 ** -24
    assert list(lanczos_real(F32(0))) == [0, 0, 0, 1, 0, 0, 0, 0] and list(lanczos_real(F32(1e-8))) == [0, 0, 0, 1, 0, 0, 0, 0]


def _lanczos_f64_resample(img, Hd, Wd):
    """-> (fp64 result clipped to [0, 255], the allowed deviation per output pixel)"""
    xi, xa, _, tx = lanczos_axis(img.shape[1], Wd)
    yi, yb, _, ty = lanczos_axis(img.shape[0], Hd)

    def weights(t):
        w = np.stack([lanczos_f64(v) if v >= np.finfo(F32).eps else np.eye(8)[3] for v in t])
        return w / w.sum(1, keepdims=True)
    wx, wy = weights(tx), weights(ty)
    src = img.astype(np.float64)
    S = (src[:, xi, :] * wx[None, :, :, None]).sum(2)
    ref = (S[yi] * wy[:, :, None, None]).sum(1)
    # |kernel - fp64| <= 0.5 (the last rounding) + 255 sum_ij |beta~_i alpha~_j / 2^22 - beta_i alpha_j|
    dev = np.abs(yb[:, None, :, None] * xa[None, :, None, :] / float(1 << 22) - wy[:, None, :, None] * wx[None, :, None, :]).sum((2, 3))
    return np.clip(ref, 0, 255), 0.5 + 255.0 * dev


def test_restatement_of_5x7_is_within_one_level_of_fp64():
    img = _images(1, 5, 7, 3)[0]
    ref, bound = _lanczos_f64_resample(img, 64, 128)
    err = np.abs(ref_lanczos4(img, 64, 128).astype(np.float64) - ref).max()
    print(f"Lanczos4 5x7 -> 64x128 restatement vs fp64: {err:.3f} levels (bound up to {bound.max():.3f})")
    assert err <= 1.0


@pytest.mark.parametrize("src_hw,dst_hw", [((5, 7), (64, 128)), ((23, 19), (31, 52)), ((41, 29), (17, 11))])
def test_lanczos4_against_fp64(backend, src_hw, dst_hw):
    from pcdms_amd import preprocess
    img = _images(2, *src_hw, 11)[1]
    got = preprocess.resize_cv(_dev(img, backend), dst_hw[::-1], "lanczos4").cpu().numpy().astype(np.float64)
    ref, bound = _lanczos_f64_resample(img, *dst_hw)
    err = np.abs(got - ref).max(2)
    print(f"Lanczos4 {src_hw} -> {dst_hw}: max |kernel - fp64| = {err.max():.3f} levels, bound {bound.min():.3f} .. {bound.max():.3f}")
    _record(f"lanczos4_vs_fp64/{backend.name}/{src_hw[0]}x{src_hw[1]}->{dst_hw[0]}x{dst_hw[1]}",
            {"max_err_levels": float(err.max()), "max_bound_levels": float(bound.max()), "max_err_over_bound": float((err / bound).max())})
    assert (err <= bound).all(), float((err / bound).max())


def _box_f64_axis(n_in, n_out):
    """the exact weights of the box [d scale, (d + 1) scale] cut to the image, fp64 [n_out, n_in]"""
    scale = n_in / n_out
    w = np.zeros((n_out, n_in))
    for d in range(n_out):
        lo, hi = d * scale, min((d + 1) * scale, n_in)
        for j in range(int(math.floor(lo)), min(int(math.ceil(hi)), n_in)):
            w[d, j] = max(0.0, min(hi, j + 1) - max(lo, j))
        w[d] /= w[d].sum()
    return w


def _table_weights(n_in, n_out):
    w = np.zeros((n_out, n_in))
    for d, e in enumerate(area_entries(n_in, n_out)):
        for s, a in e:
            w[d, s] += float(a)
    return w


@pytest.mark.parametrize("src_hw,dst_hw", [((41, 29), (17, 11)), ((6, 30), (4, 11)), ((34, 21), (20, 21))])
def test_true_area_against_the_box_integral(backend, src_hw, dst_hw):
    from pcdms_amd import preprocess
    img = _images(2, *src_hw, 5)[1]
    got = preprocess.resize_cv(_dev(img, backend), dst_hw[::-1], "area").cpu().numpy().astype(np.float64)
    wy, wx = _box_f64_axis(src_hw[0], dst_hw[0]), _box_f64_axis(src_hw[1], dst_hw[1])
    ref = np.einsum("yr,rcq,xc->yxq", wy, img.astype(np.float64), wx)
    ty, tx = _table_weights(src_hw[0], dst_hw[0]), _table_weights(src_hw[1], dst_hw[1])
    # 0.5 (the last rounding) + 255 sum |w~ - w| over the products + the fp32 accumulation: n_x products and sums per row, n_y per column, each
    # rounding to 2^-24 relative of a partial sum that never exceeds 255 sum w~
    dev = np.abs(ty[:, None, :, None] * tx[None, :, None, :] - wy[:, None, :, None] * wx[None, :, None, :]).sum((2, 3))
    terms = (ty > 0).sum(1)[:, None] + (tx > 0).sum(1)[None, :] + 2
    acc = 1.01 * terms * 2.0 ** -24 * 255.0 * ty.sum(1)[:, None] * tx.sum(1)[None, :]
    bound = 0.5 + 255.0 * dev + acc
    err = np.abs(got - ref).max(2)
    print(f"area {src_hw} -> {dst_hw}: max |kernel - box integral| = {err.max():.4f} levels, bound {bound.min():.4f} .. {bound.max():.4f}")
    _record(f"area_vs_box_integral/{backend.name}/{src_hw[0]}x{src_hw[1]}->{dst_hw[0]}x{dst_hw[1]}",
            {"max_err_levels": float(err.max()), "max_bound_levels": float(bound.max()), "max_err_over_bound": float((err / bound).max())})
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("src_hw,dst_hw", [((24, 36), (12, 18)), ((24, 36), (8, 18)), ((35, 20), (7, 5))])
def test_integer_area_against_pillow_box(backend, src_hw, dst_hw):
    from PIL import Image
    from pcdms_amd import preprocess
    assert area_rule(*src_hw, *dst_hw) == "box"
    img = _images(2, *src_hw, 9)[1]
    got = preprocess.resize_cv(_dev(img, backend), dst_hw[::-1], "area").cpu().numpy().astype(np.int64)
    pil = np.asarray(Image.fromarray(img).resize(dst_hw[::-1], Image.BOX)).astype(np.int64)
    err = int(np.abs(got - pil).max())
    _record(f"area_int_vs_pillow_box/{backend.name}/{src_hw[0]}x{src_hw[1]}->{dst_hw[0]}x{dst_hw[1]}", err)
    assert err <= 1


# ================================================================================================ 3. properties on the GPU
@pytest.mark.gpu
def test_graph_capture_gpu(gpu_backend):
    """one launch, no host synchronisation once the tables are cached: captured and replayed, the bytes are the eager call's"""
    from pcdms_amd import preprocess
    dev = gpu_backend.device
    for interp, (Hs, Ws), (Hd, Wd) in (("lanczos4", (23, 19), (31, 52)), ("area", (41, 29), (17, 11)), ("area", (24, 36), (8, 18)),
                                       ("area", (40, 30), (20, 64))):
        img = torch.from_numpy(_images(2, Hs, Ws, 13)).to(dev)
        eager = preprocess.resize_cv(img, (Wd, Hd), interp)                    # (also caches the tables)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                out = preprocess.resize_cv(img, (Wd, Hd), interp)
        for _ in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
        assert np.array_equal(eager.cpu().numpy()[0], ref_resize_cv(img[0].cpu().numpy(), Hd, Wd, interp))


# ================================================================================================ 4. estimate_pose_map, wrapper, containment, cv2
def test_estimate_pose_map_frame_resize(backend):
    from pcdms_amd import pose, preprocess
    from tests import test_dwpose as D
    est, frames = D._estimator(True), []

    def recording(frame, boxes=None):
        frames.append(frame)
        return est(frame, boxes)
    img = D._dev(D._images(1, 90, 60, 4)[0], backend)
    kw = dict(detect_resolution=128, image_resolution=64, return_keypoints=True)
    plain, pillow, ref = (pose.estimate_pose_map(recording, img, **kw, **extra) for extra in ({}, {"frame_resize": "pillow"}, {"frame_resize": "reference"}))
    backend.sync()
    assert all(torch.equal(a, b) for a, b in zip(plain[:3], pillow[:3])) and plain[3] == pillow[3] == ref[3] == (192, 128)
    assert torch.equal(frames[0], preprocess.resize(img, (128, 192))) and torch.equal(frames[1], frames[0])      # today's frame, bit for bit
    assert torch.equal(frames[2], pose.resize_image(img, 128)) and not torch.equal(frames[2], frames[0])
    assert np.array_equal(frames[2].cpu().numpy(), ref_resize_cv(img.cpu().numpy(), 192, 128, "lanczos4"))       # k = 128 / 60 > 1
    assert not torch.equal(ref[1], pillow[1])                                  # another frame: other keypoints
    assert ref[0].dtype == torch.uint8 and tuple(ref[0].shape) == (*pose.detect_size(90, 60, 64), 3) and ref[0].any()
    with pytest.raises(ValueError, match="frame_resize"):
        pose.estimate_pose_map(est, img, frame_resize="cv2")


def test_driver_flags_default_to_pillow():
    from tests import test_dwpose as D
    drv = D._load_tool("stage2_batchtest_inpaint_model")
    assert drv.build_parser().parse_args([]).pose_frame_resize == "pillow"
    assert drv.build_parser().parse_args(["--pose_frame_resize", "reference"]).pose_frame_resize == "reference"
    import inspect
    tool = D._load_tool("extract_pose")
    assert inspect.signature(tool.extract).parameters["frame_resize"].default == "pillow"
    assert inspect.signature(drv.load_pose).parameters["frame_resize"].default == "pillow"


def _wrapper_call():
    from pcdms_amd import ops
    I32 = torch.int32
    return {
        "lanczos4": (lambda src, dst, xtab, ytab: ops.resize_cv_u8(src, dst, ops.RESIZE_CV_LANCZOS4, xtab, ytab),
                     dict(src=torch.zeros(2, 9, 6, 3, dtype=torch.uint8), dst=torch.zeros(2, 12, 11, 3, dtype=torch.uint8),
                          xtab=torch.zeros(11 * 9, dtype=I32), ytab=torch.zeros(12 * 9, dtype=I32))),
        "area": (lambda src, dst, xtab, ytab: ops.resize_cv_u8(src, dst, ops.RESIZE_CV_AREA, xtab, ytab),      # 9 -> 4: k = 4; 6 -> 5: k = 3
                 dict(src=torch.zeros(1, 9, 6, 3, dtype=torch.uint8), dst=torch.zeros(1, 4, 5, 3, dtype=torch.uint8),
                      xtab=torch.zeros(5 * 7, dtype=I32), ytab=torch.zeros(4 * 9, dtype=I32))),
        "area_linear": (lambda src, dst, xtab, ytab: ops.resize_cv_u8(src, dst, ops.RESIZE_CV_AREA_LINEAR, xtab, ytab),
                        dict(src=torch.zeros(1, 9, 6, 3, dtype=torch.uint8), dst=torch.zeros(1, 4, 8, 3, dtype=torch.uint8),
                             xtab=torch.zeros(8 * 3, dtype=I32), ytab=torch.zeros(4 * 3, dtype=I32))),
        "area_int": (lambda src, dst: ops.resize_cv_u8(src, dst, ops.RESIZE_CV_AREA_INT),
                     dict(src=torch.zeros(1, 8, 6, 3, dtype=torch.uint8), dst=torch.zeros(1, 4, 2, 3, dtype=torch.uint8))),
    }


@pytest.mark.parametrize("name", ["lanczos4", "area", "area_linear", "area_int"])
def test_wrapper_refuses_before_the_library_is_called(monkeypatch, name):
    """``ops.resize_cv_u8`` against the recording stub of tests/test_operand_containment.py: an operand one element short, of another dtype or
    non-contiguous, and a table one entry short (or one too long), never reach the library"""
    from pcdms_amd import _lib, ops
    stub = OC._Stub()
    monkeypatch.setattr(_lib, "_lib", stub)
    monkeypatch.setattr(_lib, "_is_emu", True)
    call, operands = _wrapper_call()[name]
    call(**operands)
    assert stub.calls == ["pcdm_resize_cv_u8"], "the well-formed call does not reach the library: the case tests nothing"
    for key, t in operands.items():
        spoiled = [t.reshape(-1)[:-1], t.to(OC._OTHER[t.dtype]), OC._spoiled(t, key, "strided")]
        if key.endswith("tab"):
            spoiled += [torch.zeros(t.numel() + 1, dtype=t.dtype), None]
        for bad in spoiled:
            del stub.calls[:]
            with pytest.raises((AssertionError, ValueError, RuntimeError, TypeError, IndexError)):
                call(**dict(operands, **{key: bad}))
            assert not stub.calls, f"ops.resize_cv_u8 ({name}): operand '{key}' reached the library"
    if name == "area_int":
        with pytest.raises(AssertionError):                                    # a table where the rule reads none
            ops.resize_cv_u8(operands["src"], operands["dst"], ops.RESIZE_CV_AREA_INT, torch.zeros(6, dtype=torch.int32))
        assert not stub.calls


# ---- operand containment: one case per rule, registered in the table of tests/test_operand_containment.py (its completeness test counts them) and run
# here.  The bodies go through preprocess.resize_cv: the source, the result and -- the cache is emptied first -- both tables lie at their exact extent.
def _contained(P, interp, src_hw, dst_hw, M=1, seed=0):
    from pcdms_amd import preprocess
    preprocess._CV_TABLES.clear()
    return preprocess.resize_cv(P(OC.ru8(seed + src_hw[0], M, *src_hw, 3), 1), dst_hw[::-1], interp)


@OC.case("resize_cv", "pcdm_resize_cv_u8")
def case_resize_cv_lanczos4(P):
    return [_contained(P, "lanczos4", (5, 7), (64, 128)), _contained(P, "lanczos4", (23, 19), (31, 52), M=2), _contained(P, "lanczos4", (41, 29), (17, 11)),
            _contained(P, "lanczos4", (21, 35), (21, 35), M=2)]


@OC.case("resize_cv", "pcdm_resize_cv_u8")
def case_resize_cv_area_int(P):
    return [_contained(P, "area", (24, 36), (12, 18), M=2), _contained(P, "area", (24, 36), (8, 18)), _contained(P, "area", (35, 20), (7, 5))]


@OC.case("resize_cv", "pcdm_resize_cv_u8")
def case_resize_cv_area(P):
    return [_contained(P, "area", (41, 29), (17, 11), M=2), _contained(P, "area", (6, 30), (4, 11)), _contained(P, "area", (34, 21), (20, 21))]


@OC.case("resize_cv", "pcdm_resize_cv_u8")
def case_resize_cv_area_linear(P):
    return [_contained(P, "area", (40, 30), (20, 64), M=2), _contained(P, "area", (9, 6), (64, 64))]


CONTAINMENT_CASES = ("resize_cv_lanczos4", "resize_cv_area_int", "resize_cv_area", "resize_cv_area_linear")


def test_on_guard_pages():
    """every case on both sides in one child (tests/resize_cv_guard_child.py -> tests/operand_guard_child.py): a byte read or written beyond the
    source, the result or a table kills the child"""
    from tests.emu import build_emu
    build_emu.build()
    r = subprocess.run([sys.executable, "-m", "tests.resize_cv_guard_child", "resize_cv"], cwd=str(ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"the child ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    done = {}
    for line in r.stdout.splitlines():
        m = OC._LINE.match(line.strip())
        if m and m.group(1) == "END":
            done[(m.group(2), m.group(3))] = dict(guarded=int(m.group(4)), allocations=int(m.group(5)), gap=int(m.group(6)), calls=m.group(8).split(","))
    assert set(done) == {(n, s) for n in CONTAINMENT_CASES for s in ("end", "start")}, sorted(done)
    # the sources are placed by the case; the result of every resize and -- except for the integer box and the copy -- its two tables are
    # allocations of the library's Python layer, intercepted and guarded
    allocations = {"resize_cv_lanczos4": 3 * 3 + 1, "resize_cv_area_int": 3, "resize_cv_area": 3 * 3, "resize_cv_area_linear": 2 * 3}
    for (n, s), v in done.items():
        assert v["guarded"] > 0 and v["gap"] <= 15 and v["calls"] == ["pcdm_resize_cv_u8"], (n, s, v)
        assert v["allocations"] == allocations[n], (n, s, v)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONTAINMENT_CASES)
def test_fills_gpu(gpu_backend, name):
    OC.run_fills(name, gpu_backend.device)


def test_cases_are_in_the_table():
    assert all(OC.CASES[n].family == "resize_cv" and OC.CASES[n].exports == ("pcdm_resize_cv_u8",) for n in CONTAINMENT_CASES)
    assert "resize_cv" not in OC.KERNEL_FAMILIES                               # (that tuple was frozen before this module registered: run here)


def test_against_cv2(backend):
    """dormant where OpenCV is absent: the package's own bytes"""
    cv2 = pytest.importorskip("cv2")
    from pcdms_amd import preprocess
    for interp, (Hs, Ws), (Hd, Wd), _, M in CASES:
        img = _images(M, Hs, Ws, 21)[M - 1]
        got = preprocess.resize_cv(_dev(img, backend), (Wd, Hd), interp).cpu().numpy()
        want = cv2.resize(img, (Wd, Hd), interpolation=cv2.INTER_LANCZOS4 if interp == "lanczos4" else cv2.INTER_AREA)
        assert np.array_equal(got, want), (interp, (Hs, Ws), (Hd, Wd), int(np.abs(got.astype(int) - want.astype(int)).max()))
