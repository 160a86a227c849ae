"""The reference's metric scripts on the device (tools/calculate_metrics.py; csrc/image_prep.hip, csrc/image_metrics.hip): OpenCV's INTER_CUBIC float resize, L1 / MAE and the uniform-window
SSIM with the sample covariance, each against an fp64 restatement written here.  OpenCV and scikit-image are not dependencies; parity with the
packages themselves is not pinned.

Yardsticks and bounds
* resize: indices, ``t`` and the four coefficients exactly as include/pcdm.h states them (the fp32 coefficient values included), products and sums
  in fp64.  ``|device - yardstick| <= 16 * 2^-24 * 255 * 1.375^2 = 4.6e-4`` on 0 .. 255 inputs (1.375: the largest absolute coefficient sum of one
  pass, at t = 0.5; 16 roundings: a generous count for two 4-tap passes), divided by 255 with ``divisor=255``.  Equality where the arithmetic is
  exact (2 : 1 on dyadic inputs, identity).
* l1 / mae: numpy fp64 sums of the fp32 elementwise values; relative 1e-6 for fp32 inputs (only the final rounding is left), equality of the fp32
  result for uint8 inputs.
* box SSIM: the formula in fp64; ``|device - fp64| <= 1e-5``, the bound of the Gaussian SSIM (the same centred fp64 formulation).
The worst measured values per backend go to profiles/eval_metrics_values.json.
"""
from __future__ import annotations

import functools
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
RESIZE_TOL = 16 * 2.0 ** -24 * 255 * 1.375 ** 2
SSIM_TOL = 1e-5


def _dev(a, backend):
    return torch.from_numpy(np.ascontiguousarray(a)).to(backend.device)


def _record(backend, key, value):
    """profiles/eval_metrics_values.json[backend][key] = the worst value seen (the file is rewritten whole and moved into place)."""
    path = ROOT / "profiles" / "eval_metrics_values.json"
    try:
        values = json.loads(path.read_text()) if path.exists() else {}
    except ValueError:
        values = {}
    mine = values.setdefault(backend.name, {})
    mine[key] = max(float(value), float(mine.get(key, 0.0)))
    try:
        tmp = path.with_name(f"{path.name}.{os.getpid()}.tmp")
        tmp.write_text(json.dumps(values, indent=1, sort_keys=True) + "\n")
        os.replace(tmp, path)
    except OSError:
        pass                                                                   # a read-only checkout still runs the assertions


# ------------------------------------------------------------------------------------------------ resize: the yardstick
def _axis(n_in, n_out):
    """(indices [n_out, 4] clamped, coefficients fp32 [n_out, 4]) of one axis"""
    scale = 1.0 / (float(n_out) / float(n_in))
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    t = f - s
    assert t.dtype == np.float32
    A, one = np.float32(-0.75), np.float32(1)
    t1, t2 = t + one, one - t
    c0 = ((A * t1 - np.float32(5) * A) * t1 + np.float32(8) * A) * t1 - np.float32(4) * A
    c1 = ((A + np.float32(2)) * t - (A + np.float32(3))) * t * t + one
    c2 = ((A + np.float32(2)) * t2 - (A + np.float32(3))) * t2 * t2 + one
    c3 = one - c0 - c1 - c2
    c = np.stack([c0, c1, c2, c3], axis=1)
    assert c.dtype == np.float32
    idx = np.clip(s.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx, c


def resize64(src, Hd, Wd, divisor=None):
    """fp64 [Hd, Wd, 3]: the horizontal pass, then the vertical pass, products and sums in fp64"""
    a = np.asarray(src).astype(np.float32).astype(np.float64)
    ix, cx = _axis(a.shape[1], Wd)
    iy, cy = _axis(a.shape[0], Hd)
    h = sum(a[:, ix[:, k], :] * cx[:, k].astype(np.float64)[None, :, None] for k in range(4))
    v = sum(h[iy[:, k], :, :] * cy[:, k].astype(np.float64)[:, None, None] for k in range(4))
    return v if divisor is None else v / float(divisor)


def _source(Hs, Ws, kind, seed, dyadic=False):
    rng = np.random.default_rng(seed)
    if kind == "u8":
        a = rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
        a.reshape(-1)[:2] = (0, 255)
        return a
    if dyadic:
        return (rng.integers(0, 1021, (Hs, Ws, 3)) / 4.0).astype(np.float32)      # quarter steps: every product and sum of a 2 : 1 resize is exact
    return rng.uniform(0, 255, (Hs, Ws, 3)).astype(np.float32)


def _resize(backend, src, Hd, Wd, layout, divisor=None, **kw):
    from pcdms_amd import preprocess
    out = preprocess.resize_cv_cubic(_dev(src, backend), (Wd, Hd), divisor=divisor, layout=layout, **kw)
    return out


def _nhwc(t, layout):
    a = t.cpu().numpy()
    return a if layout == "nhwc" else a.transpose(0, 2, 3, 1)


RESIZE_CASES = [((64, 44), (32, 22), "2to1"), ((37, 29), (53, 41), "up"), ((50, 33), (17, 11), "down3"), ((9, 7), (30, 23), "edges"),
                ((20, 1), (20, 5), "one_column"), ((40, 30), (40, 30), "identity")]


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("src_hw,dst_hw,name", RESIZE_CASES, ids=[c[2] for c in RESIZE_CASES])
def test_resize_accuracy(backend, src_hw, dst_hw, name, kind, layout):
    src = _source(*src_hw, kind, seed=len(name), dyadic=name == "2to1")
    Hd, Wd = dst_hw
    want = resize64(src, Hd, Wd)
    got = _nhwc(_resize(backend, src, Hd, Wd, layout), layout)[0]
    assert got.dtype == np.float32 and got.shape == (Hd, Wd, 3)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(name, kind, layout, "max |device - fp64| =", err, "bound", RESIZE_TOL)
    _record(backend, "resize_abs_err_0_255", err)
    assert err <= RESIZE_TOL
    if name == "2to1":
        assert np.array_equal(got.astype(np.float64), want)                      # dyadic coefficients (t = 0.5): nothing rounds
    if name == "identity":
        assert np.array_equal(got, src.astype(np.float32))
    if name == "up" and kind == "u8":
        assert got.min() < 0 and got.max() > 255                               # not clipped: the cubic overshoots on noise
    got255 = _nhwc(_resize(backend, src, Hd, Wd, layout, divisor=255.0), layout)[0]
    err255 = float(np.abs(got255.astype(np.float64) - resize64(src, Hd, Wd, 255.0)).max())
    _record(backend, "resize_abs_err_0_1", err255)
    assert err255 <= RESIZE_TOL / 255
    assert np.array_equal(got255, got / np.float32(255.0))                     # a true fp32 division of the undivided result
    again = _nhwc(_resize(backend, src, Hd, Wd, layout), layout)[0]
    assert np.array_equal(again.view(np.int32), got.view(np.int32))            # reruns are bit-identical


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_resize_into_batch(backend, kind, layout):
    """33 x 47 -> 19 x 35 into index 2 of a batch of four: the other images keep their bytes"""
    from pcdms_amd import preprocess
    src = _source(33, 47, kind, seed=7)
    Hd, Wd = 19, 35
    shape = (4, Hd, Wd, 3) if layout == "nhwc" else (4, 3, Hd, Wd)
    sent = np.random.default_rng(8).integers(-2 ** 31, 2 ** 31 - 1, shape, dtype=np.int64).astype(np.int32)
    out = _dev(sent.copy(), backend).view(torch.float32)
    back = preprocess.resize_cv_cubic(_dev(src, backend), (Wd, Hd), layout=layout, out=out, index=2)
    backend.sync()
    assert back.data_ptr() == out.data_ptr()
    bits = out.view(torch.int32).cpu().numpy()
    for n in (0, 1, 3):
        assert np.array_equal(bits[n], sent[n])
    got = _nhwc(out, layout)[2]
    err = float(np.abs(got.astype(np.float64) - resize64(src, Hd, Wd)).max())
    _record(backend, "resize_abs_err_0_255", err)
    assert err <= RESIZE_TOL


def test_resize_refusals(backend):
    from pcdms_amd import ops, preprocess
    dev = backend.device
    src = _dev(_source(12, 10, "u8", 3), backend)
    dst = torch.full((2, 6, 5, 3), 7.0, device=dev)

    def refused(fn):
        with pytest.raises(RuntimeError, match="code -1"):
            fn()
        backend.sync()
        assert (dst.cpu() == 7.0).all()
    lib = ops._lib.lib()

    def raw(src_t, channels=3, Hs=12, Ws=10, N=2, Hd=6, Wd=5, index=0, ptr=None):
        return lambda: ops._chk(lib.pcdm_resize_cubic_f32(src_t.data_ptr(), 0, Hs, Ws, channels, dst.data_ptr() if ptr is None else ptr, N, Hd, Wd, index,
                                                          0, 0.0, ops._stream(dst)), "pcdm_resize_cubic_f32")
    refused(raw(src, channels=1))
    refused(raw(src, channels=4))
    refused(raw(src, Hs=0))
    refused(raw(src, Ws=-3))
    refused(raw(src, Hd=0))
    refused(raw(src, Wd=0))
    refused(raw(src, index=2))
    refused(raw(src, index=-1))
    refused(raw(src, N=0))
    refused(raw(src, ptr=dst.data_ptr() + 2))                                  # unaligned destination
    refused(lambda: ops.resize_cubic_f32(src, dst, 5, nchw=False))
    # the python surface
    with pytest.raises(ValueError, match="layout"):
        preprocess.resize_cv_cubic(src, (5, 6), layout="hwc")
    with pytest.raises(ValueError, match="index"):
        preprocess.resize_cv_cubic(src, (5, 6), out=dst, index=2)
    with pytest.raises(ValueError, match="out must be"):
        preprocess.resize_cv_cubic(src, (5, 7), out=dst)
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        preprocess.resize_cv_cubic(src[:, :, :1], (5, 6))
    with pytest.raises(ValueError, match="divisor"):
        preprocess.resize_cv_cubic(src, (5, 6), divisor=0.0)
    assert (dst.cpu() == 7.0).all()


# ------------------------------------------------------------------------------------------------ L1 / MAE
def absdiff64(cand, ref):
    """(l1, mae) per candidate: a - b and a + b in fp32 elementwise as numpy forms them, the sums in fp64"""
    l1, mae = [], []
    for n in range(cand.shape[0]):
        a, b = cand[n].astype(np.float32), ref[0 if ref.shape[0] == 1 else n].astype(np.float32)
        d, s = np.abs(a - b), a + b
        assert d.dtype == np.float32 and s.dtype == np.float32
        sd, ss = d.astype(np.float64).sum(), s.astype(np.float64).sum()
        l1.append(sd / d.size)
        with np.errstate(invalid="ignore", divide="ignore"):
            mae.append(np.float64(sd) / np.float64(ss))
    return np.array(l1), np.array(mae)


def _absdiff_check(backend, cand, ref, what, **kw):
    from pcdms_amd import metrics
    l1 = metrics.l1(_dev(cand, backend), _dev(ref, backend), **kw).cpu().numpy()
    mae = metrics.mae(_dev(cand, backend), _dev(ref, backend), **kw).cpu().numpy()
    assert l1.dtype == np.float32 and mae.dtype == np.float32 and l1.shape == mae.shape == (cand.shape[0],)
    return l1, mae


@pytest.mark.parametrize("H,W", [(48, 40), (17, 23)])
@pytest.mark.parametrize("ref_n", [1, 3])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_l1_mae(backend, H, W, ref_n, kind):
    rng = np.random.default_rng(H + ref_n)
    if kind == "u8":
        cand, ref = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8), rng.integers(0, 256, (ref_n, H, W, 3), dtype=np.uint8)
    else:
        ref = rng.uniform(-0.05, 1.05, (ref_n, H, W, 3)).astype(np.float32)
        cand = (ref[:1] + rng.normal(0, 0.1, (3, H, W, 3))).astype(np.float32)
    l1, mae = _absdiff_check(backend, cand, ref, f"{kind}_{H}x{W}_ref{ref_n}")
    w1, wm = absdiff64(cand, ref)
    print(kind, H, W, ref_n, "l1", l1, w1, "mae", mae, wm)
    if kind == "u8":
        assert np.array_equal(l1, w1.astype(np.float32)) and np.array_equal(mae, wm.astype(np.float32))
    else:
        e1, em = np.abs(l1 - w1) / np.abs(w1), np.abs(mae - wm) / np.abs(wm)
        _record(backend, "l1_rel_err_f32", e1.max())
        _record(backend, "mae_rel_err_f32", em.max())
        assert (e1 <= 1e-6).all() and (em <= 1e-6).all()
    again = _absdiff_check(backend, cand, ref, "rerun")
    assert np.array_equal(again[0].view(np.int32), l1.view(np.int32)) and np.array_equal(again[1].view(np.int32), mae.view(np.int32))


def test_l1_mae_window_and_special_values(backend):
    rng = np.random.default_rng(5)
    H, W = 17, 23
    ref = rng.uniform(0, 1, (1, H, W, 3)).astype(np.float32)
    canvas = rng.uniform(0, 1, (3, H + 4, 2 * W + 3, 3)).astype(np.float32)                # the candidates are windows of a wider canvas
    win = (W + 2, 3, W, H)
    crop = canvas[:, 3:3 + H, W + 2:2 * W + 2]
    l1, mae = _absdiff_check(backend, canvas, ref, "window", cand_window=win)
    w1, wm = absdiff64(crop, ref)
    assert (np.abs(l1 - w1) <= 1e-6 * w1).all() and (np.abs(mae - wm) <= 1e-6 * wm).all()
    same = _absdiff_check(backend, crop.copy(), ref, "crop")
    assert np.array_equal(same[0], l1) and np.array_equal(same[1], mae)
    for imgs in (ref, rng.integers(1, 256, (2, H, W, 3), dtype=np.uint8)):                 # identical images
        l1, mae = _absdiff_check(backend, imgs, imgs, "identical")
        assert (l1 == 0).all() and (mae == 0).all()
    for zeros in (np.zeros((2, H, W, 3), np.float32), np.zeros((2, H, W, 3), np.uint8)):   # 0 / 0, as numpy divides
        l1, mae = _absdiff_check(backend, zeros, zeros, "zeros")
        assert (l1 == 0).all() and np.isnan(mae).all()
    neg = np.full((1, H, W, 3), -1.0, np.float32)                                          # x / 0: inf
    l1, mae = _absdiff_check(backend, neg, -neg, "inf")
    assert l1[0] == 2.0 and np.isposinf(mae[0])


def test_absdiff_refusals(backend):
    from pcdms_amd import ops
    N, H, W = 2, 9, 8
    cand, ref = torch.zeros((N, H, W, 3), dtype=torch.uint8, device=backend.device), torch.zeros((1, H, W, 3), dtype=torch.uint8, device=backend.device)
    out = torch.full((N,), 7.0, device=backend.device)
    ws = torch.empty(ops.metrics_ws_bytes(N, 1, W, H, 0.0) // 8, dtype=torch.float64, device=backend.device)
    win = (0, 0, W, H)
    for fn in (lambda: ops.absdiff(cand, ref, (1, 0, W, H), win, out, None, ws),                     # the window leaves the image
               lambda: ops.absdiff(cand, ref, (0, 0, W - 1, H), win, out, None, ws),                 # windows of different sizes
               lambda: ops.absdiff(cand, ref, win, win, None, None, ws),                             # no output
               lambda: ops.absdiff(cand, ref, win, win, out, None, ws[:1]),                          # workspace too small
               lambda: ops.absdiff(cand, torch.zeros((3, H, W, 3), dtype=torch.uint8, device=backend.device), win, win, out, None, ws),
               lambda: ops.absdiff(cand[..., :2].contiguous(), ref[..., :2].contiguous(), win, win, out, None, ws)):
        with pytest.raises(RuntimeError, match="code -1"):
            fn()
    backend.sync()
    assert (out.cpu() == 7.0).all()


# ------------------------------------------------------------------------------------------------ box SSIM
def _usum(a, w, axis):
    v = np.lib.stride_tricks.sliding_window_view(a, w, axis=axis)
    return v.sum(axis=-1)


def _umean(a, w):
    """the w x w mean filter of a [H, W] array at the pixels whose window lies inside it: [H - w + 1, W - w + 1]"""
    return _usum(_usum(a, w, 1), w, 0) / float(w * w)


def box_ssim64(ref, cand, w, data_range=None, sample=True):
    a, b = np.asarray(ref, dtype=np.float64), np.asarray(cand, dtype=np.float64)
    R = float(b.max() - b.min()) if data_range is None else float(data_range)
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    NP = w * w
    cn = NP / (NP - 1.0) if sample else 1.0
    vals = []
    for ch in range(3):
        x, y = a[..., ch], b[..., ch]
        ux, uy = _umean(x, w), _umean(y, w)
        vx, vy, vxy = cn * (_umean(x * x, w) - ux * ux), cn * (_umean(y * y, w) - uy * uy), cn * (_umean(x * y, w) - ux * uy)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        vals.append(s.mean())
    return float(np.mean(vals))


def box_ssim64_batch(ref, cand, w, **kw):
    return np.array([box_ssim64(ref[0 if ref.shape[0] == 1 else n], cand[n], w, **kw) for n in range(cand.shape[0])])


def test_box_yardstick_matches_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    z = np.random.default_rng(0).uniform(0, 1, (60, 56))
    for w in (7, 51):
        p = (w - 1) // 2
        assert np.abs(_umean(z, w) - ndi.uniform_filter(z, size=w)[p:60 - p, p:56 - p]).max() <= 1e-12


def _smooth(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([127.5 + 100 * np.sin(x / 5.0 + ph) * np.cos(y / 7.0 + 2 * ph) for ph in (0.0, 0.7, 1.9)], axis=-1)


def _u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _box_case(name, H, W):
    """(ref [1 | N, H, W, 3], cand [N, H, W, 3], data_range or None)"""
    rng = np.random.default_rng(sum(map(ord, name)) + H)
    if name == "noise":
        return rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8), rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8), 255.0
    if name == "smooth_noise":
        base = _smooth(H, W)
        return _u8(base)[None], np.stack([_u8(base + rng.normal(0, s, base.shape)) for s in (5, 40)]), None
    if name == "identical":
        img = _u8(_smooth(H, W) + rng.normal(0, 10, (H, W, 3)))
        return img[None], np.stack([img, img]), 255.0
    if name == "near_constant":
        ref = (0.7 + 1e-4 * rng.standard_normal((2, H, W, 3))).astype(np.float32)
        return ref, (ref + 1e-4 * rng.standard_normal((2, H, W, 3))).astype(np.float32), 1.0
    if name == "unit_f32":                                                     # the evaluation's images: fp32 around [0, 1] with overshoot, data range 1
        ref = (_smooth(H, W) / 255.0 + rng.normal(0, 0.02, (H, W, 3))).astype(np.float32)
        return ref[None], np.stack([(ref + rng.normal(0, s, ref.shape)).astype(np.float32) for s in (0.02, 0.2)]), 1.0
    if name == "unit_f32_auto":
        ref, cand, _ = _box_case("unit_f32", H, W)
        return ref, cand, None
    raise KeyError(name)


BOX_CASES = [("noise", 7, 48, 40), ("smooth_noise", 7, 48, 40), ("identical", 7, 48, 40), ("near_constant", 7, 48, 40), ("unit_f32", 7, 48, 40),
             ("unit_f32_auto", 7, 48, 40), ("smooth_noise", 3, 17, 23), ("noise", 51, 60, 56), ("smooth_noise", 51, 60, 56), ("unit_f32", 51, 60, 56),
             ("identical", 51, 51, 51), ("smooth_noise", 51, 51, 51), ("unit_f32_auto", 51, 51, 51)]


@pytest.mark.parametrize("name,w,H,W", BOX_CASES)
def test_box_ssim_accuracy(backend, name, w, H, W):
    from pcdms_amd import metrics
    ref, cand, R = _box_case(name, H, W)
    want = box_ssim64_batch(ref, cand, w, data_range=R)
    got = metrics.ssim_box(_dev(cand, backend), _dev(ref, backend), win_size=w, data_range=R).cpu().numpy()
    err = np.abs(got.astype(np.float64) - want)
    print(name, w, H, W, "got", got, "want", want, "err", err)
    _record(backend, "ssim_box_abs_err", err.max())
    assert got.dtype == np.float32 and (err <= SSIM_TOL).all()
    if name == "identical":
        assert (got == 1.0).all()
    again = metrics.ssim_box(_dev(cand, backend), _dev(ref, backend), win_size=w, data_range=R).cpu().numpy()
    assert np.array_equal(again.view(np.int32), got.view(np.int32))


def test_box_ssim_tells_sample_from_population(backend):
    """dropping NP / (NP - 1) misses the bound on the w = 7 noise case"""
    from pcdms_amd import metrics
    ref, cand, R = _box_case("noise", 48, 40)
    sample, population = box_ssim64_batch(ref, cand, 7, data_range=R), box_ssim64_batch(ref, cand, 7, data_range=R, sample=False)
    assert (np.abs(sample - population) > 10 * SSIM_TOL).all(), (sample, population)
    got = metrics.ssim_box(_dev(cand, backend), _dev(ref, backend), win_size=7, data_range=R).cpu().numpy().astype(np.float64)
    assert (np.abs(got - sample) <= SSIM_TOL).all() and (np.abs(got - population) > SSIM_TOL).all()


def test_box_ssim_window_and_refusals(backend):
    from pcdms_amd import metrics, ops
    ref, cand, _ = _box_case("smooth_noise", 48, 40)
    canvas = np.random.default_rng(1).integers(0, 256, (2, 50, 90, 3), dtype=np.uint8)
    canvas[:, 1:49, 45:85] = cand
    a = metrics.ssim_box(_dev(canvas, backend), _dev(ref, backend), win_size=7, cand_window=(45, 1, 40, 48))
    b = metrics.ssim_box(_dev(cand, backend), _dev(ref, backend), win_size=7)
    assert torch.equal(a, b)
    for w in (1, 2, 8, 53, 41):                                                # below 3, even, above 51, wider than the image
        assert ops.ssim_box_ws_bytes(2, 1, 40, 48, w) == -1
        with pytest.raises(RuntimeError, match="code -1"):
            metrics.ssim_box(_dev(cand, backend), _dev(ref, backend), win_size=w)
    assert ops.ssim_box_ws_bytes(2, 1, 40, 48, 39) > 0
    scores = torch.full((2,), 7.0, device=backend.device)
    ws = torch.empty(ops.ssim_box_ws_bytes(2, 1, 40, 48, 7) // 8 - 1, dtype=torch.float64, device=backend.device)
    with pytest.raises(RuntimeError, match="code -1"):
        ops.ssim_box(_dev(cand, backend), _dev(ref, backend), (0, 0, 40, 48), (0, 0, 40, 48), scores, ws, win_size=7)
    backend.sync()
    assert (scores.cpu() == 7.0).all()


# ------------------------------------------------------------------------------------------------ the driver
def _psnr64(cand, ref):
    return 10 * np.log10(1.0 / ((cand.astype(np.float64) - ref.astype(np.float64)) ** 2).reshape(cand.shape[0], -1).mean(1))


def _tree(tmp_path, n=6, H=40, W=30):
    from PIL import Image
    rng = np.random.default_rng(17)
    gen_dir, gt_dir, real_dir = tmp_path / "gen", tmp_path / "gt", tmp_path / "real"
    for d in (gen_dir, gt_dir, real_dir):
        d.mkdir()
    gens, gts = [], []
    for i in range(n):
        base = _smooth(H, W) * (0.6 + 0.07 * i)
        gt, gen = _u8(base + rng.normal(0, 4, base.shape)), _u8(base + rng.normal(0, 6 + 9 * i, base.shape))
        Image.fromarray(gt).save(gt_dir / f"t{i}.png")
        Image.fromarray(gen).save(gen_dir / f"xs{n - i}_to_t{i}.png")             # sorted by the SOURCE name: the reverse of the targets' order
        Image.fromarray(_u8(base + rng.normal(0, 25, base.shape))).save(real_dir / f"r{i}.png")
        gens.append(gen)
        gts.append(gt)
    Image.fromarray(gens[0]).save(gen_dir / "xs9_to_missing.png")                # no ground truth: reported and skipped
    order = list(range(n - 1, -1, -1))
    return gen_dir, gt_dir, real_dir, [gens[i] for i in order], [gts[i] for i in order], [f"xs{n - i}_to_t{i}.png" for i in order]


def test_calculate_metrics_tool(backend, tmp_path, capsys):
    """40 x 30 files, --size 24 36, uniform window 7 through the test keyword (51 cannot fit); FID at dims 64 without the 299 x 299 resize, so the lane
    emulator can run it.  LPIPS needs 31 pixels per side (pcdm_lpips), so its part runs at --size 32 36."""
    from pcdms_amd import metrics, preprocess
    from tests import test_fid, test_lpips, test_metrics
    from tools import calculate_metrics as cm
    gen_dir, gt_dir, real_dir, gens, gts, names = _tree(tmp_path)
    torch.save(dict(test_fid._state_dict()), tmp_path / "inception.pth")
    torch.save(dict(test_lpips._state_dict()), tmp_path / "lpips.pth")
    W, H = 24, 36
    fid_args = ["--real", str(real_dir), "--fid-weights", str(tmp_path / "inception.pth"), "--fid-dims", "64", "--fid-no-resize"]
    common = [str(gen_dir), str(gt_dir), "--size", str(W), str(H)]
    res = cm.main(common + fid_args + ["--save-dir", str(tmp_path), "--batch", "4"], device=backend.device, win_size=7)
    text = capsys.readouterr().out
    # pairing
    assert [os.path.basename(f) for f in res["skipped"]] == ["xs9_to_missing.png"] and "xs9_to_missing.png" in text and "lpips" not in res
    assert list(res["names"]) == names
    # every array of the .npz: each stage against its own yardstick -- the resized images against the resize yardstick, the metrics of THOSE images
    # against the metric yardsticks
    with np.load(tmp_path / f"{W}_{H}_metrics.npz") as f:
        saved = {k: f[k] for k in f.files}
    assert sorted(saved) == sorted(["psnr", "ssim", "ssim_256", "mae", "l1", "names"]) and list(saved["names"]) == names
    pred = np.stack([preprocess.resize_cv_cubic(_dev(g, backend), (W, H), divisor=255.0).cpu().numpy()[0] for g in gens])
    gt = np.stack([preprocess.resize_cv_cubic(_dev(g, backend), (W, H), divisor=255.0).cpu().numpy()[0] for g in gts])
    for dev_imgs, files in ((pred, gens), (gt, gts)):
        for a, src in zip(dev_imgs, files):
            assert np.abs(a.astype(np.float64) - resize64(src, H, W, 255.0)).max() <= RESIZE_TOL / 255
    for k in ("psnr", "ssim", "ssim_256", "mae", "l1"):
        assert np.array_equal(saved[k], res[k]) and saved[k].shape == (6,)
    want_psnr = _psnr64(pred, gt)
    assert (np.abs(saved["psnr"] - want_psnr) <= 1e-5 * np.abs(want_psnr)).all()
    assert (np.abs(saved["ssim"] - box_ssim64_batch(gt, pred, 7, data_range=1.0)) <= SSIM_TOL).all()
    p255, g255 = pred * np.float32(255.0), gt * np.float32(255.0)
    assert (np.abs(saved["ssim_256"] - test_metrics.ssim64_batch(g255, p255, sigma=1.2)) <= SSIM_TOL).all()
    w1, wm = absdiff64(pred, gt)
    assert (np.abs(saved["l1"] - w1) <= 1e-6 * w1).all() and (np.abs(saved["mae"] - wm) <= 1e-6 * wm).all()
    assert "PSNR: %.4f PSNR Variance: %.4f SSIM_256: %.4f" % (round(float(np.mean(res["psnr"])), 4), round(float(np.var(res["psnr"])), 4),
                                                             round(float(np.mean(res["ssim_256"])), 4)) in text
    assert "MAE: %.4f MAE Variance: %.4f l1: %.4f l1 Variance: %.4f" % (round(float(np.mean(res["mae"])), 4), round(float(np.var(res["mae"])), 4),
                                                                       round(float(np.mean(res["l1"])), 4), round(float(np.var(res["l1"])), 4)) in text
    # FID: all seven generated files against the real set; the statistics cache is written once ...
    cache = real_dir / f"{W}_{H}_statistics.npz"
    assert cache.exists() and "FID: %.4f" % res["fid"] in text and np.isfinite(res["fid"])
    model = metrics.InceptionV3Features(64, resize_input=False).load_state_dict(test_fid._state_dict())
    fid = metrics.FID(model)

    def nchw(files):
        return torch.cat([preprocess.resize_cv_cubic(_dev(g, backend), (W, H), divisor=255.0, layout="nchw") for g in files])
    from PIL import Image
    reals = [np.array(Image.open(f).convert("RGB")) for f in cm.image_files(real_dir)]
    gen_all = [np.array(Image.open(f).convert("RGB")) for f in cm.image_files(gen_dir)]
    assert len(gen_all) == 7
    assert res["fid"] == fid(fid.statistics([nchw(gen_all)]), fid.statistics([nchw(reals)]))
    # ... and then read: with other statistics in the file the FID is theirs, and the file stays as it is
    other = fid.statistics([nchw(reals[:4])])
    other.save(cache)
    stamp = cache.read_bytes()
    res2 = cm.main(common + fid_args, device=backend.device, win_size=7)
    capsys.readouterr()
    assert res2["fid"] == fid(fid.statistics([nchw(gen_all)]), other) and res2["fid"] != res["fid"] and cache.read_bytes() == stamp
    # --reference-remainders: 7 // 4 = one full FID batch of the generated files, 6 // 4 = one of the real ones
    cache.unlink()
    res3 = cm.main(common + fid_args + ["--fid-batch", "4", "--reference-remainders"], device=backend.device, win_size=7)
    capsys.readouterr()
    assert res3["fid"] == fid(fid.statistics([nchw(gen_all[:4])]), other)
    for k in ("psnr", "ssim", "ssim_256", "mae", "l1"):
        assert np.array_equal(res3[k], res[k])                                 # the per-pair metrics count every pair either way
    # LPIPS (31 pixels per side at least): every pair, then 6 // 4 = one full batch
    W2 = 32
    lp_args = [str(gen_dir), str(gt_dir), "--size", str(W2), str(H), "--lpips-weights", str(tmp_path / "lpips.pth"), "--lpips-batch", "4"]
    lp_all = cm.main(lp_args, device=backend.device, win_size=7)
    text = capsys.readouterr().out
    lp_ref = cm.main(lp_args + ["--reference-remainders"], device=backend.device, win_size=7)
    capsys.readouterr()
    m = metrics.LPIPS().load_state_dict(test_lpips._state_dict())

    def nchw2(files):
        return torch.cat([preprocess.resize_cv_cubic(_dev(g, backend), (W2, H), divisor=255.0, layout="nchw") for g in files])
    want = m(nchw2(gens), nchw2(gts))[:, 0, 0, 0].cpu().numpy()
    assert np.array_equal(lp_all["lpips"], want) and np.array_equal(lp_ref["lpips"], want[:4]) and "fid" not in lp_all
    assert "lpips: %.3f" % float(np.mean(want)) in text
    x0, x1 = nchw2(gens).cpu().double(), nchw2(gts).cpu().double()
    assert (np.abs(want - test_lpips._net(x0, x1)[0]) <= test_lpips.TOL).all()


# ------------------------------------------------------------------------------------------------ full size, graph capture
@pytest.mark.gpu
@pytest.mark.parametrize("Hd,Wd", [(256, 176), (512, 352)])
def test_full_size(gpu_backend, Hd, Wd):
    """1101 x 750 uint8 -> the two evaluation sizes, N = 4: resize, l1 / mae and ssim_box(51) against the yardsticks, and a graph-captured rerun of
    the whole chain bit-identical to the eager one"""
    from pcdms_amd import metrics, preprocess
    dev = gpu_backend.device
    rng = np.random.default_rng(Hd)
    N, Hs, Ws = 4, 1101, 750
    base = np.stack([127.5 + 100 * np.sin(np.mgrid[0:Hs, 0:Ws][1] / 37.0 + ph) * np.cos(np.mgrid[0:Hs, 0:Ws][0] / 53.0 + 2 * ph) for ph in (0.0, 0.7, 1.9)], -1)
    gt_u8 = _u8(base + rng.normal(0, 8, base.shape))
    gens_u8 = [_u8(base + rng.normal(0, s, base.shape)) for s in (4, 12, 30, 60)]
    gt_d, gens_d = torch.from_numpy(gt_u8).to(dev), [torch.from_numpy(g).to(dev) for g in gens_u8]
    pred, gt = torch.empty((N, Hd, Wd, 3), device=dev), torch.empty((1, Hd, Wd, 3), device=dev)

    def chain():
        for i, g in enumerate(gens_d):
            preprocess.resize_cv_cubic(g, (Wd, Hd), divisor=255.0, out=pred, index=i)
        preprocess.resize_cv_cubic(gt_d, (Wd, Hd), divisor=255.0, out=gt)
        return metrics.l1(pred, gt), metrics.mae(pred, gt), metrics.ssim_box(pred, gt, win_size=51, data_range=1.0)
    eager = [t.clone() for t in chain()]
    eager_pred = pred.clone()
    p, g = pred.cpu().numpy(), gt.cpu().numpy()
    err = max(float(np.abs(p[i].astype(np.float64) - resize64(gens_u8[i], Hd, Wd, 255.0)).max()) for i in range(N))
    err = max(err, float(np.abs(g[0].astype(np.float64) - resize64(gt_u8, Hd, Wd, 255.0)).max()))
    print("resize", Hd, Wd, "max |device - fp64| =", err, "bound", RESIZE_TOL / 255)
    _record(gpu_backend, f"full_size_resize_abs_err_0_1_{Hd}x{Wd}", err)
    assert err <= RESIZE_TOL / 255
    assert p.min() < 0 and p.max() > 1                                         # noise on a saturating pattern: the cubic overshoots, nothing clips
    w1, wm = absdiff64(p, g)
    l1, mae, ss = (t.cpu().numpy().astype(np.float64) for t in eager)
    want = box_ssim64_batch(g, p, 51, data_range=1.0)
    print("l1", l1, w1, "mae", mae, wm, "ssim_box", ss, want)
    _record(gpu_backend, f"full_size_ssim_box_abs_err_{Hd}x{Wd}", np.abs(ss - want).max())
    assert (np.abs(l1 - w1) <= 1e-6 * w1).all() and (np.abs(mae - wm) <= 1e-6 * wm).all() and (np.abs(ss - want) <= SSIM_TOL).all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    pred.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain()
    pred.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(pred.view(torch.int32), eager_pred.view(torch.int32))
    for a, b in zip(outs, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
