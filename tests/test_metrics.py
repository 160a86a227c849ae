"""Device-side SSIM / PSNR and the best-of-N pick (pcdms_amd/metrics.py, csrc/image_metrics.hip: pcdm_ssim / pcdm_psnr / pcdm_select_image).

The yardstick is an fp64 restatement, written here with numpy only, of
``skimage.metrics.structural_similarity(ref, cand, gaussian_weights=True, sigma=s, use_sample_covariance=False, channel_axis=2, data_range=R)``:
radius ``int(3.5 s + 0.5)``, taps ``exp(-(i / s)^2 / 2)`` normalised to 1, scipy's ``reflect`` boundary (``np.pad(mode="symmetric")``), five
filtered moments per channel, population covariances, the map averaged over ``[r, H - r) x [r, W - r)`` and then over the channels.  Where scipy
imports, ``test_yardstick_matches_scipy`` checks the restatement's filter against ``scipy.ndimage.gaussian_filter`` to 1e-12.

Tolerance: ``|device - fp64| <= 1e-5`` absolute.  A numpy fp32 model of the centred formulation was at most 9.9e-7 off the fp64 restatement over
these case families; the bound is ten times that, and the plain fp32 ``E[x^2] - mu^2`` form misses it by a factor of 600 on the near-constant
case, so the bound tells the two apart.  The kernels accumulate in fp64 on centred values and sit well inside it.

Kernel tests take the ``backend`` fixture: each runs under the lane emulator (sides <= 48) in the CPU suite and on the MI355X under ``-m gpu``.
"""
from __future__ import annotations

import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

TOL = 1e-5


# ------------------------------------------------------------------------------------------------ the fp64 yardstick
def _taps(sigma):
    r = int(3.5 * sigma + 0.5)
    i = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 * (i / sigma) ** 2)
    return w / w.sum(), r


def _gfilt(z, sigma):
    w, r = _taps(sigma)
    H, W = z.shape
    p = np.pad(z, r, mode="symmetric")
    t = sum(w[k] * p[:, k:k + W] for k in range(2 * r + 1))
    return sum(w[k] * t[k:k + H, :] for k in range(2 * r + 1))


def ssim64(ref, cand, sigma=1.2, data_range=None):
    a, b = np.asarray(ref, dtype=np.float64), np.asarray(cand, dtype=np.float64)
    R = float(b.max() - b.min()) if data_range is None else float(data_range)
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    r = _taps(sigma)[1]
    vals = []
    for ch in range(3):
        x, y = a[..., ch], b[..., ch]
        ux, uy = _gfilt(x, sigma), _gfilt(y, sigma)
        vx, vy, vxy = _gfilt(x * x, sigma) - ux * ux, _gfilt(y * y, sigma) - uy * uy, _gfilt(x * y, sigma) - ux * uy
        with np.errstate(invalid="ignore", divide="ignore"):
            s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        vals.append(s[r:s.shape[0] - r, r:s.shape[1] - r].mean())
    return float(np.mean(vals))


def ssim64_batch(ref, cand, **kw):
    return np.array([ssim64(ref[0 if ref.shape[0] == 1 else n], cand[n], **kw) for n in range(cand.shape[0])])


def test_yardstick_matches_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    z = rng.uniform(0, 1, (37, 29))
    for sigma in (1.2, 1.5):
        assert np.abs(_gfilt(z, sigma) - ndi.gaussian_filter(z, sigma, truncate=3.5, mode="reflect")).max() <= 1e-12
    # ... and the whole formula against the drivers' host scorer (which filters with scipy)
    drv = _load_driver("stage2_batchtest_inpaint_model")
    a, b = rng.integers(0, 256, (40, 30, 3)), rng.integers(0, 256, (40, 30, 3))
    assert abs(ssim64(a, b) - drv.ssim_gaussian(a.astype(np.float64), b.astype(np.float64))) <= 1e-12


# ------------------------------------------------------------------------------------------------ cases
def _smooth(H, W, rng):
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([127.5 + 100 * np.sin(x / 5.0 + ph) * np.cos(y / 7.0 + 2 * ph) for ph in (0.0, 0.7, 1.9)], axis=-1)
    return img


def _u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def _case(name, H=48, W=40):
    """-> (ref [1 | N, H, W, 3], cand [N, H, W, 3], kwargs of ssim)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    kw = {}
    if name == "noise":
        ref, cand = rng.integers(0, 256, (1, H, W, 3)), rng.integers(0, 256, (3, H, W, 3))
    elif name == "smooth_noise5_40":
        base = _smooth(H, W, rng)
        ref = _u8(base)[None]
        cand = np.stack([_u8(base + rng.normal(0, 5, base.shape)), _u8(base + rng.normal(0, 40, base.shape))])
    elif name == "identical":
        ref = rng.integers(0, 256, (2, H, W, 3))
        cand = ref.copy()
    elif name == "near_constant":
        ref = np.full((1, H, W, 3), 200)
        cand = np.full((2, H, W, 3), 200)
        n = max(3, int(round(0.001 * cand[0].size)))
        for i in range(2):
            cand[i].reshape(-1)[rng.choice(cand[i].size, n, replace=False)] += 3
    elif name == "dark_vs_bright":
        ref = 20 + rng.integers(-5, 6, (1, H, W, 3))
        cand = 200 + rng.integers(-5, 6, (2, H, W, 3))
    elif name == "tiny_range":
        ref, cand = rng.integers(0, 6, (2, H, W, 3)), rng.integers(0, 6, (2, H, W, 3))
    elif name == "size_33x21":
        ref, cand = rng.integers(0, 256, (1, 33, 21, 3)), rng.integers(0, 256, (2, 33, 21, 3))
    elif name == "min_size_9x9":
        ref, cand = rng.integers(0, 256, (1, 9, 9, 3)), rng.integers(0, 256, (2, 9, 9, 3))
    elif name == "sigma_1.5":
        base = _smooth(H, W, rng)
        ref, cand = _u8(base)[None], _u8(base + rng.normal(0, 20, (2,) + base.shape))
        kw["sigma"] = 1.5
    elif name == "data_range":
        base = _smooth(H, W, rng)
        ref, cand = _u8(base)[None], _u8(base + rng.normal(0, 20, (2,) + base.shape))
        kw["data_range"] = 255.0
    elif name == "fp32_unit":
        base = _smooth(H, W, rng) / 255.0
        ref = base[None].astype(np.float32)
        cand = np.clip(base + rng.normal(0, 0.05, (2,) + base.shape), 0, 1).astype(np.float32)
        return ref, cand, kw
    else:
        raise KeyError(name)
    return ref.astype(np.uint8), cand.astype(np.uint8), kw


CASES = ["noise", "smooth_noise5_40", "identical", "near_constant", "dark_vs_bright", "tiny_range", "size_33x21", "min_size_9x9", "sigma_1.5",
         "data_range", "fp32_unit"]


def _dev(a, backend):
    return torch.from_numpy(np.ascontiguousarray(a)).to(backend.device)


def _check(backend, ref, cand, kw, what):
    from pcdms_amd import metrics
    got = metrics.ssim(_dev(cand, backend), _dev(ref, backend), **kw)
    backend.sync()
    assert got.dtype == torch.float32 and got.shape == (cand.shape[0],) and got.device.type == backend.device.type
    got = got.cpu().numpy().astype(np.float64)
    want = ssim64_batch(ref, cand, **kw)
    err = np.abs(got - want)
    print(f"{what}: device {got} fp64 {want} |err| max {err.max():.3e}")
    assert np.isfinite(want).all() and (err <= TOL).all(), (what, got, want, err)
    return got, want


@pytest.mark.parametrize("name", CASES)
def test_ssim_accuracy(backend, name):
    ref, cand, kw = _case(name)
    got, want = _check(backend, ref, cand, kw, name)
    if name == "identical":
        assert (np.abs(got - 1.0) <= TOL).all()
    if name == "near_constant":   # the case the plain fp32 E[x^2] - mu^2 form misses: the scores must still be real, not saturated
        assert (want < 1.0 - 100 * TOL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,N,per_cand", [(512, 352, 4, False), (512, 352, 8, True), (512, 512, 4, True), (512, 512, 8, False)])
def test_ssim_accuracy_full_size(gpu_backend, H, W, N, per_cand):
    rng = np.random.default_rng(H + W + N)
    base = _smooth(H, W, rng)
    ref = np.stack([_u8(base + 3 * i) for i in range(N if per_cand else 1)])
    cand = np.stack([_u8(base + rng.normal(0, 6 + 5 * i, base.shape)) for i in range(N)])
    _check(gpu_backend, ref, cand, {}, f"{H}x{W} N={N} per_cand={per_cand}")


def test_ssim_window_equals_crop(backend):
    """A window at an offset inside a wider canvas scores bit for bit like the cropped copy: no pixel outside the window enters."""
    from pcdms_amd import metrics
    rng = np.random.default_rng(5)
    H, W, N = 40, 36, 3
    cand, ref = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8), rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    canvas = np.empty((N, H + 9, 2 * W + 5, 3), dtype=np.uint8)
    canvas[:] = (np.arange(canvas.size, dtype=np.int64).reshape(canvas.shape) * 37 % 251).astype(np.uint8)      # sentinel pattern
    cx, cy = W + 2, 6
    canvas[:, cy:cy + H, cx:cx + W] = cand
    rcanvas = np.full((1, H + 3, W + 4, 3), 255, dtype=np.uint8)
    rcanvas[:, 1:1 + H, 3:3 + W] = ref
    a = metrics.ssim(_dev(cand, backend), _dev(ref, backend))
    b = metrics.ssim(_dev(canvas, backend), _dev(rcanvas, backend), cand_window=(cx, cy, W, H), ref_window=(3, 1, W, H))
    backend.sync()
    assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32)), (a, b)
    assert (np.abs(a.cpu().numpy() - ssim64_batch(ref, cand)) <= TOL).all()
    pa = metrics.psnr(_dev(cand, backend), _dev(ref, backend))
    pb = metrics.psnr(_dev(canvas, backend), _dev(rcanvas, backend), cand_window=(cx, cy, W, H), ref_window=(3, 1, W, H))
    assert torch.equal(pa.cpu().view(torch.int32), pb.cpu().view(torch.int32))


def test_ssim_tolerance_bites(backend):
    """One channel of one candidate replaced: its score must move by more than the tolerance (a test that cannot fail guards nothing)."""
    from pcdms_amd import metrics
    ref, cand, _ = _case("smooth_noise5_40")
    other = cand.copy()
    other[0, ..., 1] = np.random.default_rng(9).integers(0, 256, other.shape[1:3])
    a = metrics.ssim(_dev(cand, backend), _dev(ref, backend)).cpu().numpy()
    b = metrics.ssim(_dev(other, backend), _dev(ref, backend)).cpu().numpy()
    assert abs(float(a[0]) - float(b[0])) > 100 * TOL
    assert abs(float(b[0]) - ssim64(ref[0], other[0])) <= TOL
    assert abs(float(a[0]) - ssim64(ref[0], other[0])) > TOL            # the old score does not pass for the new image


# ------------------------------------------------------------------------------------------------ PSNR / MSE
def test_psnr_and_mse(backend):
    from pcdms_amd import metrics
    rng = np.random.default_rng(11)
    H, W = 37, 29
    ref = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    cand = np.stack([_u8(ref[0] + rng.normal(0, s, ref[0].shape)) for s in (2, 20, 90)] + [ref[0]])
    sse = ((cand.astype(np.int64) - ref.astype(np.int64)) ** 2).reshape(4, -1).sum(1)            # the integer reference
    mse = metrics.mse(_dev(cand, backend), _dev(ref, backend)).cpu().numpy()
    assert mse.dtype == np.float32 and np.array_equal(mse, (sse / (H * W * 3)).astype(np.float32)), (mse, sse / (H * W * 3))
    got = metrics.psnr(_dev(cand, backend), _dev(ref, backend)).cpu().numpy().astype(np.float64)
    want = 10 * np.log10(255.0 ** 2 / (sse[:3] / (H * W * 3)))
    print("psnr", got, want)
    assert (np.abs(got[:3] - want) <= 1e-5 * np.abs(want)).all() and np.isposinf(got[3])
    # per-candidate references, fp32 images, another data range
    reff = rng.uniform(0, 1, (2, H, W, 3)).astype(np.float32)
    candf = np.clip(reff + rng.normal(0, 0.1, reff.shape), 0, 1).astype(np.float32)
    got = metrics.psnr(_dev(candf, backend), _dev(reff, backend), data_range=1.0).cpu().numpy().astype(np.float64)
    want = 10 * np.log10(1.0 / ((candf.astype(np.float64) - reff.astype(np.float64)) ** 2).reshape(2, -1).mean(1))
    assert (np.abs(got - want) <= 1e-5 * np.abs(want)).all(), (got, want)


# ------------------------------------------------------------------------------------------------ determinism, containment
SENT = 0xA5


def _guarded(nbytes, backend, dtype, pad=64):
    """A tensor of ``nbytes`` that is a window of a sentinel-filled buffer: (whole buffer as uint8, the window viewed as dtype)."""
    whole = torch.full((nbytes + 2 * pad,), SENT, dtype=torch.uint8, device=backend.device)
    return whole, whole[pad:pad + nbytes].view(dtype)


def _outside_untouched(whole, nbytes, pad=64):
    w = whole.cpu()
    return bool((w[:pad] == SENT).all() and (w[pad + nbytes:] == SENT).all())


def test_determinism_and_containment(backend):
    from pcdms_amd import ops
    rng = np.random.default_rng(13)
    N, H, W = 5, 45, 38
    cand, ref = _dev(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8), backend), _dev(rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8), backend)
    win = (0, 0, W, H)
    nws = ops.metrics_ws_bytes(N, 1, W, H, 1.2)
    assert nws > 0 and nws % 8 == 0
    runs = []
    for _ in range(2):
        ws_all, ws = _guarded(nws, backend, torch.uint8)
        sc_all, sc = _guarded(4 * N, backend, torch.float32)
        ix_all, ix = _guarded(4, backend, torch.int32)
        ops.ssim(cand, ref, win, win, sc, ix, ws)
        im_all, im = _guarded(H * W * 3, backend, torch.uint8)
        ops.select_image(cand, win, ix, im.view(H, W, 3), False)
        nm_all, nm = _guarded(4 * H * W * 3, backend, torch.float32)
        ops.select_image(cand, win, ix, nm.view(1, 3, H, W), True)
        ms_all, ms = _guarded(4 * N, backend, torch.float32)
        ps_all, ps = _guarded(4 * N, backend, torch.float32)
        ws2_all, ws2 = _guarded(ops.metrics_ws_bytes(N, 1, W, H, 0.0), backend, torch.uint8)
        ops.psnr(cand, ref, win, win, ms, ps, ws2)
        backend.sync()
        for whole, n in ((ws_all, nws), (sc_all, 4 * N), (ix_all, 4), (im_all, H * W * 3), (nm_all, 4 * H * W * 3), (ms_all, 4 * N), (ps_all, 4 * N),
                         (ws2_all, ws2.numel())):
            assert _outside_untouched(whole, n)
        runs.append([t.cpu().clone() for t in (sc.view(torch.int32), ix, im, nm.view(torch.int32), ms.view(torch.int32), ps.view(torch.int32))])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # a workspace one byte-word short of the query is refused
    ws_all, ws = _guarded(nws - 8, backend, torch.uint8)
    sc = torch.full((N,), 7.0, device=backend.device)
    with pytest.raises(RuntimeError, match="-1"):
        ops.ssim(cand, ref, win, win, sc, None, ws)
    assert (sc.cpu() == 7.0).all() and (ws_all.cpu() == SENT).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(backend):
    """Every refusal of include/pcdm.h returns -1 (RuntimeError from ops) and leaves scores, index and workspace untouched."""
    from pcdms_amd import ops
    dev = backend.device
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)  # noqa: E731

    def refused(cand, ref, cw, rw, sigma=1.2):
        sc = torch.full((cand.shape[0],), 7.0, device=dev)
        ix = torch.full((1,), -3, dtype=torch.int32, device=dev)
        ws = torch.full((1 << 16,), SENT, dtype=torch.uint8, device=dev)
        with pytest.raises(RuntimeError, match="-1"):
            ops.ssim(cand, ref, cw, rw, sc, ix, ws, sigma=sigma)
        backend.sync()
        assert (sc.cpu() == 7.0).all() and int(ix.cpu()) == -3 and (ws.cpu() == SENT).all()

    c, r = u8(3, 20, 24, 3), u8(1, 20, 24, 3)
    full = (0, 0, 24, 20)
    refused(c, r, (0, 0, 24, 8), (0, 0, 24, 8))                  # H < 2r + 1
    refused(c, r, (0, 0, 8, 20), (0, 0, 8, 20))                  # W < 2r + 1
    refused(c, r, full, full, sigma=2.5)                         # r = 9 > 8
    refused(c, r, (5, 0, 24, 20), full)                          # the candidate window leaves its image (x)
    refused(c, r, full, (0, 1, 24, 20))                          # the reference window leaves its image (y)
    refused(c, r, (-1, 0, 24, 20), full)                         # negative origin
    refused(c, r, full, (0, 0, 23, 20))                          # windows of different sizes
    refused(c, u8(2, 20, 24, 3), full, full)                     # reference batch neither 1 nor N
    refused(u8(3, 20, 24, 4), u8(1, 20, 24, 4), full, full)      # four channels
    refused(u8(3, 20, 24, 1), u8(1, 20, 24, 1), full, full)      # one channel
    assert ops.metrics_ws_bytes(3, 2, 24, 20, 1.2) == -1 and ops.metrics_ws_bytes(3, 1, 24, 8, 1.2) == -1 and ops.metrics_ws_bytes(3, 1, 24, 20, 2.5) == -1

    def refused_psnr(cand, ref, cw, rw):
        ps = torch.full((cand.shape[0],), 7.0, device=dev)
        ws = torch.full((1 << 12,), SENT, dtype=torch.uint8, device=dev)
        with pytest.raises(RuntimeError, match="-1"):
            ops.psnr(cand, ref, cw, rw, None, ps, ws)
        assert (ps.cpu() == 7.0).all() and (ws.cpu() == SENT).all()

    refused_psnr(c, r, (5, 0, 24, 20), full)
    refused_psnr(c, u8(2, 20, 24, 3), full, full)
    refused_psnr(u8(3, 20, 24, 4), u8(1, 20, 24, 4), full, full)
    out = torch.full((20, 24, 3), 9, dtype=torch.uint8, device=dev)
    ix = torch.zeros(1, dtype=torch.int32, device=dev)
    for cand, win in ((c, (1, 0, 24, 20)), (u8(3, 20, 24, 4), full)):
        with pytest.raises(RuntimeError, match="-1"):
            ops.select_image(cand, win, ix, out, False)
    assert (out.cpu() == 9).all()


def test_python_surface_refuses(backend):
    from pcdms_amd import metrics
    dev = backend.device
    a, b = torch.zeros(2, 20, 24, 3, dtype=torch.uint8, device=dev), torch.zeros(1, 20, 24, 3, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        metrics.ssim(a, b)                                        # mixed types
    with pytest.raises(ValueError):
        metrics.pick_best(b, b)                                   # selects from uint8 only
    with pytest.raises(ValueError):
        metrics.pick_best(a, a[:1], out="pil")
    with pytest.raises(RuntimeError, match="-1"):
        metrics.ssim(a, a[:1], sigma=2.5)


def test_cpu_tensors_refused_without_emulator(monkeypatch):
    """As everywhere in ops: CPU tensors are taken only when the emulator library is the loaded one."""
    from pcdms_amd import _lib, metrics
    from tests.emu import build_emu
    _lib.use_library(build_emu.load())
    monkeypatch.setattr(_lib, "_is_emu", False)            # what the product library answers
    a = torch.zeros(2, 20, 24, 3, dtype=torch.uint8)
    for call in (lambda: metrics.ssim(a, a[:1]), lambda: metrics.psnr(a, a[:1]), lambda: metrics.pick_best(a, a[:1])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


# ------------------------------------------------------------------------------------------------ pick and select
def _pick_candidates(H, W, levels, seed=21):
    rng = np.random.default_rng(seed)
    base = _smooth(H, W, rng)
    ref = _u8(base)[None]
    order = rng.permutation(len(levels))                                  # the best one is not at index 0 by construction
    cand = np.stack([_u8(base + rng.normal(0, levels[i], base.shape)) for i in order])
    return ref, cand


def _to_tensor_normalized(img_u8):
    """tools/stage2_batchtest_inpaint_model.py: transforms.Compose([ToTensor(), Normalize([0.5], [0.5])])."""
    x = torch.from_numpy(np.asarray(img_u8, dtype=np.float32) / 255.0).permute(2, 0, 1)
    return (x - 0.5) / 0.5


def test_pick_best(backend):
    from pcdms_amd import metrics
    H, W = (48, 40) if backend.is_emu else (512, 352)
    levels = [19 + 0.5 * i for i in range(8)] if not backend.is_emu else [19 + 3.0 * i for i in range(8)]   # (fewer pixels: wider spacing)
    ref, cand = _pick_candidates(H, W, levels)
    want = ssim64_batch(ref, cand)
    top = np.sort(want)[::-1]
    print("fp64 scores", want, "top two", top[:2])
    assert top[0] - top[1] >= 1e-3, "precondition: the generator must space the candidates a hundred tolerances apart"
    canvas = np.full((8, H + 4, 2 * W, 3), 77, dtype=np.uint8)             # the candidates are the right part of a canvas
    canvas[:, 2:2 + H, W:] = cand
    win = (W, 2, W, H)
    img, idx, scores = metrics.pick_best(_dev(canvas, backend), _dev(ref, backend), cand_window=win)
    backend.sync()
    assert idx.dtype == torch.int32 and idx.shape == (1,) and int(idx.cpu()) == int(np.argmax(want)) != 0
    assert (np.abs(scores.cpu().numpy() - want) <= TOL).all()
    best = cand[int(np.argmax(want))]
    assert img.dtype == torch.uint8 and np.array_equal(img.cpu().numpy(), best)
    imgn, idxn, _ = metrics.pick_best(_dev(canvas, backend), _dev(ref, backend), cand_window=win, out="normalized")
    assert int(idxn.cpu()) == int(idx.cpu()) and imgn.shape == (1, 3, H, W) and imgn.dtype == torch.float32
    assert torch.equal(imgn.cpu()[0].view(torch.int32), _to_tensor_normalized(best).view(torch.int32))


def test_pick_ties_and_nan(backend):
    from pcdms_amd import metrics
    rng = np.random.default_rng(23)
    H, W = 24, 20
    base = _smooth(H, W, rng)
    ref = _u8(base)[None]
    good, bad = _u8(base + rng.normal(0, 10, base.shape)), _u8(base + rng.normal(0, 60, base.shape))
    cand = np.stack([bad, good, bad, good])                                # two identical best candidates: the first wins
    img, idx, scores = metrics.pick_best(_dev(cand, backend), _dev(ref, backend))
    s = scores.cpu().numpy()
    assert int(idx.cpu()) == 1 == int(np.argmax(ssim64_batch(ref, cand))) and s[1] == s[3] and s[0] == s[2] and np.array_equal(img.cpu().numpy(), good)
    # constant candidate against constant reference: R = 0, 0/0 = NaN, and np.argmax ranks a NaN as the maximum (the first one)
    for cval, rval in ((0, 0), (200, 200), (200, 77)):
        const_ref = np.full((1, H, W, 3), rval, dtype=np.uint8)
        cand = np.stack([_u8(base), np.full((H, W, 3), cval, dtype=np.uint8), _u8(base), np.full((H, W, 3), cval, dtype=np.uint8)])
        img, idx, scores = metrics.pick_best(_dev(cand, backend), _dev(const_ref, backend))
        s = scores.cpu().numpy()
        assert np.isnan(s[1]) and np.isnan(s[3]) and np.isfinite(s[0]) and np.isfinite(s[2]), (cval, rval, s)
        assert int(idx.cpu()) == int(np.argmax(s)) == 1 and np.array_equal(img.cpu().numpy(), cand[1])
    assert np.isnan(ssim64(np.zeros((H, W, 3)), np.zeros((H, W, 3))))      # ... as the formula gives on the host


# ------------------------------------------------------------------------------------------------ no host sync
@pytest.mark.gpu
def test_pick_best_graph_capture(gpu_backend):
    """pick_best holds no host synchronisation: it is captured in a graph and replayed on new candidates copied into the same buffers."""
    from pcdms_amd import metrics
    dev = gpu_backend.device
    H, W = 128, 96
    ref, cand_a = _pick_candidates(H, W, [19 + 2.0 * i for i in range(8)], seed=31)
    _, cand_b = _pick_candidates(H, W, [19 + 2.0 * i for i in range(8)], seed=32)
    ia, ib = int(np.argmax(ssim64_batch(ref, cand_a))), int(np.argmax(ssim64_batch(ref, cand_b)))
    assert ia != ib
    cand, target = torch.from_numpy(cand_a).to(dev), torch.from_numpy(ref).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        metrics.pick_best(cand, target, out="normalized")           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        img, idx, scores = metrics.pick_best(cand, target, out="normalized")
    g.replay()
    torch.cuda.synchronize()
    assert int(idx.cpu()) == ia and torch.equal(img.cpu()[0], _to_tensor_normalized(cand_a[ia]))
    cand.copy_(torch.from_numpy(cand_b).to(dev))
    g.replay()
    torch.cuda.synchronize()
    assert int(idx.cpu()) == ib and torch.equal(img.cpu()[0], _to_tensor_normalized(cand_b[ib]))
    assert (np.abs(scores.cpu().numpy() - ssim64_batch(ref, cand_b)) <= TOL).all()


# ------------------------------------------------------------------------------------------------ drivers
def _load_driver(name):
    p = Path(__file__).resolve().parent.parent / "tools" / f"{name}.py"
    spec = importlib.util.spec_from_file_location(name, p)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fabricate(tmp_path):
    """Tiny checkpoints and data in the layouts of the stage-2 / stage-3 reference drivers (as tests/test_driver_stage2.py builds them)."""
    from PIL import Image
    from safetensors.torch import save_file

    from oracle import cond as OC
    from oracle import vae as OV
    from oracle.unet import UNetConfig, synth_state_dict
    from tests.test_encoders import TINY, _hf, _hf_clip
    from tests.test_from_pretrained import SD21_UNET_JSON
    sd21 = tmp_path / "sd21"
    for sub in ("unet", "vae", "scheduler"):
        (sd21 / sub).mkdir(parents=True)
    (sd21 / "unet" / "config.json").write_text(json.dumps(SD21_UNET_JSON))
    vcfg = OV.VAEConfig.tiny()
    (sd21 / "vae" / "config.json").write_text(json.dumps({"block_out_channels": list(vcfg.block_out_channels), "in_channels": 3, "out_channels": 3,
                                                          "latent_channels": 4, "layers_per_block": 2, "norm_num_groups": 32, "scaling_factor": 0.18215}))
    save_file({k: v.contiguous() for k, v in OV.synth_state_dict(vcfg, 2).items()}, str(sd21 / "vae" / "diffusion_pytorch_model.safetensors"))
    (sd21 / "scheduler" / "scheduler_config.json").write_text(json.dumps({
        "_class_name": "PNDMScheduler", "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085, "clip_sample": False,
        "num_train_timesteps": 1000, "prediction_type": "epsilon", "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1}))
    _, hf_dino = _hf(TINY, seed=3)
    hf_dino.save_pretrained(tmp_path / "dinov2")
    _, hf_clip = _hf_clip(dict(hidden_size=320, intermediate_size=640, num_hidden_layers=2, num_attention_heads=4, image_size=224, patch_size=14,
                               hidden_act="gelu", projection_dim=64), seed=4)
    hf_clip.save_pretrained(tmp_path / "clip")
    ucfg = UNetConfig.tiny()
    iproj = OC.synth(OC.image_proj_param_shapes(128, 64, ucfg.cross_attention_dim), 7, 1.0)
    module = {"unet." + k: v for k, v in synth_state_dict(ucfg, seed=5, random_affine=True).items()}
    module.update({"pose_proj." + k: v for k, v in OC.synth(OC.pose_param_shapes(ucfg.block_out_channels[0], 3, (16, 32, 96, 256)), 6).items()})
    module.update({"image_proj_model_p." + k: v for k, v in iproj.items()})
    u3 = UNetConfig.tiny(in_channels=8, class_embed_type=None, projection_class_embeddings_input_dim=None)
    module3 = {"unet." + k: v for k, v in synth_state_dict(u3, seed=8, random_affine=True).items()}
    module3.update({"image_proj_model_p." + k: v for k, v in iproj.items()})
    for d, m in (("ck2", module), ("ck3", module3)):
        (tmp_path / d).mkdir()
        torch.save({"module": m}, tmp_path / d / "mp_rank_00_model_states.pt")
    rng = np.random.default_rng(0)
    for d in ("img", "pose"):
        (tmp_path / d).mkdir()
    for n in ("a", "b", "c"):
        Image.fromarray(rng.integers(0, 255, (150, 90, 3), dtype=np.uint8)).save(tmp_path / "img" / f"{n}.png")
        Image.fromarray(rng.integers(0, 255, (150, 90, 3), dtype=np.uint8)).save(tmp_path / "pose" / f"{n}_pose.jpg")
    pairs = [{"source_image": "a.jpg", "target_image": "b.jpg"}, {"source_image": "b.jpg", "target_image": "c.jpg"}]
    (tmp_path / "train_data.json").write_text(json.dumps(pairs))          # "train": the CLIP embedding of the target, no stage-1 files
    common = ["--pretrained_model_name_or_path", str(sd21), "--image_encoder_p_path", str(tmp_path / "dinov2"), "--img_path", str(tmp_path / "img") + "/",
              "--pose_path", str(tmp_path / "pose") + "/", "--json_path", str(tmp_path / "train_data.json"), "--num_inference_steps", "3",
              "--img_width", "64", "--img_height", "128", "--calculate_metrics"]
    return pairs, common


TAG = "guidancescale2.0_seed42_numsteps3"


def _run_both(drv, common, pairs, tmp_path, stem):
    """The driver on the same seed with --metrics_device host and gpu -> {device: (ssim list, [(name, best index)], output directory)}."""
    res = {}
    for where in ("host", "gpu"):
        log = drv.BEST_INDEX_LOG
        del log[:]
        args = drv.build_parser().parse_args(common + ["--save_path", str(tmp_path / f"{stem}_{where}"), "--metrics_device", where])
        ssims = drv.inference(args, 0, pairs)
        res[where] = (ssims, list(log), tmp_path / f"{stem}_{where}" / TAG)
    (sh, ih, dh), (sg, ig, dg) = res["host"], res["gpu"]
    print(stem, "host", sh, ih, "gpu", sg, ig)
    assert len(sh) == len(sg) == len(pairs) and ih == ig and len(ih) == len(pairs)
    assert (np.abs(np.array(sh) - np.array(sg)) <= TOL).all(), (sh, sg)
    names = sorted(p.name for p in dh.glob("*.png"))
    assert names == sorted(n for n, _ in ih) == sorted(p.name for p in dg.glob("*.png"))
    for n in names:
        assert (dh / n).read_bytes() == (dg / n).read_bytes(), n
    return dh


@pytest.mark.gpu
def test_drivers_metrics_device(gpu_backend, tmp_path):
    """Stage-2 and stage-3 drivers with ``--metrics_device gpu`` against ``host`` on the same seed: the same best index per pair, SSIM lists within
    the tolerance, byte-identical PNGs; the default stays ``host``."""
    pytest.importorskip("transformers")
    pairs, common = _fabricate(tmp_path)
    d2, d3 = _load_driver("stage2_batchtest_inpaint_model"), _load_driver("stage3_batchtest_refined_model")
    assert d2.build_parser().parse_args([]).metrics_device == "host" and d3.build_parser().parse_args([]).metrics_device == "host"
    s2_dir = _run_both(d2, common + ["--image_encoder_g_path", str(tmp_path / "clip"), "--weights_name", str(tmp_path / "ck2")], pairs, tmp_path, "s2")
    _run_both(d3, common + ["--gen_t_img_path", str(s2_dir) + "/", "--weights_name", str(tmp_path / "ck3")], pairs, tmp_path, "s3")
