"""Device-side FID (pcdms_amd/metrics.py: InceptionV3Features, FIDStatistics, frechet_distance, FID; csrc/eval_nets.hip: pcdm_inception_features,
pcdm_conv2d_f32_ex, the pools, pcdm_inception_input, pcdm_fid_accumulate / _finalize).

The yardstick is an fp64 restatement of torchvision's ``inception_v3`` trunk with ``torch.nn.functional`` on the CPU (``_trunk`` below) on synthetic
seeded weights: He-scaled convolutions, BatchNorm gamma in U(0.5, 1.5), beta in U(-0.1, 0.1).  The running statistics are CALIBRATED on a seeded
batch, as a trained network's are: with means and variances drawn blindly (small means, variances in U(0.5, 1.5)) a random ReLU network 48
convolutions deep maps every image to nearly the same activation pattern, and 30 % (dims 768) to 50 % (dims 2048) of the features are 0 on
every test image -- a dead network that checks little.  So running_var = the channel's variance on a calibration batch of eight 75 x 75 images x U(0.5, 1.5), and
running_mean = the channel's mean - 2 standard deviations + U(-0.1, 0.1): 98 % of the pre-activations are positive, which keeps more than 90 %
of the features alive even where the last feature map is one pixel (75 x 75 inputs, batch 2).  ``_trunk_case`` asserts that on the fp64
reference.  Neither ``torchvision`` nor its checkpoint is available, so parity with upstream on its weights is not pinned here.

Tolerances.  The convolution: the fp32-input MFMA's documented error, 3.5e-7 sum |a b| per output.  The average pool: nine fp32 roundings,
9 * 2^-24 < 1e-6 of max |x|.  The input stage: 16 x the error of the same torch call in fp32, floor 2^-22 max |x|.  The trunk: MEASURED, not fixed --
e_ref = the largest feature error of the fp32 CPU restatement (convolution, then unfused BatchNorm, as torchvision computes it) against fp64,
relative to max |feature|; the device must be within 16 e_ref (it adds each output as one sequential chain where the CPU library adds in blocks),
and a restatement with bf16 convolution operands must EXCEED that bound, so the bound discriminates.  ``test_trunk_gpu`` writes e_ref, the device
error and the bf16 error per case to profiles/fid_values.json.
"""
from __future__ import annotations

import functools
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
MFMA_F32_ERR = 3.5e-7            # per output, times sum |a b| (fp32-input MFMA = a k-ordered fmaf chain)
SCALE = (0.229 / 0.5, 0.224 / 0.5, 0.225 / 0.5)
SHIFT = ((0.485 - 0.5) / 0.5, (0.456 - 0.5) / 0.5, (0.406 - 0.5) / 0.5)


# ------------------------------------------------------------------------------------------------ synthetic weights and the fp64 restatement
@functools.lru_cache(maxsize=None)
def _state_dict(seed=0):
    from pcdms_amd.metrics import INCEPTION_CONVS
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, co, ci, kh, kw in INCEPTION_CONVS:
        sd[f"{name}.conv.weight"] = torch.randn(co, ci, kh, kw, generator=g) * math.sqrt(2.0 / (ci * kh * kw))
        sd[f"{name}.bn.weight"] = torch.rand(co, generator=g) + 0.5
        sd[f"{name}.bn.bias"] = (torch.rand(co, generator=g) * 2 - 1) * 0.1
        sd[f"{name}.bn.running_mean"] = (torch.rand(co, generator=g) * 2 - 1) * 0.1
        sd[f"{name}.bn.running_var"] = torch.rand(co, generator=g) + 0.5
        sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(7)
    _trunk(_net_input(_images(8, 75, 75, 99), resize=False), 2048, calibrate=(sd, g))       # the size of most trunk cases
    sd["fc.weight"] = torch.zeros(4, 2048)                                     # torchvision has more keys: ignored
    sd["AuxLogits.conv0.conv.weight"] = torch.zeros(128, 768, 1, 1)
    return sd


def _trunk(x, dims, dtype=torch.float64, operand=None, calibrate=None, sd=None, as_tensor=False):
    """x: the NETWORK input [N, 3, H, W] (resized and remapped) -> the [N, dims] features as fp64 numpy.  ``dtype``: the arithmetic; ``operand``:
    a narrower type the convolution operands are rounded to first (the bf16 implicit-GEMM model).  ``calibrate`` = (state dict, generator):
    set every layer's running statistics from this batch as it passes (the module docstring), once, while the weights are made."""
    sd = sd if sd is not None else _state_dict() if calibrate is None else calibrate[0]     # (sd: the weights on another device, tools/bench_fid.py)
    q = (lambda t: t) if operand is None else (lambda t: t.to(operand).to(dtype))

    def bc(h, name, stride=1, padding=0):
        h = F.conv2d(q(h), q(sd[f"{name}.conv.weight"].to(dtype)), None, stride=stride, padding=padding)
        if calibrate is not None:
            co, var = h.shape[1], h.var((0, 2, 3))
            sd[f"{name}.bn.running_var"] = (var * (torch.rand(co, generator=calibrate[1]) + 0.5)).float()
            sd[f"{name}.bn.running_mean"] = (h.mean((0, 2, 3)) - 2.0 * var.sqrt() + (torch.rand(co, generator=calibrate[1]) * 2 - 1) * 0.1).float()
        p = [sd[f"{name}.bn.{k}"].to(dtype) for k in ("running_mean", "running_var", "weight", "bias")]
        return F.relu(F.batch_norm(h, p[0], p[1], p[2], p[3], False, 0.0, 1e-3))

    def inc_a(h, n):
        b1 = bc(h, f"{n}.branch1x1")
        b5 = bc(bc(h, f"{n}.branch5x5_1"), f"{n}.branch5x5_2", padding=2)
        b3 = bc(bc(bc(h, f"{n}.branch3x3dbl_1"), f"{n}.branch3x3dbl_2", padding=1), f"{n}.branch3x3dbl_3", padding=1)
        return torch.cat([b1, b5, b3, bc(F.avg_pool2d(h, 3, 1, 1), f"{n}.branch_pool")], 1)

    def inc_b(h, n):
        b3 = bc(h, f"{n}.branch3x3", stride=2)
        bd = bc(bc(bc(h, f"{n}.branch3x3dbl_1"), f"{n}.branch3x3dbl_2", padding=1), f"{n}.branch3x3dbl_3", stride=2)
        return torch.cat([b3, bd, F.max_pool2d(h, 3, 2)], 1)

    def inc_c(h, n):
        b1 = bc(h, f"{n}.branch1x1")
        b7 = bc(bc(bc(h, f"{n}.branch7x7_1"), f"{n}.branch7x7_2", padding=(0, 3)), f"{n}.branch7x7_3", padding=(3, 0))
        bd = bc(h, f"{n}.branch7x7dbl_1")
        for i, pad in ((2, (3, 0)), (3, (0, 3)), (4, (3, 0)), (5, (0, 3))):
            bd = bc(bd, f"{n}.branch7x7dbl_{i}", padding=pad)
        return torch.cat([b1, b7, bd, bc(F.avg_pool2d(h, 3, 1, 1), f"{n}.branch_pool")], 1)

    def inc_d(h, n):
        b3 = bc(bc(h, f"{n}.branch3x3_1"), f"{n}.branch3x3_2", stride=2)
        b7 = bc(bc(bc(h, f"{n}.branch7x7x3_1"), f"{n}.branch7x7x3_2", padding=(0, 3)), f"{n}.branch7x7x3_3", padding=(3, 0))
        return torch.cat([b3, bc(b7, f"{n}.branch7x7x3_4", stride=2), F.max_pool2d(h, 3, 2)], 1)

    def inc_e(h, n):
        b1 = bc(h, f"{n}.branch1x1")
        b3 = bc(h, f"{n}.branch3x3_1")
        b3 = torch.cat([bc(b3, f"{n}.branch3x3_2a", padding=(0, 1)), bc(b3, f"{n}.branch3x3_2b", padding=(1, 0))], 1)
        bd = bc(bc(h, f"{n}.branch3x3dbl_1"), f"{n}.branch3x3dbl_2", padding=1)
        bd = torch.cat([bc(bd, f"{n}.branch3x3dbl_3a", padding=(0, 1)), bc(bd, f"{n}.branch3x3dbl_3b", padding=(1, 0))], 1)
        return torch.cat([b1, b3, bd, bc(F.avg_pool2d(h, 3, 1, 1), f"{n}.branch_pool")], 1)

    h = x.to(dtype)
    h = F.max_pool2d(bc(bc(bc(h, "Conv2d_1a_3x3", stride=2), "Conv2d_2a_3x3"), "Conv2d_2b_3x3", padding=1), 3, 2)
    if dims > 64:
        h = F.max_pool2d(bc(bc(h, "Conv2d_3b_1x1"), "Conv2d_4a_3x3"), 3, 2)
    if dims > 192:
        for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            h = inc_a(h, n)
        h = inc_b(h, "Mixed_6a")
        for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            h = inc_c(h, n)
    if dims > 768:
        h = inc_e(inc_e(inc_d(h, "Mixed_7a"), "Mixed_7b"), "Mixed_7c")
    assert h.shape[1] == dims
    return h.mean((2, 3)) if as_tensor else h.mean((2, 3)).double().cpu().numpy()


def _net_input(img, window=None, resize=True, dtype=torch.float64):
    """uint8 NHWC or fp32 NCHW numpy -> the network input [N, 3, H', W'] in ``dtype``: x = p / 255, crop, bilinear 299 x 299, the reference's remap"""
    x = torch.from_numpy(img)
    x = x.permute(0, 3, 1, 2).to(dtype) / 255.0 if img.dtype == np.uint8 else x.to(dtype)
    if window is not None:
        x0, y0, W, H = window
        x = x[:, :, y0:y0 + H, x0:x0 + W]
    if resize:
        x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    return x * torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1) + torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)


def _images(N, H, W, seed, kind="f32"):
    """smooth structure + noise in [0, 1]: fp32 NCHW, or the same pictures as uint8 NHWC"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    imgs = []
    for n in range(N):
        ph = rng.uniform(0, 6.28, 3)
        base = np.stack([0.5 + 0.3 * np.sin(x / (4.0 + n) + p) * np.cos(y / (6.0 + c) + 2 * p) for c, p in enumerate(ph)])
        imgs.append(np.clip(base + rng.normal(0, 0.15, base.shape), 0, 1))
    a = np.stack(imgs)
    if kind == "u8":
        return np.ascontiguousarray(np.rint(a * 255).astype(np.uint8).transpose(0, 2, 3, 1))
    return np.ascontiguousarray(a.astype(np.float32))


def _dev(a, backend):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(backend.device)


@functools.lru_cache(maxsize=None)
def _model(dims, resize):
    from pcdms_amd import metrics
    return metrics.InceptionV3Features(dims, resize_input=resize).load_state_dict(_state_dict())


@functools.lru_cache(maxsize=None)
def _trunk_case(dims, H, W, kind, resize, seed):
    """-> (images, fp64 features, e_ref, e_bf16): the errors of the fp32 CPU restatement and of the bf16-operand one, relative to max |feature|"""
    img = _images(2, H, W, seed, kind)
    want = _trunk(_net_input(img, resize=resize), dims)
    f32 = _trunk(_net_input(img, resize=resize, dtype=torch.float32), dims, dtype=torch.float32)
    bf16 = _trunk(_net_input(img, resize=resize), dims, dtype=torch.float32, operand=torch.bfloat16)
    scale = np.abs(want).max()
    alive = (want[0] != want[1]).mean()
    assert np.isfinite(want).all() and alive >= 0.9, f"the synthetic network is dead: {alive:.2f} of the features vary"
    return img, want, np.abs(f32 - want).max() / scale, np.abs(bf16 - want).max() / scale


def _trunk_check(backend, dims, H, W, kind, resize, seed):
    img, want, e_ref, e_bf16 = _trunk_case(dims, H, W, kind, resize, seed)
    m = _model(dims, resize)
    x = _dev(img, backend)
    got, again = m(x), m(x)
    swapped = m(_dev(img[::-1].copy(), backend))
    backend.sync()
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, dims) and got.device.type == backend.device.type
    e_dev = np.abs(got.cpu().double().numpy() - want).max() / np.abs(want).max()
    print(f"dims {dims} {H}x{W} {kind} resize={resize}: e_ref {e_ref:.3e} device {e_dev:.3e} bf16 {e_bf16:.3e} (bound {16 * e_ref:.3e})")
    assert e_dev <= 16 * e_ref, (e_dev, e_ref)
    assert e_bf16 > 16 * e_ref, (e_bf16, e_ref)                                 # the bound would not admit bf16 operands
    assert torch.equal(got, again)                                             # reruns are bit-identical
    assert torch.equal(swapped.flip(0), got)                                   # a row does not depend on its place in the batch
    return e_ref, e_dev, e_bf16


# ------------------------------------------------------------------------------------------------ 1. the generalised convolution
CONV_CASES = [(1, 7, 1, (0, 3)), (7, 1, 1, (3, 0)), (1, 3, 1, (0, 1)), (3, 1, 1, (1, 0)), (3, 3, 2, (0, 0)), (5, 5, 1, (2, 2))]


@pytest.mark.parametrize("Cin", [8, 12])
@pytest.mark.parametrize("kh,kw,stride,pad", CONV_CASES)
def test_conv_ex(backend, Cin, kh, kw, stride, pad):
    from pcdms_amd import ops
    B, Hi, Wi, Cout, pitch, off, sentinel = 2, 5, 6, 20, 40, 12, -77.25
    g = torch.Generator().manual_seed(100 * kh + 10 * kw + Cin)
    x = torch.rand(B, Cin, Hi, Wi, generator=g) * 2 - 1
    w = torch.randn(Cout, Cin, kh, kw, generator=g) * math.sqrt(2.0 / (Cin * kh * kw))
    bias = (torch.rand(Cout, generator=g) * 2 - 1) * 0.1
    pw = ops.pack_lpips_conv(w, bias, backend.device)
    xn = _dev(x.permute(0, 2, 3, 1).contiguous(), backend)
    want = F.relu(F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=pad))
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, stride=stride, padding=pad)
    Ho, Wo = want.shape[2:]
    out = torch.full((B, Ho, Wo, pitch), sentinel, dtype=torch.float32, device=backend.device)
    ops.conv2d_f32_ex(xn, pw, stride=stride, pad=pad, relu=True, out=out, offset=off)
    backend.sync()
    o = out.cpu()
    assert (o[..., :off] == sentinel).all() and (o[..., off + Cout:] == sentinel).all()      # nothing outside the slice was written
    err = (o[..., off:off + Cout].double().permute(0, 3, 1, 2) - want).abs()
    print(f"conv {kh}x{kw} s{stride} p{pad} Cin {Cin}: max err / sum|ab| = {(err / mag).max().item():.3e}")
    assert (err <= MFMA_F32_ERR * mag).all()
    tight = ops.conv2d_f32_ex(xn, pw, stride=stride, pad=pad, relu=True)
    backend.sync()
    assert torch.equal(tight.cpu(), o[..., off:off + Cout])
    if pad[0] == pad[1]:                                                       # the old entry point: bit for bit
        assert torch.equal(ops.conv2d_f32(xn, pw, stride=stride, pad=pad[0], relu=True).cpu(), tight.cpu())


# ------------------------------------------------------------------------------------------------ 2. the pools
def test_pools(backend):
    from pcdms_amd import ops
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 5, 7, 8, generator=g)
    got = ops.avgpool3_f32(_dev(x, backend))
    backend.sync()
    want = F.avg_pool2d(x.double().permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1)
    assert (got.cpu().double() - want).abs().max().item() <= 1e-6 * x.abs().max().item()
    for nan in (False, True):
        xm = x.clone()
        if nan:
            xm[0, 2, 2, 3] = float("nan")                                      # the centre pixel: in four of the six windows
            xm[1, 0, 6, 0] = float("nan")
        out = torch.full((2, 2, 3, 16), 5.5, dtype=torch.float32, device=backend.device)
        ops.maxpool3s2_f32_ex(_dev(xm, backend), out, offset=4)
        backend.sync()
        o = out.cpu()
        want = F.max_pool2d(xm.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
        assert (o[..., :4] == 5.5).all() and (o[..., 12:] == 5.5).all()
        got = o[..., 4:12]
        assert torch.equal(got.isnan(), want.isnan()) and want.isnan().any().item() == nan
        assert torch.equal(got.nan_to_num(nan=9e9), want.nan_to_num(nan=9e9))


# ------------------------------------------------------------------------------------------------ 3. the input stage
@pytest.mark.parametrize("H,W,N", [(48, 32, 2), (352, 512, 1)])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_input_stage(backend, H, W, N, kind):
    from pcdms_amd import ops
    img = _images(N, H, W, H + W, kind)
    got = ops.inception_input(_dev(img, backend), (0, 0, W, H), resize=True, normalize=True)
    backend.sync()
    got = got.cpu()
    want = _net_input(img)
    e32 = (_net_input(img, dtype=torch.float32).double() - want).abs().max().item()
    bound = max(16 * e32, 2.0 ** -22 * want.abs().max().item())
    err = (got[..., :3].double().permute(0, 3, 1, 2) - want).abs().max().item()
    print(f"input {H}x{W} {kind}: device err {err:.3e}, torch fp32 err {e32:.3e}, bound {bound:.3e}")
    assert tuple(got.shape) == (N, 299, 299, 4) and (got[..., 3] == 0).all() and err <= bound


def test_input_stage_window(backend):
    from pcdms_amd import ops
    H, W, N = 40, 36, 2
    src, tgt = _images(N, H, W, 1, "u8"), _images(N, H, W, 2, "u8")
    canvas = np.concatenate([src, tgt], axis=2)                                # [source | target]
    win = (W, 0, W, H)
    got = ops.inception_input(_dev(canvas, backend), win, resize=True, normalize=True)
    crop = ops.inception_input(_dev(tgt, backend), (0, 0, W, H), resize=True, normalize=True)
    same = ops.inception_input(_dev(canvas, backend), win, resize=False, normalize=False)
    backend.sync()
    assert torch.equal(got, crop)
    want = _net_input(canvas, window=win)
    e32 = (_net_input(canvas, window=win, dtype=torch.float32).double() - want).abs().max().item()
    assert (got.cpu()[..., :3].double().permute(0, 3, 1, 2) - want).abs().max().item() <= max(16 * e32, 2.0 ** -22 * want.abs().max().item())
    assert tuple(same.shape) == (N, H, W, 4)                                   # no resize, no remap: the fp32 image itself
    assert (same.cpu()[..., :3].double() - torch.from_numpy(tgt).double() / 255).abs().max().item() <= 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 4. global pool and statistics
def test_global_pool(backend):
    from pcdms_amd import ops
    x = torch.randn(3, 5, 7, 40, generator=torch.Generator().manual_seed(8)) + 0.5
    got = ops.global_avgpool_f32(_dev(x, backend))
    backend.sync()
    want = x.double().mean((1, 2))
    assert tuple(got.shape) == (3, 40) and ((got.cpu().double() - want).abs() <= 2.0 ** -24 * want.abs() + 1e-30).all()


def test_statistics(backend, tmp_path):
    from pcdms_amd import metrics
    D = 40
    feats = (torch.randn(13, D, generator=torch.Generator().manual_seed(9)) * 0.3 + 0.5).float()
    whole, split = metrics.FIDStatistics(D), metrics.FIDStatistics(D)
    whole.update(_dev(feats, backend))
    for part in (feats[:5], feats[5:6], feats[6:]):
        split.update(_dev(part.contiguous(), backend))
    mu, sigma = whole.finalize()
    mu2, sigma2 = split.finalize()
    backend.sync()
    assert whole.count == split.count == 13 and mu.dtype == sigma.dtype == torch.float64
    assert torch.equal(whole.sum, split.sum) and torch.equal(whole.gram, split.gram) and torch.equal(mu, mu2) and torch.equal(sigma, sigma2)
    a = feats.double().numpy()
    want_mu, want_sigma = np.mean(a, 0), np.cov(a, rowvar=False)
    assert np.abs(mu.cpu().numpy() - want_mu).max() <= 1e-12 * np.abs(want_mu).max()
    assert np.abs(sigma.cpu().numpy() - want_sigma).max() <= 1e-12 * np.abs(want_sigma).max()
    assert torch.equal(sigma, sigma.T)
    whole.save(tmp_path / "stats.npz")
    with np.load(tmp_path / "stats.npz") as f:
        assert sorted(f.files) == ["mu", "sigma"] and f["mu"].dtype == np.float64
        assert np.array_equal(f["mu"], mu.cpu().numpy()) and np.array_equal(f["sigma"], sigma.cpu().numpy())
    back = metrics.FIDStatistics.load(tmp_path / "stats.npz").finalize()
    assert torch.equal(back[0], mu.cpu()) and torch.equal(back[1], sigma.cpu())
    np.savez(tmp_path / "theirs.npz", mu=want_mu, sigma=want_sigma)            # a file as the reference writes it
    # 13 samples of 40 features: rank 12.  Each of the 28 zero eigenvalues of S^1/2 S S^1/2 comes out as +-eps lambda_max^2 and its square root as
    # sqrt(eps) lambda_max = 1.5e-8 lambda_max, so identical statistics are 0 only to D sqrt(eps) tr S here (1e-9 tr S needs full rank: test 5)
    assert abs(metrics.FID(None)(whole, tmp_path / "theirs.npz")) <= D * math.sqrt(2.0 ** -52) * np.trace(want_sigma)
    with pytest.raises(ValueError):
        metrics.FIDStatistics(D).update(_dev(feats[:1], backend)).finalize()   # one sample has no covariance
    with pytest.raises(ValueError):
        whole.update(_dev(feats[:, :8].contiguous(), backend))


# ------------------------------------------------------------------------------------------------ 5. the Frechet distance (host)
def _cov(n, D, seed, shift=0.0):
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 1, (n, D)) @ rng.normal(0, 1 / math.sqrt(D), (D, D)) + shift
    return np.mean(a, 0), np.cov(a, rowvar=False)


def test_frechet_distance():
    from pcdms_amd.metrics import frechet_distance
    D = 48
    rng = np.random.default_rng(0)
    a, b = rng.uniform(0.1, 2.0, D), rng.uniform(0.1, 2.0, D)
    m1, m2 = rng.normal(0, 1, D), rng.normal(0, 1, D)
    closed = np.sum((m1 - m2) ** 2) + np.sum((np.sqrt(a) - np.sqrt(b)) ** 2)
    assert abs(frechet_distance(m1, np.diag(a), m2, np.diag(b)) - closed) <= 1e-12 * closed
    mu1, s1 = _cov(200, D, 1)
    mu2, s2 = _cov(200, D, 2, shift=0.3)
    assert abs(frechet_distance(mu1, s1, mu1, s1)) <= 1e-9 * np.trace(s1)
    d12, d21 = frechet_distance(mu1, s1, mu2, s2), frechet_distance(mu2, s2, mu1, s1)
    assert d12 > 0.1 and abs(d12 - d21) <= 1e-10 * d12
    assert frechet_distance(torch.from_numpy(mu1), torch.from_numpy(s1), mu2, s2) == d12      # tensors or arrays
    r1, r2 = _cov(20, D, 3), _cov(20, D, 4, shift=0.1)                         # 20 samples of 48 features: rank 19
    d = frechet_distance(*r1, *r2)
    assert np.isfinite(d) and d > 0 and np.isfinite(frechet_distance(*r1, *r1))
    with pytest.raises(ValueError):
        frechet_distance(mu1, s1, mu2[:8], s2[:8, :8])


def test_frechet_distance_vs_scipy():
    linalg = pytest.importorskip("scipy.linalg")
    from pcdms_amd.metrics import frechet_distance
    mu1, s1 = _cov(200, 48, 1)
    mu2, s2 = _cov(200, 48, 2, shift=0.3)
    covmean = linalg.sqrtm(s1.dot(s2))
    assert np.isfinite(covmean).all()
    want = np.sum((mu1 - mu2) ** 2) + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean.real)
    assert abs(frechet_distance(mu1, s1, mu2, s2) - want) <= 1e-9 * want


# ------------------------------------------------------------------------------------------------ 6. / 7. the trunk
@pytest.mark.parametrize("dims", [64, 192])
def test_trunk_stem(backend, dims):
    """35 x 35 without the resize: the stem alone, small enough for the lane emulator (blocks 2 and 3: test_trunk_gpu)"""
    _trunk_check(backend, dims, 35, 35, "f32", False, seed=11)


@pytest.mark.slow
def test_trunk_full_emulator():
    """all 94 convolutions and every pool of the table under the lane emulator, once, at the smallest input (75 x 75, batch 2; about 25 s): the
    wiring of blocks 2 and 3 is then checked without a GPU too"""
    from pcdms_amd import _lib
    from tests.emu import build_emu
    from tests.conftest import Backend
    _lib.use_library(build_emu.load())
    _trunk_check(Backend("emu", torch.device("cpu")), 2048, 75, 75, "f32", False, seed=12)


TRUNK_GPU_CASES = [(64, 75, 75, "f32", False), (192, 75, 75, "f32", False), (768, 75, 75, "f32", False), (2048, 75, 75, "f32", False),
                   (2048, 64, 48, "u8", True)]


@pytest.mark.gpu
@pytest.mark.parametrize("dims,H,W,kind,resize", TRUNK_GPU_CASES)
def test_trunk_gpu(gpu_backend, dims, H, W, kind, resize):
    e_ref, e_dev, e_bf16 = _trunk_check(gpu_backend, dims, H, W, kind, resize, seed=12)
    path = ROOT / "profiles" / "fid_values.json"
    values = json.loads(path.read_text()) if path.exists() else {}
    values[f"dims{dims}_{H}x{W}_{kind}_{'resize299' if resize else 'own_size'}"] = {
        "e_ref_fp32_cpu": e_ref, "device": e_dev, "bf16_operands": e_bf16, "bound_16_e_ref": 16 * e_ref}
    try:
        path.write_text(json.dumps(values, indent=1, sort_keys=True) + "\n")
    except OSError:
        pass                                                                   # a read-only checkout still runs the assertions above


# ------------------------------------------------------------------------------------------------ 8. end to end
@functools.lru_cache(maxsize=None)
def _e2e_sets():
    """two sets of 200 images of 35 x 35 that differ by a smooth perturbation; their fp64 and fp32-CPU features at dims = 64"""
    a = _images(200, 35, 35, 31)
    y, x = np.mgrid[0:35, 0:35]
    b = np.clip(_images(200, 35, 35, 32) + (0.08 * np.sin(x / 9.0) * np.cos(y / 7.0)).astype(np.float32), 0, 1).astype(np.float32)
    f64 = [_trunk(_net_input(s, resize=False), 64) for s in (a, b)]
    f32 = [_trunk(_net_input(s, resize=False, dtype=torch.float32), 64, dtype=torch.float32) for s in (a, b)]
    return a, b, f64, f32


def _host_fid(fa, fb):
    from pcdms_amd.metrics import frechet_distance
    return frechet_distance(np.mean(fa, 0), np.cov(fa, rowvar=False), np.mean(fb, 0), np.cov(fb, rowvar=False))


@pytest.mark.gpu
def test_fid_end_to_end(gpu_backend):
    from pcdms_amd import metrics
    a, b, f64, f32 = _e2e_sets()
    want, cpu32 = _host_fid(*f64), _host_fid(*f32)
    tr = sum(np.trace(np.cov(f, rowvar=False)) for f in f64)
    fid = metrics.FID(_model(64, False))
    sa = fid.statistics(_dev(a[i:i + 64], gpu_backend) for i in range(0, 200, 64))
    sb = fid.statistics(_dev(b[i:i + 64], gpu_backend) for i in range(0, 200, 64))
    got = fid(sa, sb)
    bound = max(16 * abs(cpu32 - want), 1e-6 * tr)
    print(f"FID device {got:.9g} fp64 {want:.9g} fp32 CPU {cpu32:.9g} bound {bound:.3e} tr {tr:.4g}")
    assert sa.count == sb.count == 200 and want > 1e-4 * tr, "precondition: the two sets are apart"
    assert abs(got - want) <= bound
    dropped = fid.statistics((_dev(a[i:i + 64], gpu_backend) for i in range(0, 200, 64)), drop_remainder=128)
    assert dropped.count == 128                                                # the reference's 200 // 128 full batches
    # model + update inside one captured graph: no host synchronisation, no allocation inside the library
    m, x = _model(64, False), _dev(a[:64], gpu_backend)
    eager = metrics.FIDStatistics(64).update(m(x))
    torch.cuda.synchronize()
    st = metrics.FIDStatistics(64).update(m(x)[:0])                             # allocates the zeroed state outside the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st.update(m(x))
    g.replay()
    torch.cuda.synchronize()
    assert st.count == 64 and torch.equal(st.sum, eager.sum) and torch.equal(st.gram, eager.gram)


# ------------------------------------------------------------------------------------------------ 9. refusals, loading, the tool
def test_refusals(backend):
    from pcdms_amd import metrics, ops
    dev = backend.device
    assert ops.inception_ws_bytes(1, 75, 75, 2048) > 0 and ops.inception_ws_bytes(1, 74, 75, 2048) == -1 and ops.inception_ws_bytes(1, 75, 74, 2048) == -1
    assert ops.inception_ws_bytes(1, 75, 75, 100) == -1 and ops.inception_ws_bytes(0, 75, 75, 64) == -1 and ops.inception_ws_bytes(2, 299, 299, 2048) > 0
    full = _model(2048, False)
    for shape, window in (((1, 3, 74, 80), None), ((1, 3, 80, 74), None), ((1, 3, 80, 80), (2, 2, 74, 75))):
        with pytest.raises(ValueError, match="75"):
            full(torch.zeros(shape, device=dev), window=window)
    with pytest.raises(ValueError, match="window"):
        full(torch.zeros(1, 3, 80, 80, device=dev), window=(10, 0, 75, 75))
    for dims in (0, 100, 1024):
        with pytest.raises(ValueError, match="dims"):
            metrics.InceptionV3Features(dims)
    stem = _model(64, False)
    with pytest.raises(ValueError):
        stem(torch.zeros(1, 3, 35, 35, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        stem(torch.zeros(1, 35, 35, 3, device=dev))                            # fp32 is NCHW
    with pytest.raises(RuntimeError, match="no weights"):
        metrics.InceptionV3Features(64)(torch.zeros(1, 3, 35, 35, device=dev))
    st = metrics.FIDStatistics(64)
    with pytest.raises(ValueError):
        st.update(torch.zeros(2, 64, dtype=torch.float64, device=dev))
    if dev.type == "cuda":                                                     # mixed devices
        st.update(torch.zeros(2, 64, device=dev))
        with pytest.raises(ValueError):
            st.update(torch.zeros(2, 64))
    # the library itself: a slice that does not fit its tensor, a workspace that is too small
    pw = ops.pack_lpips_conv(torch.zeros(20, 8, 1, 1), None, dev)
    x = torch.zeros(1, 4, 4, 8, device=dev)
    with pytest.raises(RuntimeError, match="code -1"):
        ops.conv2d_f32_ex(x, pw, out=torch.zeros(1, 4, 4, 40, device=dev), offset=21)
    with pytest.raises(RuntimeError, match="code -1"):
        ops.maxpool3s2_f32_ex(x, torch.zeros(1, 1, 1, 12, device=dev), offset=8)
    before = torch.full((1, 64), 3.0, device=dev)
    with pytest.raises(RuntimeError, match="code -1"):
        ops.inception_features(torch.zeros(1, 3, 35, 35, device=dev), (0, 0, 35, 35), stem._weights(dev), before,
                               torch.empty(2, dtype=torch.float64, device=dev), dims=64, resize=False, normalize=True)
    backend.sync()
    assert (before == 3.0).all()                                               # refused: nothing written


def test_state_dict_loading(backend, tmp_path):
    from pcdms_amd import metrics
    sd = dict(_state_dict())
    a = metrics.InceptionV3Features(192).load_state_dict(sd)
    assert len(a.packed) == 5
    from safetensors.torch import save_file
    torch.save(sd, tmp_path / "inception.pth")
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "inception.safetensors"))
    for name in ("inception.pth", "inception.safetensors"):
        b = metrics.InceptionV3Features.from_pretrained(tmp_path / name, dims=192)
        assert all(torch.equal(p["w"], q["w"]) and torch.equal(p["bias"], q["bias"]) for p, q in zip(a.packed, b.packed))
    assert len(metrics.InceptionV3Features().load_state_dict(sd).packed) == 94
    bad = dict(sd)
    del bad["Conv2d_4a_3x3.bn.running_var"]
    with pytest.raises(KeyError, match="Conv2d_4a_3x3.bn.running_var"):
        metrics.InceptionV3Features(192).load_state_dict(bad)
    metrics.InceptionV3Features(64).load_state_dict(bad)                       # dims = 64 does not need that layer
    bad = dict(sd)
    bad["Conv2d_2b_3x3.conv.weight"] = torch.zeros(64, 32, 1, 3)
    with pytest.raises(ValueError, match=r"Conv2d_2b_3x3.*\(64, 32, 1, 3\).*\(64, 32, 3, 3\)"):
        metrics.InceptionV3Features(64).load_state_dict(bad)
    bad = dict(sd)
    bad["Mixed_7c.branch_pool.bn.bias"] = torch.zeros(191)
    with pytest.raises(ValueError, match=r"Mixed_7c.branch_pool.*\(191,\).*\(192,\)"):
        metrics.InceptionV3Features().load_state_dict(bad)


def test_score_pairs_tool_fid(backend, tmp_path, capsys):
    """the tool with --fid-*: dims 64 without the resize, so the lane emulator can run it"""
    from PIL import Image

    from pcdms_amd import metrics
    from tools import score_pairs
    H, W = 40, 36
    gen, real = _images(6, H, W, 41, "u8"), _images(6, H, W, 42, "u8")
    for d, imgs in (("gen", gen), ("real", real)):
        (tmp_path / d).mkdir()
        for i, im in enumerate(imgs):
            Image.fromarray(im).save(tmp_path / d / f"{i:03d}.png")
    torch.save(dict(_state_dict()), tmp_path / "inception.pth")
    common = [str(tmp_path / "gen"), str(tmp_path / "real"), "--fid-weights", str(tmp_path / "inception.pth"), "--fid-dims", "64", "--fid-no-resize"]
    res = score_pairs.main(common + ["--fid-real", str(tmp_path / "real"), "--fid-batch", "4", "--fid-drop-remainder"], device=backend.device)
    text = capsys.readouterr().out
    fid = metrics.FID(_model(64, False))
    first4 = fid(fid.statistics([_dev(gen[:4], backend)]), fid.statistics([_dev(real[:4], backend)]))
    assert res["fid"] == first4 and np.isfinite(first4) and "FID: %.4f" % first4 in text and "PSNR:" in text and "lpips" not in res
    every = fid.statistics([_dev(real, backend)])
    every.save(tmp_path / "real.npz")
    res = score_pairs.main(common + ["--fid-real", str(tmp_path / "real.npz"), "--fid-batch", "4"], device=backend.device)
    capsys.readouterr()
    assert res["fid"] == fid(fid.statistics([_dev(gen, backend)]), every) and res["fid"] != first4
    want = _host_fid(_trunk(_net_input(gen, resize=False), 64), _trunk(_net_input(real, resize=False), 64))
    assert abs(res["fid"] - want) <= 1e-4 * abs(want)                          # six samples of 64 features: ill-conditioned, a sanity check only
