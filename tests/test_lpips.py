"""Device-side LPIPS v0.1 (AlexNet) in exact fp32 (pcdms_amd/metrics.py: LPIPS; csrc/eval_nets.hip: pcdm_lpips / pcdm_conv2d_f32 / pcdm_maxpool3s2_f32).

The yardstick is an fp64 restatement of the network with ``torch.nn.functional`` on the CPU (``_net`` below), on synthetic seeded weights:
neither the ``lpips`` package nor ``torchvision`` nor a real checkpoint is available, so parity with upstream on its weights is not pinned here.

Tolerance ``TOL`` = 1e-6 absolute, on the total AND on each of the five per-tap values.  Where it comes from: the same restatement run in fp32
(torch, CPU) is at most 5e-8 from fp64, and one whose convolution operands are rounded to bf16 is 5e-6 .. 9e-5 away on every non-identical
case; 1e-6 is 20x the former and below the latter, so it separates an exact-fp32 kernel from a reduced-precision one.  ``test_yardstick_models``
recomputes both models for this file's seeds and asserts exactly that, so the bound cannot quietly admit a bf16 path.

Measured on the MI355X (profiles/lpips_values.json): worst |device - fp64| over every case of this file 1.3e-7 on the total, 5.0e-8 on a tap;
the convolution alone at most 3.9 * 2^-24 * sum |a||w|.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

TOL = 1e-6
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
CONVS = ((64, 3, 11, 4, 2), (192, 64, 5, 1, 2), (384, 192, 3, 1, 1), (256, 384, 3, 1, 1), (256, 256, 3, 1, 1))   # Cout, Cin, k, stride, pad
SLICES = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
FEATURES = ("features.0", "features.3", "features.6", "features.8", "features.10")


# ------------------------------------------------------------------------------------------------ weights and the yardstick
@functools.lru_cache(maxsize=None)
def _state_dict(seed=0):
    """The lpips package's layout with synthetic weights: convolutions U(-1, 1) / sqrt(fan_in), biases U(-0.1, 0.1), lin weights U(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {"scaling_layer.shift": torch.tensor(SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(SCALE).view(1, 3, 1, 1)}
    for l, (name, (co, ci, k, _, _)) in enumerate(zip(SLICES, CONVS)):
        sd[f"{name}.weight"] = (torch.rand(co, ci, k, k, generator=g) * 2 - 1) / math.sqrt(ci * k * k)
        sd[f"{name}.bias"] = (torch.rand(co, generator=g) * 2 - 1) * 0.1
        sd[f"lin{l}.model.1.weight"] = torch.rand(1, co, 1, 1, generator=g)
        sd[f"lins.{l}.model.1.weight"] = sd[f"lin{l}.model.1.weight"]          # the package saves every lin layer twice
    return sd


def _net(x0, x1, dtype=torch.float64, operand=None):
    """LPIPS of x0 [N, 3, H, W] against x1 [1 | N, 3, H, W] (network inputs, fp64 tensors) -> (total [N], layers [5, N]) as fp64 numpy.  ``dtype``:
    the arithmetic; ``operand``: a narrower type the convolution operands are rounded to first (the bf16 implicit-GEMM model)."""
    sd = _state_dict()
    q = (lambda t: t) if operand is None else (lambda t: t.to(operand).to(dtype))
    shift, scale = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1), torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)

    def feats(x):
        h, taps = (x.to(dtype) - shift) / scale, []
        for l, (name, (_, _, _, stride, pad)) in enumerate(zip(SLICES, CONVS)):
            if l in (1, 2):
                h = F.max_pool2d(h, 3, 2)
            h = F.relu(F.conv2d(q(h), q(sd[f"{name}.weight"].to(dtype)), sd[f"{name}.bias"].to(dtype), stride=stride, padding=pad))
            taps.append(h)
        return taps

    layers = []
    for l, (f0, f1) in enumerate(zip(feats(x0), feats(x1))):
        n0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        lin = sd[f"lin{l}.model.1.weight"].to(dtype)
        layers.append((lin * (n0 - n1) ** 2).sum(1).mean((1, 2)))
    layers = torch.stack(layers)
    total = layers[0]
    for l in range(1, 5):
        total = total + layers[l]
    return total.double().numpy(), layers.double().numpy()


def _inputs(img, normalize):
    """uint8 NHWC or fp32 NCHW numpy -> the fp64 NCHW network input"""
    x = torch.from_numpy(img.astype(np.float64))
    x = x.permute(0, 3, 1, 2) / 255.0 if img.dtype == np.uint8 else x
    return 2 * x - 1 if normalize else x


# ------------------------------------------------------------------------------------------------ image families (as tests/test_metrics.py builds them)
def _smooth(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([127.5 + 100 * np.sin(x / 5.0 + ph) * np.cos(y / 7.0 + 2 * ph) for ph in (0.0, 0.7, 1.9)], axis=-1)


def _u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _family(name, H, W, N):
    """-> (img0 [N, H, W, 3], img1 [1 | N, H, W, 3]) uint8"""
    rng = np.random.default_rng(sum(map(ord, name)) + 1000 * H + W)
    if name == "noise":
        return _u8(rng.integers(0, 256, (N, H, W, 3))), _u8(rng.integers(0, 256, (N, H, W, 3)))
    if name == "smooth_noise":                       # smooth image + N(0, 0.02) and + N(0, 0.15) (of the [0, 1] range), one shared reference
        base = _smooth(H, W)
        sig = [0.02 * 255, 0.15 * 255, 0.05 * 255][:N]
        return np.stack([_u8(base + rng.normal(0, s, base.shape)) for s in sig]), _u8(base)[None]
    if name == "identical":
        a = _u8(rng.integers(0, 256, (N, H, W, 3)))
        return a, a.copy()
    if name == "dark_bright":
        return _u8(20 + rng.integers(-5, 6, (N, H, W, 3))), _u8(200 + rng.integers(-5, 6, (N, H, W, 3)))
    raise KeyError(name)


def _as_input(img_u8, kind):
    """uint8 NHWC stays; "f32": the same picture as fp32 NCHW in [0, 1]"""
    if kind == "u8":
        return img_u8
    return np.ascontiguousarray((img_u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))


@functools.lru_cache(maxsize=None)
def _want(name, H, W, N, kind, normalize):
    a, b = _family(name, H, W, N)
    a, b = _as_input(a, kind), _as_input(b, kind)
    return a, b, _net(_inputs(a, normalize), _inputs(b, normalize))


def _dev(a, backend):
    return torch.from_numpy(np.ascontiguousarray(a)).to(backend.device)


@functools.lru_cache(maxsize=None)
def _model():
    from pcdms_amd import metrics
    return metrics.LPIPS("alex").load_state_dict(_state_dict())


def _lpips(backend):
    """One model per test process (called after the ``backend`` fixture has installed a library): the packed weights are host tensors, the
    device copies are cached per device."""
    return _model()


def _check(backend, name, H, W, N, kind, normalize):
    a, b, (want, want_layers) = _want(name, H, W, N, kind, normalize)
    got, layers = _lpips(backend)(_dev(a, backend), _dev(b, backend), normalize=normalize, return_layers=True)
    backend.sync()
    assert got.dtype == torch.float32 and got.shape == (N, 1, 1, 1) and layers.shape == (5, N) and got.device.type == backend.device.type
    got, layers = got.cpu().numpy().astype(np.float64)[:, 0, 0, 0], layers.cpu().numpy().astype(np.float64)
    err, err_l = np.abs(got - want), np.abs(layers - want_layers)
    print(f"{name} {H}x{W} N={N} {kind} normalize={normalize}: device {got} fp64 {want} |err| total {err.max():.3e} per tap {err_l.max(1)}")
    assert np.isfinite(want).all() and (err <= TOL).all() and (err_l <= TOL).all(), (got, want, err, err_l)
    if name == "identical":
        assert (got == 0.0).all() and (layers == 0.0).all()
    else:
        assert (want > 1e-3).all(), "precondition: a non-identical pair is far from zero"
    return got


# ------------------------------------------------------------------------------------------------ the two models behind the tolerance
def test_yardstick_models():
    worst32, bf = 0.0, {}
    for name, H, W in (("noise", 35, 47), ("dark_bright", 35, 47), ("smooth_noise", 64, 48), ("noise", 31, 31)):
        for normalize in (False, True):
            a, b, (want, want_l) = _want(name, H, W, 2, "u8", normalize)
            x0, x1 = _inputs(a, normalize), _inputs(b, normalize)
            t32, l32 = _net(x0, x1, dtype=torch.float32)
            tbf, lbf = _net(x0, x1, operand=torch.bfloat16)
            worst32 = max(worst32, np.abs(t32 - want).max(), np.abs(l32 - want_l).max())
            bf[(name, H, normalize)] = np.abs(tbf - want).min()
    print(f"fp32 torch worst |err| {worst32:.3e}; bf16-operand model, smallest total |err| per case: {bf}")
    assert worst32 <= 1e-7
    for (name, _, _), e in bf.items():
        if name in ("noise", "dark_bright"):
            assert e > TOL, (name, e)


# ------------------------------------------------------------------------------------------------ accuracy
# 31x31: the minimum, conv3-5 run on ONE pixel (M tails of 1, 2, 3 rows); 35x47: odd sides, no multiple of a stride or a tile; N = 1, 2, 3
CASES = [("noise", 31, 31, 1, "u8", False), ("identical", 31, 31, 2, "u8", True), ("smooth_noise", 35, 47, 2, "u8", False),
         ("dark_bright", 35, 47, 1, "f32", True), ("noise", 64, 48, 2, "f32", False), ("dark_bright", 64, 48, 2, "u8", True)]


@pytest.mark.parametrize("name,H,W,N,kind,normalize", CASES)
def test_lpips_accuracy(backend, name, H, W, N, kind, normalize):
    _check(backend, name, H, W, N, kind, normalize)


@pytest.mark.gpu
@pytest.mark.parametrize("name,H,W,N,kind,normalize", [("noise", 256, 176, 3, "u8", False), ("smooth_noise", 256, 176, 3, "u8", True),
                                                       ("dark_bright", 256, 176, 2, "f32", False), ("identical", 256, 176, 3, "f32", True),
                                                       ("smooth_noise", 35, 47, 3, "f32", False), ("noise", 31, 31, 3, "u8", True)])
def test_lpips_accuracy_gpu_sizes(gpu_backend, name, H, W, N, kind, normalize):
    _check(gpu_backend, name, H, W, N, kind, normalize)


def test_window_into_canvas(backend):
    """the right half of a [source | target] canvas against a stand-alone target == the cropped images, bit for bit"""
    H, W, N = 33, 37, 2
    a, b = _family("smooth_noise", H, W, N)
    canvas = np.full((N, H + 5, 2 * W + 3, 3), 77, dtype=np.uint8)
    canvas[:, 2:2 + H, W + 1:2 * W + 1] = a
    m = _lpips(backend)
    got = m(_dev(canvas, backend), _dev(b, backend), cand_window=(W + 1, 2, W, H))
    crop = m(_dev(a, backend), _dev(b, backend))
    refwin = np.full((1, H + 4, W + 9, 3), 13, dtype=np.uint8)
    refwin[:, 4:, 3:3 + W] = b
    got2 = m(_dev(canvas, backend), _dev(refwin, backend), cand_window=(W + 1, 2, W, H), ref_window=(3, 4, W, H))
    backend.sync()
    assert torch.equal(got, crop) and torch.equal(got2, crop)
    want = _net(_inputs(a, False), _inputs(b, False))[0]
    assert (np.abs(got.cpu().numpy()[:, 0, 0, 0] - want) <= TOL).all()


# ------------------------------------------------------------------------------------------------ the convolution and the pool on their own
def _conv_check(backend, B, Hi, Wi, Cin, Cout, k, stride, pad, relu, seed):
    """|device - fp64| <= min(K, 8 sqrt(K)) 2^-24 (sum_k |a_k| |w_k| + |bias|) per output, K = k k Cin products.  K 2^-24 is the worst case of a
    chain of K fmaf (one rounding each, every partial sum bounded by sum |a||w|); 8 sqrt(K) is its random-walk counterpart with a margin of 8 for
    the maximum over ~1e5 outputs -- asserted as well because beyond K ~ 1000 the worst-case bound alone would also admit bf16 operands
    (2^-9 relative per product, ~2^-9 / sqrt(K) of sum |a||w| in total).  Measured: profiles/lpips_values.json."""
    from pcdms_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, Cin, Hi, Wi, generator=g) * 2 - 1
    w = (torch.rand(Cout, Cin, k, k, generator=g) * 2 - 1) / math.sqrt(Cin * k * k)
    bias = (torch.rand(Cout, generator=g) * 2 - 1) * 0.1
    pw = ops.pack_lpips_conv(w, bias, backend.device)
    cp = pw["cin"]
    assert cp == (Cin + 3) // 4 * 4
    xn = torch.zeros(B, Hi, Wi, cp)
    xn[..., :Cin] = x.permute(0, 2, 3, 1)
    got = ops.conv2d_f32(xn.to(backend.device), pw, stride=stride, pad=pad, relu=relu)
    backend.sync()
    want = F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=pad)
    mag = F.conv2d(x.double().abs(), w.double().abs(), bias.double().abs(), stride=stride, padding=pad)
    if relu:
        want = F.relu(want)
    got = got.cpu().double().permute(0, 3, 1, 2)
    assert got.shape == want.shape, (got.shape, want.shape)
    K = Cin * k * k
    ratio = ((got - want).abs() / mag).max().item() / 2.0 ** -24
    print(f"conv {k}x{k} s{stride} p{pad} Cin {Cin} Cout {Cout} out {tuple(want.shape)}: max |err| / (sum|a||w| 2^-24) = {ratio:.2f} (bound {min(K, 8 * math.sqrt(K)):.0f})")
    assert ratio <= min(K, 8 * math.sqrt(K))
    return got


@pytest.mark.parametrize("B,Hi,Wi,Cin,Cout,k,stride,pad", [
    (2, 31, 35, 3, 64, 11, 4, 2),      # conv1: Cin 3 padded to 4, K = 484 (not a multiple of 16), taps outside on every side
    (3, 7, 5, 64, 192, 5, 1, 2),       # conv2: Cout = 192, M = 105 (a 32-row tile cut after 9 rows)
    (1, 3, 4, 192, 72, 3, 1, 1),       # conv3's geometry with a Cout that is no multiple of 16: a cut 64-column tile AND a cut 16-column sub-tile
    (1, 3, 3, 8, 40, 3, 1, 0),         # output of 1 x 1 pixels: M = 1
    (5, 9, 9, 4, 16, 3, 2, 1),         # stride 2: M = 125, two waves of a workgroup, the rest idle
])
def test_conv_f32(backend, B, Hi, Wi, Cin, Cout, k, stride, pad):
    a = _conv_check(backend, B, Hi, Wi, Cin, Cout, k, stride, pad, True, seed=Cin + Cout)
    b = _conv_check(backend, B, Hi, Wi, Cin, Cout, k, stride, pad, True, seed=Cin + Cout)
    assert torch.equal(a, b)
    if Cout == 40:
        _conv_check(backend, B, Hi, Wi, Cin, Cout, k, stride, pad, False, seed=1)      # and without the ReLU


@pytest.mark.gpu
def test_conv_f32_many_tiles(gpu_backend):
    _conv_check(gpu_backend, 4, 27, 19, 64, 192, 5, 1, 2, True, seed=5)       # M = 2052: 17 workgroups, K = 1600
    _conv_check(gpu_backend, 2, 13, 11, 384, 256, 3, 1, 1, True, seed=6)      # K = 3456, the longest chain of the network


def test_maxpool_bit_exact(backend):
    from pcdms_amd import ops
    g = torch.Generator().manual_seed(3)
    for B, H, W, Cn in ((2, 7, 8, 64), (1, 3, 3, 192), (3, 15, 11, 4)):
        x = torch.randn(B, H, W, Cn, generator=g)
        got = ops.maxpool3s2_f32(x.to(backend.device))
        backend.sync()
        want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
        assert torch.equal(got.cpu(), want), (B, H, W, Cn)


# ------------------------------------------------------------------------------------------------ properties
def test_properties(backend):
    H, W, N = 33, 31, 2
    a, b = _family("noise", H, W, N)
    m = _lpips(backend)
    da, db = _dev(a, backend), _dev(b, backend)
    one, lay1 = m(da, db, return_layers=True)
    two, lay2 = m(da, db, return_layers=True)
    perm = m(_dev(a[::-1], backend), _dev(b[::-1], backend))
    swap = m(db, da)
    same = m(da, da.clone())
    first = m(da, db[:1])                                                      # reference batch 1: every candidate against b[0]
    backend.sync()
    assert torch.equal(one, two) and torch.equal(lay1, lay2)                   # reruns are bit-identical
    assert torch.equal(perm.flip(0), one)                                      # a batch permutation permutes the result, bit for bit
    assert (same == 0).all()                                                   # d(x, x) == 0
    assert (swap - one).abs().max().item() <= TOL                              # d(x, y) == d(y, x)
    want = _net(_inputs(a, False), _inputs(b[:1], False))[0]
    assert (np.abs(first.cpu().numpy()[:, 0, 0, 0] - want) <= TOL).all() and first[0].item() == one[0].item()


def test_refusals(backend):
    from pcdms_amd import metrics, ops
    m = _lpips(backend)
    ok = torch.zeros(1, 31, 31, 3, dtype=torch.uint8, device=backend.device)
    m(ok, ok)
    assert ops.lpips_ws_bytes(1, 1, 30, 31) == -1 and ops.lpips_ws_bytes(1, 1, 31, 30) == -1 and ops.lpips_ws_bytes(1, 1, 31, 31) > 0
    assert ops.lpips_ws_bytes(3, 2, 64, 64) == -1 and ops.lpips_ws_bytes(0, 1, 64, 64) == -1
    for shape in ((1, 30, 31, 3), (1, 31, 30, 3)):
        small = torch.zeros(shape, dtype=torch.uint8, device=backend.device)
        with pytest.raises(ValueError, match="31"):
            m(small, small)
    with pytest.raises(ValueError, match="31"):
        m(ok, ok, cand_window=(0, 0, 30, 31), ref_window=(0, 0, 30, 31))
    with pytest.raises(ValueError):
        m(ok, ok.float())                                                      # mixed types
    with pytest.raises(ValueError):
        m(torch.zeros(3, 31, 31, 3, dtype=torch.uint8), torch.zeros(2, 31, 31, 3, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        metrics.LPIPS("vgg")
    with pytest.raises(RuntimeError, match="no weights"):
        metrics.LPIPS()(ok, ok)
    # the library itself: -1 for sides of 30, a missing workspace, a window outside its image
    with pytest.raises(RuntimeError, match="code -1"):
        ops.lpips(ok, ok, (0, 0, 31, 31), (0, 0, 31, 31), m._weights(backend.device), torch.empty(1, device=backend.device), None, None,
                  torch.empty(2, dtype=torch.float64, device=backend.device), normalize=False)
    with pytest.raises(RuntimeError, match="code -1"):
        ops.lpips(ok, ok, (1, 0, 31, 31), (0, 0, 31, 31), m._weights(backend.device), torch.empty(1, device=backend.device), None, None,
                  torch.empty(1 << 20, dtype=torch.float64, device=backend.device), normalize=False)


def test_state_dict_layouts(backend, tmp_path):
    from pcdms_amd import metrics
    sd = dict(_state_dict())
    a = metrics.LPIPS().load_state_dict(sd)
    two_file = {f"{f}.{s}": sd[f"{n}.{s}"] for n, f in zip(SLICES, FEATURES) for s in ("weight", "bias")}
    two_file["classifier.1.weight"] = torch.zeros(4, 4)                        # torchvision's alexnet has more keys: ignored
    lin = {f"lin{l}.model.1.weight": sd[f"lin{l}.model.1.weight"] for l in range(5)}
    b = metrics.LPIPS().load_state_dict({**two_file, **lin})
    assert sorted(a.packed) == sorted(b.packed) and len(a.packed) == 15
    assert all(torch.equal(a.packed[k], b.packed[k]) for k in a.packed)
    # files: .pth of the package's layout, safetensors + .pth of the two-file form
    from safetensors.torch import save_file
    torch.save(sd, tmp_path / "alex_lpips.pth")
    save_file({k: v.contiguous() for k, v in two_file.items()}, str(tmp_path / "alexnet.safetensors"))
    torch.save(lin, tmp_path / "alex.pth")
    c = metrics.LPIPS.from_pretrained(tmp_path / "alex_lpips.pth")
    d = metrics.LPIPS.from_pretrained(tmp_path / "alexnet.safetensors", tmp_path / "alex.pth")
    assert all(torch.equal(a.packed[k], c.packed[k]) and torch.equal(a.packed[k], d.packed[k]) for k in a.packed)
    # wrong shapes and wrong constants
    bad = dict(sd)
    bad["net.slice2.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match="slice2"):
        metrics.LPIPS().load_state_dict(bad)
    bad = dict(sd)
    bad["lin3.model.1.weight"] = torch.zeros(1, 384, 1, 1)
    with pytest.raises(ValueError, match="lin3"):
        metrics.LPIPS().load_state_dict(bad)
    bad = dict(sd)
    bad["scaling_layer.scale"] = torch.tensor([.458, .448, .451]).view(1, 3, 1, 1)
    with pytest.raises(ValueError, match="scaling_layer.scale"):
        metrics.LPIPS().load_state_dict(bad)
    bad = dict(sd)
    del bad["net.slice5.10.bias"]
    with pytest.raises(KeyError):
        metrics.LPIPS().load_state_dict(bad)


# ------------------------------------------------------------------------------------------------ pick_best
def test_pick_best_lpips(backend):
    from pcdms_amd import metrics
    H, W = 35, 33
    rng = np.random.default_rng(21)
    base = _smooth(H, W)
    ref = _u8(base)[None]
    levels = [40.0, 25.0, 4.0, 60.0]                                           # a clear winner, not at index 0
    cand = np.stack([_u8(base + rng.normal(0, s, base.shape)) for s in levels])
    want = _net(_inputs(cand, False), _inputs(ref, False))[0]
    top = np.sort(want)
    assert top[1] - top[0] >= 1e-3 and int(np.argmin(want)) == 2
    m = _lpips(backend)
    img, idx, scores = metrics.pick_best(_dev(cand, backend), _dev(ref, backend), metric="lpips", lpips=m)
    backend.sync()
    assert idx.dtype == torch.int32 and idx.shape == (1,) and int(idx.cpu()) == int(np.argmin(want))
    assert (np.abs(scores.cpu().numpy() - want) <= TOL).all() and np.array_equal(img.cpu().numpy(), cand[2])
    tie = np.stack([cand[0], cand[2], cand[3], cand[2]])                       # two identical best candidates: the first wins
    img, idx, scores = metrics.pick_best(_dev(tie, backend), _dev(ref, backend), metric="lpips", lpips=m, out="normalized")
    s = scores.cpu().numpy()
    assert int(idx.cpu()) == 1 and s[1] == s[3] and img.shape == (1, 3, H, W)
    # the default is what it was: SSIM scores and np.argmax, no LPIPS involved
    img, idx, scores = metrics.pick_best(_dev(cand, backend), _dev(ref, backend))
    ss = metrics.ssim(_dev(cand, backend), _dev(ref, backend))
    backend.sync()
    assert torch.equal(scores, ss) and int(idx.cpu()) == int(np.argmax(ss.cpu().numpy())) and np.array_equal(img.cpu().numpy(), cand[int(idx.cpu())])
    with pytest.raises(ValueError):
        metrics.pick_best(_dev(cand, backend), _dev(ref, backend), metric="lpips")
    with pytest.raises(ValueError):
        metrics.pick_best(_dev(cand, backend), _dev(ref, backend), metric="fid")


# ------------------------------------------------------------------------------------------------ no host sync, no allocation inside the library
@pytest.mark.gpu
def test_lpips_graph_capture(gpu_backend):
    dev = gpu_backend.device
    a, b = _family("smooth_noise", 64, 48, 3)
    a2, _ = _family("noise", 64, 48, 3)
    m = _lpips(gpu_backend)
    x0, x1 = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    eager_a, eager_a2 = m(x0, x1).clone(), m(torch.from_numpy(a2).to(dev), x1).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(x0, x1)                                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m(x0, x1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_a)
    x0.copy_(torch.from_numpy(a2).to(dev))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_a2)


# ------------------------------------------------------------------------------------------------ the command-line tool
def test_score_pairs_tool(backend, tmp_path, capsys):
    from PIL import Image

    from pcdms_amd import metrics
    from tools import score_pairs
    H, W = 40, 36
    rng = np.random.default_rng(5)
    base = _smooth(H, W)
    gen = np.stack([_u8(base + rng.normal(0, s, base.shape)) for s in (5, 15, 30, 50)])
    gt = np.stack([_u8(base + rng.normal(0, 2, base.shape)) for _ in range(4)])
    (tmp_path / "gen").mkdir()
    (tmp_path / "gt").mkdir()
    for i in range(4):
        Image.fromarray(gen[i]).save(tmp_path / "gen" / f"{i:03d}.png")
        Image.fromarray(gt[i]).save(tmp_path / "gt" / f"{i:03d}.png")
    torch.save(dict(_state_dict()), tmp_path / "w.pth")
    res = score_pairs.main([str(tmp_path / "gen"), str(tmp_path / "gt"), "--lpips-weights", str(tmp_path / "w.pth"), "--batch", "3"],
                           device=backend.device)
    text = capsys.readouterr().out
    m = _lpips(backend)
    lp = m(_dev(gen, backend), _dev(gt, backend))[:, 0, 0, 0].cpu().numpy()
    ss = metrics.ssim(_dev(gen, backend), _dev(gt, backend)).cpu().numpy()
    ps = metrics.psnr(_dev(gen, backend), _dev(gt, backend)).cpu().numpy()
    assert np.array_equal(res["lpips"], lp) and np.array_equal(res["ssim_256"], ss) and np.array_equal(res["psnr"], ps)
    assert (np.abs(lp - _net(_inputs(gen, False), _inputs(gt, False))[0]) <= TOL).all()
    assert "PSNR: %.4f" % round(float(np.mean(ps)), 4) in text and "SSIM_256: %.4f" % round(float(np.mean(ss)), 4) in text
    assert "SSIM_256 Variance: %.4f" % round(float(np.var(ss)), 4) in text and "lpips: %.3f" % float(np.mean(lp)) in text
