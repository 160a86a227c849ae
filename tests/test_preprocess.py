"""Device-side input preparation (pcdms_amd/preprocess.py, csrc/image_prep.hip: pcdm_resample_u8 / pcdm_u8_to_nchw).

The yardsticks are the installed libraries the drivers call on the host: ``Image.resize(..., Image.BICUBIC)`` of Pillow, the drivers' own
``to_tensor_normalized`` and ``transformers.CLIPImageProcessor()``.  Pillow's 8-bit resampler is integer arithmetic, so the tolerance of every
resize check is zero bytes.  The two float conversions repeat the operation order of their host originals -- ``float32(p) / 255`` then
``(x - 0.5) / 0.5``; ``float32(float64(p) * (1 / 255))`` then ``(x - mean) / std`` in fp32, read from transformers' numpy ``rescale`` /
``normalize`` -- so they are held to bit equality as well (``torch.equal``), over all 256 x 3 possible inputs.

Kernel tests take the ``backend`` fixture: each runs under the lane emulator (sides <= 64 or so; the two-launch cases are long and thin) in the
CPU suite and on the MI355X under ``-m gpu``.
"""
from __future__ import annotations

import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image


def _load_driver(name):
    p = Path(__file__).resolve().parent.parent / "tools" / f"{name}.py"
    spec = importlib.util.spec_from_file_location(name, p)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pil_resize(x: np.ndarray, size) -> np.ndarray:
    img = Image.fromarray(x[..., 0] if x.shape[2] == 1 else x)
    y = np.asarray(img.resize(size, Image.BICUBIC))
    return y[..., None] if y.ndim == 2 else y


def _random(rng, H, W, C=3):
    return rng.integers(0, 256, (H, W, C), dtype=np.uint8)


def _saturated(H, W):
    """0 / 255 checkerboard (red), stripes two wide (green) and stripes three tall (blue): bicubic overshoots on every edge, so the clamp works"""
    y, x = np.mgrid[0:H, 0:W]
    return (np.stack([(x + y) % 2, (x // 2) % 2, (y // 3) % 2], axis=-1) * 255).astype(np.uint8)


def _dev(backend, a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(backend.device)


# (Ws, Hs) -> (Wd, Hd); the emulator's twins of the GPU's sizes stay small
RESIZE_CASES = {
    "down_noninteger": {"emu": ((47, 69), (22, 32)), "gpu": ((750, 1101), (352, 512))},
    "down_to_square": {"emu": ((47, 69), (32, 32)), "gpu": ((750, 1101), (512, 512))},
    "up": {"emu": ((22, 32), (44, 64)), "gpu": ((176, 256), (352, 512))},
    "mixed_x_up_y_down": {"emu": ((20, 60), (33, 25)), "gpu": ((200, 300), (301, 77))},
    "mixed_x_down_y_up": {"emu": ((60, 20), (25, 33)), "gpu": ((200, 300), (77, 301))},
    "identity_x": {"emu": ((33, 50), (33, 21)), "gpu": ((352, 700), (352, 512))},
    "identity_y": {"emu": ((50, 33), (21, 33)), "gpu": ((700, 512), (352, 512))},
    "identity_both": {"emu": ((35, 21), (35, 21)), "gpu": ((352, 512), (352, 512))},
    "side_1": {"emu": ((40, 30), (1, 1)), "gpu": ((40, 30), (1, 1))},
    "width_1": {"emu": ((40, 30), (1, 17)), "gpu": ((400, 300), (1, 170))},
    "height_1": {"emu": ((40, 30), (17, 1)), "gpu": ((400, 300), (170, 1))},
    "odd": {"emu": ((37, 53), (19, 31)), "gpu": ((373, 531), (191, 313))},
    "clip_224": {"emu": ((30, 40), (48, 64)), "gpu": ((30, 40), (224, 224))},
    # rows of one 16-row tile exceed the LDS budget: two launches through the workspace / one vertical launch / Pillow's vertical-first rule
    "two_launch": {"emu": ((8, 800), (5, 2)), "gpu": ((300, 6000), (123, 40))},
    "two_launch_vertical_only": {"emu": ((9, 700), (9, 3)), "gpu": ((300, 6000), (300, 40))},
    "tall_vertical_first": {"emu": ((6, 800), (4, 2)), "gpu": ((20, 4000), (13, 100))},
}


@pytest.mark.parametrize("case", sorted(RESIZE_CASES))
def test_resize_matches_pillow(backend, case):
    import pcdms_amd.preprocess as PP
    from pcdms_amd import ops
    (Ws, Hs), (Wd, Hd) = RESIZE_CASES[case][backend.name]
    if case == "two_launch":
        assert ops.resample_ws_bytes(Hs, Ws, Hd, Wd, 3, PP.coeff_table(Hs, Hd)[3]) == Hs * Wd * 3     # (the case does take the fallback)
    if case == "down_noninteger":
        assert ops.resample_ws_bytes(Hs, Ws, Hd, Wd, 3, PP.coeff_table(Hs, Hd)[3]) == 0
    rng = np.random.default_rng(sum(map(ord, case)))
    for x in (_random(rng, Hs, Ws), _saturated(Hs, Ws)):
        got = PP.resize(_dev(backend, x), (Wd, Hd)).cpu().numpy()
        ref = _pil_resize(x, (Wd, Hd))
        assert got.shape == ref.shape
        print(case, backend.name, "mismatching bytes:", int((got != ref).sum()))
        assert np.array_equal(got, ref)


def test_resize_one_channel(backend):
    import pcdms_amd.preprocess as PP
    rng = np.random.default_rng(5)
    x = _random(rng, 45, 31, 1)
    assert np.array_equal(PP.resize(_dev(backend, x), (20, 29)).cpu().numpy(), _pil_resize(x, (20, 29)))


def test_resize_pastes_into_window_only(backend):
    import pcdms_amd.preprocess as PP
    rng = np.random.default_rng(7)
    for (Ws, Hs), (Wd, Hd), (Wc, Hc), at in ((((47, 69), (22, 32), (50, 40), (5, 3))), ((21, 33), (21, 33), (64, 33), (43, 0)),
                                             ((8, 800), (5, 2), (9, 4), (3, 1)), ((30, 20), (33, 16), (66, 16), (33, 0))):
        x, before = _random(rng, Hs, Ws), _random(rng, Hc, Wc)
        canvas = _dev(backend, before)
        back = PP.resize(_dev(backend, x), (Wd, Hd), out=canvas, at=at)
        assert back is canvas
        want = before.copy()
        want[at[1]:at[1] + Hd, at[0]:at[0] + Wd] = _pil_resize(x, (Wd, Hd))
        assert np.array_equal(canvas.cpu().numpy(), want)     # the window is Pillow's, every other byte is what it was
    with pytest.raises(ValueError):
        PP.resize(_dev(backend, _random(rng, 8, 8)), (8, 8), out=_dev(backend, _random(rng, 8, 12)), at=(5, 0))


@pytest.mark.gpu
def test_resize_refuses_cpu_tensors_on_the_product_library(gpu_backend):
    import pcdms_amd.preprocess as PP
    with pytest.raises(RuntimeError):
        PP.resize(torch.zeros((8, 8, 3), dtype=torch.uint8), (4, 4))


@pytest.mark.parametrize("w_in,w_out", [(41, 17), (23, 52), (64, 9)])
def test_one_hot_rows_give_pillows_coefficients(backend, w_in, w_out):
    """A 1 x W row with a single 255 reads one column of the fixed-point table back: every position, three scale factors (down by a
    non-integer factor, up, down by about seven)."""
    import pcdms_amd.preprocess as PP
    if backend.name == "gpu":
        w_in, w_out = 4 * w_in + 1, 4 * w_out + 3
    bad = 0
    for pos in range(w_in):
        x = np.zeros((1, w_in, 3), dtype=np.uint8)
        x[0, pos] = 255
        got = PP.resize(_dev(backend, x), (w_out, 1)).cpu().numpy()
        bad += int((got != _pil_resize(x, (w_out, 1))).sum())
    assert bad == 0


def test_coeff_table_shape():
    """(no kernel) every row of a table sums to 2^22 within the rounding of its entries and stays inside the input"""
    import pcdms_amd.preprocess as PP
    for n_in, n_out in ((1101, 512), (176, 352), (30, 224), (800, 2)):
        lo, count, coeff, k = PP.coeff_table(n_in, n_out)
        assert len(lo) == len(count) == n_out and len(coeff) == n_out * k
        for o in range(n_out):
            assert 0 <= lo[o] and 0 < count[o] <= k and lo[o] + count[o] <= n_in
            assert abs(sum(coeff[o * k:o * k + count[o]]) - (1 << 22)) <= count[o] and not any(coeff[o * k + count[o]:(o + 1) * k])
    with pytest.raises(ValueError):
        PP.coeff_table(10, 5, "lanczos")


def _sizes(backend):
    """(source (w, h), pose (w, h), W, H)"""
    return ((47, 69), (40, 52), 24, 32) if backend.name == "emu" else ((750, 1101), (256, 256), 352, 512)


def test_stage2_inputs_match_the_drivers_host_path(backend):
    import pcdms_amd.preprocess as PP
    drv = _load_driver("stage2_batchtest_inpaint_model")
    (ws, hs), (wp, hp), W, H = _sizes(backend)
    rng = np.random.default_rng(11)
    s, sp, tp = _random(rng, hs, ws), _saturated(hp, wp), _random(rng, hp, wp)
    # the driver's host path (tools/stage2_batchtest_inpaint_model.py: load, the two canvases, to_tensor_normalized)
    load = lambda a: Image.fromarray(a).convert("RGB").resize((W, H), Image.BICUBIC)  # noqa: E731
    s_img, s_pose, t_pose = load(s), load(sp), load(tp)
    s_img_t_mask = Image.new("RGB", (2 * W, H))
    s_img_t_mask.paste(s_img, (0, 0))
    st_pose = Image.new("RGB", (2 * W, H))
    st_pose.paste(s_pose, (0, 0))
    st_pose.paste(t_pose, (W, 0))
    want_vae, want_pose = drv.to_tensor_normalized(s_img_t_mask).unsqueeze(0), drv.to_tensor_normalized(st_pose).unsqueeze(0)
    vae_image, st_pose_t, s_u8 = PP.stage2_inputs(_dev(backend, s), _dev(backend, sp), _dev(backend, tp), W, H)
    assert vae_image.dtype == torch.float32 and tuple(vae_image.shape) == (1, 3, H, 2 * W)
    assert torch.equal(vae_image.cpu(), want_vae)
    assert torch.equal(st_pose_t.cpu(), want_pose)
    assert np.array_equal(s_u8.cpu().numpy(), np.asarray(s_img))
    assert float(vae_image[..., W:].max()) == -1.0          # the right half is black


def test_stage3_inputs_match_the_drivers_host_path(backend):
    import pcdms_amd.preprocess as PP
    drv = _load_driver("stage3_batchtest_refined_model")
    (ws, hs), (wp, hp), W, H = _sizes(backend)
    rng = np.random.default_rng(12)
    s, g = _random(rng, hs, ws), _random(rng, hp, wp)
    load = lambda a: Image.fromarray(a).convert("RGB").resize((W, H), Image.BICUBIC)  # noqa: E731
    vae_gen, s_u8 = PP.stage3_inputs(_dev(backend, s), _dev(backend, g), W, H)
    assert torch.equal(vae_gen.cpu(), drv.to_tensor_normalized(load(g)).unsqueeze(0))
    assert np.array_equal(s_u8.cpu().numpy(), np.asarray(load(s)))


def test_to_tensor_normalized_all_bytes(backend):
    import pcdms_amd.preprocess as PP
    drv = _load_driver("stage2_batchtest_inpaint_model")
    x = np.stack([np.arange(256, dtype=np.uint8).reshape(16, 16)] * 3, axis=-1)
    assert torch.equal(PP.to_tensor_normalized(_dev(backend, x)).cpu(), drv.to_tensor_normalized(Image.fromarray(x)).unsqueeze(0))
    assert torch.equal(PP.to_tensor_normalized(_dev(backend, x), (3, 2, 7, 5)).cpu(),
                       drv.to_tensor_normalized(Image.fromarray(x[2:7, 3:10])).unsqueeze(0))


def _clip_processor():
    transformers = pytest.importorskip("transformers")
    return transformers.CLIPImageProcessor()


def test_clip_values_all_768_inputs(backend):
    """What is left after the resize is three fp32 operations on 256 x 3 possible (byte, channel) inputs: all of them, on a 224-sided image
    that the processor neither resizes nor crops, bit for bit."""
    import pcdms_amd.preprocess as PP
    proc = _clip_processor()
    x = np.zeros((224, 224, 3), dtype=np.uint8)
    x[:16, :16] = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    want = proc(images=Image.fromarray(x), return_tensors="pt").pixel_values
    got = PP.clip_pixel_values(_dev(backend, x)).cpu()
    print("max |device - processor| over the 768 inputs:", float((got - want).abs().max()))
    assert torch.equal(got, want)


@pytest.mark.parametrize("case", ["portrait", "landscape", "square", "short_side_224", "driver"])
def test_clip_pixel_values_match_the_processor(backend, case):
    import pcdms_amd.preprocess as PP
    proc = _clip_processor()
    w, h = {"portrait": (352, 512), "landscape": (301, 233), "square": (300, 300), "short_side_224": (224, 301), "driver": (512, 512)}[case]
    if backend.name == "emu":    # (the crop is 224 wide whatever comes in: smaller sources keep the horizontal pass short)
        w, h = {"portrait": (33, 48), "landscape": (45, 35), "square": (40, 40), "short_side_224": (224, 230), "driver": (64, 64)}[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    x = _random(rng, h, w)
    want = proc(images=Image.fromarray(x), return_tensors="pt").pixel_values
    got = PP.clip_pixel_values(_dev(backend, x)).cpu()
    assert got.shape == want.shape == (1, 3, 224, 224) and got.dtype == torch.float32
    print(case, backend.name, "max |device - processor|:", float((got - want).abs().max()))
    assert torch.equal(got, want)


def test_library_refuses_bad_arguments(backend):
    """-1 and nothing written: a table where the axis keeps its size (or none where it changes), channels other than 1 / 3, a window beyond the
    pitch, a missing workspace on the two-launch path, a window that leaves the image."""
    import pcdms_amd.preprocess as PP
    from pcdms_amd import ops
    dev = backend.device
    src = torch.zeros((20, 10, 3), dtype=torch.uint8, device=dev)
    dst = torch.full((10, 10, 3), 7, dtype=torch.uint8, device=dev)
    ytab, ky = PP._table(20, 10, "bicubic", dev)
    with pytest.raises(RuntimeError):
        ops.resample_u8(src, ytab, ky, ytab, ky, dst, (10, 10), (0, 0), None)       # x keeps its size but has a table
    with pytest.raises(RuntimeError):
        ops.resample_u8(src, None, 0, None, 0, dst, (10, 10), (0, 0), None)         # y changes and has none
    with pytest.raises(ValueError):
        ops.resample_u8(src, None, 0, ytab, ky, dst, (10, 10), (1, 0), None)        # leaves the canvas
    tall = torch.zeros((800, 8, 3), dtype=torch.uint8, device=dev)
    xt, kx = PP._table(8, 5, "bicubic", dev)
    yt, ky2 = PP._table(800, 2, "bicubic", dev)
    with pytest.raises(RuntimeError):
        ops.resample_u8(tall, xt, kx, yt, ky2, dst, (5, 2), (0, 0), None)           # two launches need the workspace
    assert ops.resample_ws_bytes(20, 10, 10, 10, 2, ky) == -1
    with pytest.raises(RuntimeError):
        ops.u8_to_nchw(src, (0, 0, 11, 20), torch.empty(3 * 11 * 20, device=dev), mode=0, scale=255.0, mean=(0.5,) * 3, std=(0.5,) * 3)
    assert bool((dst == 7).all())


@pytest.mark.gpu
def test_graph_replay(gpu_backend):
    """stage2_inputs + clip_pixel_values captured once (the tables of these sizes are cached by the eager warm-up), replayed after the input bytes
    are overwritten in place: nothing in the chain synchronises with the host, and the replay equals an eager call on the new bytes."""
    import pcdms_amd.preprocess as PP
    dev = gpu_backend.device
    rng = np.random.default_rng(21)
    W, H = 352, 512
    bufs = [torch.from_numpy(_random(rng, 1101, 750)).to(dev), torch.from_numpy(_random(rng, 256, 256)).to(dev),
            torch.from_numpy(_random(rng, 256, 256)).to(dev)]

    def chain():
        vae_image, st_pose, s_u8 = PP.stage2_inputs(bufs[0], bufs[1], bufs[2], W, H)
        return vae_image, st_pose, PP.clip_pixel_values(s_u8)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain()
    for b in bufs:
        b.copy_(torch.from_numpy(_random(rng, b.shape[0], b.shape[1])).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    want = chain()
    for got, ref in zip(outs, want):
        assert torch.equal(got, ref)
    # ... and the replayed values are the host path's
    proc = _clip_processor()
    s_img = Image.fromarray(bufs[0].cpu().numpy()).resize((W, H), Image.BICUBIC)
    assert torch.equal(outs[2].cpu(), proc(images=s_img, return_tensors="pt").pixel_values)


def _fabricate_stage2(tmp_path, names=("a", "b", "c")):
    """Tiny checkpoints and data in the layouts the stage-2 driver reads, as tests/test_driver_stage2.py fabricates them; the images on disk
    are 90 x 150 and the driver runs at 64 x 128, so the resize is really exercised.  -> (driver module, common arguments, pairs, W, H)"""
    import json

    from oracle import cond as OC
    from oracle import vae as OV
    from oracle.unet import UNetConfig, synth_state_dict
    from safetensors.torch import save_file
    from tests.test_driver_stage2 import _load_driver as load_driver
    from tests.test_encoders import TINY, _hf, _hf_clip
    from tests.test_from_pretrained import SD21_UNET_JSON
    drv = load_driver()
    sd21 = tmp_path / "sd21"
    for sub in ("unet", "vae", "scheduler"):
        (sd21 / sub).mkdir(parents=True)
    (sd21 / "unet" / "config.json").write_text(json.dumps(SD21_UNET_JSON))
    stock = UNetConfig.tiny(in_channels=4, class_embed_type=None, projection_class_embeddings_input_dim=None)
    save_file({k: v.contiguous() for k, v in synth_state_dict(stock, seed=1).items()}, str(sd21 / "unet" / "diffusion_pytorch_model.safetensors"))
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
    module = {"unet." + k: v for k, v in synth_state_dict(ucfg, seed=5, random_affine=True).items()}
    module.update({"pose_proj." + k: v for k, v in OC.synth(OC.pose_param_shapes(ucfg.block_out_channels[0], 3, (16, 32, 96, 256)), 6).items()})
    module.update({"image_proj_model_p." + k: v for k, v in OC.synth(OC.image_proj_param_shapes(128, 64, ucfg.cross_attention_dim), 7, 1.0).items()})
    (tmp_path / "ckpt").mkdir()
    torch.save({"module": module}, tmp_path / "ckpt" / "mp_rank_00_model_states.pt")
    rng = np.random.default_rng(0)
    for d in ("img", "pose", "embed"):
        (tmp_path / d).mkdir()
    for n in names:
        Image.fromarray(rng.integers(0, 255, (150, 90, 3), dtype=np.uint8)).save(tmp_path / "img" / f"{n}.png")
        Image.fromarray(rng.integers(0, 255, (150, 90, 3), dtype=np.uint8)).save(tmp_path / "pose" / f"{n}_pose.jpg")
    pairs = [{"source_image": f"{s}.jpg", "target_image": f"{t}.jpg"} for s, t in zip(names[:-1], names[1:])]
    for p in pairs:
        np.save(tmp_path / "embed" / (p["source_image"].replace(".jpg", "_to_") + p["target_image"].replace(".jpg", ".npy")),
                rng.standard_normal((1, 64)).astype(np.float32) * 0.4)
    W, H = 64, 128
    common = ["--pretrained_model_name_or_path", str(sd21), "--image_encoder_g_path", str(tmp_path / "clip"), "--image_encoder_p_path",
              str(tmp_path / "dinov2"), "--img_path", str(tmp_path / "img") + "/", "--pose_path", str(tmp_path / "pose") + "/",
              "--target_embed_path", str(tmp_path / "embed") + "/", "--num_inference_steps", "3", "--img_width", str(W), "--img_height", str(H),
              "--weights_name", str(tmp_path / "ckpt"), "--calculate_metrics", "--metrics_device", "gpu"]
    return drv, common, pairs, W, H


@pytest.mark.gpu
def test_stage2_driver_gpu_preprocess_writes_the_same_files(gpu_backend, tmp_path):
    """The stage-2 driver on fabricated tiny checkpoints, ``--preprocess_device host`` against ``gpu``, same seed, both with
    ``--calculate_metrics --metrics_device gpu``: byte-identical PNGs and the same best indices, in the ``test`` json mode (stage-1 embeddings
    from disk) and the ``train`` mode (CLIP pixels of the target too)."""
    pytest.importorskip("transformers")
    import json
    drv, common, pairs, W, H = _fabricate_stage2(tmp_path)
    assert Image.open(tmp_path / "img" / "a.png").size != (W, H)
    for split in ("test", "train"):
        (tmp_path / f"{split}_data.json").write_text(json.dumps(pairs))
        files, logs = {}, {}
        for where in ("host", "gpu"):
            args = drv.build_parser().parse_args(common + ["--save_path", str(tmp_path / f"out_{split}_{where}"), "--json_path",
                                                           str(tmp_path / f"{split}_data.json"), "--preprocess_device", where])
            del drv.BEST_INDEX_LOG[:]
            drv.inference(args, 0, pairs)
            logs[where] = list(drv.BEST_INDEX_LOG)
            out = tmp_path / f"out_{split}_{where}" / "guidancescale2.0_seed42_numsteps3"
            files[where] = {f.name: f.read_bytes() for f in sorted(out.glob("*.png"))}
        assert sorted(files["host"]) == ["a_to_b.png", "b_to_c.png"]
        assert files["gpu"] == files["host"]
        assert logs["gpu"] == logs["host"] and len(logs["host"]) == 2
    assert drv.build_parser().parse_args([]).preprocess_device == "host"
