#!/usr/bin/env python3
"""The reference's stage-2 evaluation driver on pcdms_amd, file formats and flags unchanged.

Same command line, checkpoint layout and outputs as /root/reference/stage2_batchtest_inpaint_model.py (flags :242-262, model
loading :95-133, per-pair conditioning :141-186, sampling call :188-200, best-SSIM / grid output :203-232, one process per GPU
over ``split_list_into_chunks`` :266-285); every model object is the pcdms_amd one, so the whole driver -- encoders, pose
embedding, VAE, UNet, scheduler -- runs on the MI355X through libpcdm.so.  What stays host-side is what the reference does
on the host too: PIL resize / canvas pasting, ``CLIPImageProcessor``, PNG writing, SSIM -- unless ``--metrics_device gpu`` is given: then the samples
stay on the device as uint8, ``pcdms_amd.metrics.pick_best`` scores and selects there, and only the chosen image and the scores come back.
With ``--preprocess_device gpu`` the input side moves as well: the decoded pixels of each image are uploaded once as uint8 and
``pcdms_amd.preprocess`` resizes, pastes, normalises and forms the CLIP pixels on the device -- the same bytes, so the same PNGs and best indices.
With ``--pose_source keypoints`` the pose maps are not read as images: ``<pose name>.npz`` (keypoints, scores, size: tools/README.md) next to where
the pose image would be is rendered on the device by ``pcdms_amd.pose.draw_pose`` -- the pixels tools/render_pose.py writes for that file.
With ``--pose_source estimator --pose_weights CKPT`` no pose file is read at all: the pose map of each source / target IMAGE is estimated on the
device by ``pcdms_amd.pose.estimate_pose_map`` (DWPose-l from the mmpose checkpoint CKPT; the whole image is the person box: tools/README.md --
or, with ``--pose_det_weights CKPT``, the boxes of the person detector, YOLOX-l from the mmdet checkpoint, as in the reference;
``--pose_frame_resize reference`` makes the detection frame with the reference's ``resize_image`` instead of Pillow bicubic).
That map is estimated from the picture as it lies on disk with detect_resolution = image_resolution = 512 and then resized to the driver's size
like a pose file; it is NOT the file tools/extract_pose.py writes, which follows the reference's ``single_extract_pose.py`` (the picture resized to
1024 x 1024 first, image_resolution 1024).  A pair's maps are estimated again where the driver reads a pose file again (the grid's thumbnails).

Differences, on purpose: ``--img_width`` is honoured (the reference parses it but reads ``args.img_weigh``); ``ImageProjModel_p``
takes its sizes from the checkpoint / encoder config instead of the literals 1536 / 768 / 1024 (identical for the published
checkpoints); SSIM is a numpy restatement of ``skimage.metrics.structural_similarity`` with the driver's arguments (skimage is not
in the image); per-rank work is the reference's block partition.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.multiprocessing as mp
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import pcdms_amd as P  # noqa: E402


def to_tensor_normalized(img: Image.Image) -> torch.Tensor:
    """transforms.Compose([ToTensor(), Normalize([0.5], [0.5])]) (:86-89)."""
    x = torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1)
    return (x - 0.5) / 0.5


def ssim_gaussian(a: np.ndarray, b: np.ndarray, sigma: float = 1.2) -> float:
    """skimage.metrics.structural_similarity(a, b, gaussian_weights=True, sigma=1.2, use_sample_covariance=False, channel_axis=2,
    data_range=b.max() - b.min()) as the driver calls it (:206-211), restated."""
    from scipy.ndimage import gaussian_filter
    a, b = a.astype(np.float64), b.astype(np.float64)
    R = b.max() - b.min()
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    pad = (2 * int(3.5 * sigma + 0.5) + 1 - 1) // 2
    vals = []
    for ch in range(a.shape[2]):
        x, y = a[..., ch], b[..., ch]
        f = lambda z: gaussian_filter(z, sigma, truncate=3.5, mode="reflect")  # noqa: E731
        ux, uy = f(x), f(y)
        vx, vy, vxy = f(x * x) - ux * ux, f(y * y) - uy * uy, f(x * y) - ux * uy
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        vals.append(s[pad:-pad, pad:-pad].mean())
    return float(np.mean(vals))


BEST_INDEX_LOG: list = []   # (output name, index of the saved sample) of every --calculate_metrics pair this process scored


def pick_best_on_device(images: torch.Tensor, t_img: Image.Image, window=None):
    """``--metrics_device gpu``: the uint8 NHWC samples stay on the device, the target is uploaded once, pcdms_amd.metrics.pick_best scores the
    window of every sample and selects the best; only the chosen image, its index and the N scores come back.  ``t_img`` is a PIL image or a uint8
    [H, W, 3] tensor on the samples' device.  Returns (PIL image, index, [scores])."""
    target = t_img if isinstance(t_img, torch.Tensor) else torch.from_numpy(np.array(t_img)).to(images.device)   # (already there: --preprocess_device gpu)
    image, index, scores = P.pick_best(images, target, cand_window=window)
    return Image.fromarray(image.cpu().numpy()), int(index.item()), [float(v) for v in scores.tolist()]


def load_detector(args):
    """``--pose_det_weights``: the person detector for ``--pose_source estimator`` (None without the flag: the whole picture is the person box)"""
    if not getattr(args, "pose_det_weights", None):
        return None
    return P.PersonDetector.from_checkpoint(args.pose_det_weights, size=getattr(args, "pose_det_size", 640),
                                            widen_factor=getattr(args, "pose_det_widen_factor", 1.0),
                                            deepen_factor=getattr(args, "pose_det_deepen_factor", 1.0),
                                            num_classes=getattr(args, "pose_det_num_classes", 80))


def load_pose(path: str, source: str, device, on_device: bool, image_path: str = None, estimator=None, detector=None, frame_resize: str = "pillow"):
    """The pose map the driver reads at ``path``, not yet resized: decoded from the image file (``source`` "image"), rendered on ``device`` from
    the keypoint file of the same name with the extension .npz ("keypoints"), or estimated on ``device`` from the picture at ``image_path`` by
    ``estimator`` ("estimator"; with ``detector`` the person boxes come from it, else the box is the whole picture; ``frame_resize``: how the
    detection frame is made, ``--pose_frame_resize``).  A uint8 [h, w, 3] tensor on
    ``device`` (``on_device``) or a PIL image."""
    if source == "estimator":
        pose = P.estimate_pose_map(estimator, torch.from_numpy(np.array(Image.open(image_path).convert("RGB"))).to(device), detector=detector,
                                   frame_resize=frame_resize)
        return pose if on_device else Image.fromarray(pose.cpu().numpy())
    if source == "keypoints":
        with np.load(os.path.splitext(path)[0] + ".npz") as f:
            kp, sc, (w, h) = torch.from_numpy(f["keypoints"].astype(np.float32)), torch.from_numpy(f["scores"].astype(np.float32)), (int(v) for v in f["size"])
        pose = P.draw_pose(kp.to(device), sc.to(device), (h, w))[0]
        return pose if on_device else Image.fromarray(pose.cpu().numpy())
    img = Image.open(path).convert("RGB")
    return torch.from_numpy(np.array(img)).to(device) if on_device else img


def image_grid(imgs, rows, cols):
    w, h = imgs[0].size
    grid = Image.new("RGB", size=(cols * w, rows * h))
    for i, img in enumerate(imgs):
        grid.paste(img, box=(i % cols * w, i // cols * h))
    return grid


def inference(args, rank, select_test_datas):
    from transformers import CLIPImageProcessor
    device = torch.device(f"cuda:{rank}")
    torch.cuda.set_device(device)
    generator = torch.Generator(device=device).manual_seed(args.seed_number)
    tag = "guidancescale{}_seed{}_numsteps{}/".format(args.guidance_scale, args.seed_number, args.num_inference_steps)
    save_dir, save_dir_metric = f"{args.save_path}/show_{tag}", f"{args.save_path}/{tag}"
    os.makedirs(save_dir, exist_ok=True)
    os.makedirs(save_dir_metric, exist_ok=True)
    clip_image_processor = CLIPImageProcessor()

    # ---- models (:95-133)
    image_encoder_g = P.CLIPVisionModelWithProjection.from_pretrained(args.image_encoder_g_path).to(device).eval()
    image_encoder_p = P.Dinov2Model.from_pretrained(args.image_encoder_p_path).to(device).eval()
    model_sd = torch.load("{}/mp_rank_00_model_states.pt".format(args.weights_name), map_location="cpu")["module"]
    pose_proj_dict, image_proj_dict, unet_dict = {}, {}, {}
    for k, v in model_sd.items():
        if k.startswith("pose_proj"):
            pose_proj_dict[k.replace("pose_proj.", "")] = v
        elif k.startswith("image_proj_model_p"):
            image_proj_dict[k.replace("image_proj_model_p.", "")] = v
        elif k.startswith("unet"):
            unet_dict[k.replace("unet.", "")] = v
        else:
            print(k)
    hid, in_dim = image_proj_dict["net.0.weight"].shape
    image_proj_model_p = P.ImageProjModel_p(in_dim=in_dim, hidden_dim=hid, out_dim=image_proj_dict["net.4.weight"].shape[0]).to(device).eval()
    pose_proj = P.ControlNetConditioningEmbedding(pose_proj_dict["conv_out.weight"].shape[0], 3, (16, 32, 96, 256)).to(device).eval()
    pose_proj.load_state_dict(pose_proj_dict)
    image_proj_model_p.load_state_dict(image_proj_dict)

    pipe = P.Stage2_InpaintDiffusionPipeline.from_pretrained(args.pretrained_model_name_or_path, torch_dtype=torch.float16).to(device)
    pipe.unet = P.Stage2_InapintUNet2DConditionModel.from_pretrained(
        args.pretrained_model_name_or_path, subfolder="unet", in_channels=9, class_embed_type="projection",
        projection_class_embeddings_input_dim=unet_dict["class_embedding.linear_1.weight"].shape[1], torch_dtype=torch.float16,
        low_cpu_mem_usage=False, ignore_mismatched_sizes=True).to(device)
    pipe.unet.load_state_dict(unet_dict)
    if getattr(args, "freeu", None):   # opt-in (no reference counterpart in this driver): pipe.enable_freeu(s1, s2, b1, b2)
        pipe.enable_freeu(*args.freeu)
    scheduler = getattr(args, "scheduler", "unipc")
    simple = {"ddim": P.DDIMScheduler, "euler": P.EulerDiscreteScheduler, "euler_a": P.EulerAncestralDiscreteScheduler,
              "lms": P.LMSDiscreteScheduler, "pndm": P.PNDMScheduler}
    if scheduler == "unipc":   # the reference driver's choice
        pipe.scheduler = P.UniPCMultistepScheduler.from_config(pipe.scheduler.config)
    elif scheduler in simple:  # the other members of the reference's scheduler slot (src/pipelines/stage2_inpaint_pipeline.py:547-558)
        pipe.scheduler = simple[scheduler].from_config(pipe.scheduler.config)
    else:                      # DPM++ 2M ("dpmpp"), its Karras-sigma and SDE forms
        pipe.scheduler = P.DPMSolverMultistepScheduler.from_config(
            pipe.scheduler.config, use_karras_sigmas=scheduler == "dpmpp_2m_karras",
            algorithm_type="sde-dpmsolver++" if scheduler == "dpmpp_2m_sde" else "dpmsolver++")
    pipe.enable_xformers_memory_efficient_attention()
    print("====================== json_data: {}, model load finish ===================".format(args.json_path.split("/")[-1]))

    W, H = args.img_width, args.img_height
    pre_gpu = getattr(args, "preprocess_device", "host") == "gpu"
    pose_source = getattr(args, "pose_source", "image")
    estimator = None
    if pose_source == "estimator":
        if not getattr(args, "pose_weights", None):
            raise ValueError("--pose_source estimator needs --pose_weights (the mmpose DWPose-l checkpoint)")
        estimator = P.DWPoseEstimator.from_checkpoint(args.pose_weights, input_size=tuple(getattr(args, "pose_input_size", (288, 384))),
                                                      widen_factor=getattr(args, "pose_widen_factor", 1.0),
                                                      deepen_factor=getattr(args, "pose_deepen_factor", 1.0))
    detector = load_detector(args) if pose_source == "estimator" else None
    all_ssim = []
    start_time = time.time()
    split = args.json_path.split("/")[-1].split("_")[0]
    for data in select_test_datas:
        s_img_path = args.img_path + data["source_image"].replace(".jpg", ".png")
        t_img_path = args.img_path + data["target_image"].replace(".jpg", ".png")
        s_pose_path = args.pose_path + data["source_image"].replace(".jpg", "_pose.jpg")
        t_pose_path = args.pose_path + data["target_image"].replace(".jpg", "_pose.jpg")
        t_img_dev = None
        load = lambda p: Image.open(p).convert("RGB").resize((W, H), Image.BICUBIC)  # noqa: E731
        pose_of = lambda p, img, dev: load_pose(p, pose_source, device, dev, img, estimator, detector,  # noqa: E731
                                                getattr(args, "pose_frame_resize", "pillow"))
        load_p = lambda p, img: pose_of(p, img, False).resize((W, H), Image.BICUBIC)  # noqa: E731
        if pre_gpu:      # decode on the host, upload the raw pixels once per image, everything else on the device (pcdms_amd/preprocess.py)
            raw = lambda p: torch.from_numpy(np.array(Image.open(p).convert("RGB"))).to(device)  # noqa: E731
            vae_image, st_pose_t, s_img_u8 = P.stage2_inputs(raw(s_img_path), pose_of(s_pose_path, s_img_path, True),
                                                            pose_of(t_pose_path, t_img_path, True), W, H)
            t_img_dev = P.resize(raw(t_img_path), (W, H))    # also what --metrics_device gpu scores against
            pix = P.clip_pixel_values(s_img_u8)
        else:
            s_img, t_img, s_pose, t_pose = load(s_img_path), load(t_img_path), load_p(s_pose_path, s_img_path), load_p(t_pose_path, t_img_path)
            s_img_t_mask = Image.new("RGB", (2 * W, H))          # [source | black]
            s_img_t_mask.paste(s_img, (0, 0))
            st_pose = Image.new("RGB", (2 * W, H))               # [source pose | target pose]
            st_pose.paste(s_pose, (0, 0))
            st_pose.paste(t_pose, (W, 0))
            pix = clip_image_processor(images=s_img, return_tensors="pt").pixel_values
            vae_image = to_tensor_normalized(s_img_t_mask).unsqueeze(0)
            st_pose_t = to_tensor_normalized(st_pose).unsqueeze(0)
        s_img_proj_f = image_proj_model_p(image_encoder_p(pix.to(device)).last_hidden_state)
        st_pose_f = pose_proj(st_pose_t.to(device))
        if split == "train":
            pix_t = P.clip_pixel_values(t_img_dev) if pre_gpu else clip_image_processor(images=t_img, return_tensors="pt").pixel_values
            pred_t_img_embed = image_encoder_g(pix_t.to(device)).image_embeds.unsqueeze(1)
        elif split == "test":
            name = s_img_path.split("/")[-1].replace(".png", "_to_") + t_img_path.split("/")[-1].replace(".png", ".npy")
            pred_t_img_embed = torch.tensor(np.load(args.target_embed_path + name)).to(device).unsqueeze(1)
        else:
            raise ValueError("Check the input JSON file path")

        on_device = args.calculate_metrics and getattr(args, "metrics_device", "host") == "gpu"
        if pre_gpu and not on_device:      # the host scorer and the grid take PIL images: the device's bytes, brought back
            t_img = Image.fromarray(t_img_dev.cpu().numpy())
            if not args.calculate_metrics:   # (the grid's thumbnails; the pose halves are not kept as uint8 on the device)
                s_img, s_pose, t_pose = Image.fromarray(s_img_u8.cpu().numpy()), load_p(s_pose_path, s_img_path), load_p(t_pose_path, t_img_path)
        output = pipe(height=H, width=2 * W, guidance_rescale=0.0, vae_image=vae_image, s_img_proj_f=s_img_proj_f, st_pose_f=st_pose_f,
                      pred_t_img_embed=pred_t_img_embed, num_images_per_prompt=4, guidance_scale=args.guidance_scale, generator=generator,
                      num_inference_steps=args.num_inference_steps, **({"output_type": "uint8"} if on_device else {}))
        out_name = s_img_path.split("/")[-1].replace(".png", "") + "_to_" + t_img_path.split("/")[-1]
        if on_device:      # the target half of each [source | generated] canvas against the target, scored where the decoder left it
            best_img, best, ssim_values = pick_best_on_device(output.images, t_img_dev if pre_gpu else t_img, (W, 0, W, H))
            all_ssim.append(ssim_values[best])
            BEST_INDEX_LOG.append((out_name, best))
            best_img.save(save_dir_metric + out_name)
        elif args.calculate_metrics:
            ssim_values = []
            for gen_img in output.images:
                gen = np.array(gen_img.crop((W, 0, 2 * W, H))) * 255.0
                ssim_values.append(ssim_gaussian(np.array(t_img) * 255.0, gen))
            best = int(np.argmax(ssim_values))
            all_ssim.append(ssim_values[best])
            BEST_INDEX_LOG.append((out_name, best))
            output.images[best].crop((W, 0, 2 * W, H)).save(save_dir_metric + out_name)
        else:
            vis_pose = Image.new("RGB", (2 * W, H))
            vis_pose.paste(s_pose, (0, 0))
            vis_pose.paste(t_pose, (W, 0))
            vis_img = Image.new("RGB", (2 * W, H))
            vis_img.paste(s_img, (0, 0))
            vis_img.paste(t_img, (W, 0))
            image_grid([vis_img, vis_pose] + list(output.images), 2, 3).save(save_dir + out_name)
    print(time.time() - start_time)
    if args.calculate_metrics and all_ssim:
        print(sum(all_ssim) / len(all_ssim))
    return all_ssim


def _guidance(s: str):
    """The reference declares ``type=int, default=2.0``: the untouched default formats as ``guidancescale2.0`` and an explicit
    ``--guidance_scale 2`` as ``guidancescale2`` (which is what the stage-3 driver's default ``--gen_t_img_path`` expects).  Same
    here; non-integer values (an argparse error in the reference) are accepted as floats."""
    try:
        return int(s)
    except ValueError:
        return float(s)


def build_parser():
    p = argparse.ArgumentParser(description="Stage-2 inpaint evaluation driver (reference flags) on pcdms_amd.")
    p.add_argument("--pretrained_model_name_or_path", type=str, default="./stable-diffusion-2-1-base")
    p.add_argument("--image_encoder_g_path", type=str, default="./OpenCLIP-ViT-H-14")
    p.add_argument("--image_encoder_p_path", type=str, default="./dinov2-giant")
    p.add_argument("--img_path", type=str, default="./datasets/deepfashing/train_all_png/")
    p.add_argument("--pose_path", type=str, default="./datasets/deepfashing/openpose_all_img/")
    p.add_argument("--json_path", type=str, default="./datasets/deepfashing/test_data.json")
    p.add_argument("--target_embed_path", type=str, default="./save_data/stage1/guidancescale0_seed42_numsteps20/")
    p.add_argument("--save_path", type=str, default="./save_data/stage2")
    p.add_argument("--guidance_scale", type=_guidance, default=2.0)   # ref: type=int, default=2.0 => "2.0" by default, "2" when given
    p.add_argument("--seed_number", type=int, default=42)
    p.add_argument("--num_inference_steps", type=int, default=20)
    p.add_argument("--img_width", type=int, default=512)
    p.add_argument("--img_height", type=int, default=512)
    p.add_argument("--calculate_metrics", action="store_true")
    p.add_argument("--metrics_device", choices=("host", "gpu"), default="host",
                   help="where --calculate_metrics scores the samples: host (scipy, as the reference) or gpu (pcdms_amd.metrics.pick_best)")
    p.add_argument("--preprocess_device", choices=("host", "gpu"), default="host",
                   help="where the inputs are resized, pasted, normalised and turned into CLIP pixels: host (PIL / CLIPImageProcessor, as the "
                        "reference) or gpu (pcdms_amd.preprocess, the same bytes)")
    p.add_argument("--pose_source", choices=("image", "keypoints", "estimator"), default="image",
                   help="where the pose maps come from: image (the pose image files, as the reference), keypoints (<pose name>.npz next to them, "
                        "rendered on the device by pcdms_amd.pose) or estimator (estimated on the device from the source / target images with "
                        "--pose_weights; no pose file is read)")
    p.add_argument("--pose_weights", type=str, default=None, help="the mmpose DWPose-l checkpoint (dw-ll_ucoco_384.pth) for --pose_source estimator")
    p.add_argument("--pose_input_size", type=int, nargs=2, default=(288, 384), metavar=("W", "H"), help="crop size of the --pose_weights network")
    p.add_argument("--pose_widen_factor", type=float, default=1.0, help="CSPNeXt widen_factor of --pose_weights (DWPose-l: 1)")
    p.add_argument("--pose_deepen_factor", type=float, default=1.0, help="CSPNeXt deepen_factor of --pose_weights (DWPose-l: 1)")
    p.add_argument("--pose_frame_resize", choices=("pillow", "reference"), default="pillow",
                   help="--pose_source estimator: the detection frame by Pillow bicubic (default) or by the reference's resize_image (cv2 Lanczos4 / area)")
    p.add_argument("--pose_det_weights", type=str, default=None,
                   help="the mmdet YOLOX-l checkpoint for --pose_source estimator: person boxes from the detector (default: the whole picture)")
    p.add_argument("--pose_det_size", type=int, default=640, help="square input size of the --pose_det_weights network (YOLOX-l: 640)")
    p.add_argument("--pose_det_widen_factor", type=float, default=1.0, help="widen_factor of --pose_det_weights (YOLOX-l: 1)")
    p.add_argument("--pose_det_deepen_factor", type=float, default=1.0, help="deepen_factor of --pose_det_weights (YOLOX-l: 1)")
    p.add_argument("--pose_det_num_classes", type=int, default=80, help="classes of --pose_det_weights (COCO: 80; class 0 is the person)")
    p.add_argument("--scheduler", choices=("unipc", "ddim", "dpmpp", "dpmpp_2m", "dpmpp_2m_karras", "dpmpp_2m_sde", "euler", "euler_a", "lms", "pndm"),
                   default="unipc")
    p.add_argument("--freeu", type=float, nargs=4, default=None, metavar=("S1", "S2", "B1", "B2"),
                   help="FreeU in the two lowest-resolution decoder blocks (pipe.enable_freeu; e.g. 0.9 0.2 1.2 1.4); default: off")
    p.add_argument("--weights_name", type=str, default="./Checkpoints/stage2_checkpoints/512")
    return p


if __name__ == "__main__":
    args = build_parser().parse_args()
    print(args)
    num_devices = torch.cuda.device_count()
    print("using {} num_processes inference".format(num_devices))
    datas = json.load(open(args.json_path))
    print(len(datas))
    mp.set_start_method("spawn")
    chunks = P.split_list_into_chunks(datas, num_devices)
    procs = [mp.Process(target=inference, args=(args, r, chunks[r])) for r in range(num_devices)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join()
