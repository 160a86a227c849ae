"""The reference's ``caculate_metrics_256.py`` / ``caculate_metrics_512.py`` as one tool, computed on the device: every image goes through
OpenCV's ``INTER_CUBIC`` float resize to ``--size`` and ``/ 255.0`` first (``pcdms_amd.preprocess.resize_cv_cubic``), then the pairs are scored
with PSNR, the 51 x 51 uniform-window SSIM, the Gaussian ``ssim_256``, MAE and L1 (``Reconstruction_Metrics.calculate_from_disk``), LPIPS
(``LPIPS.calculate_from_disk``) and the generated set against a real set with FID (``FID.calculate_from_disk``).

    python tools/calculate_metrics.py GENERATED_DIR GT_DIR --size W H [--real REAL_DIR|STATS.npz --fid-weights inception_v3.pth]
                                      [--lpips-weights alex_lpips.pth [--lpips-lin alex.pth]] [--save-dir DIR] [--reference-remainders]

Pairing is the reference's ``preprocess_path_for_deform_task``: for every ``.jpg`` / ``.png`` of GENERATED_DIR (sorted), drop the first character
of the basename, keep what follows the last ``_to_``, replace ``jpg`` by ``png`` and look that name up in GT_DIR; generated files without a
ground-truth file are reported and skipped.  Files are decoded with PIL and ``convert("RGB")``; the reference's ``imageio.imread`` returns the same
uint8 array for RGB files, but a grey file (two dimensions there) or an RGBA file (four channels there) differs -- the reference's scripts fail or
score other channels on those, this tool scores their RGB conversion.

Per pair, on the resized [0, 1] fp32 images: ``psnr`` (data range 1), ``ssim`` (uniform 51 x 51 window, sample covariance, data range 1),
``ssim_256`` (Gaussian, sigma 1.2, on ``img * 255.0``, data range = max - min of the generated image), ``mae`` and ``l1``.  Over the sets: LPIPS
of the pairs (fed [0, 1] images without the [-1, 1] remap, as the reference does; pcdms_amd/metrics.py: LPIPS) and the FID of ALL ``.jpg`` /
``.png`` files of GENERATED_DIR against ``--real``, on the resized [0, 1] NCHW images.  ``--real`` is a directory or a ``.npz`` with ``mu`` and
``sigma``; a directory's statistics are read from ``<W>_<H>_statistics.npz`` inside it when that file exists and written there otherwise, as the
reference caches them.  ``--reference-remainders`` reproduces the reference's full batches only -- ``n // 64`` batches of LPIPS pairs and
``n // 128`` batches of FID images, the rest silently dropped (a set smaller than one batch counts whole); without it every image counts.
Prints the reference's report line (means and variances rounded to four places) and, when computed, ``lpips`` and ``FID``; ``--save-dir`` also
writes ``<W>_<H>_metrics.npz`` with the keys ``psnr, ssim, ssim_256, mae, l1, names``.

OpenCV, scikit-image, lpips and torchvision are not dependencies of this project: the resize and the metrics are restated from their published
definitions and checked against fp64 restatements (tests/test_eval_metrics.py, test_metrics.py, test_lpips.py, test_fid.py).  Parity with the
packages themselves is NOT pinned by a test here.
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

KEYS = ("psnr", "ssim", "ssim_256", "mae", "l1")


def image_files(directory) -> list:
    """The ``.jpg`` and ``.png`` files of a directory, sorted (the reference's ``get_image_list``)."""
    return sorted(str(f) for f in Path(directory).iterdir() if f.suffix in (".jpg", ".png"))


def pair_files(generated_dir, gt_dir):
    """``(gt_list, generated_list, skipped)`` by the reference's ``preprocess_path_for_deform_task``."""
    gt_list, gen_list, skipped = [], [], []
    for gen in image_files(generated_dir):
        name = os.path.basename(gen)[1:].split("_to_")[-1].replace("jpg", "png")
        gt = os.path.join(str(gt_dir), name)
        if not os.path.isfile(gt):
            skipped.append(gen)
            continue
        gt_list.append(gt)
        gen_list.append(gen)
    return gt_list, gen_list, skipped


def load_resized(files, size, device, layout: str) -> torch.Tensor:
    """fp32 batch on the device, ``cv2.resize(imread(f).astype(np.float32), size, interpolation=cv2.INTER_CUBIC) / 255.0`` of every file."""
    from PIL import Image

    from pcdms_amd import preprocess
    W, H = size
    out = torch.empty((len(files), H, W, 3) if layout == "nhwc" else (len(files), 3, H, W), dtype=torch.float32, device=device)
    for i, f in enumerate(files):
        img = torch.from_numpy(np.asarray(Image.open(f).convert("RGB"), dtype=np.uint8).copy()).to(device)
        preprocess.resize_cv_cubic(img, size, divisor=255.0, layout=layout, out=out, index=i)
    return out


def reconstruction(gen_files, gt_files, size, device, *, win_size: int = 51, batch: int = 16) -> dict:
    """Per-pair fp32 arrays ``psnr, ssim, ssim_256, mae, l1`` of the reference's ``Reconstruction_Metrics.calculate_from_disk``."""
    from pcdms_amd import metrics
    res = {k: [] for k in KEYS}
    for i in range(0, len(gen_files), batch):
        pred, gt = load_resized(gen_files[i:i + batch], size, device, "nhwc"), load_resized(gt_files[i:i + batch], size, device, "nhwc")
        res["psnr"].append(metrics.psnr(pred, gt, data_range=1.0))
        res["ssim"].append(metrics.ssim_box(pred, gt, win_size=win_size, data_range=1.0))
        res["ssim_256"].append(metrics.ssim(pred * 255.0, gt * 255.0, sigma=1.2))
        res["mae"].append(metrics.mae(pred, gt))
        res["l1"].append(metrics.l1(pred, gt))
    return {k: torch.cat(v).cpu().numpy() for k, v in res.items()}


def lpips_pairs(gen_files, gt_files, size, device, model, *, batch: int = 64, reference_remainders: bool = False) -> np.ndarray:
    n = len(gen_files)
    if reference_remainders and n >= batch:
        n = n // batch * batch
    out = []
    for i in range(0, n, batch):
        a, b = load_resized(gen_files[i:min(i + batch, n)], size, device, "nchw"), load_resized(gt_files[i:min(i + batch, n)], size, device, "nchw")
        out.append(model(a, b)[:, 0, 0, 0])
    return torch.cat(out).cpu().numpy()


def fid_statistics(files, size, device, fid, *, batch: int = 128, reference_remainders: bool = False):
    if not files:
        raise ValueError("no images for the FID statistics")
    batches = (load_resized(files[i:i + batch], size, device, "nchw") for i in range(0, len(files), batch))
    return fid.statistics(batches, drop_remainder=batch if reference_remainders else None)


def real_statistics(real, size, device, fid, **kw):
    """``FIDStatistics`` of ``--real``: a ``.npz``, or a directory with its ``<W>_<H>_statistics.npz`` cache (read when present, else written)."""
    from pcdms_amd import metrics
    if str(real).lower().endswith(".npz"):
        return metrics.FIDStatistics.load(real)
    cache = Path(real) / f"{size[0]}_{size[1]}_statistics.npz"
    if cache.exists():
        return metrics.FIDStatistics.load(cache)
    st = fid_statistics(image_files(real), size, device, fid, **kw)
    st.save(cache)
    return st


def report(res: dict) -> str:
    def mv(label, key):
        return "%s: %.4f %s Variance: %.4f" % (label, round(float(np.mean(res[key])), 4), label, round(float(np.var(res[key])), 4))
    lines = [" ".join((mv("PSNR", "psnr"), mv("SSIM_256", "ssim_256"), mv("MAE", "mae"), mv("l1", "l1")))]
    if "lpips" in res:
        lines.append("lpips: %.3f" % float(np.mean(res["lpips"])))
    if "fid" in res:
        lines.append("FID: %.4f" % res["fid"])
    return "\n".join(lines)


def main(argv=None, device=None, *, win_size: int = 51) -> dict:
    """``win_size``: the uniform SSIM window (the reference's 51; a keyword for tests, whose images are smaller than that)."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("generated")
    ap.add_argument("ground_truth")
    ap.add_argument("--size", type=int, nargs=2, required=True, metavar=("W", "H"), help="evaluation size: 176 256 or 352 512 in the paper")
    ap.add_argument("--real", help="the real set of the FID: a directory of images or a .npz with mu and sigma")
    ap.add_argument("--fid-weights", help="torchvision inception_v3 state dict (.pth / .safetensors)")
    ap.add_argument("--fid-dims", type=int, default=2048, choices=(64, 192, 768, 2048), help="feature block (the reference's BLOCK_INDEX_BY_DIM)")
    ap.add_argument("--fid-no-resize", action="store_true", help="feed the images at the evaluation size (resize_input=False)")
    ap.add_argument("--fid-batch", type=int, default=128)
    ap.add_argument("--lpips-weights", help="LPIPS checkpoint: the lpips package's layout, or torchvision's alexnet with --lpips-lin")
    ap.add_argument("--lpips-lin", help="the lpips package's alex.pth (lin layers) when --lpips-weights is torchvision's alexnet")
    ap.add_argument("--lpips-batch", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16, help="pairs per launch of the per-pair metrics")
    ap.add_argument("--save-dir", help="write <W>_<H>_metrics.npz here")
    ap.add_argument("--reference-remainders", action="store_true", help="only n // batch full batches for LPIPS and FID, as the reference")
    args = ap.parse_args(argv)
    if bool(args.fid_weights) != bool(args.real):
        ap.error("--fid-weights and --real go together")
    from pcdms_amd import metrics
    device = torch.device("cuda:0") if device is None else device
    size = (int(args.size[0]), int(args.size[1]))
    gt_list, gen_list, skipped = pair_files(args.generated, args.ground_truth)
    for f in skipped:
        print(f"no ground truth for {f}: skipped")
    print(len(gt_list), len(gen_list))
    if not gen_list:
        raise ValueError(f"no generated image of {args.generated} has a ground-truth file in {args.ground_truth}")
    res = reconstruction(gen_list, gt_list, size, device, win_size=win_size, batch=args.batch)
    res["names"] = np.array([os.path.basename(f) for f in gen_list])
    if args.save_dir:
        with open(Path(args.save_dir) / f"{size[0]}_{size[1]}_metrics.npz", "wb") as f:
            np.savez(f, **{k: res[k] for k in KEYS}, names=res["names"])
    if args.lpips_weights:
        model = metrics.LPIPS.from_pretrained(args.lpips_weights, args.lpips_lin)
        res["lpips"] = lpips_pairs(gen_list, gt_list, size, device, model, batch=args.lpips_batch, reference_remainders=args.reference_remainders)
    if args.fid_weights:
        fid = metrics.FID(metrics.InceptionV3Features.from_pretrained(args.fid_weights, dims=args.fid_dims, resize_input=not args.fid_no_resize))
        kw = dict(batch=args.fid_batch, reference_remainders=args.reference_remainders)
        res["fid"] = fid(fid_statistics(image_files(args.generated), size, device, fid, **kw), real_statistics(args.real, size, device, fid, **kw))
    res["skipped"] = skipped
    print(report(res))
    return res


if __name__ == "__main__":
    main()
