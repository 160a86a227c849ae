"""Score two sets of equal-sized images pair by pair on the device: PSNR, Gaussian-weighted SSIM and LPIPS (AlexNet), printed the way the
reference's ``Reconstruction_Metrics.calculate_from_disk`` / ``LPIPS.calculate_from_disk`` print them (means and variances over the pairs),
and, with ``--fid-weights``, the FID of ALL generated images against a real set.

    python tools/score_pairs.py GENERATED_DIR GT_DIR --lpips-weights alex_lpips.pth [--lpips-lin alex.pth] [--normalize]
                                [--fid-weights inception_v3.pth --fid-real REAL_DIR|STATS.npz [--fid-batch 128 --fid-drop-remainder]]

Each argument is a directory (its image files, sorted by name), a ``.txt`` list of paths, or one image file.  Files are decoded with PIL and
scored AS THEY ARE: the images of a pair, and all pairs, must have one size.  The reference resizes every image with
``cv2.resize(..., INTER_CUBIC)`` first: ``tools/calculate_metrics.py`` is the tool that does that (the reference's metric scripts as a whole, with
its pairing, MAE, L1 and the uniform-window SSIM); this one scores files that already are at the evaluation size.
SSIM is the reference's ``ssim_256`` (sigma 1.2, data range = max - min of the generated image); LPIPS follows the reference in feeding [0, 1]
images without the [-1, 1] remap unless ``--normalize`` is given (pcdms_amd/metrics.py: LPIPS).  FID is the reference's: InceptionV3 pool3
features of the bilinearly resized (299 x 299) images with its [0, 1]-input remap quirk, fp64 statistics, Frechet distance
(pcdms_amd/metrics.py: InceptionV3Features, FID); ``--fid-real`` is a directory / list of real images or a ``.npz`` with ``mu`` and ``sigma``
(the reference's statistics format).  ``--fid-batch 128 --fid-drop-remainder`` reproduces the reference's ``n // 128`` full batches, which
silently drop the last ``n % 128`` images of each set; without it every image counts.  Parity with torchvision's checkpoint is not pinned by
a test of this project.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

IMAGE_SUFFIXES = {".png", ".jpg", ".jpeg", ".bmp", ".webp"}


def image_list(arg: str) -> list:
    p = Path(arg)
    if p.is_dir():
        return sorted(str(f) for f in p.iterdir() if f.suffix.lower() in IMAGE_SUFFIXES)
    if p.suffix.lower() == ".txt":
        return sorted(ln.strip() for ln in p.read_text().splitlines() if ln.strip())
    return [str(p)]


def load_batch(files, device) -> torch.Tensor:
    from PIL import Image
    arrs = [np.asarray(Image.open(f).convert("RGB"), dtype=np.uint8) for f in files]
    if len({a.shape for a in arrs}) != 1:
        raise ValueError(f"images of different sizes: {sorted({a.shape[:2] for a in arrs})} (resize them first; see --help)")
    return torch.from_numpy(np.stack(arrs)).to(device)


def score(files_a, files_b, lpips_model, device, *, normalize: bool = False, batch: int = 16) -> dict:
    """Per-pair fp32 arrays ``{"psnr", "ssim_256", "lpips"}`` (``lpips`` only with a model)."""
    from pcdms_amd import metrics
    if len(files_a) != len(files_b) or not files_a:
        raise ValueError(f"{len(files_a)} generated images against {len(files_b)} ground-truth images")
    res = {"psnr": [], "ssim_256": []}
    if lpips_model is not None:
        res["lpips"] = []
    for i in range(0, len(files_a), batch):
        a, b = load_batch(files_a[i:i + batch], device), load_batch(files_b[i:i + batch], device)
        if a.shape != b.shape:
            raise ValueError(f"generated images {tuple(a.shape[1:3])}, ground truth {tuple(b.shape[1:3])}")
        res["psnr"].append(metrics.psnr(a, b))
        res["ssim_256"].append(metrics.ssim(a, b))
        if lpips_model is not None:
            res["lpips"].append(lpips_model(a, b, normalize=normalize)[:, 0, 0, 0])
    return {k: torch.cat(v).cpu().numpy() for k, v in res.items()}


def fid_statistics(files, fid, device, *, batch: int = 128, drop_remainder: bool = False):
    """``FIDStatistics`` of the image files (decoded in batches of ``batch``; the images of one batch must have one size)."""
    if not files:
        raise ValueError("no images for the FID statistics")
    batches = (load_batch(files[i:i + batch], device) for i in range(0, len(files), batch))
    return fid.statistics(batches, drop_remainder=batch if drop_remainder else None)


def report(res: dict) -> str:
    lines = ["PSNR: %.4f PSNR Variance: %.4f SSIM_256: %.4f SSIM_256 Variance: %.4f" % (
        round(float(np.mean(res["psnr"])), 4), round(float(np.var(res["psnr"])), 4), round(float(np.mean(res["ssim_256"])), 4),
        round(float(np.var(res["ssim_256"])), 4))]
    if "lpips" in res:
        lines.append("lpips: %.3f lpips Variance: %.4f" % (float(np.mean(res["lpips"])), round(float(np.var(res["lpips"])), 4)))
    if "fid" in res:
        lines.append("FID: %.4f" % res["fid"])
    return "\n".join(lines)


def main(argv=None, device=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("generated")
    ap.add_argument("ground_truth")
    ap.add_argument("--lpips-weights", help="LPIPS checkpoint (.pth / .safetensors): the lpips package's layout, or torchvision's alexnet with --lpips-lin")
    ap.add_argument("--lpips-lin", help="the lpips package's alex.pth (lin layers) when --lpips-weights is torchvision's alexnet")
    ap.add_argument("--normalize", action="store_true", help="map [0, 1] to [-1, 1] before LPIPS (the reference's evaluation does not)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--fid-weights", help="torchvision inception_v3 state dict (.pth / .safetensors): also print the FID of all generated images")
    ap.add_argument("--fid-real", help="the real set of the FID: a directory / .txt list of images, or a .npz with mu and sigma")
    ap.add_argument("--fid-batch", type=int, default=128)
    ap.add_argument("--fid-drop-remainder", action="store_true", help="use only n // fid-batch full batches of each set, as the reference does")
    ap.add_argument("--fid-dims", type=int, default=2048, choices=(64, 192, 768, 2048), help="feature block (the reference's BLOCK_INDEX_BY_DIM)")
    ap.add_argument("--fid-no-resize", action="store_true", help="feed the images at their own size (resize_input=False)")
    args = ap.parse_args(argv)
    from pcdms_amd import metrics
    device = torch.device("cuda:0") if device is None else device
    model = metrics.LPIPS.from_pretrained(args.lpips_weights, args.lpips_lin) if args.lpips_weights else None
    res = score(image_list(args.generated), image_list(args.ground_truth), model, device, normalize=args.normalize, batch=args.batch)
    if bool(args.fid_weights) != bool(args.fid_real):
        ap.error("--fid-weights and --fid-real go together")
    if args.fid_weights:
        fid = metrics.FID(metrics.InceptionV3Features.from_pretrained(args.fid_weights, dims=args.fid_dims, resize_input=not args.fid_no_resize))
        kw = dict(batch=args.fid_batch, drop_remainder=args.fid_drop_remainder)
        real = (metrics.FIDStatistics.load(args.fid_real) if args.fid_real.lower().endswith(".npz")
                else fid_statistics(image_list(args.fid_real), fid, device, **kw))
        res["fid"] = fid(fid_statistics(image_list(args.generated), fid, device, **kw), real)
    print(report(res))
    return res


if __name__ == "__main__":
    main()
