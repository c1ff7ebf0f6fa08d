"""Test-view evaluation: render.py:36-95 (render every view in eval mode with the plane noise off, time it) and
metrics.py:38-108 (score each render against its ground truth) of the reference, without the PNG round trip through
the disk: the renders stay on the device, `quantize` reproduces the 8-bit files the reference scores.

Scores per view: SSIM (the fused L1 + SSIM kernel's forward), PSNR (from the FLIP pass's mean squared error), LDR-FLIP
(csrc/flip.hip), all kept on the device until one host read at the end.  LPIPS, the fourth score of metrics.py, is
ABSENT from the result (not zero): it needs pretrained VGG weights, which this project cannot obtain."""
import contextlib
import json
import os
import time

import torch

from . import metrics
from .renderer import prefilter_voxel, render


@contextlib.contextmanager
def _eval_mode(pc):
    """render.py:76-81: eval mode, plane noise off (Q0 = 0); the previous mode and Q0 come back on exit, on error too."""
    was_training = pc.get_color_mlp.training
    q0 = pc.feat_planes.Q0
    try:
        pc.eval()
        pc.feat_planes.Q0 = 0
        yield
    finally:
        pc.feat_planes.Q0 = q0
        pc.train(was_training)


def render_views(views, pc, pipe, bg_color, antialiased=None, filter_3d=None):
    """Render every view as render.py:47-53 does: under no_grad, prefilter_voxel then render, each view timed between
    two device synchronisations.  Returns (images: list of [3,H,W] device tensors, times: list of seconds, fps).
    fps = 1 / mean(times[5:]) as render.py:63-64 prints it (the first five views warm up); with 5 views or fewer there
    is no such tail, and the mean of all of them is taken instead of the reference's NaN.  antialiased: handed to render()
    (None: pipe.antialiasing decides).  filter_3d: Mip-Splatting's 3D smoothing filter, handed to render() (a
    filter3d.Filter3D or an [N] tensor; None: no filter)."""
    extra = {} if antialiased is None else {"antialiased": antialiased}
    if filter_3d is not None:
        extra["filter_3d"] = filter_3d
    images, times = [], []
    with _eval_mode(pc), torch.no_grad():
        for view in views:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vis = prefilter_voxel(view, pc, pipe, bg_color)
            img = render(view, pc, pipe, bg_color, visible_mask=vis, **extra)["render"]
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            images.append(img)
    tail = times[5:] if len(times) > 5 else times
    fps = 1.0 / (sum(tail) / len(tail)) if tail else float("nan")
    return images, times, fps


def score_views(images, gts, quantize=True, pixels_per_degree=metrics.DEFAULT_PPD):
    """(ssim [V], psnr [V], flip [V]) device tensors for lists of [3,H,W] renders and ground truths (metrics.py:89-93).
    With `quantize` both are first rounded to 8 bits, as the PNGs metrics.py reads."""
    ssims, psnrs, flips = [], [], []
    with torch.no_grad():
        for img, gt in zip(images, gts):
            img, gt = img.contiguous().float(), gt.contiguous().float()
            f, mse = metrics.flip_and_mse(img, gt, pixels_per_degree, quantize)
            a, b = (metrics.quantize8(img), metrics.quantize8(gt)) if quantize else (img.clamp(0, 1), gt.clamp(0, 1))
            ssims.append(metrics.ssim_value(a, b))
            psnrs.append(metrics.psnr_from_mse(mse))
            flips.append(f)
    return torch.stack(ssims), torch.stack(psnrs), torch.stack(flips)


def evaluate_views(views, pc, pipe, bg_color, gts=None, names=None, quantize=True,
                   pixels_per_degree=metrics.DEFAULT_PPD, antialiased=None, filter_3d=None):
    """Render and score test views; the result is shaped like metrics.py's per-method entry:
      {"SSIM", "PSNR", "FLIPS", "NUM", "FPS", "per_view": {"SSIM": {name: v}, "PSNR": {...}, "FLIPS": {...}}}
    gts: ground-truth [3,H,W] images, by default view.original_image[0:3] (render.py:58); names: by default
    "00000.png", ... (render.py:59).  NUM is the anchor count (render.py:91-95), FPS render.py's.  Renders are clamped
    to [0,1] (and with `quantize` rounded to 8 bits) before scoring, as saving them as PNG does.  LPIPS is absent:
    no pretrained weights can be obtained for it here.  antialiased: the views are rendered in the rasterizer's antialiased
    mode (render(); None: pipe.antialiasing decides).  filter_3d: rendered with the 3D smoothing filter (render())."""
    images, times, fps = render_views(views, pc, pipe, bg_color, **({} if antialiased is None else {"antialiased": antialiased}),
                                      **({} if filter_3d is None else {"filter_3d": filter_3d}))
    if gts is None:
        gts = [v.original_image[0:3] for v in views]
    if len(gts) != len(images):
        raise ValueError(f"{len(gts)} ground truths for {len(images)} views")
    if names is None:
        names = ["{0:05d}.png".format(i) for i in range(len(images))]
    ssim, psnr, flip = score_views(images, gts, quantize, pixels_per_degree)
    vals = torch.stack((ssim, psnr.reshape(-1), flip)).double().cpu()         # the one host read
    s, p, f = (vals[i].tolist() for i in range(3))
    mean = lambda x: float(torch.tensor(x, dtype=torch.float32).mean())       # metrics.py: torch.tensor(list).mean()
    return {"SSIM": mean(s), "PSNR": mean(p), "FLIPS": mean(f), "NUM": int(pc.get_anchor.shape[0]), "FPS": fps,
            "per_view": {"SSIM": dict(zip(names, s)), "PSNR": dict(zip(names, p)), "FLIPS": dict(zip(names, f))}}


def write_results(model_dir, result, method="ours"):
    """results.json and per_view.json in model_dir, laid out as metrics.py:96-108 writes them:
    {method: {"SSIM", "PSNR", "FLIPS", "NUM", ...}} and {method: {"SSIM": {name: v}, ...}}.  Returns the two paths."""
    full = {k: v for k, v in result.items() if k != "per_view"}
    paths = os.path.join(model_dir, "results.json"), os.path.join(model_dir, "per_view.json")
    os.makedirs(model_dir, exist_ok=True)
    with open(paths[0], "w") as fp:
        json.dump({method: full}, fp, indent=True)
    with open(paths[1], "w") as fp:
        json.dump({method: result["per_view"]}, fp, indent=True)
    return paths
