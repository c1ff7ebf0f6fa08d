"""Image-quality scores of test views (metrics.py:38-108 of the reference): LDR-FLIP in one fused HIP pass
(csrc/flip.hip), SSIM forward-only through the fused L1 + SSIM kernel (csrc/ssim.hip), PSNR.

All functions take device fp32 images, return device tensors and make no host synchronisation.  None of them has a
backward: they are evaluation metrics.  LPIPS is not here -- it needs pretrained VGG weights, which this project
cannot obtain."""
import math

import numpy as np
import torch

# the reference's default observer: a 0.7 m wide 4K monitor seen from 0.7 m (utils/flip.py LDRFLIPLoss.forward)
DEFAULT_PPD = (0.7 * 3840 / 0.7) * math.pi / 180

_FILTER_NAMES = ("a", "rg", "by1", "by2", "edge", "point", "gauss")


def flip_filters(pixels_per_degree=DEFAULT_PPD):
    """The filters the FLIP kernel receives for `pixels_per_degree`, from the library's host code (binary64; the kernel
    gets them rounded to binary32).  Returns a dict: `csf_radius`, `feature_radius`; the 1-D profiles `a`, `rg`, `by1`,
    `by2` (length 2 csf_radius + 1) and `edge`, `point`, `gauss` (length 2 feature_radius + 1), tap k at offset k - r;
    `by_c1`, `by_c2` and `cmax`.  The 2-D kernels of the reference are
      A = outer(a, a), RG = outer(rg, rg), BY = by_c1 outer(by1, by1) + by_c2 outer(by2, by2),
      edge / point detector along x = outer(gauss, edge / point)  (rows y, columns x), along y = its transpose.
    Raises ValueError when the radii exceed the kernel's limit or pixels_per_degree < 1."""
    from . import _C
    nw = 2 * _C.FLIP_MAX_RADIUS + 1
    w = np.zeros(7 * nw, dtype=np.float64)
    radii = np.zeros(2, dtype=np.int32)
    sc = np.zeros(3, dtype=np.float64)
    rc = _C.lib.scr_flip_filters(float(pixels_per_degree), w.ctypes.data, radii.ctypes.data, sc.ctypes.data)
    if rc != 0:
        raise ValueError("flip: " + _C.lib.scr_last_error().decode())
    rcsf, rfeat = int(radii[0]), int(radii[1])
    out = {"csf_radius": rcsf, "feature_radius": rfeat, "by_c1": float(sc[0]), "by_c2": float(sc[1]), "cmax": float(sc[2])}
    for i, name in enumerate(_FILTER_NAMES):
        r = rcsf if i < 4 else rfeat
        out[name] = w[i * nw:i * nw + 2 * r + 1].copy()
    return out


def _pairs(test, reference, what):
    if not (isinstance(test, torch.Tensor) and isinstance(reference, torch.Tensor)):
        raise TypeError(f"{what}: test and reference must be tensors")
    if torch.is_grad_enabled() and (test.requires_grad or reference.requires_grad):
        raise RuntimeError(f"{what} has no backward: call it under torch.no_grad() or pass detached tensors")
    if test.shape != reference.shape or test.dim() not in (3, 4) or test.shape[-3] != 3:
        raise ValueError(f"{what}: expected two [3,H,W] or [N,3,H,W] images of one shape, got "
                         f"{tuple(test.shape)} and {tuple(reference.shape)}")
    if not (test.is_cuda and reference.is_cuda) or test.device != reference.device:
        raise ValueError(f"{what}: the images must be on one GPU (the kernel is HIP only)")
    if test.dtype != torch.float32 or reference.dtype != torch.float32:
        raise TypeError(f"{what}: expected float32 images")
    if min(test.shape[-2:]) < 1 or (test.dim() == 4 and test.shape[0] < 1):
        raise ValueError(f"{what}: empty image")
    single = test.dim() == 3
    t = test.detach().contiguous()
    r = reference.detach().contiguous()
    return (t[None], r[None]) if single else (t, r), single


def _flip_run(test, reference, pixels_per_degree, quantize, return_map):
    from . import _C
    (t, r), single = _pairs(test, reference, "flip")
    N, _, H, W = t.shape
    dev = t.device
    scratch = torch.empty(max(_C.lib.scr_flip_scratch_bytes(N, H, W), 1), dtype=torch.uint8, device=dev)
    mean = torch.empty(N, dtype=torch.float32, device=dev)
    mse = torch.empty(N, dtype=torch.float32, device=dev)
    fmap = torch.empty(N, H, W, dtype=torch.float32, device=dev) if return_map else None
    if _C.call("scr_flip_forward", N, H, W, t, r, float(pixels_per_degree), int(bool(quantize)), scratch, mean, mse, fmap,
                check=False) != 0:
        raise ValueError("flip: " + _C.lib.scr_last_error().decode())
    if single:
        mean, mse = mean[0], mse[0]
        fmap = None if fmap is None else fmap[0]
    return mean, mse, fmap


def flip(test, reference, pixels_per_degree=DEFAULT_PPD, quantize=False, return_map=False):
    """LDR-FLIP of sRGB images in [0,1] (utils/flip.py LDRFLIPLoss at its defaults, `.mean()` per image as metrics.py
    takes it).  test / reference: [3,H,W] or [N,3,H,W] device float32; values are clamped to [0,1], and with
    `quantize` rounded to 8 bits as a PNG written by save_image and read back by to_tensor.  Returns the mean FLIP
    ([] or [N]), and with `return_map` also the per-pixel map ([H,W] or [N,H,W]).  No backward: inputs that require
    grad are refused under grad mode."""
    mean, _, fmap = _flip_run(test, reference, pixels_per_degree, quantize, return_map)
    return (mean, fmap) if return_map else mean


def flip_and_mse(test, reference, pixels_per_degree=DEFAULT_PPD, quantize=False):
    """(mean FLIP, mean squared error) of the same clamped (quantized) pairs from one pass; psnr_from_mse turns the
    second into the PSNR."""
    mean, mse, _ = _flip_run(test, reference, pixels_per_degree, quantize, False)
    return mean, mse


def psnr_from_mse(mse):
    """20 log10(1 / sqrt(mse)), as utils/image_utils.py psnr forms it."""
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def psnr(img1, img2):
    """PSNR per image of [3,H,W] ([1]) or [N,3,H,W] ([N,1]) device images (losses.psnr, utils/image_utils.py)."""
    from .losses import psnr as _psnr
    if torch.is_grad_enabled() and (img1.requires_grad or img2.requires_grad):
        raise RuntimeError("psnr has no backward here: call it under torch.no_grad() or pass detached tensors")
    return _psnr(img1.detach(), img2.detach())


def quantize8(img):
    """The 8-bit round trip of an image written by torchvision's save_image and read back by to_tensor: k / 255
    correctly rounded to binary32, as the kernel and to_tensor's host division form it (a device tensor divided by
    a scalar is multiplied by its reciprocal instead, 1 ulp off for half of the 256 levels)."""
    return (torch.floor(img.clamp(0, 1) * 255 + 0.5).double() / 255).float()


def ssim_value(a, b):
    """Mean SSIM (11x11 Gaussian window, sigma 1.5, zero padding; losses.ssim, utils/loss_utils.py) of two [3,H,W]
    device images as a 0-d device tensor: the forward of the fused L1 + SSIM kernel without its derivative maps."""
    from . import _C
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)) or a.shape != b.shape or a.dim() != 3:
        raise ValueError("ssim_value: expected two [C,H,W] images of one shape")
    if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad):
        raise RuntimeError("ssim_value has no backward: use losses.l1_ssim for a differentiable SSIM")
    if not (a.is_cuda and b.is_cuda) or a.device != b.device:
        raise ValueError("ssim_value: the images must be on one GPU")
    x, y = a.detach().contiguous().float(), b.detach().contiguous().float()
    Cc, H, W = x.shape
    scratch = torch.empty(_C.lib.scr_l1_ssim_scratch_bytes(Cc, H, W, 0), dtype=torch.uint8, device=x.device)
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    _C.call("scr_l1_ssim_forward", Cc, H, W, x, y, scratch, 0, out)
    return out[1]
