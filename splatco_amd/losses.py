"""Loss / metric functions of the training step around the rasterizer (plain PyTorch), restating
utils/loss_utils.py:17-63 and utils/image_utils.py:14-19; pinned by tests/golden/losses.npz.
psnr() is the parity metric of BASELINE.json ("PSNR-match")."""
from math import exp

import os

import torch
import torch.nn.functional as F


def l1_loss(network_output, gt):
    return torch.abs(network_output - gt).mean()


def l2_loss(network_output, gt):
    return ((network_output - gt) ** 2).mean()


def psnr(img1, img2):
    mse = ((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def _window(window_size, channel, like):
    g = torch.tensor([exp(-(x - window_size // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(window_size)])
    g = (g / g.sum()).unsqueeze(1)
    w2d = g.mm(g.t()).float().unsqueeze(0).unsqueeze(0)
    return w2d.expand(channel, 1, window_size, window_size).contiguous().to(like)


def ssim(img1, img2, window_size=11, size_average=True):
    channel = img1.size(-3)
    window = _window(window_size, channel, img1)
    pad = window_size // 2
    mu1 = F.conv2d(img1, window, padding=pad, groups=channel)
    mu2 = F.conv2d(img2, window, padding=pad, groups=channel)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, window, padding=pad, groups=channel) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, window, padding=pad, groups=channel) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, window, padding=pad, groups=channel) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean() if size_average else ssim_map.mean(1).mean(1).mean(1)


class _L1Ssim(torch.autograd.Function):
    """(mean |x - y|, mean SSIM(x, y)) of two [C,H,W] device images in one fused HIP pass
    (csrc/ssim.hip); the gradient flows to x only.  11 ms -> ~0.3 ms forward+backward at 1080p."""

    @staticmethod
    def forward(ctx, x, y):
        from . import _C
        # whether the derivative maps are needed is a property of the INPUT: grad mode is off inside forward, so a
        # converted copy (non-contiguous crop, other dtype) would report requires_grad = False
        need = bool(ctx.needs_input_grad[0])
        x, y = x.contiguous().float(), y.contiguous().float()
        C, H, W = x.shape
        scratch = torch.empty(_C.lib.scr_l1_ssim_scratch_bytes(C, H, W, int(need)), dtype=torch.uint8, device=x.device)
        out = torch.empty(2, dtype=torch.float32, device=x.device)
        _C.call("scr_l1_ssim_forward", C, H, W, x, y, scratch, int(need), out)
        ctx.save_for_backward(x, y, scratch)
        ctx.have_maps = need
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_l1, g_ssim):
        from . import _C
        x, y, scratch = ctx.saved_tensors
        if not ctx.have_maps:
            raise RuntimeError("l1_ssim backward without the derivative maps of the forward pass")
        C, H, W = x.shape
        g_l1 = g_l1.contiguous().float().reshape(1)
        g_ssim = g_ssim.contiguous().float().reshape(1)
        dx = torch.empty_like(x)
        _C.call("scr_l1_ssim_backward", C, H, W, x, y, scratch, g_l1, g_ssim, dx)
        return dx, None


class _PairL1(torch.autograd.Function):
    """mean |(real1 - real2) - (gen1 - gen2)| of four equally shaped device images (the L1 of the cross-view consistency
    term, train.py:208-217) in one pass per direction (csrc/ssim.hip); the gradient flows to gen1 / gen2."""

    @staticmethod
    def forward(ctx, gen1, gen2, real1, real2):
        from . import _C
        c = lambda t: t.detach().contiguous().float()
        gen1, gen2, real1, real2 = c(gen1), c(gen2), c(real1), c(real2)
        n, dev = gen1.numel(), gen1.device
        scratch = torch.empty(_C.lib.scr_pair_l1_scratch_bytes(n), dtype=torch.uint8, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        _C.call("scr_pair_l1_forward", n, gen1, gen2, real1, real2, scratch, out)
        ctx.save_for_backward(gen1, gen2, real1, real2)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        from . import _C
        gen1, gen2, real1, real2 = ctx.saved_tensors
        n = gen1.numel()
        g = g.contiguous().float().reshape(1)
        d1 = torch.empty_like(gen1) if ctx.needs_input_grad[0] else None
        d2 = torch.empty_like(gen2) if ctx.needs_input_grad[1] else None
        _C.call("scr_pair_l1_backward", n, gen1, gen2, real1, real2, g, d1, d2)
        return d1, d2, None, None


def pair_l1(gen1, gen2, real1, real2):
    """l1_loss(real1 - real2, gen1 - gen2) (train.py:213): the fused op on the GPU, the reference's ops elsewhere."""
    if gen1.is_cuda and gen1.shape == gen2.shape == real1.shape == real2.shape and gen1.numel() > 0 and not (real1.requires_grad or real2.requires_grad):
        return _PairL1.apply(gen1, gen2, real1, real2)
    return l1_loss(real1 - real2, gen1 - gen2)


def l1_ssim(image, gt_image):
    """Fused (l1_loss, ssim) for [C,H,W] device images; falls back to the torch ops on CPU, and where gt_image wants a
    gradient (the fused backward has none for it).  The kernel reads gt_image with image's extents: another shape or
    device is an error here, before any launch."""
    if image.is_cuda and image.dim() == 3:
        if gt_image.shape != image.shape or gt_image.device != image.device:
            raise ValueError(f"l1_ssim: gt_image {tuple(gt_image.shape)} on {gt_image.device} does not match "
                             f"image {tuple(image.shape)} on {image.device}")
        if not (torch.is_grad_enabled() and gt_image.requires_grad):
            return _L1Ssim.apply(image, gt_image)
    return l1_loss(image, gt_image), ssim(image, gt_image)


class _ScalingReg(torch.autograd.Function):
    """mean(prod(scaling, dim=1)) for scaling [P,3] on the GPU (csrc/ssim.hip).  torch's prod backward first counts the
    zeros of its input (a compare, an int64 reduction and a host read) -- 2.5 ms per step at 85 M Gaussians."""

    @staticmethod
    def forward(ctx, scaling):
        from . import _C
        s = scaling.detach().contiguous().float()
        P = s.shape[0]
        scratch = torch.empty(_C.lib.scr_scaling_reg_scratch_bytes(P), dtype=torch.uint8, device=s.device)
        out = torch.empty(1, dtype=torch.float32, device=s.device)
        _C.call("scr_scaling_reg_forward", P, s, scratch, out)
        ctx.save_for_backward(s)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        from . import _C
        (s,) = ctx.saved_tensors
        g = g.contiguous().float().reshape(1)
        d = torch.empty_like(s)
        _C.call("scr_scaling_reg_backward", s.shape[0], s, g, d)
        return d


class _ScalingRegTap(torch.autograd.Function):
    """The same value as _ScalingReg for the `scaling` output of expand.expand_compact, with the gradient sent to the
    expansion's `tap` instead of to `scaling`: csrc/expand.hip's backward kernel adds dL/dreg * d reg / d scaling to the
    rasterizer's dL/dscales while it reads them (at 88 M Gaussians the separate gradient tensor and autograd's
    accumulation pass were 0.9 ms of the cfg4 step)."""

    @staticmethod
    def forward(ctx, tap, scaling):
        from . import _C
        s = scaling.detach().contiguous().float()
        P = s.shape[0]
        scratch = torch.empty(_C.lib.scr_scaling_reg_scratch_bytes(P), dtype=torch.uint8, device=s.device)
        out = torch.empty(1, dtype=torch.float32, device=s.device)
        _C.call("scr_scaling_reg_forward", P, s, scratch, out)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        return g.reshape(1), None


def scaling_reg(scaling):
    """mean(prod(scaling, dim=1)) (train.py:192-196)."""
    if scaling.is_cuda and scaling.dim() == 2 and scaling.shape[1] == 3 and scaling.shape[0] > 0:
        tap = None if os.environ.get("SPLATCO_NO_REG_TAP") else getattr(scaling, "_scr_reg_tap", None)
        if tap is not None and tap.requires_grad and scaling.dtype == torch.float32:
            return _ScalingRegTap.apply(tap, scaling)
        return _ScalingReg.apply(scaling)
    return scaling.prod(dim=1).mean()


def view_loss(image, gt_image, scaling, lambda_dssim=0.2):
    """Per-view training loss (train.py:192-196): 0.8 L1 + 0.2 (1 - SSIM) + 0.01 mean(prod(scaling))."""
    l1, s = l1_ssim(image, gt_image)
    return (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - s) + 0.01 * scaling_reg(scaling)


_DEPTH_MODES = {"inverse": 0, "expected": 1}


def _depth_loss_torch(depth, alpha, target, mask, mode, align, min_alpha):
    """The definition of depth_loss in torch ops: float32 prediction, float64 moments, residual and sum.  Every hole is
    replaced by finite values BEFORE anything is computed from it, so that neither its value nor 0 * its value reaches a
    sum or a gradient."""
    m = torch.ones_like(depth) if mask is None else (mask.to(depth.dtype) if mask.is_floating_point() else (mask != 0).to(depth.dtype))
    valid = (m > 0) & torch.isfinite(target) & torch.isfinite(depth) & torch.isfinite(alpha) & (alpha >= min_alpha) & (depth > 0)
    one, zero = torch.ones_like(depth), torch.zeros_like(depth)
    D, A = torch.where(valid, depth, one), torch.where(valid, alpha, one)
    g, m = torch.where(valid, target, zero).double(), torch.where(valid, m, zero).double()
    p = (A / D if mode == "inverse" else D / A).double()
    n_valid = valid.sum()
    s, t = p.new_ones(()), p.new_zeros(())
    if align:
        with torch.no_grad():
            S0, Sp, Spp, Sg, Spg = m.sum(), (m * p).sum(), (m * (p * p)).sum(), (m * g).sum(), (m * (p * g)).sum()
            det = S0 * Spp - Sp * Sp
            ok = (n_valid >= 2) & (det > 1e-12 * (S0 * Spp))
            safe = torch.where(ok, det, torch.ones_like(det))
            s_fit = (S0 * Spg - Sp * Sg) / safe
            t_fit = (Sg - s_fit * Sp) / torch.where(ok, S0, torch.ones_like(S0))
            s, t = torch.where(ok, s_fit, s), torch.where(ok, t_fit, t)
    loss = ((m * ((s * p + t) - g).abs()).sum() / depth.numel()).float()
    return loss, torch.stack((s.float(), t.float(), n_valid.float())).detach()


class _DepthLoss(torch.autograd.Function):
    """depth_loss on the GPU (csrc/depth_loss.hip): a moment pass and a residual pass with fixed-order float64 sums, one
    element-wise backward pass; the gradient flows to depth and alpha only."""

    @staticmethod
    def forward(ctx, depth, alpha, target, mask, mode, align, min_alpha):
        from . import _C
        c = lambda t: t.detach().contiguous().float()
        depth, alpha, target = c(depth), c(alpha), c(target)
        kind = 0
        if mask is not None:
            mask = mask.detach().contiguous()
            if mask.dtype == torch.bool:
                mask = mask.view(torch.uint8)           # the same bytes: no conversion pass
            if mask.dtype != torch.uint8:
                mask = mask.float()
            kind = 2 if mask.dtype == torch.uint8 else 1
        H, W = depth.shape
        dev = depth.device
        scratch = torch.empty(_C.lib.scr_depth_loss_scratch_bytes(H, W), dtype=torch.uint8, device=dev)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        _C.call("scr_depth_loss_forward", H, W, depth, alpha, target, _C.ptr(mask), kind, mode, int(align), min_alpha, scratch, out)
        ctx.save_for_backward(depth, alpha, target, mask, scratch)
        ctx.args = (kind, mode, min_alpha)
        stats = out[1:]
        ctx.mark_non_differentiable(stats)
        return out[0], stats

    @staticmethod
    def backward(ctx, g, _):
        from . import _C
        depth, alpha, target, mask, scratch = ctx.saved_tensors
        kind, mode, min_alpha = ctx.args
        H, W = depth.shape
        g = g.contiguous().float().reshape(1)
        dd = torch.empty_like(depth) if ctx.needs_input_grad[0] else None
        da = torch.empty_like(alpha) if ctx.needs_input_grad[1] else None
        _C.call("scr_depth_loss_backward", H, W, depth, alpha, target, _C.ptr(mask), kind, mode, min_alpha, scratch, g, dd, da)
        return dd, da, None, None, None, None, None


def depth_loss(depth, alpha, target, mask=None, mode="inverse", align=True, min_alpha=0.5, return_stats=False):
    """Depth supervision on the rasterizer's maps (render(aux=True): out["depth"] = sum w z, out["alpha"] = sum w), the
    aligned inverse-depth L1 of upstream 3DGS (depth_l1_weight, invdepthmap, depth_mask).  All maps are [H, W].

    A pixel is valid where mask > 0 (absent: everywhere; float weights >= 0, or bool / uint8 with nonzero = 1), target,
    depth and alpha are finite, alpha >= min_alpha and depth > 0; every other pixel is a hole that adds nothing to the loss
    and gets exactly zero gradient, whatever it holds.  The prediction is p = alpha / depth (mode "inverse": monocular or
    inverse-depth priors) or depth / alpha (mode "expected": metric depth).  With align=True the scale and shift (s, t) that
    minimise sum mask (s p + t - target)^2 over the valid pixels are solved in closed form in float64; they are CONSTANTS of
    the backward pass (detached: no gradient flows through the fit), and (1, 0) where the fit is degenerate (fewer than two
    valid pixels, or p constant).  The loss is sum_valid mask |s p + t - target| / (H W): the mean over ALL pixels, so a
    hole never raises the weight of the others.

    On the GPU this is the fused op of csrc/depth_loss.hip: float64 sums in a fixed order (the same bits run after run), no
    host read; the gradient flows to depth and alpha.  On CPU tensors, and where target or mask wants a gradient, the same
    definition runs in torch ops.  return_stats=True: also the detached device tensor (s, t, n_valid)."""
    if mode not in _DEPTH_MODES:
        raise ValueError(f"depth_loss: mode {mode!r} is not one of {sorted(_DEPTH_MODES)}")
    min_alpha = float(min_alpha)
    if not (0.0 <= min_alpha < float("inf")):
        raise ValueError(f"depth_loss: min_alpha {min_alpha} must be finite and >= 0")
    if depth.dim() != 2 or depth.numel() == 0:
        raise ValueError(f"depth_loss: depth {tuple(depth.shape)} is not a non-empty [H, W] map")
    for name, x in (("alpha", alpha), ("target", target), ("mask", mask)):
        if x is not None and (x.shape != depth.shape or x.device != depth.device):
            raise ValueError(f"depth_loss: {name} {tuple(x.shape)} on {x.device} does not match depth {tuple(depth.shape)} on {depth.device}")
    wants = torch.is_grad_enabled() and (target.requires_grad or (mask is not None and mask.requires_grad))
    if depth.is_cuda and not wants:
        loss, stats = _DepthLoss.apply(depth, alpha, target, mask, _DEPTH_MODES[mode], bool(align), min_alpha)
    else:
        loss, stats = _depth_loss_torch(depth.float(), alpha.float(), target.float(), mask, mode, bool(align), min_alpha)
    return (loss, stats) if return_stats else loss
