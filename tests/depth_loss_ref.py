"""The definition of splatco_amd.losses.depth_loss restated in torch ops (include/splatco_raster.h, scr_depth_loss_*): what
the host and GPU tests of the depth term compare against.

dtype=torch.float64 is the reference: the prediction p carries the VALUE of the one division in the inputs' dtype (float32
maps: the binary32 quotient the kernel forms) and the DERIVATIVE of the division in float64, and moments, residual, sum and
the closed-form fit are float64.  dtype=torch.float32 is the framework chain a user would write without the fused op:
everything in float32, sum() in whatever order the framework picks.

Holes are replaced by finite stand-ins before anything is computed from them, so neither a hole's value nor 0 * its value
is ever formed and autograd gives it exactly zero."""
import torch


def valid_pixels(depth, alpha, target, mask, min_alpha):
    m = torch.ones_like(depth, dtype=torch.bool) if mask is None else (mask > 0 if mask.is_floating_point() else mask != 0)
    return m & torch.isfinite(target) & torch.isfinite(depth) & torch.isfinite(alpha) & (alpha >= min_alpha) & (depth > 0)


def depth_loss_ref(depth, alpha, target, mask=None, mode="inverse", align=True, min_alpha=0.5, dtype=torch.float64):
    """Returns a dict: loss (0-d, `dtype`; differentiable w.r.t. depth and alpha), s, t (0-d, detached), n_valid (int tensor),
    valid ([H,W] bool), residual ([H,W] `dtype`, detached; 0 at holes)."""
    assert mode in ("inverse", "expected")
    valid = valid_pixels(depth, alpha, target, mask, min_alpha)
    one = torch.ones_like(depth)
    D, A = torch.where(valid, depth, one), torch.where(valid, alpha, one)
    g = torch.where(valid, target, torch.zeros_like(target)).to(dtype)
    if mask is None:
        m = valid.to(dtype)
    else:
        w = mask.to(dtype) if mask.is_floating_point() else (mask != 0).to(dtype)
        m = torch.where(valid, w, torch.zeros_like(w))
    num, den = (A, D) if mode == "inverse" else (D, A)
    p = num.to(dtype) / den.to(dtype)                       # the derivative: d p / d num = 1 / den, d p / d den = -num / den^2
    p = p + ((num / den).to(dtype) - p).detach()            # the value: the quotient rounded in the inputs' dtype
    n_valid = valid.sum()
    s, t = torch.ones((), dtype=dtype, device=depth.device), torch.zeros((), dtype=dtype, device=depth.device)
    if align:
        pd = p.detach()
        S0, Sp, Spp, Sg, Spg = m.sum(), (m * pd).sum(), (m * pd * pd).sum(), (m * g).sum(), (m * pd * g).sum()
        det = S0 * Spp - Sp * Sp
        if int(n_valid) >= 2 and bool(det > 1e-12 * S0 * Spp):
            s = (S0 * Spg - Sp * Sg) / det
            t = (Sg - s * Sp) / S0
    r = s * p + t - g
    loss = (m * r.abs()).sum() / depth.numel()
    return dict(loss=loss, s=s, t=t, n_valid=n_valid, valid=valid, residual=torch.where(valid, r.detach(), torch.zeros_like(r)))


def closed_form_grads(depth, alpha, target, mask, mode, s, t, min_alpha=0.5, g_up=1.0):
    """The gradient formulas of the definition, in float64, with (s, t) given: (dL/ddepth, dL/dalpha)."""
    valid = valid_pixels(depth, alpha, target, mask, min_alpha)
    f = lambda x, fill: torch.where(valid, x, torch.full_like(x, fill)).double()
    D, A, g = f(depth, 1.0), f(alpha, 1.0), f(target, 0.0)
    m = valid.double() if mask is None else torch.where(valid, mask.double() if mask.is_floating_point() else (mask != 0).double(),
                                                         torch.zeros_like(D))
    p = A / D if mode == "inverse" else D / A
    q = g_up * m * float(s) * torch.sign(float(s) * p + float(t) - g) / depth.numel()
    if mode == "inverse":
        return -q * A / D ** 2, q / D
    return q / A, -q * D / A ** 2


def recipe(H, W, seed, device="cpu", mask_kind="f32", mode="inverse", line=(1.7, -0.08)):
    """The issue's input recipe: A = 0.05 + 0.95 U, z = 0.5 + 7.5 U, D = A z, g = 1.7 p - 0.08 +- u with u in [0.05, 0.2],
    m in [0.25, 1.25) and zero on 20 % of the pixels.  p is the prediction of `mode`.  Generated on the CPU (the same
    numbers whatever the device).  mask_kind: None, "f32", "u8", "bool".  line: the (1.7, -0.08) of the target; a test WITHOUT
    alignment passes (1, 0), the line that s = 1, t = 0 assumes -- under 1.7 p - 0.08 the unaligned residual -0.7 p + 0.08 +- u
    crosses zero inside the recipe's range of p, and no seed keeps it away from the kink of |.|."""
    gen = torch.Generator().manual_seed(seed)
    U = lambda: torch.rand(H, W, generator=gen)
    A = 0.05 + 0.95 * U()
    z = 0.5 + 7.5 * U()
    D = A * z
    p = A / D if mode == "inverse" else D / A
    u = 0.05 + 0.15 * U()
    sign = torch.where(U() < 0.5, -1.0, 1.0)
    g = line[0] * p + line[1] + sign * u
    m = 0.25 + U()
    m = torch.where(U() < 0.2, torch.zeros_like(m), m)
    mask = {None: None, "f32": m, "u8": (m > 0).to(torch.uint8) * 3, "bool": m > 0}[mask_kind]
    mv = lambda x: None if x is None else x.to(device)
    return mv(D), mv(A), mv(g), mv(mask)
