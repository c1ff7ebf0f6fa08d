"""The definition of splatco_amd.normals.depth_normals / normal_loss restated in torch ops (include/splatco_normals.h): what
the host and GPU tests of the normals compare against, and the input recipe they share.

dtype=torch.float64 is the reference: z carries the VALUE of the one division in the inputs' dtype (float32 maps: the binary32
quotient the kernel forms) and the DERIVATIVE of the division in float64; rays, points, tangents, the cross product, the
normalisation, the terms and the sum are float64.  dtype=torch.float32 is the float32 chain: every per-pixel op in float32,
the sum of the loss in float64 rounded once (the definition's).

Pixels that are not ok are replaced by finite stand-ins before anything is computed from them, and a hole's c (and a hole's
prior) by (0, 0, -1) before it is normalised, so neither a hole's value nor 0 * its value is ever formed and autograd gives
it exactly zero."""
import math

import torch


def intrinsics_fov(H, W, fov_x=math.radians(60.0)):
    """(fx, fy, cx, cy) of the recipe's camera: FoVx 60 degrees, fy = fx, the principal point at the image centre."""
    fx = W / (2.0 * math.tan(fov_x * 0.5))
    return (fx, fx, W * 0.5, H * 0.5)


def ok_pixels(depth, alpha, min_alpha=0.5):
    return torch.isfinite(depth) & torch.isfinite(alpha) & (alpha >= min_alpha) & (depth > 0)


def normals_ref(depth, alpha, intr, min_alpha=0.5, dtype=torch.float64, rot=None):
    """Returns a dict: n ([3,H,W] `dtype`, differentiable w.r.t. depth and alpha; in the world frame if the camera-to-world
    rotation `rot` [3,3] is given), valid ([H,W] bool), ok ([H,W] bool), cc ([H,W] `dtype`, detached: c.c, 0 where not valid)."""
    H, W = depth.shape
    fx, fy, cx, cy = intr
    dev = depth.device
    ok = ok_pixels(depth, alpha, min_alpha)
    valid = torch.zeros(H, W, dtype=torch.bool, device=dev)
    cc_map = torch.zeros(H, W, dtype=dtype, device=dev)
    if H < 3 or W < 3:
        zero = torch.zeros_like(depth)
        hang = ((torch.where(ok, depth, zero) + torch.where(ok, alpha, zero)) * 0.0).sum().to(dtype)
        return dict(n=torch.zeros(3, H, W, dtype=dtype, device=dev) + hang, valid=valid, ok=ok, cc=cc_map)
    one = torch.ones_like(depth)
    D, A = torch.where(ok, depth, one), torch.where(ok, alpha, one)
    z = D.to(dtype) / A.to(dtype)                         # the derivative: dz/dD = 1 / A, dz/dA = -D / A^2
    z = z + ((D / A).to(dtype) - z).detach()              # the value: the quotient rounded in the inputs' dtype
    xs = (torch.arange(W, dtype=dtype, device=dev) + 0.5 - cx) / fx
    ys = (torch.arange(H, dtype=dtype, device=dev) + 0.5 - cy) / fy
    P = torch.stack((z * xs[None, :], z * ys[:, None], z))
    tx = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    ty = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    c = torch.cross(ty, tx, dim=0)
    inner = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1]
    cc = (c.detach() * c.detach()).sum(0)
    inner = inner & (cc > 1e-24)
    front = torch.tensor([0.0, 0.0, -1.0], dtype=dtype, device=dev).reshape(3, 1, 1)
    c = torch.where(inner, c, front)
    unit = c / (c * c).sum(0).sqrt()
    n = torch.nn.functional.pad(torch.where(inner, unit, torch.zeros_like(unit)), (1, 1, 1, 1))
    valid[1:-1, 1:-1] = inner
    cc_map[1:-1, 1:-1] = torch.where(inner, cc, torch.zeros_like(cc))
    if rot is not None:
        n = torch.einsum("ij,jhw->ihw", rot.to(dev, dtype), n)
    return dict(n=n, valid=valid, ok=ok, cc=cc_map)


def mask_weights(mask, like, dtype):
    if mask is None:
        return torch.ones(like.shape, dtype=dtype, device=like.device)
    return mask.to(dtype) if mask.is_floating_point() else (mask != 0).to(dtype)


def normal_loss_ref(depth, alpha, prior, intr, mask=None, min_alpha=0.5, dtype=torch.float64):
    """Returns a dict: loss (0-d `dtype`, differentiable w.r.t. depth and alpha), n_valid (int tensor), good ([H,W] bool: the
    pixels that carry a term), weight_sum (float: sum of the mask over them), and normals_ref's n, valid, ok, cc."""
    r = normals_ref(depth, alpha, intr, min_alpha, dtype)
    dev = depth.device
    m = mask_weights(mask, depth, dtype)
    finite = torch.isfinite(prior).all(0)
    front = torch.tensor([0.0, 0.0, -1.0], dtype=dtype, device=dev).reshape(3, 1, 1)
    p = torch.where(finite, prior.to(dtype), front)
    good = r["valid"] & (m > 0) & finite & ((p.detach() * p.detach()).sum(0) > 1e-24)
    p = torch.where(good, p, front)
    unit = p / (p * p).sum(0).sqrt()
    term = 1.0 - (r["n"] * unit).sum(0)
    zero = torch.zeros_like(term)
    m_good = torch.where(good, m, zero)
    loss = ((m_good * torch.where(good, term, zero)).double().sum() / depth.numel()).to(dtype)
    return dict(r, loss=loss, n_valid=good.sum(), good=good, weight_sum=float(m_good.double().sum()))


def neighbourhood(valid):
    """[H,W] bool: the pixels that are valid or a 4-neighbour of a valid pixel (the only ones that may get a gradient)."""
    near = valid.clone()
    near[:, 1:] |= valid[:, :-1]
    near[:, :-1] |= valid[:, 1:]
    near[1:, :] |= valid[:-1, :]
    near[:-1, :] |= valid[1:, :]
    return near


def recipe(H, W, seed, device="cpu", mask_kind="f32"):
    """The issue's input recipe, generated on the CPU (the same numbers whatever the device):
      z = 2 + 0.3 u + 0.2 v + 0.1 sin(3 u + 1) cos(2 v) + 1e-3 (U - 0.5), u, v in [-1, 1] at the pixel centres
      A = 0.55 + 0.45 U, set to 0.2 (below min_alpha) on a random 10 % of the pixels;  D = float32(A z)
      FoVx 60 degrees, fy = fx;  prior = normalize(n_ref + 0.3 (U - 0.5)^3), n_ref the float64 reference's normals
      mask: m in [0.25, 1.25), zero on 20 % of the pixels (the depth recipe's); mask_kind None, "f32", "u8", "bool"
    Returns (D, A, prior, mask, intr)."""
    gen = torch.Generator().manual_seed(seed)
    U = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64)
    u = ((torch.arange(W, dtype=torch.float64) + 0.5) / W * 2.0 - 1.0)[None, :]
    v = ((torch.arange(H, dtype=torch.float64) + 0.5) / H * 2.0 - 1.0)[:, None]
    z = 2.0 + 0.3 * u + 0.2 * v + 0.1 * torch.sin(3.0 * u + 1.0) * torch.cos(2.0 * v) + 1e-3 * (U(H, W) - 0.5)
    A = 0.55 + 0.45 * U(H, W)
    A = torch.where(U(H, W) < 0.1, torch.full_like(A, 0.2), A)
    D = (A * z).float()
    A = A.float()
    intr = intrinsics_fov(H, W)
    n_ref = normals_ref(D, A, intr)["n"]
    prior = n_ref + 0.3 * (U(3, H, W) - 0.5) ** 3
    prior = (prior / prior.norm(dim=0).clamp_min(1e-30)).float()
    m = (0.25 + U(H, W)).float()
    m = torch.where(U(H, W) < 0.2, torch.zeros_like(m), m)
    mask = {None: None, "f32": m, "u8": (m > 0).to(torch.uint8) * 3, "bool": m > 0}[mask_kind]
    mv = lambda x: None if x is None else x.to(device)
    return mv(D), mv(A), mv(prior), mv(mask), intr
