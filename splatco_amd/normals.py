"""Surface normals of the rasterizer's depth map and the normal-prior loss on them (host side of csrc/normals.hip).

Depth priors are known up to scale only, so on low-texture surfaces -- walls, floors, roads -- depth supervision leaves the
surface free to bend and float.  The remedy of 2DGS, PGSR, GOF and DN-Splatter is to supervise the NORMAL that the depth map
implies against a monocular normal prior.  The definition (normative; include/splatco_normals.h and tests/normals_ref.py
restate it), on the maps of render(aux=True), out["depth"] = D = sum w z and out["alpha"] = A = sum w, float32, COLMAP camera
(+x right, +y down, +z forward), per pixel e = (px, py):

  ok(e)     D, A finite, A >= min_alpha, D > 0
  z         D / A (ONE binary32 division);  ray = ((px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy, 1);  P = z ray
  tx, ty    P(px + 1, py) - P(px - 1, py),  P(px, py + 1) - P(px, py - 1);  c = ty x tx  (fronto-parallel: (0, 0, -1))
  valid(e)  the four neighbours lie inside the image, ok holds at e and at all four, and c . c > 1e-24
  n         c / |c| at valid pixels, exactly (0, 0, 0) at holes (every other pixel; the one-pixel border is all holes)
  L         (1 / (H W)) sum_valid m (1 - n . prior / |prior|): the mean over ALL pixels

    out = render(cam, pc, pipe, bg, aux=True)
    normals = depth_normals(out["depth"], out["alpha"], cam, frame="world")           # [3, H, W], for inspection or export
    loss = loss + 0.05 * normal_loss(out["depth"], out["alpha"], prior, cam, mask)   # prior [3, H, W], camera frame

or, in a training step, collaborative_step(..., normal_targets=priors, normal_masks=masks, normal_weight=0.05).

Out of scope: rendered per-Gaussian normals and 2DGS's depth-normal consistency (they need a rasterizer channel), smoothness
terms, the L1 form of the loss, camera gradients through the normals, and priors in the world frame.

Every launch goes through _C.family_call.  On CPU tensors, and where the prior or the mask wants a gradient, the same
definition runs in torch ops."""
import math

import torch

from . import _C

_FRAMES = ("camera", "world")


def intrinsics(cam):
    """(fx, fy, cx, cy) in pixels of a camera with image_width, image_height, FoVx, FoVy: the symmetric frustum of
    cameras.get_projection_matrix (P[0, 0] = 2 fx / W) and the rasterizer's pixel centres (pixel px covers [px, px + 1))."""
    W, H = int(cam.image_width), int(cam.image_height)
    return (W / (2.0 * math.tan(cam.FoVx * 0.5)), H / (2.0 * math.tan(cam.FoVy * 0.5)), W * 0.5, H * 0.5)


def _resolve(fn, cam_or_intrinsics):
    if hasattr(cam_or_intrinsics, "FoVx"):
        intr = intrinsics(cam_or_intrinsics)
    else:
        intr = tuple(float(v) for v in cam_or_intrinsics)
        if len(intr) != 4:
            raise ValueError(f"{fn}: expected a camera or (fx, fy, cx, cy), got {len(intr)} values")
    fx, fy, cx, cy = intr
    if not (0.0 < fx < float("inf") and 0.0 < fy < float("inf")):
        raise ValueError(f"{fn}: fx = {fx}, fy = {fy} must be finite and > 0")
    if not (math.isfinite(cx) and math.isfinite(cy)):
        raise ValueError(f"{fn}: cx = {cx}, cy = {cy} must be finite")
    return intr


def _check_maps(fn, depth, alpha, min_alpha, **others):
    min_alpha = float(min_alpha)
    if not (0.0 <= min_alpha < float("inf")):
        raise ValueError(f"{fn}: min_alpha {min_alpha} must be finite and >= 0")
    if depth.dim() != 2 or depth.numel() == 0:
        raise ValueError(f"{fn}: depth {tuple(depth.shape)} is not a non-empty [H, W] map")
    if depth.numel() >= 2 ** 31:
        raise ValueError(f"{fn}: H W = {depth.numel()} is not below 2^31")
    if alpha.shape != depth.shape or alpha.device != depth.device:
        raise ValueError(f"{fn}: alpha {tuple(alpha.shape)} on {alpha.device} does not match depth {tuple(depth.shape)} on {depth.device}")
    for name, (x, lead) in others.items():
        if x is not None and (tuple(x.shape) != lead + tuple(depth.shape) or x.device != depth.device):
            raise ValueError(f"{fn}: {name} {tuple(x.shape)} on {x.device} does not match depth {tuple(depth.shape)} on {depth.device}")
    return min_alpha


def _normals_torch(depth, alpha, intr, min_alpha):
    """The definition in torch ops, in the maps' dtype: (n [3, H, W] in the camera frame, valid [H, W]).  Every pixel that is
    not ok is replaced by finite values BEFORE anything is computed from it, and every hole's c by (0, 0, -1) before it is
    normalised, so that neither a hole's value nor 0 * its value reaches a result or a gradient."""
    H, W = depth.shape
    fx, fy, cx, cy = intr
    dt, dev = depth.dtype, depth.device
    ok = torch.isfinite(depth) & torch.isfinite(alpha) & (alpha >= min_alpha) & (depth > 0)
    n = torch.zeros(3, H, W, dtype=dt, device=dev)
    valid = torch.zeros(H, W, dtype=torch.bool, device=dev)
    if H < 3 or W < 3:
        zero = torch.zeros_like(depth)                  # all holes: exact zeros that still hang on depth and alpha
        return n + ((torch.where(ok, depth, zero) + torch.where(ok, alpha, zero)) * 0.0).sum(), valid
    one = torch.ones_like(depth)
    z = torch.where(ok, depth, one) / torch.where(ok, alpha, one)
    xs = (torch.arange(W, dtype=dt, device=dev) + 0.5 - cx) / fx
    ys = (torch.arange(H, dtype=dt, device=dev) + 0.5 - cy) / fy
    P = torch.stack((z * xs[None, :], z * ys[:, None], z))
    tx = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    ty = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    c = torch.cross(ty, tx, dim=0)
    inner = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1]
    inner = inner & ((c.detach() * c.detach()).sum(0) > 1e-24)
    front = torch.tensor([0.0, 0.0, -1.0], dtype=dt, device=dev).reshape(3, 1, 1)
    c = torch.where(inner, c, front)
    unit = c / (c * c).sum(0).sqrt()
    n = torch.nn.functional.pad(torch.where(inner, unit, torch.zeros_like(unit)), (1, 1, 1, 1))
    valid[1:-1, 1:-1] = inner
    return n, valid


def _normal_loss_torch(depth, alpha, prior, intr, mask, min_alpha):
    """The definition of normal_loss in torch ops: per-pixel terms in the maps' dtype, the sum in float64, rounded once."""
    n, valid = _normals_torch(depth, alpha, intr, min_alpha)
    dt = depth.dtype
    m = torch.ones_like(depth) if mask is None else (mask.to(dt) if mask.is_floating_point() else (mask != 0).to(dt))
    finite = torch.isfinite(prior).all(0)
    front = torch.tensor([0.0, 0.0, -1.0], dtype=dt, device=depth.device).reshape(3, 1, 1)
    p = torch.where(finite, prior.to(dt), front)
    good = valid & (m > 0) & finite & ((p.detach() * p.detach()).sum(0) > 1e-24)
    p = torch.where(good, p, front)
    unit = p / (p * p).sum(0).sqrt()
    term = 1.0 - (n * unit).sum(0)
    zero = torch.zeros_like(depth)
    total = (torch.where(good, m, zero) * torch.where(good, term, zero)).double().sum() / depth.numel()
    return total.to(dt), good.sum().to(dt).reshape(1).detach()


def _mask_operand(mask):
    """(mask as the kernels read it, mask_kind)"""
    if mask is None:
        return None, 0
    mask = mask.detach().contiguous()
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)                   # the same bytes: no conversion pass
    elif not mask.is_floating_point() and mask.dtype != torch.uint8:
        mask = (mask != 0).view(torch.uint8)            # any other integer: nonzero = 1, as the torch path reads it
    if mask.dtype != torch.uint8:
        mask = mask.float()
    return mask, 2 if mask.dtype == torch.uint8 else 1


class _DepthNormals(torch.autograd.Function):
    """depth_normals on the GPU (csrc/normals.hip): one stencil pass; the backward pass recomputes the normals and gathers."""

    @staticmethod
    def forward(ctx, depth, alpha, intr, rot, min_alpha):
        c = lambda t: t.detach().contiguous().float()
        depth, alpha = c(depth), c(alpha)
        H, W = depth.shape
        out = torch.empty(3, H, W, dtype=torch.float32, device=depth.device)
        _C.family_call("scr_normals_map", H, W, depth, alpha, *intr, None if rot is None else _C.host_array(rot, _C.f32), min_alpha,
                       out, device=depth.device)
        ctx.save_for_backward(depth, alpha)
        ctx.args = (intr, rot, min_alpha)
        return out

    @staticmethod
    def backward(ctx, g_out):
        depth, alpha = ctx.saved_tensors
        intr, rot, min_alpha = ctx.args
        H, W = depth.shape
        g_out = g_out.contiguous().float()
        dd = torch.empty_like(depth) if ctx.needs_input_grad[0] else None
        da = torch.empty_like(alpha) if ctx.needs_input_grad[1] else None
        _C.family_call("scr_normals_map_backward", H, W, depth, alpha, *intr, None if rot is None else _C.host_array(rot, _C.f32),
                       min_alpha, g_out, dd, da, device=depth.device)
        return dd, da, None, None, None


class _NormalLoss(torch.autograd.Function):
    """normal_loss on the GPU (csrc/normals.hip): one stencil pass with a record per workgroup and a one-workgroup fold (float64
    sums in a fixed order), one gather-shaped backward pass; the gradient flows to depth and alpha only."""

    @staticmethod
    def forward(ctx, depth, alpha, prior, mask, intr, min_alpha):
        c = lambda t: t.detach().contiguous().float()
        depth, alpha, prior = c(depth), c(alpha), c(prior)
        mask, kind = _mask_operand(mask)
        H, W = depth.shape
        dev = depth.device
        scratch = _C.scratch(_C.lib.scr_normals_loss_scratch_bytes(H, W), dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        _C.family_call("scr_normals_loss_forward", H, W, depth, alpha, prior, _C.ptr(mask), kind, *intr, min_alpha, scratch, out,
                       device=dev)
        ctx.save_for_backward(depth, alpha, prior, mask)
        ctx.args = (kind, intr, min_alpha)
        stats = out[1:]
        ctx.mark_non_differentiable(stats)
        return out[0], stats

    @staticmethod
    def backward(ctx, g, _):
        depth, alpha, prior, mask = ctx.saved_tensors
        kind, intr, min_alpha = ctx.args
        H, W = depth.shape
        g = g.contiguous().float().reshape(1)
        dd = torch.empty_like(depth) if ctx.needs_input_grad[0] else None
        da = torch.empty_like(alpha) if ctx.needs_input_grad[1] else None
        _C.family_call("scr_normals_loss_backward", H, W, depth, alpha, prior, _C.ptr(mask), kind, *intr, min_alpha, g, dd, da,
                       device=depth.device)
        return dd, da, None, None, None, None


def depth_normals(depth, alpha, cam_or_intrinsics, frame="camera", min_alpha=0.5, return_valid=False):
    """The normal map [3, H, W] that the rasterizer's maps imply (render(aux=True): out["depth"], out["alpha"], both [H, W]):
    unit normals facing the camera at valid pixels, exactly (0, 0, 0) at holes (see the module's definition).
    cam_or_intrinsics: a camera (image_width, image_height, FoVx, FoVy -> intrinsics(cam)) or (fx, fy, cx, cy) in pixels.
    frame="world" multiplies by the camera-to-world rotation cam.world_view_transform[:3, :3] (needs a camera); the rotation
    is a constant of the backward pass, and one that requires grad is refused.  Differentiable with respect to depth and
    alpha.  return_valid=True: also the bool map [H, W] of the valid pixels."""
    if frame not in _FRAMES:
        raise ValueError(f"depth_normals: frame {frame!r} is not one of {list(_FRAMES)}")
    min_alpha = _check_maps("depth_normals", depth, alpha, min_alpha)
    intr = _resolve("depth_normals", cam_or_intrinsics)
    rot = None
    if frame == "world":
        wvt = getattr(cam_or_intrinsics, "world_view_transform", None)
        if wvt is None:
            raise ValueError('depth_normals: frame="world" needs a camera with world_view_transform, not bare intrinsics')
        if wvt.requires_grad and torch.is_grad_enabled():
            raise ValueError("depth_normals: the rotation requires grad, and camera gradients through the normals are not built")
        rot = wvt.detach()[:3, :3]
    if depth.is_cuda:
        n = _DepthNormals.apply(depth, alpha, intr, None if rot is None else [float(v) for v in rot.reshape(-1).tolist()], min_alpha)
        valid = (n.detach() != 0).any(0) if return_valid else None
    else:
        n, valid = _normals_torch(depth.float(), alpha.float(), intr, min_alpha)
        if rot is not None:
            n = torch.einsum("ij,jhw->ihw", rot.to(n.device, n.dtype), n)
    return (n, valid) if return_valid else n


def normal_loss(depth, alpha, prior, cam_or_intrinsics, mask=None, min_alpha=0.5, return_stats=False):
    """Normal supervision on the rasterizer's maps: L = (1 / (H W)) sum_valid mask (1 - n . prior / |prior|), n the normal
    that depth and alpha imply (depth_normals, camera frame).  prior: [3, H, W] in the camera frame (+x right, +y down, +z
    forward; a surface seen head-on is (0, 0, -1)), of any length; a pixel whose prior is not finite or has squared length
    <= 1e-24 is a hole.  mask follows depth_loss: absent, float weights >= 0, or bool / uint8 with nonzero = 1; mask <= 0 is a
    hole.  A hole adds nothing to the loss and gets no gradient through its own normal, whatever it holds; the mean is over
    ALL pixels, so a hole never raises the weight of the others.

    On the GPU this is the fused op of csrc/normals.hip: float64 sums in a fixed order (the same bits run after run), no
    [3, H, W] intermediate, no host read; the gradient flows to depth and alpha.  On CPU tensors, and where prior or mask wants
    a gradient, the same definition runs in torch ops.  return_stats=True: also the detached device tensor (n_valid,)."""
    min_alpha = _check_maps("normal_loss", depth, alpha, min_alpha, prior=(prior, (3,)), mask=(mask, ()))
    intr = _resolve("normal_loss", cam_or_intrinsics)
    wants = torch.is_grad_enabled() and (prior.requires_grad or (mask is not None and mask.requires_grad))
    if depth.is_cuda and not wants:
        loss, stats = _NormalLoss.apply(depth, alpha, prior, mask, intr, min_alpha)
    else:
        loss, stats = _normal_loss_torch(depth.float(), alpha.float(), prior.float(), intr, mask, min_alpha)
    return (loss, stats) if return_stats else loss
