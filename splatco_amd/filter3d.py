"""Mip-Splatting's 3D smoothing filter (host side of csrc/filter3d.hip): the world-space half of Mip-Splatting, next to the
rasterizer's antialiased mode (the screen-space half).

Every anchor gets a lower size limit f from the highest sampling rate at which a training camera observed it, and every
neural Gaussian expanded from it is widened to sqrt(s^2 + f^2) with its opacity scaled by the ratio of the volumes.  The
definition (normative; include/splatco_raster.h scr_filter3d_* and tests/filter3d_ref.py restate it), all float32 except
that the packed cameras are formed on the host in float64 and rounded once:

  packed camera   16 floats: rows 0..2 of the 3x4 [R | t] of W2C = world_view_transform^T, tx = 1.3 tan(FoVx / 2)
                  (= 0.65 W / fx), ty = 1.3 tan(FoVy / 2), focal = max(fx, fy) with fx = W / (2 tan(FoVx / 2)), 0
  observed        p = R x + t; x finite, p.z > 0.2, |p.x| <= tx p.z and |p.y| <= ty p.z (upstream's test: z > 0.2 and the
                  pixel inside the image enlarged by 15 % per side, bounds inclusive)
  m(x)            min over the observing cameras of p.z / focal, +inf when there is none: no order, the same bits for every
                  order of the cameras
  f(x)            sqrt(variance) m(x) for an observed point; the largest f of any observed point for an unobserved one; 0
                  everywhere when no point is observed.  With equal focal lengths upstream's compute_3D_filter exactly,
                  with unequal ones each camera's own rate.  No gradient.
  apply           t_i = sqrt(s_i^2 + f^2), r_i = s_i / t_i: s'_i = t_i, o' = o r_0 r_1 r_2; rows with f == 0 pass through
"""
import math
import weakref

import torch

from . import _C

CAMERA_FLOATS = 16


def pack_cameras(views):
    """[C, 16] float32 (on the host): one packed row per camera of `views` (objects with world_view_transform, FoVx, FoVy,
    image_width, image_height).  Formed in float64, rounded once.  ValueError for a camera with a non-finite entry."""
    rows = []
    for i, v in enumerate(views):
        w2c = v.world_view_transform.detach().to("cpu", torch.float64).transpose(0, 1)
        if not (math.isfinite(float(v.FoVx)) and math.isfinite(float(v.FoVy))):
            raise ValueError(f"pack_cameras: camera {i} has a non-finite entry")
        tanx, tany = math.tan(float(v.FoVx) * 0.5), math.tan(float(v.FoVy) * 0.5)
        fx, fy = float(v.image_width) / (2.0 * tanx), float(v.image_height) / (2.0 * tany)
        row = torch.cat([w2c[:3, :].reshape(12), torch.tensor([1.3 * tanx, 1.3 * tany, max(fx, fy), 0.0], dtype=torch.float64)])
        if not bool(torch.isfinite(row).all()):
            raise ValueError(f"pack_cameras: camera {i} has a non-finite entry")
        rows.append(row)
    if not rows:
        raise ValueError("pack_cameras: no cameras")
    return torch.stack(rows).float().contiguous()


def _packed(cameras, device):
    if not isinstance(cameras, torch.Tensor):
        cameras = pack_cameras(cameras)
    if cameras.dim() != 2 or cameras.shape[0] < 1 or cameras.shape[1] != CAMERA_FLOATS:
        raise ValueError(f"filter3d: cameras {tuple(cameras.shape)} is not a [C >= 1, {CAMERA_FLOATS}] table (pack_cameras)")
    return cameras.detach().to(device, torch.float32).contiguous()


def sampling_distance(points, cameras):
    """m [N] float32 for device points [N, 3]; cameras: a list of views or a packed [C, 16] table.  csrc/filter3d.hip:
    one point per lane, the cameras read as wave-uniform data; any C >= 1."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"sampling_distance: points {tuple(points.shape)} is not [N, 3]")
    if not points.is_cuda:
        raise RuntimeError("sampling_distance needs device tensors: it is a HIP kernel (csrc/filter3d.hip) and has no CPU path")
    points = points.detach().contiguous().float()
    cameras = _packed(cameras, points.device)
    m = torch.empty(points.shape[0], dtype=torch.float32, device=points.device)
    _C.call("scr_filter3d_distance", points.shape[0], _C.ptr(points), cameras.shape[0], cameras, _C.ptr(m), device=points.device)
    return m


def compute_filter_3d(points, cameras, variance=0.2):
    """f [N] float32 (no gradient): sqrt(variance) m for observed points, the observed maximum for the others, 0 everywhere
    when nothing is observed."""
    m = sampling_distance(points, cameras)
    if m.numel() == 0:
        return m
    seen = torch.isfinite(m)
    f = m * math.sqrt(float(variance))
    top = torch.where(seen, f, torch.zeros_like(f)).amax()          # 0 when no point is observed
    return torch.where(seen, f, top)


class _ApplyFilter3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling, opacity, row_filter, out_index, k):
        ctx.set_materialize_grads(False)
        c = lambda t: t.detach().contiguous().float()
        scaling, opacity, row_filter = c(scaling), c(opacity), c(row_filter)
        P, V = scaling.shape[0], row_filter.shape[0]
        s_out, o_out = torch.empty_like(scaling), torch.empty_like(opacity)
        _C.call("scr_filter3d_apply", V, k, P, _C.ptr(out_index), _C.ptr(row_filter), _C.ptr(scaling), _C.ptr(opacity),
                _C.ptr(s_out), _C.ptr(o_out), device=scaling.device)
        ctx.save_for_backward(scaling, opacity, row_filter, out_index)
        ctx.k = k
        return s_out, o_out

    @staticmethod
    def backward(ctx, g_s, g_o):
        scaling, opacity, row_filter, out_index = ctx.saved_tensors
        if g_s is None and g_o is None:
            return None, None, None, None, None
        c = lambda t: None if t is None else t.contiguous().float()
        g_s, g_o = c(g_s), c(g_o)
        d_s, d_o = torch.empty_like(scaling), torch.empty_like(opacity)
        _C.call("scr_filter3d_apply_backward", row_filter.shape[0], ctx.k, scaling.shape[0], _C.ptr(out_index), _C.ptr(row_filter),
                _C.ptr(scaling), _C.ptr(opacity), _C.ptr(g_s), _C.ptr(g_o), _C.ptr(d_s), _C.ptr(d_o), device=scaling.device)
        return d_s, d_o, None, None, None


def apply_filter_3d(scaling, opacity, row_filter, mask, k):
    """(scaling' [P,3], opacity' [P,1]) of the P neural Gaussians that expand_compact kept of V anchors with k offsets each.
    row_filter [V]: the filter value of every row's anchor (no gradient); mask [V k]: expand_compact's mask, whose
    `_scr_out_index` (each candidate's position among the Gaussians, -1 = dropped) says which row a Gaussian came from --
    where the mask carries none (a test's own expand hook) it is formed from a cumulative sum.  One pass over the V k
    candidates per direction (csrc/filter3d.hip); the gradient flows to scaling and opacity."""
    k = int(k)
    V, P = row_filter.shape[0], scaling.shape[0]
    if not scaling.is_cuda:
        raise RuntimeError("apply_filter_3d needs device tensors: it is a HIP kernel (csrc/filter3d.hip) and has no CPU path")
    if k < 1 or mask.shape != (V * k,) or scaling.shape != (P, 3) or opacity.numel() != P or row_filter.dim() != 1:
        raise ValueError(f"apply_filter_3d: scaling {tuple(scaling.shape)}, opacity {tuple(opacity.shape)}, row_filter "
                         f"{tuple(row_filter.shape)}, mask {tuple(mask.shape)} do not fit k = {k}")
    out_index = getattr(mask, "_scr_out_index", None)
    if out_index is None:
        kept = mask.to(torch.bool)
        out_index = torch.where(kept, torch.cumsum(kept, 0) - 1, -1).to(torch.int32)
    return _ApplyFilter3D.apply(scaling, opacity, row_filter, out_index, k)


class Filter3D:
    """The filter of one model over one set of training cameras.  `values` [N] follows `update(pc)`; it must be recomputed
    whenever the anchors change (`stale(pc)`), and `every` iterations while they train (train_step.collaborative_step does
    both).  The filter is a function of the parameters and the cameras alone, so every rank computes the same values.
    It is not stored with the model: after loading, recompute it from the cameras."""

    def __init__(self, views, variance=0.2, every=100):
        self.cameras = views if isinstance(views, torch.Tensor) else pack_cameras(views)
        self.variance, self.every = float(variance), int(every)
        self.values = None
        self._anchor = None

    def update(self, pc):
        with torch.no_grad():
            anchor = pc.get_anchor
            self.cameras = _packed(self.cameras, anchor.device)          # moved to the model's device once
            self.values = compute_filter_3d(anchor, self.cameras, self.variance)
        # WHICH parameter and which memory, not how long: sort_anchors permutes the rows and keeps N (the densifier's
        # replaces the parameter object, the model's own gives the same object new memory)
        self._anchor = (weakref.ref(pc._anchor), pc._anchor.data_ptr())
        return self.values

    def stale(self, pc):
        """True until update(), and again once pc._anchor is no longer the parameter object (and memory) update() read."""
        if self.values is None or self._anchor is None:
            return True
        ref, address = self._anchor
        return ref() is not pc._anchor or pc._anchor.data_ptr() != address

    def due(self, pc, iteration=None):
        return self.stale(pc) or (iteration is not None and self.every > 0 and iteration % self.every == 0)


def anchor_values(filter_3d, pc):
    """The [N] filter tensor behind a render()'s `filter_3d` argument: a Filter3D's values or the tensor itself, checked
    against the model."""
    n, dev = pc.get_anchor.shape[0], pc.get_anchor.device
    if isinstance(filter_3d, Filter3D):
        if filter_3d.stale(pc):
            raise ValueError("filter_3d: the Filter3D is stale (never updated, or the model's anchors were replaced by "
                             "adjust_anchor / prune_anchor / sort_anchors since): call filter_3d.update(pc) first")
        return filter_3d.values
    if not isinstance(filter_3d, torch.Tensor):
        raise TypeError(f"filter_3d: a Filter3D or an [N] tensor, not {type(filter_3d).__name__}")
    if filter_3d.shape != (n,) or filter_3d.device != dev:
        raise ValueError(f"filter_3d: tensor {tuple(filter_3d.shape)} on {filter_3d.device} does not match the model's {n} "
                         f"anchors on {dev}: recompute it with compute_filter_3d(pc.get_anchor, cameras)")
    return filter_3d.detach().float()
