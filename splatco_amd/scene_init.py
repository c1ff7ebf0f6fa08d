"""A scene from a point cloud: GaussianModel.create_from_pcd (scene/gaussian_model.py:472-508, with voxelize_sample,
:447-451) restated for the device.  The reference voxelises with a lexicographic row sort in numpy on the host and takes
the initial scales from `simple_knn._C.distCUDA2`, a native package whose source is NOT in the reference tree.  Its
parity is therefore unpinned in the same sense as the rasterizer's: the semantics below are this
project's specification, tied to a float64 brute force by tests/test_scene_init_host.py.

Semantics, all in binary32 on float32 [N,3] points (float64 input is converted to float32 first, as the reference's
fetchPly delivers float32, scene/dataset_readers.py:107-113):

  dist2      for every point the mean of the squared distances to its 3 nearest OTHER points; an exact duplicate is
             another point, at distance 0.  e = p_j - p_i per component, d = (ex*ex + ey*ey) + ez*ez, the three smallest
             d ascending b0 <= b1 <= b2, result ((b0 + b1) + b2) / 3.0f with a correctly rounded division, no fused
             multiply-add.  The three smallest VALUES are unique even where neighbours tie, so the result does not
             depend on tie-breaking.  N < 4 is a ValueError.
  voxelize   q = rint(p / v) (float32 division by float32(v), round half to even), duplicate rows of q dropped, the
             survivors ordered lexicographically by (qx, qy, qz) -- what np.unique(axis=0) returns -- output
             float32(q) * float32(v).  The reference's np.random.shuffle before it has no effect on the result and is
             not reproduced.

Device tensors go through the C-ABI (csrc/scene_init.hip; dist2 buckets its points with knn_grid.py); CPU tensors take a plain torch branch of the same arithmetic
(the pattern of densify._knn_indices), which is what the CPU-only tests exercise."""
import ctypes as C

import numpy as np
import torch

from .densify import inverse_sigmoid
from .knn_grid import bounds, buckets

_PACK_BITS = 21                 # bits per axis of the packed voxel key


def _points(points):
    pts = torch.as_tensor(points).detach()
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be [N,3], got {tuple(pts.shape)}")
    if pts.shape[0] >= 1 << 31:
        raise ValueError("more than 2^31 - 1 points")
    return pts.float().contiguous()


# ------------------------------------------------------------------ dist2
def _dist2_device(pts):
    from . import _C
    N, dev = pts.shape[0], pts.device
    grid, spts, order, cell_start = buckets(pts)
    out = torch.empty(N, dtype=torch.float32, device=dev)
    _C.call("scr_knn3_dist2", N, grid, spts, order, cell_start, out)
    return out


def _dist2_host(pts):
    N = pts.shape[0]
    out = torch.empty(N, dtype=torch.float32, device=pts.device)
    x, y, z = pts[:, 0].contiguous(), pts[:, 1].contiguous(), pts[:, 2].contiguous()
    step = max(1, (1 << 23) // N)
    for s in range(0, N, step):
        e = min(s + step, N)
        ex, ey, ez = x[None, :] - x[s:e, None], y[None, :] - y[s:e, None], z[None, :] - z[s:e, None]
        d = (ex * ex + ey * ey) + ez * ez                     # separate torch ops: nothing is contracted
        d[torch.arange(e - s), torch.arange(s, e)] = float("inf")   # the point itself; its duplicates stay
        b = d.topk(3, dim=1, largest=False, sorted=True).values
        t = (b[:, 0] + b[:, 1]) + b[:, 2]
        out[s:e] = t / torch.full_like(t, 3.0)               # a true division of every element, as in voxelize
    return out


def dist2(points):
    """simple_knn's distCUDA2: [N] float32, the mean squared distance of every point to its 3 nearest other points
    (module docstring for the exact arithmetic).  float64 input is converted to float32 first."""
    pts = _points(points)
    if pts.shape[0] < 4:
        raise ValueError("dist2 needs at least 4 points")
    if pts.is_cuda:
        return _dist2_device(pts)
    bounds(pts)
    return _dist2_host(pts)


# ------------------------------------------------------------------ voxelize
def _voxel_range(pts, voxel_size):
    """(float32 v, lo[3], extent[3]) of q = rint(p / v): rint(x / v) is monotone in x, so the bounding box gives both."""
    v = np.float32(voxel_size)
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f"voxel_size must be positive and finite in float32, got {voxel_size}")
    lo, hi = bounds(pts)
    with np.errstate(over="ignore"):
        qlo, qhi = np.rint(lo / v), np.rint(hi / v)
    if not (np.isfinite(qlo).all() and np.isfinite(qhi).all()) or max(np.abs(qlo).max(), np.abs(qhi).max()) >= 2.0 ** 31:
        raise ValueError(f"voxel_size {voxel_size} is too small for this cloud: rint(x / v) does not fit int32")
    qlo, qhi = qlo.astype(np.int64), qhi.astype(np.int64)
    return v, qlo, qhi - qlo


def _unique_rows(q, v):
    """The slower path (an axis spans 2^21 voxels or more): three integer columns, sorted lexicographically."""
    u = torch.unique(q, dim=0)
    return u.float() * torch.full((), float(v), dtype=torch.float32, device=q.device)


def _voxelize_device(pts, v, lo, packed):
    from . import _C
    N, dev = pts.shape[0], pts.device
    lo_host = _C.host_array([int(a) for a in lo], _C.i32)
    keys = torch.empty((N,) if packed else (N, 3), dtype=torch.long, device=dev)
    _C.call("scr_voxel_keys", N, pts, float(v), lo_host, int(packed), keys)
    if not packed:
        return _unique_rows(keys, v)
    skeys = torch.sort(keys).values
    del keys
    scratch = _C.scratch(_C.lib.scr_voxel_unique_scratch_bytes(N), dev)
    cnt = C.c_int64(0)
    _C.call("scr_voxel_unique_plan", N, skeys, scratch, C.byref(cnt))
    out = torch.empty(cnt.value, 3, dtype=torch.float32, device=dev)
    _C.call("scr_voxel_unique_run", N, skeys, scratch, float(v), lo_host, out)
    return out


def _voxelize_host(pts, v, lo, packed):
    # the divisor as a full tensor: a true float32 division of every element, no scalar shortcut
    q = torch.round(pts / torch.full_like(pts, float(v))).long()
    if not packed:
        return _unique_rows(q, v)
    q = q - torch.as_tensor(lo, dtype=torch.long)
    key = (q[:, 0] << (2 * _PACK_BITS)) | (q[:, 1] << _PACK_BITS) | q[:, 2]
    key = torch.unique_consecutive(torch.sort(key).values)
    mask = (1 << _PACK_BITS) - 1
    u = torch.stack([key >> (2 * _PACK_BITS), (key >> _PACK_BITS) & mask, key & mask], dim=1) + torch.as_tensor(lo, dtype=torch.long)
    return u.float() * torch.full((), float(v), dtype=torch.float32)


def voxelize(points, voxel_size, _force_rows=False):
    """The reference's voxelize_sample, `np.unique(np.round(points / v), axis=0) * v`, value for value in the same order:
    [M,3] float32 on the device of `points` (module docstring).  float64 input is converted to float32 first.
    _force_rows: take the three-column path whatever the extent (tests compare the two paths)."""
    pts = _points(points)
    if pts.shape[0] == 0:
        return pts.new_zeros(0, 3)
    v, lo, ext = _voxel_range(pts, voxel_size)
    packed = bool((ext < (1 << _PACK_BITS)).all()) and not _force_rows
    return (_voxelize_device if pts.is_cuda else _voxelize_host)(pts, v, lo, packed)


# ------------------------------------------------------------------ create_from_pcd
@torch.no_grad()
def create_from_pcd(model, points, voxel_size, ratio=1):
    """scene/gaussian_model.py:472-508 on `model` (an AnchorGaussianModel), on the model's device, quirks kept.
    Returns (voxel size used, points taken, anchors made); the voxel size is also stored as `model.voxel_size` -- hand
    the same value to AnchorDensifier(model, opt, voxel_size=...)."""
    dev = model._anchor.device
    pts = _points(torch.as_tensor(points)[::ratio]).to(dev)                       # :474
    if voxel_size <= 0:
        # :476-480 -- the median of the SQUARED 3-NN distances of the raw cloud, used as a length (the reference's
        # quirk); kthvalue(int(N * 0.5)) is the lower median for even N and one below the median for odd N
        init_dist = dist2(pts)
        voxel_size = torch.kthvalue(init_dist, int(init_dist.shape[0] * 0.5)).values.item()
    anchors = voxelize(pts, voxel_size)                                            # :487-488
    M, k = anchors.shape[0], model.n_offsets
    offsets = torch.zeros(M, k, 3, device=dev)
    anchor_feat = torch.zeros(M, model.feat_dim, device=dev)
    d = torch.clamp_min(dist2(anchors), 0.0000001)                                 # :494
    scales = torch.log(torch.sqrt(d))[..., None].repeat(1, 6)                      # :495
    opacities = inverse_sigmoid(0.1 * torch.ones(M, 1, dtype=torch.float, device=dev))     # :500
    model.set_anchors(anchors, offsets, anchor_feat, scales, rotation=None, opacity=opacities)   # identity rotation, :497-498
    model.voxel_size = voxel_size
    return voxel_size, pts.shape[0], M
