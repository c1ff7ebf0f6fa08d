"""The definition of splatco_amd.filter3d restated in torch ops (include/splatco_raster.h, scr_filter3d_*): what
csrc/filter3d.hip is checked against.  TEST INFRASTRUCTURE ONLY; nothing here imports the native library.

Every function takes a `dtype`: on float64 it is the reference, on float32 the "framework chain" whose own error against the
float64 result sets the bar of the kernel (f64_refs.bar).  The packed cameras [C, 16] are data: they are converted to `dtype`
as they are (the float32 table the kernel reads is exact in float64)."""
import math

import torch

Z_NEAR = 0.2            # as the kernel compares: with the float32 constant, in every dtype
INF = float("inf")


def decisions(points, cameras, dtype=torch.float64):
    """(observed [N, C] bool, depth / focal [N, C], margin [N, C]) of every point against every camera.  margin: the
    smallest relative distance of the three comparisons from their bounds (0 = on a bound); NaN-free for finite points."""
    x = points.detach().to("cpu", dtype)
    k = cameras.detach().to("cpu", dtype)
    R, t = k[:, :12].reshape(-1, 3, 4)[:, :, :3], k[:, :12].reshape(-1, 3, 4)[:, :, 3]
    p = torch.einsum("cij,nj->nci", R, x) + t[None]
    px, py, pz = p.unbind(-1)
    tx, ty, focal = k[None, :, 12], k[None, :, 13], k[None, :, 14]
    znear = torch.tensor(Z_NEAR, dtype=torch.float32).to(dtype)
    finite = torch.isfinite(x).all(dim=1, keepdim=True)
    seen = finite & (pz > znear) & (px.abs() <= tx * pz) & (py.abs() <= ty * pz)
    rel = lambda a, b: (a - b).abs() / torch.maximum(a.abs(), b.abs()).clamp_min(1e-30)
    margin = torch.minimum(rel(pz, znear.expand_as(pz)), torch.minimum(rel(px.abs(), tx * pz), rel(py.abs(), ty * pz)))
    return seen, pz / focal, margin


def sampling_distance(points, cameras, dtype=torch.float64):
    """m [N]: min over the observing cameras of p.z / focal, +inf without one."""
    seen, rate, _ = decisions(points, cameras, dtype)
    return torch.where(seen, rate, torch.full_like(rate, INF)).amin(dim=1) if rate.shape[0] else rate.new_zeros(0)


def filter_from_distance(m, variance=0.2):
    seen = torch.isfinite(m)
    f = m * math.sqrt(variance)
    if not bool(seen.any()):
        return torch.zeros_like(m)
    return torch.where(seen, f, f[seen].max())


def compute_filter_3d(points, cameras, variance=0.2, dtype=torch.float64):
    return filter_from_distance(sampling_distance(points, cameras, dtype), variance)


def upstream_loop(points, cameras, variance=0.2):
    """Mip-Splatting's compute_3D_filter as upstream writes it: a loop of torch ops per camera on the points' device and
    dtype (pixel coordinates against the image enlarged by 15 % per side), one focal length for all cameras (the last)."""
    xyz = points
    distance = torch.full((xyz.shape[0],), 100000.0, device=xyz.device, dtype=xyz.dtype)
    valid_points = torch.zeros(xyz.shape[0], device=xyz.device, dtype=torch.bool)
    focal = 0.0
    for row in cameras.to(xyz.device, xyz.dtype):
        R, T = row[:12].reshape(3, 4)[:, :3], row[:12].reshape(3, 4)[:, 3]
        xyz_cam = xyz @ R.transpose(0, 1) + T[None, :]
        valid_depth = xyz_cam[:, 2] > 0.2
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z = torch.clamp(z, min=0.001)
        in_screen = torch.logical_and(torch.logical_and(x / z >= -row[12], x / z <= row[12]),
                                      torch.logical_and(y / z >= -row[13], y / z <= row[13]))
        valid = torch.logical_and(valid_depth, in_screen)
        distance[valid] = torch.min(distance[valid], z[valid])
        valid_points = torch.logical_or(valid_points, valid)
        focal = row[14]
    distance[~valid_points] = distance[valid_points].max()
    return distance / focal * (variance ** 0.5)


def row_of_gaussian(mask, k):
    """[P] int64: the row (visible anchor) every kept candidate of mask [V k] came from, in order."""
    return torch.nonzero(mask.reshape(-1).to(torch.bool)).squeeze(1) // k


def apply(scaling, opacity, f_gauss, dtype=torch.float64):
    """(scaling' [P,3], opacity' [P,1]) for per-Gaussian filter values f_gauss [P]; differentiable in scaling and opacity.
    Rows with f == 0 pass through."""
    s, o, f = scaling.to(dtype), opacity.to(dtype).reshape(-1, 1), f_gauss.detach().to(dtype).reshape(-1, 1)
    t = torch.sqrt(s * s + f * f)
    r = s / torch.where(f == 0, torch.ones_like(t), t)
    coef = r[:, 0:1] * r[:, 1:2] * r[:, 2:3]
    on = f != 0
    return torch.where(on, t, s), torch.where(on, o * coef, o)


def apply_backward(scaling, opacity, f_gauss, g_scaling, g_opacity, dtype=torch.float64):
    """The closed-form gradients of apply(): ds_i = g_s'_i r_i + g_o' o prod_{j != i} r_j f^2 / t_i^3, do = g_o' coef; a
    missing upstream gradient is zero; rows with f == 0 get the upstream gradients."""
    s, o, f = scaling.detach().to(dtype), opacity.detach().to(dtype).reshape(-1, 1), f_gauss.detach().to(dtype).reshape(-1, 1)
    gs = torch.zeros_like(s) if g_scaling is None else g_scaling.to(dtype)
    go = torch.zeros_like(o) if g_opacity is None else g_opacity.to(dtype).reshape(-1, 1)
    on = f != 0
    t = torch.where(on, torch.sqrt(s * s + f * f), torch.ones_like(s))
    r = s / t
    others = torch.stack((r[:, 1] * r[:, 2], r[:, 0] * r[:, 2], r[:, 0] * r[:, 1]), dim=1)
    ds = gs * r + go * o * others * (f * f) / (t * t * t)
    do = go * (r[:, 0:1] * r[:, 1:2] * r[:, 2:3])
    return torch.where(on, ds, gs), torch.where(on, do, go)
