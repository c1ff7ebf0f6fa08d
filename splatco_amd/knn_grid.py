"""The host half of the grid-bucketed nearest-neighbour search (csrc/knn_grid.h): the bounding box, the cell size with the
slack the search's stop test needs, and the points sorted by cell.  densify._knn_indices (scr_knn) and scene_init.dist2
(scr_knn3_dist2) both bucket their points here, so the one policy "how points are bucketed and when the search may
stop" holds for both."""
import numpy as np
import torch

_MAX_AXIS_CELLS = 1 << 18       # per-axis bound of the grid: keeps the cell function's rounding below 1/4 cell


def bounds(pts):
    """(min[3], max[3]) as float32 numpy; non-finite coordinates are a ValueError (torch's amin / amax propagate NaN;
    the device reduction drops it and raises a flag instead)."""
    if pts.is_cuda:
        from . import _C
        N, dev = pts.shape[0], pts.device
        out = torch.empty(7, dtype=torch.float32, device=dev)
        scratch = _C.scratch(_C.lib.scr_points_bounds_scratch_bytes(N), dev)
        _C.call("scr_points_bounds", N, pts, scratch, out)
        out = out.cpu().numpy()
        lo, hi, bad = out[:3], out[3:6], out[6] > 0
    else:
        lo, hi = torch.aminmax(pts, dim=0)
        lo, hi, bad = lo.numpy(), hi.numpy(), False
    if bad or not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("points has non-finite coordinates")
    return lo, hi


def grid(lo, hi, N, h=None, per_cell=2.0):
    """Uniform grid over the bounding box: cell size `h` (default: about `per_cell` points per cell of a cloud that fills
    the box), at most 8 N + 64 (and 2^31 - 2) cells and 2^18 per axis.  Returns (h as float32, [nx, ny, nz], slack)."""
    ext = (hi.astype(np.float64) - lo.astype(np.float64))
    m = float(ext.max())
    if m <= 0.0:                                     # every point is the same point
        return np.float32(1.0), [1, 1, 1], 0.0
    ext = np.maximum(ext, m * 1e-6)
    if h is None:
        h = float((ext.prod() * per_cell / N) ** (1.0 / 3.0))
    h = max(h, m / (_MAX_AXIS_CELLS - 2))
    cap = min(8.0 * N + 64, 2.0 ** 31 - 2)           # (cell_start is int32-indexed by the kernel's host checks)
    for _ in range(200):                             # flat / degenerate clouds: bound the cell count
        n = np.maximum(np.ceil(ext / h), 1.0)
        over = float(n.prod()) / cap
        if over <= 1.0:
            break
        h *= max(over ** (1.0 / 3.0), 1.02)
    h = np.float32(h)
    n = [int(v) for v in np.maximum(np.ceil(ext / float(h)), 1.0)]
    # The search kernel assumes that a point closer than (r + f) * h to the query lies within r cells of the query's
    # cell.  The cell function t = (x - x0) * (1 / h) carries up to ~3 roundings of relative size 2^-24 on t <= max(n),
    # for the query and for the point: 8 * max(n) * 2^-23 cells bounds both with room; 1e-4 covers the rounding of the
    # squared distances compared.
    slack = float(h) * (8.0 * max(n) * 2.0 ** -23 + 1e-4)
    return h, n, slack


def cell_order(pts, grid_host):
    """The order that walks the device points [N,3] float32 by their CLAMPED cell key under ANOTHER set's grid descriptor
    (`buckets(...)[0]`): int64 [N].  What a search from one set into another sorts its queries by (surface_eval.nearest)."""
    from . import _C
    keys = torch.empty(pts.shape[0], dtype=torch.long, device=pts.device)
    _C.call("scr_knn_cell_keys", pts.shape[0], grid_host, pts, keys)
    return torch.sort(keys).indices


def buckets(pts):
    """The device points [N,3] float32 bucketed for scr_knn / scr_knn3_dist2: (grid_host, points in cell order, their
    original indices, cell_start)."""
    from . import _C
    N, dev = pts.shape[0], pts.device
    lo, hi = bounds(pts)
    keys = torch.empty(N, dtype=torch.long, device=dev)
    h = None
    for attempt in range(2):
        h, (nx, ny, nz), slack = grid(lo, hi, N, h)
        ncell = nx * ny * nz
        grid_host = _C.host_array((float(lo[0]), float(lo[1]), float(lo[2]), float(h), nx, ny, nz, slack), _C.f32)
        _C.call("scr_knn_cell_keys", N, grid_host, pts, keys)
        counts = torch.bincount(keys, minlength=ncell)
        if attempt:
            break
        # A cloud that is a surface in a mostly empty box fills few cells with many points each, and the search
        # is quadratic in that.  Re-bucket once with the cell size a sheet wants (occupancy falls with h^2 there),
        # as far as the bound on the cell count lets it.
        occupancy = N / max(int((counts > 0).sum()), 1)
        if occupancy <= 6.0:
            break
        h = float(h) * (3.0 / occupancy) ** 0.5
    cell_start = torch.zeros(ncell + 1, dtype=torch.int32, device=dev)
    cell_start[1:] = counts.cumsum(0)
    del counts
    order = torch.sort(keys).indices
    return grid_host, pts.index_select(0, order), order, cell_start
