"""Mesh evaluation on the device: area-weighted surface sampling, the exact nearest neighbour from one point set into another,
and the scores the geometric branch is judged by -- accuracy, completeness and Chamfer (DTU), precision, recall and F-score at
a threshold (Tanks and Temples) -- without Open3D or scipy (host side of csrc/surfeval.hip).

The definitions (normative; include/splatco_surfeval.h and tests/surfeval_ref.py restate them):

Sampling.  For face f with corners p0, p1, p2 (float32 widened to binary64): e1 = p1 - p0, e2 = p2 - p0, c = e1 x e2,
A = 0.5 * sqrt((cx cx + cy cy) + cz cz).  u32(seed, f, c) = mix(mix(mix(seed) ^ f) ^ c) in uint32 with mix(x): x ^= x >> 16;
x *= 0x21f0aaad; x ^= x >> 15; x *= 0x735a2d97; x ^= x >> 15, and U = (double)u32 * 2^-32.  The face gets
n_f = floor(A * density + U(seed, f, 0)) samples (stochastic rounding: the expected count is A * density, slivers are not
over-sampled), 0 where A is not finite.  Samples lie face by face in ascending f, then ascending j; sample j of face f has
r1 = U(seed, f, 1 + 2 j), r2 = U(seed, f, 2 + 2 j), both replaced by 1 - r where r1 + r2 > 1, and is (p0 + r1 e1) + r2 e2 per
coordinate in binary64, rounded to float32 once.  The same seed gives the same bits.

Nearest neighbour.  d(i, j) = (ex ex + ey ey) + ez ez in float32, e = target_j - query_i; cap2 = +inf without max_dist,
otherwise m * m with m = (float)max_dist; dist2[i] = min(cap2, min_j d(i, j)); index[i] = the smallest j with
d(i, j) == dist2[i], -1 where there is none.  Unique, so a brute-force float32 loop is the reference bit for bit.  A query may
lie anywhere: the search clips every loop to the target's grid, and a query further than max_dist from it costs nothing.

Score.  Per direction d = sqrt((double)dist2), mean = sum d / n with the sum in binary64 in one fixed order, and for each of up
to 8 thresholds t the count of d <= (double)(float)t.  accuracy = mean(pred -> gt), completeness = mean(gt -> pred), chamfer =
(accuracy + completeness) / 2; precision = count(pred -> gt) / Np, recall = count(gt -> pred) / Ng, fscore = 2 P R / (P + R),
0 where P + R = 0.

    points, face_index = sample_surface(vertices, faces, spacing=0.01)
    dist2, index = nearest(points, gt_points, max_dist=0.2)
    res = evaluate_mesh(vertices, faces, gt_points, spacing=0.01, thresholds=(0.02, 0.05))
    write_mesh_results(model_dir, res)

Not built: point-to-triangle distances, observation masks, ICP alignment and crop volumes, voxel down-sampling, normal
consistency, gradients.

Every launch of the family goes through _C.family_call.  There is no CPU path: a CPU tensor is a ValueError.  Shapes, dtypes and
sizes are checked first, devices next, values (the face index range, finite coordinates) last, all before anything of the
family is launched."""
import json
import math
import os

import numpy as np
import torch

from . import _C, knn_grid
from .mesh import _check_mesh, _device_only, _faces_shape, _vertices_shape

THREADS = 256                   # workgroup size of every kernel of the family (SE_THREADS)
MAX_THRESHOLDS = _C.SURFEVAL_MAX_THRESHOLDS


def _points_shape(fn, name, t):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{fn}: {name} is not a tensor")
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32:
        raise ValueError(f"{fn}: {name} {tuple(t.shape)} {t.dtype} is not a float32 [N, 3] tensor")
    if t.shape[0] >= 2 ** 31:
        raise ValueError(f"{fn}: {name} has {t.shape[0]} points, not below 2^31")


def _finite(fn, name, pts):
    if pts.shape[0]:
        try:
            knn_grid.bounds(pts)
        except ValueError:
            raise ValueError(f"{fn}: {name} has non-finite coordinates") from None


def _real(fn, name, x, least_open=None):
    """x as a float: a finite number, > 0 (least_open=0) or >= 0 (None)."""
    if isinstance(x, bool) or not isinstance(x, (int, float, np.floating, np.integer)) or not math.isfinite(x) \
            or (x <= 0 if least_open is not None else x < 0):
        raise ValueError(f"{fn}: {name} = {x!r} must be a finite number {'> 0' if least_open is not None else '>= 0'}")
    return float(x)


def _thresholds(fn, thresholds):
    if isinstance(thresholds, (int, float, np.floating, np.integer)) and not isinstance(thresholds, bool):
        thresholds = (thresholds,)
    thresholds = [_real(fn, "threshold", t) for t in thresholds]
    if len(thresholds) > MAX_THRESHOLDS:
        raise ValueError(f"{fn}: {len(thresholds)} thresholds, at most {MAX_THRESHOLDS}")
    if any(t > 3.4e38 for t in thresholds):
        raise ValueError(f"{fn}: a threshold is beyond float32")
    return thresholds


def _max_dist(fn, max_dist):
    if max_dist is None:
        return -1.0
    m = _real(fn, "max_dist", max_dist)
    if m > 1.8e19:
        raise ValueError(f"{fn}: max_dist = {max_dist!r}: its square is beyond float32; pass None for no cap")
    return m


def sample_surface(vertices, faces, spacing=None, density=None, seed=0):
    """-> (points [Ns, 3] float32, face_index [Ns] int32) on the device: `density` samples per unit area (= 1 / spacing^2; give
    exactly one of the two), placed as the module's definition says.  vertices [Nv, 3] float32 and faces [Nf, 3] int32 or
    int64 on the GPU.  Three host reads: the index range, the finite check, Ns."""
    fn = "sample_surface"
    if (spacing is None) == (density is None):
        raise ValueError(f"{fn}: give exactly one of spacing and density")
    if density is None:
        s2 = _real(fn, "spacing", spacing, 0) ** 2
        if s2 == 0.0 or not math.isfinite(1.0 / s2):
            raise ValueError(f"{fn}: spacing = {spacing!r} is too small")
        density = 1.0 / s2
    density = _real(fn, "density", density, 0)
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 32:
        raise ValueError(f"{fn}: seed = {seed!r} must be an int in 0 .. 2^32 - 1")
    vertices, faces, _ = _check_mesh(fn, vertices, faces)
    _finite(fn, "vertices", vertices)
    dev, nf = vertices.device, faces.shape[0]
    none = torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    if nf == 0:
        return none
    counts = torch.empty(nf, dtype=torch.int64, device=dev)
    _C.family_call("scr_surfeval_face_counts", nf, vertices, faces, density, seed, counts, device=dev)
    ends = torch.cumsum(counts, 0)                          # integers only: no float reaches the prefix
    ns = int(ends[-1])
    if ns >= 2 ** 31:
        raise ValueError(f"{fn}: {ns} samples or more, not below 2^31: lower the density")
    if ns == 0:
        return none
    points = torch.empty(ns, 3, dtype=torch.float32, device=dev)
    face_index = torch.empty(ns, dtype=torch.int32, device=dev)
    _C.family_call("scr_surfeval_sample", nf, ns, vertices, faces, ends, seed, points, face_index, device=dev)
    return points, face_index


def _check_pair(fn, a_name, a, b_name, b, a_least=0):
    _points_shape(fn, a_name, a)
    _points_shape(fn, b_name, b)
    for name, t, least in ((a_name, a, a_least), (b_name, b, 1)):
        if t.shape[0] < least:
            raise ValueError(f"{fn}: {name} is empty")
    _device_only(fn, a_name, a)
    _device_only(fn, b_name, b)
    if a.device != b.device:
        raise ValueError(f"{fn}: {a_name} is on {a.device}, {b_name} on {b.device}")
    return a.detach().contiguous(), b.detach().contiguous()


def _nearest(query, target, max_dist):
    """Checked operands, finite coordinates."""
    nq, nt, dev = query.shape[0], target.shape[0], query.device
    dist2 = torch.empty(nq, dtype=torch.float32, device=dev)
    index = torch.empty(nq, dtype=torch.int32, device=dev)
    if nq == 0:
        return dist2, index
    grid_host, sorted_target, target_id, cell_start = knn_grid.buckets(target)
    query_id = knn_grid.cell_order(query, grid_host)
    _C.family_call("scr_surfeval_nearest", nq, nt, grid_host, query.index_select(0, query_id), query_id, sorted_target, target_id,
                   cell_start, max_dist, dist2, index, device=dev)
    return dist2, index


def nearest(query, target, max_dist=None):
    """-> (dist2 [Nq] float32, index [Nq] int32) on the device: for every query point the squared distance to its nearest
    target point, capped at max_dist^2, and that point's index (the smallest among equals; -1: none within max_dist).
    query [Nq, 3], target [Nt, 3] float32 on the GPU, Nt >= 1, finite coordinates.  Nq = 0 gives empty tensors."""
    fn = "nearest"
    max_dist = _max_dist(fn, max_dist)
    query, target = _check_pair(fn, "query", query, "target", target)
    _finite(fn, "query", query)
    _finite(fn, "target", target)
    return _nearest(query, target, max_dist)


def _reduce(dist2, thresholds):
    """dist2: checked [n] float32, n >= 1.  -> the device record [10] float64: sum, max, eight counts.  No host read."""
    n, dev = dist2.shape[0], dist2.device
    out = torch.empty(2 + MAX_THRESHOLDS, dtype=torch.float64, device=dev)
    scratch = _C.scratch(_C.lib.scr_surfeval_score_scratch_bytes(n), dev)
    _C.family_call("scr_surfeval_score", n, dist2, len(thresholds), _C.host_array(thresholds, _C.f32) if thresholds else None,
                   scratch, out, device=dev)
    return out


def _check_dist2(fn, name, t):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{fn}: {name} is not a tensor")
    if t.dim() != 1 or t.dtype != torch.float32:
        raise ValueError(f"{fn}: {name} {tuple(t.shape)} {t.dtype} is not a float32 [N] tensor")
    if not 1 <= t.shape[0] < 2 ** 31:
        raise ValueError(f"{fn}: {name} has {t.shape[0]} entries: an empty side cannot be scored" if t.shape[0] == 0 else
                         f"{fn}: {name} has {t.shape[0]} entries, not below 2^31")


def score(dist2_pred_to_gt, dist2_gt_to_pred, thresholds=()):
    """The scores of two lists of squared nearest distances (see the module's definition) -> dict: accuracy, completeness,
    chamfer, max_pred_to_gt, max_gt_to_pred, num_pred, num_gt, thresholds, and per threshold precision, recall, fscore,
    count_pred_to_gt, count_gt_to_pred (lists).  Everything is reduced on the device; one host read."""
    fn = "score"
    thresholds = _thresholds(fn, thresholds)
    _check_dist2(fn, "dist2_pred_to_gt", dist2_pred_to_gt)
    _check_dist2(fn, "dist2_gt_to_pred", dist2_gt_to_pred)
    _device_only(fn, "dist2_pred_to_gt", dist2_pred_to_gt)
    _device_only(fn, "dist2_gt_to_pred", dist2_gt_to_pred)
    if dist2_pred_to_gt.device != dist2_gt_to_pred.device:
        raise ValueError(f"{fn}: dist2_pred_to_gt is on {dist2_pred_to_gt.device}, dist2_gt_to_pred on {dist2_gt_to_pred.device}")
    a, b = dist2_pred_to_gt.detach().contiguous(), dist2_gt_to_pred.detach().contiguous()
    rec = torch.stack((_reduce(a, thresholds), _reduce(b, thresholds))).tolist()
    return _result(rec[0], rec[1], a.shape[0], b.shape[0], thresholds)


def _result(p2g, g2p, n_pred, n_gt, thresholds):
    k = len(thresholds)
    accuracy, completeness = p2g[0] / n_pred, g2p[0] / n_gt
    cp, cg = [int(c) for c in p2g[2:2 + k]], [int(c) for c in g2p[2:2 + k]]
    precision, recall = [c / n_pred for c in cp], [c / n_gt for c in cg]
    fscore = [2.0 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(precision, recall)]
    return {"accuracy": accuracy, "completeness": completeness, "chamfer": (accuracy + completeness) / 2.0,
            "max_pred_to_gt": p2g[1], "max_gt_to_pred": g2p[1], "num_pred": n_pred, "num_gt": n_gt,
            "thresholds": [float(np.float32(t)) for t in thresholds], "precision": precision, "recall": recall, "fscore": fscore,
            "count_pred_to_gt": cp, "count_gt_to_pred": cg}


def _evaluate(pred, gt, thresholds, max_dist):
    """pred, gt: checked and finite, both non-empty."""
    a, _ = _nearest(pred, gt, max_dist)
    b, _ = _nearest(gt, pred, max_dist)
    rec = torch.stack((_reduce(a, thresholds), _reduce(b, thresholds))).tolist()
    return _result(rec[0], rec[1], pred.shape[0], gt.shape[0], thresholds)


def evaluate_points(pred_points, gt_points, thresholds=(), max_dist=None):
    """score() of the nearest distances between two clouds, both ways.  max_dist caps every distance (DTU caps at 20 mm)."""
    fn = "evaluate_points"
    thresholds, max_dist = _thresholds(fn, thresholds), _max_dist(fn, max_dist)
    pred, gt = _check_pair(fn, "pred_points", pred_points, "gt_points", gt_points, a_least=1)
    _finite(fn, "pred_points", pred)
    _finite(fn, "gt_points", gt)
    return _evaluate(pred, gt, thresholds, max_dist)


def evaluate_mesh(vertices, faces, gt_points, spacing, thresholds=(), max_dist=None, seed=0):
    """Sample the mesh at `spacing` (sample_surface) and score the samples against the ground-truth cloud.  The result also
    carries spacing and seed.  A mesh that yields no sample is a ValueError."""
    fn = "evaluate_mesh"
    thresholds, max_dist = _thresholds(fn, thresholds), _max_dist(fn, max_dist)
    _points_shape(fn, "gt_points", gt_points)
    if gt_points.shape[0] == 0:
        raise ValueError(f"{fn}: gt_points is empty")
    _real(fn, "spacing", spacing, 0)
    _vertices_shape(fn, vertices, None)
    _faces_shape(fn, faces, vertices.shape[0])
    _device_only(fn, "vertices", vertices)
    _device_only(fn, "gt_points", gt_points)
    if gt_points.device != vertices.device:
        raise ValueError(f"{fn}: gt_points is on {gt_points.device}, vertices on {vertices.device}")
    gt = gt_points.detach().contiguous()
    _finite(fn, "gt_points", gt)
    pred, _ = sample_surface(vertices, faces, spacing=spacing, seed=seed)
    if pred.shape[0] == 0:
        raise ValueError(f"{fn}: the mesh yields no sample at spacing {spacing!r}: an empty side cannot be scored")
    res = _evaluate(pred, gt, thresholds, max_dist)
    res.update(spacing=float(spacing), seed=seed)
    return res


def write_mesh_results(model_dir, res, method="ours"):
    """mesh_results.json in model_dir: {method: res}, beside evaluate.write_results' results.json, which is left alone.
    Returns the path."""
    path = os.path.join(model_dir, "mesh_results.json")
    os.makedirs(model_dir, exist_ok=True)
    with open(path, "w") as fp:
        json.dump({method: res}, fp, indent=True)
    return path
