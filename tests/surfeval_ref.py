"""The definitions of splatco_amd.surface_eval (include/splatco_surfeval.h) restated in plain numpy and Python: what the kernels
are tested against, bit for bit where the definition fixes the bits (the samples, the nearest distances and indices, the
counts) and against math.fsum where it fixes an order of summation only (the means).  numpy rounds every float32 and float64
operation on its own and fuses nothing, which is the library's -ffp-contract=off."""
import math

import numpy as np

THREADS = 256                       # the kernels' workgroup size


# ------------------------------------------------------------------ random numbers
def mix(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x21f0aaad)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x735a2d97)
    x ^= x >> np.uint32(15)
    return x


def u32(seed, f, c):
    with np.errstate(over="ignore"):
        return mix(mix(mix(np.uint32(seed)) ^ np.asarray(f).astype(np.uint32)) ^ np.asarray(c).astype(np.uint32))


def uniform(seed, f, c):
    return u32(seed, f, c).astype(np.float64) * 2.0 ** -32


# ------------------------------------------------------------------ sampling
def _corners(vertices, faces):
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    p0 = v[f[:, 0]]
    return p0, v[f[:, 1]] - p0, v[f[:, 2]] - p0


def areas_ref(vertices, faces):
    _, e1, e2 = _corners(vertices, faces)
    with np.errstate(all="ignore"):
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def face_counts_ref(vertices, faces, density, seed=0):
    a = areas_ref(vertices, faces)
    with np.errstate(all="ignore"):
        want = a * np.float64(density) + uniform(seed, np.arange(len(a)), 0)
        n = np.where(want >= 2.0 ** 31, 2.0 ** 31, np.floor(want))
    return np.where(np.isfinite(a), n, 0.0).astype(np.int64)


def sample_ref(vertices, faces, density, seed=0):
    """-> (points float32 [Ns, 3], face_index int32 [Ns])"""
    counts = face_counts_ref(vertices, faces, density, seed)
    ns = int(counts.sum())
    assert ns < 2 ** 31
    p0, e1, e2 = _corners(vertices, faces)
    f = np.repeat(np.arange(len(counts)), counts)
    j = np.arange(ns) - np.repeat(np.cumsum(counts) - counts, counts)
    r1, r2 = uniform(seed, f, 1 + 2 * j), uniform(seed, f, 2 + 2 * j)
    flip = r1 + r2 > 1.0
    r1, r2 = np.where(flip, 1.0 - r1, r1), np.where(flip, 1.0 - r2, r2)
    pts = (p0[f] + r1[:, None] * e1[f]) + r2[:, None] * e2[f]
    return pts.astype(np.float32).reshape(-1, 3), f.astype(np.int32)


def barycentrics(points, vertices, faces, face_index):
    """(w0, w1, w2) of every point in its face, binary64, least squares in the face's plane."""
    p0, e1, e2 = (x[face_index] for x in _corners(vertices, faces))
    d = np.asarray(points, np.float64) - p0
    a, b, c = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    u, v = (d * e1).sum(1), (d * e2).sum(1)
    det = a * c - b * b
    w1, w2 = (c * u - b * v) / det, (a * v - b * u) / det
    return np.stack((1.0 - w1 - w2, w1, w2), axis=1)


# ------------------------------------------------------------------ nearest neighbour
def cap2_ref(max_dist):
    if max_dist is None:
        return np.float32(np.inf)
    m = np.float32(max_dist)
    return np.float32(m * m)


def nearest_ref(query, target, max_dist=None, chunk=128):
    """Brute force in float32, the definition's order.  -> (dist2 float32 [Nq], index int32 [Nq])"""
    q, t = np.asarray(query, np.float32).reshape(-1, 3), np.asarray(target, np.float32).reshape(-1, 3)
    assert len(t) >= 1
    cap2 = cap2_ref(max_dist)
    dist2, index = np.empty(len(q), np.float32), np.empty(len(q), np.int32)
    with np.errstate(over="ignore"):
        for s in range(0, len(q), chunk):
            e = t[None, :, :] - q[s:s + chunk, None, :]
            d = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            assert d.dtype == np.float32
            j = d.argmin(1)                                  # the first of equals: the smallest j
            dm = d[np.arange(len(j)), j]
            dist2[s:s + chunk] = np.minimum(cap2, dm)
            index[s:s + chunk] = np.where(dm <= cap2, j, -1)
    return dist2, index


# ------------------------------------------------------------------ score
def reduce_ref(dist2, thresholds=()):
    """-> (math.fsum of d, max d, [count of d <= (double)(float)t])"""
    d = np.sqrt(np.asarray(dist2, np.float32).astype(np.float64))
    return math.fsum(d.tolist()), float(d.max()), [int((d <= np.float64(np.float32(t))).sum()) for t in thresholds]


def score_ref(dist2_pred_to_gt, dist2_gt_to_pred, thresholds=()):
    (sp, mp, cp), (sg, mg, cg) = reduce_ref(dist2_pred_to_gt, thresholds), reduce_ref(dist2_gt_to_pred, thresholds)
    n_pred, n_gt = len(dist2_pred_to_gt), len(dist2_gt_to_pred)
    accuracy, completeness = sp / n_pred, sg / n_gt
    precision, recall = [c / n_pred for c in cp], [c / n_gt for c in cg]
    return {"accuracy": accuracy, "completeness": completeness, "chamfer": (accuracy + completeness) / 2.0,
            "max_pred_to_gt": mp, "max_gt_to_pred": mg, "num_pred": n_pred, "num_gt": n_gt,
            "thresholds": [float(np.float32(t)) for t in thresholds], "precision": precision, "recall": recall,
            "fscore": [2.0 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(precision, recall)],
            "count_pred_to_gt": cp, "count_gt_to_pred": cg}


# ------------------------------------------------------------------ recipes
def unit_square():
    v = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], np.float32)
    return v, np.array([(0, 1, 2), (0, 2, 3)], np.int32)


def small_faces(nf, seed, size=0.05):
    """nf separate small triangles of unit-scale position: -> (vertices [3 nf, 3], faces)"""
    gen = np.random.default_rng(seed)
    base = gen.uniform(-1, 1, size=(nf, 1, 3))
    v = (base + size * gen.uniform(-1, 1, size=(nf, 3, 3))).astype(np.float32).reshape(-1, 3)
    return v, np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)


def unit_triangles(nf, seed):
    """nf separate equilateral triangles of side 1 in random poses, every coordinate inside (-1, 1): altitude 0.866, so a point
    moved by float32 rounding (at most 2^-25 per coordinate) moves its barycentrics by about 2^-24."""
    gen = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(3) / 3
    tri = np.stack((np.cos(ang), np.sin(ang), np.zeros(3)), axis=1) / math.sqrt(3.0)           # circumradius 0.577
    out = []
    for _ in range(nf):
        rot, _ = np.linalg.qr(gen.standard_normal((3, 3)))
        out.append(tri @ rot.T + gen.uniform(-0.4, 0.4, size=3))
    return np.array(out).astype(np.float32).reshape(-1, 3), np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)


def targets(shape, n, seed):
    """The target clouds of the nearest-neighbour tests, float32 [n, 3]."""
    gen = np.random.default_rng(seed)
    p = gen.uniform(-1, 1, size=(n, 3))
    if shape == "cube":
        pass
    elif shape == "sheet":
        p[:, 2] = 0.37
    elif shape == "line":
        p[:, 1], p[:, 2] = -0.21, 0.37
    elif shape == "point":
        p[:] = (0.3, -0.7, 0.11)
    elif shape == "clusters":                               # two clusters 100 extents apart, nothing between them
        p *= 0.5
        p[n // 2:, 0] += 100.0
    else:
        raise ValueError(shape)
    return p.astype(np.float32)


def queries(target, n, seed):
    """n queries of every kind in one array, in shuffled order: copies of targets, points on the box's faces and corners,
    points 10 and 1000 extents outside along one axis and along the diagonal, points inside."""
    gen = np.random.default_rng(seed)
    t = np.asarray(target, np.float64)
    lo, hi = t.min(0), t.max(0)
    ext = max(float((hi - lo).max()), 1.0)
    mid = 0.5 * (lo + hi)
    out = []
    for i in range(n):
        kind = i % 8
        if kind == 0:
            q = t[gen.integers(len(t))]
        elif kind == 1:                                     # on a face of the box
            q = gen.uniform(lo, hi)
            a = gen.integers(3)
            q[a] = (lo, hi)[gen.integers(2)][a]
        elif kind == 2:                                     # a corner
            q = np.where(gen.integers(2, size=3) == 1, hi, lo)
        elif kind in (3, 4):                                # outside along one axis
            q = gen.uniform(lo, hi)
            q[gen.integers(3)] += (10.0, 1000.0)[kind - 3] * ext * (1 if gen.integers(2) else -1)
        elif kind in (5, 6):                                # outside along the diagonal
            q = mid + (10.0, 1000.0)[kind - 5] * ext * np.where(gen.integers(2, size=3) == 1, 1.0, -1.0)
        else:
            q = gen.uniform(lo, hi)
        out.append(q)
    out = np.array(out).reshape(-1, 3)
    return out[gen.permutation(n)].astype(np.float32)


def sphere_points(centre, radius, n, seed):
    g = np.random.default_rng(seed).standard_normal((n, 3))
    return (np.asarray(centre, np.float64) + radius * g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
