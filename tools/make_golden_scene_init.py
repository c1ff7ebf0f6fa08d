#!/usr/bin/env python3
"""Generate tests/golden/scene_init.npz by IMPORTING the reference's own Python (GaussianModel.voxelize_sample and
create_from_pcd, scene/gaussian_model.py:447-451,472-508; build container only) on a seeded cloud.  Only arrays are
written.  `simple_knn._C.distCUDA2` has no source in the reference tree: tools/make_golden.py stubs it with None, and
this tool replaces that stub, before the reference module is imported, by a float64 brute force of the same quantity
(mean squared distance to the 3 nearest other points) written below.

  points        [N,3] float32, N ~ 3.9 k: Gaussian clusters + a uniform background in [-2, 2]^3 (negative coordinates),
                10 % exact duplicate rows, and rows with a coordinate exactly on a half-way case x / v = k + 0.5 in
                float32 (even and odd k, both signs) for each voxel size
  voxel_sizes   [2] float64: 0.05, 0.01;  vox0 / vox1: the reference's voxelize_sample(points, v) for each
  _anchor, _scaling, _rotation, _opacity      what create_from_pcd(voxel_size = voxel_sizes[0]) leaves on the model
  dist2_f64     [M] float64: the brute force on those anchors (what `_scaling` was made from, before .float())
  auto_voxel_size   the voxel size create_from_pcd picks for voxel_size <= 0 (kthvalue of the raw cloud's distCUDA2)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

VOXEL_SIZES = (0.05, 0.01)


def dist2_f64(points):
    """float64 brute force: mean of the 3 smallest squared distances to OTHER points (by index: duplicates count)."""
    p = torch.as_tensor(np.asarray(points.detach().cpu() if torch.is_tensor(points) else points)).double()
    N = p.shape[0]
    out = torch.empty(N, dtype=torch.float64)
    step = max(1, (1 << 22) // N)
    for s in range(0, N, step):
        e = min(s + step, N)
        d = ((p[None, :, :] - p[s:e, None, :]) ** 2).sum(-1)
        d[torch.arange(e - s), torch.arange(s, e)] = float("inf")
        out[s:e] = d.topk(3, dim=1, largest=False).values.sum(1) / 3.0
    return out


def halfway_rows(rng, v, n):
    """Rows whose first coordinate satisfies float32(x) / float32(v) == k + 0.5 exactly (kept only when it does)."""
    v32 = np.float32(v)
    k = rng.integers(-int(1.9 / v), int(1.9 / v), size=4 * n)
    x = ((k.astype(np.float64) + 0.5) * float(v32)).astype(np.float32)
    ok = (x / v32) == (k + 0.5).astype(np.float32)
    x, k = x[ok], k[ok]
    even, odd = x[k % 2 == 0][: n // 2], x[k % 2 != 0][: n // 2]
    x = np.concatenate([even, odd])
    assert len(even) and len(odd) and (x < 0).any() and (x > 0).any()
    rows = rng.uniform(-1.9, 1.9, size=(len(x), 3)).astype(np.float32)
    rows[:, 0] = x
    rows[::3, 1] = rows[::3, 0]            # some rows half-way in two coordinates
    return rows


def make_cloud():
    rng = np.random.default_rng(20240607)
    centres = rng.uniform(-1.5, 1.5, size=(6, 3))
    parts = [(c + rng.standard_normal((450, 3)) * s).astype(np.float32) for c, s in zip(centres, (0.02, 0.05, 0.1, 0.2, 0.03, 0.3))]
    parts.append(rng.uniform(-2, 2, size=(500, 3)).astype(np.float32))
    parts += [halfway_rows(rng, v, 60) for v in VOXEL_SIZES]
    pts = np.concatenate(parts)
    dup = pts[rng.integers(0, len(pts), size=len(pts) // 10)]
    pts = np.concatenate([pts, dup]).astype(np.float32)
    return pts[rng.permutation(len(pts))]


def make_scene_init():
    sys.modules["simple_knn._C"].distCUDA2 = dist2_f64          # before scene.gaussian_model binds the name
    zeros, ones = torch.zeros, torch.ones

    def drop_cuda(fn):
        def wrapped(*a, **k):
            if str(k.get("device", "")).startswith("cuda"):
                k.pop("device")
            return fn(*a, **k)
        return wrapped

    torch.zeros, torch.ones = drop_cuda(zeros), drop_cuda(ones)
    try:
        pc, _, _ = mg._ref_model([], 8, 0)
        pts = make_cloud()
        out = {"points": pts, "voxel_sizes": np.asarray(VOXEL_SIZES, dtype=np.float64)}
        for i, v in enumerate(VOXEL_SIZES):
            out[f"vox{i}"] = pc.voxelize_sample(pts.copy(), voxel_size=v)      # (it shuffles its argument in place)
            assert out[f"vox{i}"].dtype == np.float32

        class Pcd:
            points = None

        pcd = Pcd()
        pcd.points = pts.copy()
        pc.voxel_size, pc.ratio = VOXEL_SIZES[0], 1
        pc.create_from_pcd(pcd, 1.0)
        for name in ("_anchor", "_scaling", "_rotation", "_opacity"):
            out[name] = mg.f32(getattr(pc, name))
        assert np.array_equal(out["_anchor"], out["vox0"])
        out["dist2_f64"] = dist2_f64(out["_anchor"]).numpy()
        pcd.points = pts.copy()
        pc.voxel_size = 0
        pc.create_from_pcd(pcd, 1.0)
        out["auto_voxel_size"] = np.float64(pc.voxel_size)
    finally:
        torch.zeros, torch.ones = zeros, ones
    np.savez_compressed(os.path.join(mg.OUT, "scene_init.npz"), **out)
    return out


if __name__ == "__main__":
    mg.install_stubs()
    o = make_scene_init()
    print("scene_init.npz", os.path.getsize(os.path.join(mg.OUT, "scene_init.npz")),
          {k: getattr(v, "shape", v) for k, v in o.items()})
