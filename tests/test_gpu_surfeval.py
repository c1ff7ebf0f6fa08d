"""Mesh evaluation on the device against tests/surfeval_ref.py: every integer and every float32 bit for bit (the samples, the
nearest distances and indices, the counts), the binary64 sums against math.fsum within n * 2^-52, and the whole evaluation on a
sphere whose scores are known."""
import functools
import json
import math

import numpy as np
import pytest
import torch

import mesh_ref
import surfeval_ref as ref
import tsdf_ref
import splatco_amd.surface_eval                # noqa: F401  (the module under test: without it nothing here can run)
from splatco_amd.surface_eval import THREADS as T, evaluate_mesh, evaluate_points, nearest, sample_surface, score, write_mesh_results

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
bits = lambda a: np.ascontiguousarray(a).view(np.int32)


def _same(got, want):
    d2, idx = (x.cpu().numpy() for x in got)
    assert d2.dtype == np.float32 and idx.dtype == np.int32 and d2.shape == want[0].shape and idx.shape == want[1].shape
    bad = np.nonzero((bits(d2) != bits(want[0])) | (idx != want[1]))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(d2)} differ, first {bad[0]}: got ({d2[bad[0]]}, {idx[bad[0]]}) want ({want[0][bad[0]]}, {want[1][bad[0]]})"


# ------------------------------------------------------------------ nearest neighbour
def test_the_workgroup_size_is_the_reference_s():
    assert T == ref.THREADS == 256


@pytest.mark.parametrize("shape", ("cube", "sheet", "line", "point", "clusters"))
def test_nearest_on_every_target_shape_and_size(shape):
    """Queries of every kind mixed in one launch: copies of targets (distance exactly 0, the smallest duplicate), points on the
    box's faces and corners, points 10 and 1000 extents outside along one axis and along the diagonal, points inside."""
    for nt in (1, 2, 63, 64, 65, 1000, 5000):
        t = ref.targets(shape, nt, 10 + nt)
        if nt >= 63:
            t[nt // 2:nt // 2 + 20] = t[:20]                                      # duplicates: ties at distance 0
        q_all = ref.queries(t, 4 * T + 1, nt)
        want_all = ref.nearest_ref(q_all, t)
        td = dev(t)
        for nq in (1, T - 1, T, T + 1, 4 * T + 1):
            _same(nearest(dev(q_all[:nq]), td), (want_all[0][:nq], want_all[1][:nq]))
        copies = np.nonzero((want_all[0] == 0))[0]
        assert len(copies) >= (4 * T + 1) // 8


def test_nearest_settles_ties_by_the_smallest_index():
    """An integer lattice with every point stored twice in shuffled order; the queries are the centres of its cells: all
    arithmetic is exact in float32, eight targets and their duplicates tie at 0.75."""
    g = np.arange(5, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    t = np.concatenate((lattice, lattice))[np.random.default_rng(0).permutation(2 * len(lattice))]
    c = np.arange(4, dtype=np.float32) + 0.5
    q = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
    want = ref.nearest_ref(q, t)
    assert (want[0] == 0.75).all()
    ties = ((t[None] - q[:, None]) ** 2).sum(-1) == 0.75
    assert (ties.sum(1) == 16).all() and np.array_equal(want[1], ties.argmax(1))
    _same(nearest(dev(q), dev(t)), want)
    _same(nearest(dev(q), dev(t), max_dist=math.sqrt(0.75)), ref.nearest_ref(q, t, math.sqrt(0.75)))


@pytest.mark.parametrize("shape", ("cube", "clusters"))
def test_nearest_under_a_cap(shape):
    t = ref.targets(shape, 1000, 3)
    q = ref.queries(t, 4 * T + 1, 4)
    td, qd = dev(t), dev(q)
    free = ref.nearest_ref(q, t)
    # 0: only coincident points match, the rest get cap2 = 0 and no index
    want = ref.nearest_ref(q, t, 0.0)
    assert (want[0] == 0).all() and 0 < (want[1] >= 0).sum() < len(q)
    _same(nearest(qd, td, max_dist=0.0), want)
    # a cap that some queries meet and some do not: the median distance of those that are not copies
    m = float(np.sqrt(np.median(free[0][free[0] > 0])))
    want = ref.nearest_ref(q, t, m)
    assert 0.3 * len(q) < (want[1] < 0).sum() < 0.6 * len(q)
    _same(nearest(qd, td, max_dist=m), want)
    _same(nearest(qd, td, max_dist=None), free)
    # far queries only, all beyond the cap: nothing is searched, nothing matches
    far = q[free[0] > 25.0]
    assert len(far) > T
    got = nearest(dev(far), td, max_dist=1.0)
    assert (got[0] == 1.0).all() and (got[1] == -1).all()


def test_a_distance_exactly_at_the_cap_is_a_match():
    g = np.arange(4, dtype=np.float32)
    t = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    q = t[t[:, 0] == 0] + np.array([-3.0, 4.0, 0.0], np.float32)                   # (-3, y + 4, z): 5 from (0, y, z) where y + 4 > 3
    q = np.concatenate((q, t[t[:, 0] == 0] + np.array([-1.0, 0.0, 0.0], np.float32)))
    for m in (1.0, 5.0, 0.999, 4.999):
        want = ref.nearest_ref(q, t, m)
        _same(nearest(dev(q), dev(t), max_dist=m), want)
    want = ref.nearest_ref(q, t, 1.0)
    assert (want[0][16:] == 1.0).all() and (want[1][16:] >= 0).all() and (want[1][:16] == -1).all()
    assert (ref.nearest_ref(q, t, 0.999)[1] == -1).all()


def test_nearest_of_nothing_and_its_rejections():
    t = dev(ref.targets("cube", 10, 0))
    d2, idx = nearest(t[:0], t)
    assert d2.shape == (0,) and d2.dtype == torch.float32 and idx.shape == (0,) and idx.dtype == torch.int32
    bad = t.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError, match="target has non-finite"):
        nearest(t, bad)
    bad[3, 1] = float("inf")
    with pytest.raises(ValueError, match="query has non-finite"):
        nearest(bad, t)
    with pytest.raises(ValueError, match="target is empty"):
        nearest(t, t[:0])
    with pytest.raises(ValueError, match="cpu"):
        nearest(t.cpu(), t)


# ------------------------------------------------------------------ sampling
def _sample_same(v, f, density, seed=0):
    pts, fi = (x.cpu().numpy() for x in sample_surface(dev(v), dev(f), density=density, seed=seed))
    want = ref.sample_ref(v, f, density, seed)
    assert pts.dtype == np.float32 and fi.dtype == np.int32 and pts.shape == want[0].shape and fi.shape == want[1].shape
    assert np.array_equal(fi, want[1]) and np.array_equal(bits(pts), bits(want[0]))
    return pts, fi


@pytest.mark.parametrize("nf", (1, 2, T - 1, T, T + 1, 5000))
def test_samples_of_small_faces(nf):
    v, f = ref.small_faces(nf, nf)
    area = ref.areas_ref(v, f)
    mean = 1.0 / float(area.mean())
    for density in (3.0 * mean, 0.1 * mean):                  # a few per face; most faces get none
        pts, fi = _sample_same(v, f, density, seed=nf)
        assert abs(len(pts) - density * area.sum()) < nf
    assert sample_surface(dev(v), dev(f), density=1e-9)[0].shape == (0, 3)            # nothing at all: empty outputs
    assert sample_surface(dev(v), dev(f), density=1e-9)[1].dtype == torch.int32


def test_samples_of_the_unit_square_and_the_template_meshes():
    v, f = ref.unit_square()
    pts, fi = _sample_same(v, f, 20000.0)
    assert np.bincount(fi).tolist() == [10000, 10000]
    a = sample_surface(dev(v), dev(f), spacing=0.01, seed=1)
    b = sample_surface(dev(v), dev(f), density=10000.0, seed=1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].shape[0] == 10000
    assert not torch.equal(a[0], sample_surface(dev(v), dev(f), spacing=0.01, seed=2)[0])          # another seed, other points
    c = sample_surface(dev(v), dev(f), spacing=0.01, seed=1)
    assert torch.equal(a[0].view(torch.int32), c[0].view(torch.int32))                              # the same seed, the same bits
    for v, f in (mesh_ref.mixed_mesh(40, 5, 3)[:2], mesh_ref.fan(70), mesh_ref.deep_strip(300), mesh_ref.octahedron()):
        _sample_same(v, f, 25.0, seed=7)
        _sample_same(v, f.astype(np.int64), 25.0, seed=7)


def test_degenerate_faces_get_no_samples_and_one_face_takes_a_long_run():
    v = np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (0.5, 0.25, 3.0)], np.float32)
    f = np.array([(0, 0, 1), (1, 1, 1), (0, 1, 2), (0, 1, 3), (2, 0, 1), (3, 1, 4)], np.int32)
    pts, fi = _sample_same(v, f, 1000.0, seed=5)
    assert set(fi.tolist()) == {3, 5} and (fi == 3).sum() == 500
    # 100 000 samples on one face, between two faces that get a few: the binary search over a single long run
    v = np.array([(0, 0, 0), (0.01, 0, 0), (0, 0.01, 0), (10, 0, 0), (0, 10, 0), (5, 5, 1)], np.float32)
    f = np.array([(0, 1, 2), (0, 3, 4), (1, 2, 5)], np.int32)
    pts, fi = _sample_same(v, f, 2000.0, seed=1)
    assert (fi == 1).sum() == 100000 and len(pts) > 100000
    w = ref.barycentrics(pts[fi == 1], v, f, np.ones(100000, np.int64))
    assert w.min() >= -2.0 ** -20


def test_sampling_refuses_bad_values():
    v, f = ref.unit_square()
    bad = v.copy()
    bad[1, 0] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        sample_surface(dev(bad), dev(f), density=10.0)
    with pytest.raises(ValueError, match="face indices"):
        sample_surface(dev(v), dev(f + 2), density=10.0)
    with pytest.raises(ValueError, match="2\\^31"):
        sample_surface(dev(v), dev(f), density=3e9)
    assert sample_surface(dev(v), dev(f[:0]), density=10.0)[0].shape == (0, 3)


# ------------------------------------------------------------------ score
@pytest.mark.parametrize("n", (1, T, T + 1, 100003))
def test_score_counts_are_exact_and_sums_within_the_bound(n):
    gen = np.random.default_rng(n)
    a = (gen.uniform(0, 2, size=n) ** 2).astype(np.float32)
    b = (gen.uniform(0, 1, size=max(n // 3, 1)) ** 2).astype(np.float32)
    # thresholds that equal some distances exactly: float32 values whose squares are float32 too
    exact = np.float32([0.5, 1.25, 0.0])
    a[:3], b[:1] = (exact * exact)[:min(n, 3)], exact[:1] * exact[:1]
    thresholds = (0.5, 1.25, 0.0, 0.1, 3.0)
    res = score(dev(a), dev(b), thresholds)
    want = ref.score_ref(a, b, thresholds)
    for key in ("count_pred_to_gt", "count_gt_to_pred", "num_pred", "num_gt", "max_pred_to_gt", "max_gt_to_pred", "thresholds",
                "precision", "recall", "fscore"):
        assert res[key] == want[key], key
    assert res["count_pred_to_gt"][0] >= 1 and res["count_pred_to_gt"][4] == n
    for key, m in (("accuracy", n), ("completeness", len(b))):
        rel = abs(res[key] - want[key]) / want[key]
        print(f"{key}: n = {m}, relative difference {rel:.3e}, bound {m * 2.0 ** -52:.3e}")
        assert rel <= m * 2.0 ** -52, key
    assert res["chamfer"] == (res["accuracy"] + res["completeness"]) / 2
    assert set(res) == set(want)
    again = score(dev(a), dev(b), thresholds)
    assert again == res                                                           # the same bits run after run
    assert score(dev(a), dev(b)) == {**res, **{k: [] for k in ("thresholds", "precision", "recall", "fscore", "count_pred_to_gt",
                                                                 "count_gt_to_pred")}}


# ------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _sphere():
    """The unit sphere on a grid of h = 1 / 3.5 (numpy extraction), and points on the analytic sphere."""
    vol, lo, h, centre, r = tsdf_ref.sphere_volume(dims=(16, 16, 16), h=1.0 / 3.5, radius_cells=3.5)
    m = tsdf_ref.extract_ref(vol, lo, h)
    assert abs(r - 1.0) < 1e-6
    return m["vertices"], m["faces"], float(h), ref.sphere_points(centre, r, 20000, 1)


def test_evaluate_mesh_of_a_sphere(tmp_path):
    v, f, h, gt = _sphere()
    vd, fd, gd = dev(v), dev(f), dev(gt)
    res = evaluate_mesh(vd, fd, gd, spacing=0.04, thresholds=(2 * h, 0.0))
    assert res["num_gt"] == len(gt) and abs(res["num_pred"] - 4 * math.pi / 0.04 ** 2) < 0.1 * res["num_pred"]
    assert 0 < res["accuracy"] < h and 0 < res["completeness"] < h and res["chamfer"] == (res["accuracy"] + res["completeness"]) / 2
    assert res["fscore"] == [1.0, 0.0] and res["precision"] == [1.0, 0.0] and res["recall"] == [1.0, 0.0]
    assert res["spacing"] == 0.04 and res["seed"] == 0
    # twice: the same bits; another seed: other samples, nearly the same scores
    assert evaluate_mesh(vd, fd, gd, spacing=0.04, thresholds=(2 * h, 0.0)) == res
    other = evaluate_mesh(vd, fd, gd, spacing=0.04, thresholds=(2 * h, 0.0), seed=3)
    assert other["accuracy"] != res["accuracy"] and abs(other["accuracy"] - res["accuracy"]) < 0.05 * res["accuracy"]
    # the same mesh shifted by 10 h along a diagonal: no sample within 2 h of the sphere
    shift = np.float32(10 * h / math.sqrt(3.0))
    far = evaluate_mesh(dev(v + shift), fd, gd, spacing=0.04, thresholds=(2 * h,))
    assert far["precision"] == [0.0] and far["recall"] == [0.0] and far["fscore"] == [0.0] and far["accuracy"] > 2 * h
    capped = evaluate_mesh(dev(v + shift), fd, gd, spacing=0.04, thresholds=(2 * h,), max_dist=2 * h)
    cap = math.sqrt(float(ref.cap2_ref(2 * h)))                                   # every distance is the cap
    assert capped["max_pred_to_gt"] == cap == capped["max_gt_to_pred"] and abs(capped["chamfer"] - cap) <= len(gt) * 2.0 ** -52 * cap
    # the pieces give what the whole gives
    pts, _ = sample_surface(vd, fd, spacing=0.04)
    a, ia = nearest(pts, gd)
    b, ib = nearest(gd, pts)
    keys = [k for k in res if k not in ("spacing", "seed")]
    pieces = score(a, b, (2 * h, 0.0))
    assert {k: res[k] for k in keys} == pieces == evaluate_points(pts, gd, (2 * h, 0.0))
    want = ref.score_ref(a.cpu().numpy(), b.cpu().numpy(), (2 * h, 0.0))
    assert all(pieces[k] == want[k] for k in keys if k not in ("accuracy", "completeness", "chamfer"))
    assert abs(pieces["chamfer"] - want["chamfer"]) <= len(gt) * 2.0 ** -52 * want["chamfer"]
    # a sample of the indices against brute force
    sub = np.random.default_rng(0).choice(len(gt), 300, replace=False)
    w = ref.nearest_ref(gt[sub], pts.cpu().numpy())
    assert np.array_equal(bits(b.cpu().numpy()[sub]), bits(w[0])) and np.array_equal(ib.cpu().numpy()[sub], w[1])
    path = write_mesh_results(str(tmp_path), res)
    assert json.load(open(path)) == {"ours": res}
