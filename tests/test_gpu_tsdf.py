"""TSDF fusion and mesh extraction on the device against the numpy float64 restatement (tests/tsdf_ref.py).

Both sides perform the same correctly rounded binary64 operations in the same order, so identical bits are expected and one
float32 ulp is the most a differing last operation can cost; the count of non-identical values is printed.  Nodes whose
verdicts hang on the last bit of the reference's own u, v, sdf or zc (tsdf_ref.fragile_nodes) are left out, and must be at
most 1 % of the nodes.  The reference of each volume is computed once and shared."""
import functools
import math
import types

import numpy as np
import pytest
import torch

import tsdf_ref as ref
import splatco_amd.tsdf                       # noqa: F401  (the module under test: without it nothing here can run)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MASK_DTYPES = {"f32": torch.float32, "u8": torch.uint8, "bool": torch.bool}


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)            # a copy: the shared references are read-only


def _upload(views):
    """(depths, alphas, cams, images, masks) on the device."""
    return ([_dev(v["depth"]) for v in views], [_dev(v["alpha"]) for v in views], [(v["intr"], torch.from_numpy(v["w2c"])) for v in views],
            [_dev(v["image"]) for v in views], [_dev(v["mask"]) for v in views])


def _host(vol):
    return dict(tsdf=vol.tsdf.cpu().numpy(), weight=vol.weight.cpu().numpy(), color=None if vol.color is None else vol.color.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _parity_reference(dims, shift):
    lo, h = ref.volume_geometry(dims)
    views = ref.parity_views(dims, corner_shift=shift)
    vol, fragile = ref.integrate_views_ref(ref.fresh(dims), lo, h, views, 4.0 * float(h))
    for a in (vol["tsdf"], vol["weight"], vol["color"], fragile):
        a.setflags(write=False)
    return lo, h, views, vol, fragile


def _volume(dims, lo, h, **kw):
    from splatco_amd.tsdf import TSDFVolume
    return TSDFVolume(lo, float(h), dims, device=DEV, **kw)


# ------------------------------------------------------------------ integration
@pytest.mark.parametrize("dims,shift", [((20, 13, 9), 0.6), ((2, 5, 7), 0.6), ((64, 4, 3), 0.4)])
def test_integration_matches_the_float64_restatement(dims, shift):
    """20 x 13 x 9: 2340 nodes in three workgroups, 16-byte accesses; 2 x 5 x 7: nx = 2, two rows in every run of 4 nodes, 70
    nodes (not a multiple of 4: guarded dword accesses and a partial last run); 64 x 4 x 3: rows of 16 whole runs.  Three views
    each, in one pass: float32, uint8 and bool masks; holes of every kind."""
    lo, h, views, want, fragile = _parity_reference(dims, shift)
    vol = _volume(dims, lo, h)
    assert float(vol.tsdf.min()) == 1.0 and not vol.weight.any() and not vol.color.any() and vol.trunc == 4.0 * float(h)
    D, A, cams, images, masks = _upload(views)
    assert [m.dtype for m in masks] == [torch.float32, torch.uint8, torch.bool]
    vol.integrate_views(D, A, cams, images, masks, batch=3)
    got = _host(vol)
    keep = ~fragile
    assert fragile.sum() <= 0.01 * fragile.size
    assert np.array_equal(got["weight"][keep], want["weight"][keep])
    worst = {}
    for name in ("tsdf", "color"):
        k = keep if name == "tsdf" else np.broadcast_to(keep, got[name].shape)
        d = ref.ulp_distance(got[name], want[name])[k]
        worst[name] = (int(d.max()), int((d != 0).sum()), int(k.sum()))
    print(f"tsdf integration {dims}: non-identical tsdf {worst['tsdf'][1]} of {worst['tsdf'][2]} (max {worst['tsdf'][0]} ulp), "
          f"colour {worst['color'][1]} of {worst['color'][2]} (max {worst['color'][0]} ulp), left out {int(fragile.sum())}")
    assert worst["tsdf"][0] <= 1 and worst["color"][0] <= 1
    assert (got["weight"] == 2).any() and (got["weight"] == 0).any()


def test_integration_without_colour_and_through_unaligned_tensors():
    """color=False gives the tsdf and weight of the colour volume; a volume over tensors that start 4 bytes into an
    allocation (from_tensors) takes the guarded dword path and gives the same bits."""
    from splatco_amd.tsdf import TSDFVolume
    dims = (20, 13, 9)
    lo, h, views, want, fragile = _parity_reference(dims, 0.6)
    D, A, cams, images, masks = _upload(views)
    base = _volume(dims, lo, h)
    base.integrate_views(D, A, cams, images, masks)
    plain = _volume(dims, lo, h, color=False)
    assert plain.color is None
    plain.integrate_views(D, A, cams, None, masks)
    assert torch.equal(plain.tsdf, base.tsdf) and torch.equal(plain.weight, base.weight)
    n = 20 * 13 * 9
    raw = [torch.zeros(k * n + 1, device=DEV) for k in (1, 1, 3)]
    t, w, c = raw[0][1:].view(9, 13, 20), raw[1][1:].view(9, 13, 20), raw[2][1:].view(3, 9, 13, 20)
    t.fill_(1.0)
    assert t.data_ptr() % 16 == 4
    off = TSDFVolume.from_tensors(lo, float(h), t, w, c)
    off.integrate_views(D, A, cams, images, masks)
    assert torch.equal(off.tsdf, base.tsdf) and torch.equal(off.weight, base.weight) and torch.equal(off.color, base.color)
    assert float(raw[0][0]) == 0.0 and float(raw[2][0]) == 0.0
    # max_weight caps the weight and nothing else
    capped = _volume(dims, lo, h, max_weight=1.0)
    capped.integrate_views(D, A, cams, images, masks)
    assert float(capped.weight.max()) == 1.0 and torch.equal(capped.weight > 0, base.weight > 0)


def test_a_camera_object_gives_what_its_matrices_give_and_raises_near_to_its_znear():
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.normals import intrinsics
    dims = (12, 12, 12)
    lo, h = ref.volume_geometry(dims)
    mid = lo.astype(np.float64) + 0.5 * float(h) * 11
    cam = look_at_camera(eye=tuple(mid + np.array([0.2, -0.1, -0.3])), target=tuple(mid + np.array([0.0, 0.1, 0.4])), up=(0, -1, 0),
                         FoVx=math.radians(70), width=16, height=12).to(torch.device(DEV))
    cam.znear = 0.3
    w2c = cam.world_view_transform.t().double().cpu()
    view = ref.render_scene(12, 16, intrinsics(cam), w2c.numpy(), seed=3, holes=False)
    D, A, img = _dev(view["depth"]), _dev(view["alpha"]), _dev(view["image"])
    a, b, c = (_volume(dims, lo, h) for _ in range(3))
    a.integrate(D, A, cam, image=img, near=0.05)                       # raised to znear = 0.3
    b.integrate(D, A, (intrinsics(cam), w2c), image=img, near=0.3)
    c.integrate(D, A, (intrinsics(cam), w2c), image=img, near=0.05)
    assert torch.equal(a.tsdf, b.tsdf) and torch.equal(a.weight, b.weight) and torch.equal(a.color, b.color)
    assert int(c.weight.sum()) > int(a.weight.sum()) > 0
    want = ref.integrate_ref(ref.fresh(dims), lo, h, view["depth"], view["alpha"], view["intr"], view["w2c"], 4.0 * float(h),
                             image=view["image"], near=0.3)
    assert np.array_equal(_host(a)["weight"], want["weight"])


@functools.lru_cache(maxsize=None)
def _orbit():
    dims = (12, 12, 12)
    lo, h = ref.volume_geometry(dims, 0.08)
    return dims, lo, h, ref.orbit_views(19, 12, 16, dims, 0.08, holes=True)


def test_batching_gives_the_bits_of_one_view_per_call_and_of_a_second_run():
    """19 views of 16 x 12 maps into a 12^3 volume: one call at the batch limit (split 16 + 3 by the wrapper), 19 calls, an
    explicit split at the limit, batches of 5, the default (one view per pass) and the first again: the same bits in all three
    tensors."""
    dims, lo, h, views = _orbit()
    D, A, cams, images, masks = _upload(views)

    def run(how):
        vol = _volume(dims, lo, h)
        if how == "one":
            vol.integrate_views(D, A, cams, images, batch=16)
        elif how == "each":
            for i in range(19):
                vol.integrate(D[i], A[i], cams[i], image=images[i])
        elif how == "split":
            vol.integrate_views(D[:16], A[:16], cams[:16], images[:16], batch=16)
            vol.integrate_views(D[16:], A[16:], cams[16:], images[16:], batch=16)
        elif how == "default":
            vol.integrate_views(D, A, cams, images)
        else:
            vol.integrate_views(D, A, cams, images, batch=5)
        return vol

    base = run("one")
    assert int(base.weight.max()) >= 8 and bool((base.tsdf < 0).any())
    for how in ("each", "split", "five", "default", "one"):
        other = run(how)
        for name in ("tsdf", "weight", "color"):
            assert torch.equal(getattr(other, name).view(torch.int32), getattr(base, name).view(torch.int32)), (how, name)
    want, _ = ref.integrate_views_ref(ref.fresh(dims), lo, h, views, 4.0 * float(h))
    assert np.array_equal(_host(base)["weight"], want["weight"])


def test_launches_are_refused_for_maps_on_the_cpu(monkeypatch):
    from splatco_amd import _C
    dims, lo, h, views = _orbit()
    vol = _volume(dims, lo, h)
    made = []
    monkeypatch.setattr(_C, "family_call", lambda *a, **k: made.append(a[0]))
    D, A, cams, images, _ = _upload(views[:1])
    with pytest.raises(ValueError, match="cpu"):
        vol.integrate(D[0].cpu(), A[0], cams[0])
    with pytest.raises(ValueError, match="cpu"):
        vol.integrate(D[0], A[0], cams[0], image=images[0].cpu())
    with pytest.raises(ValueError, match="alpha"):
        vol.integrate(D[0], A[0][:5], cams[0])
    assert made == []


# ------------------------------------------------------------------ extraction
def _extract(vol_np, lo, h, min_weight=0.0):
    from splatco_amd.tsdf import TSDFVolume
    t, w = _dev(vol_np["tsdf"]), _dev(vol_np["weight"])
    c = _dev(vol_np.get("color"))
    return TSDFVolume.from_tensors(lo, float(h), t, w, c).extract(min_weight=min_weight)


def _compare_mesh(got, want):
    v, f, c = got
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda
    assert tuple(v.shape) == want["vertices"].shape and tuple(f.shape) == want["faces"].shape
    dv = ref.ulp_distance(v.cpu().numpy(), want["vertices"])
    assert dv.size == 0 or dv.max() <= 1
    bad = int((dv != 0).sum())
    if want["colors"] is None:
        assert c is None
    else:
        dc = ref.ulp_distance(c.cpu().numpy(), want["colors"])
        assert tuple(c.shape) == want["colors"].shape and (dc.size == 0 or dc.max() <= 1)
        bad += int((dc != 0).sum())
    assert np.array_equal(ref.canonical_faces(f.cpu().numpy()), ref.canonical_faces(want["faces"]))
    assert np.array_equal(f.cpu().numpy(), want["faces"])              # and in the definition's order: cube, q, triangle
    return bad


def test_extraction_matches_the_reference_on_the_integrated_volume():
    """The reference's integrated 20 x 13 x 9 volume (unobserved nodes, weights 0..2): 16,380 edge ids = 16 compaction
    workgroups, 21,888 triangle slots = 22."""
    dims = (20, 13, 9)
    lo, h, _, vol, _ = _parity_reference(dims, 0.6)
    want = ref.extract_ref(vol, lo, h)
    got = _extract(vol, lo, h)
    bad = _compare_mesh(got, want)
    print(f"tsdf extraction {dims}: {want['vertices'].shape[0]} vertices, {want['faces'].shape[0]} faces, non-identical values {bad}")
    again = _extract(vol, lo, h)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    # a bar on the weight removes the cubes seen once
    want1 = ref.extract_ref(vol, lo, h, min_weight=1.0)
    assert 0 < want1["faces"].shape[0] < want["faces"].shape[0]
    _compare_mesh(_extract(vol, lo, h, min_weight=1.0), want1)
    # without colour
    plain = dict(vol, color=None)
    assert _extract(plain, lo, h)[2] is None and torch.equal(_extract(plain, lo, h)[1], got[1])


@pytest.mark.parametrize("slab", (None, slice(9, 11)))
def test_extraction_of_the_analytic_sphere(slab):
    dims = (24, 24, 24)
    vol, lo, h, centre, r = ref.sphere_volume(dims, slab=slab)
    want = ref.extract_ref(vol, lo, h)
    v, f, c = _extract(vol, lo, h)
    _compare_mesh((v, f, c), want)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    if slab is None:
        rep = ref.assert_closed_manifold(v, f)
        assert rep["duplicates"] == 0 and abs(rep["volume"] / (4.0 / 3.0 * math.pi * r ** 3) - 1.0) < 0.02 and rep["volume"] > 0
        n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).astype(np.float64)
        assert (np.einsum("ij,ij->i", n, v[f].mean(1) - centre) > 0).all()
        assert ref.on_lattice_edges(v, want["edge_ids"], lo, h, dims, 1e-5) < 1e-6 * float(h)
    else:
        rep = ref.mesh_report(v, f)
        assert rep["nonmanifold"] == 0 and rep["unreferenced"] == 0 and rep["duplicates"] == 0 and len(rep["boundary"]) > 0


def test_extraction_edge_cases():
    from splatco_amd.tsdf import TSDFVolume
    lo, h = np.float32([0.1, -0.2, 0.3]), np.float32(0.25)
    # nothing inside: [0, 3] tensors
    v, f, c = _volume((5, 4, 3), lo, h).extract()
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and tuple(c.shape) == (0, 3)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda
    assert _volume((5, 4, 3), lo, h, color=False).extract()[2] is None
    # a sign change, but no observed cube: still nothing
    vol = _volume((5, 4, 3), lo, h)
    vol.tsdf[1, 1, 1] = -0.5
    assert tuple(vol.extract()[0].shape) == (0, 3)
    # one cube, one inside node, at each of its eight corners; exactly 0 is outside
    for node in range(8):
        t = np.full(8, 0.5, np.float32)
        t[node] = -0.25
        t[(node + 3) % 8] = 0.0
        one = dict(tsdf=t.reshape(2, 2, 2), weight=np.ones((2, 2, 2), np.float32), color=np.linspace(0, 1, 24, dtype=np.float32).reshape(3, 2, 2, 2))
        want = ref.extract_ref(one, lo, h)
        assert want["vertices"].shape[0] == (7 if node in (0, 7) else 4) and want["faces"].shape[0] == (6 if node in (0, 7) else 2)
        _compare_mesh(_extract(one, lo, h), want)
    # all inside: nothing either
    full = dict(tsdf=np.full((2, 2, 2), -1.0, np.float32), weight=np.ones((2, 2, 2), np.float32), color=None)
    assert tuple(_extract(full, lo, h)[1].shape) == (0, 3)
    # random signs and random holes in the weights: every case of every tetrahedron
    gen = np.random.default_rng(11)
    rnd = dict(tsdf=gen.uniform(-1, 1, (6, 7, 9)).astype(np.float32), weight=(gen.random((6, 7, 9)) > 0.1).astype(np.float32),
               color=gen.random((3, 6, 7, 9)).astype(np.float32))
    want = ref.extract_ref(rnd, lo, h)
    assert want["faces"].shape[0] > 500
    _compare_mesh(_extract(rnd, lo, h), want)


# ------------------------------------------------------------------ end to end
def test_extract_mesh_end_to_end(tmp_path):
    from splatco_amd import knn_grid, scene_io
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.synthetic import synthetic_anchor_model
    from splatco_amd.tsdf import extract_mesh
    W, H = 70, 52
    torch.manual_seed(11)
    pc = synthetic_anchor_model(3000, 9, DEV, plane_size=64)
    pc.feat_planes.Q0 = 3
    eyes = ((0.3, -0.2, -6.0), (6.0, 0.4, 0.3), (-0.3, 0.5, 6.0), (-6.0, -0.4, -0.2))
    cams = [look_at_camera(eye=e, target=(0, 0, 0), up=(0, -1, 0), FoVx=math.radians(60), width=W, height=H, uid=i).to(torch.device(DEV))
            for i, e in enumerate(eyes)]
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    bg = torch.ones(3, device=DEV)
    v, f, c = extract_mesh(cams, pc, pipe, bg, voxel_size=0.25, min_alpha=0.2)
    assert pc.get_color_mlp.training and pc.feat_planes.Q0 == 3                 # training mode and the plane noise are back
    lo, hi = knn_grid.bounds(pc.get_anchor.detach())
    print(f"extract_mesh: {v.shape[0]} vertices, {f.shape[0]} faces")
    assert v.shape[0] > 0 and f.shape[0] > 0 and tuple(c.shape) == tuple(v.shape) and v.is_cuda
    vn, fn, cn = v.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy()
    assert np.isfinite(vn).all() and (vn >= lo - 1.0 - 1e-5).all() and (vn <= hi + 1.0 + 0.25 + 1e-5).all()
    assert fn.min() >= 0 and fn.max() < v.shape[0] and len(np.unique(fn)) == v.shape[0]
    assert np.isfinite(cn).all() and cn.min() >= -1e-6 and cn.max() <= 1.0 + 1e-6
    path = str(tmp_path / "mesh.ply")
    scene_io.write_ply_mesh(path, v, f, c)
    v2, f2, c2 = scene_io.read_ply_mesh(path)
    assert np.array_equal(v2, vn) and np.array_equal(f2, fn) and np.abs(c2 - np.clip(cn, 0, 1)).max() <= 0.5 / 255 + 1e-7
    # the same call without colour, in explicit bounds
    v3, f3, c3 = extract_mesh(cams[:2], pc, pipe, bg, voxel_size=0.5, bounds=((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)), min_alpha=0.2, color=False)
    assert c3 is None and v3.shape[0] > 0 and float(v3.min()) >= -2.0 - 1e-5 and float(v3.max()) <= 2.0 + 1e-5
