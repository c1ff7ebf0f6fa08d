"""The block-sparse TSDF volume on the device (splatco_amd.tsdf_sparse, csrc/tsdf_sparse.hip): allocation against the numpy rule
(tests/tsdf_sparse_ref.py) and against the band of a device dense volume, integration and extraction against the dense family
bit for bit (both sides run the same device code: no exclusions, no tolerance), growth, determinism, refusals and
extract_mesh(sparse=True)."""
import functools
import math
import types

import numpy as np
import pytest
import torch

import tsdf_ref as ref
import tsdf_sparse_ref as sref
import splatco_amd.tsdf_sparse                # noqa: F401  (the module under test: without it nothing here can run)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(40, 27, 19), (17, 9, 10), (9, 8, 17)]        # the latter two have last blocks of 1 node along x


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)            # a copy: the shared references are read-only


def _upload(views):
    """(depths, alphas, cams, images, masks) on the device."""
    return ([_dev(v["depth"]) for v in views], [_dev(v["alpha"]) for v in views], [(v["intr"], torch.from_numpy(v["w2c"])) for v in views],
            [_dev(v["image"]) for v in views], [_dev(v["mask"]) for v in views])


@functools.lru_cache(maxsize=None)
def _parity(dims):
    lo, h = ref.volume_geometry(dims)
    return lo, h, ref.parity_views(dims)


def _sparse(dims, lo, h, **kw):
    from splatco_amd.tsdf_sparse import SparseTSDFVolume
    return SparseTSDFVolume(lo, float(h), dims, device=DEV, **kw)


def _dense(dims, lo, h, **kw):
    from splatco_amd.tsdf import TSDFVolume
    return TSDFVolume(lo, float(h), dims, device=DEV, **kw)


def _blocks(vol):
    """bool [nbz, nby, nbx] numpy: the allocated blocks."""
    nbx, nby, nbz = vol.block_dims
    out = np.zeros(nbx * nby * nbz, bool)
    out[vol.keys.cpu().numpy()] = True
    return out.reshape(nbz, nby, nbx)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_layout(vol):
    """keys ascending and distinct, slots a permutation of the rows 0 .. Nb - 1, the block coordinates those of the keys."""
    keys, slots = vol.keys.cpu().numpy(), vol.slots.cpu().numpy()
    assert keys.dtype == np.int32 and slots.dtype == np.int32 and (np.diff(keys) > 0).all()
    assert sorted(slots.tolist()) == list(range(len(keys))) and vol.num_blocks == len(keys) <= vol.capacity
    nbx, nby, _ = vol.block_dims
    want = np.stack((keys % nbx, keys // nbx % nby, keys // (nbx * nby)), 1)
    assert np.array_equal(vol.block_coords().cpu().numpy(), want)
    return keys, slots


def _assert_equals_dense_on_blocks(sparse, dense, blocks=None, names=("tsdf", "weight", "color")):
    """to_dense() of the sparse volume carries the dense volume's bits on the nodes of `blocks` (default: the allocated ones) and
    a fresh volume's on every other node."""
    got = sparse.to_dense()
    allocated = torch.from_numpy(sref.nodes_of(_blocks(sparse), sparse.dims)).to(DEV)
    inside = allocated if blocks is None else torch.from_numpy(sref.nodes_of(blocks, sparse.dims)).to(DEV)
    for name in names:
        g, d = getattr(got, name), getattr(dense, name)
        assert g.shape == d.shape and g.dtype == d.dtype
        assert torch.equal(_bits(g)[..., inside], _bits(d)[..., inside]), name
        fresh = 1.0 if name == "tsdf" else 0.0
        assert bool((g[..., ~allocated] == fresh).all()), f"{name}: an unallocated node is not fresh"


# ------------------------------------------------------------------ 1. allocation
@pytest.mark.parametrize("dims", SHAPES)
def test_allocation_follows_the_rule_and_covers_the_band(dims):
    lo, h, views = _parity(dims)
    trunc = 4.0 * float(h)
    D, A, cams, _, masks = _upload(views)
    for i, view in enumerate(views):
        vol = _sparse(dims, lo, h)
        new = vol.allocate(D[i], A[i], cams[i], mask=masks[i])
        got = _blocks(vol)
        inner, outer = (sref.allocate_ref(dims, lo, h, trunc, view, pad=float(h) * (0.125 + e)) for e in (-1e-6, 1e-6))
        print(f"dims {dims} view {i}: {new} of {got.size} blocks allocated, rule {int(inner.sum())} .. {int(outer.sum())}")
        assert new == vol.num_blocks == int(got.sum()) > 0
        assert not (inner & ~got).any() and not (got & ~outer).any()
        keys, slots = _assert_layout(vol)
        assert np.array_equal(slots, np.arange(len(keys)))          # one allocation: the rows follow the ascending keys
        assert vol.allocate(D[i], A[i], cams[i], mask=masks[i]) == 0 and np.array_equal(_blocks(vol), got)
        dense = _dense(dims, lo, h, color=False)
        dense.integrate(D[i], A[i], cams[i], mask=masks[i])
        band = sref.blocks_of(((dense.weight > 0) & (dense.tsdf < 1)).cpu().numpy())
        assert band.any() and not (band & ~got).any(), f"{int((band & ~got).sum())} band blocks were not allocated"
        # fresh storage: tsdf 1, weight 0, colour 0 on every allocated row
        n = vol.num_blocks
        assert bool((vol.tsdf[:n] == 1).all()) and bool((vol.weight[:n] == 0).all()) and bool((vol.color[:n] == 0).all())


def test_rows_are_given_in_allocation_order():
    dims = SHAPES[0]
    lo, h, views = _parity(dims)
    D, A, cams, _, masks = _upload(views)
    vol = _sparse(dims, lo, h, capacity=2)
    seen = {}
    for i in (2, 1, 0):                                  # the corner view first: the later views add blocks among its keys
        old = vol.num_blocks
        new = vol.allocate(D[i], A[i], cams[i], mask=masks[i])
        keys, slots = _assert_layout(vol)
        fresh = [k for k in keys.tolist() if k not in seen]
        assert len(fresh) == new > 0
        for rank, k in enumerate(fresh):                 # ascending: keys is
            seen[k] = old + rank
        assert [seen[k] for k in keys.tolist()] == slots.tolist()
    assert vol.capacity >= vol.num_blocks > 2


# ------------------------------------------------------------------ 2. two-pass: the dense volume on every allocated block
@pytest.mark.parametrize("dims", SHAPES)
def test_two_pass_gives_the_dense_volume_on_every_allocated_block(dims):
    lo, h, views = _parity(dims)                         # float32, uint8 and bool masks; every kind of hole
    D, A, cams, images, masks = _upload(views)
    dense = _dense(dims, lo, h)
    dense.integrate_views(D, A, cams, images, masks)
    vol = _sparse(dims, lo, h)
    vol.integrate_views(D, A, cams, images, masks, two_pass=True)
    _assert_layout(vol)
    assert 0 < vol.num_blocks and int(vol.weight[:vol.num_blocks].max()) >= 2
    _assert_equals_dense_on_blocks(vol, dense)
    plain = _sparse(dims, lo, h, color=False)
    plain.integrate_views(D, A, cams, None, masks, two_pass=True)
    assert plain.color is None and torch.equal(plain.keys, vol.keys) and torch.equal(plain.slots, vol.slots)
    n = vol.num_blocks
    assert torch.equal(_bits(plain.tsdf[:n]), _bits(vol.tsdf[:n])) and torch.equal(_bits(plain.weight[:n]), _bits(vol.weight[:n]))


# ------------------------------------------------------------------ 3. streaming: a block holds the views from its first sighting on
def test_streaming_blocks_hold_the_views_since_their_allocation():
    dims = SHAPES[0]
    lo, h, views = _parity(dims)
    order = (2, 1, 0)                                    # the corner view first, so that later views allocate new blocks
    D, A, cams, images, masks = _upload([views[i] for i in order])
    vol = _sparse(dims, lo, h)
    first = np.full(_blocks(vol).shape, -1)
    for a in range(3):
        vol.integrate(D[a], A[a], cams[a], image=images[a], mask=masks[a])
        first[_blocks(vol) & (first < 0)] = a
    assert all((first == a).any() for a in range(3)), "every view must allocate blocks of its own for this test to bite"
    for a in range(3):
        dense = _dense(dims, lo, h)
        dense.integrate_views(D[a:], A[a:], cams[a:], images[a:], masks[a:])
        _assert_equals_dense_on_blocks(vol, dense, blocks=first == a)


# ------------------------------------------------------------------ 4. extraction
def _soups(sparse_mesh, dense_mesh):
    """The two meshes as canonical faces over ONE numbering of the distinct (position bits, colour bits) rows."""
    rows, faces = [], []
    for v, f, c in (sparse_mesh, dense_mesh):
        r = v.cpu().numpy().view(np.int32)
        rows.append(r if c is None else np.concatenate((r, c.cpu().numpy().view(np.int32)), 1))
        faces.append(f.cpu().numpy().astype(np.int64))
    uniq, inv = np.unique(np.concatenate(rows), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    a, b = inv[:len(rows[0])], inv[len(rows[0]):]
    assert len(np.unique(a)) == len(a) and len(np.unique(b)) == len(b), "a mesh lists a vertex twice"
    return ref.canonical_faces(a[faces[0]]), ref.canonical_faces(b[faces[1]])


def _assert_same_mesh(vol, dense, min_weight=0.0, expect_faces=True):
    """vol.extract() against TSDFVolume.extract on the dense volume whose weights are zeroed outside the allocated blocks."""
    from splatco_amd.tsdf import TSDFVolume
    allocated = torch.from_numpy(sref.nodes_of(_blocks(vol), vol.dims)).to(DEV)
    masked = TSDFVolume.from_tensors(dense.lo, dense.voxel_size, dense.tsdf, dense.weight * allocated, dense.color, trunc=dense.trunc)
    got, want = vol.extract(min_weight), masked.extract(min_weight)
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (got[0].shape, want[0].shape, got[1].shape, want[1].shape)
    assert got[1].dtype == torch.int32 and (got[2] is None) == (want[2] is None)
    assert not expect_faces or got[1].shape[0] > 0
    if got[1].shape[0]:
        assert int(got[1].min()) == 0 and int(got[1].max()) == got[0].shape[0] - 1 and len(torch.unique(got[1])) == got[0].shape[0]
    s, d = _soups(got, want)
    assert np.array_equal(s, d)
    return got


@functools.lru_cache(maxsize=None)
def _sphere():
    from splatco_amd.tsdf import TSDFVolume
    vol, lo, h, _, _ = ref.sphere_volume((24, 24, 24))   # the surface crosses the block faces at 8 and 16
    return TSDFVolume.from_tensors(lo, float(h), _dev(vol["tsdf"]), _dev(vol["weight"]), _dev(vol["color"]))


def test_extraction_of_the_sphere_across_block_faces():
    from splatco_amd.tsdf_sparse import SparseTSDFVolume
    dense = _sphere()
    vol = SparseTSDFVolume.from_dense(dense)
    assert vol.num_blocks == 27 and vol.block_dims == (3, 3, 3)
    _assert_layout(vol)
    _assert_equals_dense_on_blocks(vol, dense)
    v, f, c = _assert_same_mesh(vol, dense)
    ref.assert_closed_manifold(v.cpu().numpy(), f.cpu().numpy())
    # the compactions cut into passes of 1, 4 and 26 blocks (27 = 6 x 4 + 3 = 26 + 1): the same bits, the same order
    for blocks in (1, 4, 26):
        got = vol.extract(pass_blocks=blocks)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, (v, f, c))), blocks
    part = vol.extract(min_weight=1.0, pass_blocks=5)
    assert part[0].shape == (0, 3) and part[1].shape == (0, 3) and part[2].shape == (0, 3)


def test_extraction_with_a_block_missing_and_with_min_weight():
    from splatco_amd.tsdf import TSDFVolume
    from splatco_amd.tsdf_sparse import SparseTSDFVolume
    dense = _sphere()
    mask = torch.ones(3, 3, 3, dtype=torch.bool, device=DEV)
    mask[0, 1, 1] = False                                # the block under the sphere's south pole
    vol = SparseTSDFVolume.from_dense(dense, blocks=mask)
    assert vol.num_blocks == 26 and (0 * 3 + 1) * 3 + 1 not in vol.keys.tolist()
    v, f, _ = _assert_same_mesh(vol, dense)
    assert len(ref.mesh_report(v.cpu().numpy(), f.cpu().numpy())["boundary"]) > 0          # the hole has a rim
    by_keys = SparseTSDFVolume.from_dense(dense, blocks=vol.keys.flip(0))
    assert torch.equal(by_keys.keys, vol.keys) and torch.equal(_bits(by_keys.tsdf), _bits(vol.tsdf))
    # min_weight acts as in the dense family: weight 2 on a slab of nodes, 1 elsewhere
    w = dense.weight.clone()
    w[:, :, 5:14] = 2.0
    heavy = TSDFVolume.from_tensors(dense.lo, dense.voxel_size, dense.tsdf, w, dense.color)
    hv = SparseTSDFVolume.from_dense(heavy)
    full = _assert_same_mesh(hv, heavy, min_weight=0.0)
    part = _assert_same_mesh(hv, heavy, min_weight=1.0)
    assert 0 < part[1].shape[0] < full[1].shape[0]
    none = _assert_same_mesh(hv, heavy, min_weight=2.0, expect_faces=False)
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3) and none[2].shape == (0, 3)


def test_extraction_of_an_empty_volume_and_of_the_fused_orbit():
    dims = (20, 20, 20)
    lo, h = ref.volume_geometry(dims, 0.06)
    empty = _sparse(dims, lo, h)
    v, f, c = empty.extract()
    assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3) and f.dtype == torch.int32 and v.is_cuda
    assert _sparse(dims, lo, h, color=False).extract()[2] is None
    views = ref.orbit_views(7, 30, 40, dims, 0.06, holes=True)
    D, A, cams, images, _ = _upload(views)
    dense = _dense(dims, lo, h)
    dense.integrate_views(D, A, cams, images)
    vol = _sparse(dims, lo, h)
    vol.integrate_views(D, A, cams, images, two_pass=True)
    assert 0 < vol.num_blocks <= 27
    _assert_equals_dense_on_blocks(vol, dense)
    v, f, c = _assert_same_mesh(vol, dense)
    assert c is not None and bool(torch.isfinite(c).all()) and f.shape[0] > 100


# ------------------------------------------------------------------ 5. growth and determinism
def test_growth_from_one_row_and_a_second_run_give_the_same_bits():
    dims = SHAPES[0]
    lo, h, views = _parity(dims)
    D, A, cams, images, masks = _upload(views)

    def run(capacity):
        vol = _sparse(dims, lo, h, capacity=capacity)
        for i in (2, 1, 0):
            vol.integrate(D[i], A[i], cams[i], image=images[i], mask=masks[i])
        n = vol.num_blocks
        return vol, [vol.keys, vol.slots, _bits(vol.tsdf[:n]), _bits(vol.weight[:n]), _bits(vol.color[:n])] + [_bits(t) for t in vol.extract()]

    small, base = run(1)
    assert small.capacity >= small.num_blocks > 8
    for capacity in (4096, 1):
        vol, got = run(capacity)
        assert capacity == 1 or vol.capacity == 4096
        assert len(got) == len(base) and all(torch.equal(a, b) for a, b in zip(got, base)), capacity


# ------------------------------------------------------------------ 6. refusals
def test_cpu_maps_are_refused_before_any_launch_and_max_blocks_holds(monkeypatch):
    from splatco_amd import _C
    dims = SHAPES[0]
    lo, h, views = _parity(dims)
    D, A, cams, images, masks = _upload(views[:1])
    vol = _sparse(dims, lo, h, max_blocks=3)
    with pytest.raises(RuntimeError, match="max_blocks"):
        vol.allocate(D[0], A[0], cams[0], mask=masks[0])
    assert vol.capacity == 60
    assert vol.num_blocks == 0 and int(vol._marks.max()) == 0                   # nothing grew, no mark is left behind
    with pytest.raises(RuntimeError, match="max_blocks"):
        vol.integrate(D[0], A[0], cams[0], image=images[0], mask=masks[0])
    assert vol.num_blocks == 0
    made = []
    monkeypatch.setattr(_C, "family_call", lambda *a, **k: made.append(a[0]))
    with pytest.raises(ValueError, match="cpu"):
        vol.allocate(D[0].cpu(), A[0], cams[0])
    with pytest.raises(ValueError, match="cpu"):
        vol.integrate(D[0], A[0], cams[0], image=images[0].cpu())
    with pytest.raises(ValueError, match="cpu"):
        vol.integrate_views(D, A, cams, masks=[masks[0].cpu()], two_pass=True)
    with pytest.raises(ValueError, match="alpha"):
        vol.integrate(D[0], A[0][:5], cams[0])
    assert made == []


# ------------------------------------------------------------------ 7. extract_mesh(sparse=True)
def test_extract_mesh_sparse_equals_the_manual_loop():
    from splatco_amd import knn_grid
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.evaluate import _eval_mode
    from splatco_amd.mesh import clean_mesh
    from splatco_amd.renderer import prefilter_voxel, render
    from splatco_amd.synthetic import synthetic_anchor_model
    from splatco_amd.tsdf import extract_mesh
    from splatco_amd.tsdf_sparse import SparseTSDFVolume
    W, H = 70, 52                                        # the small scene of the dense end-to-end test
    torch.manual_seed(11)
    pc = synthetic_anchor_model(3000, 9, DEV, plane_size=64)
    pc.feat_planes.Q0 = 3
    eyes = ((0.3, -0.2, -6.0), (6.0, 0.4, 0.3), (-0.3, 0.5, 6.0), (-6.0, -0.4, -0.2))
    cams = [look_at_camera(eye=e, target=(0, 0, 0), up=(0, -1, 0), FoVx=math.radians(60), width=W, height=H, uid=i).to(torch.device(DEV))
            for i, e in enumerate(eyes)]
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    bg = torch.ones(3, device=DEV)
    v, f, c = extract_mesh(cams, pc, pipe, bg, voxel_size=0.25, min_alpha=0.2, sparse=True)
    assert pc.get_color_mlp.training and pc.feat_planes.Q0 == 3
    lo, hi = knn_grid.bounds(pc.get_anchor.detach())
    vol = SparseTSDFVolume.from_bounds(np.asarray(lo, np.float64) - 1.0, np.asarray(hi, np.float64) + 1.0, 0.25, trunc=1.0, device=DEV)
    with _eval_mode(pc), torch.no_grad():
        for cam in cams:
            out = render(cam, pc, pipe, bg, visible_mask=prefilter_voxel(cam, pc, pipe, bg), aux=True)
            vol.integrate(out["depth"], out["alpha"], cam, image=out["render"], min_alpha=0.2)
    v2, f2, c2 = vol.extract()
    print(f"extract_mesh(sparse=True): {v.shape[0]} vertices, {f.shape[0]} faces, {vol.num_blocks} blocks")
    assert v.shape[0] > 0 and f.shape[0] > 0 and v.is_cuda
    assert torch.equal(_bits(v), _bits(v2)) and torch.equal(f, f2) and torch.equal(_bits(c), _bits(c2))
    cleaned = clean_mesh(v, f, c, keep_largest=1)
    assert cleaned[0].shape[0] > 0 and cleaned[1].shape[0] > 0
    v3, f3, _ = extract_mesh(cams, pc, pipe, bg, voxel_size=0.25, min_alpha=0.2, sparse=True, keep_largest=1)
    assert torch.equal(_bits(v3), _bits(cleaned[0])) and torch.equal(f3, cleaned[1])
