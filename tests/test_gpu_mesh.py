"""splatco_amd.mesh on the device against tests/mesh_ref.py: integer outputs and copied floats equal the reference exactly, and
so do the normals, bit for bit (every operation between the float32 inputs and the float32 outputs is a correctly rounded
binary64 operation, followed by one rounding)."""
import functools

import numpy as np
import pytest
import torch

import mesh_ref as ref
import tsdf_ref
import splatco_amd.mesh                       # noqa: F401  (the module under test: without it nothing here can run)
from splatco_amd.mesh import clean_mesh, connected_components, vertex_normals

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_components(got, want):
    for g, w in zip(got, want):
        g = _np(g)
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w)


def _same_mesh(got, want):
    """(vertices, faces, colors, info) of clean_mesh against clean_ref's."""
    v, f, c, info = got
    wv, wf, wc, winfo = want
    assert info == winfo
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and tuple(v.shape) == wv.shape and tuple(f.shape) == wf.shape
    assert np.array_equal(_bits(_np(v)), _bits(wv)) and np.array_equal(_np(f), wf)
    assert (c is None) == (wc is None)
    if c is not None:
        assert c.dtype == torch.float32 and np.array_equal(_bits(_np(c)), _bits(wc))


def _check_kept(got, v, f, labels, counts_of_label, t):
    """On a result: re-running connected_components confirms what was kept, every vertex is referenced, order is preserved."""
    v2, f2, _, info = got
    keep_v = counts_of_label[labels] >= t
    assert np.array_equal(_bits(_np(v2)), _bits(v[keep_v]))                       # the kept vertices, in their order
    f2n = _np(f2)
    assert np.array_equal(_np(v2)[f2n], v[f[keep_v[f[:, 0]]]])                    # the kept faces, in their order
    if len(f2n):
        assert np.array_equal(np.unique(f2n), np.arange(len(v2)))                   # every vertex is referenced
        l2, r2, c2 = connected_components(f2, v2.shape[0])
        assert len(r2) == info["components_kept"] and int(c2.min()) >= t and int(c2.sum()) == len(f2n)
        assert sorted(_np(c2).tolist()) == sorted(counts_of_label[counts_of_label >= t].tolist())


# ------------------------------------------------------------------ components
@pytest.mark.parametrize("n_parts,unref,seed", [(1, 0, 0), (4, 0, 1), (9, 3, 2), (400, 57, 3)])
def test_components_of_template_meshes(n_parts, unref, seed):
    v, f, part, _ = ref.mixed_mesh(n_parts, unref, seed)
    want = ref.components_ref(f, len(v))
    assert np.array_equal(want[0], ref.labels_by_construction(part))
    got = connected_components(_dev(f), len(v))
    _same_components(got, want)
    _same_components(connected_components(_dev(f.astype(np.int64)), len(v)), want)      # int64 faces
    _same_components(connected_components(_dev(f), len(v)), want)                       # a second run: the same bits


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3001])
def test_compaction_sizes(n):
    """Nv = Nf = n at the edges of compact.h's 1024-item workgroups: roots, kept vertices and kept faces."""
    v, f, part, _ = ref.sized_mesh(n, seed=n)
    assert len(v) == n and len(f) == n
    c = np.random.default_rng(n).random(v.shape).astype(np.float32)
    want = ref.components_ref(f, n)
    _same_components(connected_components(_dev(f), n), want)
    for kw in (dict(), dict(min_faces=2), dict(keep_largest=3)):
        _same_mesh(clean_mesh(_dev(v), _dev(f), _dev(c), **kw), ref.clean_ref(v, f, c, **kw))
    # every vertex kept but one: the kept counts sit at the edges too
    if n > 1:
        _same_mesh(clean_mesh(_dev(v), _dev(f[1:]), None), ref.clean_ref(v, f[1:], None))
    assert np.array_equal(_bits(_np(vertex_normals(_dev(v), _dev(f)))), _bits(ref.normals_ref(v, f)))


@functools.lru_cache(maxsize=None)
def _soup():
    return ref.triangle_soup(1_100_000, 1234, seed=8)


def test_large_mesh_of_single_triangles():
    """3.3 M vertices in 1.1 M components: the compaction scan sees more than 1024 workgroup counts (3224 for the roots, 1075
    for the faces).  Expected values come from the construction."""
    v, f, labels = _soup()
    nv, nf = len(v), len(f)
    fd = _dev(f)
    got_l, got_r, got_c = connected_components(fd, nv)
    assert torch.equal(got_l, _dev(labels))
    roots = np.nonzero(labels == np.arange(nv))[0].astype(np.int32)
    assert len(roots) == nf + 1234 and torch.equal(got_r, _dev(roots))
    is_face_root = np.zeros(nv, bool)
    is_face_root[f.min(1)] = True
    assert torch.equal(got_c, _dev(is_face_root[roots].astype(np.int32)))
    vd = _dev(v)
    v2, f2, c2, info = clean_mesh(vd, fd)
    ref_v = np.zeros(nv, bool)
    ref_v[f.reshape(-1)] = True
    assert c2 is None and info == dict(components=nf + 1234, components_kept=nf, threshold=1, vertices_before=nv, vertices_after=3 * nf,
                                       faces_before=nf, faces_after=nf)
    assert torch.equal(v2, vd[_dev(ref_v)])
    remap = np.cumsum(ref_v) - 1
    assert torch.equal(f2, _dev(remap[f].astype(np.int32)))


def test_deep_tree():
    """A strip of 5000 triangles numbered descending and interleaved, faces from the far end: hooking builds a deep tree."""
    v, f = ref.deep_strip(5000)
    want = ref.components_ref(f, len(v))
    assert want[1].tolist() == [0] and want[2].tolist() == [5000]
    for faces in (f, f[::-1].copy(), f[np.random.default_rng(2).permutation(len(f))]):
        _same_components(connected_components(_dev(faces), len(v)), want)
    # two such strips and a bridge: one face joins them late
    f2 = np.concatenate((f, f + len(v), [[len(v) - 1, len(v), 2 * len(v) - 1]])).astype(np.int32)
    _same_components(connected_components(_dev(f2), 2 * len(v)), ref.components_ref(f2, 2 * len(v)))


# ------------------------------------------------------------------ the filter
@functools.lru_cache(maxsize=None)
def _filter_mesh():
    """Tetrahedra and strips (4 faces), triangles and degenerate faces (1 face), one 12-face strip-pair, unreferenced
    vertices: ties at every interesting place."""
    big = (10, [(0, 1, 2), (1, 3, 2), (2, 3, 4), (3, 5, 4), (4, 5, 6), (5, 7, 6), (6, 7, 8), (7, 9, 8), (0, 2, 1), (1, 2, 3), (8, 7, 9), (9, 9, 0)])
    parts = [ref.TEMPLATES[i % 4] for i in range(22)] + [big]
    v, f, part, faces_of = ref.assemble(parts, unreferenced=9, seed=12)
    c = np.random.default_rng(5).random(v.shape).astype(np.float32)
    labels, roots, counts = ref.components_ref(f, len(v))
    counts_of_label = np.zeros(len(v), np.int64)
    counts_of_label[roots] = counts
    return v, f, c, labels, counts_of_label, sorted(counts.tolist(), reverse=True)


@pytest.mark.parametrize("kw,t", [
    (dict(keep_largest=1), 12),
    (dict(keep_largest=5), 4),                    # the 5th largest is one of twelve components with 4 faces: all are kept
    (dict(keep_largest=13), 4),
    (dict(keep_largest=14), 1),
    (dict(keep_largest=32), 1),                   # Nc = 32 with the unreferenced vertices: the K-th count is 0, t stays 1
    (dict(keep_largest=1000), 1),                 # more than there are components: not taken
    (dict(min_faces=0), 1), (dict(min_faces=2), 2), (dict(min_faces=4), 4), (dict(min_faces=5), 5), (dict(min_faces=12), 12),
    (dict(keep_largest=5, min_faces=2), 4), (dict(keep_largest=5, min_faces=6), 6), (dict(keep_largest=1, min_faces=3), 12),
    (dict(), 1),
])
@pytest.mark.parametrize("colors,int64", [(True, False), (False, True)])
def test_filter(kw, t, colors, int64):
    v, f, c, labels, counts_of_label, ranked = _filter_mesh()
    assert ranked[:14] == [12] + [4] * 12 + [1] and ranked[22:24] == [1, 0] and len(ranked) == 32
    c = c if colors else None
    want = ref.clean_ref(v, f, c, **kw)
    assert want[3]["threshold"] == t
    got = clean_mesh(_dev(v), _dev(f.astype(np.int64) if int64 else f), _dev(c), **kw)
    _same_mesh(got, want)
    _check_kept(got, v, f, labels, counts_of_label, t)
    again = clean_mesh(_dev(v), _dev(f), _dev(c), **kw)
    assert all(torch.equal(a, b) for a, b in zip(got[:2], again[:2])) and got[3] == again[3]


@pytest.mark.parametrize("colors", (False, True))
def test_filter_that_removes_everything_and_empty_inputs(colors):
    v, f, c, *_ = _filter_mesh()
    c = c if colors else None
    for kw in (dict(min_faces=13), dict(keep_largest=1, min_faces=100), dict(min_faces=2 ** 40)):
        v2, f2, c2, info = clean_mesh(_dev(v), _dev(f), _dev(c), **kw)
        assert tuple(v2.shape) == (0, 3) and v2.dtype == torch.float32 and tuple(f2.shape) == (0, 3) and f2.dtype == torch.int32
        assert (c2 is None) if c is None else (tuple(c2.shape) == (0, 3) and c2.dtype == torch.float32)
        assert v2.device == f2.device == torch.device(DEV)
        assert info["components"] == 32 and info["components_kept"] == 0 and info["vertices_after"] == 0 and info["faces_after"] == 0
        assert info["threshold"] == ref.clean_ref(v, f, c, **kw)[3]["threshold"]
    none_f = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    v2, f2, c2, info = clean_mesh(_dev(v), none_f, _dev(c))
    assert tuple(v2.shape) == (0, 3) and tuple(f2.shape) == (0, 3) and info["components"] == len(v) and info["vertices_before"] == len(v)
    v2, f2, c2, info = clean_mesh(torch.zeros(0, 3, device=DEV), none_f, None)
    assert tuple(v2.shape) == (0, 3) and tuple(f2.shape) == (0, 3) and c2 is None and info["components"] == 0
    labels, roots, counts = connected_components(none_f, 5)
    assert labels.tolist() == [0, 1, 2, 3, 4] and roots.tolist() == [0, 1, 2, 3, 4] and counts.tolist() == [0] * 5
    assert [x.numel() for x in connected_components(none_f, 0)] == [0, 0, 0]
    n = vertex_normals(_dev(v), none_f)
    assert tuple(n.shape) == v.shape and not n.any()
    assert tuple(vertex_normals(torch.zeros(0, 3, device=DEV), none_f).shape) == (0, 3)


# ------------------------------------------------------------------ normals
def _normals_match(v, f):
    want = ref.normals_ref(v, f)
    got = vertex_normals(_dev(v), _dev(f))
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    g = _np(got)
    diff = int((_bits(g) != _bits(want)).sum())
    print(f"normals: {len(v)} vertices, {len(f)} faces, {diff} of {want.size} components differ in their bits")
    assert diff == 0
    assert torch.equal(got, vertex_normals(_dev(v), _dev(f.astype(np.int64))))           # int64 faces, and a second run
    return g


def test_normals_alone():
    v, f = ref.octahedron()
    assert np.array_equal(_normals_match(v, f), v)
    # degenerate and duplicate-index faces, an unreferenced vertex, opposite faces that cancel to an exact zero
    v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (5, 5, 5), (0.25, 0.5, 1), (-1, 2, 0.125)], np.float32)
    f = np.array([(0, 1, 2), (1, 1, 0), (2, 0, 2), (4, 0, 1), (4, 4, 4), (1, 4, 2), (5, 1, 5), (2, 1, 0), (0, 1, 2)], np.int32)
    g = _normals_match(v, f)
    assert not g[3].any() and not g[5].any() and g[4].any()
    # a vertex of degree 70 and one of degree 300; random soup with repeated indices
    for n in (70, 300):
        g = _normals_match(*ref.fan(n))
        assert g[0, 2] > 0.9
    gen = np.random.default_rng(17)
    v = (gen.standard_normal((500, 3)) * np.array([1e-3, 1.0, 1e3])).astype(np.float32)
    _normals_match(v, gen.integers(0, 500, size=(4000, 3)).astype(np.int32))
    _normals_match(v[:40], gen.integers(0, 40, size=(3000, 3)).astype(np.int32))         # degree about 220 everywhere
    # the float32 range: float64 inside, no overflow; a non-finite position gives exactly 0 at the vertices it reaches
    big = np.array([(0, 0, 0), (3e38, 0, 0), (0, 3e38, 0), (1e-30, 0, 0), (0, 1e-30, 0)], np.float32)
    g = _normals_match(big, np.array([(0, 1, 2), (0, 3, 4)], np.int32))
    assert g.tolist() == [[0, 0, 1]] * 5
    bad = np.array([(0, 0, 0), (np.inf, 0, 0), (0, 1, 0), (np.nan, 1, 1), (1, 0, 0), (0, 0, 1)], np.float32)
    g = _normals_match(bad, np.array([(0, 1, 2), (0, 4, 5), (3, 4, 5)], np.int32))
    assert not g[:4].any() and not g[4].any() and not g[5].any()


def test_normals_of_the_template_meshes():
    for args in ((60, 9, 5), (700, 0, 6)):
        v, f, *_ = ref.mixed_mesh(*args)
        _normals_match(v, f)
    _normals_match(*ref.deep_strip(5000))


# ------------------------------------------------------------------ end to end
def test_fused_spheres_end_to_end(tmp_path):
    """Two spheres and a tiny blob fused from synthetic depth maps into a 40^3 volume: clean_mesh(keep_largest=1) leaves exactly
    the large sphere, and its normals match the reference and point away from its centre."""
    from splatco_amd import scene_io
    from splatco_amd.tsdf import TSDFVolume
    views, lo, h, dims, blobs = ref.blob_scene()
    vol = TSDFVolume(lo, float(h), dims, color=False, device=DEV)
    vol.integrate_views([_dev(x["depth"]) for x in views], [_dev(x["alpha"]) for x in views],
                        [(x["intr"], torch.from_numpy(x["w2c"])) for x in views])
    v, f, _ = vol.extract()
    vn, fn = _np(v), _np(f)
    (centre, radius), others = blobs[0], blobs[1:]
    dist = np.linalg.norm(vn.astype(np.float64) - centre, axis=1)
    on_big = np.abs(dist - radius) < 1.5 * float(h)
    for c, r in others:                                                            # the other two are there, and far away
        d = np.linalg.norm(vn.astype(np.float64) - c, axis=1)
        assert (np.abs(d - r) < 1.5 * float(h)).sum() > 50 and not (on_big & (d < r + 4 * float(h))).any()
    labels, roots, counts = connected_components(f, v.shape[0])
    _same_components((labels, roots, counts), ref.components_ref(fn, len(vn)))
    assert len(roots) >= 3
    got = clean_mesh(v, f, keep_largest=1)
    _same_mesh(got, ref.clean_ref(vn, fn, None, keep_largest=1))
    v2, f2, _, info = got
    assert info["components_kept"] == 1 and 3000 < info["vertices_after"] == int(on_big.sum())
    assert np.array_equal(_bits(_np(v2)), _bits(vn[on_big]))                       # exactly the large sphere's vertices
    assert np.array_equal(_np(v2)[_np(f2)], vn[fn[on_big[fn[:, 0]]]])              # and faces
    assert len(tsdf_ref.mesh_report(_np(v2), _np(f2))["boundary"]) == 0            # closed
    n = vertex_normals(v2, f2)
    want = ref.normals_ref(_np(v2), _np(f2))
    assert np.array_equal(_bits(_np(n)), _bits(want))
    rad = _np(v2).astype(np.float64) - centre
    dots = (_np(n).astype(np.float64) * rad / np.linalg.norm(rad, axis=1, keepdims=True)).sum(1)
    print(f"fused spheres: {len(vn)} vertices in {len(roots)} components (faces {sorted(_np(counts).tolist(), reverse=True)[:6]} ...), "
          f"kept {info['vertices_after']} vertices, {info['faces_after']} faces; smallest normal . radial = {dots.min():.4f}")
    assert (dots > 0).all()
    # and into a file with its normals
    path = str(tmp_path / "sphere.ply")
    scene_io.write_ply_mesh(path, v2, f2, None, normals=n)
    rv, rf, rc, rn = scene_io.read_ply_mesh(path, normals=True)
    assert np.array_equal(rv, _np(v2)) and np.array_equal(rf, _np(f2)) and rc is None and np.array_equal(_bits(rn), _bits(want))


def test_extract_mesh_ends_in_clean_mesh_when_asked():
    """tsdf.extract_mesh(..., keep_largest=, min_faces=): with both None today's function, the same bits; otherwise what
    clean_mesh makes of that mesh, as the same 3-tuple."""
    import math
    import types
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.synthetic import synthetic_anchor_model
    from splatco_amd.tsdf import extract_mesh
    torch.manual_seed(11)
    pc = synthetic_anchor_model(3000, 9, DEV, plane_size=64)
    eyes = ((0.3, -0.2, -6.0), (6.0, 0.4, 0.3))
    cams = [look_at_camera(eye=e, target=(0, 0, 0), up=(0, -1, 0), FoVx=math.radians(60), width=70, height=52, uid=i).to(torch.device(DEV))
            for i, e in enumerate(eyes)]
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    bg = torch.ones(3, device=DEV)
    args = dict(voxel_size=0.25, min_alpha=0.2)
    v, f, c = extract_mesh(cams, pc, pipe, bg, **args)
    v0, f0, c0 = extract_mesh(cams, pc, pipe, bg, keep_largest=None, min_faces=None, **args)
    assert torch.equal(v, v0) and torch.equal(f, f0) and torch.equal(c, c0) and f.shape[0] > 0
    counts = _np(connected_components(f, v.shape[0])[2])
    print(f"extract_mesh: {v.shape[0]} vertices, {f.shape[0]} faces, {len(counts)} components, largest {sorted(counts.tolist())[-3:]}")
    for kw in (dict(keep_largest=1), dict(min_faces=int(counts.max())), dict(keep_largest=2, min_faces=3)):
        out = extract_mesh(cams, pc, pipe, bg, **args, **kw)
        want = clean_mesh(v, f, c, **kw)
        assert len(out) == 3 and all(torch.equal(a, b) for a, b in zip(out, want[:3]))
        _same_mesh(want, ref.clean_ref(_np(v), _np(f), _np(c), **kw))
        assert 0 < out[1].shape[0] <= f.shape[0]


# ------------------------------------------------------------------ rejections
def test_rejections_launch_nothing(monkeypatch):
    from splatco_amd import _C
    v, f = ref.octahedron()
    vd, fd = _dev(v), _dev(f)
    made = []
    real = _C.family_call
    monkeypatch.setattr(_C, "family_call", lambda *a, **k: made.append(a[0]) or real(*a, **k))
    cases = [
        (lambda: connected_components(torch.from_numpy(f), 6), "cpu"),
        (lambda: vertex_normals(torch.from_numpy(v), fd), "cpu"),
        (lambda: vertex_normals(vd, torch.from_numpy(f)), "cpu"),
        (lambda: clean_mesh(vd, fd, torch.from_numpy(v)), "colors is on cpu"),
        (lambda: clean_mesh(vd, fd, vd[:5]), "5 colors for 6 vertices"),
        (lambda: clean_mesh(vd, fd, vd.double()), "float32"),
        (lambda: clean_mesh(vd[:, :2], fd), r"\[Nv, 3\]"),
        (lambda: clean_mesh(vd.double(), fd), "float32"),
        (lambda: clean_mesh(vd, fd[:, :2]), r"\[Nf, 3\]"),
        (lambda: clean_mesh(vd, fd.float()), "int32 or int64"),
        (lambda: connected_components(fd.reshape(-1), 6), r"\[Nf, 3\]"),
        (lambda: connected_components(fd, -1), "num_vertices"),
        (lambda: clean_mesh(vd, fd, keep_largest=0), "keep_largest"),
        (lambda: clean_mesh(vd, fd, min_faces=-1), "min_faces"),
    ]
    for index in (-1, 6):
        for dt in (torch.int32, torch.int64):
            bad = fd.to(dt).clone()
            bad[5, 1] = index
            cases += [(lambda bad=bad: connected_components(bad, 6), "outside"), (lambda bad=bad: clean_mesh(vd, bad), "outside"),
                      (lambda bad=bad: vertex_normals(vd, bad), "outside")]
    cases.append((lambda: connected_components(fd, 5), "outside"))                # an index of Nv
    for fn, text in cases:
        with pytest.raises(ValueError, match=text):
            fn()
    assert made == []
    # and the same arguments, put right, run
    assert connected_components(fd, 6)[1].tolist() == [0] and made[:1] == ["scr_mesh_components"]


def test_every_operator_twice_gives_the_same_bits():
    v, f, *_ = ref.mixed_mesh(900, 31, 9)
    c = np.random.default_rng(1).random(v.shape).astype(np.float32)
    vd, fd, cd = _dev(v), _dev(f), _dev(c)

    def run():
        out = list(connected_components(fd, len(v)))
        out += [x for x in clean_mesh(vd, fd, cd, keep_largest=50, min_faces=4)[:3]]
        out.append(vertex_normals(vd, fd))
        return out

    a, b = run(), run()
    assert len(a) == 7 and all(x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
