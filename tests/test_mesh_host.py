"""Mesh clean-up, everything that needs no device: the numpy restatement (tests/mesh_ref.py) on meshes whose components are
known by construction and against scipy, the C-ABI surface of include/splatco_mesh.h against _C.MESH_SIGNATURES,
_C.family_call, the argument rejections of the entry points and of splatco_amd.mesh, and the mesh PLY with normals."""
import ast
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

import mesh_ref as ref
import splatco_amd.mesh                       # noqa: F401  (the module under test: without it nothing here can run)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "splatco_mesh.h")
NAMES = ["scr_mesh_abi_version", "scr_mesh_scratch_bytes", "scr_mesh_components", "scr_mesh_roots_plan", "scr_mesh_roots_run",
         "scr_mesh_vertices_plan", "scr_mesh_vertices_run", "scr_mesh_faces_plan", "scr_mesh_faces_run", "scr_mesh_vertex_normals"]
STREAMED = [n for n in NAMES if n not in ("scr_mesh_abi_version", "scr_mesh_scratch_bytes")]


# ------------------------------------------------------------------ the reference alone
def test_reference_components_on_meshes_known_by_construction():
    for n_parts, unref, seed in ((1, 0, 0), (4, 0, 1), (9, 3, 2), (40, 7, 3)):
        v, f, part, faces_of = ref.mixed_mesh(n_parts, unref, seed)
        labels, roots, counts = ref.components_ref(f, len(v))
        want = ref.labels_by_construction(part)
        assert labels.dtype == np.int32 and np.array_equal(labels, want)
        assert np.array_equal(roots, np.unique(want)) and len(roots) == n_parts + unref
        by_root = {int(np.nonzero(part == i)[0].min()): int(faces_of[i]) for i in range(n_parts)}
        assert counts.tolist() == [by_root.get(int(r), 0) for r in roots]
        assert counts.sum() == len(f)
    # two tetrahedra that share ONE vertex are one component here (vertex connectivity); edge connectivity would say two
    f = np.array(ref.TETRA[1] + [(3, 4, 5), (3, 6, 4), (4, 6, 5), (3, 5, 6)])
    labels, roots, counts = ref.components_ref(f, 8)
    assert labels.tolist() == [0] * 7 + [7] and roots.tolist() == [0, 7] and counts.tolist() == [8, 0]
    # nothing at all, vertices without faces, a degenerate face
    assert [len(x) for x in ref.components_ref(np.zeros((0, 3), int), 0)] == [0, 0, 0]
    labels, roots, counts = ref.components_ref(np.zeros((0, 3), int), 3)
    assert labels.tolist() == [0, 1, 2] and counts.tolist() == [0, 0, 0]
    labels, roots, counts = ref.components_ref([(2, 2, 2), (1, 1, 0)], 3)
    assert labels.tolist() == [0, 0, 2] and roots.tolist() == [0, 2] and counts.tolist() == [1, 1]


def test_reference_components_against_scipy():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    for v, f in ([ref.mixed_mesh(60, 9, 5)[:2], ref.deep_strip(300)]):
        nv = len(v)
        i = np.concatenate((f[:, 0], f[:, 1])).astype(np.int64)
        j = np.concatenate((f[:, 1], f[:, 2])).astype(np.int64)
        g = sp.coo_matrix((np.ones(len(i)), (i, j)), shape=(nv, nv))
        nc, lab = connected_components(g, directed=False)
        labels, roots, counts = ref.components_ref(f, nv)
        assert nc == len(roots)
        first = np.full(nc, nv)
        np.minimum.at(first, lab, np.arange(nv))
        assert np.array_equal(first[lab], labels)
        assert np.array_equal(np.bincount(lab[f[:, 0]], minlength=nc)[lab[roots]], counts)


def test_reference_filter_and_threshold():
    assert ref.threshold_ref([5, 3, 3, 1], keep_largest=2) == 3                   # ties at the K-th place are all kept
    assert ref.threshold_ref([5, 3, 3, 1], keep_largest=5) == 1                   # fewer components than K: not taken
    assert ref.threshold_ref([5, 3, 3, 1], keep_largest=4, min_faces=2) == 2
    assert ref.threshold_ref([5, 3, 3, 0], keep_largest=4) == 1                   # never below 1
    assert ref.threshold_ref([5, 3], min_faces=0) == 1 and ref.threshold_ref([], keep_largest=1) == 1
    v, f, part, _ = ref.mixed_mesh(8, 5, 6)
    c = np.random.default_rng(0).random(v.shape).astype(np.float32)
    v2, f2, c2, info = ref.clean_ref(v, f, c, keep_largest=4)                     # 2 tetrahedra and 2 strips: 4 faces each
    assert info == dict(components=13, components_kept=4, threshold=4, vertices_before=len(v), vertices_after=20,
                        faces_before=len(f), faces_after=16)
    keep = np.isin(part, (0, 1, 4, 5))
    assert np.array_equal(v2, v[keep]) and np.array_equal(c2, c[keep]) and f2.dtype == np.int32
    assert np.array_equal(v2[f2], v[f[keep[f[:, 0]]]])                            # same faces in the same order
    assert len(np.unique(f2)) == len(v2)                                          # welded: none unused
    v3, f3, c3, info = ref.clean_ref(v, f, None, min_faces=5)
    assert v3.shape == (0, 3) and f3.shape == (0, 3) and c3 is None and info["components_kept"] == 0 and info["threshold"] == 5


def test_reference_normals():
    v, f = ref.octahedron()
    n = ref.normals_ref(v, f)
    assert np.array_equal(n, v)                                                   # outward, unit length, exactly
    for v, f in ((ref.mixed_mesh(12, 4, 7)[:2]), ref.fan(70), ref.deep_strip(40)):
        a, b = ref.normals_ref(v, f), ref.normals_loop_ref(v, f)
        assert a.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))
        length = np.linalg.norm(a.astype(np.float64), axis=1)
        assert (np.abs(length[length > 0] - 1) < 1e-6).all()
    # a face that holds a vertex twice is added once; an unreferenced vertex and a zero sum give exactly 0
    v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (5, 5, 5), (0, 0, 1)], np.float32)
    f = np.array([(0, 1, 2), (1, 1, 0), (2, 0, 2), (0, 2, 1), (4, 0, 1), (4, 1, 0)])
    n = ref.normals_ref(v, f)
    assert np.array_equal(n, ref.normals_loop_ref(v, f)) and not n.any()          # every face has its opposite or no area
    n = ref.normals_ref(v, f[:1])
    assert n.tolist() == [[0, 0, 1]] * 3 + [[0, 0, 0]] * 2
    big = np.array([(0, 0, 0), (3e38, 0, 0), (0, 3e38, 0)], np.float32)
    assert np.array_equal(ref.normals_ref(big, [(0, 1, 2)]), np.array([[0, 0, 1]] * 3, np.float32))      # float64 inside: no overflow
    assert not ref.normals_ref(np.array([(0, 0, 0), (np.inf, 0, 0), (0, 1, 0)], np.float32), [(0, 1, 2)]).any()


def test_deep_strip_and_fan_recipes():
    v, f = ref.deep_strip(5000)
    assert len(v) == 5002 and len(f) == 5000 and sorted(np.unique(f).tolist()) == list(range(5002))
    labels, roots, counts = ref.components_ref(f, len(v))
    assert not labels.any() and counts.tolist() == [5000]
    assert f[-1].tolist() == [0, 5001, 1] and f[0].tolist()[0] > 2000             # descending and interleaved
    v, f = ref.fan(70)
    assert (np.bincount(f.reshape(-1))[0]) == 70


def test_blob_scene_meets_the_preconditions_of_the_end_to_end_test():
    """On the numpy fusion and extraction (tests/tsdf_ref.py): three separate objects and a few floaters, the largest component
    is the large sphere's shell, closed, and nothing else lies near it."""
    import tsdf_ref
    views, lo, h, dims, blobs = ref.blob_scene()
    assert max(dims) <= 48 and [r for _, r in blobs] == sorted((r for _, r in blobs), reverse=True)
    vol, _ = tsdf_ref.integrate_views_ref(tsdf_ref.fresh(dims, color=False), lo, h, views, 4.0 * float(h))
    m = tsdf_ref.extract_ref(vol, lo, h)
    v, f = m["vertices"], m["faces"]
    labels, roots, counts = ref.components_ref(f, len(v))
    assert len(roots) > 3 and sorted(counts.tolist())[-3] > 100 and min(counts) < 20             # three objects, and floaters
    near = [np.abs(np.linalg.norm(v.astype(np.float64) - c, axis=1) - r) < 1.5 * float(h) for c, r in blobs]
    assert not (near[0] & near[1]).any() and not (near[0] & near[2]).any() and not (near[1] & near[2]).any()
    v2, f2, _, info = ref.clean_ref(v, f, None, keep_largest=1)
    assert info["components_kept"] == 1 and np.array_equal(v2, v[near[0]])
    assert len(tsdf_ref.mesh_report(v2, f2)["boundary"]) == 0
    n = ref.normals_ref(v2, f2)
    rad = v2.astype(np.float64) - blobs[0][0]
    assert ((n * rad).sum(1) / np.linalg.norm(rad, axis=1) > 0.5).all()


# ------------------------------------------------------------------ the header and the binding
_SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double}


def _header():
    hdr = open(HEADER).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    return hdr, re.sub(r"^\s*#[^\n]*", "", hdr, flags=re.M)


def _prototypes():
    protos = re.findall(r"([A-Za-z_][\w\s*]*?)\b(scr_\w+)\s*\(([^()]*)\)\s*;", _header()[1])
    return [(ret.strip(), name, [] if params.strip() == "void" else [p.strip() for p in params.split(",")])
            for ret, name, params in protos]


def _streamed():
    return {name: bool(params) and "".join(params[-1].split()) == "void*stream" for _, name, params in _prototypes()}


def _c_type(decl):
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    return next(w for w in words if w != "*"), words.count("*")


def _binds(decl, got):
    base, depth = _c_type(decl)
    if depth == 0:
        return got is _SCALARS.get(base, object())
    if decl.split()[-1].endswith("_host"):
        return base == "int64_t" and got is ctypes.POINTER(ctypes.c_int64)
    return got is ctypes.c_void_p


def test_binding_matches_the_header():
    from splatco_amd import _C
    hdr, _ = _header()
    m = re.search(r"^\s*#\s*define\s+SCR_MESH_ABI_VERSION\s+(\d+)\s*$", hdr, flags=re.M)
    assert m and int(m.group(1)) == _C.MESH_ABI_VERSION == _C.lib.scr_mesh_abi_version() == 1
    protos = _prototypes()
    assert [name for _, name, _ in protos] == [s[0] for s in _C.MESH_SIGNATURES] == NAMES
    for (ret, name, params), (_, restype, *argtypes) in zip(protos, _C.MESH_SIGNATURES):
        assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes for {len(params)} parameters"
        assert _binds(ret + " r", restype), f"{name}: restype {restype.__name__} does not bind {ret}"
        for i, (p, got) in enumerate(zip(params, argtypes)):
            assert _binds(p, got), f"{name} parameter {i} `{p}`: {got.__name__}"
        f = getattr(_C.lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, f"{name}: not bound from MESH_SIGNATURES"
    assert [n for n, s in _streamed().items() if s] == STREAMED
    assert [len(p) for _, _, p in protos] == [0, 2, 8, 6, 8, 7, 12, 8, 10, 7]
    assert _C._FAMILY_HEADERS["include/splatco_mesh.h"] is _C.MESH_SIGNATURES
    # the definition is in the header
    text = open(HEADER).read()
    for phrase in ("smallest vertex index", "VERTEX connectivity", "ASCENDING face index", "binary64", "threshold >= 1"):
        assert phrase in text, phrase


def test_every_declared_symbol_is_exported_and_the_other_headers_know_none_of_them():
    from splatco_amd import _C
    lib = ctypes.CDLL(os.path.join(ROOT, "splatco_amd", "csrc", "libsplatco_raster.so"))
    for name in NAMES:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert not [s for s in _C.SYMBOLS if s.startswith("scr_mesh")]
    assert not [s for s in _C.BILAGRID_SIGNATURES + _C.NORMALS_SIGNATURES + _C.TSDF_SIGNATURES if s[0].startswith("scr_mesh")]
    for other in ("splatco_raster.h", "splatco_bilagrid.h", "splatco_normals.h", "splatco_tsdf.h"):
        assert "scr_mesh" not in open(os.path.join(ROOT, "include", other)).read()
    assert _C.ABI_VERSION == 37 and _C.BILAGRID_ABI_VERSION == 1 and _C.NORMALS_ABI_VERSION == 1 and _C.TSDF_ABI_VERSION == 1
    # the size query (no device needed): one uint32 per workgroup of 1024 items of the larger compaction, + 1, 256-byte
    # aligned, + 256 for the total
    q = _C.lib.scr_mesh_scratch_bytes
    for nv, nf in ((3000, 5000), (5000, 10), (1, 0), (0, 0)):
        want = ((max(nv, nf, 1) + 1023) // 1024 + 1) * 4
        assert q(nv, nf) == want + (-want) % 256 + 256
    assert q(-1, 5) == 256 and q(2 ** 31, 5) == 256


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    return ".".join(reversed(parts + [node.id])) if isinstance(node, ast.Name) else ""


def test_the_module_launches_through_family_call_only():
    streamed = _streamed()
    tree = ast.parse(open(os.path.join(ROOT, "splatco_amd", "mesh.py")).read())
    called = []
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        name, where = _dotted(node.func), f"mesh.py:{node.lineno}"
        if name in ("_C.family_call", "family_call"):
            first = node.args[0] if node.args else None
            assert isinstance(first, ast.Constant) and isinstance(first.value, str), f"{where}: the name is not a string literal"
            assert streamed.get(first.value, False), f"{where}: {first.value} is not a streamed function of splatco_mesh.h"
            called.append(first.value)
        elif ".lib.scr_" in "." + name:
            assert not streamed.get(name.rsplit(".", 1)[1], True), f"{where}: {name} takes a stream: launch it through _C.family_call"
        else:
            assert name not in ("_C.call", "call"), f"{where}: this family launches through _C.family_call"
            assert not name.endswith("cuda.device"), f"{where}: torch.cuda.device(...) outside _C"
    assert sorted(set(called)) == sorted(STREAMED)


class _Recorder:
    def __init__(self, rc=0):
        self.rc, self.args = rc, None

    def __call__(self, *args):
        self.args = args
        return self.rc


def test_family_call_accepts_the_new_names_and_still_refuses_others(monkeypatch):
    from splatco_amd import _C
    other, own = _Recorder(), _Recorder()
    monkeypatch.setattr(_C.lib, "scr_depth_loss_forward", other)
    monkeypatch.setattr(_C.lib, "scr_mesh_vertex_normals", own)
    a = torch.zeros(4)
    for name in ("scr_depth_loss_forward", "scr_no_such_entry_point", "scr_mesh"):
        with pytest.raises(ValueError, match=name):
            _C.family_call(name, a)
    assert other.args is None
    with pytest.raises(ValueError) as e:
        _C.family_call("scr_mesh_vertex_normals", 4, 2, a, torch.zeros(4, device="meta"), None, None)
    assert "scr_mesh_vertex_normals" in str(e.value) and "argument 3" in str(e.value) and "meta" in str(e.value)
    assert own.args is None
    for name in NAMES:
        assert name in _C._FAMILY_NAMES
    assert "scr_bilagrid_slice" in _C._FAMILY_NAMES and "scr_normals_map" in _C._FAMILY_NAMES and "scr_tsdf_integrate" in _C._FAMILY_NAMES


@pytest.mark.skipif(torch.cuda.is_available(), reason="replays rejected calls only where nothing can be launched")
def test_c_abi_checks_sizes_and_scalars_first():
    """Validated before anything is launched; 16 stands for any non-null device address (never dereferenced on the host)."""
    from splatco_amd import _C
    lib, p = _C.lib, 16
    err = lambda: lib.scr_last_error().decode()
    cnt = ctypes.c_int64(7)
    ref_cnt = ctypes.byref(cnt)
    cases = [
        ("scr_mesh_components", lambda nv=5, nf=3, f=p, par=p, lab=p, vf=p, s=p: lib.scr_mesh_components(nv, nf, f, par, lab, vf, s, None),
         ((dict(nv=-1), "nv ="), (dict(nv=2 ** 31), "nv ="), (dict(nf=-1), "nf ="), (dict(nf=2 ** 31 // 3 + 1), "3 nf"), (dict(nv=0), "no vertices"),
          (dict(s=None), "status"), (dict(par=None), "NULL"), (dict(lab=None), "NULL"), (dict(vf=None), "NULL"), (dict(f=None), "faces"))),
        ("scr_mesh_roots_plan", lambda nv=5, lab=p, s=p, sc=p, c=ref_cnt: lib.scr_mesh_roots_plan(nv, lab, s, sc, c, None),
         ((dict(c=None), "count_host"), (dict(nv=0), "nv ="), (dict(nv=2 ** 31), "nv ="), (dict(lab=None), "NULL"), (dict(s=None), "NULL"),
          (dict(sc=None), "NULL"))),
        ("scr_mesh_roots_run", lambda nv=5, lab=p, vf=p, sc=p, nc=2, r=p, fc=p: lib.scr_mesh_roots_run(nv, lab, vf, sc, nc, r, fc, None),
         ((dict(nv=0), "nv ="), (dict(nc=-1), "nc ="), (dict(nc=6), "nc ="), (dict(lab=None), "NULL"), (dict(r=None), "NULL"), (dict(fc=None), "NULL"))),
        ("scr_mesh_vertices_plan", lambda nv=5, lab=p, vf=p, t=1, sc=p, c=ref_cnt: lib.scr_mesh_vertices_plan(nv, lab, vf, t, sc, c, None),
         ((dict(c=None), "count_host"), (dict(nv=0), "nv ="), (dict(t=0), "threshold"), (dict(t=-3), "threshold"), (dict(vf=None), "NULL"),
          (dict(sc=None), "NULL"))),
        ("scr_mesh_vertices_run",
         lambda nv=5, lab=p, vf=p, t=1, sc=p, n=2, v=p, c=p, ov=p, oc=p, rm=p: lib.scr_mesh_vertices_run(nv, lab, vf, t, sc, n, v, c, ov, oc, rm, None),
         ((dict(nv=0), "nv ="), (dict(t=0), "threshold"), (dict(n=-1), "nkept"), (dict(n=6), "nkept"), (dict(v=None), "NULL"), (dict(rm=None), "NULL"),
          (dict(c=None), "both or neither"), (dict(oc=None), "both or neither"))),
        ("scr_mesh_faces_plan", lambda nf=5, f=p, lab=p, vf=p, t=1, sc=p, c=ref_cnt: lib.scr_mesh_faces_plan(nf, f, lab, vf, t, sc, c, None),
         ((dict(c=None), "count_host"), (dict(nf=0), "nf ="), (dict(nf=2 ** 30), "3 nf"), (dict(t=0), "threshold"), (dict(f=None), "NULL"),
          (dict(sc=None), "NULL"))),
        ("scr_mesh_faces_run", lambda nf=5, f=p, lab=p, vf=p, t=1, sc=p, n=2, rm=p, o=p: lib.scr_mesh_faces_run(nf, f, lab, vf, t, sc, n, rm, o, None),
         ((dict(nf=0), "nf ="), (dict(t=0), "threshold"), (dict(n=-1), "nkept"), (dict(n=6), "nkept"), (dict(rm=None), "NULL"), (dict(o=None), "NULL"))),
        ("scr_mesh_vertex_normals", lambda nv=5, nf=3, v=p, f=p, k=p, n=p: lib.scr_mesh_vertex_normals(nv, nf, v, f, k, n, None),
         ((dict(nv=-1), "nv ="), (dict(nf=2 ** 30), "3 nf"), (dict(v=None), "NULL"), (dict(n=None), "NULL"), (dict(f=None), "faces or keys"),
          (dict(k=None), "faces or keys"))),
    ]
    for name, fn, bad in cases:
        for kw, text in bad:
            cnt.value = 7
            assert fn(**kw) == 1 and err().startswith(name + ":") and text in err(), (name, kw, err())
            if "plan" in name and "c" not in kw:
                assert cnt.value == 0
    # nothing to do: a no-op whatever the pointers
    assert lib.scr_mesh_roots_run(5, None, None, None, 0, None, None, None) == 0
    assert lib.scr_mesh_vertices_run(5, None, None, 1, None, 0, None, None, None, None, None, None) == 0
    assert lib.scr_mesh_faces_run(5, None, None, None, 1, None, 0, None, None, None) == 0
    assert lib.scr_mesh_vertex_normals(0, 0, None, None, None, None, None) == 0


# ------------------------------------------------------------------ the host side: every ValueError, and no launch
@pytest.fixture
def no_launch(monkeypatch):
    from splatco_amd import _C
    made = []
    monkeypatch.setattr(_C, "family_call", lambda *a, **k: made.append(a[0]))
    yield made
    assert made == [], f"launched {made}"


def test_the_operators_refuse_bad_arguments_before_any_launch(no_launch):
    from splatco_amd.mesh import clean_mesh, connected_components, vertex_normals
    v, f = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int32)
    meta = lambda t: t.to("meta")
    for faces, text in ((f[:, :2], r"\[Nf, 3\]"), (f[0], r"\[Nf, 3\]"), (f.float(), "int32 or int64"), (f.to(torch.int16), "int32 or int64"),
                        (f.numpy(), "not a tensor"), (f, "cpu"), (f.long(), "cpu")):
        with pytest.raises(ValueError, match=text):
            connected_components(faces, 5)
        with pytest.raises(ValueError, match="vertices is on meta" if text == "cpu" else text):     # shapes first, devices next
            vertex_normals(meta(v), faces)
    for nv in (-1, 2 ** 31, 2.0, None, True):
        with pytest.raises(ValueError, match="num_vertices"):
            connected_components(meta(f), nv)
    with pytest.raises(ValueError, match="2\\^31"):
        connected_components(torch.zeros(1, dtype=torch.int32, device="meta").expand(2 ** 31 // 3 + 1, 3), 5)
    for vertices, text in ((v[:, :2], r"\[Nv, 3\]"), (v.double(), "float32"), (v.numpy(), "not a tensor"), (v, "cpu")):
        with pytest.raises(ValueError, match=text):
            vertex_normals(vertices, meta(f))
        with pytest.raises(ValueError, match=text):
            clean_mesh(vertices, meta(f))
    for colors, text in ((v[:4], "4 colors for 5 vertices"), (v.double(), "colors .*float32"), (v[:, :1], "colors")):
        with pytest.raises(ValueError, match=text):
            clean_mesh(meta(v), meta(f), meta(colors))
    for kw, text in ((dict(keep_largest=0), "keep_largest"), (dict(keep_largest=-2), "keep_largest"), (dict(keep_largest=2.0), "keep_largest"),
                     (dict(keep_largest=True), "keep_largest"), (dict(min_faces=-1), "min_faces"), (dict(min_faces=1.5), "min_faces")):
        with pytest.raises(ValueError, match=text):
            clean_mesh(meta(v), meta(f), **kw)
    with pytest.raises(ValueError, match="meta"):
        clean_mesh(meta(v), meta(f), min_faces=0)               # min_faces = 0 is legal: the device check comes next


def test_extract_mesh_has_the_filter_arguments_and_defaults_to_none():
    import inspect
    from splatco_amd.tsdf import extract_mesh
    sig = inspect.signature(extract_mesh)
    assert sig.parameters["keep_largest"].default is None and sig.parameters["min_faces"].default is None
    assert list(sig.parameters)[-2:] == ["keep_largest", "min_faces"]


# ------------------------------------------------------------------ PLY
def _ply_bytes(v, f, colors=None, normals=None):
    """The documented layout, built by hand: the header, then per vertex x y z [nx ny nz] [red green blue], then per face the
    byte 3 and three little-endian int32."""
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
    if normals is not None:
        head += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    out = ("\n".join(head) + "\n").encode("ascii")
    for i in range(len(v)):
        out += struct.pack("<3f", *v[i])
        if normals is not None:
            out += struct.pack("<3f", *normals[i])
        if colors is not None:
            out += struct.pack("<3B", *colors[i])
    for face in f:
        out += struct.pack("<B3i", 3, *face)
    return out


@pytest.mark.parametrize("with_colors", (False, True))
def test_mesh_ply_with_and_without_normals(tmp_path, with_colors):
    from splatco_amd import scene_io
    v, f = ref.fan(9)
    n = ref.normals_ref(v, f)
    c8 = np.random.default_rng(3).integers(0, 256, size=v.shape)
    c = (c8 / 255.0).astype(np.float32) if with_colors else None
    plain, full = str(tmp_path / "plain.ply"), str(tmp_path / "sub" / "normals.ply")
    # without normals=: the bytes of the function as it was
    scene_io.write_ply_mesh(plain, torch.from_numpy(v), torch.from_numpy(f), None if c is None else torch.from_numpy(c))
    assert open(plain, "rb").read() == _ply_bytes(v, f, c8 if with_colors else None)
    out = scene_io.read_ply_mesh(plain)
    assert len(out) == 3 and np.array_equal(out[0], v) and np.array_equal(out[1], f) and ((out[2] is None) if c is None else np.array_equal(out[2], c))
    out = scene_io.read_ply_mesh(plain, normals=True)
    assert len(out) == 4 and out[3] is None and np.array_equal(out[0], v)
    # with normals: nx ny nz as float right after x y z
    scene_io.write_ply_mesh(full, v, f, c, normals=torch.from_numpy(n))
    assert open(full, "rb").read() == _ply_bytes(v, f, c8 if with_colors else None, n)
    v2, f2, c2, n2 = scene_io.read_ply_mesh(full, normals=True)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and n2.dtype == np.float32 and np.array_equal(n2.view(np.int32), n.view(np.int32))
    assert (c2 is None) if c is None else np.array_equal(c2, c)
    out = scene_io.read_ply_mesh(full)                          # the default call skips the extra scalar properties
    assert len(out) == 3 and np.array_equal(out[0], v) and np.array_equal(out[1], f)
    assert len(scene_io.read_ply_vertices(full)) == len(v)
    with pytest.raises(ValueError, match="normals"):
        scene_io.write_ply_mesh(full, v, f, c, normals=n[:3])
    scene_io.write_ply_mesh(full, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None, normals=np.zeros((0, 3), np.float32))
    out = scene_io.read_ply_mesh(full, normals=True)
    assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and out[3].shape == (0, 3)
