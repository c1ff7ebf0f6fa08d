"""Mesh evaluation, everything that needs no device: the numpy restatement (tests/surfeval_ref.py) on constructions known in closed
form and against scipy's k-d tree, the C-ABI surface of include/splatco_surfeval.h against _C.SURFEVAL_SIGNATURES,
_C.family_call, and the argument rejections of the entry points and of splatco_amd.surface_eval."""
import ast
import ctypes
import json
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import surfeval_ref as ref
import splatco_amd.surface_eval                # noqa: F401  (the module under test: without it nothing here can run)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "splatco_surfeval.h")
NAMES = ["scr_surfeval_abi_version", "scr_surfeval_score_scratch_bytes", "scr_surfeval_face_counts", "scr_surfeval_sample",
         "scr_surfeval_nearest", "scr_surfeval_score"]
STREAMED = NAMES[2:]


# ------------------------------------------------------------------ the reference alone
def test_reference_hash_is_the_written_one():
    def mix(x):
        x ^= x >> 16
        x = (x * 0x21f0aaad) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x735a2d97) & 0xFFFFFFFF
        return x ^ (x >> 15)
    for seed, f, c in ((0, 0, 0), (1, 2, 3), (2 ** 32 - 1, 123456, 200001), (77, 2 ** 31 // 3, 1)):
        assert int(ref.u32(seed, f, c)) == mix(mix(mix(seed) ^ f) ^ c)
    u = ref.uniform(5, np.arange(1000), 0)
    assert u.dtype == np.float64 and (u >= 0).all() and (u < 1).all() and np.array_equal(u * 2.0 ** 32, np.floor(u * 2.0 ** 32))


def test_reference_samples_the_unit_square_evenly():
    v, f = ref.unit_square()
    for seed in range(4):
        pts, fi = ref.sample_ref(v, f, 20000.0, seed)
        assert pts.dtype == np.float32 and fi.dtype == np.int32
        assert np.bincount(fi).tolist() == [10000, 10000]                         # A * density is an integer: U adds nothing
        assert (np.diff(fi) >= 0).all()
        n = len(pts)
        quad = np.histogram2d(pts[:, 0], pts[:, 1], bins=2, range=((0, 1), (0, 1)))[0]
        assert (np.abs(quad - n / 4) < 4.0 * math.sqrt(n * 0.25 * 0.75)).all()
        cells = np.histogram2d(pts[:, 0], pts[:, 1], bins=8, range=((0, 1), (0, 1)))[0]
        assert cells.sum() == n and (np.abs(cells - n / 64) < 5.0 * math.sqrt(n / 64)).all()
        assert (pts[:, 2] == 0).all()
    a, b = ref.sample_ref(v, f, 20000.0, 0)[0], ref.sample_ref(v, f, 20000.0, 1)[0]
    assert not np.array_equal(a, b) and np.array_equal(a, ref.sample_ref(v, f, 20000.0, 0)[0])


def test_reference_counts_round_stochastically_and_samples_stay_inside():
    v, f = ref.small_faces(5000, 3)
    area = ref.areas_ref(v, f)
    for density in (2000.0, 3.0, 1e-3):
        counts = ref.face_counts_ref(v, f, density, 9)
        assert (np.abs(counts - area * density) < 1).all()
        assert abs(int(counts.sum()) - density * math.fsum(area.tolist())) < len(f)          # |n_f - A_f density| < 1
    assert ref.face_counts_ref(v, f, 1e-3, 9).sum() < 50
    # degenerate faces get no samples: repeated indices, collinear corners, and an area that is not finite
    dv = np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (np.inf, 0, 0), (0, 3e38, 0), (-3e38, -3e38, 0)], np.float32)
    df = np.array([(0, 0, 1), (1, 1, 1), (0, 1, 2), (4, 5, 6), (0, 1, 3)], np.int32)
    assert ref.face_counts_ref(dv, df, 1e-9, 0)[:3].tolist() == [0, 0, 0]
    c = ref.face_counts_ref(dv, df, 100.0, 0)
    assert c[:4].tolist() == [0, 0, 0, 0] and c[4] == 50
    # every sample inside its triangle: triangles of unit scale, barycentrics recovered in binary64
    v, f = ref.unit_triangles(300, 4)
    pts, fi = ref.sample_ref(v, f, 40.0, 2)
    assert len(pts) > 5000
    w = ref.barycentrics(pts, v, f, fi)
    assert w.min() >= -2.0 ** -22 and np.abs(w.sum(1) - 1).max() < 1e-12


def test_reference_nearest_against_a_kd_tree():
    spatial = pytest.importorskip("scipy.spatial")
    for shape, n in (("cube", 3000), ("sheet", 2000), ("clusters", 1000)):
        t = ref.targets(shape, n, 1)
        q = ref.queries(t, 400, 2)
        d2, idx = ref.nearest_ref(q, t)
        dist, _ = spatial.cKDTree(t.astype(np.float64)).query(q.astype(np.float64))
        want = dist * dist
        # three roundings of the differences enter twice, three of the squares and two of the sums: under 6 * 2^-24; 8 leaves room
        assert (np.abs(d2.astype(np.float64) - want) <= 8 * 2.0 ** -24 * want).all()
        e = t[idx].astype(np.float64) - q.astype(np.float64)
        assert (np.abs((e * e).sum(1) - want) <= 16 * 2.0 ** -24 * want).all()             # the index names such a point
    # the cap, the smallest index among equals, a match exactly at the cap
    t = np.array([(0, 0, 0), (2, 0, 0), (0, 0, 0), (2, 0, 0)], np.float32)
    q = np.array([(0, 0, 0), (1, 0, 0), (5, 4, 0), (2.5, 0, 0)], np.float32)
    d2, idx = ref.nearest_ref(q, t)
    assert d2.tolist() == [0, 1, 25, 0.25] and idx.tolist() == [0, 0, 1, 1]
    d2, idx = ref.nearest_ref(q, t, max_dist=0)
    assert d2.tolist() == [0, 0, 0, 0] and idx.tolist() == [0, -1, -1, -1]
    d2, idx = ref.nearest_ref(q, t, max_dist=1.0)
    assert d2.tolist() == [0, 1, 1, 0.25] and idx.tolist() == [0, 0, -1, 1]
    d2, idx = ref.nearest_ref(q, t, max_dist=0.75)
    assert d2.tolist() == [0, 0.5625, 0.5625, 0.25] and idx.tolist() == [0, -1, -1, 1]


def test_reference_score_of_hand_made_lists():
    a = np.array([0.0, 0.25, 1.0, 4.0], np.float32)                   # d = 0, 0.5, 1, 2
    b = np.array([0.0625, 0.0625, 9.0], np.float32)                   # d = 0.25, 0.25, 3
    res = ref.score_ref(a, b, thresholds=(0.5, 1.0, 0.0, 10.0))
    assert res["accuracy"] == 3.5 / 4 and res["completeness"] == 3.5 / 3 and res["chamfer"] == (3.5 / 4 + 3.5 / 3) / 2
    assert res["count_pred_to_gt"] == [2, 3, 1, 4] and res["count_gt_to_pred"] == [2, 2, 0, 3]
    assert res["max_pred_to_gt"] == 2.0 and res["max_gt_to_pred"] == 3.0 and res["num_pred"] == 4 and res["num_gt"] == 3
    for k, (cp, cg) in enumerate(zip(res["count_pred_to_gt"], res["count_gt_to_pred"])):
        p, r = Fraction(cp, 4), Fraction(cg, 3)
        assert res["precision"][k] == cp / 4 and res["recall"][k] == cg / 3
        want = 2 * p * r / (p + r) if p + r else Fraction(0)
        assert abs(res["fscore"][k] - float(want)) <= 2.0 ** -52
    assert ref.score_ref(a, b, thresholds=(0.1,))["fscore"] == [0.0]                    # P = 1/4, R = 0
    assert ref.score_ref(b, b, thresholds=(0.1,))["fscore"] == [0.0]                    # P + R = 0
    # a threshold is compared as (double)(float)t
    t = 0.1
    d2 = np.array([np.float32(t) * np.float32(t)], np.float32)
    d = math.sqrt(float(d2[0]))
    assert ref.reduce_ref(d2, (t,))[2] == [int(d <= float(np.float32(t)))]


# ------------------------------------------------------------------ the header and the binding
_SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double, "uint32_t": ctypes.c_uint32}


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
        return base == "float" and got is ctypes.POINTER(ctypes.c_float)
    return got is ctypes.c_void_p


def test_binding_matches_the_header():
    from splatco_amd import _C
    hdr, _ = _header()
    m = re.search(r"^\s*#\s*define\s+SCR_SURFEVAL_ABI_VERSION\s+(\d+)\s*$", hdr, flags=re.M)
    assert m and int(m.group(1)) == _C.SURFEVAL_ABI_VERSION == _C.lib.scr_surfeval_abi_version() == 1
    m = re.search(r"^\s*#\s*define\s+SCR_SURFEVAL_MAX_THRESHOLDS\s+(\d+)\s*$", hdr, flags=re.M)
    assert m and int(m.group(1)) == _C.SURFEVAL_MAX_THRESHOLDS == 8
    protos = _prototypes()
    assert [name for _, name, _ in protos] == [s[0] for s in _C.SURFEVAL_SIGNATURES] == NAMES
    for (ret, name, params), (_, restype, *argtypes) in zip(protos, _C.SURFEVAL_SIGNATURES):
        assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes for {len(params)} parameters"
        assert _binds(ret + " r", restype), f"{name}: restype {restype.__name__} does not bind {ret}"
        for i, (p, got) in enumerate(zip(params, argtypes)):
            assert _binds(p, got), f"{name} parameter {i} `{p}`: {got.__name__}"
        f = getattr(_C.lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, f"{name}: not bound from SURFEVAL_SIGNATURES"
    assert [n for n, s in _streamed().items() if s] == STREAMED
    assert [len(p) for _, _, p in protos] == [0, 1, 7, 9, 12, 7]
    assert _C._FAMILY_HEADERS["include/splatco_surfeval.h"] is _C.SURFEVAL_SIGNATURES
    # the definitions and the bound are in the header
    text = open(HEADER).read()
    for phrase in ("0x21f0aaad", "0x735a2d97", "floor(A * density + U(seed, f, 0))", "(p0 + r1 e1) + r2 e2", "smallest j",
                   "(ex ex + ey ey) + ez ez", "once plus one step per shell", "never negative",
                   "without a search", "fixed order"):
        assert phrase in text, phrase


def test_every_declared_symbol_is_exported_and_the_other_headers_know_none_of_them():
    from splatco_amd import _C
    lib = ctypes.CDLL(os.path.join(ROOT, "splatco_amd", "csrc", "libsplatco_raster.so"))
    for name in NAMES:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert not [s for s in _C.SYMBOLS if s.startswith("scr_surfeval")]
    others = _C.BILAGRID_SIGNATURES + _C.NORMALS_SIGNATURES + _C.TSDF_SIGNATURES + _C.MESH_SIGNATURES
    assert not [s for s in others if s[0].startswith("scr_surfeval")]
    for other in ("splatco_raster.h", "splatco_bilagrid.h", "splatco_normals.h", "splatco_tsdf.h", "splatco_mesh.h"):
        assert "scr_surfeval" not in open(os.path.join(ROOT, "include", other)).read()
    assert not [n for n in NAMES if n.startswith(("scr_mesh", "scr_tsdf", "scr_normals", "scr_bilagrid"))]
    assert (_C.ABI_VERSION, _C.BILAGRID_ABI_VERSION, _C.NORMALS_ABI_VERSION, _C.TSDF_ABI_VERSION, _C.MESH_ABI_VERSION) == (37, 1, 1, 1, 1)
    # the size query (no device needed): ten binary64 per workgroup of 4096 items, 256-byte aligned
    q = _C.lib.scr_surfeval_score_scratch_bytes
    for n in (1, 4096, 4097, 100003):
        want = (n + 4095) // 4096 * 80
        assert q(n) == want + (-want) % 256
    assert q(0) == 256 and q(2 ** 31) == 256


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    return ".".join(reversed(parts + [node.id])) if isinstance(node, ast.Name) else ""


def test_the_module_launches_through_family_call_only():
    streamed = _streamed()
    tree = ast.parse(open(os.path.join(ROOT, "splatco_amd", "surface_eval.py")).read())
    called = []
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        name, where = _dotted(node.func), f"surface_eval.py:{node.lineno}"
        if name in ("_C.family_call", "family_call"):
            first = node.args[0] if node.args else None
            assert isinstance(first, ast.Constant) and isinstance(first.value, str), f"{where}: the name is not a string literal"
            assert streamed.get(first.value, False), f"{where}: {first.value} is not a streamed function of splatco_surfeval.h"
            called.append(first.value)
        elif ".lib.scr_" in "." + name:
            assert not streamed.get(name.rsplit(".", 1)[1], True), f"{where}: {name} takes a stream: launch it through _C.family_call"
        else:
            assert name not in ("_C.call", "call"), f"{where}: this family launches through _C.family_call"
            assert not name.endswith("cuda.device"), f"{where}: torch.cuda.device(...) outside _C"
    assert sorted(set(called)) == sorted(STREAMED)
    # knn_grid.py serves the module, not the other way round
    grid = ast.parse(open(os.path.join(ROOT, "splatco_amd", "knn_grid.py")).read())
    for node in ast.walk(grid):
        if isinstance(node, ast.ImportFrom):
            assert "surface_eval" not in [a.name for a in node.names] and "surface_eval" not in (node.module or "")
        elif isinstance(node, ast.Import):
            assert not [a for a in node.names if "surface_eval" in a.name]


class _Recorder:
    def __init__(self, rc=0):
        self.rc, self.args = rc, None

    def __call__(self, *args):
        self.args = args
        return self.rc


def test_family_call_accepts_the_new_names_and_still_refuses_others(monkeypatch):
    from splatco_amd import _C
    other, own = _Recorder(), _Recorder()
    monkeypatch.setattr(_C.lib, "scr_knn_cell_keys", other)
    monkeypatch.setattr(_C.lib, "scr_surfeval_score", own)
    a = torch.zeros(4)
    for name in ("scr_knn_cell_keys", "scr_no_such_entry_point", "scr_surfeval"):
        with pytest.raises(ValueError, match=name):
            _C.family_call(name, a)
    assert other.args is None
    with pytest.raises(ValueError) as e:
        _C.family_call("scr_surfeval_score", 4, a, 0, None, torch.zeros(4, device="meta"), None)
    assert "scr_surfeval_score" in str(e.value) and "argument 4" in str(e.value) and "meta" in str(e.value)
    assert own.args is None
    for name in NAMES:
        assert name in _C._FAMILY_NAMES
    assert "scr_mesh_components" in _C._FAMILY_NAMES and "scr_tsdf_integrate" in _C._FAMILY_NAMES


@pytest.mark.skipif(torch.cuda.is_available(), reason="replays rejected calls only where nothing can be launched")
def test_c_abi_checks_sizes_and_scalars_first():
    """Validated before anything is launched; 16 stands for any non-null device address (never dereferenced on the host)."""
    from splatco_amd import _C
    lib, p = _C.lib, 16
    err = lambda: lib.scr_last_error().decode()
    grid = _C.host_array((0.0, 0.0, 0.0, 1.0, 2, 2, 2, 0.0), _C.f32)
    bad_grid = _C.host_array((0.0, 0.0, 0.0, 0.0, 2, 2, 2, 0.0), _C.f32)
    thr = _C.host_array((0.5, 1.0), _C.f32)
    neg = _C.host_array((0.5, -1.0), _C.f32)
    nan = _C.host_array((math.nan,), _C.f32)
    cases = [
        ("scr_surfeval_face_counts", lambda nf=5, v=p, f=p, d=2.0, c=p: lib.scr_surfeval_face_counts(nf, v, f, d, 0, c, None),
         ((dict(nf=0), "nf ="), (dict(nf=2 ** 30), "3 nf"), (dict(d=0.0), "density"), (dict(d=-1.0), "density"), (dict(d=math.inf), "density"),
          (dict(d=math.nan), "density"), (dict(v=None), "NULL"), (dict(f=None), "NULL"), (dict(c=None), "NULL"))),
        ("scr_surfeval_sample", lambda nf=5, ns=9, v=p, f=p, e=p, o=p, i=p: lib.scr_surfeval_sample(nf, ns, v, f, e, 0, o, i, None),
         ((dict(nf=0), "nf ="), (dict(ns=-1), "ns ="), (dict(ns=2 ** 31), "ns ="), (dict(v=None), "NULL"), (dict(e=None), "NULL"),
          (dict(o=None), "NULL"), (dict(i=None), "NULL"))),
        ("scr_surfeval_nearest",
         lambda nq=5, nt=7, g=grid, q=p, qi=p, t=p, ti=p, cs=p, m=-1.0, d=p, i=p: lib.scr_surfeval_nearest(nq, nt, g, q, qi, t, ti, cs, m, d, i, None),
         ((dict(nq=0), "nq ="), (dict(nq=2 ** 31), "nq ="), (dict(nt=0), "N"), (dict(g=None), "grid_host"), (dict(g=bad_grid), "bad grid"),
          (dict(m=math.nan), "max_dist"), (dict(q=None), "NULL"), (dict(ti=None), "NULL"), (dict(cs=None), "NULL"), (dict(d=None), "NULL"),
          (dict(i=None), "NULL"))),
        ("scr_surfeval_score", lambda n=5, d=p, k=2, t=thr, s=p, o=p: lib.scr_surfeval_score(n, d, k, t, s, o, None),
         ((dict(n=0), "n ="), (dict(n=2 ** 31), "n ="), (dict(k=-1), "num_thresholds"), (dict(k=9), "num_thresholds"), (dict(t=None), "thresholds_host"),
          (dict(t=neg), "threshold 1"), (dict(t=nan, k=1), "threshold 0"), (dict(d=None), "NULL"), (dict(s=None), "NULL"), (dict(o=None), "NULL"))),
    ]
    for name, fn, bad in cases:
        for kw, text in bad:
            assert fn(**kw) == 1 and err().startswith(name + ":") and text in err(), (name, kw, err())
    assert lib.scr_surfeval_sample(5, 0, None, None, None, 0, None, None, None) == 0           # nothing to do: a no-op


# ------------------------------------------------------------------ the host side: every ValueError, and no launch
@pytest.fixture
def no_launch(monkeypatch):
    from splatco_amd import _C
    made = []
    monkeypatch.setattr(_C, "family_call", lambda *a, **k: made.append(a[0]))
    for name in STREAMED:
        monkeypatch.setattr(_C.lib, name, lambda *a, _n=name: made.append(_n))
    yield made
    assert made == [], f"launched {made}"


def test_the_operators_refuse_bad_arguments_before_any_launch(no_launch):
    from splatco_amd.surface_eval import evaluate_mesh, evaluate_points, nearest, sample_surface, score
    v, f, pts = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int32), torch.zeros(6, 3)
    meta = lambda t: t.to("meta")
    # sample_surface: exactly one of spacing and density, a positive finite one; the seed; then the mesh as mesh.py checks it
    for kw, text in ((dict(), "exactly one"), (dict(spacing=0.1, density=5.0), "exactly one"), (dict(spacing=0.0), "spacing"),
                     (dict(spacing=-1.0), "spacing"), (dict(spacing=math.nan), "spacing"), (dict(spacing=1e-200), "too small"),
                     (dict(density=0.0), "density"), (dict(density=math.inf), "density"), (dict(density="3"), "density"),
                     (dict(density=True), "density"), (dict(density=1.0, seed=-1), "seed"), (dict(density=1.0, seed=2 ** 32), "seed"),
                     (dict(density=1.0, seed=1.5), "seed")):
        with pytest.raises(ValueError, match=text):
            sample_surface(meta(v), meta(f), **kw)
    for vertices, faces, text in ((v[:, :2], f, r"\[Nv, 3\]"), (v.double(), f, "float32"), (v.numpy(), f, "not a tensor"), (v, f.float(), "int32 or int64"),
                                  (v, f[:, :2], r"\[Nf, 3\]"), (v, meta(f), "vertices is on cpu"), (meta(v), f, "vertices is on meta"), (meta(v), meta(f), "meta")):
        with pytest.raises(ValueError, match=text):
            sample_surface(vertices, faces, density=10.0)
        with pytest.raises(ValueError, match=text):
            evaluate_mesh(vertices, faces, meta(pts), 0.1)
    # nearest: shapes and sizes first, devices next
    for q, t, text in ((pts[:, :2], pts, r"query .*\[N, 3\]"), (pts, pts.double(), "target .*float32"), (pts.numpy(), pts, "query is not a tensor"),
                       (meta(pts), meta(pts[:0]), "target is empty"), (pts, meta(pts), "query is on cpu"), (meta(pts), pts, "query is on meta"),
                       (meta(pts), meta(pts), "meta")):
        with pytest.raises(ValueError, match=text):
            nearest(q, t)
    for m in (-1.0, math.nan, math.inf, "1", True, 1e20):
        with pytest.raises(ValueError, match="max_dist"):
            nearest(meta(pts), meta(pts), max_dist=m)
    # score: an empty side, the thresholds
    d = torch.zeros(7)
    for a, b, kw, text in ((d[:0], d, {}, "empty side"), (d, d[:0], {}, "empty side"), (d.double(), d, {}, "float32"), (pts, d, {}, r"\[N\]"),
                           (d, d, dict(thresholds=(-0.1,)), "threshold"), (d, d, dict(thresholds=(math.nan,)), "threshold"),
                           (d, d, dict(thresholds=tuple(range(9))), "at most 8"), (d, d, dict(thresholds=(1e39,)), "float32"),
                           (d, meta(d), {}, "cpu"), (meta(d), meta(d), dict(thresholds=(0.5,)), "meta")):
        with pytest.raises(ValueError, match=text):
            score(meta(a) if a.shape[0] == 0 else a, meta(b) if b.shape[0] == 0 else b, **kw)
    # the end-to-end calls
    for kw, text in ((dict(thresholds=(-1,)), "threshold"), (dict(max_dist=-2), "max_dist")):
        with pytest.raises(ValueError, match=text):
            evaluate_points(meta(pts), meta(pts), **kw)
        with pytest.raises(ValueError, match=text):
            evaluate_mesh(meta(v), meta(f), meta(pts), 0.1, **kw)
    with pytest.raises(ValueError, match="pred_points is empty"):
        evaluate_points(meta(pts[:0]), meta(pts))
    with pytest.raises(ValueError, match="gt_points is empty"):
        evaluate_points(meta(pts), meta(pts[:0]))
    with pytest.raises(ValueError, match="gt_points is empty"):
        evaluate_mesh(meta(v), meta(f), meta(pts[:0]), 0.1)
    with pytest.raises(ValueError, match="spacing"):
        evaluate_mesh(meta(v), meta(f), meta(pts), 0.0)
    with pytest.raises(ValueError, match="vertices is on meta"):                # devices in argument order
        evaluate_mesh(meta(v), meta(f), pts, 0.1)


def test_mesh_results_round_trip_and_leave_results_json_alone(tmp_path):
    from splatco_amd.surface_eval import write_mesh_results
    res = ref.score_ref(np.array([0.25, 1.0], np.float32), np.array([4.0], np.float32), thresholds=(0.5, 1.5))
    other = tmp_path / "results.json"
    other.write_text('{"ours": {"PSNR": 30.0}}')
    path = write_mesh_results(str(tmp_path), res, method="mine")
    assert path == str(tmp_path / "mesh_results.json")
    assert json.load(open(path)) == {"mine": res}
    assert json.load(open(other)) == {"ours": {"PSNR": 30.0}}
    assert write_mesh_results(str(tmp_path / "new" / "dir"), res).endswith(os.path.join("new", "dir", "mesh_results.json"))
