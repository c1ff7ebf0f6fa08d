"""TSDF fusion and mesh extraction, everything that needs no device: the C-ABI surface of include/splatco_tsdf.h against
_C.TSDF_SIGNATURES and _C.TsdfView, _C.family_call, the argument rejections of the entry points and of splatco_amd.tsdf, the
numpy restatement (tests/tsdf_ref.py) alone on an analytic sphere, closed and with an unobserved slab, the recipe's
preconditions, and the mesh PLY round trip."""
import ast
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import tsdf_ref as ref
import splatco_amd.tsdf                       # noqa: F401  (the module under test: without it nothing here can run)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "splatco_tsdf.h")
NAMES = ["scr_tsdf_abi_version", "scr_tsdf_integrate", "scr_tsdf_extract_scratch_bytes", "scr_tsdf_extract_vertices_plan",
         "scr_tsdf_extract_vertices_run", "scr_tsdf_extract_faces_plan", "scr_tsdf_extract_faces_run"]
STREAMED = [n for n in NAMES if n not in ("scr_tsdf_abi_version", "scr_tsdf_extract_scratch_bytes")]

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


def _binds(base, depth, got):
    from splatco_amd import _C
    if depth == 0:
        return got is _SCALARS.get(base, object())
    pointee = {"scr_tsdf_view": _C.TsdfView, "int64_t": ctypes.c_int64}.get(base)
    return got is ctypes.c_void_p or (pointee is not None and got is ctypes.POINTER(pointee) and base in ("scr_tsdf_view", "int64_t"))


def test_binding_matches_the_header():
    from splatco_amd import _C
    hdr, _ = _header()
    m = re.search(r"^\s*#\s*define\s+SCR_TSDF_ABI_VERSION\s+(\d+)\s*$", hdr, flags=re.M)
    assert m and int(m.group(1)) == _C.TSDF_ABI_VERSION == _C.lib.scr_tsdf_abi_version() == 1
    m = re.search(r"^\s*#\s*define\s+SCR_TSDF_MAX_VIEWS\s+(\d+)\s*$", hdr, flags=re.M)
    assert m and int(m.group(1)) == _C.TSDF_MAX_VIEWS == splatco_amd.tsdf.BATCH == 16
    protos = _prototypes()
    assert [name for _, name, _ in protos] == [s[0] for s in _C.TSDF_SIGNATURES] == NAMES
    for (ret, name, params), (_, restype, *argtypes) in zip(protos, _C.TSDF_SIGNATURES):
        assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes for {len(params)} parameters"
        assert _binds(*_c_type(ret), restype), f"{name}: restype {restype.__name__} does not bind {ret}"
        for i, (p, got) in enumerate(zip(params, argtypes)):
            assert _binds(*_c_type(p), got), f"{name} parameter {i} `{p}`: {got.__name__}"
        f = getattr(_C.lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, f"{name}: not bound from TSDF_SIGNATURES"
    assert [n for n, s in _streamed().items() if s] == STREAMED
    assert [len(p) for _, _, p in protos] == [0, 13, 3, 9, 15, 9, 12]


def test_view_struct_matches_the_header():
    from splatco_amd import _C
    body = re.search(r"typedef\s+struct\s+scr_tsdf_view\s*\{(.*?)\}\s*scr_tsdf_view\s*;", _header()[1], flags=re.S).group(1)
    fields = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        base, depth = _c_type(decl)
        for nm in decl.replace("*", " ").split(base, 1)[1].split(","):
            nm = nm.strip()
            arr = re.fullmatch(r"(\w+)\[(\d+)\]", nm)
            ctype = ctypes.c_void_p if depth else _SCALARS[base]
            fields.append((arr.group(1), ctype * int(arr.group(2))) if arr else (nm, ctype))
    assert [(n, t) for n, t in _C.TsdfView._fields_] == fields
    assert ctypes.sizeof(_C.TsdfView) == 184 and _C.TsdfView.near.offset == 176 and _C.TsdfView.fx.offset == 48
    # 16 views and the volume's own arguments fit the 4 KiB kernel-argument segment (csrc/tsdf.hip asserts the same)
    assert 16 * ctypes.sizeof(_C.TsdfView) + 8 + 72 + 24 <= 4096


def test_every_declared_symbol_is_exported_and_the_other_headers_know_none_of_them():
    from splatco_amd import _C
    lib = ctypes.CDLL(os.path.join(ROOT, "splatco_amd", "csrc", "libsplatco_raster.so"))
    for name in NAMES:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert not [s for s in _C.SYMBOLS if s.startswith("scr_tsdf")]
    assert not [s for s in _C.BILAGRID_SIGNATURES + _C.NORMALS_SIGNATURES if s[0].startswith("scr_tsdf")]
    for other in ("splatco_raster.h", "splatco_bilagrid.h", "splatco_normals.h"):
        assert "scr_tsdf" not in open(os.path.join(ROOT, "include", other)).read()
    assert _C.ABI_VERSION == 37 and _C.BILAGRID_ABI_VERSION == 1 and _C.NORMALS_ABI_VERSION == 1
    # the size query (no device needed): one uint32 per workgroup of 1024 items of the larger compaction, + 1, 256-byte
    # aligned, + 256 for the total
    q = _C.lib.scr_tsdf_extract_scratch_bytes
    items = max(7 * 20 * 13 * 9, 12 * 19 * 12 * 8)
    want = ((items + 1023) // 1024 + 1) * 4
    assert q(20, 13, 9) == want + (-want) % 256 + 256
    assert q(1, 5, 5) == 256 and q(-1, 2, 2) == 256 and q(1024, 1024, 1024) == 256


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    return ".".join(reversed(parts + [node.id])) if isinstance(node, ast.Name) else ""


def test_the_module_launches_through_family_call_only():
    streamed = _streamed()
    tree = ast.parse(open(os.path.join(ROOT, "splatco_amd", "tsdf.py")).read())
    called = []
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        name, where = _dotted(node.func), f"tsdf.py:{node.lineno}"
        if name in ("_C.family_call", "family_call"):
            first = node.args[0] if node.args else None
            assert isinstance(first, ast.Constant) and isinstance(first.value, str), f"{where}: the name is not a string literal"
            assert streamed.get(first.value, False), f"{where}: {first.value} is not a streamed function of splatco_tsdf.h"
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
    monkeypatch.setattr(_C.lib, "scr_tsdf_integrate", own)
    a = torch.zeros(4)
    for name in ("scr_depth_loss_forward", "scr_no_such_entry_point", "scr_copy_probe", "scr_tsdf"):
        with pytest.raises(ValueError, match=name):
            _C.family_call(name, a)
    assert other.args is None
    with pytest.raises(ValueError) as e:
        _C.family_call("scr_tsdf_integrate", 2, 2, 2, None, 0.1, 0.4, 255.0, a, torch.zeros(4, device="meta"), None, 1, None)
    assert "scr_tsdf_integrate" in str(e.value) and "argument 8" in str(e.value) and "meta" in str(e.value)
    with pytest.raises(ValueError, match="device"):
        _C.family_call("scr_tsdf_integrate", 2, 2, 2, None, 0.1, 0.4, 255.0, None, None, None, 1, None)
    assert own.args is None
    for name in NAMES:
        assert name in _C._FAMILY_NAMES
    assert "scr_bilagrid_slice" in _C._FAMILY_NAMES and "scr_normals_map" in _C._FAMILY_NAMES


@pytest.mark.skipif(torch.cuda.is_available(), reason="replays rejected calls only where nothing can be launched")
def test_c_abi_checks_sizes_and_scalars_first():
    """Validated before anything is launched; 16 stands for any non-null device address (never dereferenced on the host)."""
    from splatco_amd import _C
    lib, p = _C.lib, 16
    err = lambda: lib.scr_last_error().decode()
    nan, inf = float("nan"), float("inf")
    lo = _C.host_array((0.0, 0.0, 0.0), _C.f32)

    def view(**kw):
        f = dict(depth=p, alpha=p, image=None, mask=None, H=4, W=5, mask_kind=0, min_alpha=0.5, fx=3.0, fy=3.0, cx=2.0, cy=2.0,
                 w2c=(ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0), near=0.05)
        f.update(kw)
        return _C.TsdfView(*[f[n] for n, _ in _C.TsdfView._fields_])

    def integ(dims=(4, 3, 2), lo=lo, h=0.1, trunc=0.4, mw=255.0, tsdf=p, weight=p, color=p, n=1, views=None, **kw):
        arr = (_C.TsdfView * 16)(*([view(**kw)] * 16)) if views is None else views
        return lib.scr_tsdf_integrate(*dims, lo, h, trunc, mw, tsdf, weight, color, n, arr, None)

    name = "scr_tsdf_integrate"
    bad_w2c = (ctypes.c_double * 12)(1, 0, 0, 0, 0, nan, 0, 0, 0, 0, 1, 0)
    for kw, text in ((dict(dims=(1, 3, 3)), ">= 2"), (dict(dims=(3, 3, 0)), ">= 2"), (dict(dims=(2048, 2048, 512)), "2^31"),
                     (dict(dims=(65536, 65536, 2)), "2^31"), (dict(h=0.0), "h ="), (dict(h=nan), "h ="), (dict(h=inf), "h ="),
                     (dict(trunc=0.0), "trunc"), (dict(trunc=-1.0), "trunc"), (dict(trunc=nan), "trunc"), (dict(mw=0.0), "max_weight"),
                     (dict(mw=inf), "max_weight"), (dict(lo=None), "lo_host"), (dict(lo=_C.host_array((0.0, nan, 0.0), _C.f32)), "lo is not finite"),
                     (dict(n=0), "nviews"), (dict(n=17), "nviews"), (dict(views=ctypes.POINTER(_C.TsdfView)()), "views_host"),
                     (dict(H=0), "H = 0"), (dict(W=-2), "W = -2"), (dict(H=65536, W=32768), "2^31"), (dict(fx=0.0), "fx"),
                     (dict(fy=nan), "fy"), (dict(cx=inf), "cx"), (dict(cy=nan), "cy"), (dict(w2c=bad_w2c), "w2c"),
                     (dict(near=-0.1), "near"), (dict(near=nan), "near"), (dict(min_alpha=-0.5), "min_alpha"),
                     (dict(min_alpha=inf), "min_alpha"), (dict(mask_kind=3), "mask_kind"), (dict(mask_kind=-1), "mask_kind")):
        assert integ(**kw) == 1 and err().startswith(name + ":") and text in err(), (kw, err())
    # sizes and scalars before the pointers
    assert integ(dims=(1, 3, 3), tsdf=None) == 1 and ">= 2" in err()
    assert integ(fx=0.0, depth=None) == 1 and "fx" in err()
    for kw, text in ((dict(tsdf=None), "NULL volume"), (dict(weight=None), "NULL volume"), (dict(depth=None), "NULL map"),
                     (dict(alpha=None), "NULL map"), (dict(mask_kind=1), "mask is NULL"), (dict(mask_kind=2), "mask is NULL"),
                     (dict(image=p, color=None), "no colour")):
        assert integ(**kw) == 1 and err().startswith(name + ":") and text in err(), (kw, err())

    cnt = ctypes.c_int64(7)
    plans = ((lib.scr_tsdf_extract_vertices_plan, "scr_tsdf_extract_vertices_plan"), (lib.scr_tsdf_extract_faces_plan, "scr_tsdf_extract_faces_plan"))
    for fn, name in plans:
        def plan(dims=(4, 3, 2), tsdf=p, weight=p, mw=0.0, scratch=p, count=ctypes.byref(cnt)):
            return fn(*dims, tsdf, weight, mw, scratch, count, None)
        for kw, text in ((dict(count=None), "count_host"), (dict(dims=(4, 1, 2)), ">= 2"), (dict(dims=(1024, 1024, 512)), "7 nx ny nz"),
                         (dict(dims=(2048, 2048, 512)), "2^31"), (dict(mw=nan), "min_weight"), (dict(tsdf=None), "NULL"),
                         (dict(weight=None), "NULL"), (dict(scratch=None), "NULL")):
            cnt.value = 7
            assert plan(**kw) == 1 and err().startswith(name + ":") and text in err(), (name, kw, err())
            assert kw.get("count", 0) is None or cnt.value == 0

    def vrun(dims=(4, 3, 2), lo=lo, h=0.1, tsdf=p, weight=p, color=p, mw=0.0, scratch=p, nv=5, ids=p, verts=p, cols=p):
        return lib.scr_tsdf_extract_vertices_run(*dims, lo, h, tsdf, weight, color, mw, scratch, nv, ids, verts, cols, None)

    def frun(dims=(4, 3, 2), tsdf=p, weight=p, mw=0.0, scratch=p, nv=5, ids=p, nf=3, faces=p):
        return lib.scr_tsdf_extract_faces_run(*dims, tsdf, weight, mw, scratch, nv, ids, nf, faces, None)

    name = "scr_tsdf_extract_vertices_run"
    for kw, text in ((dict(dims=(4, 3, 1)), ">= 2"), (dict(dims=(1024, 1024, 512)), "7 nx ny nz"), (dict(h=0.0), "h ="), (dict(lo=None), "lo_host"),
                     (dict(mw=nan), "min_weight"), (dict(nv=-1), "nv"), (dict(nv=2 ** 31), "nv"), (dict(tsdf=None), "NULL"),
                     (dict(ids=None), "NULL"), (dict(verts=None), "NULL"), (dict(color=None), "both or neither"), (dict(cols=None), "both or neither")):
        assert vrun(**kw) == 1 and err().startswith(name + ":") and text in err(), (kw, err())
    assert vrun(nv=0, tsdf=None, ids=None) == 0               # nothing kept: a no-op whatever the pointers
    name = "scr_tsdf_extract_faces_run"
    for kw, text in ((dict(dims=(0, 3, 3)), ">= 2"), (dict(mw=nan), "min_weight"), (dict(nv=-1), "nv"), (dict(nf=-1), "nf"), (dict(nf=2 ** 31), "nf"),
                     (dict(nv=0), "no vertices"), (dict(tsdf=None), "NULL"), (dict(ids=None), "NULL"), (dict(faces=None), "NULL")):
        assert frun(**kw) == 1 and err().startswith(name + ":") and text in err(), (kw, err())
    assert frun(nf=0, faces=None) == 0


# ------------------------------------------------------------------ the host side: every ValueError, and no launch
@pytest.fixture
def no_launch(monkeypatch):
    from splatco_amd import _C
    made = []
    monkeypatch.setattr(_C, "family_call", lambda *a, **k: made.append(a[0]))
    yield made
    assert made == [], f"launched {made}"


def _meta_volume(dims=(6, 5, 4), color=True):
    """A volume whose tensors live on the meta device: enough for every check that comes before a launch."""
    from splatco_amd.tsdf import TSDFVolume
    nx, ny, nz = dims
    vol = TSDFVolume.__new__(TSDFVolume)
    vol._geometry("test", (0.0, 0.0, 0.0), 0.1, dims, None, 255.0)
    vol.tsdf, vol.weight = torch.empty(nz, ny, nx, device="meta"), torch.empty(nz, ny, nx, device="meta")
    vol.color = torch.empty(3, nz, ny, nx, device="meta") if color else None
    return vol


def test_the_volume_refuses_bad_geometry_and_cpu_tensors(no_launch):
    from splatco_amd.tsdf import TSDFVolume
    lo = (0.0, 0.0, 0.0)
    for h in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            TSDFVolume(lo, h, (4, 4, 4))
        with pytest.raises(ValueError, match="voxel_size"):
            TSDFVolume.from_bounds(lo, (1.0, 1.0, 1.0), h)
    for trunc in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="trunc"):
            TSDFVolume(lo, 0.1, (4, 4, 4), trunc=trunc)
    for dims in ((1, 4, 4), (4, 4, 0), (4, 4), (2, 2, 2, 2)):
        with pytest.raises(ValueError, match="dims"):
            TSDFVolume(lo, 0.1, dims)
    with pytest.raises(ValueError, match="2\\^31"):
        TSDFVolume(lo, 0.1, (2048, 2048, 512))
    with pytest.raises(ValueError, match="2\\^31"):
        TSDFVolume.from_bounds(lo, (204.7, 204.7, 51.1), 0.1)
    with pytest.raises(ValueError, match="lo"):
        TSDFVolume((0.0, float("nan"), 0.0), 0.1, (4, 4, 4))
    with pytest.raises(ValueError, match="bounds"):
        TSDFVolume.from_bounds((0.0, 0.0, 0.0), (1.0, -1.0, 1.0), 0.1)
    with pytest.raises(ValueError, match="max_weight"):
        TSDFVolume(lo, 0.1, (4, 4, 4), max_weight=0.0)
    with pytest.raises(ValueError, match="cpu"):
        TSDFVolume(lo, 0.1, (4, 4, 4), device="cpu")
    t, w, c = torch.ones(4, 5, 6), torch.zeros(4, 5, 6), torch.zeros(3, 4, 5, 6)
    with pytest.raises(ValueError, match="cpu"):
        TSDFVolume.from_tensors(lo, 0.1, t, w, c)
    with pytest.raises(ValueError, match=r"\[nz, ny, nx\]"):
        TSDFVolume.from_tensors(lo, 0.1, t[0], w[0])
    with pytest.raises(ValueError, match="weight"):
        TSDFVolume.from_tensors(lo, 0.1, t, w[:3])
    with pytest.raises(ValueError, match="color"):
        TSDFVolume.from_tensors(lo, 0.1, t, w, c[:2])
    with pytest.raises(ValueError, match="float32"):
        TSDFVolume.from_tensors(lo, 0.1, t.double(), w)
    with pytest.raises(ValueError, match="tsdf is not contiguous"):
        TSDFVolume.from_tensors(lo, 0.1, torch.ones(6, 5, 4).permute(2, 1, 0), w)
    with pytest.raises(ValueError, match="color is not contiguous"):
        TSDFVolume.from_tensors(lo, 0.1, t, w, torch.zeros(3, 4, 5, 12)[..., ::2])
    with pytest.raises(ValueError, match="dims"):
        TSDFVolume.from_tensors(lo, 0.1, torch.ones(4, 5, 1), torch.zeros(4, 5, 1))
    # from_bounds: dims = ceil((hi - lo) / h) + 1, at least 2
    seen = {}

    class Probe(TSDFVolume):
        def __init__(self, lo, h, dims, **kw):
            seen["dims"] = list(dims)

    Probe.from_bounds((0.0, -1.0, 2.0), (1.0, 0.25, 2.0), 0.25)
    assert seen["dims"] == [5, 6, 2]


def test_integrate_and_extract_refuse_bad_arguments_before_any_launch(no_launch):
    vol = _meta_volume()
    H, W = 5, 7
    D, A = torch.ones(H, W), torch.ones(H, W)
    cam = ((4.0, 4.0, 3.5, 2.5), torch.eye(4))
    cases = [
        (dict(depth=D[None]), r"\[H, W\]"), (dict(depth=torch.ones(0, 3), alpha=torch.ones(0, 3)), r"\[H, W\]"),
        (dict(depth=torch.ones(1).expand(2, 2 ** 30), alpha=torch.ones(1).expand(2, 2 ** 30)), "2\\^31"),
        (dict(alpha=A[:4]), "alpha"), (dict(image=torch.ones(H, W)), "image"), (dict(image=torch.ones(4, H, W)), "image"),
        (dict(mask=torch.ones(H, W + 1)), "mask"), (dict(min_alpha=-0.1), "min_alpha"), (dict(min_alpha=float("nan")), "min_alpha"),
        (dict(near=-1.0), "near"), (dict(near=float("inf")), "near"), (dict(cam=((0.0, 4.0, 3.5, 2.5), torch.eye(4))), "fx"),
        (dict(cam=((4.0, 4.0, 3.5), torch.eye(4))), "4|fx, fy, cx, cy"), (dict(cam=(cam[0], torch.eye(3))), r"\(4, 4\)"),
        (dict(cam=(cam[0], torch.full((4, 4), float("nan")))), "not finite"), (dict(cam=(cam[0],)), "cam must be"),
        (dict(depth=np.ones((H, W))), "not a tensor"),
        (dict(), "cpu"),                                                       # everything right but the device
    ]
    for kw, text in cases:
        args = dict(depth=D, alpha=A, cam=cam, image=None, mask=None, min_alpha=0.5, near=0.05)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            vol.integrate(args.pop("depth"), args.pop("alpha"), args.pop("cam"), **args)
    with pytest.raises(ValueError, match="color=False"):
        _meta_volume(color=False).integrate(D, A, cam, image=torch.ones(3, H, W))
    with pytest.raises(ValueError, match="alphas"):
        vol.integrate_views([D, D], [A], [cam, cam])
    with pytest.raises(ValueError, match="masks"):
        vol.integrate_views([D, D], [A, A], [cam, cam], masks=[None])
    with pytest.raises(ValueError, match="batch"):
        vol.integrate_views([D], [A], [cam], batch=17)
    # the volume itself: a tensor swapped for a non-contiguous or a CPU one
    for swap, text in ((torch.empty(4, 5, 12, device="meta")[..., ::2], "weight is not contiguous"),
                       (torch.empty(4, 5, 7, device="meta"), "weight is not a float32 tensor of shape")):
        bad = _meta_volume()
        bad.weight = swap
        with pytest.raises(ValueError, match=text):
            bad.extract()
    bad = _meta_volume()
    bad.tsdf, bad.weight, bad.color = torch.ones(4, 5, 6), torch.zeros(4, 5, 6), torch.zeros(3, 4, 5, 6)
    with pytest.raises(ValueError, match="cpu"):
        bad.extract()
    with pytest.raises(ValueError, match="min_weight"):
        vol.extract(min_weight=float("nan"))
    with pytest.raises(ValueError, match="meta"):
        vol.extract()
    with pytest.raises(ValueError, match="7 nx ny nz"):
        _meta_volume((1024, 1024, 512)).extract()


def test_a_camera_gives_its_intrinsics_its_rows_and_its_znear():
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.normals import intrinsics
    from splatco_amd.tsdf import _camera
    cam = look_at_camera(eye=(0.3, -0.2, -3.0), target=(0.1, 0.0, 0.2), up=(0, -1, 0), FoVx=math.radians(55), width=70, height=52)
    intr, rows, znear = _camera("t", cam)
    assert intr == intrinsics(cam) and znear == cam.znear
    w2c = cam.world_view_transform.t().double()
    assert rows == w2c[:3].reshape(-1).tolist() and torch.equal(w2c[3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64))
    centre = torch.cat((cam.camera_center.double().cpu(), torch.ones(1, dtype=torch.float64)))
    assert float((w2c @ centre)[:3].abs().max()) < 1e-5                      # the camera centre maps to the origin
    intr2, rows2, znear2 = _camera("t", (intr, w2c))
    assert intr2 == intr and rows2 == rows and znear2 is None


# ------------------------------------------------------------------ the reference alone
R_CELLS = 8.0


def _lattice_tolerance(h):
    return 1e-6 * float(h)               # float32 vertices of a |p| < 1 volume: rounding is 6e-8, six orders below a cell


def test_reference_on_an_analytic_sphere_is_a_closed_oriented_manifold_of_the_right_volume():
    vol, lo, h, centre, r = ref.sphere_volume((24, 24, 24), radius_cells=R_CELLS)
    m = ref.extract_ref(vol, lo, h)
    rep = ref.assert_closed_manifold(m["vertices"], m["faces"])          # every directed edge has exactly one opposite
    assert rep["V"] - rep["E"] + rep["F"] == 2 and rep["duplicates"] == 0 and rep["unreferenced"] == 0
    assert 2 * rep["E"] == 3 * rep["F"]
    assert ref.on_lattice_edges(m["vertices64"], m["edge_ids"], lo, h, (24, 24, 24), 1e-12) < 1e-12 * float(h)
    assert ref.on_lattice_edges(m["vertices"], m["edge_ids"], lo, h, (24, 24, 24), 1e-5) < _lattice_tolerance(h)
    assert np.all(np.diff(m["edge_ids"]) > 0)
    want = 4.0 / 3.0 * math.pi * r ** 3
    print(f"sphere r = {R_CELLS} h: V {rep['V']} E {rep['E']} F {rep['F']}, volume {rep['volume']:.6f} / {want:.6f} = {rep['volume'] / want:.4f}")
    assert rep["volume"] > 0 and abs(rep["volume"] / want - 1.0) < 0.02
    # on the surface: |v - c| = r up to the interpolation error of a distance field along an edge (h^2 / (8 r) per cell)
    d = np.linalg.norm(m["vertices64"] - centre, axis=1)
    assert np.abs(d - r).max() < 0.05 * float(h)
    # every normal points away from the centre (consistent orientation, counter-clockwise from outside)
    v, f = m["vertices64"], m["faces"]
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    out = v[f].mean(1) - centre
    assert (np.einsum("ij,ij->i", n, out) > 0).all()
    # the colour is linear in p, so interpolating it with the vertex's t reproduces it at the vertex
    want_c = (m["vertices64"] - lo.astype(np.float64)) / (float(h) * 24)
    assert np.abs(m["colors64"] - want_c).max() < 1e-6


def test_reference_with_an_unobserved_slab_is_open_exactly_along_the_slab():
    dims = (24, 24, 24)
    vol, lo, h, centre, r = ref.sphere_volume(dims, radius_cells=R_CELLS, slab=slice(9, 11))
    m = ref.extract_ref(vol, lo, h)
    rep = ref.mesh_report(m["vertices"], m["faces"])
    assert rep["F"] > 0 and rep["nonmanifold"] == 0 and rep["duplicates"] == 0 and rep["unreferenced"] == 0 and rep["degenerate"] == 0
    assert len(rep["boundary"]) > 0
    # the cubes that touch a weight-0 node are i = 8, 9, 10; the mesh stops at the node planes i = 8 and i = 11, and every
    # boundary edge lies in one of them, i.e. on a cube next to an invalid one
    x = (m["vertices64"][:, 0] - float(lo[0])) / float(h)
    assert not ((x > 8 + 1e-9) & (x < 11 - 1e-9)).any()
    bx = x[rep["boundary"]]
    assert ((np.abs(bx - 8) < 1e-9).all(1) | (np.abs(bx - 11) < 1e-9).all(1)).all()
    full = ref.extract_ref(ref.sphere_volume(dims, radius_cells=R_CELLS)[0], lo, h)
    assert 0 < rep["F"] < len(full["faces"])
    # min_weight: with a bar at or above every weight nothing is valid
    none = ref.extract_ref(vol, lo, h, min_weight=1.0)
    assert none["vertices"].shape == (0, 3) and none["faces"].shape == (0, 3)


def test_reference_winding_table_is_the_kernels_parity_rule():
    """csrc/tsdf.hip swaps the last two vertices of a triangle when bit `mask` of 0x4D24 differs from the parity of pi."""
    odd = [0, 1, 1, 0, 0, 1]
    for q in range(6):
        for mask in range(1, 15):
            assert bool(ref.TRI_FLIP[q, mask]) == bool(((0x4D24 >> mask) & 1) ^ odd[q]), (q, mask)


@pytest.mark.parametrize("dims,shift", [((20, 13, 9), 0.6), ((2, 5, 7), 0.6), ((64, 4, 3), 0.4)])
def test_recipe_meets_the_preconditions_of_the_gpu_tests(dims, shift):
    lo, h = ref.volume_geometry(dims)
    views = ref.parity_views(dims, corner_shift=shift)
    trunc = 4.0 * float(h)
    vol, parts = ref.fresh(dims), []
    for view in views:
        o = ref.integrate_ref(vol, lo, h, view["depth"], view["alpha"], view["intr"], view["w2c"], trunc, image=view["image"],
                              mask=view["mask"], details=True)
        parts.append(o.pop("details"))
        vol = o
    _, fragile = ref.integrate_views_ref(ref.fresh(dims), lo, h, views, trunc)
    n = fragile.size
    seen = [float(d["ok"].mean()) for d in parts]
    print(f"recipe {dims}: nodes updated per view {[round(float(d['upd'].mean()), 3) for d in parts]}, fragile {int(fragile.sum())} of {n}")
    assert fragile.sum() <= 0.01 * n
    assert parts[0]["front"].all() and parts[0]["upd"].mean() > 0.5                   # the first view sees the whole volume
    assert 0 < (~parts[1]["front"]).mean() < 1                                        # part of the volume behind `near`
    with np.errstate(all="ignore"):
        inimg = parts[2]["front"] & (np.floor(parts[2]["u"]) >= 0) & (np.floor(parts[2]["u"]) < 29) & (np.floor(parts[2]["v"]) >= 0) & \
            (np.floor(parts[2]["v"]) < 37)
    assert 0 < inimg.mean() < (0.8 if dims[0] == 2 else 0.2), inimg.mean()            # only a corner (nx = 2: a slab, most of it)
    assert all(s > 0 for s in seen)
    if dims == (20, 13, 9):
        for view in views:      # every kind of hole is in the maps
            D, A = view["depth"], view["alpha"]
            assert np.isnan(D).any() and np.isinf(D).any() and np.isnan(A).any() and np.isinf(A).any()
            assert (D == 0).any() and (D < 0).any() and ((A > 0) & (A < 0.5)).any() and not np.isfinite(view["image"]).all()
            assert view["mask"] is not None and (np.asarray(view["mask"]) == 0).any()
        assert (vol["weight"] == 0).any() and (vol["weight"] == 2).any() and (vol["tsdf"] < 0).any()
        m = ref.extract_ref(vol, lo, h)
        assert len(m["vertices"]) > 100 and len(m["faces"]) > 100 and 7 * 20 * 13 * 9 == 16380
        rep = ref.mesh_report(m["vertices"], m["faces"])
        assert rep["nonmanifold"] == 0 and rep["unreferenced"] == 0 and rep["duplicates"] == 0


def test_ulp_distance_and_canonical_faces():
    a = np.array([1.0, -1.0, 0.0, -0.0, 1e-45], np.float32)
    assert ref.ulp_distance(a, a).tolist() == [0] * 5
    assert ref.ulp_distance(np.float32([1.0, 0.0, -0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), -0.0, 1e-45])).tolist() == [1, 0, 1]
    f = np.array([[5, 2, 9], [3, 4, 1], [2, 9, 5]])
    assert ref.canonical_faces(f).tolist() == [[1, 3, 4], [2, 9, 5], [2, 9, 5]]
    assert ref.canonical_faces(np.array([[2, 5, 9]])).tolist() != ref.canonical_faces(np.array([[2, 9, 5]])).tolist()


# ------------------------------------------------------------------ PLY
@pytest.mark.parametrize("with_colors", (False, True))
def test_mesh_ply_round_trip(tmp_path, with_colors):
    from splatco_amd import scene_io
    vol, lo, h, _, _ = ref.sphere_volume((8, 8, 8), radius_cells=2.5)
    m = ref.extract_ref(vol, lo, h)
    v, f = m["vertices"], m["faces"]
    c = (np.random.default_rng(3).integers(0, 256, size=v.shape) / 255.0).astype(np.float32) if with_colors else None
    path = str(tmp_path / "sub" / "mesh.ply")
    scene_io.write_ply_mesh(path, torch.from_numpy(v), torch.from_numpy(f), None if c is None else torch.from_numpy(c))
    v2, f2, c2 = scene_io.read_ply_mesh(path)
    assert v2.dtype == np.float32 and f2.dtype == np.int32 and np.array_equal(v2, v) and np.array_equal(f2, f)
    assert (c2 is None) if c is None else (c2.dtype == np.float32 and np.array_equal(c2, c))
    head = open(path, "rb").read(400).split(b"end_header\n")[0].decode("ascii").split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    assert f"element face {len(f)}" in head and "property list uchar int vertex_indices" in head
    assert ("property uchar red" in head) == with_colors
    size = len("\n".join(head)) + len("end_header\n") + len(v) * (12 + 3 * with_colors) + len(f) * 13
    assert os.path.getsize(path) == size
    # an empty mesh, and numpy input
    scene_io.write_ply_mesh(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32) if with_colors else None)
    v3, f3, c3 = scene_io.read_ply_mesh(path)
    assert v3.shape == (0, 3) and f3.shape == (0, 3) and ((c3 is None) or c3.shape == (0, 3))
    # the vertex reader of the anchor files reads the same file's vertex element
    assert len(scene_io.read_ply_vertices(path)) == 0
    with pytest.raises(ValueError, match="colours"):
        scene_io.write_ply_mesh(path, v, f, np.zeros((3, 3)))
