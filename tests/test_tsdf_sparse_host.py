"""The block-sparse TSDF volume, everything that needs no device: the C-ABI surface of include/splatco_tsdf_sparse.h against
_C.TSDFS_SIGNATURES and _C.TsdfsView, the argument rejections of the entry points and of splatco_amd.tsdf_sparse, and the numpy
allocation rule (tests/tsdf_sparse_ref.py) against the band of the dense update."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tsdf_ref as ref
import tsdf_sparse_ref as sref
import splatco_amd.tsdf_sparse                # noqa: F401  (the module under test: without it nothing here can run)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "splatco_tsdf_sparse.h")
NAMES = ["scr_tsdfs_abi_version", "scr_tsdfs_alloc_scratch_bytes", "scr_tsdfs_alloc_plan", "scr_tsdfs_alloc_run", "scr_tsdfs_init_blocks",
         "scr_tsdfs_integrate", "scr_tsdfs_neighbors", "scr_tsdfs_extract_scratch_bytes", "scr_tsdfs_extract_vertices_plan",
         "scr_tsdfs_extract_vertices_run", "scr_tsdfs_extract_faces_plan", "scr_tsdfs_extract_faces_run"]
UNSTREAMED = ("scr_tsdfs_abi_version", "scr_tsdfs_alloc_scratch_bytes", "scr_tsdfs_extract_scratch_bytes")
SHAPES = [(40, 27, 19), (17, 9, 10), (9, 8, 17)]

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


def _c_type(decl):
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    return next(w for w in words if w != "*"), words.count("*")


def _binds(base, depth, got):
    from splatco_amd import _C
    if depth == 0:
        return got is _SCALARS.get(base, object())
    pointee = {"scr_tsdfs_view": _C.TsdfsView, "int64_t": ctypes.c_int64}.get(base)
    return got is ctypes.c_void_p or (pointee is not None and got is ctypes.POINTER(pointee))


# ------------------------------------------------------------------ the header and the binding
def test_binding_matches_the_header():
    from splatco_amd import _C
    hdr, _ = _header()
    m = re.search(r"^\s*#\s*define\s+SCR_TSDFS_ABI_VERSION\s+(\d+)\s*$", hdr, flags=re.M)
    assert m and int(m.group(1)) == _C.TSDFS_ABI_VERSION == _C.lib.scr_tsdfs_abi_version() == 1
    m = re.search(r"^\s*#\s*define\s+SCR_TSDFS_BLOCK\s+(\d+)\s*$", hdr, flags=re.M)
    assert m and int(m.group(1)) == _C.TSDFS_BLOCK == splatco_amd.tsdf_sparse.B == sref.B == 8
    protos = _prototypes()
    assert [name for _, name, _ in protos] == [s[0] for s in _C.TSDFS_SIGNATURES] == NAMES
    for (ret, name, params), (_, restype, *argtypes) in zip(protos, _C.TSDFS_SIGNATURES):
        assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes for {len(params)} parameters"
        assert _binds(*_c_type(ret), restype), f"{name}: restype {restype.__name__} does not bind {ret}"
        for i, (p, got) in enumerate(zip(params, argtypes)):
            assert _binds(*_c_type(p), got), f"{name} parameter {i} `{p}`: {got.__name__}"
        f = getattr(_C.lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, f"{name}: not bound from TSDFS_SIGNATURES"
        assert (bool(params) and "".join(params[-1].split()) == "void*stream") == (name not in UNSTREAMED), name
        assert name in _C._FAMILY_NAMES
    assert _C._FAMILY_HEADERS["include/splatco_tsdf_sparse.h"] is _C.TSDFS_SIGNATURES
    assert _C.TSDF_ABI_VERSION == 1 and _C.ABI_VERSION == 37          # a family of its own: the other versions stay


def test_view_struct_extends_the_dense_view():
    from splatco_amd import _C
    body = re.search(r"typedef\s+struct\s+scr_tsdfs_view\s*\{(.*?)\}\s*scr_tsdfs_view\s*;", _header()[1], flags=re.S).group(1)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert decls == ["scr_tsdf_view view", "double c2w[12]"]
    assert [(n, t) for n, t in _C.TsdfsView._fields_] == [("view", _C.TsdfView), ("c2w", ctypes.c_double * 12)]
    assert ctypes.sizeof(_C.TsdfsView) == 184 + 96 and _C.TsdfsView.c2w.offset == 184


def test_every_declared_symbol_is_exported_and_no_other_header_knows_it():
    from splatco_amd import _C
    lib = ctypes.CDLL(os.path.join(ROOT, "splatco_amd", "csrc", "libsplatco_raster.so"))
    for name in NAMES:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "splatco_tsdf_sparse.h":
            assert "scr_tsdfs" not in open(os.path.join(ROOT, "include", other)).read(), other
    # the size queries (no device needed): one uint32 per workgroup of 1024 items, + 1, 256-byte aligned, + 256 for the total
    size = lambda items: (((items + 1023) // 1024 + 1) * 4 + 255) // 256 * 256 + 256
    assert _C.lib.scr_tsdfs_alloc_scratch_bytes(40, 27, 19) == size(5 * 4 * 3)
    assert _C.lib.scr_tsdfs_alloc_scratch_bytes(2048, 2048, 2048) == size(256 ** 3)
    assert _C.lib.scr_tsdfs_alloc_scratch_bytes(1, 5, 5) == 256 and _C.lib.scr_tsdfs_alloc_scratch_bytes(2 ** 20, 8, 8) == 256
    assert _C.lib.scr_tsdfs_extract_scratch_bytes(60) == size(6144 * 60)
    assert _C.lib.scr_tsdfs_extract_scratch_bytes(0) == 256 and _C.lib.scr_tsdfs_extract_scratch_bytes(349526) == 256
    assert splatco_amd.tsdf_sparse.MAX_EXTRACT_BLOCKS == 349525 and _C.lib.scr_tsdfs_extract_scratch_bytes(349525) > 256


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    return ".".join(reversed(parts + [node.id])) if isinstance(node, ast.Name) else ""


def test_the_module_launches_through_family_call_only():
    streamed = {n: n not in UNSTREAMED for n in NAMES}
    tree = ast.parse(open(os.path.join(ROOT, "splatco_amd", "tsdf_sparse.py")).read())
    called = []
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        name, where = _dotted(node.func), f"tsdf_sparse.py:{node.lineno}"
        if name in ("_C.family_call", "family_call"):
            first = node.args[0] if node.args else None
            assert isinstance(first, ast.Constant) and isinstance(first.value, str), f"{where}: the name is not a string literal"
            assert streamed.get(first.value, False), f"{where}: {first.value} is not a streamed function of splatco_tsdf_sparse.h"
            called.append(first.value)
        elif ".lib.scr_" in "." + name:
            assert not streamed.get(name.rsplit(".", 1)[1], True), f"{where}: {name} takes a stream: launch it through _C.family_call"
        else:
            assert name not in ("_C.call", "call"), f"{where}: this family launches through _C.family_call"
            assert not name.endswith("cuda.device"), f"{where}: torch.cuda.device(...) outside _C"
    assert sorted(set(called)) == sorted(n for n in NAMES if n not in UNSTREAMED)


@pytest.mark.skipif(torch.cuda.is_available(), reason="replays rejected calls only where nothing can be launched")
def test_c_abi_checks_sizes_and_scalars_first():
    """Validated before anything is launched; 16 stands for any non-null device address (never dereferenced on the host)."""
    from splatco_amd import _C
    lib, p = _C.lib, 16
    err = lambda: lib.scr_last_error().decode()
    nan, inf = float("nan"), float("inf")
    lo = _C.host_array((0.0, 0.0, 0.0), _C.f32)
    eye = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)

    def view(c2w=eye, **kw):
        f = dict(depth=p, alpha=p, image=None, mask=None, H=4, W=5, mask_kind=0, min_alpha=0.5, fx=3.0, fy=3.0, cx=2.0, cy=2.0,
                 w2c=(ctypes.c_double * 12)(*eye), near=0.05)
        f.update(kw)
        return _C.TsdfsView(_C.TsdfView(*[f[n] for n, _ in _C.TsdfView._fields_]), (ctypes.c_double * 12)(*c2w))

    cnt = ctypes.c_int64(7)

    def plan(dims=(40, 27, 19), lo=lo, h=0.1, trunc=0.4, marks=p, scratch=p, count=ctypes.byref(cnt), v=None, **kw):
        return lib.scr_tsdfs_alloc_plan(*dims, lo, h, trunc, ctypes.byref(view(**kw)) if v is None else v, marks, scratch, count, None)

    name = "scr_tsdfs_alloc_plan"
    for kw, text in ((dict(count=None), "count_host"), (dict(dims=(1, 3, 3)), ">= 2"), (dict(dims=(2 ** 20, 3, 3)), "2^20"),
                     (dict(dims=(2 ** 20 - 1, 2 ** 20 - 1, 2 ** 20 - 1)), "block count"), (dict(h=0.0), "h ="), (dict(trunc=nan), "trunc"),
                     (dict(lo=None), "lo_host"), (dict(v=ctypes.POINTER(_C.TsdfsView)()), "view_host"), (dict(H=0), "H = 0"),
                     (dict(fx=0.0), "fx"), (dict(cy=inf), "cy"), (dict(c2w=(nan,) * 12), "c2w"), (dict(near=-1.0), "near"),
                     (dict(min_alpha=nan), "min_alpha"), (dict(mask_kind=3), "mask_kind"), (dict(marks=None), "NULL"),
                     (dict(scratch=None), "NULL"), (dict(depth=None), "NULL map"), (dict(mask_kind=1), "mask is NULL")):
        cnt.value = 7
        assert plan(**kw) == 1 and err().startswith(name + ":") and text in err(), (kw, err())
        assert kw.get("count", 0) is None or cnt.value == 0
    assert plan(dims=(1, 3, 3), marks=None) == 1 and ">= 2" in err()          # sizes and scalars before the pointers
    assert plan(fx=0.0, depth=None) == 1 and "fx" in err()

    def run(dims=(40, 27, 19), marks=p, scratch=p, old=3, ko=p, so=p, new=2, nk=p, keys=p, slots=p):
        return lib.scr_tsdfs_alloc_run(*dims, marks, scratch, old, ko, so, new, nk, keys, slots, None)

    name = "scr_tsdfs_alloc_run"
    for kw, text in ((dict(dims=(3, 3, 0)), ">= 2"), (dict(old=-1), "nb ="), (dict(old=61), "nb ="), (dict(new=-1), "nnew"),
                     (dict(old=59, new=2), "nnew"), (dict(marks=None), "NULL"), (dict(nk=None), "NULL"), (dict(keys=None), "NULL"),
                     (dict(ko=None), "old lists")):
        assert run(**kw) == 1 and err().startswith(name + ":") and text in err(), (kw, err())
    assert run(new=0, marks=None) == 0                                          # nothing new: a no-op whatever the pointers

    name = "scr_tsdfs_init_blocks"
    for args, text in (((-1, 2, p, p, p), "rows"), ((0, -2, p, p, p), "rows"), ((2 ** 31, 1, p, p, p), "rows"), ((0, 2, None, p, p), "NULL"),
                       ((0, 2, p, 20, p), "aligned")):
        assert lib.scr_tsdfs_init_blocks(*args, None) == 1 and err().startswith(name + ":") and text in err(), (args, err())
    assert lib.scr_tsdfs_init_blocks(5, 0, None, None, None, None) == 0

    def integ(dims=(40, 27, 19), lo=lo, h=0.1, trunc=0.4, mw=255.0, nb=4, keys=p, slots=p, tsdf=p, weight=p, color=p, **kw):
        return lib.scr_tsdfs_integrate(*dims, lo, h, trunc, mw, nb, keys, slots, tsdf, weight, color, ctypes.byref(view(**kw)), None)

    name = "scr_tsdfs_integrate"
    for kw, text in ((dict(dims=(1, 3, 3)), ">= 2"), (dict(h=inf), "h ="), (dict(trunc=0.0), "trunc"), (dict(mw=0.0), "max_weight"),
                     (dict(nb=-1), "nb ="), (dict(nb=61), "nb ="), (dict(W=-2), "W = -2"), (dict(w2c=(ctypes.c_double * 12)(*(nan,) * 12)), "w2c"),
                     (dict(keys=None), "NULL volume"), (dict(weight=None), "NULL volume"), (dict(tsdf=24), "aligned"),
                     (dict(alpha=None), "NULL map"), (dict(image=p, color=None), "no colour")):
        assert integ(**kw) == 1 and err().startswith(name + ":") and text in err(), (kw, err())
    assert integ(mw=0.0, tsdf=None) == 1 and "max_weight" in err()
    assert integ(nb=0, tsdf=None, keys=None) == 0

    name = "scr_tsdfs_neighbors"
    for args, text in (((3, 3, 1, 2, p, p), ">= 2"), ((40, 27, 19, 61, p, p), "nb ="), ((40, 27, 19, 2, None, p), "NULL"), ((40, 27, 19, 2, p, None), "NULL")):
        assert lib.scr_tsdfs_neighbors(*args, None) == 1 and err().startswith(name + ":") and text in err(), (args, err())

    big = (2 ** 20 - 1, 8192, 64)
    for fn, name in ((lib.scr_tsdfs_extract_vertices_plan, "scr_tsdfs_extract_vertices_plan"), (lib.scr_tsdfs_extract_faces_plan, "scr_tsdfs_extract_faces_plan")):
        def eplan(dims=(40, 27, 19), nb=4, first=0, n=4, keys=p, slots=p, table=p, tsdf=p, weight=p, mw=0.0, scratch=p, count=ctypes.byref(cnt)):
            return fn(*dims, nb, first, n, keys, slots, table, tsdf, weight, mw, scratch, count, None)
        for kw, text in ((dict(count=None), "count_host"), (dict(dims=(4, 1, 2)), ">= 2"), (dict(nb=61), "nb ="), (dict(first=3, n=2), "blocks 3 + 2"),
                         (dict(first=-1), "blocks -1"), (dict(n=-1), "blocks 0 + -1"), (dict(dims=big, nb=349526, n=349526), "6144 count"),
                         (dict(mw=nan), "min_weight"), (dict(table=None), "NULL"), (dict(scratch=None), "NULL")):
            cnt.value = 7
            assert eplan(**kw) == 1 and err().startswith(name + ":") and text in err(), (name, kw, err())
            assert kw.get("count", 0) is None or cnt.value == 0
        cnt.value = 7
        assert eplan(n=0, keys=None) == 0 and cnt.value == 0                    # an empty pass: nothing to count
        assert eplan(dims=big, nb=349526, first=1, n=349525, keys=None) == 1 and "NULL" in err()      # a pass of a larger volume is in range

    def vrun(dims=(40, 27, 19), lo=lo, h=0.1, nb=4, first=0, n=4, keys=p, table=p, color=p, mw=0.0, nv=5, ids=p, verts=p, cols=p):
        return lib.scr_tsdfs_extract_vertices_run(*dims, lo, h, nb, first, n, keys, p, table, p, p, color, mw, p, nv, ids, verts, cols, None)

    name = "scr_tsdfs_extract_vertices_run"
    for kw, text in ((dict(dims=(4, 3, 1)), ">= 2"), (dict(h=0.0), "h ="), (dict(lo=None), "lo_host"), (dict(nb=61), "nb ="), (dict(mw=nan), "min_weight"),
                     (dict(nv=-1), "nv"), (dict(nv=2 ** 31), "nv"), (dict(n=0), "no blocks"), (dict(first=4, n=1), "blocks 4 + 1"), (dict(keys=None), "NULL"),
                     (dict(ids=None), "NULL"),
                     (dict(color=None), "both or neither"), (dict(cols=None), "both or neither")):
        assert vrun(**kw) == 1 and err().startswith(name + ":") and text in err(), (kw, err())
    assert vrun(nv=0, keys=None, ids=None) == 0

    def frun(dims=(40, 27, 19), nb=4, first=0, n=4, keys=p, mw=0.0, nv=5, ids=p, nf=3, faces=p):
        return lib.scr_tsdfs_extract_faces_run(*dims, nb, first, n, keys, p, p, p, p, mw, p, nv, ids, nf, faces, None)

    name = "scr_tsdfs_extract_faces_run"
    for kw, text in ((dict(dims=(0, 3, 3)), ">= 2"), (dict(mw=nan), "min_weight"), (dict(nv=-1), "nv"), (dict(nf=-1), "nf"), (dict(nf=2 ** 31), "nf"),
                     (dict(nv=0), "no vertices"), (dict(n=0), "no vertices"), (dict(first=2, n=3), "blocks 2 + 3"), (dict(keys=None), "NULL"), (dict(ids=None), "NULL"), (dict(faces=None), "NULL")):
        assert frun(**kw) == 1 and err().startswith(name + ":") and text in err(), (kw, err())
    assert frun(nf=0, faces=None) == 0


# ------------------------------------------------------------------ the allocation rule
@pytest.mark.parametrize("dims", SHAPES)
def test_allocation_rule_covers_the_band(dims):
    """Every block with a node that the dense update moves with sdf <= trunc is allocated by the same view, at the definition's
    pad and at the two pads the GPU test brackets the device with; at (40, 27, 19) the rule leaves blocks out."""
    lo, h = ref.volume_geometry(dims)
    trunc = 4.0 * float(h)
    nb = int(np.prod(sref.block_dims(dims)))
    for view in ref.parity_views(dims):
        band = sref.band_blocks(dims, lo, h, trunc, view)
        assert band.any()
        sets = [sref.allocate_ref(dims, lo, h, trunc, view, pad=float(h) * (0.125 + e)) for e in (-1e-6, 0.0, 1e-6)]
        for got in sets:
            assert got.shape == band.shape and not (band & ~got).any(), f"{int((band & ~got).sum())} band blocks were not allocated"
        assert np.array_equal(sets[0], sets[1]) and np.array_equal(sets[1], sets[2]), "the recipe's set hangs on the pad's last bits"
        assert np.array_equal(sets[1], sref.allocate_ref(dims, lo, h, trunc, view))
        if dims == (40, 27, 19):
            assert nb == 60 and 0 < int(sets[1].sum()) < nb


def test_block_helpers_round_trip():
    dims = (17, 9, 10)
    assert sref.block_dims(dims) == (3, 2, 2)
    nodes = np.zeros((10, 9, 17), bool)
    nodes[9, 8, 16] = nodes[0, 0, 7] = True
    blocks = sref.blocks_of(nodes)
    assert blocks.shape == (2, 2, 3) and np.nonzero(blocks.reshape(-1))[0].tolist() == [0, (1 * 2 + 1) * 3 + 2]
    back = sref.nodes_of(blocks, dims)
    assert back.shape == nodes.shape and back[9, 8, 16] and back[7, 7, 0] and not back[0, 0, 8] and int(back.sum()) == 512 + 2 * 1 * 1


# ------------------------------------------------------------------ the host side: every ValueError, and no launch
@pytest.fixture
def no_launch(monkeypatch):
    from splatco_amd import _C
    made = []
    monkeypatch.setattr(_C, "family_call", lambda *a, **k: made.append(a[0]))
    yield made
    assert made == [], f"launched {made}"


def _meta_volume(dims=(17, 9, 10), color=True):
    """A volume whose tensors live on the meta device: enough for every check that comes before a launch."""
    from splatco_amd.tsdf import TSDFVolume
    from splatco_amd.tsdf_sparse import SparseTSDFVolume, _check_dims
    vol = SparseTSDFVolume.__new__(SparseTSDFVolume)
    TSDFVolume._geometry(vol, "test", (0.0, 0.0, 0.0), 0.1, (2, 2, 2), None, 255.0)
    vol.dims, vol.block_dims = _check_dims("test", dims)
    vol.max_blocks, vol._color = 12, color
    vol.keys = vol.slots = torch.zeros(0, dtype=torch.int32, device="meta")
    vol._marks = torch.empty(12, dtype=torch.uint8, device="meta")
    vol._store(4, "meta")
    return vol


def test_python_refusals(no_launch):
    from splatco_amd.tsdf_sparse import SparseTSDFVolume
    for kw, text in ((dict(dims=(1, 4, 4)), ">= 2"), (dict(dims=(4, 4)), "three sizes"), (dict(dims=(2 ** 20, 4, 4)), "below 2.20"),
                     (dict(dims=(2 ** 20 - 1,) * 3), "block count"), (dict(voxel_size=0.0), "voxel_size"), (dict(trunc=-1.0), "trunc"),
                     (dict(lo=(0.0, float("nan"), 0.0)), "finite"), (dict(max_weight=0.0), "max_weight"), (dict(device="cpu"), "no CPU path"),
                     (dict(max_blocks=0), "max_blocks"), (dict(capacity=0), "capacity")):
        args = dict(lo=(0.0, 0.0, 0.0), voxel_size=0.1, dims=(17, 9, 10), device="meta")
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            SparseTSDFVolume(**args)
    with pytest.raises(ValueError, match="lo <= hi"):
        SparseTSDFVolume.from_bounds((0, 0, 0), (1, -1, 1), 0.1)
    vol = _meta_volume()
    assert vol.num_blocks == 0 and vol.capacity == 4 and vol.block_dims == (3, 2, 2) and vol.color.shape == (4, 3, 512)
    H, W = 6, 5
    cam = ((4.0, 4.0, 2.5, 3.0), torch.eye(4, dtype=torch.float64))
    meta = lambda *s: torch.empty(*s, device="meta")
    cpu = torch.ones(H, W)
    for call, text in ((lambda: vol.allocate(cpu, meta(H, W), cam), "no CPU path"),
                       (lambda: vol.integrate(meta(H, W), cpu, cam), "no CPU path"),
                       (lambda: vol.integrate(meta(H, W), meta(H, W), cam, image=torch.ones(3, H, W)), "no CPU path"),
                       (lambda: vol.integrate_views([meta(H, W)], [meta(H, W)], [cam], masks=[cpu > 0]), "no CPU path"),
                       (lambda: vol.allocate(meta(H, W), meta(H, W + 1), cam), "does not match"),
                       (lambda: vol.allocate(meta(H, W), meta(H, W), cam, near=-1.0), "near"),
                       (lambda: vol.allocate(meta(H, W), meta(H, W), cam, min_alpha=float("inf")), "min_alpha"),
                       (lambda: vol.integrate_views([meta(H, W)], [meta(H, W)], [cam, cam]), "2 cams for 1 depths"),
                       (lambda: vol.extract(min_weight=float("nan")), "NaN"),
                       (lambda: SparseTSDFVolume.from_dense(object()), "not a TSDFVolume")):
        with pytest.raises(ValueError, match=text):
            call()
    with pytest.raises(ValueError, match="color=False"):
        _meta_volume(color=False).integrate(meta(H, W), meta(H, W), cam, image=meta(3, H, W))
    big = _meta_volume(dims=(2048, 2048, 2048))
    assert big.block_dims == (256, 256, 256)
    with pytest.raises(ValueError, match="2\\^31"):
        big.to_dense()
    for bad in (0, 349526):
        with pytest.raises(ValueError, match="pass_blocks"):
            big.extract(pass_blocks=bad)
    assert _meta_volume().extract()[0].shape == (0, 3)                          # an empty volume: nothing is launched
