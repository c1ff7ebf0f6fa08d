"""Per-view bilateral grids, everything that needs no device: the restatement the GPU tests compare against
(tests/bilagrid_ref.py) on a per-pixel loop written out here and against float64 autograd, the C-ABI surface of
include/splatco_bilagrid.h against _C.BILAGRID_SIGNATURES, _C.family_call, the argument rejections of the entry points and
the Python wrapper's own."""
import ast
import ctypes
import math
import os
import re

import pytest
import torch

import bilagrid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "splatco_bilagrid.h")
SHAPES = [(7, 5, 16, 16, 8), (9, 13, 3, 5, 4), (1, 1, 2, 2, 2)]            # (H, W, Gh, Gw, L)


def _inputs(H, W, Gh, Gw, L, seed=0):
    g = torch.Generator().manual_seed(seed)
    grid = torch.randn(12, L, Gh, Gw, generator=g, dtype=torch.float64)
    rgb = 1.6 * torch.rand(3, H, W, generator=g, dtype=torch.float64) - 0.3
    dout = torch.randn(3, H, W, generator=g, dtype=torch.float64)
    return grid, rgb, dout


def _loop(grid, rgb, dout):
    """The definition pixel by pixel in Python floats (binary64): out, dL/drgb, dL/dgrid and the clamp flags."""
    _, L, Gh, Gw = grid.shape
    _, H, W = rgb.shape
    G = grid.tolist()
    out = torch.zeros(3, H, W, dtype=torch.float64)
    d_rgb = torch.zeros(3, H, W, dtype=torch.float64)
    d_grid = torch.zeros(12, L, Gh, Gw, dtype=torch.float64)
    low = high = 0
    for py in range(H):
        for px in range(W):
            c = [float(rgb[k, py, px]) for k in range(3)] + [1.0]
            go = [float(dout[k, py, px]) for k in range(3)]
            u, v = (px + 0.5) / W * (Gw - 1), (py + 0.5) / H * (Gh - 1)
            lum = (0.299 * c[0] + 0.587 * c[1]) + 0.114 * c[2]
            low, high = low + (lum <= 0), high + (lum >= 1)
            z = min(max(lum, 0.0), 1.0) * (L - 1)
            x0, y0, l0 = min(int(math.floor(u)), Gw - 2), min(int(math.floor(v)), Gh - 2), min(int(math.floor(z)), L - 2)
            fx, fy, fz = u - x0, v - y0, z - l0
            A, dA = [0.0] * 12, [0.0] * 12
            for dl, wl, sl in ((0, 1 - fz, -1.0), (1, fz, 1.0)):
                for dy, wy in ((0, 1 - fy), (1, fy)):
                    for dx, wx in ((0, 1 - fx), (1, fx)):
                        for ch in range(12):
                            val = G[ch][l0 + dl][y0 + dy][x0 + dx]
                            A[ch] += wl * wy * wx * val
                            dA[ch] += sl * wy * wx * val
                            d_grid[ch, l0 + dl, y0 + dy, x0 + dx] += wl * wy * wx * go[ch // 4] * c[ch % 4]
            through = 0.0
            for i in range(3):
                out[i, py, px] = sum(A[4 * i + j] * c[j] for j in range(4))
                through += go[i] * sum(dA[4 * i + j] * c[j] for j in range(4))
            through = through * (L - 1) if 0 < lum < 1 else 0.0
            for j, k in enumerate(ref.LUMA):
                d_rgb[j, py, px] = sum(A[4 * i + j] * go[i] for i in range(3)) + through * k
    return out, d_rgb, d_grid, low, high


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1.0)


@pytest.mark.parametrize("H,W,Gh,Gw,L", SHAPES)
def test_restatement_equals_the_per_pixel_loop_and_float64_autograd(H, W, Gh, Gw, L):
    # (1, 1): one pixel cannot clamp on both sides; test_one_pixel_images_clamp_on_either_side covers its clamps
    grid, rgb, dout = _inputs(H, W, Gh, Gw, L)
    want = _loop(grid, rgb, dout)
    if H * W > 1:
        assert want[3] >= 1 and want[4] >= 1, "the inputs must clamp on either side"
    auto = ref.slice_with_grads(grid, rgb, dout)
    expl = ref.slice_explicit(grid, rgb, dout)
    for k, name in enumerate(("out", "dL/drgb", "dL/dgrid")):
        assert _close(auto[k], want[k]), (name, "grid_sample + autograd against the loop")
        assert _close(expl[k], want[k]), (name, "closed form against the loop")
    assert int((expl[3] < 0).sum()) == want[3] and int((expl[3] > 0).sum()) == want[4]
    # where the luminance is clamped the guide carries nothing: autograd's dL/drgb is A[:, :3]^T dL/dout alone
    no_guide = ref.rgb_grad_without_guide(grid, rgb, dout)
    hit = (expl[3] != 0).expand(3, H, W)
    assert torch.allclose(auto[1][hit], no_guide[hit], rtol=1e-12, atol=1e-12)
    if H * W > 1:
        assert not torch.allclose(auto[1][~hit], no_guide[~hit], rtol=1e-6, atol=1e-6)


def test_one_pixel_images_clamp_on_either_side():
    for value, flag in ((-0.2, -1), (1.3, 1), (0.0, -1)):
        grid, _, dout = _inputs(1, 1, 2, 2, 2, seed=3)
        rgb = torch.full((3, 1, 1), value, dtype=torch.float64)
        want = _loop(grid, rgb, dout)
        auto = ref.slice_with_grads(grid, rgb, dout)
        expl = ref.slice_explicit(grid, rgb, dout)
        assert int(expl[3]) == flag
        for k in range(3):
            assert _close(auto[k], want[k]) and _close(expl[k], want[k])
        assert torch.allclose(auto[1], ref.rgb_grad_without_guide(grid, rgb, dout), rtol=1e-12, atol=1e-12)


def test_cell_shift_gives_the_other_one_sided_derivative_on_a_level():
    """z a hair above level 1 of 3 (even a constant 0.5 does not give a luminance of exactly 0.5: the three weights do not add
    up to 1 in binary arithmetic).  out and dL/dgrid are the same from either cell to that hair; dL/drgb from the cell below
    is the derivative on the other side of the level."""
    g = torch.Generator().manual_seed(5)
    grid = torch.randn(12, 3, 2, 2, generator=g, dtype=torch.float64)
    dout = torch.randn(3, 2, 2, generator=g, dtype=torch.float64)
    above, below = (torch.full((3, 2, 2), 0.5 + s * 1e-9, dtype=torch.float64) for s in (1, -1))
    lum = lambda c: (0.299 * c[0] + 0.587 * c[1]) + 0.114 * c[2]
    assert bool((lum(above) * 2 > 1).all()) and bool((lum(below) * 2 < 1).all())
    own = ref.slice_explicit(grid, above, dout)
    shifted = ref.slice_explicit(grid, above, dout, cell_shift=torch.full((2, 2), -1, dtype=torch.long))
    assert _close(own[0], shifted[0], 1e-7) and _close(own[2], shifted[2], 1e-7)
    assert not _close(own[1], shifted[1], 1e-3)
    assert _close(own[1], ref.slice_with_grads(grid, above, dout)[1])
    assert _close(shifted[1], ref.slice_with_grads(grid, below, dout)[1], 1e-7)


@pytest.mark.parametrize("N,L,Gh,Gw", [(1, 2, 2, 2), (3, 8, 16, 16), (2, 4, 5, 3)])
def test_closed_form_tv_gradient_equals_float64_autograd(N, L, Gh, Gw):
    g = torch.Generator().manual_seed(N)
    grids = torch.randn(N, 12, L, Gh, Gw, generator=g, dtype=torch.float64).requires_grad_()
    weight = 10.0
    (weight * ref.tv(grids)).backward()
    got = ref.tv_grad_closed_form(grids.detach(), weight)
    assert float((got - grids.grad).abs().max() / grids.grad.abs().max()) < 1e-13
    # c_d: the pairs of ONE view's grid, 12 channels included
    one = torch.zeros(1, 12, L, Gh, Gw, dtype=torch.float64)
    one[:, :, 1:] = 1.0                                                   # one unit step along L at every (channel, y, x)
    assert float(ref.tv(one)) == pytest.approx(1.0 / (L - 1), rel=1e-15)


# ------------------------------------------------------------------ the header and the binding
_SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double}


def _header():
    hdr = open(HEADER).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    return hdr, re.sub(r"^\s*#[^\n]*", "", hdr, flags=re.M)


def _prototypes():
    """[(return type, name, [parameter text])] of the header's functions, in header order."""
    protos = re.findall(r"([A-Za-z_][\w\s*]*?)\b(scr_\w+)\s*\(([^()]*)\)\s*;", _header()[1])
    return [(ret.strip(), name, [] if params.strip() == "void" else [p.strip() for p in params.split(",")])
            for ret, name, params in protos]


def _streamed():
    return {name: bool(params) and "".join(params[-1].split()) == "void*stream" for _, name, params in _prototypes()}


def _c_type(decl):
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    return next(w for w in words if w != "*"), words.count("*")


def _binds(base, depth, got):
    if depth == 0:
        return got is _SCALARS.get(base, object())
    return got is ctypes.c_void_p


def test_binding_matches_the_new_header():
    from splatco_amd import _C
    hdr, _ = _header()
    m = re.search(r"^\s*#\s*define\s+SCR_BILAGRID_ABI_VERSION\s+(\d+)\s*$", hdr, flags=re.M)
    assert m and int(m.group(1)) == _C.BILAGRID_ABI_VERSION == _C.lib.scr_bilagrid_abi_version() == 1
    protos = _prototypes()
    assert [name for _, name, _ in protos] == [s[0] for s in _C.BILAGRID_SIGNATURES] == [
        "scr_bilagrid_abi_version", "scr_bilagrid_scratch_bytes", "scr_bilagrid_slice", "scr_bilagrid_slice_backward",
        "scr_bilagrid_tv_add_grad"]
    for (ret, name, params), (_, restype, *argtypes) in zip(protos, _C.BILAGRID_SIGNATURES):
        assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes for {len(params)} parameters"
        assert _binds(*_c_type(ret), restype), f"{name}: restype {restype.__name__} does not bind {ret}"
        for i, (p, got) in enumerate(zip(params, argtypes)):
            assert _binds(*_c_type(p), got), f"{name} parameter {i} `{p}`: {got.__name__}"
        f = getattr(_C.lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, f"{name}: not bound from BILAGRID_SIGNATURES"
    streamed = _streamed()
    assert [n for n, s in streamed.items() if s] == ["scr_bilagrid_slice", "scr_bilagrid_slice_backward", "scr_bilagrid_tv_add_grad"]
    assert [len(p) for _, _, p in protos] == [0, 5, 9, 13, 8]


def test_every_declared_symbol_is_exported_and_the_first_header_knows_none_of_them():
    from splatco_amd import _C
    lib = ctypes.CDLL(os.path.join(ROOT, "splatco_amd", "csrc", "libsplatco_raster.so"))
    names = [name for _, name, _ in _prototypes()]
    assert len(names) == 5
    for name in names:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert not [s for s in _C.SYMBOLS if s.startswith("scr_bilagrid")]
    assert "scr_bilagrid" not in open(os.path.join(ROOT, "include", "splatco_raster.h")).read()
    assert _C.ABI_VERSION == 37
    # pure size queries (no device needed): 256-byte aligned, growing with the parts a vertex's rectangle is split into
    q = _C.lib.scr_bilagrid_scratch_bytes
    small, full_hd = q(8, 16, 16, 7, 5), q(8, 16, 16, 1080, 1920)
    assert small % 256 == 0 and small == 256 * 8 * 12 * 4 and full_hd > small and full_hd % 256 == 0
    assert q(8, 16, 16, 1080, 1920) == q(8, 16, 16, 1080, 64)              # the rows decide, not the columns
    assert q(1, 16, 16, 7, 5) == 256 and q(8, 16, 16, 0, 5) == 256


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    return ".".join(reversed(parts + [node.id])) if isinstance(node, ast.Name) else ""


def test_the_module_launches_through_family_call_only():
    streamed = _streamed()
    tree = ast.parse(open(os.path.join(ROOT, "splatco_amd", "bilagrid.py")).read())
    calls = 0
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        name, where = _dotted(node.func), f"bilagrid.py:{node.lineno}"
        if name in ("_C.family_call", "family_call"):
            calls += 1
            first = node.args[0] if node.args else None
            assert isinstance(first, ast.Constant) and isinstance(first.value, str), f"{where}: the name is not a string literal"
            assert streamed.get(first.value, False), f"{where}: {first.value} is not a streamed function of splatco_bilagrid.h"
        elif ".lib.scr_bilagrid_" in "." + name:
            assert not streamed.get(name.rsplit(".", 1)[1], True), f"{where}: {name} takes a stream: launch it through _C.family_call"
        else:
            assert name not in ("_C.call", "call"), f"{where}: this family launches through _C.family_call"
            assert not name.endswith("cuda.device"), f"{where}: torch.cuda.device(...) outside _C"
    assert calls == 3


class _Recorder:
    def __init__(self, rc=0):
        self.rc, self.args = rc, None

    def __call__(self, *args):
        self.args = args
        return self.rc


def test_family_call_refuses_other_names_before_anything_is_called(monkeypatch):
    from splatco_amd import _C
    other, own = _Recorder(), _Recorder()
    monkeypatch.setattr(_C.lib, "scr_forward_run", other)
    monkeypatch.setattr(_C.lib, "scr_bilagrid_slice", own)
    a = torch.zeros(4)
    with pytest.raises(ValueError, match="scr_forward_run"):
        _C.family_call("scr_forward_run", a)
    with pytest.raises(ValueError, match="scr_no_such_entry_point"):
        _C.family_call("scr_no_such_entry_point", a)
    with pytest.raises(ValueError, match="scr_bilagrid_abi_version|scr_copy_probe"):
        _C.family_call("scr_copy_probe", a, a, 16)
    assert other.args is None
    # call()'s own checks, through the same code: operands on two devices, no device at all
    with pytest.raises(ValueError) as e:
        _C.family_call("scr_bilagrid_slice", a, 8, 16, 16, torch.zeros(4, device="meta"), 1, 1, None)
    assert "scr_bilagrid_slice" in str(e.value) and "argument 4" in str(e.value) and "meta" in str(e.value)
    with pytest.raises(ValueError, match="device"):
        _C.family_call("scr_bilagrid_slice", None, 8, 16, 16, None, 1, 1, None)
    assert own.args is None
    assert _C.call.__code__ is not _C.family_call.__code__ and "_launch" in _C.call.__code__.co_names + _C.family_call.__code__.co_names


@pytest.mark.skipif(torch.cuda.is_available(), reason="replays rejected calls only where nothing can be launched")
def test_c_abi_checks_sizes_first_and_takes_empty_input():
    """Validated before anything is launched; 16 stands for any non-null device address (never dereferenced on the host)."""
    from splatco_amd import _C
    lib, p = _C.lib, 16
    err = lambda: lib.scr_last_error().decode()
    fwd = lambda L=8, Gh=16, Gw=16, H=4, W=4, grid=p, rgb=p, out=p: lib.scr_bilagrid_slice(grid, L, Gh, Gw, rgb, H, W, out, None)
    bwd = lambda L=8, Gh=16, Gw=16, H=4, W=4, grid=p, rgb=p, dout=p, drgb=p, dgrid=p, scratch=p, nbytes=1 << 30: \
        lib.scr_bilagrid_slice_backward(grid, L, Gh, Gw, rgb, dout, H, W, drgb, dgrid, scratch, nbytes, None)
    tv = lambda N=1, L=8, Gh=16, Gw=16, grids=p, grads=32: lib.scr_bilagrid_tv_add_grad(grids, grads, N, L, Gh, Gw, 1.0, None)
    for fn, name in ((fwd, "scr_bilagrid_slice"), (bwd, "scr_bilagrid_slice_backward"), (tv, "scr_bilagrid_tv_add_grad")):
        for kw, text in ((dict(L=1), "L = 1"), (dict(L=17), "L = 17"), (dict(Gw=65), "Gw = 65"), (dict(Gh=1), "Gh = 1")):
            assert fn(**kw) == 1 and err().startswith(name + ":") and text in err(), (name, kw, err())
    for fn, name in ((fwd, "scr_bilagrid_slice"), (bwd, "scr_bilagrid_slice_backward")):
        assert fn(H=-1) == 1 and err().startswith(name + ":") and "H = -1" in err()
        assert fn(H=65536, W=32768) == 1 and err().startswith(name + ":") and "2^31" in err()
        assert fn(H=46341, W=46341) == 1 and "2^31" in err()
        # sizes are checked before the pointers
        assert fn(L=17, grid=None, rgb=None) == 1 and "L = 17" in err()
        assert fn(grid=None) == 1 and err().startswith(name + ":") and "NULL" in err()
        assert fn(rgb=None) == 1 and "NULL" in err()
        # H W == 0: a no-op, whatever the pointers
        assert fn(H=0, grid=None, rgb=None) == 0 and fn(W=0) == 0 and fn(H=0, W=0) == 0
    assert fwd(out=None) == 1 and "NULL" in err()
    assert bwd(dout=None) == 1 and "NULL" in err()
    assert bwd(scratch=None) == 1 and err().startswith("scr_bilagrid_slice_backward:") and "scratch" in err()
    assert bwd(nbytes=16) == 1 and "scratch" in err()
    assert tv(N=0, grids=None, grads=None) == 0
    assert tv(N=-1) == 1 and err().startswith("scr_bilagrid_tv_add_grad:") and "N = -1" in err()
    assert tv(grids=None) == 1 and "NULL" in err()
    assert tv(grads=None) == 1 and "NULL" in err()
    assert tv(grads=p) == 1 and "distinct" in err()
    assert tv(N=2 ** 31 // (12 * 8 * 16 * 16) + 1) == 1 and "2^31" in err()


def test_python_side_refuses_what_the_kernels_do_not_take():
    from splatco_amd import bilagrid
    grid = torch.zeros(12, 8, 16, 16)
    image = torch.zeros(3, 6, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        bilagrid.slice_apply(grid, image)
    with pytest.raises(ValueError, match=r"\[3, H, W\]"):
        bilagrid.slice_apply(grid, torch.zeros(4, 6, 5))
    with pytest.raises(ValueError, match="float32"):
        bilagrid.slice_apply(grid.double(), image)
    with pytest.raises(ValueError, match="float32"):
        bilagrid.slice_apply(grid, image.double())
    with pytest.raises(ValueError, match=r"\[12, L, Gh, Gw\]"):
        bilagrid.slice_apply(grid[:11], image)
    with pytest.raises(ValueError, match="outside"):
        bilagrid.slice_apply(torch.zeros(12, 17, 16, 16), image)
    bil = bilagrid.BilateralGrid(3, device="cpu")
    assert bil.grids.shape == (3, 12, 8, 16, 16) and bil.grids.dtype == torch.float32 and bil.num_views == 3
    A = bil.grids.detach().reshape(3, 3, 4, 8, 16, 16)
    assert torch.equal(A[0, :, :, 5, 7, 9], torch.eye(3, 4)) and torch.equal(A, A[:1, :, :, :1, :1, :1].expand_as(A))
    assert [n for n, _ in bil.named_parameters()] == ["grids"]
    for index in (3, -1):
        with pytest.raises(IndexError):
            bil(image, index)
    with pytest.raises(RuntimeError, match="no CPU path"):
        bil(image, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        bilagrid.tv_add_grad(bil.grids, 10.0)
    with pytest.raises(ValueError):
        bilagrid.BilateralGrid(3, grid_w=1, device="cpu")
    with pytest.raises(ValueError):
        bilagrid.BilateralGrid(0, device="cpu")
    shape = bilagrid.BilateralGrid(2, grid_x=5, grid_y=3, grid_w=4, device="cpu").grids.shape
    assert shape == (2, 12, 4, 3, 5)


def test_step_takes_a_bilateral_grid_and_defaults_to_none():
    import inspect
    from splatco_amd import train_step
    params = inspect.signature(train_step.collaborative_step).parameters
    assert params["bilateral_grid"].default is None and params["bilagrid_tv_weight"].default == 10.0
