"""Depth-map normals and the normal-prior loss, everything that needs no device: the C-ABI surface of
include/splatco_normals.h against _C.NORMALS_SIGNATURES, _C.family_call, the argument rejections of the entry points, the
intrinsics, the torch path against the restatement (tests/normals_ref.py), analytic planes, the recipe's preconditions and
the arguments of collaborative_step."""
import ast
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

import normals_ref as ref
import splatco_amd.normals                    # noqa: F401  (the module under test: without it nothing here can run)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "splatco_normals.h")
NAMES = ["scr_normals_abi_version", "scr_normals_map", "scr_normals_map_backward", "scr_normals_loss_scratch_bytes",
         "scr_normals_loss_forward", "scr_normals_loss_backward"]
STREAMED = ["scr_normals_map", "scr_normals_map_backward", "scr_normals_loss_forward", "scr_normals_loss_backward"]

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


def test_binding_matches_the_header():
    from splatco_amd import _C
    hdr, _ = _header()
    m = re.search(r"^\s*#\s*define\s+SCR_NORMALS_ABI_VERSION\s+(\d+)\s*$", hdr, flags=re.M)
    assert m and int(m.group(1)) == _C.NORMALS_ABI_VERSION == _C.lib.scr_normals_abi_version() == 1
    protos = _prototypes()
    assert [name for _, name, _ in protos] == [s[0] for s in _C.NORMALS_SIGNATURES] == NAMES
    for (ret, name, params), (_, restype, *argtypes) in zip(protos, _C.NORMALS_SIGNATURES):
        assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes for {len(params)} parameters"
        assert _binds(*_c_type(ret), restype), f"{name}: restype {restype.__name__} does not bind {ret}"
        for i, (p, got) in enumerate(zip(params, argtypes)):
            assert _binds(*_c_type(p), got), f"{name} parameter {i} `{p}`: {got.__name__}"
        f = getattr(_C.lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, f"{name}: not bound from NORMALS_SIGNATURES"
    assert [n for n, s in _streamed().items() if s] == STREAMED
    assert [len(p) for _, _, p in protos] == [0, 12, 14, 2, 15, 16]


def test_every_declared_symbol_is_exported_and_the_other_headers_know_none_of_them():
    from splatco_amd import _C
    lib = ctypes.CDLL(os.path.join(ROOT, "splatco_amd", "csrc", "libsplatco_raster.so"))
    for name in NAMES:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert not [s for s in _C.SYMBOLS if s.startswith("scr_normals")]
    assert not [s for s in _C.BILAGRID_SIGNATURES if s[0].startswith("scr_normals")]
    for other in ("splatco_raster.h", "splatco_bilagrid.h"):
        assert "scr_normals" not in open(os.path.join(ROOT, "include", other)).read()
    assert _C.ABI_VERSION == 37 and _C.BILAGRID_ABI_VERSION == 1
    # the size query (no device needed): one record of two doubles per 128 x 8 tile, 256-byte aligned
    q = _C.lib.scr_normals_loss_scratch_bytes
    assert q(8, 128) == 256 and q(9, 129) == 256 and q(0, 5) == 256 and q(-1, -1) == 256
    assert q(1080, 1920) == 135 * 15 * 16 + (-(135 * 15 * 16)) % 256


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    return ".".join(reversed(parts + [node.id])) if isinstance(node, ast.Name) else ""


def test_the_module_launches_through_family_call_only():
    streamed = _streamed()
    tree = ast.parse(open(os.path.join(ROOT, "splatco_amd", "normals.py")).read())
    called = []
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        name, where = _dotted(node.func), f"normals.py:{node.lineno}"
        if name in ("_C.family_call", "family_call"):
            first = node.args[0] if node.args else None
            assert isinstance(first, ast.Constant) and isinstance(first.value, str), f"{where}: the name is not a string literal"
            assert streamed.get(first.value, False), f"{where}: {first.value} is not a streamed function of splatco_normals.h"
            called.append(first.value)
        elif ".lib.scr_" in "." + name:
            assert not streamed.get(name.rsplit(".", 1)[1], True), f"{where}: {name} takes a stream: launch it through _C.family_call"
        else:
            assert name not in ("_C.call", "call"), f"{where}: this family launches through _C.family_call"
            assert not name.endswith("cuda.device"), f"{where}: torch.cuda.device(...) outside _C"
    assert sorted(called) == sorted(STREAMED)


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
    monkeypatch.setattr(_C.lib, "scr_normals_map", own)
    a = torch.zeros(4)
    for name in ("scr_depth_loss_forward", "scr_no_such_entry_point", "scr_copy_probe", "scr_normals"):
        with pytest.raises(ValueError, match=name):
            _C.family_call(name, a)
    assert other.args is None
    # the new names pass the gate and reach call()'s own checks: operands on two devices, no device at all
    with pytest.raises(ValueError) as e:
        _C.family_call("scr_normals_map", 1, 1, a, torch.zeros(4, device="meta"), 1.0, 1.0, 0.5, 0.5, None, 0.5, None)
    assert "scr_normals_map" in str(e.value) and "argument 3" in str(e.value) and "meta" in str(e.value)
    with pytest.raises(ValueError, match="device"):
        _C.family_call("scr_normals_map", 1, 1, None, None, 1.0, 1.0, 0.5, 0.5, None, 0.5, None)
    assert own.args is None
    for name in NAMES:
        assert name in _C._FAMILY_NAMES
    assert "scr_bilagrid_slice" in _C._FAMILY_NAMES


@pytest.mark.skipif(torch.cuda.is_available(), reason="replays rejected calls only where nothing can be launched")
def test_c_abi_checks_sizes_and_scalars_first_and_takes_empty_input():
    """Validated before anything is launched; 16 stands for any non-null device address (never dereferenced on the host)."""
    from splatco_amd import _C
    lib, p = _C.lib, 16
    err = lambda: lib.scr_last_error().decode()
    nan, inf = float("nan"), float("inf")

    def fmap(H=4, W=4, D=p, A=p, fx=3.0, fy=3.0, cx=2.0, cy=2.0, min_alpha=0.5, out=p):
        return lib.scr_normals_map(H, W, D, A, fx, fy, cx, cy, None, min_alpha, out, None)

    def bmap(H=4, W=4, D=p, A=p, fx=3.0, fy=3.0, cx=2.0, cy=2.0, min_alpha=0.5, dn=p, dD=p, dA=p):
        return lib.scr_normals_map_backward(H, W, D, A, fx, fy, cx, cy, None, min_alpha, dn, dD, dA, None)

    def floss(H=4, W=4, D=p, A=p, prior=p, mask=p, kind=1, fx=3.0, fy=3.0, cx=2.0, cy=2.0, min_alpha=0.5, scratch=p, out=p):
        return lib.scr_normals_loss_forward(H, W, D, A, prior, mask, kind, fx, fy, cx, cy, min_alpha, scratch, out, None)

    def bloss(H=4, W=4, D=p, A=p, prior=p, mask=p, kind=1, fx=3.0, fy=3.0, cx=2.0, cy=2.0, min_alpha=0.5, g=p, dD=p, dA=p):
        return lib.scr_normals_loss_backward(H, W, D, A, prior, mask, kind, fx, fy, cx, cy, min_alpha, g, dD, dA, None)

    fns = ((fmap, "scr_normals_map"), (bmap, "scr_normals_map_backward"), (floss, "scr_normals_loss_forward"),
           (bloss, "scr_normals_loss_backward"))
    for fn, name in fns:
        for kw, text in ((dict(H=-1), "H = -1"), (dict(W=-3), "W = -3"), (dict(H=65536, W=32768), "2^31"), (dict(H=46341, W=46341), "2^31"),
                         (dict(H=1, W=2 ** 31 - 256), "2^31 - 257"), (dict(H=2 ** 31 - 1, W=1), "2^31 - 257"),
                         (dict(fx=0.0), "fx"), (dict(fy=-1.0), "fy"), (dict(fx=nan), "fx"), (dict(fy=inf), "fy"), (dict(cx=nan), "cx"),
                         (dict(cy=inf), "cy"), (dict(min_alpha=-0.1), "min_alpha"), (dict(min_alpha=nan), "min_alpha"),
                         (dict(min_alpha=inf), "min_alpha")):
            assert fn(**kw) == 1 and err().startswith(name + ":") and text in err(), (name, kw, err())
        # sizes and scalars are checked before the pointers
        assert fn(H=-1, D=None, A=None) == 1 and "H = -1" in err()
        assert fn(fx=0.0, D=None) == 1 and "fx" in err()
        assert fn(D=None) == 1 and err().startswith(name + ":") and "NULL" in err()
        assert fn(A=None) == 1 and "NULL" in err()
        # H W == 0: a no-op, whatever the pointers
        assert fn(H=0, D=None, A=None) == 0 and fn(W=0) == 0 and fn(H=0, W=0) == 0
        # but not whatever the scalars
        assert fn(H=0, fx=nan) == 1 and "fx" in err()
    for fn, name in fns[2:]:
        for kind in (-1, 3):
            assert fn(kind=kind, D=None) == 1 and err().startswith(name + ":") and "mask_kind" in err()
        assert fn(prior=None) == 1 and "NULL" in err()
        assert fn(mask=None) == 1 and "mask is NULL" in err()
        assert fn(mask=None, kind=2) == 1 and "mask is NULL" in err()
    assert fmap(out=None) == 1 and "NULL" in err()
    assert bmap(dn=None) == 1 and "NULL" in err()
    assert floss(scratch=None) == 1 and "NULL" in err()
    assert floss(out=None) == 1 and "NULL" in err()
    assert bloss(g=None) == 1 and "NULL" in err()
    # neither gradient map wanted: nothing to do
    assert bmap(dD=None, dA=None) == 0 and bloss(dD=None, dA=None) == 0


# ------------------------------------------------------------------ the host side
def test_intrinsics_are_the_symmetric_frustum_of_the_projection_matrix():
    from splatco_amd.cameras import get_projection_matrix, look_at_camera
    from splatco_amd.normals import intrinsics
    for W, H, fov in ((70, 52, 60.0), (133, 70, 47.5), (1920, 1080, 90.0)):
        cam = look_at_camera(eye=(0.0, 0.0, 0.0), target=(0.0, 0.0, 1.0), up=(0, -1, 0), FoVx=math.radians(fov), width=W, height=H)
        fx, fy, cx, cy = intrinsics(cam)
        P = get_projection_matrix(cam.znear, cam.zfar, cam.FoVx, cam.FoVy)
        assert float(P[0, 0]) == pytest.approx(2.0 * fx / W, rel=1e-6) and float(P[1, 1]) == pytest.approx(2.0 * fy / H, rel=1e-6)
        assert float(P[0, 2]) == 0.0 and float(P[1, 2]) == 0.0 and (cx, cy) == (W / 2, H / 2)
        assert fx == pytest.approx(fy, rel=1e-12)                       # look_at_camera: square pixels
        assert fx == pytest.approx(ref.intrinsics_fov(H, W, math.radians(fov))[0], rel=1e-15)


SHAPES = [(3, 3), (17, 17), (52, 70), (70, 133), (270, 480)]


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("seed", (0, 1, 2))
def test_recipe_gives_what_was_measured_when_the_gpu_tests_were_specified(H, W, seed):
    """The figures the GPU tests' preconditions and bars were chosen on, re-measured: float32 and float64 give the same valid
    set; 51-62 % of the interior pixels are valid (about 0.9^5: one pixel in ten is below min_alpha), 100 % at 3 x 3; the
    minimum of c.c over the valid pixels is >= 2e-9; the float32 chain's rel-L2 against float64 is 4e-8 .. 1.4e-6 for n and up
    to 3.8e-6 for the map's gradients under a random upstream.  The LOSS gradients of the chain are worse and carry no bound
    here, only a printed figure: the prior lies within 0.3 (U - .5)^3 of n, so projecting it off a float32 n divides n's
    error by that distance (measured: 4e-6 at 17 x 17 to 1.0e-4 at 270 x 480)."""
    D, A, prior, mask, intr = ref.recipe(H, W, seed)
    G = torch.randn(3, H, W, generator=torch.Generator().manual_seed(seed + 10), dtype=torch.float64)
    out = []
    for dtype in (torch.float64, torch.float32):
        D_, A_ = D.clone().requires_grad_(), A.clone().requires_grad_()
        r = ref.normal_loss_ref(D_, A_, prior, intr, mask, dtype=dtype)
        r["dD"], r["dA"] = torch.autograd.grad(r["loss"], (D_, A_), retain_graph=True)
        r["map_dD"], r["map_dA"] = torch.autograd.grad((r["n"] * G.to(dtype)).sum(), (D_, A_))
        out.append(r)
    r64, r32 = out
    assert torch.equal(r64["valid"], r32["valid"]) and torch.equal(r64["good"], r32["good"])
    frac = float(r64["valid"][1:-1, 1:-1].double().mean())
    rel = lambda k: float((r32[k].detach().double() - r64[k].detach()).norm() / r64[k].detach().norm())
    print(f"normals chain {H}x{W} seed {seed}: valid {frac:.3f} of the interior, min c.c {float(r64['cc'][r64['valid']].min()):.2e}, "
          f"rel-L2 n {rel('n'):.2e} map dD {rel('map_dD'):.2e} dA {rel('map_dA'):.2e} loss dD {rel('dD'):.2e} dA {rel('dA'):.2e}")
    assert frac == 1.0 if (H, W) == (3, 3) else 0.51 <= frac <= 0.62, frac
    assert float(r64["cc"][r64["valid"]].min()) >= 2e-9
    assert rel("n") < 1.45e-6                                 # (the lower ends of the ranges are figures, not properties)
    assert rel("map_dD") < 3.85e-6 and rel("map_dA") < 3.85e-6
    assert not r64["dD"][~ref.neighbourhood(r64["valid"])].any() and not r64["n"][:, ~r64["valid"]].any()


def test_three_by_three_has_one_valid_pixel_when_all_nine_are_ok():
    D = torch.full((3, 3), 1.5)
    D[1, 2] = 1.6
    r = ref.normals_ref(D, torch.full((3, 3), 0.75), ref.intrinsics_fov(3, 3))
    assert int(r["valid"].sum()) == 1 and bool(r["valid"][1, 1]) and float(r["n"][:, 1, 1].norm()) == pytest.approx(1.0, abs=1e-15)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 9), (3, 3), (17, 17), (52, 70)])
@pytest.mark.parametrize("mk", (None, "f32", "u8", "bool"))
def test_torch_path_on_cpu_tensors_is_the_float32_restatement_bit_for_bit(H, W, mk):
    from splatco_amd.normals import depth_normals, normal_loss
    D, A, prior, mask, intr = ref.recipe(H, W, 1, mask_kind=mk)
    Da, Aa, Db, Ab = (x.clone().requires_grad_() for x in (D, A, D, A))
    n, valid = depth_normals(Da, Aa, intr, return_valid=True)
    want = ref.normals_ref(Db, Ab, intr, dtype=torch.float32)
    assert n.dtype == torch.float32 and torch.equal(n, want["n"]) and torch.equal(valid, want["valid"])
    loss, stats = normal_loss(Da, Aa, prior, intr, mask, return_stats=True)
    w = ref.normal_loss_ref(Db, Ab, prior, intr, mask, dtype=torch.float32)
    assert loss.dtype == torch.float32 and torch.equal(loss, w["loss"]) and int(stats[0]) == int(w["n_valid"]) and not stats.requires_grad
    ga, gb = torch.autograd.grad(loss, (Da, Aa)), torch.autograd.grad(w["loss"], (Db, Ab))
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])
    if H < 3 or W < 3:
        assert float(loss.detach()) == 0.0 and not n.any() and not valid.any() and not ga[0].any() and not ga[1].any()
    # a prior or a mask that wants a gradient gets one
    p_ = prior.clone().requires_grad_()
    normal_loss(D, A, p_, intr, mask).backward()
    assert p_.grad is not None and (H < 3 or W < 3 or p_.grad.abs().sum() > 0)


@pytest.mark.parametrize("a,b,c", [(2.0, 0.0, 0.0), (3.0, 0.4, -0.25), (1.5, -0.7, 0.6)])
def test_a_plane_in_camera_space_gives_its_analytic_normal(a, b, c):
    """z = a + b x + c y in camera space: the surface z - b x - c y = a has the normal (b, c, -1) / |.| facing the camera.
    Along the ray of pixel (px, py), z = a / (1 - b rx - c ry).  Float64 maps, alpha = 1."""
    from splatco_amd.normals import _normals_torch
    H, W = 21, 29
    intr = (31.0, 27.0, 14.5, 10.5)
    rx = ((torch.arange(W, dtype=torch.float64) + 0.5 - intr[2]) / intr[0])[None, :]
    ry = ((torch.arange(H, dtype=torch.float64) + 0.5 - intr[3]) / intr[1])[:, None]
    z = a / (1.0 - b * rx - c * ry)
    want = torch.tensor([b, c, -1.0], dtype=torch.float64)
    want = want / want.norm()
    for n, valid in (_normals_torch(z, torch.ones_like(z), intr, 0.5),
                     (lambda r: (r["n"], r["valid"]))(ref.normals_ref(z, torch.ones_like(z), intr))):
        assert bool(valid[1:-1, 1:-1].all()) and not valid[0].any() and not valid[:, 0].any() and not valid[-1].any() and not valid[:, -1].any()
        assert float((n[:, 1:-1, 1:-1] - want.reshape(3, 1, 1)).abs().max()) <= 1e-12
        assert not n[:, 0].any() and not n[:, :, -1].any()


def test_world_frame_rotates_by_the_camera_to_world_rotation_and_refuses_one_that_wants_a_gradient():
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.normals import depth_normals, intrinsics
    cam = look_at_camera(eye=(0.0, 0.0, 0.0), target=(1.0, 0.0, 0.0), up=(0, -1, 0), FoVx=math.radians(60), width=9, height=7)
    D = torch.full((7, 9), 2.0)
    A = torch.ones(7, 9)
    n_cam = depth_normals(D, A, cam)
    n_world = depth_normals(D, A, cam, frame="world")
    assert torch.allclose(n_cam[:, 3, 4], torch.tensor([0.0, 0.0, -1.0]), atol=1e-6)
    assert torch.allclose(n_world[:, 3, 4], torch.tensor([-1.0, 0.0, 0.0]), atol=1e-6)     # faces the camera, which looks along +x
    assert torch.equal(depth_normals(D, A, intrinsics(cam)), n_cam)
    with pytest.raises(ValueError, match="world"):
        depth_normals(D, A, intrinsics(cam), frame="world")
    with pytest.raises(ValueError, match="frame"):
        depth_normals(D, A, cam, frame="view")
    cam.world_view_transform = cam.world_view_transform.clone().requires_grad_()
    with pytest.raises(ValueError, match="requires grad"):
        depth_normals(D, A, cam, frame="world")


def test_wrappers_refuse_bad_arguments():
    from splatco_amd.normals import depth_normals, normal_loss
    D, A, prior, mask, intr = ref.recipe(9, 11, 0)
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="min_alpha"):
            depth_normals(D, A, intr, min_alpha=bad)
        with pytest.raises(ValueError, match="min_alpha"):
            normal_loss(D, A, prior, intr, min_alpha=bad)
    with pytest.raises(ValueError, match="alpha"):
        depth_normals(D, A[:8], intr)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        depth_normals(D[None], A[None], intr)
    with pytest.raises(ValueError, match="prior"):
        normal_loss(D, A, prior[:2], intr)
    with pytest.raises(ValueError, match="prior"):
        normal_loss(D, A, prior.to("meta"), intr)
    with pytest.raises(ValueError, match="mask"):
        normal_loss(D, A, prior, intr, mask[:8])
    with pytest.raises(ValueError, match="fx"):
        depth_normals(D, A, (0.0, 1.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="4|fx, fy, cx, cy"):
        depth_normals(D, A, (1.0, 1.0, 0.0))


def test_step_takes_normal_arguments_and_refuses_bad_lists_before_anything_runs():
    from splatco_amd import train_step
    params = inspect.signature(train_step.collaborative_step).parameters
    assert params["normal_targets"].default is None and params["normal_masks"].default is None
    assert params["normal_weight"].default == 0.0 and params["normal_options"].default is None
    views, t = [object(), object()], torch.zeros(3, 4, 4)
    for kw in (dict(), dict(normal_targets=[t]), dict(normal_targets=[t, t], normal_masks=[None])):
        with pytest.raises(ValueError, match="normal_targets|normal_masks"):
            train_step.collaborative_step(None, views, [t, t], None, None, normal_weight=0.1, **kw)
