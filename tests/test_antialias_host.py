"""Antialiased mode, host side (no GPU): the torch restatement of h (tests/antialias_refs.py) against closed forms, the float64
oracle's projection and finite differences; the scenes the GPU tests rely on; the public surface and the C-ABI."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import antialias_refs as A
from util import oracle_settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_pre(cam, g):
    from oracle import raster_oracle as orc
    st = oracle_settings(orc, cam, g["bg"])
    return orc.preprocess(st, g["means3D"], g["scales"], g["rotations"], opacities=g["opacities"],
                          colors_precomp=g["colors"], f64=True)


# ------------------------------------------------------------------ 1. closed form
@pytest.mark.parametrize("s2", [0.3, 1.0, 4.0, 37.5])
def test_isotropic_on_axis_closed_form(s2):
    """One isotropic Gaussian on the optical axis, world sigma at depth z: s^2 = (fx sigma / z)^2, h = s^2 / (s^2 + 0.3)."""
    W = H = 64
    cam, g = A.one_splat(s2, (W / 2.0 - 0.5, H / 2.0 - 0.5), W, H)
    assert abs(float(g["means3D"][0, 0])) < 1e-12 and abs(float(g["means3D"][0, 1])) < 1e-12      # on the axis
    fx = W / (2.0 * float(np.float32(math.tan(cam.FoVx * 0.5))))
    sigma, z = float(g["scales"][0, 0]), float(g["means3D"][0, 2])          # the float32 values the reference reads
    s2_in = (fx * sigma / z) ** 2
    tm = A.aa_terms_scene(cam, g)
    assert abs(s2_in / s2 - 1.0) < 1e-6
    for k in ("a0", "c0"):
        assert abs(float(tm[k][0]) / s2_in - 1.0) < 1e-14, k
    assert abs(float(tm["b"][0])) < 1e-14 * s2_in
    assert abs(float(tm["h"][0]) / (s2_in / (s2_in + 0.3)) - 1.0) < 1e-14


def test_floored_closed_form():
    """s^2 = 1e-4 px^2: r = (s^2 / (s^2 + 0.3))^2 = 1.1e-7 < 0.000025, h = 0.005; and so does a rank-deficient Sigma."""
    cam, g = A.one_splat(1e-4, (31.5, 31.5))
    tm = A.aa_terms_scene(cam, g)
    assert float(tm["r"][0]) < A.FLOOR and bool(tm["on_floor"][0])
    assert float(tm["h"][0]) == math.sqrt(A.FLOOR) and abs(float(tm["h"][0]) - A.H_FLOOR) < 1e-17
    assert float(A.aa_terms_scene(cam, g, dtype=torch.float32)["h"][0]) == float(np.sqrt(np.float32(A.FLOOR)))
    g["scales"][0] = (0.3, 0.0, 0.0)      # a needle along x: det0 = 0 up to rounding, of either sign
    tm = A.aa_terms_scene(cam, g)
    assert abs(float(tm["det0"][0])) < 1e-12 and float(tm["h"][0]) == math.sqrt(A.FLOOR)


# ------------------------------------------------------------------ 2. projection pin
@pytest.mark.parametrize("scene", ["mixed", "wide"])
def test_projection_matches_the_float64_oracle(scene):
    """(a, b, c) of the reference against the inverse of the float64 oracle's conic: two float64 evaluations of one formula."""
    cam, g = A.mixed_scene() if scene == "mixed" else A.wide_scene()
    pre = _oracle_pre(cam, g)
    vis = pre["radii"] > 0
    co = pre["conic_opacity"][vis]
    dq = co[:, 0] * co[:, 2] - co[:, 1] ** 2
    want = dict(a=co[:, 2] / dq, b=-co[:, 1] / dq, c=co[:, 0] / dq)
    tm = A.aa_terms_scene(cam, g)
    for k, w in want.items():
        got = tm[k].numpy()[vis]
        # b passes through zero: relative to the element or to 1e-6 of the tensor's largest, whichever is larger
        err = float((np.abs(got - w) / np.maximum(np.abs(w), 1e-6 * np.abs(w).max())).max())
        assert err <= 1e-9, (k, err)


# ------------------------------------------------------------------ 3. gradients
def test_gradcheck_of_h():
    """Finite differences of the float64 h in means3D, scales, rotations and viewmatrix, away from the floor and the clamp."""
    cam, g = A.mixed_scene()
    with torch.no_grad():
        tm = A.aa_terms_scene(cam, g)
    vis = torch.as_tensor(_oracle_pre(cam, g)["radii"] > 0)
    pick = torch.nonzero(vis & (tm["r"] > 4 * A.FLOOR) & (tm["h"] < 0.95) & ~tm["clx"] & ~tm["cly"]).reshape(-1)[:6]
    assert pick.numel() == 6
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)[pick].clone().requires_grad_()
    m, s, q = t(g["means3D"]), t(g["scales"]), t(g["rotations"])
    V = cam.world_view_transform.double().clone().requires_grad_()
    tf = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    fn = lambda m_, s_, q_, V_: A.aa_terms(m_, V_, cam.image_width, cam.image_height, *tf, scales=s_, rotations=q_)["h"]
    h = fn(m, s, q, V)
    assert float(h.detach().min()) > 2 * A.H_FLOOR and float(h.detach().max()) < 0.95
    assert torch.autograd.gradcheck(fn, (m, s, q, V), eps=1e-6, atol=1e-7, rtol=1e-5)
    # ... and the floor passes nothing
    s0 = (s.detach() * 1e-4).requires_grad_()
    h0 = fn(m, s0, q, V)
    assert bool((h0 == math.sqrt(A.FLOOR)).all())
    assert all(x is None or not x.any() for x in torch.autograd.grad(h0.sum(), (m, s0, q, V), allow_unused=True))


# ------------------------------------------------------------------ 4. scene conditions
def test_scene_conditions():
    cam, g = A.mixed_scene()
    assert cam.image_width % 16 and cam.image_height % 16
    c = A.scene_counts(cam, g, _oracle_pre(cam, g)["radii"] > 0)
    print("[antialias] mixed scene:", c)
    assert c == dict(c, visible=509, floor=137, near_kink=0, near_cut=0, below_cut=143)
    assert c["high"] >= 0.05 and c["mid"] >= 0.30 and c["floor"] >= 100 and c["near_kink"] == 0
    assert abs(c["high"] - 0.067) < 0.001 and abs(c["mid"] - 0.37) < 0.005
    cam, g = A.wide_scene()
    pre = _oracle_pre(cam, g)
    c = A.scene_counts(cam, g, pre["radii"] > 0)
    print("[antialias] wide scene:", c, "largest rect", int(pre["tiles_touched"].max()))
    assert c["visible"] == 403 and c["clamped"] == 60 and int(pre["tiles_touched"].max()) == 35
    assert c["clamped"] >= 30 and int(pre["tiles_touched"].max()) > 32


# ------------------------------------------------------------------ 5. surface
def test_public_surface():
    from splatco_amd import _C
    from splatco_amd.evaluate import evaluate_views
    from splatco_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from splatco_amd.renderer import render
    p = inspect.signature(GaussianRasterizer.forward).parameters
    assert p["antialiased"].default is False and p["return_aux"].default is False
    assert inspect.signature(render).parameters["antialiased"].default is None
    assert inspect.signature(evaluate_views).parameters["antialiased"].default is None
    assert len(GaussianRasterizationSettings._fields) == 12
    assert _C.ABI_VERSION >= 32 and _C.lib.scr_abi_version() == _C.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "splatco_raster.h")).read()
    value = lambda name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, hdr).group(1))
    assert value("SCR_MODE_ANTIALIASED") == _C.MODE_ANTIALIASED == 1
    assert value("SCR_PLAN_ANTIALIASED") == _C.PLAN_ANTIALIASED == 4
    assert not _C.PLAN_ANTIALIASED & (_C.PLAN_NONFINITE_COLOUR | _C.PLAN_LARGE_RECTS)


def test_unknown_mode_bit_is_refused():
    """Before anything is launched: the call fails on a machine without a GPU as it does on one with."""
    from splatco_amd import _C
    plan = (ctypes.c_int64 * 4)(7, 7, 7, 7)
    for mode in (2, 3, 1 << 40, -1):
        rc = _C.lib.scr_forward_plan(mode, 0, 0, *[None] * 7, None, None, None, plan, None)
        assert rc != 0 and "mode" in _C.lib.scr_last_error().decode()
        rc = _C.lib.scr_forward_plan_run(mode, 0, 0, *[None] * 7, None, None, None, plan, None, 0, *[None] * 5)
        assert rc != 0 and "mode" in _C.lib.scr_last_error().decode()
    # a known mode gets as far as the argument checks
    assert _C.lib.scr_forward_plan(_C.MODE_ANTIALIASED, 0, 0, *[None] * 7, None, None, None, plan, None) != 0
    assert "settings" in _C.lib.scr_last_error().decode()
    # one map without the other is refused before anything is launched, whichever of the two is given
    one = ctypes.c_void_p(256)      # never dereferenced: the call fails on the pair
    for maps in ((one, None), (None, one)):
        assert _C.lib.scr_forward_run(0, 0, 0, 0, None, None, None, None, None, *maps, None) != 0
        assert "out_depth / out_alpha" in _C.lib.scr_last_error().decode()
