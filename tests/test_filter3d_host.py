"""Mip-Splatting's 3D smoothing filter, everything that needs no device: the restatement the GPU tests compare against
(tests/filter3d_ref.py) on a case worked by hand and against float64 autograd, splatco_amd.filter3d.pack_cameras against
cameras.make_camera, the C-ABI surface of scr_filter3d_* (include/splatco_raster.h) and Filter3D's staleness rule."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import filter3d_ref as ref
from splatco_amd import filter3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scr_filter3d_distance", "scr_filter3d_apply", "scr_filter3d_apply_backward")
NAN, INF = float("nan"), float("inf")


def identity_camera(tx=1.625, ty=1.0, focal=512.0):
    """The packed row written by hand: R = I, t = 0, so p = x exactly."""
    return torch.tensor([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, tx, ty, focal, 0]], dtype=torch.float32)


def test_restatement_on_a_case_worked_by_hand():
    cam = identity_camera()
    pts = torch.tensor([[0.5, -0.25, 2.0], [0.0, 0.0, -1.0], [NAN, 0.0, 1.0]])
    for dtype in (torch.float64, torch.float32):
        m = ref.sampling_distance(pts, cam, dtype)
        assert m.dtype == dtype and m.tolist() == [2.0 / 512.0, INF, INF]
        f = ref.compute_filter_3d(pts, cam, 0.2, dtype)
        want = math.sqrt(0.2) * 2.0 / 512.0
        # the point behind the camera and the NaN point receive the observed maximum
        assert f.tolist() == pytest.approx([want] * 3, rel=1e-6 if dtype == torch.float32 else 1e-15)
    # a second observed point further away: the unobserved ones get ITS value, the largest
    pts2 = torch.cat([pts, torch.tensor([[0.0, 0.0, 8.0]])])
    f = ref.compute_filter_3d(pts2, cam)
    assert f.tolist() == pytest.approx([math.sqrt(0.2) * z / 512.0 for z in (2.0, 8.0, 8.0, 8.0)], rel=1e-15)
    # nothing observed: every value is 0
    assert ref.compute_filter_3d(pts[1:], cam).tolist() == [0.0, 0.0]
    # inclusive bounds, strict depth test
    edge = torch.tensor([[1.625, 0.0, 1.0], [0.0, 1.0, 1.0], [0.0, 0.0, np.float32(0.2)], [np.nextafter(np.float32(1.625), np.float32(2)), 0.0, 1.0]])
    assert torch.isfinite(ref.sampling_distance(edge, cam)).tolist() == [True, True, False, False]
    # the minimum over two cameras takes each camera's own focal length
    two = torch.cat([cam, identity_camera(focal=128.0)])
    assert ref.sampling_distance(pts[:1], two).tolist() == [2.0 / 512.0]
    assert ref.sampling_distance(pts[:1], two.flip(0)).tolist() == [2.0 / 512.0]


def test_restatement_equals_upstreams_loop_for_equal_focal_lengths():
    g = torch.Generator().manual_seed(3)
    pts = (torch.rand(400, 3, generator=g, dtype=torch.float64) * 2 - 1) * 1.5
    cams = scene_cameras(9, seed=5, focal=(80.0, 80.0)).double()
    ours = ref.compute_filter_3d(pts, cams, 0.2, torch.float64)
    theirs = ref.upstream_loop(pts, cams, 0.2)
    assert bool(torch.isfinite(ref.sampling_distance(pts, cams)).any())
    assert torch.allclose(ours, theirs, rtol=1e-12, atol=0)


def scene_cameras(C, seed, focal=(40.0, 120.0), width=64, height=48):
    """C cameras on a shell of radius 2.5 - 5 looking at the origin, focal length `focal` px at width x height, packed."""
    from splatco_amd.cameras import look_at_camera
    rng = np.random.default_rng(seed)
    views = []
    for i in range(C):
        d = rng.standard_normal(3)
        eye = d / np.linalg.norm(d) * rng.uniform(2.5, 5.0)
        up = np.array([0.0, -1.0, 0.0]) if abs(eye[1]) < 0.9 * np.linalg.norm(eye) else np.array([1.0, 0.0, 0.0])
        fx = rng.uniform(*focal)
        views.append(look_at_camera(eye, (0.0, 0.0, 0.0), up, 2.0 * math.atan(width / (2.0 * fx)), width, height, uid=i))
    return filter3d.pack_cameras(views)


def test_pack_cameras_follows_make_camera():
    from splatco_amd.cameras import look_at_camera, make_camera
    cam = look_at_camera((1.0, -2.0, -4.0), (0.2, 0.1, 0.0), (0.0, -1.0, 0.0), math.radians(50.0), 64, 48)
    wide = make_camera(np.eye(3), np.array([0.1, -0.2, 0.3]), math.radians(40.0), math.radians(70.0), 32, 80)
    packed = filter3d.pack_cameras([cam, wide])
    assert packed.shape == (2, 16) and packed.dtype == torch.float32 and packed.is_contiguous()
    x = torch.tensor([[0.3, -0.7, 1.1], [2.0, 0.5, -0.4]], dtype=torch.float64)
    for row, v in zip(packed.double(), (cam, wide)):
        Rt = row[:12].reshape(3, 4)
        want = (torch.cat([x, torch.ones(2, 1, dtype=torch.float64)], dim=1) @ v.world_view_transform.double())[:, :3]
        assert torch.allclose(x @ Rt[:, :3].T + Rt[:, 3], want, rtol=0, atol=1e-6)
        tanx, tany = math.tan(v.FoVx / 2), math.tan(v.FoVy / 2)
        fx, fy = v.image_width / (2 * tanx), v.image_height / (2 * tany)
        assert float(row[12]) == pytest.approx(1.3 * tanx, rel=1e-7) and float(row[12]) == pytest.approx(0.65 * v.image_width / fx, rel=1e-7)
        assert float(row[13]) == pytest.approx(1.3 * tany, rel=1e-7)
        assert float(row[14]) == pytest.approx(max(fx, fy), rel=1e-7) and float(row[15]) == 0.0
    assert float(packed[1, 14]) == pytest.approx(80 / (2 * math.tan(math.radians(35.0))), rel=1e-7)     # fy > fx there: the larger
    bad = types.SimpleNamespace(world_view_transform=cam.world_view_transform.clone(), FoVx=cam.FoVx, FoVy=cam.FoVy,
                                image_width=64, image_height=48)
    bad.world_view_transform[3, 1] = NAN
    with pytest.raises(ValueError, match="camera 1"):
        filter3d.pack_cameras([cam, bad])
    bad.world_view_transform[3, 1] = 0.0
    bad.FoVy = INF
    with pytest.raises(ValueError, match="non-finite"):
        filter3d.pack_cameras([bad])
    with pytest.raises(ValueError):
        filter3d.pack_cameras([])


def test_backward_formulas_against_float64_autograd():
    g = torch.Generator().manual_seed(11)
    P = 500
    lu = lambda lo, hi, *s: torch.exp(torch.rand(*s, generator=g, dtype=torch.float64) * (math.log(hi) - math.log(lo)) + math.log(lo))
    s, o = lu(1e-4, 10.0, P, 3).requires_grad_(), torch.rand(P, 1, generator=g, dtype=torch.float64).requires_grad_()
    f = lu(1e-4, 100.0, P)
    f[::4] = 0.0
    gs, go = torch.randn(P, 3, generator=g, dtype=torch.float64), torch.randn(P, 1, generator=g, dtype=torch.float64)
    s2, o2 = ref.apply(s, o, f)
    assert torch.equal(s2[::4], s[::4]) and torch.equal(o2[::4], o[::4])            # f == 0 passes through
    on = f != 0
    assert bool((s2[on] > s[on]).all()) and bool((o2[on] < o[on]).all())
    for gs_, go_ in ((gs, go), (gs, None), (None, go)):
        loss = (0 if gs_ is None else (s2 * gs_).sum()) + (0 if go_ is None else (o2 * go_).sum())
        ds, do = torch.autograd.grad(loss, (s, o), retain_graph=True, allow_unused=True)
        ds = torch.zeros_like(s) if ds is None else ds
        do = torch.zeros_like(o) if do is None else do
        ds_f, do_f = ref.apply_backward(s, o, f, gs_, go_)
        assert float((ds_f - ds).abs().max() / ds.abs().max().clamp_min(1e-300)) < 1e-13
        assert float((do_f - do).abs().max() / do.abs().max().clamp_min(1e-300)) < 1e-13
        if go_ is None:
            assert torch.equal(do_f, torch.zeros_like(do_f))
    # the ratio form survives where the product of the squares underflows
    tiny = torch.full((1, 3), 1e-12, dtype=torch.float32)
    s3, o3 = ref.apply(tiny, torch.ones(1, 1), torch.ones(1), torch.float32)
    assert bool(torch.isfinite(s3).all()) and 0.0 <= float(o3) < 1e-30


def test_binding_and_header_declare_the_three_entry_points_at_abi_37():
    from splatco_amd import _C
    hdr = open(os.path.join(ROOT, "include", "splatco_raster.h")).read()
    assert _C.ABI_VERSION >= 37 and _C.lib.scr_abi_version() == _C.ABI_VERSION
    assert f"#define SCR_ABI_VERSION {_C.ABI_VERSION}" in hdr
    sig = {s[0]: s for s in _C.SIGNATURES}
    for name in NAMES:
        assert hasattr(_C.lib, name) and name in _C.SYMBOLS and re.search(rf"\bint {name}\s*\(", hdr), name
        assert sig[name][1] is _C.i32 and sig[name][-1] is _C.vp                   # a status; the stream last
    i = _C.SYMBOLS.index(NAMES[0])
    assert _C.SYMBOLS[i:i + 3] == list(NAMES)
    assert sig[NAMES[0]][2:] == (_C.i64, _C.vp, _C.i32, _C.vp, _C.vp, _C.vp)
    assert len(sig[NAMES[1]]) - 2 == 10 and len(sig[NAMES[2]]) - 2 == 12
    assert sig[NAMES[1]][2:5] == sig[NAMES[2]][2:5] == (_C.i64, _C.i32, _C.i64)


def test_c_abi_checks_sizes_first_and_takes_empty_input():
    """Validated before anything is launched; 16 stands for any non-null device address (never dereferenced on the host)."""
    from splatco_amd import _C
    lib, p = _C.lib, 16
    err = lambda: lib.scr_last_error().decode()
    assert lib.scr_filter3d_distance(0, None, 1, None, None, None) == 0            # N == 0: a no-op, whatever the pointers
    assert lib.scr_filter3d_distance(5, p, 0, p, p, None) == 1 and "C = 0" in err()
    assert lib.scr_filter3d_distance(-1, p, 1, p, p, None) == 1 and "N = -1" in err()
    assert lib.scr_filter3d_distance(5, p, 1, None, p, None) == 1 and "NULL" in err()
    for name in NAMES[1:]:
        fn = getattr(lib, name)
        tail = (None,) * (len(fn.argtypes) - 3)
        assert fn(0, 10, 0, *tail) == 0 and fn(7, 10, 0, *tail) == 0               # P == 0: a no-op
        assert fn(7, 0, 0, *tail) == 1 and "k = 0" in err()
        assert fn(7, 10, 71, *tail) == 1 and "P = 71" in err()
        assert fn(2 ** 31 // 10 + 1, 10, 0, *tail) == 1 and "2^31" in err()
        assert fn(7, 10, 3, *tail) == 1 and "NULL" in err()


def test_rejection_table_holds_the_first_recorded_table_and_adds_only_the_new_entry_points():
    """tests/golden/capi_rejections.json stays as it was recorded at ABI 36; the table tests/test_capi_rejections_host.py
    replays (tools/make_golden_rejections.py OUT) holds every one of its rows, unchanged and in order, plus rows of
    scr_filter3d_* only."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_rejections as gen
    assert os.path.basename(gen.BASE) == "capi_rejections.json" and gen.OUT != gen.BASE
    with open(gen.BASE) as f:
        base = json.load(f)
    with open(gen.OUT) as f:
        table = json.load(f)
    assert len(base) == 303
    new = gen.added_rows(base, table)
    assert {r["name"] for r in new} == set(NAMES) and len(new) == 15
    assert all(r["rc"] == 1 and r["error"].startswith(r["name"] + ":") for r in new)
    assert not {r["name"] for r in base} & set(NAMES)
    with pytest.raises(AssertionError):
        gen.added_rows(base, table[1:])
    with pytest.raises(AssertionError):
        gen.added_rows(base, [dict(table[0], error="reworded")] + table[1:])


def test_filter3d_stale_follows_a_replacement_of_the_anchor_parameter(monkeypatch):
    monkeypatch.setattr(filter3d, "compute_filter_3d", lambda points, cameras, variance=0.2: ref.compute_filter_3d(points, cameras, variance, torch.float32))
    pc = types.SimpleNamespace(_anchor=torch.nn.Parameter(torch.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, 4.0], [0.0, 0.0, -1.0]])))
    pc.get_anchor = pc._anchor
    flt = filter3d.Filter3D(identity_camera(), variance=0.2, every=100)
    assert flt.stale(pc) and flt.due(pc) and flt.values is None
    with pytest.raises(ValueError, match="update"):
        filter3d.anchor_values(flt, pc)
    values = flt.update(pc)
    assert values.tolist() == pytest.approx([math.sqrt(0.2) * z / 512 for z in (2.0, 4.0, 4.0)], rel=1e-6)
    assert not flt.stale(pc) and filter3d.anchor_values(flt, pc) is values
    assert not flt.due(pc, 7) and flt.due(pc, 200) and not flt.due(pc)
    with torch.no_grad():
        pc._anchor.add_(0.0)                                   # an optimizer step: the same parameter
    assert not flt.stale(pc)
    # the same N, other rows: a length check alone would pass
    pc._anchor = torch.nn.Parameter(pc._anchor.detach().flip(0).contiguous())
    pc.get_anchor = pc._anchor
    assert flt.stale(pc) and flt.due(pc, 7)
    with pytest.raises(ValueError, match="stale"):
        filter3d.anchor_values(flt, pc)
    assert flt.update(pc).tolist() == pytest.approx([math.sqrt(0.2) * z / 512 for z in (4.0, 4.0, 2.0)], rel=1e-6)
    assert not flt.stale(pc)
    # the model's own sort_anchors keeps the parameter object and gives it new memory
    pc._anchor.data = pc._anchor.data.flip(0).contiguous()
    assert flt.stale(pc)
    # a plain tensor: the length and the device are what can be checked
    assert filter3d.anchor_values(torch.ones(3), pc).shape == (3,)
    with pytest.raises(ValueError, match="compute_filter_3d"):
        filter3d.anchor_values(torch.ones(4), pc)
    with pytest.raises(TypeError):
        filter3d.anchor_values([1.0, 2.0, 3.0], pc)


def test_public_calls_take_filter_3d_and_default_to_none():
    import inspect
    from splatco_amd import evaluate, renderer, train_step
    for fn in (renderer.generate_neural_gaussians, renderer.render, evaluate.render_views, evaluate.evaluate_views,
               train_step.collaborative_step):
        assert inspect.signature(fn).parameters["filter_3d"].default is None, fn.__name__
