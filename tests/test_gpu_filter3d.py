"""Mip-Splatting's 3D smoothing filter on the GPU (csrc/filter3d.hip, splatco_amd/filter3d.py) against the restatement of
its definition (tests/filter3d_ref.py): the sampling distance on its exact boundaries and on a random scene, the fused apply
step forward and backward, and the filter through render(), evaluate_views() and collaborative_step().

The bar is the project's: max(2e-5, 1.5 e_chain) (f64_refs.bar), e_chain = the float32 restatement's own error against the
float64 one in the same process.  Every case prints its figures before it asserts.

Chunk sizes.  The sampling-distance kernel reads the cameras as wave-uniform data, one 64-byte row per loop pass: it has NO
camera chunks, so there is no chunk size to test both sides of.  The loop asks for row min(c + 1, C - 1) ahead of pass c;
C = 1 and C = 2 are the sizes at which that clamp acts on the first pass.  The apply kernels run one candidate per lane in
workgroups of 256: the (V, k) list covers candidate counts of 0, 1, 10, 65, 70 and 3000."""
import math
import types

import numpy as np
import pytest
import torch

import filter3d_ref as ref
import poison
from f64_refs import bar, err
from test_filter3d_host import identity_camera, scene_cameras
from splatco_amd import filter3d

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN, INF = float("nan"), float("inf")
f32 = np.float32
up = lambda v, to=INF: np.nextafter(f32(v), f32(to))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------------- sampling distance
def test_sampling_distance_sits_on_the_exact_boundaries():
    cam = identity_camera(1.625, 1.0, 512.0).to(DEV)
    rows = [((0.0, 0.0, f32(0.2)), False), ((0.0, 0.0, up(0.2)), True),
            ((1.625, 0.0, 1.0), True), ((up(1.625), 0.0, 1.0), False), ((-1.625, 0.0, 1.0), True), ((-up(1.625), 0.0, 1.0), False),
            ((0.0, 1.0, 1.0), True), ((0.0, up(1.0), 1.0), False), ((0.0, -1.0, 1.0), True), ((0.0, -up(1.0), 1.0), False),
            ((NAN, 0.0, 1.0), False), ((0.0, NAN, 1.0), False), ((0.0, 0.0, NAN), False),
            ((INF, 0.0, 1.0), False), ((0.0, -INF, 1.0), False), ((0.0, 0.0, INF), False), ((0.0, 0.0, -INF), False),
            ((0.3, -0.2, 3.0), True), ((0.0, 0.0, -1.0), False), ((0.0, 0.0, 1e30), True)]
    pts = torch.tensor(np.array([r[0] for r in rows], dtype=f32), device=DEV)
    m = filter3d.sampling_distance(pts, cam).cpu()
    want = torch.tensor([float(f32(r[0][2]) / f32(512.0)) if r[1] else INF for r in rows], dtype=torch.float32)
    print("boundaries:", [(r[0], float(v)) for r, v in zip(rows, m)])
    assert torch.equal(torch.isfinite(m), torch.tensor([r[1] for r in rows]))
    assert torch.equal(bits(m), bits(want))                      # z / 512 bit for bit
    # the float64 restatement takes the same decisions on these inputs
    assert torch.equal(torch.isfinite(ref.sampling_distance(pts, cam)), torch.isfinite(m))


def scene_points(N, seed, behind=None):
    """N points in the [-1.5, 1.5]^3 box the cameras look at; with `behind` (a packed camera row) the second half is moved
    behind that camera."""
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(N, 3, generator=g) * 2 - 1) * 1.5
    if behind is not None and N > 1:
        Rt = behind[:12].reshape(3, 4)
        eye = -Rt[:, :3].T @ Rt[:, 3]
        pts[N // 2:] = eye + (eye / eye.norm()) * (0.5 + pts[N // 2:, :1].abs()) + 0.1 * pts[N // 2:]
    return pts


@pytest.fixture(scope="module")
def distance_chain_error():
    """e_chain of the sampling distance: the float32 restatement against the float64 one at N = 1000, C = 65."""
    pts, cams = scene_points(1000, 1), scene_cameras(65, 2)
    m64, m32 = ref.sampling_distance(pts, cams), ref.sampling_distance(pts, cams, torch.float32)
    both = torch.isfinite(m64) & torch.isfinite(m32)
    return err(m32[both], m64[both])


@pytest.mark.parametrize("C", [1, 2, 3, 63, 64, 65, 130])
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 1000])
def test_sampling_distance_random_scene(N, C, distance_chain_error):
    cams = scene_cameras(C, seed=100 + C)
    pts = scene_points(N, seed=7 * N + C, behind=cams[0] if C == 1 else None)
    m = filter3d.sampling_distance(pts.to(DEV), cams.to(DEV))
    assert m.shape == (N,) and m.dtype == torch.float32
    if N == 0:
        return
    seen, _, margin = ref.decisions(pts, cams)
    keep = ~((margin < 1e-4).any(dim=1))
    m64 = ref.sampling_distance(pts, cams)
    got = m.cpu()
    left_out = int((~keep).sum())
    e = err(got[keep & torch.isfinite(m64)], m64[keep & torch.isfinite(m64)]) if bool((keep & torch.isfinite(m64)).any()) else 0.0
    print(f"distance N={N} C={C}: observed {int(torch.isfinite(m64).sum())}, left out {left_out}, err {e:.3g}, "
          f"e_chain {distance_chain_error:.3g}, bar {bar(distance_chain_error):.3g}")
    assert left_out <= 0.05 * N
    assert torch.equal(torch.isfinite(got)[keep], torch.isfinite(m64)[keep])
    assert bool(((got == INF) | torch.isfinite(got)).all())
    if C == 1 and N >= 63:
        assert int((~torch.isfinite(m64)).sum()) >= N // 2        # half of the points lie behind the only camera
        assert bool(torch.isfinite(m64).any())
    assert e <= bar(distance_chain_error)
    # a minimum has no order: the same bits for permuted cameras, and on a second run
    perm = torch.randperm(C, generator=torch.Generator().manual_seed(C))
    assert torch.equal(bits(filter3d.sampling_distance(pts.to(DEV), cams[perm].to(DEV))), bits(m))
    assert torch.equal(bits(filter3d.sampling_distance(pts.to(DEV), cams.to(DEV))), bits(m))


def test_compute_filter_3d_fills_unobserved_points_and_survives_poison():
    cams = scene_cameras(1, seed=101)
    pts = scene_points(1000, seed=5, behind=cams[0])
    pts[3] = NAN
    dpts, dcams = pts.to(DEV), cams.to(DEV)
    rep = poison.check(lambda: [filter3d.compute_filter_3d(dpts, dcams), filter3d.sampling_distance(dpts, dcams)[:3]],
                       sync=torch.cuda.synchronize)
    f = rep["outputs"][0].cpu()
    f64 = ref.compute_filter_3d(pts, cams)
    seen = torch.isfinite(ref.sampling_distance(pts, cams))
    assert 0 < int(seen.sum()) < 1000 and not bool(seen[3])
    assert err(f, f64) <= 2e-5 and bool((f[~seen] == f[seen].max()).all())
    assert float(filter3d.compute_filter_3d(dpts, dcams, variance=0.8)[0]) == pytest.approx(2.0 * float(f[0]), rel=1e-6)
    # nothing observed: every value is 0
    away = pts[~seen][:10].clone()
    assert torch.equal(filter3d.compute_filter_3d(away.to(DEV), dcams).cpu(), torch.zeros(away.shape[0]))
    assert filter3d.compute_filter_3d(dpts[:0], dcams).shape == (0,)
    with pytest.raises(ValueError):
        filter3d.sampling_distance(dpts, dcams[:, :12])
    with pytest.raises(ValueError):
        filter3d.sampling_distance(dpts[:, :2], dcams)


# ------------------------------------------------------------------------------------------------------------------ apply
def log_uniform(g, lo, hi, *shape):
    return torch.exp(torch.rand(*shape, generator=g) * (math.log(hi) - math.log(lo)) + math.log(lo))


def apply_case(V, k, mask_kind, seed):
    """Inputs on the host: mask [V k] bool, scaling [P,3], opacity [P,1], row_filter [V] (a quarter exactly 0), upstream
    gradients."""
    g = torch.Generator().manual_seed(seed)
    n = V * k
    mask = {"all": torch.ones(n, dtype=torch.bool), "none": torch.zeros(n, dtype=torch.bool),
            "random": torch.rand(n, generator=g) < 0.6}[mask_kind]
    P = int(mask.sum())
    s, o = log_uniform(g, 1e-4, 10.0, P, 3), torch.rand(P, 1, generator=g)
    f = log_uniform(g, 1e-4, 100.0, V)
    f[torch.rand(V, generator=g) < 0.25] = 0.0
    if V >= 4:
        f[::4] = 0.0
    return mask, s, o, f, torch.randn(P, 3, generator=g), torch.randn(P, 1, generator=g)


def device_mask(mask, with_index):
    """expand_compact's mask: the bool tensor carrying its compaction index (or not: apply_filter_3d then forms it)."""
    m = mask.to(DEV)
    if with_index:
        m._scr_out_index = torch.where(m, torch.cumsum(m, 0) - 1, -1).to(torch.int32)
    return m


def run_apply(mask, s, o, f, gs, go, k, with_index=True):
    sd, od = s.to(DEV).requires_grad_(), o.to(DEV).requires_grad_()
    s2, o2 = filter3d.apply_filter_3d(sd, od, f.to(DEV), device_mask(mask, with_index), k)
    loss = (0 if gs is None else (s2 * gs.to(DEV)).sum()) + (0 if go is None else (o2 * go.to(DEV)).sum())
    ds, do = torch.autograd.grad(loss, (sd, od), allow_unused=True) if (gs is not None or go is not None) else (None, None)
    return s2.detach(), o2.detach(), ds, do


@pytest.mark.parametrize("mask_kind", ["all", "none", "random"])
@pytest.mark.parametrize("V,k", [(0, 10), (1, 1), (1, 10), (7, 10), (13, 5), (300, 10)])
def test_apply_forward_and_backward(V, k, mask_kind):
    mask, s, o, f, gs, go = apply_case(V, k, mask_kind, seed=31 * V + k)
    P = s.shape[0]
    fg = f[ref.row_of_gaussian(mask, k)]
    s2, o2, ds, do = run_apply(mask, s, o, f, gs, go, k)
    assert s2.shape == (P, 3) and o2.shape == (P, 1) and ds.shape == (P, 3) and do.shape == (P, 1)
    if P == 0:
        return
    want = ref.apply(s, o, fg) + ref.apply_backward(s, o, fg, gs, go)
    chain = ref.apply(s, o, fg, torch.float32) + ref.apply_backward(s, o, fg, gs, go, torch.float32)
    for name, got, w, c in zip(("scaling", "opacity", "d_scaling", "d_opacity"), (s2, o2, ds, do), want, chain):
        e, e_chain = err(got, w, rows=True), err(c, w, rows=True)
        print(f"apply V={V} k={k} {mask_kind} P={P} {name}: err {e:.3g}, e_chain {e_chain:.3g}, bar {bar(e_chain):.3g}")
        assert e <= bar(e_chain), name
    off = fg == 0
    if bool(off.any()):                                           # f == 0: the inputs' bits, forward and backward
        for got, given in ((s2, s), (o2, o), (ds, gs), (do, go)):
            assert torch.equal(bits(got.cpu()[off]), bits(given[off]))
    on = ~off
    # (not strictly: a filter far below a scale vanishes in the rounding of s^2 + f^2)
    assert bool((s2.cpu()[on] >= s[on]).all()) and bool((o2.cpu()[on] <= o[on]).all()) and bool((o2 >= 0).all())
    # each upstream gradient missing in turn: it counts as zero
    for gs_, go_ in ((gs, None), (None, go)):
        _, _, ds1, do1 = run_apply(mask, s, o, f, gs_, go_, k)
        w_ds, w_do = ref.apply_backward(s, o, fg, gs_, go_)
        c_ds, c_do = ref.apply_backward(s, o, fg, gs_, go_, torch.float32)
        assert err(ds1, w_ds, rows=True) <= bar(err(c_ds, w_ds, rows=True))
        if go_ is None:
            assert do1 is None or torch.equal(do1.cpu(), torch.zeros(P, 1))
        else:
            assert err(do1, w_do, rows=True) <= bar(err(c_do, w_do, rows=True))
    # the same bits on a second run, and with the index formed from the mask in torch
    for with_index in (True, False):
        again = run_apply(mask, s, o, f, gs, go, k, with_index)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again, (s2, o2, ds, do)))


def test_apply_with_a_tiny_scale_next_to_a_unit_filter():
    """sqrt(prod s^2 / prod t^2) underflows here (prod s^2 = 1e-72); the ratio form does not."""
    mask = torch.ones(4, dtype=torch.bool)
    s = torch.tensor([[1e-12, 1e-12, 1e-12], [1e-12, 0.5, 2.0], [3.0, 1e-12, 1e-12], [1e-12, 1e-12, 1e-12]])
    o = torch.tensor([[0.9], [0.5], [1.0], [0.0]])
    f = torch.tensor([1.0, 1.0])
    s2, o2, ds, do = run_apply(mask, s, o, f, torch.ones(4, 3), torch.ones(4, 1), 2)
    print("tiny scale:", s2.tolist(), o2.tolist(), ds.tolist(), do.tolist())
    for t in (s2, o2, ds, do):
        assert bool(torch.isfinite(t).all())
    assert bool((o2 >= 0).all()) and float(o2[1]) > 0
    fg = f[ref.row_of_gaussian(mask, 2)]
    want = ref.apply(s, o, fg) + ref.apply_backward(s, o, fg, torch.ones(4, 3), torch.ones(4, 1))
    for got, w in zip((s2, o2, ds, do), want):
        assert err(got, w, rows=True, row_floor=1e-30) <= 2e-5


def test_apply_does_not_depend_on_fresh_memory():
    mask, s, o, f, gs, go = apply_case(300, 10, "random", seed=77)
    dmask = device_mask(mask, True)
    sd, od, fd, gsd, god = (t.to(DEV) for t in (s, o, f, gs, go))

    def fn():
        a, b = sd.clone().requires_grad_(), od.clone().requires_grad_()
        s2, o2 = filter3d.apply_filter_3d(a, b, fd, dmask, 10)
        ((s2 * gsd).sum() + (o2 * god).sum()).backward()
        return [s2, o2, a.grad, b.grad]

    rep = poison.check(fn, sync=torch.cuda.synchronize)
    assert rep["nan"].count >= 4                                 # two outputs and two gradients are fresh memory
    with pytest.raises(ValueError):
        filter3d.apply_filter_3d(sd, od, fd[:-1], dmask, 10)


# --------------------------------------------------------------------------------------------------------- through render
PIPE = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
W, H = 64, 48


@pytest.fixture(scope="module")
def scene():
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.renderer import prefilter_voxel
    from splatco_amd.synthetic import synthetic_anchor_model
    pc = synthetic_anchor_model(300, 3, DEV, plane_size=64)
    cam = look_at_camera((0.4, -0.3, -6.0), (0.0, 0.0, 0.0), (0.0, -1.0, 0.0), math.radians(60.0), W, H).to(DEV)
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    vis = prefilter_voxel(cam, pc, PIPE, bg)
    vis = vis & (torch.rand(300, generator=torch.Generator().manual_seed(1)) < 0.8).to(DEV)      # drops some anchors
    assert 50 < int(vis.sum()) < 300
    weights = torch.rand(3, H, W, generator=torch.Generator().manual_seed(2)).to(DEV)
    return pc, cam, bg, vis, weights


def params_of(pc):
    return [(n, p) for n, p in pc.named_parameters() if p.requires_grad]


def render_and_grads(scene, **kw):
    from splatco_amd.renderer import render
    pc, cam, bg, vis, weights = scene
    for _, p in params_of(pc):
        p.grad = None
    res = render(cam, pc, PIPE, bg, visible_mask=vis.clone(), **kw)
    ((res["render"] * weights).sum() + res["scaling"].prod(dim=1).mean()).backward()
    return res, {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in params_of(pc)}


def same_grads(a, b):
    return a.keys() == b.keys() and all((a[n] is None) == (b[n] is None) and (a[n] is None or torch.equal(bits(a[n]), bits(b[n])))
                                        for n in a)


def test_render_without_a_filter_and_with_an_all_zero_filter_are_the_same_bits(scene):
    pc = scene[0]
    plain, g_plain = render_and_grads(scene)
    zero, g_zero = render_and_grads(scene, filter_3d=torch.zeros(300, device=DEV))
    assert torch.equal(bits(plain["render"]), bits(zero["render"])) and torch.equal(plain["radii"], zero["radii"])
    assert int((plain["radii"] > 0).sum()) > 100
    assert same_grads(g_plain, g_zero) and g_plain["_scaling"] is not None and float(g_plain["_scaling"].abs().sum()) > 0
    assert torch.equal(bits(plain["scaling"]), bits(zero["scaling"]))


def test_render_with_a_filter_equals_the_steps_by_hand(scene):
    from splatco_amd.expand import visible_indices
    from splatco_amd.rasterizer import GaussianRasterizer
    from splatco_amd.renderer import _settings, generate_neural_gaussians
    pc, cam, bg, vis, weights = scene
    flt = torch.zeros(300, device=DEV)
    flt[torch.randperm(300, generator=torch.Generator().manual_seed(4))[:150].to(DEV)] = 0.3      # large on half of the anchors
    plain, _ = render_and_grads(scene)
    res, grads = render_and_grads(scene, filter_3d=flt)
    assert not torch.equal(res["render"], plain["render"])
    assert float((res["render"] - plain["render"]).detach().abs().max()) > 1e-3
    # res["scaling"] is what the heads produced, not what the rasterizer got; the regulariser's tap stays attached
    assert torch.equal(bits(res["scaling"]), bits(plain["scaling"]))
    assert hasattr(res["scaling"], "_scr_reg_tap") == hasattr(plain["scaling"], "_scr_reg_tap")
    # the gradient reaches the MLP heads and the anchors' scaling
    for name in ("_scaling", "mlp_cov.0.weight", "mlp_opacity.0.weight"):
        assert grads[name] is not None and float(grads[name].abs().sum()) > 0, name
    # by hand: the neural Gaussians, the filter on the rows of the visible anchors, the rasterizer
    for _, p in params_of(pc):
        p.grad = None
    mask_in = vis.clone()
    xyz, color, opacity, scaling, rot, neural_opacity, mask = generate_neural_gaussians(cam, pc, mask_in, is_training=True)
    row_filter = flt[visible_indices(mask_in)]
    assert 0 < int((row_filter > 0).sum()) < row_filter.shape[0]
    s2, o2 = filter3d.apply_filter_3d(scaling, opacity, row_filter, mask, pc.n_offsets)
    means2D = torch.zeros_like(xyz, requires_grad=True)
    image, radii = GaussianRasterizer(raster_settings=_settings(cam, bg, 1.0, False))(
        means3D=xyz, means2D=means2D, shs=None, colors_precomp=color, opacities=o2, scales=s2, rotations=rot, cov3D_precomp=None)
    assert torch.equal(bits(image), bits(res["render"])) and torch.equal(radii, res["radii"])
    ((image * weights).sum() + scaling.prod(dim=1).mean()).backward()
    by_hand = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in params_of(pc)}
    assert same_grads(grads, by_hand)
    # filter rows that did NOT follow the visible-anchor index give another image
    wrong, _ = render_and_grads(scene, filter_3d=flt.flip(0))
    assert not torch.equal(wrong["render"], res["render"])
    # it combines with aux and the antialiased mode
    both, _ = render_and_grads(scene, filter_3d=flt, aux=True, antialiased=True)
    assert both["depth"].shape == (H, W) and bool(torch.isfinite(both["render"]).all())
    assert not torch.equal(both["render"], res["render"])


def test_render_refuses_a_wrong_tensor_and_a_stale_filter(scene):
    from splatco_amd.densify import AnchorDensifier
    from splatco_amd.renderer import render
    from splatco_amd.synthetic import synthetic_anchor_model
    _, cam, bg, _, _ = scene
    pc = synthetic_anchor_model(300, 3, DEV, plane_size=64)
    with pytest.raises(ValueError, match="300 anchors"):
        render(cam, pc, PIPE, bg, filter_3d=torch.zeros(299, device=DEV))
    with pytest.raises(ValueError, match="compute_filter_3d"):
        render(cam, pc, PIPE, bg, filter_3d=torch.zeros(300))
    flt = filter3d.Filter3D([cam], every=10)
    with pytest.raises(ValueError, match="update"):
        render(cam, pc, PIPE, bg, filter_3d=flt)
    flt.update(pc)
    first = render(cam, pc, PIPE, bg, filter_3d=flt)["render"]
    assert torch.equal(bits(first), bits(render(cam, pc, PIPE, bg, filter_3d=flt.values)["render"]))
    opt = torch.optim.Adam([{"params": [getattr(pc, "_" + n)], "lr": 1e-3, "name": n} for n in ("anchor", "offset", "anchor_feat", "scaling")])
    AnchorDensifier(pc, opt, voxel_size=0.01).sort_anchors()       # the same N, other rows
    assert pc.get_anchor.shape[0] == 300 and flt.stale(pc)
    with pytest.raises(ValueError, match="stale"):
        render(cam, pc, PIPE, bg, filter_3d=flt)
    flt.update(pc)
    again = render(cam, pc, PIPE, bg, filter_3d=flt)["render"]
    assert float((again - first).detach().abs().max()) < 1e-4              # a relabelling: the same picture


def test_evaluate_views_and_collaborative_step_take_the_filter():
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.evaluate import evaluate_views, render_views
    from splatco_amd.synthetic import synthetic_anchor_model
    from splatco_amd.train_step import collaborative_step
    pc = synthetic_anchor_model(300, 3, DEV, plane_size=64)
    cams = [look_at_camera((0.4 + 0.5 * i, -0.3, -6.0), (0.0, 0.0, 0.0), (0.0, -1.0, 0.0), math.radians(60.0), W, H, uid=i).to(DEV)
            for i in range(2)]
    bg = torch.ones(3, device=DEV)
    flt = filter3d.Filter3D(cams, variance=0.2, every=100)
    flt.update(pc)
    assert flt.values.shape == (300,) and bool((flt.values > 0).all())
    want = ref.compute_filter_3d(pc.get_anchor, flt.cameras)
    assert err(flt.values, want) <= 2e-5
    big = flt.values * 40.0                                        # a filter of a few pixels: visible in the picture
    plain, _, _ = render_views(cams, pc, PIPE, bg)
    filtered, _, _ = render_views(cams, pc, PIPE, bg, filter_3d=big)
    assert not torch.equal(plain[0], filtered[0])
    gts = [p.clamp(0, 1) for p in plain]
    res = evaluate_views(cams, pc, PIPE, bg, gts=gts, filter_3d=flt)
    assert res["NUM"] == 300 and math.isfinite(res["PSNR"])
    # one training step: the filter is handed to every render, and a stale one is refreshed on entry
    params = [p for p in pc.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-3)
    pc.sort_anchors()
    assert flt.stale(pc)
    before = pc._scaling.detach().clone()
    loss, out, _ = collaborative_step(pc, cams, gts, PIPE, bg, optimizer=opt, iteration=7, filter_3d=flt)
    assert not flt.stale(pc) and torch.isfinite(loss) and out["render"].shape == (3, H, W)
    assert err(flt.values, ref.compute_filter_3d(pc.get_anchor - 0 * pc.get_anchor, flt.cameras), scale_floor=1e-3) <= 1e-2
    assert not torch.equal(before, pc._scaling.detach())
    values = flt.values
    collaborative_step(pc, cams, gts, PIPE, bg, iteration=8, filter_3d=flt)
    assert flt.values is values                                    # neither stale nor due
    collaborative_step(pc, cams, gts, PIPE, bg, iteration=100, filter_3d=flt)
    assert flt.values is not values                                # iteration % every == 0
