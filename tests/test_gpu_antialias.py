"""GPU tests of the rasterizer's antialiased mode (GaussianRasterizer.forward(..., antialiased=True), render(antialiased=...)).

Three evaluations (tests/antialias_refs.py): K, the kernel with antialiased=True; R64, h = sqrt(max(0.000025, det0 / det)) in
float64 torch, rounded to float32 and multiplied into the opacities of the EXISTING operator, gradients by autograd through
both (the camera's: the operator's own camera gradients plus autograd through h); R32, the same with h in float32.

Bar for K against R64: 1e-4 absolute on the image and the maps, rel-L2 <= 1e-4 per gradient tensor (test_gpu_parity.py,
test_gpu_aux_maps.py); where R32 itself is further from R64, 4 x R32's distance for that tensor.
"""
import math
import types

import numpy as np
import pytest
import torch

import antialias_refs as A
from util import rel_l2, small_scene

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    return torch.device("cuda:0")


def _t(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=_dev(), requires_grad=grad)


def _weights(cam, seed=11):
    """Fixed random dL/dimage, dL/ddepth, dL/dalpha (test_gpu_aux_maps.py::_weights)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    H, W = cam.image_height, cam.image_width
    return tuple(torch.randn(*s, generator=gen).to(_dev()) for s in ((3, H, W), (H, W), (H, W)))


def _leaves(cam, g, shs=None, cov=None):
    """Fresh leaves: the operator's tensor arguments and the camera's three tensors, all requiring grad."""
    kw = dict(means3D=_t(g["means3D"], True), opacities=_t(g["opacities"], True))
    if cov is None:
        kw.update(scales=_t(g["scales"], True), rotations=_t(g["rotations"], True))
    else:
        kw.update(cov3D_precomp=_t(cov, True))
    kw.update(shs=_t(shs, True)) if shs is not None else kw.update(colors_precomp=_t(g["colors"], True))
    kw["means2D"] = torch.zeros(g["means3D"].shape[0], 3, device=_dev(), requires_grad=True)
    camera = dict(viewmatrix=cam.world_view_transform.to(_dev()).clone().requires_grad_(),
                  projmatrix=cam.full_proj_transform.to(_dev()).clone().requires_grad_(),
                  campos=cam.camera_center.to(_dev()).clone().requires_grad_())
    return kw, camera


def _rasterizer(cam, g, camera, scale_modifier=1.0, sh_degree=1):
    from splatco_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    return GaussianRasterizer(GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=_t(g["bg"]), scale_modifier=scale_modifier, viewmatrix=camera["viewmatrix"],
        projmatrix=camera["projmatrix"], sh_degree=sh_degree, campos=camera["campos"], prefiltered=False, debug=False))


def _finish(outs, kw, camera, G, retain=False):
    img, radii, depth, alpha = outs
    res = dict(image=img.detach(), radii=radii, depth=depth.detach(), alpha=alpha.detach())
    if G is not None:
        ((img * G[0]).sum() + (depth * G[1]).sum() + (alpha * G[2]).sum()).backward(retain_graph=retain)
        leaves = {**kw, **camera}
        res["grads"] = {k: (torch.zeros_like(v) if v.grad is None else v.grad.clone()) for k, v in leaves.items()}
    torch.cuda.synchronize()
    return res


def run_K(cam, g, G=None, antialiased=True, shs=None, cov=None, scale_modifier=1.0, sh_degree=1, mode_kw=True):
    """The kernel: one call with return_aux=True, the loss on colour, depth and alpha, the camera requiring grad.
    mode_kw=False leaves the `antialiased` argument out altogether (the call as it was before the mode existed)."""
    kw, camera = _leaves(cam, g, shs, cov)
    extra = dict(antialiased=antialiased) if mode_kw else {}
    outs = _rasterizer(cam, g, camera, scale_modifier, sh_degree)(return_aux=True, **extra, **kw)
    return _finish(outs, kw, camera, G)


def run_R(cam, g, G, dtype, shs=None, cov=None, scale_modifier=1.0, sh_degree=1):
    """The reference: h in `dtype` torch over the visible Gaussians (1 elsewhere), rounded to float32, times the opacities,
    then the existing operator; autograd through both."""
    kw, camera = _leaves(cam, g, shs, cov)
    rast = _rasterizer(cam, g, camera, scale_modifier, sh_degree)
    geo = {k: kw[k] for k in ("scales", "rotations", "cov3D_precomp") if k in kw}
    idx = torch.nonzero(rast.visible_filter(kw["means3D"].detach(), **{k: v.detach() for k, v in geo.items()}) > 0).reshape(-1)
    tm = A.aa_terms(kw["means3D"][idx], camera["viewmatrix"], cam.image_width, cam.image_height, math.tan(cam.FoVx * 0.5),
                    math.tan(cam.FoVy * 0.5), scale_modifier=scale_modifier, dtype=dtype, **{k: v[idx] for k, v in geo.items()})
    h = torch.ones(kw["means3D"].shape[0], device=_dev()).index_copy(0, idx, tm["h"].to(torch.float32))
    args = dict(kw, opacities=kw["opacities"] * h.reshape(kw["opacities"].shape))
    res = _finish(rast(return_aux=True, **args), kw, camera, G)
    res["h"], res["visible"], res["on_floor"] = h.detach(), idx, tm["on_floor"].detach()
    return res


GRADS = ["means3D", "means2D", "colors_precomp", "opacities", "scales", "rotations", "viewmatrix", "projmatrix"]


def _dist(got, want, name):
    if name in ("image", "depth", "alpha"):
        return float((got[name] - want[name]).abs().max())
    return rel_l2(got["grads"][name].cpu().numpy(), want["grads"][name].cpu().numpy())


def check_parity(cam, g, tag, names=GRADS, **variant):
    """K against R64 at the bar of the module docstring; prints both distances per tensor."""
    G = _weights(cam)
    k, r64, r32 = run_K(cam, g, G, **variant), run_R(cam, g, G, torch.float64, **variant), run_R(cam, g, G, torch.float32, **variant)
    assert torch.equal(k["radii"], r64["radii"]) and torch.equal(k["radii"], r32["radii"])
    assert float(r64["alpha"].max()) > 0.5, "the scene must cover something"
    failed = []
    for name in ["image", "depth", "alpha"] + list(names):
        if name not in ("image", "depth", "alpha"):
            assert k["grads"][name].shape == r64["grads"][name].shape, name
            assert float(r64["grads"][name].abs().max()) > 0, name
        e32, ek = _dist(r32, r64, name), _dist(k, r64, name)
        print(f"[antialias] {tag}: {name:15s} R32-R64 {e32:.3e}   K-R64 {ek:.3e}   bar {A.bar(e32):.3e}")
        if not ek <= A.bar(e32):
            failed.append((name, ek, A.bar(e32)))
    assert not failed, failed
    return k, r64, r32


def _state(cam, g, **kw):
    """The saved state of a forward (debug getters)."""
    from splatco_amd import rasterizer as R
    _, camera = _leaves(cam, g)
    cs = R._CSettings(_rasterizer(cam, g, {k: v.detach() for k, v in camera.items()}).raster_settings)
    _, radii, st = R.rasterize_forward(cs, _t(g["means3D"]), _t(g["opacities"]), _t(g["scales"]), _t(g["rotations"]), None, None,
                                       _t(g["colors"]), **kw)
    torch.cuda.synchronize()
    return st, radii


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _all_equal(x, y):
    assert all(torch.equal(x[k], y[k]) for k in ("image", "radii", "depth", "alpha"))
    assert x["grads"].keys() == y["grads"].keys()
    for k in x["grads"]:
        assert _same_bits(x["grads"][k], y["grads"][k]), k


# ------------------------------------------------------------------ 1. off is the old call
def test_off_is_the_old_call():
    import ctypes as C
    from splatco_amd import _C
    cam, g = A.mixed_scene()
    G = _weights(cam)
    old, off = run_K(cam, g, G, mode_kw=False), run_K(cam, g, G, antialiased=False)
    _all_equal(old, off)
    assert float(old["grads"]["viewmatrix"].abs().max()) > 0 and float(old["grads"]["scales"].abs().max()) > 0
    # colour only, no camera gradient: the plain call
    rast = _rasterizer(cam, g, {k: v.detach() for k, v in _leaves(cam, g)[1].items()})
    outs = []
    for extra in ({}, dict(antialiased=False)):
        kw, _ = _leaves(cam, g)
        img, radii = rast(**extra, **kw)
        (img * G[0]).sum().backward()
        outs.append((img.detach(), radii, {k: v.grad for k, v in kw.items()}))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert all(_same_bits(outs[0][2][k], outs[1][2][k]) for k in outs[0][2])
    # the records of a direct plan-only scr_forward_plan_run(0, ...) against those of the operator's default forward
    st, radii = _state(cam, g)
    assert st.flags & _C.PLAN_ANTIALIASED == 0
    vis = radii > 0
    rec = st.debug(_C.DBG_SPLAT_RECORDS)
    P = st.P
    geom = _C.scratch(_C.lib.scr_geom_bytes(P, st.cs.H, st.cs.W), _dev())
    radii0 = torch.empty(P, dtype=torch.int32, device=_dev())
    plan = (C.c_int64 * 4)(0, 0, 0, 0)
    ins = [_t(g[k]) for k in ("means3D", "scales", "rotations", "opacities", "colors")]
    with torch.cuda.device(_dev()):
        _C.check(_C.lib.scr_forward_plan_run(0, P, 0, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), None,
                                              ins[3].data_ptr(), None, ins[4].data_ptr(), st.cs.ref(), geom.data_ptr(),
                                              radii0.data_ptr(), plan, None, 0, None, None, None, None, _C.stream()))
        rec0 = torch.empty(P, 12, dtype=torch.float32, device=_dev())
        _C.check(_C.lib.scr_debug_get(_C.DBG_SPLAT_RECORDS, P, 0, st.cs.H, st.cs.W, geom.data_ptr(), None, None,
                                      rec0.data_ptr(), _C.stream()))
    torch.cuda.synchronize()
    assert (int(plan[0]), int(plan[1]), int(plan[2]), int(plan[3])) == (st.I, st.max_tile, 0, st.flags)
    assert torch.equal(radii0, radii) and int(vis.sum()) == 509
    assert _same_bits(rec0[vis], rec[vis])


# ------------------------------------------------------------------ 2. integers do not move
def test_integers_do_not_move_and_the_record_carries_o_h():
    from splatco_amd import _C
    cam, g = A.mixed_scene()
    (off, radii_off), (on, radii_on) = _state(cam, g), _state(cam, g, antialiased=True)
    assert off.flags & _C.PLAN_ANTIALIASED == 0 and on.flags == off.flags | _C.PLAN_ANTIALIASED
    assert torch.equal(radii_off, radii_on) and (off.I, off.max_tile) == (on.I, on.max_tile)
    for which in (_C.DBG_TILES_TOUCHED, _C.DBG_POINT_OFFSETS, _C.DBG_RANGES, _C.DBG_POINT_LIST):
        assert torch.equal(off.debug(which), on.debug(which)), which
    vis = radii_on > 0
    r_off, r_on = off.debug(_C.DBG_SPLAT_RECORDS)[vis], on.debug(_C.DBG_SPLAT_RECORDS)[vis]
    keep = [c for c in range(12) if c != 5]
    assert _same_bits(r_off[:, keep], r_on[:, keep])
    assert torch.equal(r_off[:, 5], _t(g["opacities"]).reshape(-1)[vis])
    # column 5 = o h: against the float64 h, at 4 x the float32 restatement's own largest relative deviation (>= 1e-6)
    vis_c = vis.cpu()
    o32 = torch.tensor(g["opacities"]).reshape(-1)[vis_c]
    h64 = A.aa_terms_scene(cam, g, torch.float64)["h"][vis_c]
    h32 = A.aa_terms_scene(cam, g, torch.float32)["h"][vis_c]
    want = o32.double() * h64
    e32 = float(((o32 * h32).double() / want - 1.0).abs().max())
    ek = float((r_on[:, 5].cpu().double() / want - 1.0).abs().max())
    print(f"[antialias] record opacity o h, largest relative deviation from R64: R32 {e32:.3e}, K {ek:.3e}, "
          f"bar {max(1e-6, 4 * e32):.3e}; K == R32 bit for bit on {int((r_on[:, 5].cpu() == o32 * h32).sum())} of {int(vis_c.sum())}")
    assert ek <= max(1e-6, 4.0 * e32)
    c = A.scene_counts(cam, g, vis_c.numpy())
    assert c["high"] >= 0.05 and c["mid"] >= 0.30 and c["floor"] >= 100 and c["near_kink"] == 0, c


# ------------------------------------------------------------------ 3. - 5. parity
def test_parity_mixed_scene():
    cam, g = A.mixed_scene()
    k, r64, _ = check_parity(cam, g, "mixed")
    n_floor = int(r64["on_floor"].sum())
    assert int(r64["visible"].numel()) == 509 and n_floor >= 100
    assert float((k["image"] - run_K(cam, g, antialiased=False)["image"]).abs().max()) > 1e-2      # the mode does something


def test_parity_wide_scene_clamped_jacobians_large_rects():
    from splatco_amd import _C
    cam, g = A.wide_scene()
    st, radii = _state(cam, g, antialiased=True)
    assert st.flags == _C.PLAN_LARGE_RECTS | _C.PLAN_ANTIALIASED and int(st.debug(_C.DBG_TILES_TOUCHED).max()) > 32
    c = A.scene_counts(cam, g, (radii > 0).cpu().numpy())
    assert c["clamped"] >= 30, c
    check_parity(cam, g, "wide")


def test_parity_cov3D_precomp():
    cam, g = A.mixed_scene()
    names = [n for n in GRADS if n not in ("scales", "rotations")] + ["cov3D_precomp"]
    check_parity(cam, g, "cov3D_precomp", names=names, cov=A.cov3d(g))


def test_parity_shs_degree_1_with_campos():
    cam, g = A.mixed_scene()
    shs = (np.random.default_rng(5).standard_normal((g["means3D"].shape[0], 4, 3)) * 0.4).astype(np.float32)
    names = [n for n in GRADS if n != "colors_precomp"] + ["shs", "campos"]
    check_parity(cam, g, "shs degree 1", names=names, shs=shs, sh_degree=1)


def test_parity_scale_modifier():
    cam, g = A.mixed_scene()
    check_parity(cam, g, "scale_modifier 0.7", scale_modifier=0.7)


def test_forced_deep_lists_are_bit_identical():
    from splatco_amd import _C
    cam, g = A.mixed_scene()
    G = _weights(cam)
    auto = run_K(cam, g, G)
    try:
        _C.check(_C.lib.scr_debug_force_deep_lists(1))
        deep = run_K(cam, g, G)
    finally:
        _C.lib.scr_debug_force_deep_lists(-1)
    _all_equal(auto, deep)


# ------------------------------------------------------------------ 6. the floor
def test_floor_is_a_constant_factor():
    """The mixed scene's floored Gaussians alone: K is the plain operator on opacities * 0.005, the same fp32 product."""
    cam, g = A.mixed_scene()
    with torch.no_grad():
        on_floor = A.aa_terms_scene(cam, g)["on_floor"].numpy()
    sub = {k: (v[on_floor] if k != "bg" else v) for k, v in g.items()}
    assert sub["means3D"].shape[0] >= 100
    G = _weights(cam)
    k = run_K(cam, sub, G)
    n_vis = int((k["radii"] > 0).sum())
    assert n_vis >= 100
    h = np.sqrt(np.float32(A.FLOOR))
    assert h == np.float32(0.005)
    plain = run_K(cam, dict(sub, opacities=sub["opacities"] * h), G, antialiased=False)
    assert torch.equal(k["image"], plain["image"]) and torch.equal(k["depth"], plain["depth"]) and torch.equal(k["alpha"], plain["alpha"])
    assert float(plain["alpha"].max()) > 0, "some floored splat must still pass 1/255"
    for name in GRADS:
        want = plain["grads"][name] * (float(h) if name == "opacities" else 1.0)
        assert float(want.abs().max()) > 0, name
        e = rel_l2(k["grads"][name].cpu().numpy(), want.cpu().numpy())
        print(f"[antialias] floor: {name:15s} rel-L2 {e:.3e}")
        assert e <= 1e-6, (name, e)


# ------------------------------------------------------------------ 7. opacity mass
@pytest.mark.parametrize("s2", [0.3, 1.0, 4.0])
@pytest.mark.parametrize("centre", [(32.0, 32.0), (32.37, 31.81), (31.5, 31.5)], ids=["pixel", "offset", "corner"])
def test_opacity_mass(s2, centre):
    """One isotropic splat of opacity 0.9 and variance s2 px^2: the compensated alpha sums to 2 pi o s2 (within 3 %: the
    1/255 cut and the 3 sigma rect take about 1 % each); without the compensation the sum is more than 6 % above it."""
    cam, g = A.one_splat(s2, centre)
    want = 2.0 * math.pi * 0.9 * s2
    on, off = float(run_K(cam, g)["alpha"].sum()), float(run_K(cam, g, antialiased=False)["alpha"].sum())
    print(f"[antialias] mass s2 {s2} centre {centre}: on {on / want - 1:+.4f}, off {off / want - 1:+.4f} (relative to 2 pi o s2)")
    assert abs(on / want - 1.0) <= 0.03
    assert off / want - 1.0 > 0.06


# ------------------------------------------------------------------ 8. determinism
def test_determinism():
    cam, g = A.wide_scene()
    G = _weights(cam)
    kw, camera = _leaves(cam, g)
    outs = _rasterizer(cam, g, camera)(return_aux=True, antialiased=True, **kw)
    first = _finish(outs, kw, camera, G, retain=True)
    for v in list(kw.values()) + list(camera.values()):
        v.grad = None
    second = _finish(outs, kw, camera, G)
    _all_equal(first, second)
    _all_equal(first, run_K(cam, g, G))


# ------------------------------------------------------------------ 9. empty inputs
@pytest.mark.parametrize("case", ["P=0", "all culled"])
def test_empty_inputs(case):
    cam, g = small_scene(P=40, W=100, H=70, seed=5)
    if case == "P=0":
        g = {k: (v[:0] if k != "bg" else v) for k, v in g.items()}
    else:
        g["means3D"] = g["means3D"] + np.array([0.6, -0.4, -9.0], np.float32)      # behind the camera
    k = run_K(cam, g, _weights(cam))
    assert torch.equal(k["image"], _t(g["bg"]).reshape(3, 1, 1).expand_as(k["image"]))
    assert not k["depth"].any() and not k["alpha"].any() and not k["radii"].any()
    for name, v in k["grads"].items():
        assert torch.isfinite(v).all() and not v.any(), name


# ------------------------------------------------------------------ 10. render()
def test_render_evaluate_and_training_step_follow_the_flag():
    from splatco_amd.evaluate import evaluate_views, render_views
    from splatco_amd.rasterizer import GaussianRasterizer
    from splatco_amd.renderer import _settings, generate_neural_gaussians, prefilter_voxel, render
    from splatco_amd.synthetic import synthetic_anchor_model, synthetic_views
    from splatco_amd.train_step import collaborative_step
    dev = _dev()
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    pipe_aa = types.SimpleNamespace(debug=False, compute_cov3D_python=False, antialiasing=True)
    pc = synthetic_anchor_model(3000, seed=5, device=dev, plane_size=64)
    views = [v.to(dev) for v in synthetic_views(2, width=96, height=64)]
    bg = torch.zeros(3, device=dev)
    pc.eval()
    pc.feat_planes.Q0 = 0          # no plane noise: every render below is a function of its arguments
    view = views[0]
    with torch.no_grad():
        vis = prefilter_voxel(view, pc, pipe, bg)
        default = render(view, pc, pipe, bg, visible_mask=vis)["render"]
        on = render(view, pc, pipe, bg, visible_mask=vis, antialiased=True)
        by_pipe = render(view, pc, pipe_aa, bg, visible_mask=vis)["render"]
        off_despite_pipe = render(view, pc, pipe_aa, bg, visible_mask=vis, antialiased=False)["render"]
        xyz, color, opacity, scaling, rot = generate_neural_gaussians(view, pc, vis, is_training=False)[:5]
        op_level, radii = GaussianRasterizer(_settings(view, bg, 1.0, False))(
            means3D=xyz, means2D=torch.zeros_like(xyz), colors_precomp=color, opacities=opacity, scales=scaling, rotations=rot,
            antialiased=True)
    assert float((on["render"] - default).abs().max()) > 1e-3
    assert torch.equal(on["render"], op_level) and torch.equal(on["radii"], radii)
    assert torch.equal(by_pipe, on["render"]) and torch.equal(off_despite_pipe, default)
    # evaluate_views scores the antialiased images
    gts = [torch.rand(3, 64, 96, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) for _ in views]
    res_on, res_off = (evaluate_views(views, pc, pipe, bg, gts=gts, antialiased=a) for a in (True, None))
    imgs_on, _, _ = render_views(views, pc, pipe, bg, antialiased=True)
    assert torch.equal(imgs_on[0], on["render"])
    from splatco_amd.evaluate import score_views
    _, psnr, _ = score_views(imgs_on, gts)
    assert list(res_on["per_view"]["PSNR"].values()) == psnr.reshape(-1).double().cpu().tolist()
    assert res_on["per_view"]["PSNR"] != res_off["per_view"]["PSNR"]
    assert evaluate_views(views, pc, pipe_aa, bg, gts=gts)["per_view"]["PSNR"] == res_on["per_view"]["PSNR"]
    # one training step follows pipe.antialiasing
    pc.train()
    grads = []
    for p in (pipe, pipe, pipe_aa):
        for q in pc.parameters():
            q.grad = None
        loss, out, _ = collaborative_step(pc, views[:1], gts[:1], p, bg)
        torch.cuda.synchronize()
        assert torch.isfinite(loss)
        gr = {n: q.grad.detach().clone() for n, q in pc.named_parameters() if q.grad is not None}
        assert gr and all(torch.isfinite(v).all() for v in gr.values())
        grads.append(gr)
    assert grads[0].keys() == grads[2].keys()
    # the mode moves the gradients, and by far more than a repetition of the default step does (nothing, or roundings)
    dist = lambda x, y: max(float((x[n] - y[n]).norm() / x[n].norm().clamp_min(1e-30)) for n in x)
    repeat, moved = dist(grads[0], grads[1]), dist(grads[0], grads[2])
    print(f"[antialias] training step: largest per-parameter rel-L2, default twice {repeat:.2e}, default against antialiased {moved:.2e}")
    assert moved > 1e-3 and moved > 100.0 * repeat


# ------------------------------------------------------------------ 11. stale plan flags at the backward
def test_stale_plan_flags_never_give_plausible_wrong_gradients():
    """The backward follows the flag the forward left in geom_buf.  The argument's bit only picks the instantiation: wrongly
    set, the results are the plain ones; wrongly clear, every gradient is NaN."""
    from splatco_amd import _C
    cam, g = A.mixed_scene()
    G = _weights(cam)

    def run(antialiased, flip):
        kw, camera = _leaves(cam, g)
        outs = _rasterizer(cam, g, camera)(return_aux=True, antialiased=antialiased, **kw)
        state = outs[0].grad_fn.state
        assert bool(state.flags & _C.PLAN_ANTIALIASED) == antialiased
        if flip:
            state.flags ^= _C.PLAN_ANTIALIASED
        return _finish(outs, kw, camera, G)

    plain, plain_stale = run(False, False), run(False, True)
    _all_equal(plain, plain_stale)
    stale = run(True, True)
    for name in ("means3D", "opacities", "scales", "rotations", "viewmatrix"):
        assert torch.isnan(stale["grads"][name]).any(), name
    assert torch.isfinite(run(True, False)["grads"]["means3D"]).all()
