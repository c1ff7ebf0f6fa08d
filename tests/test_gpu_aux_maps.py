"""GPU tests of the rasterizer's depth and opacity maps (GaussianRasterizer.forward(..., return_aux=True), render(aux=True)).

Definitions: depth = sum_i w_i z_i, alpha = sum_i w_i, w_i = alpha_i T_i over the contributors of the colour image, z_i the
view-space depth of the splat record; background excluded, depth not normalised.

Reference: the colour-only operator called twice on the same inputs -- the second call with colors_precomp = (z, 1, 0),
z = means3D @ viewmatrix[:3, 2] + viewmatrix[3, 2] formed in torch (autograd carries dL/dz), and bg = 0.  The blend is linear in
(colour, dL/dpixel), so the sum of the two passes' gradients is the gradient of <Gc, image> + <Gd, depth> + <Ga, alpha>.

Bars (those of test_gpu_parity.py): maps 1e-4 absolute, depth divided by the image's largest |depth|; gradients rel-L2 <= 1e-4
per tensor; colour image and radii of the aux call torch.equal with the plain call.
"""
import math
import types

import numpy as np
import pytest
import torch

from util import rel_l2, small_scene
from splatco_amd.synthetic import synthetic_camera

pytestmark = pytest.mark.gpu

MAP_TOL = 1e-4
GRAD_TOL = 1e-4


def _dev():
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    return torch.device("cuda:0")


def _settings(cam, bg, sh_degree=1):
    from splatco_amd.rasterizer import GaussianRasterizationSettings
    d = _dev()
    return GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=torch.as_tensor(bg, dtype=torch.float32, device=d),
        scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(d), projmatrix=cam.full_proj_transform.to(d),
        sh_degree=sh_degree, campos=cam.camera_center.to(d), prefiltered=False, debug=False)


def _leaves(g, shs=None, cov=None):
    """Fresh leaf tensors of a scene: the operator's keyword arguments (without means2D) that require grad."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=_dev(), requires_grad=True)
    kw = dict(means3D=t(g["means3D"]), opacities=t(g["opacities"]))
    if cov is None:
        kw.update(scales=t(g["scales"]), rotations=t(g["rotations"]))
    else:
        kw.update(cov3D_precomp=t(cov))
    kw.update(shs=t(shs)) if shs is not None else kw.update(colors_precomp=t(g["colors"]))
    return kw


def _weights(cam, seed=11):
    """Fixed random dL/dimage, dL/ddepth, dL/dalpha."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    H, W = cam.image_height, cam.image_width
    return (torch.randn(3, H, W, generator=gen).to(_dev()), torch.randn(H, W, generator=gen).to(_dev()),
            torch.randn(H, W, generator=gen).to(_dev()))


def _collect(kw, m2d):
    out = {k: v.grad for k, v in kw.items()}
    out["means2D"] = m2d.grad
    return out


def fused(cam, g, G=None, use="cda", shs=None, cov=None):
    """One call with return_aux=True; the loss takes the outputs named in `use` (c: image, d: depth, a: alpha)."""
    from splatco_amd.rasterizer import GaussianRasterizer
    kw = _leaves(g, shs, cov)
    m2d = torch.zeros(kw["means3D"].shape[0], 3, device=_dev(), requires_grad=True)
    img, radii, depth, alpha = GaussianRasterizer(_settings(cam, g["bg"]))(means2D=m2d, return_aux=True, **kw)
    res = dict(image=img.detach(), radii=radii, depth=depth.detach(), alpha=alpha.detach())
    if G is not None:
        parts = dict(c=(img, G[0]), d=(depth, G[1]), a=(alpha, G[2]))
        sum((parts[k][0] * parts[k][1]).sum() for k in use).backward()
        res["grads"] = _collect(kw, m2d)
    torch.cuda.synchronize()
    return res


def plain(cam, g, Gc=None, shs=None, cov=None):
    """The colour-only call."""
    from splatco_amd.rasterizer import GaussianRasterizer
    kw = _leaves(g, shs, cov)
    m2d = torch.zeros(kw["means3D"].shape[0], 3, device=_dev(), requires_grad=True)
    out = GaussianRasterizer(_settings(cam, g["bg"]))(means2D=m2d, **kw)
    assert len(out) == 2
    res = dict(image=out[0].detach(), radii=out[1])
    if Gc is not None:
        (out[0] * Gc).sum().backward()
        res["grads"] = _collect(kw, m2d)
    torch.cuda.synchronize()
    return res


def two_pass(cam, g, G, shs=None, cov=None):
    """The reference: the colour-only operator twice, the second time on the colours (z, 1, 0) over a black background."""
    from splatco_amd.rasterizer import GaussianRasterizer
    kw = _leaves(g, shs, cov)
    m2d = torch.zeros(kw["means3D"].shape[0], 3, device=_dev(), requires_grad=True)
    img, radii = GaussianRasterizer(_settings(cam, g["bg"]))(means2D=m2d, **kw)
    view = cam.world_view_transform.to(_dev())
    z = kw["means3D"] @ view[:3, 2] + view[3, 2]
    kw2 = {k: v for k, v in kw.items() if k not in ("shs", "colors_precomp")}
    kw2["colors_precomp"] = torch.stack((z, torch.ones_like(z), torch.zeros_like(z)), dim=1)
    aux, radii2 = GaussianRasterizer(_settings(cam, np.zeros(3, np.float32)))(means2D=m2d, **kw2)
    assert torch.equal(radii, radii2)
    ((img * G[0]).sum() + (aux[0] * G[1]).sum() + (aux[1] * G[2]).sum()).backward()
    torch.cuda.synchronize()
    return dict(image=img.detach(), radii=radii, depth=aux[0].detach(), alpha=aux[1].detach(), grads=_collect(kw, m2d))


def state(cam, g):
    """The saved state of an aux forward (debug getters) and its maps."""
    from splatco_amd import rasterizer as R
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=_dev())
    _, _, st = R.rasterize_forward(R._CSettings(_settings(cam, g["bg"])), t(g["means3D"]), t(g["opacities"]), t(g["scales"]),
                                   t(g["rotations"]), None, None, t(g["colors"]), aux=True)
    return st


def check_maps(got, want, tag):
    scale = max(float(want["depth"].abs().max()), 1e-30)
    ed = float((got["depth"] - want["depth"]).abs().max()) / scale
    ea = float((got["alpha"] - want["alpha"]).abs().max())
    print(f"[aux] {tag}: depth max-abs / max|depth| {ed:.2e}, alpha max-abs {ea:.2e}, max|depth| {scale:.3f}")
    assert ed <= MAP_TOL and ea <= MAP_TOL
    assert float(want["alpha"].max()) > 0.5, "the scene must cover something"


def check_grads(got, want, names, tag):
    errs = {n: rel_l2(got[n].cpu().numpy(), want[n].cpu().numpy()) for n in names}
    print(f"[aux] {tag}: gradient rel-L2 vs two passes: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    for n in names:
        assert got[n].shape == want[n].shape, n
        assert float(want[n].abs().max()) > 0, n
        assert errs[n] <= GRAD_TOL, (n, errs[n])


ALL = ["means3D", "means2D", "colors_precomp", "opacities", "scales", "rotations"]


def check_against_two_passes(cam, g, tag, names=ALL, shs=None, cov=None):
    G = _weights(cam)
    f, ref, p = fused(cam, g, G, shs=shs, cov=cov), two_pass(cam, g, G, shs=shs, cov=cov), plain(cam, g, shs=shs, cov=cov)
    same = lambda a, b: torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))
    assert same(f["image"], p["image"]) and torch.equal(f["radii"], p["radii"]), "colour image / radii of the aux call"
    check_maps(f, ref, tag)
    check_grads(f["grads"], ref["grads"], names, tag)
    return f, ref


# ------------------------------------------------------------------ scenes
def long_list_scene():
    """P = 3000 at 70x52, means scaled by 0.3: tile lists of several 64-entry chunks."""
    return small_scene(P=3000, W=70, H=52, spread=0.3)


def wall_scene():
    """An opaque wall (400 splats, opacity 0.95, over x = 10..38) in front of 1500 smaller splats in the tile column
    x = 16..31 of a 70x52 image, whose footprints stay behind the wall (the CPU oracle has every one of them without any
    gradient)."""
    W, H, nw, nb = 70, 52, 400, 1500
    cam = synthetic_camera(W, H)
    rng = np.random.default_rng(21)
    tx, ty = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
    P = nw + nb
    z = np.concatenate([rng.uniform(2.0, 2.5, nw), rng.uniform(4.0, 6.0, nb)]).astype(np.float32)
    px = np.concatenate([rng.uniform(10, 38, nw), rng.uniform(18, 30, nb)])
    py = rng.uniform(0, H, P)
    means = np.stack([((2 * px + 1) / W - 1) * tx * z, ((2 * py + 1) / H - 1) * ty * z, z], 1).astype(np.float32)
    sigma_px = np.concatenate([np.full(nw, 3.0), np.full(nb, 1.5)])[:, None]      # screen-space standard deviation
    scales = (sigma_px * 2 * tx / W * rng.uniform(0.7, 1.4, (P, 3)) * z[:, None]).astype(np.float32)
    rot = rng.standard_normal((P, 4))
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True)).astype(np.float32)
    op = np.concatenate([np.full(nw, 0.95), rng.uniform(0.3, 0.9, nb)]).astype(np.float32)[:, None]
    g = dict(means3D=means, scales=scales, rotations=rot, opacities=op, colors=rng.uniform(0, 1, (P, 3)).astype(np.float32),
             bg=np.array([0.1, 0.3, 0.7], np.float32))
    return cam, g, nw


def large_rect_scene():
    """160x112 (70 tiles): two Gaussians whose tile rects hold more than 32 tiles, plus 200 small ones."""
    cam, g = small_scene(P=202, W=160, H=112)
    g["means3D"][:2] = np.array([[0.1, 0.0, 0.2], [-0.2, 0.1, -0.1]], np.float32)
    g["scales"][:2] = np.array([[0.9, 0.7, 0.8], [0.6, 0.8, 0.7]], np.float32)
    g["opacities"][:2] = np.array([[0.25], [0.4]], np.float32)
    return cam, g


def cov3d(g):
    """Sigma = (R S)(R S)^T as the operator forms it (quaternions as given), upper triangle."""
    q, s = g["rotations"].astype(np.float64), g["scales"].astype(np.float64)
    r, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    L = R * s[:, None, :]
    S = L @ L.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)


# ------------------------------------------------------------------ cases
def test_partial_tiles_and_quadrants():
    """70x52: neither a multiple of 16 nor of 8.  Forward and every gradient."""
    cam, g = small_scene(P=96, W=70, H=52)
    f, _ = check_against_two_passes(cam, g, "partial tiles")
    assert f["depth"].shape == (52, 70) and f["alpha"].shape == (52, 70)
    assert torch.all(f["grads"]["means2D"][:, 2] == 0)


@pytest.fixture(scope="module")
def long_lists():
    """Case 2's results, shared by the tests that compare against them."""
    cam, g = long_list_scene()
    G = _weights(cam)
    return cam, g, G, fused(cam, g, G)


def test_long_lists(long_lists):
    from splatco_amd import _C
    cam, g, G, f = long_lists
    st = state(cam, g)
    ranges = st.debug(_C.DBG_RANGES).cpu().numpy().view(np.uint32).astype(np.int64)
    qm = st.debug(_C.DBG_QMASK).cpu().numpy()
    n = ranges[:, 1] - ranges[:, 0]
    # entries per (tile, quadrant wave): what a wave stages; its last group holds count mod 4 splats
    counts = np.array([int(((qm[lo:hi] >> q) & 1).sum()) for lo, hi in ranges for q in range(4)])
    print(f"[aux] long lists: largest tile {n.max()} entries, per-wave counts mod 4: {np.bincount(counts % 4, minlength=4)}")
    assert n.max() > 192, "no tile list runs over several 64-entry chunks"
    assert set(np.unique(counts[counts > 0] % 4)) == {0, 1, 2, 3}
    ref, p = two_pass(cam, g, G), plain(cam, g)
    assert torch.equal(f["image"], p["image"]) and torch.equal(f["radii"], p["radii"])
    check_maps(f, ref, "long lists")
    check_grads(f["grads"], ref["grads"], ALL, "long lists")


def test_early_stop_and_the_cut():
    from splatco_amd import _C
    cam, g, nw = wall_scene()
    f, ref = check_against_two_passes(cam, g, "wall")
    st = state(cam, g)
    ranges = st.debug(_C.DBG_RANGES).cpu().numpy().view(np.uint32).astype(np.int64)
    ncon = st.debug(_C.DBG_N_CONTRIB).cpu().numpy().view(np.uint32).astype(np.int64)
    gx = (cam.image_width + 15) // 16
    n = ranges[:, 1] - ranges[:, 0]
    wall_px = ncon[:, 16:32]
    length = np.repeat(n.reshape(-1, gx)[:, 1], 16)[:cam.image_height, None]
    print(f"[aux] wall: list lengths of the column's tiles {n.reshape(-1, gx)[:, 1]}, "
          f"pixels stopped early {(wall_px < length).mean():.0%}")
    assert (wall_px < length).mean() > 0.5, "most wall pixels stop before the end of their list"
    spare = []
    for ty in range(n.size // gx):
        t = ty * gx + 1
        top = int(ncon[16 * ty:16 * ty + 16, 16:32].max())
        spare.append((n[t] + 63) // 64 - 1 - ((top - 1) // 64 if top else -1))
    print(f"[aux] wall: spare rounds per tile of the column {spare}")
    assert max(spare) >= 3, "no tile leaves three or more rounds without records"
    # splats that no pixel reaches: their gradients are exactly zero, as the two passes have them
    hidden = np.ones(g["means3D"].shape[0], bool)
    hidden[:nw] = False
    for k in ALL:
        hidden &= (ref["grads"][k].reshape(hidden.size, -1) == 0).all(1).cpu().numpy()
    print(f"[aux] wall: {hidden.sum()} hidden splats")
    assert hidden.sum() >= 1000
    sel = torch.tensor(hidden, device=_dev())
    for k in ALL:
        assert torch.all(f["grads"][k][sel] == 0), k


def test_deep_list_variant_is_bit_identical(long_lists):
    from splatco_amd import _C
    cam, g, G, base = long_lists
    _C.check(_C.lib.scr_debug_force_deep_lists(1))
    try:
        f = fused(cam, g, G)
    finally:
        _C.check(_C.lib.scr_debug_force_deep_lists(-1))
    for k in ("image", "radii", "depth", "alpha"):
        assert torch.equal(f[k], base[k]), k
    for k in base["grads"]:
        assert torch.equal(f["grads"][k], base["grads"][k]), k


def test_large_rects():
    from splatco_amd import _C
    cam, g = large_rect_scene()
    st = state(cam, g)
    tt = st.debug(_C.DBG_TILES_TOUCHED).cpu().numpy().view(np.uint32)
    assert st.flags & _C.PLAN_LARGE_RECTS and (tt > 32).sum() >= 2, tt[:2]
    check_against_two_passes(cam, g, "large rects")


@pytest.mark.parametrize("variant", ["shs", "shs_cov3D"])
def test_sh_and_cov_inputs(variant):
    cam, g = small_scene(P=200, W=70, H=52, seed=8)
    shs = (np.random.default_rng(5).standard_normal((200, 4, 3)) * 0.4).astype(np.float32)
    cov = cov3d(g) if variant == "shs_cov3D" else None
    check_against_two_passes(cam, g, variant, names=["means3D", "opacities"], shs=shs, cov=cov)


def test_gradient_subsets():
    cam, g = small_scene(P=96, W=70, H=52)
    G = _weights(cam)
    zero = torch.zeros_like
    for use, Gs in (("d", (zero(G[0]), G[1], zero(G[2]))), ("a", (zero(G[0]), zero(G[1]), G[2]))):
        f, ref = fused(cam, g, G, use=use), two_pass(cam, g, Gs)
        names = [n for n in ALL if n != "colors_precomp"]
        check_grads(f["grads"], ref["grads"], names, f"subset {use}")
        assert torch.all(f["grads"]["colors_precomp"] == 0)       # the colours do not reach either map
    # colour only through the aux call: the colour-only kernels, the plain call's bits
    f, p = fused(cam, g, G, use="c"), plain(cam, g, G[0])
    for k in ALL:
        assert torch.equal(f["grads"][k], p["grads"][k]), k


def test_nonfinite_colour_stays_out_of_the_maps():
    cam, g = small_scene(P=96, W=70, H=52)
    clean = fused(cam, g)
    vis = np.flatnonzero(clean["radii"].cpu().numpy() > 0)
    cam_z = (g["means3D"] @ cam.world_view_transform.numpy()[:3, 2] + cam.world_view_transform.numpy()[3, 2])
    victim = int(vis[np.argmin(cam_z[vis])])                 # the front-most visible Gaussian: it contributes somewhere
    bad = {k: v.copy() for k, v in g.items()}
    bad["colors"][victim, 1] = np.nan
    f, p = fused(cam, bad), plain(cam, bad)
    assert torch.isfinite(f["depth"]).all() and torch.isfinite(f["alpha"]).all()
    assert torch.equal(f["depth"], clean["depth"]) and torch.equal(f["alpha"], clean["alpha"])
    assert torch.equal(f["image"].isnan(), p["image"].isnan()) and f["image"].isnan().any() and not f["image"].isnan().all()
    assert torch.equal(f["image"].nan_to_num(nan=0.0), p["image"].nan_to_num(nan=0.0))


def test_planar_scene_analytic():
    """All Gaussians on the plane z = z0 of view space: depth = z0 * alpha to 1e-5 relative, and alpha = 1 - final_T to 1e-6 --
    neither goes through the rasterizer twice.  The kernel forms alpha AS 1 - final_T (exact by Sterbenz for T >= 1/2), so the
    second distance is 0; the first is then dominated by the rounding of T itself, half an ulp of a number below 1 (3e-8) per
    contributor against an alpha of at least 1/255 per contributor: <= 7.6e-6 relative, plus the 1e-6 of z's own four
    roundings (measured: 6.9e-6)."""
    from splatco_amd import _C
    cam, g = small_scene(P=300, W=70, H=52)
    z0 = 4.0
    rng = np.random.default_rng(2)
    V = cam.world_view_transform.numpy().astype(np.float64)
    pv = np.concatenate([rng.uniform(-1.5, 1.5, (300, 2)), np.full((300, 1), z0), np.ones((300, 1))], 1)
    g["means3D"] = (pv @ np.linalg.inv(V))[:, :3].astype(np.float32)
    st = state(cam, g)
    depth, alpha = st.aux
    final_T = st.debug(_C.DBG_FINAL_T)
    covered = alpha > 0
    assert covered.float().mean() > 0.5
    rel = ((depth - z0 * alpha).abs() / (z0 * alpha).clamp_min(1e-30))[covered]
    print(f"[aux] planar: max relative |depth - z0 alpha| {float(rel.max()):.2e}, "
          f"max |alpha - (1 - final_T)| {float((alpha - (1 - final_T)).abs().max()):.2e}")
    assert float(rel.max()) <= 1e-5
    assert float((alpha - (1 - final_T)).abs().max()) <= 1e-6
    assert torch.all(depth[~covered] == 0)


def test_determinism(long_lists):
    cam, g, G, base = long_lists
    again = fused(cam, g, G)
    for k in ("image", "radii", "depth", "alpha"):
        assert torch.equal(again[k], base[k]), k
    for k in base["grads"]:
        assert torch.equal(again["grads"][k], base["grads"][k]), k


def test_no_gaussians():
    from splatco_amd.rasterizer import GaussianRasterizer
    cam, g = small_scene(P=96, W=70, H=52)
    e = lambda *s: torch.zeros(*s, device=_dev(), requires_grad=True)
    img, radii, depth, alpha = GaussianRasterizer(_settings(cam, g["bg"]))(
        means3D=e(0, 3), means2D=e(0, 3), opacities=e(0, 1), colors_precomp=e(0, 3), scales=e(0, 3), rotations=e(0, 4),
        return_aux=True)
    assert radii.numel() == 0 and depth.shape == (52, 70) and alpha.shape == (52, 70)
    assert torch.all(depth == 0) and torch.all(alpha == 0)
    assert torch.equal(img, torch.tensor(g["bg"], device=_dev()).reshape(3, 1, 1).expand(3, 52, 70))


def test_render_returns_the_maps():
    """renderer.render(..., aux=True) on the small anchor scene of test_gpu_renderer.py."""
    from test_gpu_renderer import _model
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.renderer import prefilter_voxel, render
    dev = _dev()
    pc, _ = _model(dev)
    cam = look_at_camera(eye=(0.3, -0.2, -4.5), target=(0, 0, 0), up=(0, -1, 0), FoVx=math.radians(60), width=200,
                         height=120).to(dev)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False, mv=4)
    bg = torch.tensor([1.0, 1.0, 1.0], device=dev)
    pc.train()
    vis = prefilter_voxel(cam, pc, pipe, bg)
    base = render(cam, pc, pipe, bg, visible_mask=vis)
    assert set(base) == {"render", "viewspace_points", "visibility_filter", "radii", "selection_mask", "neural_opacity",
                         "scaling"}
    out = render(cam, pc, pipe, bg, visible_mask=vis, aux=True)
    assert set(out) == set(base) | {"depth", "alpha"}
    assert out["depth"].shape == (120, 200) and out["alpha"].shape == (120, 200)
    assert torch.equal(out["render"], base["render"])
    gen = torch.Generator(device="cpu").manual_seed(3)
    wd, wa = torch.randn(120, 200, generator=gen).to(dev), torch.randn(120, 200, generator=gen).to(dev)
    ((out["depth"] * wd).sum() + (out["alpha"] * wa).sum()).backward()
    for p in (pc._anchor, pc._offset, pc.mlp_opacity[0].weight, pc.mlp_cov[0].weight):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0
