"""GPU tests of the rasterizer's camera gradients: dL/dviewmatrix, dL/dprojmatrix, dL/dcampos of GaussianRasterizer (returned
when the settings' camera tensors require grad), cameras.pose_delta_camera and render() with such a camera.

Reference for every numeric check: oracle/torch_ref.py::rasterize in float64 on the CPU with viewmatrix, projmatrix and campos
as leaves, loss <G, image> with a seeded G (camera_grad_refs.py).  Bar per returned tensor: rel-L2 <= max(1e-4, 1.5 e32), e32
being the float32 torch_ref's own rel-L2 against float64 on the same inputs (printed; 4e-7 .. 2.6e-6 on these scenes, so the
bar is 1e-4, the project's gradient bar against its oracle).  Structural zeros (dV[:, 3], dM[:, 2], dcampos with
colors_precomp) must be exactly 0.  All scenes are 64x48 unless stated.
"""
import dataclasses
import math
import types

import numpy as np
import pytest
import torch

import camera_grad_refs as R
from util import rel_l2, small_scene

pytestmark = pytest.mark.gpu

def _dev():
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    return torch.device("cuda:0")


def camera_leaves(cam, want=R.NAMES):
    """The camera's three tensors on the device; those named in `want` are leaves that require grad."""
    src = dict(viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center)
    return {n: src[n].to(_dev()).clone().requires_grad_(n in want) for n in R.NAMES}


def settings(cam, bg, camt, sh_degree=1):
    from splatco_amd.rasterizer import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=torch.as_tensor(bg, dtype=torch.float32, device=_dev()), scale_modifier=1.0,
        viewmatrix=camt["viewmatrix"], projmatrix=camt["projmatrix"], sh_degree=sh_degree, campos=camt["campos"],
        prefiltered=False, debug=False)


def gaussian_inputs(g, shs=None, cov=None, requires_grad=True):
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=_dev(), requires_grad=requires_grad)
    kw = dict(means3D=t(g["means3D"]), opacities=t(g["opacities"]),
              means2D=torch.zeros(g["means3D"].shape[0], 3, device=_dev(), requires_grad=requires_grad))
    if cov is None:
        kw.update(scales=t(g["scales"]), rotations=t(g["rotations"]))
    else:
        kw.update(cov3D_precomp=t(cov))
    kw.update(shs=t(shs)) if shs is not None else kw.update(colors_precomp=t(g["colors"]))
    return kw


def run(cam, g, G, want=R.NAMES, shs=None, cov=None, sh_degree=1, gaussians_require_grad=True, camt=None):
    """One forward + backward of <G, image>.  Returns dict(image, radii, camera gradients by name (None: no .grad),
    grads: per-Gaussian gradients)."""
    from splatco_amd.rasterizer import GaussianRasterizer
    camt = camt or camera_leaves(cam, want)
    kw = gaussian_inputs(g, shs, cov, gaussians_require_grad)
    img, radii = GaussianRasterizer(settings(cam, g["bg"], camt, sh_degree))(**kw)
    (img * G.to(_dev())).sum().backward()
    torch.cuda.synchronize()
    res = dict(image=img.detach(), radii=radii, grads={k: v.grad for k, v in kw.items()})
    res.update({n: camt[n].grad if camt[n].is_leaf else None for n in R.NAMES})
    return res


def check_camera(got, name, tag, names=R.NAMES):
    """The returned camera gradients of a named case against its float64 reference."""
    r64, _, e32 = R.reference(name)
    assert np.array_equal(got["radii"].cpu().numpy(), r64["radii"].numpy()), "radii differ from the reference's"
    errs = {n: rel_l2(got[n].cpu().numpy(), r64[n].numpy()) for n in names if r64[n].any()}
    print(f"[camera] {tag}: rel-L2 vs float64 " + ", ".join(f"{n} {e:.2e} (e32 {e32[n]:.2e}, bar {R.bar(e32[n]):.1e})"
                                                             for n, e in errs.items()))
    for n in names:
        assert got[n] is not None and got[n].shape == r64[n].shape and got[n].dtype == torch.float32, n
    assert torch.all(got["viewmatrix"][:, 3] == 0) if "viewmatrix" in names else True
    assert torch.all(got["projmatrix"][:, 2] == 0) if "projmatrix" in names else True
    for n in names:
        if not r64[n].any():
            assert torch.all(got[n] == 0), f"{n}: structural zeros"
        else:
            assert errs[n] <= R.bar(e32[n]), (n, errs[n])


# ------------------------------------------------------------------ 1: base case
@pytest.fixture(scope="module")
def base():
    cam, g, _ = R.case("base")
    return cam, g, R.weights(cam)[0], run(cam, g, R.weights(cam)[0])


def test_base_case(base):
    cam, g, G, got = base
    check_camera(got, "base", "base P=96")
    assert int((got["viewmatrix"][:, :3] != 0).sum()) == 12      # dense, but for the column the forward never reads
    assert int((got["projmatrix"][:, [0, 1, 3]] != 0).sum()) == 12
    plain = run(cam, g, G, want=())
    assert all(plain[n] is None for n in R.NAMES)
    assert torch.equal(got["image"], plain["image"]) and torch.equal(got["radii"], plain["radii"])
    for k, v in plain["grads"].items():
        assert v is not None and torch.equal(got["grads"][k], v), k


# ------------------------------------------------------------------ 2: workgroup edges
@pytest.mark.parametrize("P", R.EDGE_P)
def test_workgroup_edges(P):
    """One thread, a full workgroup less one, exactly one, one plus one thread, three workgroups with a ragged tail."""
    cam, g, _ = R.case(f"P={P}")
    got = run(cam, g, R.weights(cam)[0])
    check_camera(got, f"P={P}", f"P={P}")
    assert all(torch.isfinite(v).all() for v in got["grads"].values())


# ------------------------------------------------------------------ 3: clamped Jacobians
def test_clamped_jacobians():
    cam, g, _ = R.case("clamped")
    n = R.clamped_and_visible(cam, g, R.reference("clamped")[0]["radii"].numpy())
    print(f"[camera] clamped: {n} visible Gaussians with a clamped Jacobian")
    assert n >= 10
    check_camera(run(cam, g, R.weights(cam)[0]), "clamped", "clamped")


# ------------------------------------------------------------------ 4: many workgroups, few contributors
def test_many_workgroups_few_contributors():
    """P = 70 000: 274 rows of partial sums, 160 Gaussians that contribute; the rest are culled and change nothing, so the
    reference runs on the 160 alone."""
    cam, g, rows = R.scattered_scene()
    assert rows[0] == 0 and rows[-1] == 70000 - 1 and (70000 + 255) // 256 == 274
    got = run(cam, g, R.weights(cam)[0])
    radii = got["radii"].cpu().numpy()
    culled = np.ones(70000, bool)
    culled[rows] = False
    assert not radii[culled].any()
    sub = dict(got, radii=got["radii"][torch.as_tensor(rows, device=_dev())])
    check_camera(sub, "subset160", "P=70000, 160 visible")
    sel = torch.as_tensor(culled, device=_dev())
    for k, v in got["grads"].items():
        assert torch.all(v[sel] == 0), k


# ------------------------------------------------------------------ 5: other input forms
@pytest.mark.parametrize("variant", ["shs", "shs_cov3D", "cov3D"])
def test_other_input_forms(variant):
    cam, g, extra = R.case(variant)
    got = run(cam, g, R.weights(cam)[0], **extra)
    check_camera(got, variant, variant)
    if "shs" in extra:
        assert float(got["campos"].abs().max()) > 0
    # the per-Gaussian gradients are those of the call without camera gradients
    plain = run(cam, g, R.weights(cam)[0], want=(), **extra)
    for k, v in plain["grads"].items():
        assert torch.equal(got["grads"][k], v), k


# ------------------------------------------------------------------ 6: with the maps
def test_with_the_maps():
    """return_aux=True, loss on image + depth + alpha, against two passes of the colour-only operator (the construction of
    test_gpu_aux_maps.py::two_pass): the second pass renders the colours (z, 1, 0) over black, z formed in torch from the same
    leaf V, so that autograd adds the depth path's sum dL/dz (p, 1) into V.grad."""
    from splatco_amd.rasterizer import GaussianRasterizer
    cam, g, _ = R.case("base")
    G = [w.to(_dev()) for w in R.weights(cam)]
    # fused
    ct = camera_leaves(cam)
    kw = gaussian_inputs(g)
    img, radii, depth, alpha = GaussianRasterizer(settings(cam, g["bg"], ct))(return_aux=True, **kw)
    ((img * G[0]).sum() + (depth * G[1]).sum() + (alpha * G[2]).sum()).backward()
    # two passes
    c2 = camera_leaves(cam)
    kw2 = gaussian_inputs(g)
    img2, radii2 = GaussianRasterizer(settings(cam, g["bg"], c2))(**kw2)
    V = c2["viewmatrix"]
    z = kw2["means3D"] @ V[:3, 2] + V[3, 2]
    kz = {k: v for k, v in kw2.items() if k != "colors_precomp"}
    kz["colors_precomp"] = torch.stack((z, torch.ones_like(z), torch.zeros_like(z)), dim=1)
    aux, radii3 = GaussianRasterizer(settings(cam, np.zeros(3, np.float32), c2))(**kz)
    ((img2 * G[0]).sum() + (aux[0] * G[1]).sum() + (aux[1] * G[2]).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(radii, radii2) and torch.equal(radii, radii3) and torch.equal(img, img2)
    errs = {n: rel_l2(ct[n].grad.cpu().numpy(), c2[n].grad.cpu().numpy()) for n in ("viewmatrix", "projmatrix")}
    errs["means3D"] = rel_l2(kw["means3D"].grad.cpu().numpy(), kw2["means3D"].grad.cpu().numpy())
    print("[camera] with the maps: rel-L2 vs two passes " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert float(c2["viewmatrix"].grad.abs().max()) > 0
    for n, e in errs.items():
        assert e <= R.GRAD_TOL, (n, e)
    assert torch.all(ct["viewmatrix"].grad[:, 3] == 0) and torch.all(ct["projmatrix"].grad[:, 2] == 0)
    assert torch.all(ct["campos"].grad == 0)
    # the depth path is in it: the image-only loss gives another dL/dviewmatrix
    assert rel_l2(ct["viewmatrix"].grad.cpu().numpy(), R.reference("base")[0]["viewmatrix"].numpy()) > 1e-2


# ------------------------------------------------------------------ 7: subsets
def test_subsets(base):
    cam, g, G, full = base
    only_v = run(cam, g, G, want=("viewmatrix",), gaussians_require_grad=False)
    assert all(v is None for v in only_v["grads"].values())
    assert only_v["projmatrix"] is None and only_v["campos"] is None
    check_camera(only_v, "base", "only viewmatrix", names=("viewmatrix",))
    assert torch.equal(only_v["viewmatrix"], full["viewmatrix"])
    only_m = run(cam, g, G, want=("projmatrix",))
    assert only_m["viewmatrix"] is None and only_m["campos"] is None
    check_camera(only_m, "base", "only projmatrix", names=("projmatrix",))
    assert torch.equal(only_m["projmatrix"], full["projmatrix"])
    # a transposed, non-contiguous view of a leaf
    camt = camera_leaves(cam, want=())
    leaf = cam.world_view_transform.t().contiguous().to(_dev()).requires_grad_()
    camt["viewmatrix"] = leaf.t()
    assert not camt["viewmatrix"].is_contiguous()
    run(cam, g, G, camt=camt)
    assert leaf.grad is not None and leaf.grad.shape == (4, 4)
    assert torch.equal(leaf.grad.t(), full["viewmatrix"])


# ------------------------------------------------------------------ 8: determinism
def test_determinism():
    """274 rows of partial sums, every one of them in use: two backward calls leave the same bits."""
    from splatco_amd.rasterizer import GaussianRasterizer
    P = 70000
    cam, g = small_scene(P=P, spread=0.3, W=70, H=52)
    shs = (np.random.default_rng(5).standard_normal((P, 4, 3)) * 0.4).astype(np.float32)
    G = R.weights(cam)[0].to(_dev())
    outs = []
    for _ in range(2):
        camt = camera_leaves(cam)
        kw = gaussian_inputs(g, shs=shs)
        img, radii = GaussianRasterizer(settings(cam, g["bg"], camt))(**kw)
        loss = (img * G).sum()
        leaves = [camt[n] for n in R.NAMES]
        outs.append(torch.autograd.grad(loss, leaves, retain_graph=True))      # the same saved state, twice
        outs.append(torch.autograd.grad(loss, leaves))
    torch.cuda.synchronize()
    print(f"[camera] determinism: {int((radii > 0).sum())} of {P} visible")
    assert int((radii > 0).sum()) == P
    for o in outs[1:]:
        for n, a, b in zip(R.NAMES, outs[0], o):
            assert torch.isfinite(a).all() and float(a.abs().max()) > 0, n
            assert torch.equal(a, b), n


# ------------------------------------------------------------------ 9: no Gaussians
def test_no_gaussians():
    from splatco_amd.rasterizer import GaussianRasterizer
    cam, g, _ = R.case("base")
    camt = camera_leaves(cam)
    e = lambda *s: torch.zeros(*s, device=_dev(), requires_grad=True)
    img, radii = GaussianRasterizer(settings(cam, g["bg"], camt))(
        means3D=e(0, 3), means2D=e(0, 3), opacities=e(0, 1), colors_precomp=e(0, 3), scales=e(0, 3), rotations=e(0, 4))
    (img * R.weights(cam)[0].to(_dev())).sum().backward()
    for n in R.NAMES:
        assert camt[n].grad is not None and camt[n].grad.shape == camt[n].shape and torch.all(camt[n].grad == 0), n


def test_every_gaussian_culled():
    """P > 0 but no tile instance (all 300 Gaussians behind the camera): the blend backward does not run, and the camera
    gradients are zeros, not what the buffers held."""
    cam, g, _ = R.case("clamped")
    g = dict(g, means3D=g["means3D"] + np.array([0.6, -0.4, -9.0], np.float32))
    got = run(cam, g, R.weights(cam)[0], shs=R.sh_coefficients(300)[:, :4].copy())
    assert not got["radii"].any()
    for n in R.NAMES:
        assert got[n] is not None and torch.all(got[n] == 0), n
    assert all(torch.all(v == 0) for v in got["grads"].values())


# ------------------------------------------------------------------ 10: render() end to end
def test_render_with_a_pose_delta_camera():
    """xi.grad through render() = the chain rule applied by hand, in float64, to the gradients the rasterizer operator
    returned for its three camera tensors and the helper's Jacobian."""
    from test_gpu_renderer import _model
    from splatco_amd.cameras import look_at_camera, pose_delta_camera
    from splatco_amd.renderer import prefilter_voxel, render
    dev = _dev()
    pc, _ = _model(dev)
    base_cam = look_at_camera(eye=(0.3, -0.2, -4.5), target=(0, 0, 0), up=(0, -1, 0), FoVx=math.radians(60), width=200,
                              height=120)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False, mv=4)
    bg = torch.tensor([1.0, 1.0, 1.0], device=dev)
    pc.train()
    gen = torch.Generator(device="cpu").manual_seed(3)
    xi0 = (torch.rand(6, generator=gen) - 0.5) * 0.06
    target = torch.rand(3, 120, 200, generator=gen).to(dev)
    xi = xi0.clone().to(dev).requires_grad_()
    cam = pose_delta_camera(base_cam, xi)
    assert cam.world_view_transform.device == xi.device and cam.world_view_transform.dtype == torch.float32
    # what the operator receives: copies nothing else reads, so that their .grad is the operator's own result
    seen = [t.clone() for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]
    for t in seen:
        t.retain_grad()
    cam = dataclasses.replace(cam, world_view_transform=seen[0], full_proj_transform=seen[1], camera_center=seen[2])
    vis = prefilter_voxel(cam, pc, pipe, bg)
    out = render(cam, pc, pipe, bg, visible_mask=vis)
    ((out["render"] - target) ** 2).mean().backward()
    torch.cuda.synchronize()
    assert xi.grad is not None and torch.isfinite(xi.grad).all() and float(xi.grad.abs().max()) > 0
    assert seen[0].grad is not None and seen[1].grad is not None
    assert pc._anchor.grad is not None and float(pc._anchor.grad.abs().sum()) > 0
    # campos reaches the image through the MLP heads only, where it is a constant: no gradient (colors_precomp)
    assert seen[2].grad is None or torch.all(seen[2].grad == 0)
    from splatco_amd.cameras import pose_tensors
    jac = torch.autograd.functional.jacobian(lambda x: tuple(t.reshape(-1) for t in pose_tensors(base_cam, x)), xi0)
    want = sum(j.double().t() @ (torch.zeros(j.shape[0], dtype=torch.float64) if t.grad is None
                                 else t.grad.detach().cpu().double().reshape(-1)) for j, t in zip(jac, seen))
    err = rel_l2(xi.grad.cpu().numpy(), want.numpy())
    print(f"[camera] render(): xi.grad {xi.grad.cpu().numpy()}, rel-L2 vs the float64 chain rule {err:.2e}")
    assert err <= 1e-5


# ------------------------------------------------------------------ 11: pose recovery
def test_pose_recovery_on_the_raw_operator():
    """The image at xi = 0 is the target; from xi = (0.02, -0.015, 0.01, 0.03, -0.02, 0.04) 150 Adam steps at lr 2e-3 on the
    mean squared error must bring the loss down 100x and |xi| down 3x (the float32 torch_ref with the same helper:
    4.2e-3 -> 1.8e-6 and 0.060 -> 0.008)."""
    from splatco_amd.cameras import pose_delta_camera
    from splatco_amd.rasterizer import GaussianRasterizer
    cam, g, _ = R.case("recovery")
    kw = gaussian_inputs(g, requires_grad=False)

    def image(xi):
        c = pose_delta_camera(cam, xi)
        camt = dict(viewmatrix=c.world_view_transform.to(_dev()), projmatrix=c.full_proj_transform.to(_dev()),
                    campos=c.camera_center.to(_dev()))
        return GaussianRasterizer(settings(cam, g["bg"], camt))(**kw)[0]

    with torch.no_grad():
        target = image(torch.zeros(6))
    xi = torch.tensor([0.02, -0.015, 0.01, 0.03, -0.02, 0.04], requires_grad=True)
    opt = torch.optim.Adam([xi], lr=2e-3)
    first = None
    for _ in range(150):
        opt.zero_grad()
        loss = ((image(xi) - target) ** 2).mean()
        loss.backward()
        first = float(loss.detach()) if first is None else first
        opt.step()
    with torch.no_grad():
        last = float(((image(xi) - target) ** 2).mean())
    n0, n1 = float(torch.tensor([0.02, -0.015, 0.01, 0.03, -0.02, 0.04]).norm()), float(xi.detach().norm())
    print(f"[camera] pose recovery: loss {first:.2e} -> {last:.2e} ({first / max(last, 1e-30):.0f}x), "
          f"|xi| {n0:.3f} -> {n1:.4f} ({n0 / max(n1, 1e-30):.1f}x)")
    assert last * 100 <= first and n1 * 3 <= n0
