"""GPU tests of the depth-map normals: splatco_amd.normals.depth_normals / normal_loss (csrc/normals.hip) against the float64
restatement of their definition (tests/normals_ref.py), through the rasterizer's maps, and through collaborative_step.

Kernel constants (csrc/normals.hip): a workgroup of 256 lanes owns a tile of NM_TX x NM_TY = 128 x 8 pixels, each lane a quad of
four pixels of one row; z is staged with a halo of 1 (forward) or 2 (backward) rows and one quad of columns; 16-byte row
accesses where W % 4 == 0, guarded dword accesses otherwise; the loss writes one record per tile and the fold workgroup has
NM_FOLD = 1024 lanes, lane t adding records t, t + 1024, ...  Shapes:
  1 x 1, 1 x 9, 9 x 1, 2 x 9     all holes: loss 0, every output exactly zero
  3 x 3                          one valid pixel
  52 x 70, 70 x 133              the aux tests' shape and an odd one (neither width a multiple of 4; two tiles across, nine down)
  10 x {127, 128, 129, 130}      widths around NM_TX at height NM_TY + 2: the halo crosses the tile border on the left and right
  {7, 8, 9, 10} x 130            heights around NM_TY at width NM_TX + 2: the same above and below (10 x 130 is in both rows)
  8200 x 3                       1025 tiles: a fold lane's second trip (8200 x 4 among the extra cases: the 16-byte path)

Inputs: the recipe of tests/normals_ref.py, seed 0.  Each test asserts its preconditions on the float64 reference: for shapes
with an interior of 9 pixels or more at least 40 % of the interior pixels valid and min c.c over the valid pixels > 1e-12, and
the float32 chain has the same valid set.

Bars: n, dD, dA and the map's gradients under a random upstream [3, H, W] by rel-L2, max(1.5 x the float32 torch chain's own
error against the same float64 result, 2e-6) -- the constants of test_gpu_depth_loss.py.  L by absolute error,
max(1.5 x the chain's absolute error, 16 2^-24 sum_valid m / (H W)): every term is 1 - n.n^ with n.n^ near 1, so its absolute
error is a handful of float32 roundings of 1 whatever the size of the term.  n_valid, zeros at holes, zeros away from valid
pixels and run-to-run bits are exact.  Every figure is printed before it is asserted (and appended to the file
$SPLATCO_NORMALS_LOG names, if set); profiles/r18_normals.txt holds one such run.
"""
import functools
import math
import os
import types

import numpy as np
import pytest
import torch

import normals_ref as ref
import splatco_amd.normals                    # noqa: F401  (the module under test: without it nothing here can run)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C_CHAIN, FLOOR = 1.5, 2e-6
TX, TY, FOLD = 128, 8, 1024
HOLES = [(1, 1), (1, 9), (9, 1), (2, 9)]
SHAPES = ([(3, 3), (52, 70), (70, 133)] + [(TY + 2, w) for w in (TX - 1, TX, TX + 1, TX + 2)] +
          [(h, TX + 2) for h in (TY - 1, TY, TY + 1)] + [(TY * (FOLD + 1), 3)])
MASKS = (None, "f32", "u8", "bool")


def _log(line):
    print(line)
    path = os.environ.get("SPLATCO_NORMALS_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _camera(H, W):
    """A camera of the recipe's intrinsics (FoVx 60 degrees, square pixels) looking obliquely: a rotation with no zero entry."""
    from splatco_amd.cameras import look_at_camera
    return look_at_camera(eye=(0.3, -0.2, 0.1), target=(1.0, 0.7, -0.4), up=(0, -1, 0), FoVx=math.radians(60), width=W, height=H).to(
        torch.device(DEV))


@functools.lru_cache(maxsize=None)
def _inputs(H, W, mk):
    return ref.recipe(H, W, 0, device=DEV, mask_kind=mk)


def _upstream(H, W):
    return torch.randn(3, H, W, generator=torch.Generator().manual_seed(7), dtype=torch.float64).to(DEV)


@functools.lru_cache(maxsize=None)
def _loss_refs(H, W, mk):
    """(float64 reference, float32 chain) of the loss on the device, each with its gradient maps; computed once per case."""
    D, A, prior, mask, intr = _inputs(H, W, mk)
    out = []
    for dtype in (torch.float64, torch.float32):
        D_, A_ = D.clone().requires_grad_(), A.clone().requires_grad_()
        r = ref.normal_loss_ref(D_, A_, prior, intr, mask, dtype=dtype)
        r["dD"], r["dA"] = torch.autograd.grad(r["loss"], (D_, A_))
        out.append({k: (v.detach() if torch.is_tensor(v) else v) for k, v in r.items()})
    return out


@functools.lru_cache(maxsize=None)
def _map_refs(H, W, world):
    D, A, _, _, _ = _inputs(H, W, None)
    from splatco_amd.normals import intrinsics
    cam = _camera(H, W)
    rot = cam.world_view_transform[:3, :3] if world else None
    G = _upstream(H, W)
    out = []
    for dtype in (torch.float64, torch.float32):
        D_, A_ = D.clone().requires_grad_(), A.clone().requires_grad_()
        r = ref.normals_ref(D_, A_, intrinsics(cam), dtype=dtype, rot=rot)
        r["dD"], r["dA"] = torch.autograd.grad((r["n"] * G.to(dtype)).sum(), (D_, A_))
        out.append({k: v.detach() for k, v in r.items()})
    return out


def _preconditions(case, H, W, r64, r32):
    assert torch.equal(r64["valid"], r32["valid"]), (case, "the float32 chain has another valid set")
    if (H - 2) * (W - 2) >= 9:
        frac = float(r64["valid"][1:-1, 1:-1].double().mean())
        cc = float(r64["cc"][r64["valid"]].min())
        assert frac >= 0.40, (case, frac)
        assert cc > 1e-12, (case, cc)
        return frac, cc
    return float("nan"), float("nan")


def _fused_loss(D, A, prior, intr, mask, g_up=None, min_alpha=0.5):
    from splatco_amd.normals import normal_loss
    D_, A_ = D.detach().clone().requires_grad_(), A.detach().clone().requires_grad_()
    loss, stats = normal_loss(D_, A_, prior, intr, mask, min_alpha=min_alpha, return_stats=True)
    assert loss.is_cuda and stats.is_cuda and loss.dtype == torch.float32 and stats.shape == (1,) and not stats.requires_grad
    dD, dA = torch.autograd.grad(loss, (D_, A_), grad_outputs=g_up)
    return loss.detach(), stats, dD, dA


def _fused_map(D, A, cam, frame, G):
    from splatco_amd.normals import depth_normals
    D_, A_ = D.detach().clone().requires_grad_(), A.detach().clone().requires_grad_()
    n, valid = depth_normals(D_, A_, cam, frame=frame, return_valid=True)
    assert n.is_cuda and n.dtype == torch.float32 and n.shape == (3,) + D.shape and valid.dtype == torch.bool
    dD, dA = torch.autograd.grad(n, (D_, A_), grad_outputs=G.float())
    return n.detach(), valid, dD, dA


def _bars(case, rows):
    failed = []
    for name, e, e_chain, floor in rows:
        bar = max(C_CHAIN * e_chain, floor)
        _log(f"normals {case:36s} {name:6s} e {e:9.3e}  e_chain {e_chain:9.3e}  bar {bar:9.3e}{'' if e <= bar else '   <-- FAIL'}")
        if not e <= bar:
            failed.append(name)
    assert not failed, (case, failed)


def _check_loss(H, W, mk):
    D, A, prior, mask, intr = _inputs(H, W, mk)
    r64, r32 = _loss_refs(H, W, mk)
    case = f"loss {H}x{W} mask={mk}"
    frac, cc = _preconditions(case, H, W, r64, r32)
    assert torch.equal(r64["good"], r32["good"]), case
    n = int(r64["n_valid"])
    loss, stats, dD, dA = _fused_loss(D, A, prior, intr, mask)
    again = _fused_loss(D, A, prior, intr, mask)
    torch.cuda.synchronize()
    for a, b in zip((loss, stats, dD, dA), again):
        assert torch.equal(a, b), (case, "two runs differ")
    _log(f"normals {case:36s} n_valid {n:6d} of {H * W:6d}  interior valid {frac:.3f}  min c.c {cc:.2e}  L {float(r64['loss']):.6e}")
    assert int(stats[0]) == n, (case, int(stats[0]), n)
    assert torch.isfinite(loss) and torch.isfinite(dD).all() and torch.isfinite(dA).all()
    far = ~ref.neighbourhood(r64["good"])
    assert not dD[far].any() and not dA[far].any(), (case, "a gradient away from every valid pixel")
    assert not dD[~r64["ok"]].any() and not dA[~r64["ok"]].any(), (case, "a gradient at a pixel that is not ok")
    if n == 0:
        assert float(loss) == 0.0 and not dD.any() and not dA.any()
        return
    floor_l = 16.0 * 2.0 ** -24 * r64["weight_sum"] / (H * W)
    _bars(case, [("L", abs(float(loss) - float(r64["loss"])), abs(float(r32["loss"]) - float(r64["loss"])), floor_l),
                 ("dD", _rel_l2(dD, r64["dD"]), _rel_l2(r32["dD"], r64["dD"]), FLOOR),
                 ("dA", _rel_l2(dA, r64["dA"]), _rel_l2(r32["dA"], r64["dA"]), FLOOR)])


def _check_map(H, W, frame):
    D, A, _, _, _ = _inputs(H, W, None)
    world = frame == "world"
    r64, r32 = _map_refs(H, W, world)
    case = f"map {H}x{W} {frame}"
    frac, cc = _preconditions(case, H, W, r64, r32)
    cam, G = _camera(H, W), _upstream(H, W)
    n, valid, dD, dA = _fused_map(D, A, cam, frame, G)
    again = _fused_map(D, A, cam, frame, G)
    torch.cuda.synchronize()
    for a, b in zip((n, valid, dD, dA), again):
        assert torch.equal(a, b), (case, "two runs differ")
    _log(f"normals {case:36s} valid {int(r64['valid'].sum()):6d} of {H * W:6d}  interior valid {frac:.3f}  min c.c {cc:.2e}")
    assert torch.equal(valid, r64["valid"]), case
    assert not n[:, ~r64["valid"]].any(), (case, "a hole's normal is not exactly zero")
    assert torch.isfinite(n).all() and torch.isfinite(dD).all() and torch.isfinite(dA).all()
    far = ~ref.neighbourhood(r64["valid"])
    assert not dD[far].any() and not dA[far].any(), (case, "a gradient away from every valid pixel")
    assert not dD[~r64["ok"]].any() and not dA[~r64["ok"]].any(), (case, "a gradient at a pixel that is not ok")
    if not r64["valid"].any():
        assert not dD.any() and not dA.any()
        return
    if not world:                                            # three float32 roundings of components <= 1
        assert float((n[:, r64["valid"]].double().norm(dim=0) - 1.0).abs().max()) <= 3.0 * 2.0 ** -24
    _bars(case, [("n", _rel_l2(n, r64["n"]), _rel_l2(r32["n"], r64["n"]), FLOOR),
                 ("dD", _rel_l2(dD, r64["dD"]), _rel_l2(r32["dD"], r64["dD"]), FLOOR),
                 ("dA", _rel_l2(dA, r64["dA"]), _rel_l2(r32["dA"], r64["dA"]), FLOOR)])


@pytest.mark.parametrize("mk", MASKS)
@pytest.mark.parametrize("H,W", HOLES + SHAPES)
def test_loss_parity_with_the_float64_restatement(H, W, mk):
    _check_loss(H, W, mk)


@pytest.mark.parametrize("frame", ("camera", "world"))
@pytest.mark.parametrize("H,W", HOLES + SHAPES)
def test_map_parity_with_the_float64_restatement(H, W, frame):
    _check_map(H, W, frame)


def test_parity_on_the_sixteen_byte_path_with_more_tiles_than_fold_lanes():
    """8200 x 4: W % 4 == 0 (float4 rows of one quad), 1025 records."""
    _check_loss(TY * (FOLD + 1), 4, "f32")
    _check_map(TY * (FOLD + 1), 4, "world")


@pytest.mark.parametrize("mk", MASKS)
@pytest.mark.parametrize("H,W", [(52, 70), (70, 133)])
def test_loss_gradients_at_the_floor_where_the_prior_lies_far_from_the_normal(H, W, mk):
    """The recipe's prior lies within 0.3 (U - .5)^3 of n, so the float32 chain loses 1e-5 and more in the loss gradients and the
    bars above are that wide.  With the prior tilted by (0.5, -0.4, 0.3) the chain's error is that of n (7.6e-7 at 52 x 70,
    1.2e-6 at 70 x 133, measured on the host), and the same rule puts the bar of the loss backward -- the scale, the mask, the
    prior's normalisation -- at or next to the 2e-6 floor.  Precondition: the chain's own error is <= 2e-6, so no bar exceeds 3e-6."""
    D, A, prior, mask, intr = _inputs(H, W, mk)
    prior = prior + torch.tensor([0.5, -0.4, 0.3], device=DEV).reshape(3, 1, 1)
    refs = []
    for dtype in (torch.float64, torch.float32):
        D_, A_ = D.clone().requires_grad_(), A.clone().requires_grad_()
        r = ref.normal_loss_ref(D_, A_, prior, intr, mask, dtype=dtype)
        refs.append((r, *torch.autograd.grad(r["loss"], (D_, A_))))
    (r64, dD64, dA64), (r32, dD32, dA32) = refs
    assert torch.equal(r64["good"], r32["good"]) and int(r64["n_valid"]) >= 1000
    chain = _rel_l2(dD32, dD64), _rel_l2(dA32, dA64)
    assert max(chain) <= 2e-6, chain
    loss, stats, dD, dA = _fused_loss(D, A, prior, intr, mask)
    assert int(stats[0]) == int(r64["n_valid"])
    _bars(f"loss {H}x{W} mask={mk} tilted prior",
          [("L", abs(float(loss) - float(r64["loss"].detach())), abs(float(r32["loss"].detach()) - float(r64["loss"].detach())),
            16.0 * 2.0 ** -24 * r64["weight_sum"] / (H * W)),
           ("dD", _rel_l2(dD, dD64), chain[0], FLOOR), ("dA", _rel_l2(dA, dA64), chain[1], FLOOR)])


def test_all_hole_shapes_give_exact_zeros():
    for H, W in HOLES:
        D, A, prior, mask, intr = _inputs(H, W, "f32")
        loss, stats, dD, dA = _fused_loss(D, A, prior, intr, mask)
        n, valid, mD, mA = _fused_map(D, A, _camera(H, W), "world", _upstream(H, W))
        assert float(loss) == 0.0 and int(stats[0]) == 0 and not valid.any()
        for t in (dD, dA, n, mD, mA):
            assert not t.any()


def test_upstream_gradient_is_read_from_device_memory_and_scales_the_maps():
    """g_up = 0: both maps all zero.  g_up = -2.5: the float64 reference's maps times -2.5, at the parity bar."""
    D, A, prior, mask, intr = _inputs(52, 70, "f32")
    r64, r32 = _loss_refs(52, 70, "f32")
    _, _, zD, zA = _fused_loss(D, A, prior, intr, mask, g_up=torch.zeros((), device=DEV))
    assert not zD.any() and not zA.any()
    _, _, dD, dA = _fused_loss(D, A, prior, intr, mask, g_up=torch.full((), -2.5, device=DEV))
    _bars("loss 52x70 g_up=-2.5", [("dD", _rel_l2(dD, -2.5 * r64["dD"]), _rel_l2(r32["dD"], r64["dD"]), FLOOR),
                                   ("dA", _rel_l2(dA, -2.5 * r64["dA"]), _rel_l2(r32["dA"], r64["dA"]), FLOOR)])
    # one gradient map at a time: the other pointer is NULL
    from splatco_amd.normals import normal_loss
    only = D.clone().requires_grad_()
    normal_loss(only, A, prior, intr, mask).backward()
    assert torch.equal(only.grad, _fused_loss(D, A, prior, intr, mask)[2])


def _plant(D, A, prior, good):
    """NaN / Inf / negative values into pixels that carried a term: D and A of some (the pixel stops being ok: it and its four
    neighbours become holes), the prior of others (only that pixel becomes a hole of the loss).  Returns the maps and the two
    lists of flat indices."""
    shape = D.shape
    W = shape[1]
    D, A, prior = D.flatten().cpu().clone(), A.flatten().cpu().clone(), prior.reshape(3, -1).cpu().clone()
    idx = iter(good.flatten().cpu().nonzero().flatten().tolist()[5::23])
    nan, inf = float("nan"), float("inf")
    not_ok, no_prior = [], []
    for x, vals in ((D, (nan, inf, -inf, 0.0, -1.5)), (A, (nan, inf, -inf, -0.7, 0.4999))):
        for v in vals:
            i = next(idx)
            x[i] = v
            not_ok.append(i)
    i = next(idx)
    D[i], A[i], prior[:, i] = nan, -inf, inf
    not_ok.append(i)
    for c, v in ((0, nan), (1, inf), (2, -inf)):
        i = next(idx)
        prior[c, i] = v
        no_prior.append(i)
    i = next(idx)
    prior[:, i] = 0.0                                        # squared length <= 1e-24
    no_prior.append(i)
    return D.reshape(shape).to(DEV), A.reshape(shape).to(DEV), prior.reshape(3, *shape).to(DEV), not_ok, no_prior, W


def test_nan_inf_and_negative_values_in_holes_go_nowhere():
    """The planted maps give the bits of clean maps in which the same pixels are made holes by hand (alpha 0.2, mask 0), finite
    everywhere, and validity changes exactly as the reference says: the planted pixel and its four neighbours."""
    H, W = 52, 70
    D0, A0, prior0, mask0, intr = _inputs(H, W, "f32")
    clean64 = _loss_refs(H, W, "f32")[0]
    D, A, prior, not_ok, no_prior, _ = _plant(D0, A0, prior0, clean64["good"])
    assert len(not_ok) == 11 and len(no_prior) == 4
    loss, stats, dD, dA = _fused_loss(D, A, prior, intr, mask0)
    for t in (loss, stats, dD, dA):
        assert torch.isfinite(t).all()
    # by hand: the same pixels, not ok by a clean alpha / masked out
    A_hand, m_hand = A0.clone().flatten(), mask0.clone().flatten()
    A_hand[not_ok] = 0.2
    m_hand[no_prior] = 0.0
    want = _fused_loss(D0, A_hand.reshape(H, W), prior0, intr, m_hand.reshape(H, W))
    for a, b in zip((loss, stats, dD, dA), want):
        assert torch.equal(a, b)
    r = ref.normal_loss_ref(D, A, prior, intr, mask0)
    assert int(stats[0]) == int(r["n_valid"]) < int(clean64["n_valid"])
    flat = lambda t: t.flatten()
    assert not flat(dD)[not_ok].any() and not flat(dA)[not_ok].any()
    # the map: validity is lost at the planted pixels and their four neighbours, nowhere else
    cam = _camera(H, W)
    n, valid, mD, mA = _fused_map(D, A, cam, "camera", _upstream(H, W))
    n0, valid0, _, _ = _fused_map(D0, A0, cam, "camera", _upstream(H, W))
    assert torch.isfinite(n).all() and torch.isfinite(mD).all() and torch.isfinite(mA).all()
    lost = torch.zeros(H * W, dtype=torch.bool, device=DEV)
    for i in not_ok:
        for j in (i, i - 1, i + 1, i - W, i + W):
            lost[j] = True
    assert torch.equal(valid, valid0 & ~lost.reshape(H, W)) and torch.equal(valid, r["valid"])
    assert torch.equal(n[:, valid], n0[:, valid]) and not n[:, ~valid].any()


def test_wrapper_converts_its_operands_and_falls_back_where_the_prior_wants_a_gradient():
    from splatco_amd.normals import depth_normals, normal_loss
    D, A, prior, mask, intr = _inputs(52, 70, "f32")
    want = normal_loss(D, A, prior, intr, mask)
    assert torch.equal(normal_loss(D.t().contiguous().t(), A.double(), prior.double(), intr, mask), want)
    with pytest.raises(ValueError, match="prior"):
        normal_loss(D, A, prior.cpu(), intr, mask)
    # an integer mask of any width is nonzero = 1, negative entries included, on the device as in the torch path
    as_bool = normal_loss(D, A, prior, intr, mask > 0)
    for dtype in (torch.int32, torch.int64, torch.int8):
        signed = torch.where(mask > 0, -3, 0).to(dtype)
        assert torch.equal(normal_loss(D, A, prior, intr, signed), as_bool)
    assert torch.equal(normal_loss(D.cpu(), A.cpu(), prior.cpu(), intr, torch.where(mask > 0, -3, 0).cpu()),
                       normal_loss(D.cpu(), A.cpu(), prior.cpu(), intr, (mask > 0).cpu()))
    p_ = prior.clone().requires_grad_()
    loss = normal_loss(D, A, p_, intr, mask)
    loss.backward()
    assert p_.grad is not None and p_.grad.abs().sum() > 0
    r64 = _loss_refs(52, 70, "f32")[0]
    assert abs(float(loss.detach()) - float(r64["loss"])) <= 16.0 * 2.0 ** -24 * r64["weight_sum"] / (52 * 70) + 1.5 * abs(
        float(_loss_refs(52, 70, "f32")[1]["loss"]) - float(r64["loss"]))
    # the intrinsics of a camera and the tuple are the same thing
    cam = _camera(52, 70)
    from splatco_amd.normals import intrinsics
    assert torch.equal(depth_normals(D, A, cam), depth_normals(D, A, intrinsics(cam)))


# ------------------------------------------------------------------ through the rasterizer
def _scene():
    from splatco_amd.rasterizer import GaussianRasterizationSettings
    from splatco_amd.synthetic import synthetic_camera, synthetic_gaussians
    W, H, P = 70, 52, 400
    cam, g = synthetic_camera(W, H), synthetic_gaussians(P, W, H, seed=11)
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.tensor(g["bg"], device=DEV), 1.0,
                                       cam.world_view_transform.to(DEV), cam.full_proj_transform.to(DEV), 1,
                                       cam.camera_center.to(DEV), False, False)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV).requires_grad_()
    kw = dict(means3D=t(g["means3D"]), opacities=t(g["opacities"]), colors_precomp=t(g["colors"]), scales=t(g["scales"]),
              rotations=t(g["rotations"]))
    return cam, rs, kw


def test_gradients_through_the_rasterizer_match_the_float64_gradient_maps_pushed_through_it():
    """The aux tests' scene (70 x 52, 400 Gaussians).  The prior is the scene's own float64 normal plus a fixed tilt and noise.
    The gradients of the fused loss with respect to means3D, opacities and scales against the float64 reference's dD, dA pushed
    through the same rasterizer backward; the yardstick is the float32 chain's dD, dA pushed through likewise."""
    from splatco_amd.normals import intrinsics, normal_loss
    from splatco_amd.rasterizer import GaussianRasterizer
    cam, rs, kw = _scene()
    m2d = torch.zeros(kw["means3D"].shape[0], 3, device=DEV, requires_grad=True)
    img, radii, depth, alpha = GaussianRasterizer(rs)(means2D=m2d, return_aux=True, **kw)
    intr, min_alpha = intrinsics(cam), 0.25
    D, A = depth.detach(), alpha.detach()
    n0 = ref.normals_ref(D, A, intr, min_alpha)
    noise = torch.randn(3, 52, 70, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(DEV)
    prior = (n0["n"] + torch.tensor([0.2, -0.1, -0.3], dtype=torch.float64, device=DEV).reshape(3, 1, 1) + 0.1 * noise).float()
    maps = []
    for dtype in (torch.float64, torch.float32):
        D_, A_ = D.clone().requires_grad_(), A.clone().requires_grad_()
        r = ref.normal_loss_ref(D_, A_, prior, intr, None, min_alpha, dtype=dtype)
        maps.append((r, *torch.autograd.grad(r["loss"], (D_, A_))))
    (r64, dD64, dA64), (r32, dD32, dA32) = maps
    n = int(r64["n_valid"])
    _log(f"normals rasterizer 52x70: n_valid {n}, min c.c {float(r64['cc'][r64['valid']].min()):.3e}, L {float(r64['loss']):.6e}")
    assert n >= 64 and float(r64["cc"][r64["valid"]].min()) > 1e-12 and torch.equal(r64["valid"], r32["valid"])
    names = ("means3D", "opacities", "scales")
    leaves = [kw[k] for k in names]
    fused, stats = normal_loss(depth, alpha, prior, cam, min_alpha=min_alpha, return_stats=True)
    assert int(stats[0]) == n
    g_fused = torch.autograd.grad(fused, leaves, retain_graph=True)
    push = lambda dD, dA: torch.autograd.grad((depth, alpha), leaves, grad_outputs=(dD.float(), dA.float()), retain_graph=True)
    g_ref, g_chain = push(dD64, dA64), push(dD32, dA32)
    rows = [("L", abs(float(fused) - float(r64["loss"])), abs(float(r32["loss"]) - float(r64["loss"])), 16.0 * 2.0 ** -24 * n / (52 * 70))]
    for name, a, b, c in zip(names, g_fused, g_ref, g_chain):
        assert float(b.norm()) > 0, name
        rows.append(("d" + name[:5], _rel_l2(a, b), _rel_l2(c, b), FLOOR))
    _bars("rasterizer 52x70", rows)


# ------------------------------------------------------------------ through the training step
def _step_scene():
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.synthetic import synthetic_anchor_model
    W, H = 160, 96
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    bg = torch.ones(3, device=DEV)
    cams = [look_at_camera(eye=(0.0, 0.0, 0.0), target=(x, 0.0, 0.0), up=(0, -1, 0), FoVx=math.radians(60), width=W, height=H,
                           uid=i).to(torch.device(DEV)) for i, x in enumerate((1.0, -1.0))]
    gts = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(i)).to(DEV) for i in range(2)]
    make = lambda: synthetic_anchor_model(20_000, 7, torch.device(DEV), plane_size=64)
    return make, cams, gts, pipe, bg


OPTS = dict(min_alpha=0.2)


def _teacher(pc, cams, pipe, bg):
    """Normal priors tilted away from the model's own surface, and masks (where the model has a normal)."""
    from splatco_amd.normals import depth_normals
    from splatco_amd.renderer import prefilter_voxel, render
    targets, masks = [], []
    with torch.no_grad():
        for cam in cams:
            out = render(cam, pc, pipe, bg, visible_mask=prefilter_voxel(cam, pc, pipe, bg), aux=True)
            n, valid = depth_normals(out["depth"], out["alpha"], cam, return_valid=True, **OPTS)
            tilt = torch.tensor([0.3, 0.2, -0.5], device=DEV).reshape(3, 1, 1)
            targets.append(torch.where(valid, n + tilt, tilt.expand_as(n)).contiguous())
            masks.append(valid)
    return targets, masks


def _grads(pc):
    return {n: p.grad.detach().clone() for n, p in pc.named_parameters() if p.grad is not None}


def test_step_with_a_zero_normal_weight_leaves_the_parents_bits():
    from splatco_amd.train_step import collaborative_step
    make, cams, gts, pipe, bg = _step_scene()
    pc_a, pc_b, pc_c = make(), make(), make()
    targets, masks = _teacher(pc_c, cams, pipe, bg)
    loss_a, out_a, _ = collaborative_step(pc_a, cams, gts, pipe, bg)
    loss_b, out_b, _ = collaborative_step(pc_b, cams, gts, pipe, bg, normal_targets=None, normal_masks=None, normal_weight=0.0,
                                          normal_options=None)
    loss_c, out_c, _ = collaborative_step(pc_c, cams, gts, pipe, bg, normal_targets=targets, normal_masks=masks, normal_weight=0.0,
                                          normal_options=OPTS)
    assert "depth" not in out_b and "depth" not in out_c     # render() was called without aux
    ga, gb, gc = _grads(pc_a), _grads(pc_b), _grads(pc_c)
    assert len(ga) > 4 and set(ga) == set(gb) == set(gc)
    assert torch.equal(loss_a, loss_b) and torch.equal(loss_a, loss_c)
    for n in ga:
        assert torch.equal(ga[n], gb[n]) and torch.equal(ga[n], gc[n]), n
    for (na, pa), (nc, p_c) in zip(pc_a.named_parameters(), pc_c.named_parameters()):
        assert na == nc and torch.equal(pa, p_c), na


def test_step_with_a_normal_weight_equals_the_hand_written_loop_and_refuses_bad_lists():
    from splatco_amd.losses import view_loss
    from splatco_amd.normals import normal_loss
    from splatco_amd.renderer import prefilter_voxel, render
    from splatco_amd.train_step import collaborative_step
    make, cams, gts, pipe, bg = _step_scene()
    pc_s, pc_h = make(), make()
    targets, masks = _teacher(pc_h, cams, pipe, bg)
    masks[1] = None                                          # an entry may be absent
    loss_s, out_s, _ = collaborative_step(pc_s, cams, gts, pipe, bg, normal_targets=[t.cpu() for t in targets], normal_masks=masks,
                                          normal_weight=0.3, normal_options=OPTS)
    assert "depth" in out_s and "alpha" in out_s
    total, terms = None, []
    for cam, gt, tg, mk in zip(cams, gts, targets, masks):
        out = render(cam, pc_h, pipe, bg, visible_mask=prefilter_voxel(cam, pc_h, pipe, bg), retain_grad=True, aux=True)
        term, stats = normal_loss(out["depth"], out["alpha"], tg, cam, mk, return_stats=True, **OPTS)
        terms.append((float(term), int(stats[0])))
        loss = view_loss(out["render"], gt, out["scaling"]) + 0.3 * term
        total = loss if total is None else total + loss
    total.backward()
    _log(f"normals step 96x160: per-view (normal loss, n_valid) {terms}")
    assert all(t > 0 and n >= 64 for t, n in terms)
    # the bounds of test_gpu_depth_loss.py's step test: the same float32 kernels on the same inputs, composed twice
    assert abs(float(loss_s) - float(total)) <= 1e-6 * abs(float(total))
    gs, gh = _grads(pc_s), _grads(pc_h)
    assert len(gs) > 4 and set(gs) == set(gh)
    for n in gs:
        e = _rel_l2(gs[n], gh[n])
        assert e <= 1e-4, (n, e)
    # and the normal term did reach the anchors' gradients: the step without it differs
    pc_0 = make()
    collaborative_step(pc_0, cams, gts, pipe, bg)
    g0 = _grads(pc_0)
    assert any(not torch.equal(g0[n], gs[n]) for n in gs if n.startswith("_anchor") or n.startswith("_offset"))
    for kw in (dict(), dict(normal_targets=targets[:1]), dict(normal_targets=targets, normal_masks=masks + [None])):
        with pytest.raises(ValueError, match="normal_targets|normal_masks"):
            collaborative_step(pc_s, cams, gts, pipe, bg, normal_weight=0.3, **kw)
