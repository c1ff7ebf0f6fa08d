"""GPU tests of the depth term: splatco_amd.losses.depth_loss (csrc/depth_loss.hip) against the float64 restatement of its
definition (tests/depth_loss_ref.py), through the rasterizer's maps, and through collaborative_step.

Kernel constants (csrc/depth_loss.hip): a workgroup of 256 lanes owns DL_PER_WG = 4096 contiguous pixels and writes one
record; the fold workgroup has DL_FOLD = 1024 lanes (16 waves), lane t adding records t, t + 1024, ...  Shapes:
  1 x 1                         one pixel (one lane of one wave has work)
  1 x 4095, 1 x 4096, 1 x 4097  one below, at and above a workgroup's range (the last one: a second workgroup with one pixel)
  52 x 70                       the aux tests' shape (3640 pixels: a partly filled last round)
  513 x 512                     65 records: more than one wave's worth of records in the fold
  1 x 4194305                   1025 records: a fold lane's second trip (two cases only)

Inputs: the recipe of tests/depth_loss_ref.py (A = 0.05 + 0.95 U, z = 0.5 + 7.5 U, D = A z, g = 1.7 p - 0.08 +- u, u in
[0.05, 0.2], m in [0.25, 1.25) and zero on 20 %, min_alpha 0.5).  Without alignment the target's line is (1, 0), the one that
s = 1, t = 0 assumes: under 1.7 p - 0.08 the unaligned residual -0.7 p + 0.08 +- u crosses zero inside the recipe's range of p
at every size, so no seed satisfies the precondition below.  Each test asserts its preconditions on the float64 reference:
min |residual| > 1e-3 and, with alignment, at least 64 valid pixels.  With fewer than 64 valid pixels (1 x 1) the gradients are
compared without alignment; with alignment only finiteness, n_valid and the degenerate rule are checked.

Bar: max(1.5 x the float32 torch chain's own error against the same float64 result, 2e-6) -- 1.5 is the factor of
test_gpu_f64_parity.py, 2e-6 about 32 float32 roundings.  L, s, t by relative error, the gradient maps by rel-L2, holes exactly
zero.  Every figure is printed before it is asserted (and appended to the file $SPLATCO_DEPTH_LOSS_LOG names, if set);
profiles/r13_depth_loss.txt holds one such run.
"""
import math
import os
import types

import numpy as np
import pytest
import torch

from depth_loss_ref import depth_loss_ref, recipe, valid_pixels

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C_CHAIN, FLOOR = 1.5, 2e-6
SHAPES = [(1, 1), (1, 4095), (1, 4096), (1, 4097), (52, 70), (513, 512)]
COMBOS = [(mode, align, mk) for mode in ("inverse", "expected") for align in (True, False) for mk in (None, "f32", "u8", "bool")]


def _log(line):
    print(line)
    path = os.environ.get("SPLATCO_DEPTH_LOSS_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _rel(a, b):
    a, b = (float(x.detach()) if torch.is_tensor(x) else float(x) for x in (a, b))
    return abs(a - b) / max(abs(b), 1e-30)


def _rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _ref_pair(D, A, g, m, mode, align, min_alpha=0.5):
    """(float64 reference, float32 chain) on the device, each with its gradient maps."""
    out = []
    for dtype in (torch.float64, torch.float32):
        D_, A_ = D.detach().clone().requires_grad_(), A.detach().clone().requires_grad_()
        r = depth_loss_ref(D_, A_, g, m, mode, align, min_alpha, dtype=dtype)
        r["dD"], r["dA"] = torch.autograd.grad(r["loss"], (D_, A_))
        out.append(r)
    return out


def _fused(D, A, g, m, mode, align, g_up=None, min_alpha=0.5):
    from splatco_amd.losses import depth_loss
    D_, A_ = D.detach().clone().requires_grad_(), A.detach().clone().requires_grad_()
    loss, stats = depth_loss(D_, A_, g, m, mode=mode, align=align, min_alpha=min_alpha, return_stats=True)
    assert loss.is_cuda and stats.is_cuda and loss.dtype == torch.float32 and not stats.requires_grad
    if g_up is None:
        dD, dA = torch.autograd.grad(loss, (D_, A_))
    else:
        dD, dA = torch.autograd.grad(loss, (D_, A_), grad_outputs=g_up)
    return loss.detach(), stats, dD, dA


def _check_parity(H, W, mode, align, mk, seed=0):
    D, A, g, m = recipe(H, W, seed, device=DEV, mask_kind=mk, mode=mode, line=(1.7, -0.08) if align else (1.0, 0.0))
    ref, chain = _ref_pair(D, A, g, m, mode, align)
    n = int(ref["n_valid"])
    case = f"{H}x{W} {mode:8s} align={int(align)} mask={mk}"
    loss, stats, dD, dA = _fused(D, A, g, m, mode, align)
    loss2, stats2, dD2, dA2 = _fused(D, A, g, m, mode, align)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and torch.equal(stats, stats2) and torch.equal(dD, dD2) and torch.equal(dA, dA2)
    assert int(stats[2]) == n, (case, int(stats[2]), n)
    holes = ~ref["valid"]
    assert not dD[holes].any() and not dA[holes].any(), case
    assert torch.isfinite(loss) and torch.isfinite(stats).all() and torch.isfinite(dD).all() and torch.isfinite(dA).all()
    if align and n < 64:
        # too few pixels for a conditioned fit: the degenerate rule where it applies, nothing else
        if n < 2:
            assert stats[:2].tolist() == [1.0, 0.0] and float(ref["s"]) == 1.0 and float(ref["t"]) == 0.0
        _log(f"depth_loss {case:44s} n_valid {n}: finiteness, n_valid and the degenerate rule only")
        return
    assert n >= (64 if align else 1), (case, n)
    assert float(ref["residual"][ref["valid"]].abs().min()) > 1e-3, case
    rows = [("L", _rel(loss, ref["loss"]), _rel(chain["loss"], ref["loss"])),
            ("dD", _rel_l2(dD, ref["dD"]), _rel_l2(chain["dD"], ref["dD"])),
            ("dA", _rel_l2(dA, ref["dA"]), _rel_l2(chain["dA"], ref["dA"]))]
    if align:
        rows += [("s", _rel(stats[0], ref["s"]), _rel(chain["s"], ref["s"])), ("t", _rel(stats[1], ref["t"]), _rel(chain["t"], ref["t"]))]
    else:
        assert stats[:2].tolist() == [1.0, 0.0]
    failed = []
    for name, e, e_chain in rows:
        bar = max(C_CHAIN * e_chain, FLOOR)
        _log(f"depth_loss {case:44s} n_valid {n:7d} {name:2s} e {e:9.3e}  e_chain {e_chain:9.3e}  bar {bar:9.3e}{'' if e <= bar else '   <-- FAIL'}")
        if not e <= bar:
            failed.append(name)
    assert not failed, (case, failed)


@pytest.mark.parametrize("mode,align,mk", COMBOS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_parity_with_the_float64_restatement(H, W, mode, align, mk):
    _check_parity(H, W, mode, align, mk)


@pytest.mark.parametrize("mode,align,mk", [("inverse", True, "f32"), ("expected", False, "bool")])
def test_parity_where_a_fold_lane_takes_a_second_trip(mode, align, mk):
    _check_parity(1, 1024 * 4096 + 1, mode, align, mk)


@pytest.mark.parametrize("H,W", [(1, 4097), (513, 512)])
@pytest.mark.parametrize("align", (True, False))
def test_result_does_not_depend_on_what_scratch_and_outputs_held(H, W, align):
    """The C-ABI called directly, twice, on scratch / out4 / gradient maps pre-filled with NaN: the same bits, and the bits of
    the Python wrapper's call (whose buffers are torch.empty)."""
    from splatco_amd import _C
    D, A, g, m = recipe(H, W, 1, device=DEV, mask_kind="f32", line=(1.7, -0.08) if align else (1.0, 0.0))
    want = _fused(D, A, g, m, "inverse", align)
    nan = float("nan")
    g_up = torch.ones(1, device=DEV)
    got = []
    for _ in range(2):
        scratch = torch.full((_C.lib.scr_depth_loss_scratch_bytes(H, W) // 4,), nan, device=DEV)
        out = torch.full((4,), nan, device=DEV)
        dD, dA = torch.full_like(D, nan), torch.full_like(A, nan)
        with torch.cuda.device(DEV):
            _C.check(_C.lib.scr_depth_loss_forward(H, W, D.data_ptr(), A.data_ptr(), g.data_ptr(), m.data_ptr(), 1, 0, int(align), 0.5,
                                                   scratch.data_ptr(), out.data_ptr(), _C.stream(D.device)))
            _C.check(_C.lib.scr_depth_loss_backward(H, W, D.data_ptr(), A.data_ptr(), g.data_ptr(), m.data_ptr(), 1, 0, 0.5,
                                                    scratch.data_ptr(), g_up.data_ptr(), dD.data_ptr(), dA.data_ptr(), _C.stream(D.device)))
            # one map at a time: the other pointer NULL
            only = torch.full_like(D, nan)
            _C.check(_C.lib.scr_depth_loss_backward(H, W, D.data_ptr(), A.data_ptr(), g.data_ptr(), m.data_ptr(), 1, 0, 0.5,
                                                    scratch.data_ptr(), g_up.data_ptr(), None, only.data_ptr(), _C.stream(D.device)))
        torch.cuda.synchronize()
        assert torch.equal(only, dA)
        got.append((out, dD, dA))
    for a, b in zip(got[0], got[1]):
        assert torch.equal(a, b) and torch.isfinite(a).all()
    assert torch.equal(got[0][0][0], want[0]) and torch.equal(got[0][0][1:], want[1])
    assert torch.equal(got[0][1], want[2]) and torch.equal(got[0][2], want[3])


@pytest.mark.parametrize("mode", ("inverse", "expected"))
def test_upstream_gradient_is_read_from_device_memory_and_scales_the_maps(mode):
    """g_up = 0: both maps all zero.  g_up = -2.5: the float64 reference's maps times -2.5, at the parity bar."""
    D, A, g, m = recipe(52, 70, 2, device=DEV, mask_kind="f32", mode=mode)
    ref, chain = _ref_pair(D, A, g, m, mode, True)
    assert int(ref["n_valid"]) >= 64 and float(ref["residual"][ref["valid"]].abs().min()) > 1e-3
    _, _, z_dD, z_dA = _fused(D, A, g, m, mode, True, g_up=torch.zeros((), device=DEV))
    assert not z_dD.any() and not z_dA.any()
    _, _, dD, dA = _fused(D, A, g, m, mode, True, g_up=torch.full((), -2.5, device=DEV))
    for name, got, want, ch in (("dD", dD, ref["dD"], chain["dD"]), ("dA", dA, ref["dA"], chain["dA"])):
        e, bar = _rel_l2(got, -2.5 * want), max(C_CHAIN * _rel_l2(ch, want), FLOOR)
        _log(f"depth_loss g_up=-2.5 52x70 {mode:8s} {name} e {e:9.3e}  bar {bar:9.3e}")
        assert e <= bar
    assert not dD[~ref["valid"]].any() and not dA[~ref["valid"]].any()


def _poison(D, A, g, m):
    """Write every kind of hole into pixels that were valid (on the host, then to the device): NaN / +-Inf in depth, alpha and
    target, NaN / -Inf in the mask, depth <= 0, alpha < min_alpha.  Returns the maps and the bool map of the poisoned pixels."""
    shape = D.shape
    D, A, g, m = (x.flatten().cpu().clone() for x in (D, A, g, m))
    k = iter(valid_pixels(D, A, g, m, 0.5).nonzero().flatten().tolist()[::7])
    nan, inf = float("nan"), float("inf")
    hit = []
    for x, vals in ((D, (nan, inf, -inf, 0.0, -1.5)), (A, (nan, inf, -inf, 0.0, 0.4999)), (g, (nan, inf, -inf)), (m, (nan, -inf))):
        for v in vals:
            i = next(k)
            x[i] = v
            hit.append(i)
    i = next(k)
    D[i], A[i], g[i], m[i] = nan, inf, -inf, nan
    hit.append(i)
    bad = torch.zeros(D.numel(), dtype=torch.bool)
    bad[hit] = True
    return tuple(x.reshape(shape).to(DEV) for x in (D, A, g, m, bad))


@pytest.mark.parametrize("mode", ("inverse", "expected"))
@pytest.mark.parametrize("align", (True, False))
def test_holes_with_nan_inf_and_gated_values_behave_as_on_the_host(mode, align):
    """The poisoned maps give the bits of the clean maps with the same pixels masked out by hand, and exact zeros there."""
    clean = recipe(52, 70, 3, device=DEV, mask_kind="f32", mode=mode, line=(1.7, -0.08) if align else (1.0, 0.0))
    D, A, g, m, bad = _poison(*clean)
    assert int(bad.sum()) == 16
    loss, stats, dD, dA = _fused(D, A, g, m, mode, align)
    m_clean = torch.where(bad, torch.zeros_like(clean[3]), clean[3])
    want = _fused(clean[0], clean[1], clean[2], m_clean, mode, align)
    assert torch.isfinite(loss) and torch.isfinite(stats).all() and torch.isfinite(dD).all() and torch.isfinite(dA).all()
    assert not dD[bad].any() and not dA[bad].any()
    assert torch.equal(loss, want[0]) and torch.equal(stats, want[1]) and torch.equal(dD, want[2]) and torch.equal(dA, want[3])
    ref = depth_loss_ref(D, A, g, m, mode, align)
    assert int(stats[2]) == int(ref["n_valid"]) and _rel(loss, ref["loss"]) <= FLOOR
    # the byte masks: NaN-free by construction, the other three maps poisoned
    for mk in (torch.uint8, torch.bool):
        mb = (m_clean > 0).to(mk)
        l2, st2, dD2, dA2 = _fused(D, A, g, mb, mode, align)
        r2 = depth_loss_ref(D, A, g, mb, mode, align)
        assert int(st2[2]) == int(r2["n_valid"]) and _rel(l2, r2["loss"]) <= FLOOR and not dD2[bad].any() and not dA2[bad].any()
        assert torch.isfinite(dD2).all() and torch.isfinite(dA2).all()


@pytest.mark.parametrize("mode", ("inverse", "expected"))
@pytest.mark.parametrize("mk", (None, "f32", "u8"))
def test_no_valid_pixel_gives_zero_loss_zero_gradients_and_the_identity_fit(mode, mk):
    D, A, g, m = recipe(1, 4097, 4, device=DEV, mask_kind=mk, mode=mode)
    if mk is None:
        A = A * 0.5                                          # every alpha below the gate
    else:
        m = torch.zeros_like(m)
    for align in (True, False):
        loss, stats, dD, dA = _fused(D, A, g, m, mode, align)
        assert float(loss) == 0.0 and stats.tolist() == [1.0, 0.0, 0.0] and not dD.any() and not dA.any()


def test_degenerate_fits_on_the_device():
    """One valid pixel, and constant p over many: s, t = 1, 0."""
    D, A, g, m = recipe(52, 70, 5, device=DEV, mask_kind="f32")
    one = torch.zeros_like(m)
    one[17, 23] = 1.0
    A1 = A.clone()
    A1[17, 23] = 0.9
    loss, stats, _, _ = _fused(D, A1, g, one, "inverse", True)
    ref = depth_loss_ref(D, A1, g, one, "inverse", True)
    assert stats.tolist() == [1.0, 0.0, 1.0] and _rel(loss, ref["loss"]) <= FLOOR
    loss, stats, _, _ = _fused(torch.full_like(D, 1.75), torch.full_like(A, 0.875), g, None, "inverse", True)
    assert stats.tolist() == [1.0, 0.0, 3640.0]


def test_wrapper_refuses_mismatches_and_falls_back_where_the_target_wants_a_gradient():
    from splatco_amd.losses import depth_loss
    D, A, g, m = recipe(9, 11, 6, device=DEV, mask_kind="f32")
    with pytest.raises(ValueError, match="target"):
        depth_loss(D, A, g.cpu(), m)
    with pytest.raises(ValueError, match="mask"):
        depth_loss(D, A, g, m[:8])
    g_ = g.clone().requires_grad_()
    loss = depth_loss(D, A, g_, m)
    loss.backward()
    assert g_.grad is not None and g_.grad.abs().sum() > 0
    assert _rel(loss, depth_loss(D, A, g, m)) <= FLOOR
    # non-contiguous and float64 maps are converted, not misread
    want = depth_loss(D, A, g, m)
    got = depth_loss(D.t().contiguous().t(), A.double(), g, m)
    assert torch.equal(got, want)


# ------------------------------------------------------------------ through the rasterizer
def _scene(scale=1.0):
    from splatco_amd.rasterizer import GaussianRasterizationSettings
    from splatco_amd.synthetic import synthetic_camera, synthetic_gaussians
    W, H, P = 70, 52, 400
    cam, g = synthetic_camera(W, H), synthetic_gaussians(P, W, H, seed=11)
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.tensor(g["bg"], device=DEV), 1.0,
                                       cam.world_view_transform.to(DEV), cam.full_proj_transform.to(DEV), 1,
                                       cam.camera_center.to(DEV), False, False)
    t = lambda a, k=1.0: (torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV) * k).requires_grad_()
    kw = dict(means3D=t(g["means3D"], scale), opacities=t(g["opacities"]), colors_precomp=t(g["colors"]), scales=t(g["scales"], scale),
              rotations=t(g["rotations"]))
    return rs, kw


def _rasterize(rs, kw):
    from splatco_amd.rasterizer import GaussianRasterizer
    m2d = torch.zeros(kw["means3D"].shape[0], 3, device=DEV, requires_grad=True)
    return GaussianRasterizer(rs)(means2D=m2d, return_aux=True, **kw)


def test_gradients_through_the_rasterizer_match_the_float32_restatement():
    """A synthetic scene at 70 x 52 with 400 Gaussians.  The target is the inverse depth of the same scene pushed 10 % away from
    the camera (means and scales times 1.1 about the camera centre: the same image, every depth times 1.1), so without alignment
    the residual is p (1 - 1 / 1.1) >= 0.09 / 22 at every valid pixel: bounded away from the kink whatever the seed."""
    from splatco_amd.losses import depth_loss
    with torch.no_grad():
        _, _, d_far, a_far = _rasterize(*_scene(1.1))
        mask = a_far >= 0.5
        target = torch.where(mask, a_far / d_far.clamp_min(1e-6), torch.zeros_like(a_far))
    rs, kw = _scene()
    img, radii, depth, alpha = _rasterize(rs, kw)
    ref = depth_loss_ref(depth.detach(), alpha.detach(), target, mask, "inverse", False)
    n = int(ref["n_valid"])
    _log(f"depth_loss rasterizer 52x70: n_valid {n}, min |residual| {float(ref['residual'][ref['valid']].abs().min()):.3e}, "
         f"L {float(ref['loss']):.6e}")
    assert n >= 64 and float(ref["residual"][ref["valid"]].abs().min()) > 1e-4
    names = ("means3D", "opacities", "scales", "rotations")
    leaves = [kw[k] for k in names]
    fused = depth_loss(depth, alpha, target, mask, align=False)
    chain = depth_loss_ref(depth, alpha, target, mask, "inverse", False, dtype=torch.float32)["loss"]
    assert _rel(fused, ref["loss"]) <= FLOOR
    g_fused = torch.autograd.grad(fused, leaves, retain_graph=True)
    g_chain = torch.autograd.grad(chain, leaves, retain_graph=True)
    for name, a, b in zip(names, g_fused, g_chain):
        e = _rel_l2(a, b)
        _log(f"depth_loss rasterizer 52x70 d{name:10s} rel-L2 {e:9.3e} (|ref| {float(b.norm()):.3e})")
        assert float(b.norm()) > 0 and e <= 1e-4, name
    # the image and its gradient path: a zero-weight depth term changes no bit
    G = torch.randn(img.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    all_leaves = leaves + [kw["colors_precomp"]]
    plain = torch.autograd.grad((img * G).sum(), all_leaves, retain_graph=True)
    with_term = torch.autograd.grad((img * G).sum() + 0.0 * depth_loss(depth, alpha, target, mask, align=False), all_leaves)
    for a, b in zip(plain, with_term):
        assert torch.equal(a, b)
    rs2, kw2 = _scene()
    from splatco_amd.rasterizer import GaussianRasterizer
    img2, radii2 = GaussianRasterizer(rs2)(means2D=torch.zeros(400, 3, device=DEV, requires_grad=True), **kw2)
    assert torch.equal(img2, img) and torch.equal(radii2, radii)


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


OPTS = dict(align=False, min_alpha=0.2)


def _teacher(pc, cams, pipe, bg):
    """Inverse-depth targets 10 % beyond the model's own surface, and their masks (where the model is opaque enough)."""
    from splatco_amd.renderer import prefilter_voxel, render
    targets, masks = [], []
    with torch.no_grad():
        for cam in cams:
            out = render(cam, pc, pipe, bg, visible_mask=prefilter_voxel(cam, pc, pipe, bg), aux=True)
            mask = (out["alpha"] >= 0.25) & (out["depth"] > 0)
            targets.append(torch.where(mask, out["alpha"] / (1.1 * out["depth"]).clamp_min(1e-6), torch.zeros_like(out["alpha"])))
            masks.append(mask)
    return targets, masks


def _grads(pc):
    return {n: p.grad.detach().clone() for n, p in pc.named_parameters() if p.grad is not None}


def test_step_with_default_depth_arguments_leaves_the_parents_gradient_bits():
    from splatco_amd.train_step import collaborative_step
    make, cams, gts, pipe, bg = _step_scene()
    pc_a, pc_b, pc_c = make(), make(), make()
    targets, masks = _teacher(pc_c, cams, pipe, bg)
    loss_a, out_a, _ = collaborative_step(pc_a, cams, gts, pipe, bg)
    loss_b, out_b, _ = collaborative_step(pc_b, cams, gts, pipe, bg, depth_targets=None, depth_masks=None, depth_weight=0.0,
                                          depth_options=None)
    loss_c, out_c, _ = collaborative_step(pc_c, cams, gts, pipe, bg, depth_targets=targets, depth_masks=masks, depth_weight=0.0,
                                          depth_options=OPTS)
    assert "depth" not in out_b and "depth" not in out_c     # render() was called without aux
    ga, gb, gc = _grads(pc_a), _grads(pc_b), _grads(pc_c)
    assert len(ga) > 4 and set(ga) == set(gb) == set(gc)
    assert torch.equal(loss_a, loss_b) and torch.equal(loss_a, loss_c)
    for n in ga:
        assert torch.equal(ga[n], gb[n]) and torch.equal(ga[n], gc[n]), n


def test_step_with_a_depth_weight_equals_the_hand_written_loop_and_refuses_bad_lists():
    from splatco_amd.losses import depth_loss, view_loss
    from splatco_amd.renderer import prefilter_voxel, render
    from splatco_amd.train_step import collaborative_step
    make, cams, gts, pipe, bg = _step_scene()
    pc_s, pc_h = make(), make()
    targets, masks = _teacher(pc_h, cams, pipe, bg)
    masks[1] = None                                          # an entry may be absent
    loss_s, out_s, _ = collaborative_step(pc_s, cams, gts, pipe, bg, depth_targets=[t.cpu() for t in targets], depth_masks=masks,
                                          depth_weight=0.3, depth_options=OPTS)
    assert "depth" in out_s and "alpha" in out_s
    total, terms = None, []
    for cam, gt, tg, mk in zip(cams, gts, targets, masks):
        out = render(cam, pc_h, pipe, bg, visible_mask=prefilter_voxel(cam, pc_h, pipe, bg), retain_grad=True, aux=True)
        term, stats = depth_loss(out["depth"], out["alpha"], tg, mk, return_stats=True, **OPTS)
        terms.append((float(term), int(stats[2])))
        loss = view_loss(out["render"], gt, out["scaling"]) + 0.3 * term
        total = loss if total is None else total + loss
    total.backward()
    _log(f"depth_loss step 96x160: per-view (depth loss, n_valid) {terms}")
    assert all(t > 0 and n >= 64 for t, n in terms)
    assert _rel(loss_s, total) <= 1e-6
    gs, gh = _grads(pc_s), _grads(pc_h)
    assert len(gs) > 4 and set(gs) == set(gh)
    for n in gs:
        e = _rel_l2(gs[n], gh[n])
        assert e <= 1e-4, (n, e)
    # and the depth term did reach the gradients: the step without it differs
    pc_0 = make()
    collaborative_step(pc_0, cams, gts, pipe, bg)
    g0 = _grads(pc_0)
    assert any(not torch.equal(g0[n], gs[n]) for n in gs)
    for kw in (dict(), dict(depth_targets=targets[:1]), dict(depth_targets=targets, depth_masks=masks + [None])):
        with pytest.raises(ValueError, match="depth_targets|depth_masks"):
            collaborative_step(pc_s, cams, gts, pipe, bg, depth_weight=0.3, **kw)


def test_twenty_adam_steps_on_a_teacher_depth_lower_the_depth_loss():
    from splatco_amd.adam import FusedAdam
    from splatco_amd.losses import depth_loss
    from splatco_amd.renderer import prefilter_voxel, render
    from splatco_amd.train_step import collaborative_step
    make, cams, gts, pipe, bg = _step_scene()
    pc = make()
    cams = cams[:1]
    targets, masks = _teacher(pc, cams, pipe, bg)
    with torch.no_grad():
        gts = [render(cams[0], pc, pipe, bg, visible_mask=prefilter_voxel(cams[0], pc, pipe, bg))["render"].clone()]
    groups = [{"params": [getattr(pc, "_" + n)], "lr": lr, "name": n} for n, lr in
              zip(("anchor", "offset", "anchor_feat", "scaling"), (1e-4, 1e-3, 7.5e-3, 7e-3))]
    groups.append({"params": [p for n, p in pc.named_parameters() if not n.startswith("_") and p.requires_grad], "lr": 2e-3,
                   "name": "mlp_and_feat_planes"})
    opt = FusedAdam(groups, eps=1e-15)

    def measure():
        with torch.no_grad():
            out = render(cams[0], pc, pipe, bg, visible_mask=prefilter_voxel(cams[0], pc, pipe, bg), aux=True)
            return float(depth_loss(out["depth"], out["alpha"], targets[0], masks[0], **OPTS))
    initial = measure()
    for _ in range(20):
        collaborative_step(pc, cams, gts, pipe, bg, optimizer=opt, depth_targets=targets, depth_masks=masks, depth_weight=1.0,
                           depth_options=OPTS)
    final = measure()
    _log(f"depth_loss 20 Adam steps 96x160: initial {initial:.6e}  final {final:.6e}  ratio {final / initial:.4f}")
    assert initial > 0 and math.isfinite(final) and final < initial
