"""GPU tests of the per-view bilateral grids: splatco_amd.bilagrid (csrc/bilagrid.hip) against the float64 restatement of the
definition (tests/bilagrid_ref.py), its total-variation gradient, a small fit, and collaborative_step with a grid.

Kernel constants (csrc/bilagrid.hip) and the shapes that sit one below, at and one above each:
  BG_TW x BG_TH = 64 x 16     pixel tile of a slice workgroup           widths 63 / 64 / 65, heights 15 / 16 / 17
  BG_LDS_FLOATS = 12288       staged vertex columns of a tile           a 5 x 5 image (one tile, the whole grid under it) with
                                                                        L = 16 and 8 x 7 / 8 x 8 / 8 x 9 vertices: 10752 /
                                                                        12288 / 13824 floats, the last read from the grid itself
  BG_LC = 8                   levels per grid-backward pass             L = 7 / 8 / 9 (9: a second pass over the rectangle)
  BG_THREADS = 256            lanes that walk a vertex's rectangle      1 x 255 / 256 / 257 under a 2 x 2 grid (the rectangle is
                                                                        the image); 135 x 240: many trips per lane
  BG_PART_ROWS = 32           rectangle rows per workgroup              Gh = 2 (the rectangle is all rows): H = 31 / 32 / 33,
                                                                        the last split into two parts
  BG_MAX_PARTS = BG_FOLD = 64 parts per vertex = fold lanes             Gh = 2, H = 2016 / 2048 / 2049: 63 / 64 / 64 parts (the
                                                                        last with 33 rows each)
Image shapes 1 x 1, 7 x 5 (smaller than the grid), 70 x 133 (ragged against the tile), 135 x 240; grids (L, Gh, Gw) =
(8, 16, 16), (2, 2, 2), (4, 5, 3), (16, 3, 64).

Inputs: grid = N(0, 1), dL/dout = N(0, 1), rgb = 1.6 U - 0.3 so that pixels clamp on either side; the first pixel is set to
-0.2 and the last to 1.2, so that every image of two pixels or more has one of each (asserted).

Bar: max(1.5 x the float32 torch chain's own error against the same float64 result, 2e-6), rel-L2 -- the constants of
tests/test_gpu_depth_loss.py.  Every figure is printed before it is asserted (and appended to the file $SPLATCO_BILAGRID_LOG
names, if set); profiles/r17_bilagrid.txt holds one such run.
"""
import math
import os
import types

import pytest
import torch

import bilagrid_ref as ref
import poison

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C_CHAIN, FLOOR = 1.5, 2e-6
IMAGES = [(1, 1), (7, 5), (70, 133), (135, 240)]
GRIDS = [(8, 16, 16), (2, 2, 2), (4, 5, 3), (16, 3, 64)]
EDGES = ([(20, w, 8, 16, 16) for w in (63, 64, 65)] + [(h, 40, 8, 16, 16) for h in (15, 16, 17)]
         + [(5, 5, 16, 8, gw) for gw in (7, 8, 9)]
         + [(33, 47, L, 5, 3) for L in (7, 8, 9)]
         + [(1, w, 4, 2, 2) for w in (255, 256, 257)]
         + [(h, 9, 4, 2, 3) for h in (31, 32, 33)]
         + [(h, 3, 2, 2, 2) for h in (2016, 2048, 2049)])


def _log(line):
    print(line)
    path = os.environ.get("SPLATCO_BILAGRID_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _inputs(H, W, L, Gh, Gw, seed=0):
    g = torch.Generator().manual_seed(seed)
    grid = torch.randn(12, L, Gh, Gw, generator=g)
    rgb = 1.6 * torch.rand(3, H, W, generator=g) - 0.3
    dout = torch.randn(3, H, W, generator=g)
    if H * W >= 2:
        rgb[:, 0, 0], rgb[:, -1, -1] = -0.2, 1.2
    return grid.to(DEV), rgb.to(DEV), dout.to(DEV)


def _fused(grid, rgb, dout, want_grid=True, want_rgb=True):
    from splatco_amd.bilagrid import slice_apply
    g_, c_ = grid.detach().clone().requires_grad_(want_grid), rgb.detach().clone().requires_grad_(want_rgb)
    out = slice_apply(g_, c_)
    assert out.device == rgb.device and out.dtype == torch.float32 and out.shape == rgb.shape
    leaves = [t for t, w in ((c_, want_rgb), (g_, want_grid)) if w]
    grads = iter(torch.autograd.grad(out, leaves, grad_outputs=dout))
    return out.detach(), (next(grads) if want_rgb else None), (next(grads) if want_grid else None)


_REFS = {}


def _refs(H, W, L, Gh, Gw, seed=0):
    """(inputs, float64 reference, float32 chain), computed once per case and never changed."""
    key = (H, W, L, Gh, Gw, seed)
    if key not in _REFS:
        inp = _inputs(H, W, L, Gh, Gw, seed)
        _REFS[key] = (inp, ref.slice_with_grads(*inp, dtype=torch.float64), ref.slice_with_grads(*inp, dtype=torch.float32))
    return _REFS[key]


def _assert_bar(case, got, want, chain, names=("out", "dL/drgb", "dL/dgrid")):
    failed = []
    for name, a, b, c in zip(names, got, want, chain):
        e, e_chain = _rel_l2(a, b), _rel_l2(c, b)
        bar = max(C_CHAIN * e_chain, FLOOR)
        _log(f"bilagrid {case:40s} {name:8s} e {e:9.3e}  e_chain {e_chain:9.3e}  bar {bar:9.3e}{'' if e <= bar else '   <-- FAIL'}")
        assert bool(torch.isfinite(a).all()), (case, name)
        if not e <= bar:
            failed.append(name)
    assert not failed, (case, failed)


def _check_parity(H, W, L, Gh, Gw):
    (grid, rgb, dout), want, chain = _refs(H, W, L, Gh, Gw)
    case = f"{H}x{W} grid ({L},{Gh},{Gw})"
    if H * W >= 2:
        lum = (0.299 * rgb[0].double() + 0.587 * rgb[1].double()) + 0.114 * rgb[2].double()
        assert bool((lum <= 0).any()) and bool((lum >= 1).any()), case
    got = _fused(grid, rgb, dout)
    again = _fused(grid, rgb, dout)
    torch.cuda.synchronize()
    for a, b in zip(got, again):
        assert poison.same_bits(a, b), (case, "two calls differ")
    _assert_bar(case, got, want, chain)
    return got, want


@pytest.mark.parametrize("L,Gh,Gw", GRIDS)
@pytest.mark.parametrize("H,W", IMAGES)
def test_parity_with_the_float64_restatement(H, W, L, Gh, Gw):
    _check_parity(H, W, L, Gh, Gw)


@pytest.mark.parametrize("H,W,L,Gh,Gw", EDGES)
def test_parity_around_every_kernel_constant(H, W, L, Gh, Gw):
    _check_parity(H, W, L, Gh, Gw)


def test_vertices_no_pixel_reaches_get_exact_zeros():
    got, want = _check_parity(7, 5, 8, 16, 16)
    untouched = want[2] == 0
    n = int(untouched.all(dim=0).all(dim=0).sum())          # vertices (gy, gx) whose every channel and level is zero
    _log(f"bilagrid 7x5 grid (8,16,16): {n} of 256 vertices without a pixel")
    assert n >= 100
    assert not got[2][untouched].any()
    assert bool((got[2] != 0).any())


def test_clamped_pixels_have_no_guide_gradient():
    """Luminance below 0 and above 1 in two halves of the image: dL/drgb is A[:, :3]^T dL/dout alone there."""
    H, W, L, Gh, Gw = 24, 70, 8, 16, 16
    grid, rgb, dout = _inputs(H, W, L, Gh, Gw, seed=1)
    rgb = torch.where(torch.arange(W, device=DEV) < W // 2, -0.05 - 0.4 * rgb.abs(), 1.05 + 0.4 * rgb.abs())
    lum = (0.299 * rgb[0].double() + 0.587 * rgb[1].double()) + 0.114 * rgb[2].double()
    assert bool(((lum < 0) | (lum > 1)).all()) and bool((lum < 0).any()) and bool((lum > 1).any())
    got = _fused(grid, rgb, dout)
    want = ref.slice_with_grads(grid, rgb, dout, torch.float64)
    chain = ref.slice_with_grads(grid, rgb, dout, torch.float32)
    _assert_bar("24x70 all pixels clamped", got, want, chain)
    alone = ref.rgb_grad_without_guide(grid, rgb, dout, torch.float64)
    assert _rel_l2(want[1], alone) <= 1e-14
    e, bar = _rel_l2(got[1], alone), max(C_CHAIN * _rel_l2(ref.rgb_grad_without_guide(grid, rgb, dout, torch.float32), alone), FLOOR)
    _log(f"bilagrid 24x70 clamped: dL/drgb against A^T dL/dout alone  e {e:9.3e}  bar {bar:9.3e}")
    assert e <= bar


def test_luminance_exactly_on_a_level():
    """rgb = k / (L - 1) in all three channels.  out and dL/dgrid are continuous across a level and are held to the bar.  The
    guide's derivative is one-sided there, and the side is decided by the rounding of the luminance (the three weights do not
    add up to 1 exactly in either precision: tests/test_bilagrid_host.py), so every pixel's dL/drgb is compared with the
    nearest of the float64 results of its own cell, the cell below and the cell above -- for the float32 chain alike.
    k = 0 .. L - 2: level 0 is a luminance of exactly 0 in every precision (clamped: no guide term); the top level is left
    out, because there the same rounding decides whether the pixel counts as clamped at all."""
    H, W, L, Gh, Gw = 33, 47, 5, 5, 3
    grid, rgb, dout = _inputs(H, W, L, Gh, Gw, seed=2)
    k = torch.randint(0, L - 1, (H, W), generator=torch.Generator().manual_seed(3)).to(DEV)
    rgb = (k.float() / (L - 1)).expand(3, H, W).contiguous()
    got = _fused(grid, rgb, dout)
    want = ref.slice_with_grads(grid, rgb, dout, torch.float64)
    chain = ref.slice_with_grads(grid, rgb, dout, torch.float32)
    _assert_bar("33x47 on a level", (got[0], got[2]), (want[0], want[2]), (chain[0], chain[2]), names=("out", "dL/dgrid"))
    sides = [ref.slice_explicit(grid, rgb, dout, torch.float64, cell_shift=torch.full((H, W), s, device=DEV))[1] for s in (0, -1, 1)]

    def nearest(x):
        d = torch.stack([(x.double() - s).pow(2).sum(0) for s in sides]).amin(0)
        return float(d.sum().sqrt() / want[1].norm())
    assert nearest(want[1]) <= 1e-12              # float64 autograd itself takes one side or the other, pixel by pixel
    e, e_chain = nearest(got[1]), nearest(chain[1])
    bar = max(C_CHAIN * e_chain, FLOOR)
    _log(f"bilagrid 33x47 on a level: dL/drgb against the nearer side  e {e:9.3e}  e_chain {e_chain:9.3e}  bar {bar:9.3e}")
    assert e <= bar


def test_identity_grid_returns_the_image():
    from splatco_amd.bilagrid import BilateralGrid
    bil = BilateralGrid(2, device=DEV)
    _, rgb, dout = _inputs(70, 133, 8, 16, 16, seed=4)
    out = bil(rgb, 1)
    want = ref.slice_ref(bil.grids[1].detach(), rgb, torch.float64)
    chain = ref.slice_ref(bil.grids[1].detach(), rgb, torch.float32)
    assert _rel_l2(want, rgb) <= 1e-15
    e, bar = _rel_l2(out, rgb), max(C_CHAIN * _rel_l2(chain, want), FLOOR)
    _log(f"bilagrid 70x133 identity grid: out against the image  e {e:9.3e}  bar {bar:9.3e}")
    assert e <= bar
    out.backward(dout)
    assert bil.grids.grad.shape == bil.grids.shape and not bil.grids.grad[0].any() and bool(bil.grids.grad[1].any())


@pytest.mark.parametrize("N,L,Gh,Gw", [(1, 2, 2, 2), (3, 2, 2, 2), (1, 8, 16, 16), (3, 8, 16, 16)])
def test_tv_add_grad_against_float64_autograd(N, L, Gh, Gw):
    from splatco_amd.bilagrid import tv_add_grad
    g = torch.Generator().manual_seed(N + L)
    grids = torch.randn(N, 12, L, Gh, Gw, generator=g).to(DEV).requires_grad_()
    before = torch.randn(N, 12, L, Gh, Gw, generator=g).to(DEV)
    weight = 10.0
    want, chain = [], None
    for dtype in (torch.float64, torch.float32):
        x = grids.detach().to(dtype).requires_grad_()
        want.append(torch.autograd.grad(weight * ref.tv(x, dtype), x)[0])
    want, chain = want
    assert _rel_l2(ref.tv_grad_closed_form(grids.detach(), weight), want) <= 1e-13
    grids.grad = before.clone()
    tv_add_grad(grids, weight)
    increment = grids.grad.double() - before.double()
    # the increment is read back from a float32 sum: each element carries half an ulp of (before + increment) on top
    e, e_chain = _rel_l2(increment, want), _rel_l2((before + chain).double() - before.double(), want)
    bar = max(C_CHAIN * e_chain, FLOOR)
    _log(f"bilagrid tv N={N} grid ({L},{Gh},{Gw}) into a filled gradient: e {e:9.3e}  e_chain {e_chain:9.3e}  bar {bar:9.3e}")
    assert e <= bar
    grids.grad = None
    tv_add_grad(grids, weight)                                  # no gradient yet: allocated as zeros
    e, e_chain = _rel_l2(grids.grad, want), _rel_l2(chain, want)
    bar = max(C_CHAIN * e_chain, FLOOR)
    _log(f"bilagrid tv N={N} grid ({L},{Gh},{Gw}) into zeros:             e {e:9.3e}  e_chain {e_chain:9.3e}  bar {bar:9.3e}")
    assert e <= bar
    first = grids.grad.clone()
    grids.grad = None
    tv_add_grad(grids, weight)
    assert poison.same_bits(first, grids.grad)


@pytest.mark.parametrize("H,W,L,Gh,Gw", [(70, 133, 8, 16, 16), (7, 5, 16, 3, 64), (2049, 3, 2, 2, 2)])
def test_results_do_not_depend_on_what_fresh_memory_held(H, W, L, Gh, Gw):
    from splatco_amd.bilagrid import tv_add_grad
    grid, rgb, dout = _inputs(H, W, L, Gh, Gw, seed=5)
    grids = torch.stack([grid, grid.flip(1)]).contiguous().requires_grad_()

    def run():
        out, d_rgb, d_grid = _fused(grid, rgb, dout)
        _, only_rgb, _ = _fused(grid, rgb, dout, want_grid=False)          # dL_dgrid = NULL
        _, _, only_grid = _fused(grid, rgb, dout, want_rgb=False)          # dL_drgb = NULL
        grids.grad = None
        tv_add_grad(grids, 10.0)
        return [out, d_rgb, d_grid, only_rgb, only_grid, grids.grad]
    report = poison.check(run, sync=torch.cuda.synchronize)
    outs = report["outputs"]
    assert poison.same_bits(outs[1], outs[3]) and poison.same_bits(outs[2], outs[4])


@pytest.mark.parametrize("L,Gh,Gw", [(8, 16, 16), (4, 5, 3)])
def test_a_grid_learns_a_smooth_gain_and_offset(L, Gh, Gw):
    """48 x 64, rgb = U (seed 0), target = gain(x, y) rgb + (0.05, -0.03, 0.02) with gain = (1.3, 0.9, 1.1) (0.8 + 0.4 x)
    (1.1 - 0.2 y); identity grid, torch.optim.Adam(lr = 1e-2), L1 loss.  After 100 steps the loss is at most 0.05 of its
    initial value: the float32 torch restatement reaches 0.0146 / 0.0149 / 0.0150 (seeds 0 - 2; 0.0147 / 0.0150 / 0.0133 at
    (4, 5, 3)) on the CPU, the bar is three times that."""
    from splatco_amd.bilagrid import slice_apply
    H, W = 48, 64
    rgb = torch.rand(3, H, W, generator=torch.Generator().manual_seed(0)).to(DEV)
    x = ((torch.arange(W, device=DEV) + 0.5) / W).reshape(1, 1, W)
    y = ((torch.arange(H, device=DEV) + 0.5) / H).reshape(1, H, 1)
    gain = torch.tensor([1.3, 0.9, 1.1], device=DEV).reshape(3, 1, 1) * (0.8 + 0.4 * x) * (1.1 - 0.2 * y)
    target = gain * rgb + torch.tensor([0.05, -0.03, 0.02], device=DEV).reshape(3, 1, 1)
    grid = torch.eye(3, 4, device=DEV).reshape(12, 1, 1, 1).repeat(1, L, Gh, Gw).contiguous().requires_grad_()
    opt = torch.optim.Adam([grid], lr=1e-2)
    loss_of = lambda: (slice_apply(grid, rgb) - target).abs().mean()
    initial = float(loss_of().detach())
    for _ in range(100):
        opt.zero_grad()
        loss_of().backward()
        opt.step()
    final = float(loss_of().detach())
    _log(f"bilagrid fit 48x64 grid ({L},{Gh},{Gw}): initial {initial:.6e}  after 100 Adam steps {final:.6e}  ratio {final / initial:.4f}")
    assert initial > 0 and final <= 0.05 * initial


# ------------------------------------------------------------------ through the training step
def _step_scene():
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.synthetic import synthetic_anchor_model
    W, H = 160, 96
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    bg = torch.ones(3, device=DEV)
    cams = [look_at_camera(eye=(0.0, 0.0, 0.0), target=(x, 0.0, 0.0), up=(0, -1, 0), FoVx=math.radians(60), width=W, height=H,
                           uid=uid).to(torch.device(DEV)) for uid, x in ((3, 1.0), (1, -1.0))]
    gts = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(i)).to(DEV) for i in range(2)]
    make = lambda: synthetic_anchor_model(20_000, 7, torch.device(DEV), plane_size=64)
    return make, cams, gts, pipe, bg


def _grads(pc):
    return {n: p.grad.detach().clone() for n, p in pc.named_parameters() if p.grad is not None}


def _noisy_grid(num_views=5):
    from splatco_amd.bilagrid import BilateralGrid
    bil = BilateralGrid(num_views, device=DEV)
    with torch.no_grad():
        bil.grids.add_(0.05 * torch.randn(bil.grids.shape, generator=torch.Generator().manual_seed(9)).to(DEV))
    return bil


def test_step_without_a_grid_is_the_step_without_the_argument():
    from splatco_amd.train_step import collaborative_step
    make, cams, gts, pipe, bg = _step_scene()
    pc_a, pc_b = make(), make()
    loss_a, _, _ = collaborative_step(pc_a, cams, gts, pipe, bg)
    loss_b, _, _ = collaborative_step(pc_b, cams, gts, pipe, bg, bilateral_grid=None, bilagrid_tv_weight=10.0)
    ga, gb = _grads(pc_a), _grads(pc_b)
    assert len(ga) > 4 and set(ga) == set(gb) and torch.equal(loss_a, loss_b)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    for (n, p), (_, q) in zip(pc_a.named_parameters(), pc_b.named_parameters()):
        assert torch.equal(p, q), n


def test_step_with_a_grid_equals_the_hand_written_loop_and_refuses_ranks_and_arenas(monkeypatch):
    from splatco_amd import train_step
    from splatco_amd.bilagrid import tv_add_grad
    from splatco_amd.losses import view_loss
    from splatco_amd.renderer import prefilter_voxel, render
    make, cams, gts, pipe, bg = _step_scene()
    pc_s, pc_h = make(), make()
    bil_s, bil_h = _noisy_grid(), _noisy_grid()
    bil_s.grids.grad = torch.full_like(bil_s.grids, 7.0)        # cleared on entry, like the model's gradients
    loss_s, _, _ = train_step.collaborative_step(pc_s, cams, gts, pipe, bg, bilateral_grid=bil_s, bilagrid_tv_weight=10.0)
    total = None
    for cam, gt in zip(cams, gts):
        out = render(cam, pc_h, pipe, bg, visible_mask=prefilter_voxel(cam, pc_h, pipe, bg), retain_grad=True)
        loss = view_loss(bil_h(out["render"], cam.uid), gt, out["scaling"])
        total = loss if total is None else total + loss
    total.backward()
    assert torch.equal(loss_s, total.detach())
    gs, gh = _grads(pc_s), _grads(pc_h)
    assert len(gs) > 4 and set(gs) == set(gh)
    for n in gs:
        assert torch.equal(gs[n], gh[n]), n
    # the grid did reach the model's gradients: the step without it differs
    pc_0 = make()
    train_step.collaborative_step(pc_0, cams, gts, pipe, bg)
    g0 = _grads(pc_0)
    assert any(not torch.equal(g0[n], gs[n]) for n in gs)
    # the grids: the data gradient of the two uids (3 and 1) plus the TV increment; the others the TV increment alone
    data = bil_h.grids.grad.clone()
    assert bool(data[3].any()) and bool(data[1].any()) and not data[[0, 2, 4]].any()
    tv_only = _noisy_grid()
    tv_add_grad(tv_only.grids, 10.0)
    assert bool(tv_only.grids.grad.any())
    assert torch.equal(bil_s.grids.grad[[0, 2, 4]], tv_only.grids.grad[[0, 2, 4]])
    tv_add_grad(bil_h.grids, 10.0)
    assert torch.equal(bil_s.grids.grad, bil_h.grids.grad)
    assert not torch.equal(bil_s.grids.grad[[1, 3]], tv_only.grids.grad[[1, 3]])
    # an optimizer that holds the grids steps them
    from splatco_amd.adam import FusedAdam
    opt = FusedAdam([{"params": [bil_s.grids], "lr": 2e-3, "name": "bilateral_grids"}], eps=1e-15)
    before = bil_s.grids.detach().clone()
    train_step.collaborative_step(pc_s, cams, gts, pipe, bg, optimizer=opt, bilateral_grid=bil_s)
    assert not torch.equal(before, bil_s.grids.detach()) and bool(torch.isfinite(bil_s.grids).all())
    # more than one rank, or an arena: refused with the reason
    with pytest.raises(NotImplementedError, match="arena"):
        train_step.collaborative_step(pc_s, cams, gts, pipe, bg, bilateral_grid=bil_s, arena=object())
    monkeypatch.setattr(train_step, "world_info", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="rank"):
        train_step.collaborative_step(pc_s, cams, gts, pipe, bg, bilateral_grid=bil_s)
