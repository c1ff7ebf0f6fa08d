"""GPU tests of the drop-in renderer path: prefilter_voxel -> generate_neural_gaussians -> render
(gaussian_renderer/__init__.py:118-244) on the model captured in tests/golden/neural_gaussians.npz."""
import math
import os
import types

import numpy as np
import pytest
import torch

from util import oracle_settings
from splatco_amd.cameras import look_at_camera

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _model(dev):
    from test_host_golden import _model_from_fixture
    d = np.load(os.path.join(GOLD, "neural_gaussians.npz"))
    return _model_from_fixture(d).to(dev), d


def test_prefilter_and_render_contract(oracle):
    from splatco_amd.renderer import prefilter_voxel, render
    from splatco_amd.stats import training_statis
    from torch_restatements import training_statis_torch
    dev = torch.device("cuda:0")
    pc, d = _model(dev)
    cam = look_at_camera(eye=(0.3, -0.2, -4.5), target=(0, 0, 0), up=(0, -1, 0), FoVx=math.radians(60), width=200,
                         height=120).to(dev)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False, mv=4)
    bg = torch.tensor([1.0, 1.0, 1.0], device=dev)
    pc.train()
    # a2: anchor visibility == oracle radii > 0 on exp(_scaling)[:, :3], normalised rotation
    vis = prefilter_voxel(cam, pc, pipe, bg)
    cpu_cam = cam.to("cpu")
    st = oracle_settings(oracle, cpu_cam, bg.cpu().numpy())
    want = oracle.visible_filter(st, d["anchor"], np.exp(d["scaling"])[:, :3],
                                 np.tile(np.array([1, 0, 0, 0], np.float32), (512, 1)))
    assert vis.dtype == torch.bool and np.array_equal(vis.cpu().numpy(), want > 0)
    # a4: result dict, autograd contract
    out = render(cam, pc, pipe, bg, visible_mask=vis, retain_grad=True)
    assert set(out) == {"render", "viewspace_points", "visibility_filter", "radii", "selection_mask",
                        "neural_opacity", "scaling"}
    P = out["viewspace_points"].shape[0]
    # the gradient carrier is what the reference builds at :133-138: a non-leaf of zeros that requires grad
    vp = out["viewspace_points"]
    assert vp.requires_grad and not vp.is_leaf and vp.grad_fn is not None and vp.dtype == pc.get_anchor.dtype
    assert float(vp.detach().abs().max()) == 0.0
    assert out["render"].shape == (3, 120, 200) and out["render"].dtype == torch.float32
    assert out["radii"].dtype == torch.int32 and out["radii"].shape == (P,)
    assert out["visibility_filter"].dtype == torch.bool
    assert out["selection_mask"].shape == (int(vis.sum()) * pc.n_offsets,)
    assert int(out["selection_mask"].sum()) == P
    target = torch.rand(3, 120, 200, device=dev)
    loss = (out["render"] - target).abs().mean() + 0.01 * out["scaling"].prod(dim=1).mean()
    loss.backward()
    g = out["viewspace_points"].grad
    assert g is not None and g.shape == (P, 3) and torch.all(g[:, 2] == 0) and g[:, :2].abs().sum() > 0
    for p in (pc._anchor, pc._offset, pc._anchor_feat, pc._scaling, pc.mlp_color[0].weight,
              pc.feat_planes._feat.k0s[0].xy_plane):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0
    # a8: the consumer of the means2D gradient runs on these tensors
    N, k = 512, pc.n_offsets
    acc = [torch.zeros(N, 1, device=dev), torch.zeros(N, 1, device=dev), torch.zeros(N * k, 1, device=dev),
           torch.zeros(N * k, 1, device=dev)]
    acc_t = [a.clone() for a in acc]
    training_statis(*acc, k, g, out["neural_opacity"], out["visibility_filter"], out["selection_mask"], vis)
    training_statis_torch(*acc_t, k, g, out["neural_opacity"], out["visibility_filter"], out["selection_mask"], vis)
    assert acc[3].sum() == out["visibility_filter"].sum()
    assert torch.equal(acc[1], acc_t[1]) and torch.equal(acc[3], acc_t[3])
    assert torch.allclose(acc[0], acc_t[0], rtol=1e-6, atol=0) and torch.allclose(acc[2], acc_t[2], rtol=1e-6, atol=0)
    # image equals the oracle's rendering of the same neural Gaussians
    from splatco_amd.renderer import generate_neural_gaussians
    with torch.no_grad():
        xyz, color, opacity, scaling, rot, _, _ = generate_neural_gaussians(cam, pc, vis, is_training=True)
    f = oracle.forward(st, xyz.cpu().numpy(), opacity.cpu().numpy(), scaling.cpu().numpy(), rot.cpu().numpy(),
                       colors_precomp=color.cpu().numpy())
    same = f["margin"] > 1e-5
    assert np.abs(out["render"].detach().cpu().numpy() - f["color"])[:, same].max() <= 1e-4
    assert np.array_equal(out["radii"].cpu().numpy(), f["radii"])
    # without retain_grad the non-leaf carrier keeps no .grad (train.py:185-186 switches it off after update_until)
    import warnings
    out3 = render(cam, pc, pipe, bg, visible_mask=vis)
    (out3["render"] - target).abs().mean().backward()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert not out3["viewspace_points"].is_leaf and out3["viewspace_points"].grad is None
    # eval mode: 4 keys
    pc.eval()
    with torch.no_grad():
        out2 = render(cam, pc, pipe, bg, visible_mask=vis, retain_grad=True)     # retain_grad under no_grad: swallowed, as there
    assert set(out2) == {"render", "viewspace_points", "visibility_filter", "radii"}
    assert not out2["viewspace_points"].requires_grad


def test_reference_written_scene_loads_and_renders_on_the_gpu(oracle, tmp_path):
    """f4's purpose: a scene the REFERENCE's code wrote is loaded through splatco_amd.scene_io the way
    Scene.__init__ loads an iteration (scene/__init__.py:80-94, scene/gaussian_model.py:675-712,1065-1090) and rendered on
    the device.  tests/golden/ref_scene/ holds chkpnt7.pth and checkpoints.pth written by the reference's capture() /
    save_mlp_checkpoints() for the model of neural_gaussians.npz; its anchors travel as the point_cloud.ply our save_ply
    writes (byte layout pinned to the reference's save_ply by test_ply_equals_what_the_reference_hands_to_plyfile).  The model
    that loads them starts from OTHER weights, so everything checked below comes out of the files:
      * generate_neural_gaussians == the reference's own outputs for that model (fixture L0_train.*),
      * prefilter_voxel == oracle radii > 0, render image / radii == the oracle on the same neural Gaussians."""
    import shutil
    from splatco_amd import scene_io
    from splatco_amd.renderer import generate_neural_gaussians, prefilter_voxel, render
    from splatco_amd.scene_model import AnchorGaussianModel
    dev = torch.device("cuda:0")
    d = np.load(os.path.join(GOLD, "neural_gaussians.npz"))
    ref_dir = os.path.join(GOLD, "ref_scene")
    # the directory a training run of the reference leaves behind for iteration 7
    src, _ = _model(torch.device("cpu"))                       # only its anchors are used (-> point_cloud.ply)
    it_dir = tmp_path / "point_cloud" / "iteration_7"
    scene_io.save_ply(src, str(it_dir / "point_cloud.ply"))
    shutil.copy(os.path.join(ref_dir, "checkpoints.pth"), it_dir / "checkpoints.pth")        # reference-written
    shutil.copy(os.path.join(ref_dir, "chkpnt7.pth"), tmp_path / "chkpnt7.pth")              # reference-written
    torch.manual_seed(123)
    pc = AnchorGaussianModel(feat_dim=32, n_offsets=int(d["n_offsets"]), appearance_dim=0, plane_size=40, num_channels=15).to(dev)
    before = pc.mlp_color[0].weight.detach().clone()
    scene_io.load_scene(pc, str(tmp_path), 7, device=dev)
    pc.feat_planes.Q0 = 0
    assert pc._anchor.is_cuda and pc._anchor.shape == (512, 3) and not torch.equal(before, pc.mlp_color[0].weight)
    assert sorted(pc.contractor_state) == ["xyz_max", "xyz_min"]
    pc.train()
    cam0 = types.SimpleNamespace(camera_center=torch.tensor(d["camera_center"], device=dev), uid=0)
    with torch.no_grad():
        got = generate_neural_gaussians(cam0, pc, torch.tensor(d["visible_mask"], device=dev), is_training=True)
    assert np.array_equal(got[6].cpu().numpy(), d["L0_train.mask"])
    for t, name in zip(got[:6], ["xyz", "color", "opacity", "scaling", "rot", "neural_opacity"]):
        np.testing.assert_allclose(t.cpu().numpy(), d[f"L0_train.{name}"], rtol=1e-4, atol=1e-5, err_msg=name)
    # the render path on the loaded scene
    cam = look_at_camera(eye=(0.3, -0.2, -4.5), target=(0, 0, 0), up=(0, -1, 0), FoVx=math.radians(60), width=200,
                         height=120).to(dev)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False, mv=4)
    bg = torch.tensor([1.0, 1.0, 1.0], device=dev)
    vis = prefilter_voxel(cam, pc, pipe, bg)
    st = oracle_settings(oracle, cam.to("cpu"), bg.cpu().numpy())
    want = oracle.visible_filter(st, d["anchor"], np.exp(d["scaling"])[:, :3], np.tile(np.array([1, 0, 0, 0], np.float32), (512, 1)))
    assert np.array_equal(vis.cpu().numpy(), want > 0) and int(vis.sum()) > 0
    with torch.no_grad():
        out = render(cam, pc, pipe, bg, visible_mask=vis)
        xyz, color, opacity, scaling, rot, _, _ = generate_neural_gaussians(cam, pc, vis, is_training=True)
    f = oracle.forward(st, xyz.cpu().numpy(), opacity.cpu().numpy(), scaling.cpu().numpy(), rot.cpu().numpy(),
                       colors_precomp=color.cpu().numpy())
    same = f["margin"] > 1e-5
    assert same.mean() > 0.99
    assert np.abs(out["render"].cpu().numpy() - f["color"])[:, same].max() <= 1e-4       # the image tolerance of the parity suite
    assert np.array_equal(out["radii"].cpu().numpy(), f["radii"]) and int((out["radii"] > 0).sum()) > 100


def test_fused_expand_compact_matches_torch_chain():
    """The fused HIP expansion + compaction op == the reference's torch op chain
    (gaussian_renderer/__init__.py:68-111, restated in tests/torch_restatements.py and pinned by the golden
    fixture): identical mask / order, values to 1e-6, every gradient to rel-L2 1e-5; deterministic."""
    from splatco_amd.renderer import generate_neural_gaussians
    from torch_restatements import expand_torch_chain
    dev = torch.device("cuda:0")
    res = {}
    for fused in (False, True):
        pc, d = _model(dev)
        pc.train()
        cam = types.SimpleNamespace(camera_center=torch.tensor(d["camera_center"], device=dev), uid=0)
        vis = torch.tensor(d["visible_mask"], device=dev)
        out = generate_neural_gaussians(cam, pc, vis, is_training=True, expand=None if fused else expand_torch_chain)
        xyz, color, opacity, scaling, rot, neural_opacity, mask = out
        g = torch.Generator(device=dev).manual_seed(3)
        loss = sum((t * torch.randn(t.shape, device=dev, generator=g)).sum() for t in (xyz, color, opacity, scaling, rot))
        loss.backward()
        grads = {n: p.grad.clone() for n, p in pc.named_parameters() if p.grad is not None}
        res[fused] = ([t.detach() for t in out], grads)
    (o0, g0), (o1, g1) = res[False], res[True]
    want = np.load(os.path.join(GOLD, "neural_gaussians.npz"))
    assert torch.equal(o0[6], o1[6]) and np.array_equal(o1[6].cpu().numpy(), want["L0_train.mask"])
    for a, b, name in zip(o0[:6], o1[:6], ["xyz", "color", "opacity", "scaling", "rot", "neural_opacity"]):
        assert a.shape == b.shape, name
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), name
        np.testing.assert_allclose(b.cpu().numpy(), want[f"L0_train.{name}"], rtol=1e-4, atol=1e-5, err_msg=name)
    assert set(g0) == set(g1) and len(g0) > 10
    for n in g0:
        num = (g0[n] - g1[n]).norm().item()
        den = max(g0[n].norm().item(), 1e-20)
        assert num / den < 2e-4, (n, num / den)   # torch grid_sample backward itself is atomics-ordered
    # empty selection and determinism
    from splatco_amd.expand import expand_compact
    V, k = 7, 10
    z = lambda *s: torch.randn(*s, device=dev)
    no = -torch.rand(V * k, 1, device=dev)
    outs = expand_compact(no, z(V * k, 3), z(V * k, 7), z(V, k, 3), z(V, 6), z(V, 3), k)
    assert outs[0].shape == (0, 3) and not outs[5].any()
    no = torch.randn(100_003 * k, 1, device=dev)
    args = (no, z(100_003 * k, 3), z(100_003 * k, 7), z(100_003, k, 3), z(100_003, 6), z(100_003, 3), k)
    a, b = expand_compact(*args), expand_compact(*args)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ref_idx = torch.nonzero(no.view(-1) > 0).view(-1)
    assert torch.equal(a[2].view(-1), no.view(-1)[ref_idx])          # order-preserving compaction
    assert torch.equal(a[1], args[1][ref_idx])


@pytest.mark.parametrize("A,B,R", [(70, 70, 5), (133, 97, 3), (700, 700, 5)])
def test_plane_sample_backward_matches_grid_sample(A, B, R):
    """csrc/triplane.hip (tile-bucketed LDS scatter) == torch's grid_sample backward
    (scene/grids.py:148-150 semantics: bilinear, align_corners=True, zeros padding), including
    points outside the plane and on its border.  Tolerance: fp32 summation order only."""
    import torch.nn.functional as F
    from splatco_amd.triplane import plane_sample
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(A * 1000 + B)
    V = 300_000
    grid = torch.rand(V, 2, device=dev, generator=g) * 2.4 - 1.2          # ~30 % of the points leave [-1,1]
    grid[:1000] = torch.randint(0, 2, (1000, 2), device=dev, generator=g).float() * 2 - 1   # exact corners / borders
    grid[1000:2000, 0] = 1.0
    grid[2000:2010] = float("nan")
    w = torch.randn(V, R, device=dev, generator=g)
    p1 = (torch.randn(1, R, A, B, device=dev, generator=g)).requires_grad_()
    p2 = p1.detach().clone().requires_grad_()
    o1 = plane_sample(p1, grid)
    o2 = F.grid_sample(p2, grid.view(1, 1, V, 2), mode="bilinear", align_corners=True).flatten(0, 2).T
    ok = ~torch.isnan(grid).any(dim=1)
    assert torch.equal(o1[ok], o2[ok])
    w = torch.where(ok[:, None], w, torch.zeros_like(w))
    (o1[ok] * w[ok]).sum().backward()
    (o2[ok] * w[ok]).sum().backward()
    err = (p1.grad - p2.grad).abs().max().item()
    ref = p2.grad.abs().max().item()
    assert err <= 2e-5 * ref, (err, ref)
    assert torch.isfinite(p1.grad).all()


def test_plane_gradient_grid_bounds_the_error_of_quiet_nodes():
    """The exact plane sums round every term to a grid of 2^-29 of the largest |g| of the 32 x 32-cell TILE (csrc/triplane.hip,
    "DYNAMIC RANGE"): a quiet node in a tile that also holds a loud point is off by at most n_terms x 2^-30 x gmax(tile) --
    asserted per node here (the order test only bounds global norms) -- keeps its value to 1e-3 relative while its terms
    lie six decades below the loud one, and receives exactly zero once they lie more than 2^30 below it (the stated limit;
    fp32 sums would keep them).  Second case: gradient values with the largest finite exponent (2^127) -- the scale then
    is 2^-98 and the fixed-point terms stay inside int32 (clamped one exponent lower they overflowed)."""
    from splatco_amd.triplane import plane_sample
    dev = torch.device("cuda:0")
    A = B = 65          # 64 intervals: node coordinates and the grid -> pixel map are exact in fp32
    R = 5

    def run(points, weights):
        p = torch.zeros(1, R, A, B, device=dev, requires_grad=True)
        (plane_sample(p, points) * weights).sum().backward()
        return p.grad[0]

    def coord(node):            # grid coordinate of node index `node` (align_corners=True): exactly on the node
        return node / (A - 1) * 2.0 - 1.0

    gen = torch.Generator(device=dev).manual_seed(5)
    n_quiet = 2000
    for decades, expect_zero in ((6, False), (10, True)):
        quiet = 10.0 ** -decades
        # tile 0 (nodes 0..32): one loud point ON node (3, 3); n_quiet points scattered inside cell (20, 20)
        pts = torch.empty(n_quiet + 1, 2, device=dev)
        pts[0] = torch.tensor([coord(3), coord(3)], device=dev)
        frac = torch.rand(n_quiet, 2, device=dev, generator=gen) * 0.98 + 0.01
        pts[1:, 0] = ((20 + frac[:, 0]) / (B - 1)) * 2.0 - 1.0
        pts[1:, 1] = ((20 + frac[:, 1]) / (A - 1)) * 2.0 - 1.0
        wts = torch.full((n_quiet + 1, R), quiet, device=dev)
        wts[0] = 1.0
        got = run(pts, wts)
        assert abs(float(got[0, 3, 3]) - 1.0) <= 1e-6
        # the four nodes of cell (20, 20): exact sums of the fp32 terms in float64, with the kernel's own fractions
        ix, iy = ((pts[1:, 0] + 1.0) * 0.5) * float(B - 1), ((pts[1:, 1] + 1.0) * 0.5) * float(A - 1)
        fb, fa = (ix - ix.floor()), (iy - iy.floor())
        assert bool((ix.floor() == 20).all() and (iy.floor() == 20).all())
        for da, db, wt in ((0, 0, (1 - fa) * (1 - fb)), (0, 1, (1 - fa) * fb), (1, 0, fa * (1 - fb)), (1, 1, fa * fb)):
            exact = float((wt * quiet).double().sum())
            node = float(got[0, 20 + da, 20 + db])
            bound = n_quiet * 2.0 ** -30 * 1.0 + 4 * 2.0 ** -24 * abs(exact)      # the grid (gmax = 1) + the fp32 roundings of a node
            assert abs(node - exact) <= bound, (decades, da, db, node, exact, bound)
            if expect_zero:
                assert node == 0.0                      # every term is below half a grid step: the documented limit
            else:
                assert abs(node - exact) <= 1e-3 * abs(exact), (node, exact)
    # largest finite exponent
    pts = torch.tensor([[coord(3), coord(3)], [coord(10), coord(12)]], device=dev)
    big = torch.full((2, R), 2.0 ** 127, device=dev)
    big[1] = -1.5 * 2.0 ** 126
    got = run(pts, big)
    assert float(got[0, 3, 3]) == 2.0 ** 127 and float(got[0, 12, 10]) == -1.5 * 2.0 ** 126 and bool(torch.isfinite(got).all())
    assert int((got != 0).sum()) == 2 * R


@pytest.mark.parametrize("A,B,R,sheet", [(70, 70, 5, False), (133, 97, 10, False), (256, 256, 15, False), (40, 40, 2, False),
                                         (256, 256, 5, True), (200, 300, 10, True), (256, 256, 15, True)])
def test_plane_gradients_do_not_depend_on_the_order_of_the_points(A, B, R, sheet):
    """csrc/triplane.hip, exact cell sums (64-bit fixed point on a per-tile grid): the plane gradient is a function of the
    SET of points -- the same bits for any permutation of the rows (which changes every arrival order in the scatter and
    in the cell ranks far more than two runs of the same call do), run after run; and it is an order of magnitude closer to
    the exact sum of its fp32 terms than torch's fp32 atomics are.  R = 15 takes the two-round path (more than ten channels), R = 2 the
    two-workgroups-per-CU instantiation.  A non-finite gradient value sends its tile through the fp32 sums: NaN reaches
    exactly the nodes torch's backward poisons.
    sheet: three quarters of the points lie in a strip one tile high (a flat scene seen edge-on) -- those tiles hold several
    times the plane's mean and are SPLIT over several workgroups whose integer cell sums meet in whatever order they
    finish: the same bits again, and the same accuracy."""
    import torch.nn.functional as F
    from splatco_amd.triplane import plane_sample
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(A * 7 + R)
    V = 400_000
    grid = torch.rand(V, 2, device=dev, generator=g) * 2.2 - 1.1
    grid[:50_000] = grid[:50_000] * 0.02 + 0.3                          # a dense clump: thousands of points per cell, several chunks per tile
    grid[50_000:51_000] = torch.randint(0, 2, (1000, 2), device=dev, generator=g).float() * 2 - 1
    if sheet:
        grid[60_000:360_000, 1] = grid[60_000:360_000, 1] * 0.02 + 0.1
    # gradients over six decades, so that quiet tiles next to loud ones are covered
    w = torch.randn(V, R, device=dev, generator=g) * torch.exp(torch.rand(V, 1, device=dev, generator=g) * 14 - 7)

    def grad_of(order, wts=w, dtype=torch.float32, ours=True):
        p = torch.zeros(1, R, A, B, device=dev, dtype=dtype, requires_grad=True)
        gr, ww = grid[order].to(dtype), wts[order].to(dtype)
        o = plane_sample(p, gr) if ours else F.grid_sample(p, gr.view(1, 1, -1, 2), mode="bilinear", align_corners=True).flatten(0, 2).T
        (o * ww).sum().backward()
        return p.grad

    ident = torch.arange(V, device=dev)
    base = grad_of(ident)
    assert torch.equal(grad_of(ident), base)
    for seed in (1, 2):
        perm = torch.randperm(V, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
        assert torch.equal(grad_of(perm), base), "plane gradient depends on the order of the points"
    assert torch.equal(grad_of(ident.flip(0)), base)
    # the yardstick: the kernel's own fp32 weights and fp32 products (tp_cell's operation order), summed in fp64 -- what
    # an exact summation of the same terms gives.  (Against an all-fp64 grid_sample both fp32 evaluations sit at ~5e-6:
    # the bilinear fractions of an fp32 coordinate times 132 carry 1e-5 of rounding, shared by torch and this kernel.)
    ix, iy = ((grid[:, 0] + 1.0) * 0.5) * float(B - 1), ((grid[:, 1] + 1.0) * 0.5) * float(A - 1)
    fx, fy = ix.floor(), iy.floor()
    fb, fa, b0, a0 = ix - fx, iy - fy, fx.long(), fy.long()
    exact = torch.zeros(R, A * B, device=dev, dtype=torch.float64)
    for da, db, wt in ((0, 0, (1.0 - fa) * (1.0 - fb)), (0, 1, (1.0 - fa) * fb), (1, 0, fa * (1.0 - fb)), (1, 1, fa * fb)):
        a, b = a0 + da, b0 + db
        ok = (a >= 0) & (a < A) & (b >= 0) & (b < B)
        exact.index_add_(1, (a * B + b)[ok], (w[ok] * wt[ok, None]).T.double())
    exact = exact.view(1, R, A, B)
    t32 = grad_of(ident, ours=False)
    ours_err = float((base.double() - exact).norm() / exact.norm())
    torch_err = float((t32.double() - exact).norm() / exact.norm())
    print(f"[plane backward {A}x{B} R={R}] rel-L2 to the exact sum of the same fp32 terms: this kernel {ours_err:.2e}, torch's fp32 atomics {torch_err:.2e}")
    # a node is the sum of the corner sums of up to four cells (each exact, rounded to fp32 once) and, on a tile border, of up
    # to four tiles' shares, added in a fixed order: a handful of roundings per node where torch's atomics take one per
    # point (measured: 0.9 - 1.3e-7 against 0.8 - 1.8e-6); plus the fixed-point grid, 2^-30 of the tile's largest gradient
    # value per term
    assert ours_err <= 2.0 ** -22 and ours_err <= 0.5 * torch_err, (ours_err, torch_err)
    # worst node: seven roundings (four cell sums, three additions) of half an ulp of a value near the largest
    assert float((base.double() - exact).abs().max()) <= 7 * 2.0 ** -24 * float(exact.abs().max())
    ref64 = exact
    # non-finite values: as torch
    wn = w.clone()
    wn[123_456, 0] = float("nan")                   # (sheet: inside the strip -- a split tile falls back to one workgroup)
    wn[234_567, R - 1] = float("inf")
    wn[10, 0] = float("nan")                        # inside the clump
    ours_n, torch_n = grad_of(ident, wn), grad_of(ident, wn, ours=False)
    assert torch.equal(torch.isfinite(ours_n), torch.isfinite(torch_n))
    fin = torch.isfinite(torch_n)
    assert 0 < int((~fin).sum()) <= 12
    assert float((ours_n[fin].double() - ref64[fin]).norm() / ref64[fin].norm()) <= 1e-5       # the poisoned tile: fp32 sums
    assert torch.equal(grad_of(ident, torch.zeros_like(w)), torch.zeros_like(base))              # all-zero gradients: a zero tile maximum


@pytest.mark.parametrize("V", [200_000, 300_000])   # below / above triplane.CHANNEL_LAST_MIN_POINTS (both plane layouts)
@pytest.mark.parametrize("TA", [False, True])
def test_triplane_forward_backward_matches_grid_sample(TA, V):
    """csrc/triplane.hip fused three-plane forward (written straight into the concatenated feature
    matrix) and strided LDS backward == the grid_sample / cat formulation of scene/grids.py:146-182,
    for the plain and the attention (TA) grid; PlaneGrid golden fixture on the GPU as well."""
    from splatco_amd.scene_model import PlaneGrid
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    ws = [64, 64, 64] if TA else [60, 70, 50]      # the attention grid stacks the planes: equal sizes (scene/grids.py:166)
    pg = PlaneGrid(15, ws, [-2.0] * 3, [2.0] * 3, TAflag=TA).to(dev)
    ref = PlaneGrid(15, ws, [-2.0] * 3, [2.0] * 3, TAflag=TA).to(dev)
    ref.load_state_dict(pg.state_dict())
    xyz = torch.rand(V, 3, device=dev) * 4.6 - 2.3             # some anchors leave the [-2,2] box
    xyz[:500] = torch.randint(0, 2, (500, 3), device=dev).float() * 4 - 2   # exact corners / borders
    out = pg(xyz)
    # reference formulation: force the unfused path by asking for a coordinate gradient
    xr = xyz.clone().requires_grad_()
    out_ref = ref(xr)
    assert out.shape == out_ref.shape == (V, 30 if TA else 15)
    assert torch.allclose(out, out_ref, rtol=1e-5, atol=1e-6), (out - out_ref).abs().max().item()
    w = torch.randn_like(out)
    (out * w).sum().backward()
    (out_ref * w).sum().backward()
    for (n, a), (_, b) in zip(pg.named_parameters(), ref.named_parameters()):
        err, scale = (a.grad - b.grad).abs().max().item(), b.grad.abs().max().item()
        assert err <= 5e-5 * scale + 1e-7, (n, err, scale)


@pytest.mark.parametrize("name,ta", [("plain", False), ("ta", True)])
def test_plane_grid_golden_on_gpu(name, ta):
    """tests/golden/planegrid.npz (captured from the reference's scene/grids.py) through the fused kernel."""
    from splatco_amd.scene_model import PlaneGrid
    d = np.load(os.path.join(GOLD, "planegrid.npz"))
    dev = torch.device("cuda:0")
    pg = PlaneGrid(15, [24, 24, 24], [-2.0, -2.0, -2.0], [2.0, 2.0, 2.0], TAflag=ta)
    pre = name + "."
    pg.load_state_dict({k[len(pre):]: torch.tensor(d[k]) for k in d.files if k.startswith(pre) and ".out" not in k})
    with torch.no_grad():
        y = pg.to(dev)(torch.tensor(d["xyz"], device=dev), 0)
    np.testing.assert_allclose(y.cpu().numpy(), d[f"{name}.out"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name,ta", [("plain", False), ("ta", True)])
def test_plane_grid_training_noise_on_gpu(name, ta):
    """Q = 0.03 (the training setting, scene/gaussian_model.py:187,213) through the fused kernel: the attention
    grid's output equals its Q = 0 output bit for bit (scene/grids.py:160-181 discards the noised samples), a
    plain grid's differs by at most 0.5 Q per element and is uniformly spread."""
    from splatco_amd.scene_model import PlaneGrid
    d = np.load(os.path.join(GOLD, "planegrid.npz"))
    dev = torch.device("cuda:0")
    pg = PlaneGrid(15, [24, 24, 24], [-2.0, -2.0, -2.0], [2.0, 2.0, 2.0], TAflag=ta)
    pre = name + "."
    pg.load_state_dict({k[len(pre):]: torch.tensor(d[k]) for k in d.files if k.startswith(pre) and ".out" not in k})
    pg = pg.to(dev)
    xyz = torch.tensor(d["xyz"], device=dev)
    with torch.no_grad():
        y0, yq = pg(xyz, 0), pg(xyz, 0.03)
    if ta:
        assert torch.equal(y0, yq)
    else:
        diff = (yq - y0).abs()
        assert 0 < diff.max().item() <= 0.5 * 0.03 * (1 + 1e-5)
        assert abs(diff.mean().item() - 0.25 * 0.03) < 0.02 * 0.03     # E|U(-0.5, 0.5)| = 0.25
    np.testing.assert_allclose(y0.cpu().numpy(), d[f"{name}.out"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("H,W", [(64, 64), (70, 133), (1080, 1920)])
def test_fused_l1_ssim_matches_torch(H, W):
    """csrc/ssim.hip == the torch restatement of utils/loss_utils.py (itself pinned by the golden
    fixture losses.npz): values to 1e-5 relative, gradient rel-L2 <= 1e-4, bit-reproducible."""
    from splatco_amd.losses import l1_loss, l1_ssim, ssim
    dev = torch.device("cuda:0")
    if (H, W) == (64, 64):
        d = np.load(os.path.join(GOLD, "losses.npz"))
        a, b = torch.tensor(d["a1"], device=dev), torch.tensor(d["b1"], device=dev)
    else:
        g = torch.Generator(device=dev).manual_seed(H)
        a = torch.rand(3, H, W, device=dev, generator=g)
        b = (a + 0.15 * torch.randn(3, H, W, device=dev, generator=g)).clamp(0, 1)
    x1 = a.clone().requires_grad_()
    x2 = a.clone().requires_grad_()
    l1f, sf = l1_ssim(x1, b)
    l1t, st_ = l1_loss(x2, b), ssim(x2, b)
    assert abs(l1f.item() - l1t.item()) <= 1e-5 * abs(l1t.item())
    assert abs(sf.item() - st_.item()) <= 1e-5 * abs(st_.item())
    if (H, W) == (64, 64):
        assert abs(sf.item() - float(d["ssim_1"])) <= 1e-5 and abs(l1f.item() - float(d["l1_1"])) <= 1e-6
    (0.8 * l1f + 0.2 * (1.0 - sf)).backward()
    (0.8 * l1t + 0.2 * (1.0 - st_)).backward()
    rel = ((x1.grad - x2.grad).norm() / x2.grad.norm()).item()
    assert rel <= 1e-4, rel
    x3 = a.clone().requires_grad_()
    l1g, sg = l1_ssim(x3, b)
    (0.8 * l1g + 0.2 * (1.0 - sg)).backward()
    assert torch.equal(x3.grad, x1.grad) and torch.equal(sg, sf)


def test_collaborative_step_runs_and_updates_parameters():
    """configs[3]/[4] counterpart on one rank: mv = 2 views, one backward, Adam step."""
    from splatco_amd.train_step import collaborative_step
    dev = torch.device("cuda:0")
    pc, d = _model(dev)
    pc.train()
    cams = [look_at_camera(eye=(0.3 + 0.4 * i, -0.2, -4.5), target=(0, 0, 0), up=(0, -1, 0), FoVx=math.radians(60),
                           width=160, height=96, uid=i).to(dev) for i in range(2)]
    gts = [torch.rand(3, 96, 160) for _ in cams]
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    opt = torch.optim.Adam([p for p in pc.parameters() if p.requires_grad], lr=1e-3)
    before = pc._anchor_feat.detach().clone()
    loss, out, _ = collaborative_step(pc, cams, gts, pipe, torch.ones(3, device=dev), optimizer=opt)
    assert torch.isfinite(loss) and out["render"].shape == (3, 96, 160)
    assert not torch.equal(before, pc._anchor_feat.detach())
    assert out["viewspace_points"].grad is not None
    # with the cross-view consistency term (train.py:201-239) and the densification statistics of the last
    # view (train.py:266): alike ground-truth views so that SSIM(gt_i, gt_j) > 0.6 switches the term on
    from splatco_amd.densify import AnchorDensifier
    base = torch.rand(3, 96, 160)
    gts2 = [(base + 0.01 * i).clamp(0, 1) for i in range(2)]
    den = AnchorDensifier(pc, opt, voxel_size=0.01)
    loss2, out2, _ = collaborative_step(pc, cams, gts2, pipe, torch.ones(3, device=dev), optimizer=opt,
                                        consistency_weight=0.05, densifier=den)
    loss_plain, _, _ = collaborative_step(pc, cams, gts2, pipe, torch.ones(3, device=dev))
    assert torch.isfinite(loss2) and den.anchor_demon.sum() > 0 and den.offset_denom.sum() > 0
    assert den.opacity_accum.shape == (pc.get_anchor.shape[0], 1)


def test_backward_gradients_share_one_arena():
    """The operator's backward carves all per-Gaussian gradients from one buffer with the parameter
    gradients adjacent, so the sharded mv step all-reduces them in place (multiview._shared_arena)."""
    from splatco_amd import rasterizer as R
    from splatco_amd.multiview import _shared_arena, allreduce_gradients
    from splatco_amd.synthetic import synthetic_camera, synthetic_gaussians
    dev = torch.device("cuda:0")
    cam, g = synthetic_camera(160, 96), synthetic_gaussians(3000, 160, 96, 2)
    rs = R.GaussianRasterizationSettings(96, 160, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), torch.tensor(g["bg"], device=dev),
                                         1.0, cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), 1,
                                         cam.camera_center.to(dev), False, False)
    t = lambda a: torch.tensor(a, device=dev, requires_grad=True)
    m, o, s, r, c = t(g["means3D"]), t(g["opacities"]), t(g["scales"]), t(g["rotations"]), t(g["colors"])
    m2d = torch.zeros(3000, 3, device=dev, requires_grad=True)
    img, _ = R.GaussianRasterizer(rs)(means3D=m, means2D=m2d, opacities=o, colors_precomp=c, scales=s, rotations=r)
    img.square().sum().backward()
    arena = _shared_arena([m, o, s, r, c])
    assert arena is not None and arena.numel() == 3000 * 14
    before = [p.grad.clone() for p in (m, o, s, r, c)]
    assert allreduce_gradients([m, o, s, r, c]).data_ptr() == arena.data_ptr()     # world size 1: nothing moves
    assert all(torch.equal(a, p.grad) for a, p in zip(before, (m, o, s, r, c)))
    assert m2d.grad is not None and m2d.grad.shape == (3000, 3)


def test_training_statis_kernel_golden_and_random():
    """csrc/densify.hip (GaussianModel.training_statis, scene/gaussian_model.py:761-782) against the reference's own
    numbers (tests/golden/training_statis.npz) and, on a larger random case accumulated over three views, against the
    torch restatement; bit-reproducible."""
    from splatco_amd.stats import statis_apply, statis_increments, training_statis
    from torch_restatements import training_statis_torch
    dev = torch.device("cuda:0")
    d = np.load(os.path.join(GOLD, "training_statis.npz"))
    k = int(d["n_offsets"])
    Nn = d["anchor_visible_mask"].shape[0]
    t = lambda n: torch.tensor(d[n], device=dev)
    acc = [torch.zeros(Nn, 1, device=dev), torch.zeros(Nn, 1, device=dev), torch.zeros(Nn * k, 1, device=dev),
           torch.zeros(Nn * k, 1, device=dev)]
    training_statis(*acc, k, t("viewspace_grad"), t("neural_opacity"), t("update_filter"), t("offset_selection_mask"),
                    t("anchor_visible_mask"))
    for got, name in zip(acc, ["opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom"]):
        np.testing.assert_allclose(got.cpu().numpy(), d[name], rtol=1e-6, atol=1e-7, err_msg=name)
    g = torch.Generator(device=dev).manual_seed(5)
    N, k = 200_003, 10
    a1 = [torch.rand(N, 1, device=dev, generator=g), torch.rand(N, 1, device=dev, generator=g).round(),
          torch.rand(N * k, 1, device=dev, generator=g), torch.rand(N * k, 1, device=dev, generator=g).round()]
    a2 = [a.clone() for a in a1]
    a3 = [a.clone() for a in a1]
    for view in range(3):
        vis = torch.rand(N, device=dev, generator=g) < 0.6
        V = int(vis.sum())
        no = torch.randn(V * k, 1, device=dev, generator=g)
        sel = (no > 0).view(-1)
        P = int(sel.sum())
        upd = torch.rand(P, device=dev, generator=g) < 0.7
        grad = torch.randn(P, 3, device=dev, generator=g)
        training_statis(*a1, k, grad, no, upd, sel, vis)
        training_statis_torch(*a2, k, grad, no, upd, sel, vis)
        inc = statis_increments(k, grad, no, upd, sel)                  # the two-step form of the sharded step
        statis_apply(*a3, k, vis.nonzero().squeeze(1), *inc)
    for x, y, z in zip(a1, a2, a3):
        assert torch.allclose(x, y, rtol=1e-6, atol=1e-6)
        assert torch.equal(x, z)
    with pytest.raises(RuntimeError):
        training_statis(*[a.cpu() for a in a1], k, grad.cpu(), no.cpu(), upd.cpu(), sel.cpu(), vis.cpu())


@pytest.mark.parametrize("V", [1, 37, 100_003])
def test_fused_mlp_heads_match_the_torch_chain(V):
    """csrc/mlp_heads.hip (fp32 MFMA, x / hidden layer never in HBM) == the module chain of
    scene/gaussian_model.py:315-337 on x = cat(feat, ob_view, geo_fea) (gaussian_renderer/__init__.py:34-93):
    outputs to 1e-5 (abs + rel), every gradient (inputs, anchor through ob_view, all weights and biases) to rel-L2 1e-4 (fp32
    summation order over V rows is the only difference); bit-reproducible."""
    from splatco_amd.mlp_heads import mlp_heads, supported
    from splatco_amd.scene_model import AnchorGaussianModel
    dev = torch.device("cuda:0")
    torch.manual_seed(V)
    pc = AnchorGaussianModel(plane_size=16, num_channels=15).to(dev)
    with torch.no_grad():
        for p in list(pc.mlp_opacity.parameters()) + list(pc.mlp_color.parameters()) + list(pc.mlp_cov.parameters()):
            p.add_(0.2 * torch.randn_like(p))
    g = torch.Generator(device=dev).manual_seed(V + 1)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    feat, anchor, geo, cam = r(V, 32), r(V, 3) * 2, r(V, 64), torch.tensor([0.3, -0.2, -5.0], device=dev)
    two_parts = V != 37          # geo_fea as one [V,64] matrix or as its two [V,32] halves
    w = [r(V, 10), r(V, 30), r(V, 70)]
    res = {}
    for fused in (True, False, True):
        f, a, ge = (t.clone().requires_grad_() for t in (feat, anchor, geo))
        for p in pc.parameters():
            p.grad = None
        if fused:
            assert supported(pc, f, ge)
            outs = mlp_heads(pc, f, a, cam, ge[:, :32].contiguous(), ge[:, 32:].contiguous()) if two_parts else mlp_heads(pc, f, a, cam, ge)
        else:
            ob = a - cam
            ob = ob / ob.norm(dim=1, keepdim=True)
            x = torch.cat([f, ob, ge], dim=1)
            outs = (pc.mlp_opacity(x), pc.mlp_color(x), pc.mlp_cov(x))
        sum((o * wi).sum() for o, wi in zip(outs, w)).backward()
        grads = {"feat": f.grad, "anchor": a.grad, "geo": ge.grad}
        grads.update({n: p.grad.clone() for n, p in pc.named_parameters() if n.startswith("mlp_")})
        res.setdefault(fused, []).append(([o.detach() for o in outs], grads))
    (o1, g1), (o1b, g1b) = res[True]
    (o0, g0), = res[False]
    for a_, b_, name in zip(o1, o0, ("opacity", "color", "cov")):
        assert a_.shape == b_.shape
        assert torch.allclose(a_, b_, rtol=1e-5, atol=1e-5), (name, (a_ - b_).abs().max().item())
    assert set(g1) == set(g0) and len(g1) == 3 + 12
    for n in g0:
        err = (g1[n] - g0[n]).norm().item() / max(g0[n].norm().item(), 1e-20)
        assert err <= 1e-4, (n, err)
        assert torch.equal(g1[n], g1b[n]), n                # bit-reproducible
    assert all(torch.equal(x_, y_) for x_, y_ in zip(o1, o1b))


def test_generate_neural_gaussians_fused_heads_golden():
    """The whole anchor path with the fused heads against the reference's fixture (neural_gaussians.npz)."""
    from splatco_amd.renderer import generate_neural_gaussians
    dev = torch.device("cuda:0")
    pc, d = _model(dev)
    pc.train()
    cam = types.SimpleNamespace(camera_center=torch.tensor(d["camera_center"], device=dev), uid=0)
    vis = torch.tensor(d["visible_mask"], device=dev)
    with torch.no_grad():
        out = generate_neural_gaussians(cam, pc, vis, is_training=True, fused_heads=True)
    assert np.array_equal(out[6].cpu().numpy(), d["L0_train.mask"])
    for t, name in zip(out[:6], ["xyz", "color", "opacity", "scaling", "rot", "neural_opacity"]):
        np.testing.assert_allclose(t.cpu().numpy(), d[f"L0_train.{name}"], rtol=1e-4, atol=1e-5, err_msg=name)


@pytest.mark.parametrize("case", [0, 1])
def test_adjust_anchor_on_the_gpu_matches_the_reference(case):
    """splatco_amd.densify on device tensors against tests/golden/densify.npz (the reference's own adjust_anchor: growth,
    pruning, Adam-state surgery; case 1 = iteration 1600 runs the curvature branch -> device kNN + covariance kernels).
    The random candidate pick is drawn from the same CPU stream as the fixture's and moved to the device."""
    from test_densify_io import NAMES, _case
    d = np.load(os.path.join(GOLD, "densify.npz"))
    dev = torch.device("cuda:0")
    m, opt, den, pre = _case(d, case)
    # move the model, the optimizer state and the accumulators to the device
    for n in NAMES:
        old = getattr(m, "_" + n)
        new = torch.nn.Parameter(old.detach().to(dev), requires_grad=old.requires_grad)
        for grp in opt.param_groups:
            if grp["params"][0] is old:
                grp["params"][0] = new
        if old in opt.state:
            st = opt.state.pop(old)
            opt.state[new] = {k_: (v.to(dev) if torch.is_tensor(v) and k_ != "step" else v) for k_, v in st.items()}
        setattr(m, "_" + n, new)
    for n in ("offset_gradient_accum", "offset_denom", "opacity_accum", "anchor_demon", "max_radii2D"):
        setattr(den, n, getattr(den, n).to(dev))
    den.rand = lambda shape, device: torch.rand(shape).to(device)
    torch.manual_seed(int(d[pre + "seed"]))
    den.adjust_anchor(iteration=int(d[pre + "iteration"]), check_interval=100, success_threshold=0.8,
                      grad_threshold=0.0002, min_opacity=0.005)
    for n in NAMES:
        got = getattr(m, "_" + n).detach().cpu().numpy()
        assert getattr(m, "_" + n).is_cuda and got.shape == d[pre + "out." + n].shape, n
        np.testing.assert_allclose(got, d[pre + "out." + n], rtol=1e-6, atol=1e-7, err_msg=n)
        if pre + "out.exp_avg." + n in d.files:
            st = opt.state[getattr(m, "_" + n)]
            np.testing.assert_allclose(st["exp_avg"].cpu().numpy(), d[pre + "out.exp_avg." + n], rtol=1e-6, atol=1e-9)
    for n in ("offset_gradient_accum", "offset_denom", "opacity_accum", "anchor_demon", "max_radii2D"):
        np.testing.assert_allclose(getattr(den, n).cpu().numpy(), d[pre + "out." + n], rtol=1e-6, atol=1e-7, err_msg=n)


def test_device_knn_is_exact_and_curvature_matches():
    """csrc/densify.hip kNN (grid-bucketed, one thread per query) == brute force on 150 k points with clusters, planes
    and duplicates; compute_curvature == the reference's numbers (densify.npz) and the eigvalsh formulation; 5 M points
    (configs[2] scale, where the reference would go to sklearn on the host) run and are self-consistent."""
    from splatco_amd.densify import _knn_indices, compute_curvature
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    N, k = 150_000, 10
    pts = torch.rand(N, 3, device=dev, generator=g) * 4 - 2
    pts[:30_000] = torch.randn(30_000, 3, device=dev, generator=g) * 0.01 + 0.3                # a dense clump
    pts[30_000:60_000, 2] = 0.25                                                               # a plane
    pts[60_000:60_500] = pts[0]                                                                # duplicates (zero distances)
    idx = _knn_indices(pts, k)
    assert idx.shape == (N, k) and idx.dtype == torch.long and int(idx.min()) >= 0
    probe = torch.randint(0, N, (3000,), device=dev, generator=g)
    probe[:200] = torch.arange(60_000, 60_200, device=dev)
    dist = torch.cdist(pts[probe].double(), pts.double())
    dist[torch.arange(len(probe)), probe] = float("inf")
    want = dist.topk(k, dim=1, largest=False).values
    got = (pts[idx[probe]].double() - pts[probe].double()[:, None]).norm(dim=2)
    assert not (idx[probe] == probe[:, None]).any()                    # never the query itself
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-7), (got - want).abs().max()            # the same distances, nearest first
    d = np.load(os.path.join(GOLD, "densify.npz"))
    anchors = torch.tensor(d["c1.in.anchor"], device=dev)
    cur = compute_curvature(anchors)
    np.testing.assert_allclose(cur.cpu().numpy(), d["c1.curvature"], rtol=2e-4, atol=1e-6)
    nb = pts[idx].double()
    c = nb - nb.mean(dim=1, keepdim=True)
    ev = torch.linalg.eigvalsh(c.transpose(1, 2) @ c / (k - 1))
    ref = (ev[:, 0] / ev.sum(dim=1))
    ok = ev.sum(dim=1) > 1e-12
    assert torch.allclose(compute_curvature(pts)[ok].double(), ref[ok], rtol=1e-4, atol=1e-6)
    big = torch.rand(5_000_000, 3, device=dev, generator=g) * 4 - 2
    cb = compute_curvature(big)
    assert cb.shape == (5_000_000,) and torch.isfinite(cb).all() and 0.0 <= float(cb.min()) and float(cb.max()) <= 1.0 / 3 + 1e-4


def test_fused_anchor_gather_matches_the_torch_ops():
    """csrc/anchor_gather.hip == the index_select x4 / exp / cat chain of gaussian_renderer/__init__.py:23-31: values
    bit-exact (exp to 1 ulp), parameter gradients exact sums of the upstream gradients, zeros for invisible anchors."""
    from splatco_amd.anchor_gather import gather_anchors
    from splatco_amd.scene_model import AnchorGaussianModel
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    N = 50_001
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    res = []
    vis = torch.rand(N, device=dev, generator=g) < 0.6
    idx = vis.nonzero().squeeze(1)
    ws = None
    for fused in (True, False):
        pc = AnchorGaussianModel(plane_size=16, num_channels=15).to(dev)
        g2 = torch.Generator(device=dev).manual_seed(2)
        r2 = lambda *s: torch.randn(*s, device=dev, generator=g2)
        pc.set_anchors(r2(N, 3), r2(N, 10, 3), r2(N, 32), r2(N, 6) * 0.3 - 3)
        if fused:
            outs = gather_anchors(pc, idx)
        else:
            feat, anchor = pc._anchor_feat.index_select(0, idx), pc.get_anchor.index_select(0, idx)
            off, gs = pc._offset.index_select(0, idx), pc.get_scaling.index_select(0, idx)
            outs = (feat, anchor, off, gs, torch.cat((feat, anchor, off.reshape(len(idx), -1), gs), dim=1))
        if ws is None:
            ws = [r(*o.shape) for o in outs]
        sum((o * w).sum() for o, w in zip(outs, ws)).backward()
        res.append(([o.detach() for o in outs], [p.grad for p in (pc._anchor_feat, pc._anchor, pc._offset, pc._scaling)]))
    (o1, g1), (o0, g0) = res
    for a, b in zip(o1, o0):
        assert a.shape == b.shape and torch.allclose(a, b, rtol=2e-7, atol=0)
    assert torch.equal(o1[0], o0[0]) and torch.equal(o1[2], o0[2])
    for a, b in zip(g1, g0):
        assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-6, atol=1e-7)
        assert torch.all(a[~vis] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("N,second_use", [(40, False), (50_001, False), (50_001, True), (1_400_003, False)])
def test_gather_backward_forms_the_batchnorm_linear_dx_itself(N, second_use):
    """Round 6 hand-over (anchor_gather.DeferredDx, csrc/anchor_gather.hip DX): with g_fea feeding the fused BatchNorm-Linear,
    that op's backward leaves its coefficients and a stride-0 zero gradient instead of the [V,72] dx matrix, and the
    gather's backward forms dx = k0 + x k1 + dy Gi per workgroup with fp32 MFMAs.  Same parameter gradients as the path that
    materialises dx (same chain of fp32 FMAs per element up to the order of the 32-term sum: 1e-6 of the tensor's scale),
    also per anchor RANGE (what the sharded step does), also when g_fea has a second consumer whose gradient autograd adds
    to the token, and nothing is deferred when the BatchNorm-Linear is not the fused one."""
    from splatco_amd import anchor_gather as ag
    from splatco_amd import scene_model as sm
    from splatco_amd.scene_model import AnchorGaussianModel
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N + 17)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    params = (r(N, 3) * 2, r(N, 10, 3), r(N, 32) * 3 + 0.5, r(N, 6) * 0.3 - 3)
    idx = (torch.rand(N, device=dev, generator=g) < 0.8).nonzero().squeeze(1)
    V = idx.numel()
    G, c = (r(32, 71) * 0.2).requires_grad_(), r(32).requires_grad_()
    w_y, w_feat, w_off, w_gs, w_anc, w_g = r(V, 32), r(V, 32), r(V, 10, 3), r(V, 6), r(V, 3), r(V, 71)

    def run(defer, ranges=None):
        pc = AnchorGaussianModel(plane_size=16, num_channels=15).to(dev)
        pc.set_anchors(*(t.clone() for t in params))
        sink = None
        if ranges:
            grads = [torch.full_like(p, float("nan")) for p in (pc._anchor_feat, pc._anchor, pc._offset, pc._scaling)]
            sink = ag.GradSink(*grads)
            sink.ranges, seen = ranges, []
            sink.on_range = seen.append
            pc._grad_sink = sink
        feat, anc, off, gs, g_fea = ag.gather_anchors(pc, idx)
        box = g_fea._scr_deferred_dx
        if not defer:
            del g_fea._scr_deferred_dx
        for t in (G, c):
            t.grad = None
        y, _, _ = sm._NormLinearFn.apply(g_fea, G, c, 1e-5, getattr(g_fea, "_scr_col_stats", None),
                                         getattr(g_fea, "_scr_deferred_dx", None))
        loss = (y * w_y).sum() + (feat * w_feat).sum() + (off * w_off).sum() + (gs * w_gs).sum() + (anc * w_anc).sum()
        if second_use:
            loss = loss + (g_fea * w_g).sum()
        loss.backward()
        assert box.coef is None                                     # released behind the backward
        if ranges:
            assert seen == list(range(len(ranges)))
            out = grads
        else:
            out = [p.grad for p in (pc._anchor_feat, pc._anchor, pc._offset, pc._scaling)]
        return [t.detach().clone() for t in out] + [G.grad.clone(), c.grad.clone()]

    want = run(False)
    got = run(True)
    step = max(64, (N // 3 + 63) // 64 * 64)
    rng = [(a, min(N, a + step)) for a in range(0, N, step)]
    got_r = run(True, rng)
    vis = torch.zeros(N, dtype=torch.bool, device=dev)
    vis[idx] = True
    for name, a, b, b2 in zip(("feat", "anchor", "offset", "scaling", "G", "c"), want, got, got_r):
        scale = float(a.abs().max())
        assert a.shape == b.shape == b2.shape and torch.isfinite(b).all() and torch.isfinite(b2).all(), name
        assert float((a - b).abs().max()) <= 2e-6 * scale, (name, float((a - b).abs().max()), scale)
        assert torch.equal(b, b2), name            # a range is the same kernel on offset pointers: the same bits
        if name in ("feat", "anchor", "offset", "scaling"):
            assert bool((b[~vis] == 0).all()), name
    # the unfused BatchNorm-Linear (torch ops) defers nothing and still agrees
    sm.NORM_LINEAR_HIP = False
    try:
        ref = run(True)
    finally:
        sm.NORM_LINEAR_HIP = True
    for name, a, b in zip(("feat", "anchor", "offset", "scaling"), ref, got):
        assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max()), name


@pytest.mark.gpu
@pytest.mark.parametrize("V,layout,second_use", [(3000, "10-5-5", False), (300_017, "10-5-5", False), (300_017, "10-5-5", True),
                                                 (100_003, "5-5", False), (100_003, "15-5", False), (50_000, "4", False)])
def test_triplane_backward_forms_the_batchnorm_linear_dx_itself(V, layout, second_use):
    """Round 6 hand-over on the plane branch (csrc/triplane.hip tp_scatter9_kernel DX): with the sampled matrix feeding the
    fused BatchNorm-Linear, that op's backward leaves coefficients and a stride-0 zero gradient, and the pass that bins the
    points forms every point's gradient row dx = k0 + x k1 + dy Gi itself.  Same plane gradients as with the materialised
    matrix (the terms differ by the order of a 32-term fp32 sum; the plane sums themselves are exact): 2e-6 of the
    tensor's scale; also with a second consumer of the matrix; a layout outside the fused pass ("4": R = 4) materialises
    the matrix after all and agrees too."""
    from splatco_amd import scene_model as sm
    from splatco_amd.triplane import multi_triplane_sample
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(V + len(layout))
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    Rs = [int(t) for t in layout.split("-")]
    sizes = [(40, 36, 44), (24, 20, 28), (12, 16, 10)][:len(Rs)]
    ind = (torch.rand(V, 3, device=dev, generator=g) * 2.1 - 1.05)
    planes, grids, col = [], [], 0
    for R, (X, Y, Z) in zip(Rs, sizes):
        tri = [r(1, R, X, Y).requires_grad_(), r(1, R, X, Z).requires_grad_(), r(1, R, Y, Z).requires_grad_()]
        planes += tri
        grids.append((tri, (col, col + R, col + 2 * R)))
        col += 3 * R
    width = col
    G, c = (r(32, width) * 0.2).requires_grad_(), r(32).requires_grad_()
    w_y, w_x = r(V, 32), r(V, width)

    def run(defer):
        for t in planes + [G, c]:
            t.grad = None
        x = multi_triplane_sample([(ind, tuple(tri), cols) for tri, cols in grids])
        box = x._scr_deferred_dx
        assert box.width == width
        y, _, _ = sm._NormLinearFn.apply(x, G, c, 1e-5, None, box if defer else None)
        loss = (y * w_y).sum()
        if second_use:
            loss = loss + (x * w_x).sum()
        loss.backward()
        assert box.coef is None
        return [t.grad.clone() for t in planes] + [G.grad.clone(), c.grad.clone()]

    want, got = run(False), run(True)
    for k, (a, b) in enumerate(zip(want, got)):
        scale = float(a.abs().max())
        assert a.shape == b.shape and torch.isfinite(b).all()
        assert float((a - b).abs().max()) <= 2e-6 * scale, (k, float((a - b).abs().max()), scale)
    assert torch.equal(run(True)[0], got[0])        # bit-reproducible


@pytest.mark.gpu
@pytest.mark.parametrize("N", [40, 50_001, 1_400_003])      # one partial tile; 79 workgroups; more workgroups than statistics rows (second-level reduction)
def test_gather_produced_column_statistics_feed_the_batchnorm(N):
    """The anchor gather sums (x - x[0]) and (x - x[0])^2 per column of g_fea while its rows sit in LDS
    (csrc/anchor_gather.hip); the fused BatchNorm-Linear takes those partial sums instead of a statistics pass of its own
    (scr_norm_linear_forward: col_stats).  Same mean / variance / output as its own pass to fp32 summation order, and
    against float64; exp(scaling) columns (large mean, small spread) included."""
    from splatco_amd import scene_model as sm
    from splatco_amd.anchor_gather import gather_anchors
    from splatco_amd.scene_model import AnchorGaussianModel
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    pc = AnchorGaussianModel(plane_size=16, num_channels=15).to(dev)
    pc.set_anchors(r(N, 3) * 2, r(N, 10, 3), r(N, 32) * 3 + 0.5, r(N, 6) * 0.3 - 3)
    idx = (torch.rand(N, device=dev, generator=g) < 0.8).nonzero().squeeze(1)
    with torch.no_grad():
        *_, g_fea = gather_anchors(pc, idx)
    stats = g_fea._scr_col_stats
    V = idx.numel()
    from splatco_amd import _C
    assert stats.shape == (_C.lib.scr_anchor_gather_stat_rows(V), 2, 80) and stats.is_contiguous() and 1 <= stats.shape[0] <= 2048
    G, c = r(32, 71) * 0.2, r(32)
    y1, m1, v1 = sm._NormLinearFn.apply(g_fea, G, c, 1e-5, stats)
    y0, m0, v0 = sm._NormLinearFn.apply(g_fea, G, c, 1e-5)
    x64 = g_fea.double()
    m64, v64 = x64.mean(0), x64.var(0, unbiased=False)
    sd64 = v64.sqrt()
    for name, got_m, got_v in (("gather", m1, v1), ("own pass", m0, v0)):
        em, ev = float(((got_m.double() - m64).abs() / sd64).max()), float(((got_v.double() - v64).abs() / v64).max())
        print(f"[column statistics, N = {N}, {name}] mean off by {em:.1e} standard deviations at worst, variance by {ev:.1e} of itself")
        assert em <= 1e-5 and ev <= 2e-5, (name, em, ev)
    y64 = ((x64 - m64) * torch.rsqrt(v64 + 1e-5)) @ G.double().t() + c.double()
    for y in (y1, y0):
        assert float((y.double() - y64).abs().max()) <= 2e-5 * float(y64.abs().max())
    assert float((y1 - y0).abs().max()) <= 1e-5 * float(y0.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("V,d,ld", [(2, 60, 60), (15, 71, 71), (1000, 60, 64), (4099, 71, 71), (100003, 60, 60), (100003, 71, 71),
                                    (65536, 30, 30), (20000, 80, 80), (20000, 16, 99), (33333, 7, 7),
                                    (4_400_003, 60, 60)])      # more statistics slabs than the chip holds: the slabs grow
def test_fused_norm_linear_matches_batchnorm_linear_chain(V, d, ld):
    """csrc/normlinear.hip (column statistics, folded GEMM, the three backward passes) against BatchNorm1d (training
    mode) -> Linear evaluated by torch autograd in float64, and against the torch ops the CPU path uses.  Columns
    with a large mean / small spread (the log-scalings of the anchors: -5 +- 0.3) stress the variance.  Tolerance:
    fp32 summation order: max(2e-5, 1.5 x the torch ops' own error) of each column's scale for mean, var, dx and dG, of each
    row's for y and dx (floored at 1e-3 of the tensor's), of the tensor's for dc; every figure is printed first."""
    from splatco_amd import scene_model as sm
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(V * 131 + d)
    base = torch.randn(V, ld, device=dev, generator=g)
    base[:, : d // 2] = base[:, : d // 2] * 0.3 - 5.0
    x = base[:, :d].detach().requires_grad_()                          # a column block when ld > d
    G = (torch.randn(32, d, device=dev, generator=g) * 0.2).requires_grad_()
    c = torch.randn(32, device=dev, generator=g).requires_grad_()
    w = torch.randn(V, 32, device=dev, generator=g)
    eps = 1e-5

    def run(hip):
        sm.NORM_LINEAR_HIP = hip
        try:
            for t in (x, G, c):
                t.grad = None
            y, mean, var = sm._NormLinearFn.apply(x, G, c, eps)
            (y * w).sum().backward()
            return [t.detach().double().cpu() for t in (y, mean, var, x.grad, G.grad, c.grad)]
        finally:
            sm.NORM_LINEAR_HIP = True

    got, tor = run(True), run(False)
    x64, G64, c64 = (t.detach().double().cpu().requires_grad_() for t in (x, G, c))
    m64, v64 = x64.mean(0), x64.var(0, unbiased=False)
    y64 = ((x64 - m64) / torch.sqrt(v64 + eps)) @ G64.t() + c64
    (y64 * w.double().cpu()).sum().backward()
    ref = [y64.detach(), m64.detach(), v64.detach(), x64.grad, G64.grad, c64.grad]
    # per column (mean, var, dx, dG: the columns' scales differ by orders of magnitude -- inv is 3 for a log-scaling column
    # and 0.3 for a feature column) and per row (y, dx: a wrong last row must not hide behind the others): f64_refs.err takes
    # the ratio per row of what it is given, the row's scale floored at 1e-3 of the tensor's, and returns the largest
    import f64_refs as R
    views = {"y": [("rows", lambda m: m)], "mean": [("columns", lambda m: m)], "var": [("columns", lambda m: m)],
             "dx": [("rows", lambda m: m), ("columns", lambda m: m.t())], "dG": [("columns", lambda m: m.t())], "dc": [("tensor", None)]}
    failed = []
    for name, a, b, t in zip(("y", "mean", "var", "dx", "dG", "dc"), got, ref, tor):
        for how, view in views[name]:
            if view is None:
                err, err_t = R.err(a, b, scale_floor=1e-6), R.err(t, b, scale_floor=1e-6)
            else:
                err, err_t = R.err(view(a), view(b), rows=True, scale_floor=1e-6), R.err(view(t), view(b), rows=True, scale_floor=1e-6)
            # (the variance is the difference of two numbers and the folded form cancels 1 / sqrt(var) against it; there the
            #  bar is the error of the torch ops on the same formulation)
            bar = R.bar(err_t)
            print(f"norm_linear V={V} d={d} ld={ld} {name:4s} per {how:7s} fused {err:.3e}  torch ops {err_t:.3e}  bar {bar:.3e}"
                  f"{'' if err < bar else '   <-- FAIL'}")
            if not err < bar:
                failed.append((name, how, err, err_t))
    assert not failed, failed
    # bit-reproducible
    again = run(True)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.gpu
def test_sorted_anchors_render_the_same_image():
    """AnchorGaussianModel.sort_anchors (Morton order) is a pure relabelling: the rendered image and the loss are the
    same (the anchor order only breaks exact depth ties and changes the order of fp32 sums in weight gradients), the
    per-anchor gradients are the permuted ones."""
    import types
    from splatco_amd.renderer import prefilter_voxel, render
    from splatco_amd.synthetic import synthetic_anchor_model, synthetic_views
    dev = torch.device("cuda:0")
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    bg = torch.ones(3, device=dev)
    view = synthetic_views(1, 640, 360)[0].to(dev)

    def run(sort):
        pc = synthetic_anchor_model(60000, 7, dev, plane_size=256)
        perm = pc.sort_anchors() if sort else torch.arange(60000, device=dev)
        vis = prefilter_voxel(view, pc, pipe, bg)
        out = render(view, pc, pipe, bg, visible_mask=vis, retain_grad=True)
        out["render"].square().mean().backward()
        return out["render"].detach(), perm, {n: getattr(pc, n).grad for n in ("_anchor", "_offset", "_anchor_feat", "_scaling")}, \
            pc.feat_planes._feat.k0s[1].xy_plane.grad, int(vis.sum())

    img0, _, g0, gp0, n0 = run(False)
    img1, perm, g1, gp1, n1 = run(True)
    assert n0 == n1 and n0 > 10000
    # the features differ by fp32 summation order (BatchNorm statistics over differently ordered rows: 1e-7), so a splat
    # whose alpha sits at the 1/255 cut, or a pixel at the T < 1e-4 stop, can fall on the other side in a few pixels: those
    # differ by at most one splat's contribution (alpha 1/255), every other pixel by rounding only
    diff = (img0 - img1).abs()
    assert int((diff > 2e-5).sum()) <= 24 and float(diff.max()) < 1.5 / 255, (int((diff > 2e-5).sum()), float(diff.max()))
    # gradients: the same up to rounding, except for the handful of Gaussians that meet a pixel where such a cut fell the
    # other way (they change by that splat's share): at most 0.01 % of the elements beyond 2e-4 of the scale, none beyond 5 %
    def close(a, b, name):
        scale = float(a.abs().max())
        d = (a - b).abs()
        bad = int((d > 2e-4 * scale + 1e-12).sum())
        assert bad <= max(4, a.numel() // 10000) and float(d.max()) < 0.05 * scale, (name, bad, float(d.max()), scale)
    for n in g0:
        close(g0[n][perm], g1[n], n)
    close(gp0, gp1, "plane")


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 3, 4, 5, 7, 8])
def test_multi_grid_sampling_into_one_matrix_all_alignments(R):
    """multi_triplane_sample with the FeaturePlanes layout -- attention grid (six planes, columns interleaved), two plain
    grids of different sizes, all into one [V, 12 R] matrix -- against F.grid_sample per plane.  The widths 12 R put the
    grids' column blocks at every 16-byte phase (R = 5: 0 / 2 / 1 floats past a boundary), which drives the
    alignment-peeled row loads of the one-pass gradient scatter (R <= 5) and the split path for two planes with R > 5."""
    import torch.nn.functional as F
    from splatco_amd.triplane import multi_triplane_sample
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(R)
    V = 70_001
    ind = torch.rand(V, 3, device=dev, generator=g) * 2.3 - 1.15
    ind[:300] = torch.randint(0, 2, (300, 3), device=dev, generator=g).float() * 2 - 1
    mk = lambda n, X, Y, Z: [(torch.randn(1, R, a, b, device=dev, generator=g) * 0.5).requires_grad_()
                             for _ in range(n // 3) for a, b in ((X, Y), (X, Z), (Y, Z))]
    grids = [(mk(6, 40, 40, 40), tuple(c * R for c in (0, 2, 4, 1, 3, 5))),
             (mk(3, 40, 48, 56), tuple(6 * R + c * R for c in range(3))),
             (mk(3, 90, 70, 80), tuple(9 * R + c * R for c in range(3)))]
    out = multi_triplane_sample([(ind, tuple(pl), cols) for pl, cols in grids])
    assert out.shape == (V, 12 * R) and out.stride(0) % 4 == 0
    w = torch.randn(V, 12 * R, device=dev, generator=g)
    (out * w).sum().backward()
    got = [[p.grad.clone() for p in pl] for pl, _ in grids]
    pairs = ((1, 0), (2, 0), (2, 1))
    for (pl, cols), gg in zip(grids, got):
        for j, p in enumerate(pl):
            p.grad = None
            samp = F.grid_sample(p, ind[:, list(pairs[j % 3])].view(1, 1, V, 2), mode="bilinear", align_corners=True).flatten(0, 2).T
            assert torch.allclose(out[:, cols[j]:cols[j] + R], samp, rtol=1e-5, atol=1e-6), (R, j)
            (samp * w[:, cols[j]:cols[j] + R]).sum().backward()
            err, scale = float((gg[j] - p.grad).abs().max()), float(p.grad.abs().max())
            assert err <= 5e-5 * scale + 1e-7, (R, j, err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("n_views", [1, 2])
def test_arena_sink_gradients_equal_autograd_accumulation(n_views):
    """collaborative_step with a GradArena: the gather's backward kernel writes the per-anchor gradients straight into the
    arena (overwriting for the first view, adding for the second) -- same values as the step without an arena, where
    autograd accumulates them; a render() after the step goes through autograd again; the arena is not cleared for the
    parameters the kernel overwrites, so a stale step must not leak (two steps, second compared)."""
    import types
    from splatco_amd.multiview import GradArena
    from splatco_amd.renderer import prefilter_voxel, render
    from splatco_amd.synthetic import synthetic_anchor_model, synthetic_views
    from splatco_amd.train_step import collaborative_step
    dev = torch.device("cuda:0")
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    bg = torch.ones(3, device=dev)
    views = [v.to(dev) for v in synthetic_views(n_views, 640, 360)]
    g = torch.Generator(device=dev).manual_seed(5)
    gts = [torch.rand(3, 360, 640, device=dev, generator=g) for _ in views]
    names = ("_anchor_feat", "_anchor", "_offset", "_scaling")

    def run(use_arena):
        torch.manual_seed(11)
        pc = synthetic_anchor_model(50000, 9, dev, plane_size=256)
        params = [p for p in pc.parameters() if p.requires_grad]
        arena = GradArena(params) if use_arena else None
        for _ in range(2):                       # the second step sees what the first left in the buffers
            collaborative_step(pc, views, gts, pipe, bg, arena=arena)
        assert getattr(pc, "_grad_sink", None) is None
        grads = {n: getattr(pc, n).grad.detach().clone() for n in names}
        plane = pc.feat_planes._feat.k0s[1].xy_plane.grad.detach().clone()
        if use_arena:
            assert arena._sink is not None and all(getattr(pc, n).grad.data_ptr() == v.data_ptr()
                                                   for n, v in zip(names, arena._sink.tensors))
            # outside the step the same model goes through autograd as usual
            for p in params:
                p.grad = None
            vis = prefilter_voxel(views[0], pc, pipe, bg)
            render(views[0], pc, pipe, bg, visible_mask=vis)["render"].mean().backward()
            assert pc._anchor.grad is not None and pc._anchor.grad.data_ptr() != arena._sink.tensors[1].data_ptr()
        return grads, plane

    g0, p0 = run(False)
    g1, p1 = run(True)
    for n in names:
        scale = float(g0[n].abs().max())
        assert scale > 0 and float((g0[n] - g1[n]).abs().max()) <= 1e-6 * scale, n
    assert float((p0 - p1).abs().max()) <= 1e-5 * float(p0.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [(10, 5, 5), (10, 5), (10,), (5, 5, 5), (5,)])
def test_all_grids_backward_in_one_pass(layout):
    """scr_triplane_backward_multi: grids sampled at the same coordinates (one tensor) get their plane gradients from ONE
    pass over the points.  Checked against the grid-by-grid path (same kernels downstream) and
    against F.grid_sample; V above and below the row-pair threshold of the forward, and a flat scene whose crowded tiles are
    split over several workgroups."""
    import torch.nn.functional as F
    from splatco_amd import triplane as tp
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(sum(layout))
    for V in (50_000, 300_001, 300_002):
        ind = torch.rand(V, 3, device=dev, generator=g) * 2.3 - 1.15
        if V == 300_002:
            ind[:, 2] *= 0.02          # a sheet: the xz / yz projections crowd into one row of tiles, which are split (csrc/triplane.hip)
        sizes = [(40, 48, 56), (40, 48, 56), (90, 70, 80)]
        grids, col = [], 0
        for gi, r in enumerate(layout):
            X, Y, Z = sizes[gi]
            planes = [(torch.randn(1, r, a, b, device=dev, generator=g) * 0.5).requires_grad_() for a, b in ((X, Y), (X, Z), (Y, Z))]
            grids.append((planes, tuple(col + r * j for j in range(3))))
            col += 3 * r
        w = torch.randn(V, col, device=dev, generator=g)

        def run(fuse):
            tp.FUSE_GRIDS = fuse
            try:
                for pl, _ in grids:
                    for p in pl:
                        p.grad = None
                out = tp.multi_triplane_sample([(ind, tuple(pl), cols) for pl, cols in grids])
                (out * w).sum().backward()
                return out.detach(), [p.grad.clone() for pl, _ in grids for p in pl]
            finally:
                tp.FUSE_GRIDS = True

        out1, g1 = run(True)
        out0, g0 = run(False)
        assert torch.equal(out1, out0)
        pairs = ((1, 0), (2, 0), (2, 1))
        k = 0
        for pl, cols in grids:
            for j, p in enumerate(pl):
                scale = float(g0[k].abs().max())
                # (exact cell sums on both paths, but on a fixed-point grid set by the largest gradient among the channels a
                # record carries -- the fused pass may stack grids of one size into one record: equal to rounding, not bit for bit)
                assert float((g1[k] - g0[k]).abs().max()) <= 2e-6 * scale, (layout, V, k)
                p.grad = None
                samp = F.grid_sample(p, ind[:, list(pairs[j])].view(1, 1, V, 2), mode="bilinear", align_corners=True).flatten(0, 2).T
                (samp * w[:, cols[j]:cols[j] + p.shape[1]]).sum().backward()
                assert float((g1[k] - p.grad).abs().max()) <= 5e-5 * float(p.grad.abs().max()) + 1e-7, (layout, V, k)
                k += 1


@pytest.mark.gpu
@pytest.mark.parametrize("R,n_planes", [(1, 3), (2, 6)])
def test_plane_backward_one_projection_per_pass(R, n_planes):
    """csrc/triplane.hip tp_backward: a grid whose three projections together have more tiles than one workgroup's LDS
    histogram holds (TP_HIST_MAX_TILES = 16384) is bucketed one projection per pass.  2368^3 is the smallest cube over the
    limit (3 x 74 x 74 = 16428 tiles) whose planes each stay under it.  Plain planes, and plain + attended planes (two
    gradient blocks per projection); against F.grid_sample's backward, and bit for bit against a second run."""
    import torch.nn.functional as F
    from splatco_amd import triplane as tp
    dev = torch.device("cuda:0")
    # tied to csrc/triplane.hip: TP_HIST_MAX_TILES = 16384 tiles per pass, SCR_TP_TILE = 32 cells per tile edge.  With other
    # values this shape may no longer reach the branch (nothing here can tell which branch ran): move S with them.
    S, V = 2368, 20_000
    assert 3 * ((S + 31) // 32) ** 2 > 16384 >= ((S + 31) // 32) ** 2
    g = torch.Generator(device=dev).manual_seed(2368 + n_planes)
    ind = torch.rand(V, 3, device=dev, generator=g) * 2.2 - 1.1
    at = torch.randperm(V, device=dev, generator=g)[:300]
    ind[at] = torch.randint(0, 2, (300, 3), device=dev, generator=g).float() * 2.0 - 1.0      # exact corners of the planes
    planes = [(torch.randn(1, R, S, S, device=dev, generator=g) * 0.5).requires_grad_() for _ in range(n_planes)]
    w = torch.randn(V, n_planes * R, device=dev, generator=g)

    def run():
        for p in planes:
            p.grad = None
        (tp.triplane_sample(ind, planes) * w).sum().backward()
        return [p.grad for p in planes]

    got = run()
    assert all(torch.equal(a, b) for a, b in zip(got, run()))
    pairs = ((1, 0), (2, 0), (2, 1))
    for j, p in enumerate(planes):
        p.grad = None
        samp = F.grid_sample(p, ind[:, list(pairs[j % 3])].view(1, 1, V, 2), mode="bilinear", align_corners=True).flatten(0, 2).T
        (samp * w[:, j * R:(j + 1) * R]).sum().backward()
        scale = float(p.grad.abs().max())
        err = float((got[j] - p.grad).abs().max())
        print(f"plane {j}: max |ref| {scale:.4g}, max error {err:.3g}")
        assert scale > 0 and err <= 5e-5 * scale + 1e-7, (j, err, scale)
        p.grad = None


@pytest.mark.gpu
@pytest.mark.parametrize("R,H,W", [(5, 70, 70), (2, 37, 91), (5, 200, 131)])
def test_fused_plane_attention_matches_the_torch_module(R, H, W):
    """csrc/attention.hip against the torch TriPlaneAttention + chunk + cat chain it replaces (scene/grids.py:22-64,
    166-181): pair planes, and the gradients of the planes, the shared MLP and the 7x7 window."""
    import copy
    from splatco_amd import plane_attention
    from splatco_amd.scene_model import TriPlaneAttention
    torch.manual_seed(R * 1000 + H)
    dev = torch.device("cuda:0")
    ta = TriPlaneAttention(3 * R).to(dev)
    ta_ref = copy.deepcopy(ta)
    planes = [(torch.randn(1, R, H, W, device=dev) * 0.5).requires_grad_(True) for _ in range(3)]
    ref_planes = [p.detach().clone().requires_grad_(True) for p in planes]
    assert plane_attention.fused_ok(*planes, ta)
    out = plane_attention.attended_pair_planes(*planes, ta)
    tri = ta_ref(torch.cat(ref_planes, dim=1))
    ref = [torch.cat((p, a), dim=1) for p, a in zip(ref_planes, torch.chunk(tri, 3, dim=1))]
    for o, r in zip(out, ref):
        assert o.shape == r.shape
        assert torch.allclose(o, r, rtol=1e-5, atol=1e-6), float((o - r).abs().max())
    g = [torch.randn_like(o) for o in out]
    sum((o * gi).sum() for o, gi in zip(out, g)).backward()
    sum((r * gi).sum() for r, gi in zip(ref, g)).backward()

    def rel(a, b):
        return float((a - b).norm() / b.norm().clamp_min(1e-20))
    for p, q in zip(planes, ref_planes):
        assert rel(p.grad, q.grad) < 1e-4, rel(p.grad, q.grad)
    for (n, a), (_, b) in zip(ta.named_parameters(), ta_ref.named_parameters()):
        assert rel(a.grad, b.grad) < 2e-4, (n, rel(a.grad, b.grad))
    # deterministic: a second backward gives the same bits
    grads1 = [p.grad.clone() for p in planes] + [a.grad.clone() for a in ta.parameters()]
    for t in planes + list(ta.parameters()):
        t.grad = None
    out = plane_attention.attended_pair_planes(*planes, ta)
    sum((o * gi).sum() for o, gi in zip(out, g)).backward()
    for a, b in zip(grads1, [p.grad for p in planes] + [a.grad for a in ta.parameters()]):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 300_001])
def test_mask_indices_equal_nonzero(n):
    """csrc/expand.hip mask_count / mask_index kernels against torch.nonzero (the `t[visible_mask]` index of
    gaussian_renderer/__init__.py:23-29): same ascending int64 indices, for empty, full and ragged masks."""
    from splatco_amd.expand import mask_indices
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(n)
    for p in (0.0, 0.37, 1.0):
        mask = (torch.rand(n, generator=g) < p).to(dev)
        idx = mask_indices(mask)
        ref = mask.nonzero(as_tuple=False).squeeze(1)
        assert idx.dtype == torch.int64 and idx.shape == ref.shape
        assert torch.equal(idx, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 2049, 300_000])
def test_scaling_regulariser_matches_torch_prod(P):
    """csrc/ssim.hip scaling_reg_* against scaling.prod(dim=1).mean() (train.py:192-196), value and gradient, incl. rows
    with zeros (where torch's backward takes its special path)."""
    from splatco_amd.losses import scaling_reg
    dev = torch.device("cuda:0")
    torch.manual_seed(P)
    s = (torch.rand(P, 3, device=dev) * 0.2)
    if P > 10:
        s[3, 1] = 0.0
        s[7] = 0.0
    a, b = s.clone().requires_grad_(True), s.clone().requires_grad_(True)
    la, lb = scaling_reg(a), b.prod(dim=1).mean()
    assert torch.allclose(la, lb, rtol=1e-5, atol=1e-9)
    (la * 3.0).backward()
    (lb * 3.0).backward()
    assert torch.allclose(a.grad, b.grad, rtol=1e-5, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 1, 1), (3, 37, 53), (3, 1080, 1920)])
def test_fused_pair_l1_matches_the_reference_ops(shape):
    """csrc/ssim.hip pair_l1_* against l1_loss(real1 - real2, gen1 - gen2) (train.py:213): value to 2 ulp of the fp32
    mean, gradients equal to 2 ulp (same sign pattern, sign(0) = 0 in both; 1/n may be rounded once more or less), to gen1 only / gen2 only / both;
    the sum is taken in double so the value does not depend on the launch shape."""
    from splatco_amd.losses import l1_loss, pair_l1
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(shape[1])
    r1, r2, a0, b0 = (torch.rand(*shape, device=dev, generator=g) for _ in range(4))
    b0[..., :1] = a0[..., :1] - (r1[..., :1] - r2[..., :1])                  # residuals at / next to zero
    for need in ((True, True), (True, False), (False, True)):
        outs = []
        for fused in (True, False):
            a, b = a0.clone().requires_grad_(need[0]), b0.clone().requires_grad_(need[1])
            loss = pair_l1(a, b, r1, r2) if fused else l1_loss(r1 - r2, a - b)
            (loss * 0.37).backward()
            outs.append((loss.detach(), a.grad, b.grad))
        (lf, af, bf), (lt, at, bt) = outs
        exact = ((r1 - r2) - (a0 - b0)).abs().double().mean()
        assert abs(lf.double() - exact) <= 2.0 ** -23 * exact + 1e-12, (lf.item(), exact.item())
        assert abs(lf.double() - exact) <= abs(lt.double() - exact) + 2.0 ** -24 * exact + 1e-12
        for x, y, n in ((af, at, need[0]), (bf, bt, need[1])):
            assert (x is None) == (not n) and (y is None) == (not n)
            if n:
                assert torch.equal(x.sign(), y.sign()) and torch.allclose(x, y, rtol=2.0 ** -22, atol=0)
    assert pair_l1(a0, b0, r1, r2).item() == pair_l1(a0.clone(), b0.clone(), r1.clone(), r2.clone()).item()


@pytest.mark.gpu
def test_scaling_regulariser_through_the_expansion_tap():
    """losses.scaling_reg on the `scaling` output of expand_compact sends its gradient through the expansion's tap
    (csrc/expand.hip adds it to dL/dscaling while reading it): every input gradient equals what the torch chain
    `scaling.prod(1).mean()` + a second use of `scaling` gives; also twice (two taps' worth), alone (no other use of
    scaling), and not at all (tap unused)."""
    from splatco_amd.expand import expand_compact
    from splatco_amd.losses import scaling_reg
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(11)
    V, k = 20_011, 10
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    base = (r(V * k, 1), r(V * k, 3), r(V * k, 7), r(V, k, 3), torch.rand(V, 6, device=dev, generator=g) + 0.1, r(V, 3))
    w_s = None
    for uses, other in ((1, True), (2, True), (1, False), (0, True)):
        grads = []
        for tapped in (True, False):
            ins = [t.clone().requires_grad_(True) for t in base]
            xyz, color, opacity, scaling, rot, mask = expand_compact(*ins, k)
            assert hasattr(scaling, "_scr_reg_tap")
            if w_s is None:
                w_s = r(*scaling.shape)
            loss = (xyz * 0.3).sum() + (rot * 0.1).sum() + (opacity * 0.2).sum() + (color * 0.05).sum()
            if other:
                loss = loss + (scaling * w_s).sum()            # the rasterizer's dL/dscales stands in here
            for _ in range(uses):
                reg = scaling_reg(scaling) if tapped else scaling.prod(dim=1).mean()
                loss = loss + 700.0 * reg
            loss.backward()
            grads.append([t.grad.clone() for t in ins])
        for a, b, name in zip(*grads, ("neural_opacity", "color", "scale_rot", "offsets", "grid_scaling", "anchor")):
            num, den = (a - b).norm().item(), max(b.norm().item(), 1e-20)
            assert num / den < 2e-6, (uses, other, name, num / den)
        if uses and not other:
            assert grads[0][2][:, :3].abs().max() > 0          # the regulariser alone reaches the scale columns


@pytest.mark.gpu
@pytest.mark.parametrize("training", [True, False])
def test_appearance_embedding_path_on_the_gpu(training):
    """The reference's code default appearance_dim = 32 (arguments/__init__.py:76) on the device: fused anchor gather,
    HIP tri-plane / BatchNorm-Linear / expansion kernels, the three heads as GEMMs (the colour head's input carries the
    camera's code, gaussian_renderer/__init__.py:55-58,76-80) -- against the fixture captured from the reference, then a
    render() whose backward reaches the embedding row of that camera only."""
    from test_host_golden import _appearance_model
    from splatco_amd.renderer import generate_neural_gaussians, prefilter_voxel, render
    dev = torch.device("cuda:0")
    pc, d = _appearance_model(dict(np.load(os.path.join(GOLD, "neural_gaussians_app.npz"))))
    pc = pc.to(dev)
    pc.train(training)
    cam = types.SimpleNamespace(camera_center=torch.tensor(d["camera_center"], device=dev), uid=int(d["uid"]))
    with torch.no_grad():
        res = generate_neural_gaussians(cam, pc, torch.tensor(d["visible_mask"], device=dev), is_training=training)
    names = ["xyz", "color", "opacity", "scaling", "rot", "neural_opacity", "mask"][:len(res)]
    tag = "train" if training else "eval"
    for n, v in zip(names, res):
        want = d[f"{tag}.{n}"]
        assert tuple(v.shape) == want.shape, n
        if v.dtype == torch.bool:
            np.testing.assert_array_equal(v.cpu().numpy(), want)
        else:
            np.testing.assert_allclose(v.cpu().numpy(), want, rtol=1e-4, atol=1e-5, err_msg=n)
    if training:
        view = look_at_camera(eye=(0.3, -0.2, -4.5), target=(0, 0, 0), up=(0, -1, 0), FoVx=math.radians(60), width=200,
                              height=120, uid=int(d["uid"])).to(dev)
        pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
        bg = torch.ones(3, device=dev)
        vis = prefilter_voxel(view, pc, pipe, bg)
        out = render(view, pc, pipe, bg, visible_mask=vis, retain_grad=True)
        out["render"].square().mean().backward()
        g = pc.embedding_appearance.embedding.weight.grad
        assert g is not None and g[int(d["uid"])].abs().sum() > 0
        assert all(float(g[i].abs().sum()) == 0.0 for i in range(g.shape[0]) if i != int(d["uid"]))
        assert pc._anchor_feat.grad is not None and pc._anchor_feat.grad.abs().sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [False, True])
def test_norm_fold_kernels_match_the_framework_chain(shared):
    """scene_model._norm_linear on the device: the fold of L (BatchNorm, Linear) pairs into (G, c), its backward and the
    running-statistics update run as single launches (csrc/normlinear.hip nl_fold_* / nl_running_stats_kernel).  Checked
    against nn.BatchNorm1d -> Linear module by module in float64 (scene/gaussian_model.py:149-169): output, every
    parameter gradient, input gradient, running_mean / running_var / num_batches_tracked."""
    from splatco_amd import scene_model as sm
    dev = torch.device("cuda:0")
    torch.manual_seed(3 + shared)
    widths = (71, 71, 71) if shared else (30, 15, 15)
    V, d = 20011, (71 if shared else 60)
    bns = [torch.nn.BatchNorm1d(w).to(dev) for w in widths]
    lins = [sm.TallLinear(w, 32).to(dev) for w in widths]
    with torch.no_grad():
        for bn in bns:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.3)
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.5, 2.0)
    x = (torch.randn(V, d, device=dev) * 0.7 + 0.3).requires_grad_()
    w = torch.randn(V, 32, device=dev)
    ref_b = [torch.nn.BatchNorm1d(wd).double() for wd in widths]
    ref_l = [torch.nn.Linear(wd, 32).double() for wd in widths]
    for a, b in zip(bns + lins, ref_b + ref_l):
        b.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu() for k, v in a.state_dict().items()})
    y = sm._norm_linear(x, bns, lins)
    (y * w).sum().backward()
    x64 = x.detach().cpu().double().requires_grad_()
    off, y64 = 0, 0
    for bn, lin, wd in zip(ref_b, ref_l, widths):
        y64 = y64 + lin(bn(x64 if shared else x64[:, off:off + wd]))
        off += 0 if shared else wd
    (y64 * w.cpu().double()).sum().backward()

    def close(a, b, tol, name):
        scale = max(float(b.abs().max()), 1e-6)
        err = float((a.detach().cpu().double() - b).abs().max()) / scale
        assert err <= tol, (name, err)

    close(y, y64.detach(), 2e-5, "y")
    close(x.grad, x64.grad, 5e-5, "dx")
    for i, (bn, lin, rb, rl) in enumerate(zip(bns, lins, ref_b, ref_l)):
        close(lin.weight.grad, rl.weight.grad, 5e-5, f"dW{i}")
        close(lin.bias.grad, rl.bias.grad, 5e-5, f"db{i}")
        close(bn.weight.grad, rb.weight.grad, 5e-5, f"dgamma{i}")
        close(bn.bias.grad, rb.bias.grad, 5e-5, f"dbeta{i}")
        close(bn.running_mean, rb.running_mean, 1e-5, f"running_mean{i}")
        close(bn.running_var, rb.running_var, 1e-5, f"running_var{i}")
        assert int(bn.num_batches_tracked) == int(rb.num_batches_tracked) == 1


@pytest.mark.gpu
def test_box_coords_and_inverse_index_equal_the_framework_ops():
    """Two small fusions of the anchor path: PlaneGrid.box_coords == the reference's four elementwise passes
    (scene/grids.py:146) BIT FOR BIT (same IEEE operations, same order), and mask_indices' inverse map == the
    fill + arange + index_put the gather's backward used to build."""
    from splatco_amd.expand import mask_indices
    from splatco_amd.scene_model import PlaneGrid
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    pg = PlaneGrid(15, [24, 24, 24], [-2.0, -1.5, -2.5], [2.0, 2.25, 1.75]).to(dev)
    for V in (1, 7, 100_003):
        xyz = torch.randn(V, 3, device=dev, generator=g) * 3
        want = (xyz - pg.xyz_min) / (pg.xyz_max - pg.xyz_min) * 2 - 1
        assert torch.equal(pg.box_coords(xyz), want)
    for n in (1, 63, 64, 4097, 1_000_003):
        m = torch.rand(n, device=dev, generator=g) < 0.4
        idx = mask_indices(m)
        assert torch.equal(idx, m.nonzero().squeeze(1))
        inv = torch.full((n,), -1, dtype=torch.long, device=dev)
        inv[idx] = torch.arange(idx.numel(), device=dev)
        assert torch.equal(idx._scr_inverse, inv)
    empty = mask_indices(torch.zeros(100, dtype=torch.bool, device=dev))
    assert empty.numel() == 0 and torch.all(empty._scr_inverse == -1)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2])
def test_stacked_level0_grids_equal_separate_sampling(level):
    """FeaturePlanes samples the attention grid and the same-size plain grid of level 0 as ONE stacked 15-channel grid
    (scene_model.STACK_LEVEL0): features interleaved by projection, the BatchNorm-Linear fold told where each reference
    column sits.  Against the separate-grid path: output, running statistics and every parameter gradient (the planes',
    the attention module's, the BatchNorms', the Linears')."""
    from splatco_amd import scene_model as sm
    dev = torch.device("cuda:0")
    res = {}
    for stack in (False, True):
        torch.manual_seed(5)
        fp = sm.FeaturePlanes([96, 96, 96], torch.tensor([-2.0, -2.0, -2.0]), torch.tensor([2.0, 2.0, 2.0]), feat_dim=15).to(dev)
        fp.activate_level = level
        with torch.no_grad():
            for p in fp.parameters():
                p.add_(0.2 * torch.randn_like(p))
        g = torch.Generator(device=dev).manual_seed(9)
        x = torch.rand(300_007, 3, device=dev, generator=g) * 4.4 - 2.2
        g_fea = torch.randn(300_007, 72, device=dev, generator=g)[:, :71]
        w = torch.randn(300_007, 64, device=dev, generator=g)
        sm.STACK_LEVEL0 = stack
        try:
            y = fp(x, g_fea, 0)
        finally:
            sm.STACK_LEVEL0 = False
        (y * w).sum().backward()
        res[stack] = (y.detach(), {n: p.grad.clone() for n, p in fp.named_parameters() if p.grad is not None},
                      {n: b.clone() for n, b in fp.named_buffers()})
    (y0, g0, b0), (y1, g1, b1) = res[False], res[True]
    assert torch.allclose(y0, y1, rtol=1e-4, atol=1e-5), float((y0 - y1).abs().max())
    assert set(g0) == set(g1) and len(g0) > 15
    for n in g0:
        num, den = float((g0[n] - g1[n]).norm()), max(float(g0[n].norm()), 1e-20)
        assert num / den < 2e-4, (n, num / den)
    for n in b0:
        if b0[n].is_floating_point():
            assert torch.allclose(b0[n], b1[n], rtol=1e-5, atol=1e-6), n
        else:
            assert torch.equal(b0[n], b1[n]), n


@pytest.mark.gpu
def test_tv_term_on_the_gpu_matches_the_reference_fixture():
    """csrc/tv.hip against what the reference's PlaneGrid.total_variation_add_grad / GaussianLearner.tv_loss left in the
    planes' .grad (tests/golden/tv.npz; scene/grids.py:240-250, scene/gaussian_model.py:217-220): rel-L2 <= 1e-6 per
    plane, into empty and into existing gradients, scalar (odd row length) and float4 path, bit-reproducible."""
    from util import rel_l2
    from splatco_amd.scene_model import GaussianLearner, PlaneGrid
    dev = torch.device("cuda:0")
    G = np.load(os.path.join(GOLD, "tv.npz"))
    names = ("xy_plane", "xz_plane", "yz_plane")
    for tag, ws, ta in (("cube_plain", [24, 24, 24], False), ("cube_ta", [24, 24, 24], True),
                        ("odd_plain", [37, 19, 30], False), ("odd_ta", [37, 19, 30], True)):
        w = float(G[f"{tag}.w"])
        pg = PlaneGrid(15, ws, [-2.0] * 3, [2.0] * 3, TAflag=ta).to(dev)
        with torch.no_grad():
            for n in names:
                getattr(pg, n).copy_(torch.tensor(G[f"{tag}.{n}"]))
        pg.total_variation_add_grad(w)
        first = {n: getattr(pg, n).grad.clone() for n in names}
        for n in names:
            assert rel_l2(first[n].cpu().numpy(), G[f"{tag}.{n}.grad"]) <= 1e-6, (tag, n)
        if ta:
            assert all(p.grad is None for p in pg.TA.parameters())      # the attention module takes no part
        for n in names:
            getattr(pg, n).grad = torch.tensor(G[f"{tag}.{n}.prior"], device=dev)
        pg.total_variation_add_grad(w)
        for n in names:
            assert rel_l2(getattr(pg, n).grad.cpu().numpy(), G[f"{tag}.{n}.grad_acc"]) <= 1e-6, (tag, n, "accumulate")
        for n in names:
            getattr(pg, n).grad = None
        pg.total_variation_add_grad(w)
        assert all(torch.equal(getattr(pg, n).grad, first[n]) for n in names)
    for level in (0, 2):
        gl = GaussianLearner(40, 15).to(dev)
        gl._feat.activate_level = level
        with torch.no_grad():
            for gi, grid in enumerate(gl._feat.k0s):
                for n in names:
                    getattr(grid, n).copy_(torch.tensor(G[f"learner.k0s.{gi}.{n}"]))
        gl.tv_loss(4e-7)
        for gi, grid in enumerate(gl._feat.k0s):
            for n in names:
                want, got = G[f"learner.level{level}.k0s.{gi}.{n}.grad"], getattr(grid, n).grad
                if want.size == 0:
                    assert got is None, (level, gi, n)
                else:
                    assert rel_l2(got.cpu().numpy(), want) <= 1e-6, (level, gi, n)


@pytest.mark.gpu
@pytest.mark.parametrize("R,A,B", [(5, 700, 700), (5, 1400, 1400), (3, 33, 2051), (1, 1, 9), (2, 7, 1), (4, 65, 260)])
def test_tv_term_at_plane_sizes_equals_autograd(R, A, B):
    """The reference's formulation (six smooth-L1 sums -> autograd) run by torch on the GPU against csrc/tv.hip at the plane
    sizes of plane_size = 2800 (700^2 and 1400^2 are the grids tv_loss touches), at strip / tile remainders and at
    degenerate planes; the gradient must also be the exact negative under p -> -p (odd symmetry of the closed form)."""
    import torch.nn.functional as F
    from splatco_amd.tv import tv_add_grad
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(R * 1000 + A + B)
    p = torch.nn.Parameter((torch.randn(1, R, A, B, generator=g) * 0.8).to(dev))
    w = 4e-7
    loss = 0
    if A > 1:
        loss = loss + w * F.smooth_l1_loss(p[:, :, 1:], p[:, :, :-1], reduction="sum")
    if B > 1:
        loss = loss + w * F.smooth_l1_loss(p[:, :, :, 1:], p[:, :, :, :-1], reduction="sum")
    want = torch.autograd.grad(loss / 6, p)[0] if (A > 1 or B > 1) else torch.zeros_like(p)
    prior = (torch.randn(1, R, A, B, generator=g) * 1e-8).to(dev)
    p.grad = prior.clone()
    tv_add_grad([(p, w)])
    got = p.grad - prior
    err = (got - want).norm() / want.norm().clamp_min(1e-30)
    assert float(err) <= 1e-6 if float(want.norm()) > 0 else float(got.abs().max()) == 0.0, float(err)
    q = torch.nn.Parameter(-p.detach())
    tv_add_grad([(q, w)])
    p.grad = None
    tv_add_grad([(p, w)])
    assert torch.equal(q.grad, -p.grad)
    # argument validation: same buffer for plane and gradient, non-contiguous planes
    q.grad = q.data
    with pytest.raises(RuntimeError, match="distinct"):
        tv_add_grad([(q, w)])
