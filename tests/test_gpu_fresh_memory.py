"""No operator's result may depend on what its uninitialised buffers held (tests/poison.py).

Every scratch, saved-state and output buffer of splatco_amd/*.py is a `torch.empty` / `empty_like` / `_C.scratch`.  Each case
here runs one operator family forward AND backward through poison.check: unpatched, then with every such buffer pre-filled
with zero bytes, with int64 ones, and with 0xFF bytes (NaN / -1), in that order, stopping at the first pattern whose outputs
or gradients are not bit-identical to the zero-filled run.  Shapes are the smallest that still have a partial workgroup or
tile, an empty selection, and rows or nodes that nothing writes (those must come back exactly 0).  Every case asserts that
the helper really filled something and that all results are finite.  No case found a dependence: the library writes every
word it reads or returns.

The second half is parity at the same small shapes for the two families no other test takes this low: tri-plane sampling
(float64 F.grid_sample per plane, the bars of test_multi_grid_sampling_into_one_matrix_all_alignments) and the densification
statistics (training_statis_torch, the bar of test_training_statis_kernel_golden_and_random).

Every case prints its filled allocation / byte counts (and appends them to the file $SPLATCO_FRESH_MEMORY_LOG names, if
set); profiles/r15_fresh_memory.txt holds one such run.
"""
import math
import os
import types

import numpy as np
import pytest
import torch

import poison
from util import small_scene
from splatco_amd.synthetic import synthetic_camera, synthetic_gaussians

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _log(line):
    print(line)
    path = os.environ.get("SPLATCO_FRESH_MEMORY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _check(family, case, fn):
    """The ladder, with the counts reported; returns the outputs of the zero-filled run."""
    rep = poison.check(fn, sync=torch.cuda.synchronize)
    for pattern in poison.PATTERNS:
        assert rep[pattern].bytes > 0 and rep[pattern].count > 0, (family, case, pattern)
    _log(f"fresh_memory {family:14s} {case:58s} filled {rep['nan'].count:4d} buffers, {rep['nan'].bytes:10d} bytes per run")
    return rep["outputs"]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------ rasterizer
def _settings(cam, bg, sh_degree=1, camera_grad=False):
    from splatco_amd.rasterizer import GaussianRasterizationSettings
    view, proj, pos = (t.to(DEV).clone().requires_grad_(camera_grad) for t in
                       (cam.world_view_transform, cam.full_proj_transform, cam.camera_center))
    return GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=torch.tensor(bg, dtype=torch.float32, device=DEV), scale_modifier=1.0,
        viewmatrix=view, projmatrix=proj, sh_degree=sh_degree, campos=pos, prefiltered=False, debug=False)


def _scene(name):
    rng = np.random.default_rng(3)
    if name == "small":
        return small_scene(P=400, W=96, H=64)
    if name == "wide":            # the same camera on a cloud four times as wide: part of it behind the camera or outside the frustum
        return small_scene(P=400, W=96, H=64, spread=4.0)
    if name == "ragged":
        return synthetic_camera(130, 70), synthetic_gaussians(1500, 130, 70, 4)
    if name == "culled":          # two Gaussians, both culled (behind the camera / inside the near plane): no tile instance at all
        f = np.float32
        g = dict(means3D=np.array([[0.0, 0.0, -5.0], [0.0, 0.0, 0.1]], f), opacities=np.full((2, 1), 0.5, f),
                 colors=np.ones((2, 3), f), scales=np.full((2, 3), 0.1, f), rotations=np.array([[1.0, 0, 0, 0]] * 2, f),
                 bg=np.array([0.3, 0.4, 0.5], f))
        return synthetic_camera(64, 48), g
    if name == "one":             # P = 1, in front of the camera
        f = np.float32
        g = dict(means3D=np.array([[0.1, -0.05, 3.0]], f), opacities=np.full((1, 1), 0.7, f), colors=np.array([[0.2, 0.9, 0.4]], f),
                 scales=np.array([[0.3, 0.15, 0.2]], f), rotations=np.array([[0.9, 0.1, -0.3, 0.2]], f), bg=np.array([0.3, 0.4, 0.5], f))
        return synthetic_camera(64, 48), g
    assert name == "large_rects"  # the scene of test_gpu_parity.py: rects of hundreds of tiles, far records are cleared in the backward
    cam, g = synthetic_camera(320, 200), synthetic_gaussians(1200, 320, 200, 6)
    big = rng.choice(1200, 300, replace=False)
    g["scales"][big] *= rng.uniform(8, 40, (300, 1)).astype(np.float32) * np.array([[1.0, 0.5, 0.7]], np.float32)
    g["opacities"][big] = rng.uniform(0.01, 0.3, (300, 1)).astype(np.float32)
    return cam, g


RASTER_CASES = [("small", "colors"), ("small", "sh3"), ("small", "cov"), ("small", "aux"), ("small", "antialiased"), ("small", "camera"),
                ("small", "aux+antialiased+camera"), ("wide", "colors"), ("wide", "sh3"), ("wide", "cov"), ("wide", "aux+antialiased+camera"),
                ("ragged", "colors"), ("ragged", "deep"), ("ragged", "aux+antialiased"),
                ("ragged", "sh3+camera"), ("culled", "colors"), ("culled", "aux+camera"), ("one", "colors"), ("one", "aux+camera"),
                ("one", "cov+antialiased"), ("large_rects", "colors"), ("large_rects", "aux")]


@pytest.mark.parametrize("scene,variant", RASTER_CASES)
def test_rasterizer(scene, variant):
    """GaussianRasterizer forward + backward, visible_filter and markVisible.  fn renders twice: once with no plan of this
    resolution remembered (plan, then a binning buffer of the exact size) and once more (the speculative one-call path, whose
    buffer is larger than the instances need); the backward runs on the second.  Culled Gaussians: exactly 0 in every row."""
    from splatco_amd import _C
    from splatco_amd import rasterizer as R
    cam, g = _scene(scene)
    opts = set(variant.split("+"))
    P, H, W = g["means3D"].shape[0], cam.image_height, cam.image_width
    rng = np.random.default_rng(11)
    aux, aa, camera = "aux" in opts, "antialiased" in opts, "camera" in opts
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=DEV)
    shs = t(rng.standard_normal((P, 16, 3)) * 0.4) if "sh3" in opts else None
    cov = None
    if "cov" in opts:
        A = rng.standard_normal((P, 3, 3)) * 0.15
        S = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
        cov = t(np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1))
    dL, dLd, dLa = t(rng.standard_normal((3, H, W))), t(rng.standard_normal((H, W))), t(rng.standard_normal((H, W)))
    base = dict(means3D=t(g["means3D"]), opacities=t(g["opacities"]))
    base.update(dict(shs=shs) if shs is not None else dict(colors_precomp=t(g["colors"])))
    base.update(dict(cov3D_precomp=cov) if cov is not None else dict(scales=t(g["scales"]), rotations=t(g["rotations"])))
    if scene == "large_rects":
        cs = R._CSettings(_settings(cam, g["bg"]))
        _, _, st = R.rasterize_forward(cs, base["means3D"], base["opacities"], base["scales"], base["rotations"], None, None, base["colors_precomp"])
        assert st.flags & _C.PLAN_LARGE_RECTS

    def fn():
        rs = _settings(cam, g["bg"], sh_degree=3 if shs is not None else 1, camera_grad=camera)
        rast = R.GaussianRasterizer(rs)
        ins = {k: v.clone().requires_grad_() for k, v in base.items()}
        m2d = torch.zeros(P, 3, device=DEV, requires_grad=True)
        R._plan_guess.clear()
        with torch.no_grad():
            first = rast(means2D=m2d, antialiased=aa, return_aux=aux, **ins)
        out = rast(means2D=m2d, antialiased=aa, return_aux=aux, **ins)
        loss = (out[0] * dL).sum()
        if aux:
            loss = loss + (out[2] * dLd).sum() + (out[3] * dLa).sum()
        loss.backward()
        geo = {k: v for k, v in ins.items() if k in ("scales", "rotations", "cov3D_precomp")}
        res = list(first) + list(out) + [rast.visible_filter(ins["means3D"], **geo), rast.markVisible(ins["means3D"])]
        res += [ins[k].grad for k in sorted(ins)] + [m2d.grad]
        if camera:
            res += [rs.viewmatrix.grad, rs.projmatrix.grad, rs.campos.grad]
        assert all(r is not None for r in res)
        return res

    if "deep" in opts:
        _C.check(_C.lib.scr_debug_force_deep_lists(1))
    try:
        out = _check("rasterizer", f"{scene} P={P} {W}x{H} {variant}", fn)
    finally:
        if "deep" in opts:
            _C.check(_C.lib.scr_debug_force_deep_lists(-1))
    n_out = 4 if aux else 2
    for a, b in zip(out[:n_out], out[n_out:2 * n_out]):
        assert poison.same_bits(a, b)                         # the two binning paths: the same image, radii and maps
    radii = out[1]
    culled = radii == 0
    _log(f"fresh_memory rasterizer     {scene} {variant}: {int(culled.sum())} of {P} Gaussians culled")
    assert int(culled.sum()) == {"culled": 2, "one": 0}.get(scene, int(culled.sum())) and (scene != "wide" or 0 < int(culled.sum()) < P)
    for grad in out[2 * n_out + 2:2 * n_out + 2 + len(base) + 1]:
        assert grad.shape[0] == P and not grad[culled].any()


# ---------------------------------------------------------------------------------------- anchor gather, BatchNorm-Linear
def _gather_case(N, idx, defer, ranges):
    from splatco_amd import anchor_gather as ag
    from splatco_amd import scene_model as sm
    from splatco_amd.scene_model import AnchorGaussianModel
    g = _gen(N + 17)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    params = (r(N, 3) * 2, r(N, 10, 3), r(N, 32) * 3 + 0.5, r(N, 6) * 0.3 - 3)
    V = idx.numel()
    G0, c0 = r(32, 71) * 0.2, r(32)
    w_y, w_feat, w_off, w_gs, w_anc = r(V, 32), r(V, 32), r(V, 10, 3), r(V, 6), r(V, 3)
    torch.manual_seed(0)
    pc = AnchorGaussianModel(plane_size=16, num_channels=15).to(DEV)

    def fn():
        pc.set_anchors(*(t.clone() for t in params))
        G, c = G0.clone().requires_grad_(), c0.clone().requires_grad_()
        sink, seen = None, []
        if ranges:
            # the sink's tensors are the caller's gradient memory, handed over UNWRITTEN: the kernel overwrites every element
            grads = [torch.empty_like(p) for p in (pc._anchor_feat, pc._anchor, pc._offset, pc._scaling)]
            sink = ag.GradSink(*grads)
            sink.ranges, sink.on_range = ranges, seen.append
        pc._grad_sink = sink
        try:
            feat, anc, off, gs, g_fea = ag.gather_anchors(pc, idx)
        finally:
            pc._grad_sink = None
        box = g_fea._scr_deferred_dx
        y, mean, var = sm._NormLinearFn.apply(g_fea, G, c, 1e-5, getattr(g_fea, "_scr_col_stats", None), box if defer else None)
        ((y * w_y).sum() + (feat * w_feat).sum() + (off * w_off).sum() + (gs * w_gs).sum() + (anc * w_anc).sum()).backward()
        assert box.coef is None
        if ranges:
            assert seen == list(range(len(ranges)))
        else:
            grads = [p.grad for p in (pc._anchor_feat, pc._anchor, pc._offset, pc._scaling)]
        return [feat, anc, off, gs, g_fea, y, mean, var] + list(grads) + [G.grad, c.grad]
    return fn


@pytest.mark.parametrize("N,select,defer,ranged", [(40, "80%", False, False), (40, "80%", True, False), (5003, "80%", False, False),
                                                   (5003, "80%", True, False), (5003, "80%", True, True), (40, "80%", True, True),
                                                   (5003, "row0", True, False), (5003, "row0", False, False), (40, "row0", True, True)])
def test_anchor_gather_and_its_hand_over_to_the_norm_linear(N, select, defer, ranged):
    """gather_anchors -> _NormLinearFn, with and without the deferred dx (the gather's backward forms dx itself), into
    autograd's gradients or into a GradSink's unwritten memory range by range.  Invisible anchors: exactly 0."""
    g = _gen(N)
    idx = (torch.rand(N, device=DEV, generator=g) < 0.8).nonzero().squeeze(1) if select == "80%" else torch.zeros(1, dtype=torch.long, device=DEV)
    step = max(64, (N // 3 + 63) // 64 * 64)
    ranges = [(a, min(N, a + step)) for a in range(0, N, step)] if ranged else None
    out = _check("anchor_gather", f"N={N} V={idx.numel()} defer={int(defer)} ranges={len(ranges or ())}", _gather_case(N, idx, defer, ranges))
    vis = torch.zeros(N, dtype=torch.bool, device=DEV)
    vis[idx] = True
    for grad in out[8:12]:
        assert grad.shape[0] == N and not grad[~vis].any() and bool(grad[vis].any())


@pytest.mark.parametrize("V,d,ld", [(2, 60, 60), (15, 71, 71), (1000, 60, 64), (4099, 16, 99)])
def test_norm_linear_alone(V, d, ld):
    """_NormLinearFn on a column block of a wider matrix: padding columns (ld > d) and rows that are not 16-byte aligned."""
    from splatco_amd import scene_model as sm
    g = _gen(V * 131 + d)
    base = torch.randn(V, ld, device=DEV, generator=g)
    base[:, : d // 2] = base[:, : d // 2] * 0.3 - 5.0
    G0, c0, w = torch.randn(32, d, device=DEV, generator=g) * 0.2, torch.randn(32, device=DEV, generator=g), torch.randn(V, 32, device=DEV, generator=g)

    def fn():
        x = base.clone()[:, :d].requires_grad_()
        G, c = G0.clone().requires_grad_(), c0.clone().requires_grad_()
        y, mean, var = sm._NormLinearFn.apply(x, G, c, 1e-5)
        (y * w).sum().backward()
        return [y, mean, var, x.grad, G.grad, c.grad]

    out = _check("norm_linear", f"V={V} d={d} ld={ld}", fn)
    assert out[3].shape == (V, d) and out[0].shape == (V, 32)


# ---------------------------------------------------------------------------------------------------------------- tri-plane
_PAIRS = ((1, 0), (2, 0), (2, 1))
PLANES = (40, 36, 44)


def _points(V, seed, lim=1.08):
    """V sample positions: random ones, some outside the planes, the first ones exactly on corners and borders."""
    g = _gen(seed)
    ind = torch.rand(V, 3, device=DEV, generator=g) * 2 * lim - lim
    fixed = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [-1.0, 1.0, 0.3], [0.25, -1.0, 1.0], [1.0, 0.0, -1.0], [0.0, 0.0, 0.0]], device=DEV)
    n = min(V, len(fixed)) if V > 2 else 0           # V = 1 and 2 stay random (the parity test takes both kinds, see there)
    ind[:n] = fixed[:n]
    return ind


def _triple(R, sizes, g, scale=0.5):
    X, Y, Z = sizes
    return [(torch.randn(1, R, a, b, device=DEV, generator=g) * scale) for a, b in ((X, Y), (X, Z), (Y, Z))]


def _touched(ind, plane_shape, j):
    """A superset of the nodes of plane j (pair _PAIRS[j % 3]) that any sample's bilinear footprint reaches, in float64 with a
    margin of 1e-4 cells either way for the kernel's float32 coordinate."""
    _, _, A, B = plane_shape
    cx, cy = _PAIRS[j % 3]
    hit = torch.zeros(A, B, dtype=torch.bool, device=DEV)
    x = (ind[:, cx].double() + 1) * 0.5 * (B - 1)
    y = (ind[:, cy].double() + 1) * 0.5 * (A - 1)
    for ex in (-1e-4, 1e-4):
        for ey in (-1e-4, 1e-4):
            for dx in (0, 1):
                for dy in (0, 1):
                    ix, iy = torch.floor(x + ex).long() + dx, torch.floor(y + ey).long() + dy
                    ok = (ix >= 0) & (ix < B) & (iy >= 0) & (iy < A)
                    hit[iy[ok], ix[ok]] = True
    return hit


def _quiet_nodes_are_zero(ind, grads, what):
    """Every node no sample reaches holds exactly 0.  Returns their number (with 65 points or fewer there must be some)."""
    quiet_total = 0
    for j, gp in enumerate(grads):
        quiet = ~_touched(ind, gp.shape, j)
        quiet_total += int(quiet.sum())
        assert not gp[0][:, quiet].any(), (what, j)
    assert quiet_total > 0 or ind.shape[0] > 65, what
    return quiet_total


@pytest.fixture(params=["plane-major", "row-pairs"])
def layout(request, monkeypatch):
    """Both plane layouts of the forward at these sizes: the row-pair layout normally starts at 262144 points."""
    from splatco_amd import triplane
    if request.param == "row-pairs":
        monkeypatch.setattr(triplane, "CHANNEL_LAST_MIN_POINTS", 1)
    return request.param


@pytest.mark.parametrize("R", [2, 5, 15])
@pytest.mark.parametrize("V", [1, 64, 65, 3000])
def test_triplane_sample(V, R, layout):
    from splatco_amd.triplane import triplane_sample
    g = _gen(V * 16 + R)
    ind, planes0, w = _points(V, V + R), _triple(R, PLANES, g), torch.randn(V, 3 * R, device=DEV, generator=g)

    def fn():
        planes = [p.clone().requires_grad_() for p in planes0]
        out = triplane_sample(ind, planes)
        (out * w).sum().backward()
        return [out] + [p.grad for p in planes]

    out = _check("triplane", f"triplane_sample V={V} R={R} {layout}", fn)
    assert out[0].shape == (V, 3 * R)
    quiet = _quiet_nodes_are_zero(ind, out[1:], (V, R, layout))
    assert V > 65 or quiet > 0.8 * sum(p[0, 0].numel() for p in planes0)        # almost every node is untouched


@pytest.mark.parametrize("V", [1, 65, 3000])
def test_triplane_six_plane_attention_layout(V, layout):
    """Plain and attended planes of one grid, sampled at the same positions, columns interleaved (FeaturePlanes' level 0)."""
    from splatco_amd.triplane import multi_triplane_sample
    R = 5
    g = _gen(V + 600)
    ind, w = _points(V, V + 6), torch.randn(V, 6 * R, device=DEV, generator=g)
    planes0 = _triple(R, (40, 40, 40), g) + _triple(R, (40, 40, 40), g)
    cols = tuple(c * R for c in (0, 2, 4, 1, 3, 5))

    def fn():
        planes = [p.clone().requires_grad_() for p in planes0]
        out = multi_triplane_sample([(ind, tuple(planes), cols)])
        (out * w).sum().backward()
        return [out] + [p.grad for p in planes]

    out = _check("triplane", f"six planes V={V} R={R} {layout}", fn)
    _quiet_nodes_are_zero(ind, out[1:], (V, layout))


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("V", [1, 65, 3000])
def test_triplane_three_grids_and_the_hand_over_to_the_norm_linear(V, defer, fuse, layout, monkeypatch):
    """The 10-5-5 layout: three grids into one matrix that a fused BatchNorm-Linear consumes, the backward of all grids in
    one pass (FUSE_GRIDS) or grid by grid, forming the matrix's gradient rows itself (deferred dx) or reading them."""
    from splatco_amd import scene_model as sm
    from splatco_amd import triplane
    monkeypatch.setattr(triplane, "FUSE_GRIDS", fuse)
    Rs, sizes = (10, 5, 5), [PLANES, (24, 20, 28), (12, 16, 10)]
    g = _gen(V + 1055)
    ind = _points(V, V + 10, lim=1.05)
    tris0 = [_triple(R, s, g, scale=1.0) for R, s in zip(Rs, sizes)]
    width = 3 * sum(Rs)
    G0, c0, w_y = torch.randn(32, width, device=DEV, generator=g) * 0.2, torch.randn(32, device=DEV, generator=g), torch.randn(V, 32, device=DEV, generator=g)

    def fn():
        tris = [[p.clone().requires_grad_() for p in tri] for tri in tris0]
        G, c = G0.clone().requires_grad_(), c0.clone().requires_grad_()
        grids, col = [], 0
        for R, tri in zip(Rs, tris):
            grids.append((ind, tuple(tri), (col, col + R, col + 2 * R)))
            col += 3 * R
        x = triplane.multi_triplane_sample(grids)
        box = x._scr_deferred_dx
        y, mean, var = sm._NormLinearFn.apply(x, G, c, 1e-5, None, box if defer else None)
        (y * w_y).sum().backward()
        assert box.coef is None
        return [x, y, mean, var, G.grad, c.grad] + [p.grad for tri in tris for p in tri]

    out = _check("triplane", f"10-5-5 V={V} defer={int(defer)} fuse={int(fuse)} {layout}", fn)
    for k in range(3):
        _quiet_nodes_are_zero(ind, out[6 + 3 * k:9 + 3 * k], (V, defer, fuse, layout, k))


@pytest.mark.parametrize("V,R,A,B", [(1, 5, 40, 36), (65, 2, 33, 17), (3000, 15, 36, 44)])
def test_plane_sample(V, R, A, B):
    from splatco_amd.triplane import plane_sample
    g = _gen(V + R)
    grid = _points(V, V)[:, :2].contiguous()
    plane0, w = torch.randn(1, R, A, B, device=DEV, generator=g), torch.randn(V, R, device=DEV, generator=g)

    def fn():
        plane = plane0.clone().requires_grad_()
        out = plane_sample(plane, grid)
        (out * w).sum().backward()
        return [out, plane.grad]

    out = _check("triplane", f"plane_sample V={V} R={R} {A}x{B}", fn)
    ind3 = torch.cat([grid[:, 1:2], grid[:, 0:1], grid[:, 0:1]], dim=1)          # plane 0 of a triple reads (x, y) = (ind[1], ind[0])
    _quiet_nodes_are_zero(ind3, out[1:], (V, R))


@pytest.mark.parametrize("R,H,W", [(5, 24, 24), (3, 33, 17)])
def test_plane_attention(R, H, W):
    from splatco_amd import plane_attention
    from splatco_amd.scene_model import TriPlaneAttention
    torch.manual_seed(R * 1000 + H)
    ta = TriPlaneAttention(3 * R).to(DEV)
    g = _gen(R + H)
    planes0 = [torch.randn(1, R, H, W, device=DEV, generator=g) * 0.5 for _ in range(3)]
    ws = [torch.randn(1, 2 * R, H, W, device=DEV, generator=g) for _ in range(3)]
    assert plane_attention.fused_ok(*planes0, ta)

    def fn():
        planes = [p.clone().requires_grad_() for p in planes0]
        for p in ta.parameters():
            p.grad = None
        out = plane_attention.attended_pair_planes(*planes, ta)
        sum((o * wi).sum() for o, wi in zip(out, ws)).backward()
        return list(out) + [p.grad for p in planes] + [p.grad for p in ta.parameters()]

    out = _check("attention", f"R={R} {H}x{W}", fn)
    assert len(out) == 6 + len(list(ta.parameters())) and out[0].shape == (1, 2 * R, H, W)


# ---------------------------------------------------------------------------------------------------------------- MLP heads
@pytest.mark.parametrize("V", [1, 37, 257])
def test_mlp_heads(V):
    from splatco_amd.mlp_heads import mlp_heads, supported
    from splatco_amd.scene_model import AnchorGaussianModel
    torch.manual_seed(V)
    pc = AnchorGaussianModel(plane_size=16, num_channels=15).to(DEV)
    with torch.no_grad():
        for p in list(pc.mlp_opacity.parameters()) + list(pc.mlp_color.parameters()) + list(pc.mlp_cov.parameters()):
            p.add_(0.2 * torch.randn_like(p))
    g = _gen(V + 1)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    feat, anchor, geo, cam = r(V, 32), r(V, 3) * 2, r(V, 64), torch.tensor([0.3, -0.2, -5.0], device=DEV)
    w = [r(V, 10), r(V, 30), r(V, 70)]
    heads = [p for n, p in pc.named_parameters() if n.startswith("mlp_")]

    def fn():
        f, a, ge = (t.clone().requires_grad_() for t in (feat, anchor, geo))
        for p in pc.parameters():
            p.grad = None
        assert supported(pc, f, ge)
        outs = mlp_heads(pc, f, a, cam, ge) if V == 37 else mlp_heads(pc, f, a, cam, ge[:, :32].contiguous(), ge[:, 32:].contiguous())
        sum((o * wi).sum() for o, wi in zip(outs, w)).backward()
        return list(outs) + [f.grad, a.grad, ge.grad] + [p.grad for p in heads]

    out = _check("mlp_heads", f"V={V}", fn)
    assert len(out) == 3 + 3 + 12 and out[0].shape[0] == V


# ------------------------------------------------------------------------------------------------- expansion and compaction
@pytest.mark.parametrize("select", ["mixed", "none", "all"])
@pytest.mark.parametrize("V", [1, 37, 1025])
def test_expand_compact(V, select):
    from splatco_amd.expand import expand_compact
    k = 10
    g = _gen(V + len(select))
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    no = r(V * k, 1)
    no = {"mixed": no, "none": -no.abs(), "all": no.abs() + 0.01}[select]
    if select == "none":
        no[::3] = 0.0                                     # exactly 0 is not selected
    base = (no, r(V * k, 3), r(V * k, 7), r(V, k, 3), torch.rand(V, 6, device=DEV, generator=g) + 0.1, r(V, 3))
    P = int((no > 0).sum())
    ws = [r(P, n) for n in (3, 3, 1, 3, 4)]

    def fn():
        ins = [t.clone().requires_grad_() for t in base]
        *outs, mask = expand_compact(*ins, k)
        sum((o * wi).sum() for o, wi in zip(outs, ws)).backward()
        return list(outs) + [mask, mask._scr_out_index] + [t.grad for t in ins]

    out = _check("expand", f"expand_compact V={V} k={k} {select} P={P}", fn)
    mask, index = out[5], out[6]
    assert torch.equal(mask, (no > 0).view(-1)) and out[0].shape == (P, 3)
    want = torch.where(mask, torch.cumsum(mask, 0, dtype=torch.int32) - 1, torch.full_like(index, -1))
    assert torch.equal(index, want)
    for grad in out[7:10]:                                # per-candidate gradients: exactly 0 where the candidate was dropped
        assert not grad[~mask].any()
    if select == "none":
        assert all(not grad.any() for grad in out[7:])


@pytest.mark.parametrize("fill", ["none", "one", "all"])
@pytest.mark.parametrize("n", [1, 1025])
def test_mask_indices_and_visible_indices(n, fill):
    from splatco_amd.expand import mask_indices, visible_indices
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    if fill == "one":
        mask[n // 2] = True
    elif fill == "all":
        mask[:] = True

    def fn():
        a, b, c = mask_indices(mask), mask_indices(mask.view(torch.uint8), inverse=False), visible_indices(mask.clone())
        return [a, a._scr_inverse, b, c, c._scr_inverse]

    out = _check("expand", f"mask_indices n={n} {fill}", fn)
    want = mask.nonzero().squeeze(1)
    inv = torch.full((n,), -1, dtype=torch.long, device=DEV)
    inv[want] = torch.arange(want.numel(), device=DEV)
    assert all(torch.equal(out[i], want) for i in (0, 2, 3)) and torch.equal(out[1], inv) and torch.equal(out[4], inv)


def test_voxelize_through_the_unique_compaction():
    from splatco_amd import scene_init
    g = _gen(20)
    pts = torch.rand(2000, 3, device=DEV, generator=g) * 2 - 1
    pts[500:900] = pts[:400] + 1e-4                       # duplicates of a voxel

    def fn():
        return [scene_init.voxelize(pts, 0.05), scene_init.voxelize(pts, 0.05, _force_rows=True), scene_init.voxelize(pts, 10.0)]

    out = _check("expand", "voxelize 2000 points", fn)
    assert torch.equal(out[0], out[1]) and 1000 < out[0].shape[0] < 2000 and out[2].shape == (1, 3)
    assert torch.equal(out[0], scene_init.voxelize(pts.cpu(), 0.05).to(DEV))


# --------------------------------------------------------------------------------------------------- image losses, metrics
IMAGES = [(1, 1), (17, 33), (70, 130)]


@pytest.mark.parametrize("H,W", IMAGES)
def test_image_losses(H, W):
    """l1_ssim, pair_l1, scaling_reg (on its own and through the expansion's tap) and view_loss, value and gradients."""
    from splatco_amd.expand import expand_compact
    from splatco_amd.losses import l1_ssim, pair_l1, scaling_reg, view_loss
    g = _gen(H * 1000 + W)
    u = lambda *s: torch.rand(*s, device=DEV, generator=g)
    img0, gt, a0, b0, r1, r2 = (u(3, H, W) for _ in range(6))
    P = H * W
    s0 = u(P, 3) * 0.2
    if P > 10:
        s0[3, 1] = 0.0
        s0[7] = 0.0
    V, k = (P + 9) // 10, 10
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    ebase = (r(V * k, 1), r(V * k, 3), r(V * k, 7), r(V, k, 3), u(V, 6) + 0.1, r(V, 3))

    def fn():
        res = []
        img = img0.clone().requires_grad_()
        l1, ss = l1_ssim(img, gt)
        (0.8 * l1 + 0.2 * (1 - ss)).backward()
        res += [l1, ss, img.grad]
        a, b = a0.clone().requires_grad_(), b0.clone().requires_grad_()
        pl = pair_l1(a, b, r1, r2)
        (pl * 0.37).backward()
        res += [pl, a.grad, b.grad]
        a = a0.clone().requires_grad_()
        pl = pair_l1(a, b0, r1, r2)                          # one side only: the other gradient pointer is NULL
        pl.backward()
        res += [pl, a.grad]
        s = s0.clone().requires_grad_()
        reg = scaling_reg(s)
        (reg * 3.0).backward()
        res += [reg, s.grad]
        ins = [t.clone().requires_grad_() for t in ebase]
        xyz, color, opacity, scaling, rot, mask = expand_compact(*ins, k)
        if scaling.shape[0]:
            assert hasattr(scaling, "_scr_reg_tap")
            tapped = 700.0 * scaling_reg(scaling) + (scaling * 0.25).sum() + (xyz * 0.3).sum()
            tapped.backward()
            res += [tapped] + [t.grad for t in ins]
        img, s = img0.clone().requires_grad_(), s0.clone().requires_grad_()
        vl = view_loss(img, gt, s)
        vl.backward()
        return res + [vl, img.grad, s.grad]

    _check("losses", f"l1_ssim pair_l1 scaling_reg view_loss {H}x{W}", fn)


@pytest.mark.parametrize("mode", ["inverse", "expected"])
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("H,W", IMAGES)
def test_depth_loss_through_the_wrapper(H, W, mode, align):
    from depth_loss_ref import recipe
    from splatco_amd.losses import depth_loss
    D, A, tgt, m = recipe(H, W, 1, device=DEV, mask_kind="f32", mode=mode, line=(1.7, -0.08) if align else (1.0, 0.0))

    def fn():
        D_, A_ = D.clone().requires_grad_(), A.clone().requires_grad_()
        loss, stats = depth_loss(D_, A_, tgt, m, mode=mode, align=align, return_stats=True)
        (loss * 1.5).backward()
        only = D.clone().requires_grad_()
        depth_loss(only, A, tgt, m, mode=mode, align=align).backward()          # one map only: the other pointer is NULL
        return [loss, stats, D_.grad, A_.grad, only.grad]

    _check("losses", f"depth_loss {H}x{W} {mode} align={int(align)}", fn)


@pytest.mark.parametrize("H,W", IMAGES)
def test_metrics(H, W):
    from splatco_amd.metrics import flip, flip_and_mse, ssim_value
    g = _gen(H + W)
    a, b = torch.rand(2, 3, H, W, device=DEV, generator=g), torch.rand(2, 3, H, W, device=DEV, generator=g)

    def fn():
        mean, fmap = flip(a, b, return_map=True)
        mean1, fmap1 = flip(a[0], b[0], quantize=True, return_map=True)
        fm, mse = flip_and_mse(a, b)
        return [mean, fmap, mean1, fmap1, fm, mse, flip(a[1], b[1]), ssim_value(a[0], b[0])]

    out = _check("metrics", f"flip flip_and_mse ssim_value {H}x{W}", fn)
    assert out[1].shape == (2, H, W) and out[3].shape == (H, W)


# ------------------------------------------------------------------------------------------------------------ densification
def _statis_inputs(N, V, k, seed, inverted=False):
    """Accumulators over N anchors of which V are visible; k candidates per anchor, some selected, some of those rendered.
    inverted: every opacity <= 0 -- no candidate selected, no Gaussian at all (empty filter and gradient)."""
    g = _gen(seed)
    u = lambda *s: torch.rand(*s, device=DEV, generator=g)
    acc = [u(N, 1), u(N, 1).round(), u(N * k, 1), u(N * k, 1).round()]
    vis = torch.zeros(N, dtype=torch.bool, device=DEV)
    vis[torch.randperm(N, device=DEV, generator=g)[:V]] = True
    no = torch.randn(V * k, 1, device=DEV, generator=g)
    if inverted:
        no = -no.abs()
    sel = (no > 0).view(-1)
    P = int(sel.sum())
    upd = u(P) < 0.7
    grad = torch.randn(P, 3, device=DEV, generator=g)
    return acc, vis, no, sel, upd, grad


@pytest.mark.parametrize("inverted", [False, True])
@pytest.mark.parametrize("V", [1, 300])
@pytest.mark.parametrize("k", [10, 9])
def test_training_statis(k, V, inverted):
    """k = 10: two candidates per lane; k = 9: one.  The four accumulators are accumulated into (the caller's values go in);
    the increments are fresh memory, -1 where nothing is counted."""
    from splatco_amd.stats import statis_increments, training_statis
    N = V + 7
    acc0, vis, no, sel, upd, grad = _statis_inputs(N, V, k, 100 * k + V, inverted)

    def fn():
        acc = [a.clone() for a in acc0]
        training_statis(*acc, k, grad, no, upd, sel, vis.clone())
        return acc + list(statis_increments(k, grad, no, upd, sel))

    out = _check("densify", f"training_statis k={k} V={V} N={N} inverted={int(inverted)}", fn)
    for got, was in zip(out[:2], acc0[:2]):
        assert torch.equal(got[~vis], was[~vis])
    assert torch.equal(out[1][vis], acc0[1][vis] + 1)
    if inverted:
        assert bool((out[5] == -1).all()) and torch.equal(out[2], acc0[2]) and torch.equal(out[3], acc0[3]) and not out[4].any()


def test_knn_curvature_and_dist2():
    from splatco_amd import scene_init
    from splatco_amd.densify import _knn_indices, compute_curvature
    g = _gen(31)
    pts = torch.rand(2000, 3, device=DEV, generator=g) * 4 - 2
    pts[:400] = torch.randn(400, 3, device=DEV, generator=g) * 0.01 + 0.3          # a dense clump
    pts[400:800, 2] = 0.25                                                          # a plane
    pts[800:803] = pts[0]                                                           # duplicates (fewer than any k here: no neighbourhood is one point)

    def fn():
        return [_knn_indices(pts, 10), compute_curvature(pts), compute_curvature(pts, k=5), scene_init.dist2(pts)]

    out = _check("densify", "knn, curvature, dist2 at 2000 points", fn)
    assert out[0].shape == (2000, 10) and 0 <= int(out[0].min()) and int(out[0].max()) < 2000
    assert torch.equal(out[3], scene_init.dist2(pts.cpu()).to(DEV))


# ------------------------------------------------------------------------------------------------------------ the whole step
def test_two_collaborative_steps():
    """Two training steps on the same objects -- two 160 x 96 views, GradArena, FusedAdam, consistency and total-variation
    terms, an AnchorDensifier -- rebuilt from the same seeds in every run: the empties of scene_model.py, renderer.py,
    multiview.py and train_step.py that no single-operator case reaches."""
    from splatco_amd.adam import FusedAdam
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.densify import AnchorDensifier
    from splatco_amd.multiview import GradArena
    from splatco_amd.synthetic import synthetic_anchor_model
    from splatco_amd.train_step import collaborative_step
    cams = [look_at_camera(eye=(0.3 + 0.4 * i, -0.2, -6.0), target=(0, 0, 0), up=(0, -1, 0), FoVx=math.radians(60),
                           width=160, height=96, uid=i).to(DEV) for i in range(2)]
    base = torch.rand(3, 96, 160, generator=torch.Generator().manual_seed(4))
    gts = [(base + 0.01 * i).clamp(0, 1).to(DEV) for i in range(2)]       # alike: SSIM(gt_i, gt_j) > 0.6 switches the consistency term on
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    bg = torch.ones(3, device=DEV)
    seen = {}

    def fn():
        torch.manual_seed(11)
        pc = synthetic_anchor_model(3000, 9, DEV, plane_size=64)
        idle = {id(p) for p in pc.feat_planes._feat.inactive_parameters()}
        groups = [{"params": [getattr(pc, "_" + n)], "lr": 1e-3, "name": n} for n in ("anchor", "offset", "anchor_feat", "scaling")]
        rest = [p for n, p in pc.named_parameters() if not n.startswith("_") and p.requires_grad and id(p) not in idle]
        groups.append({"params": rest, "lr": 1e-3, "name": "mlp_and_feat_planes"})
        params = [p for grp in groups for p in grp["params"]]
        opt = FusedAdam(groups, eps=1e-15)
        den = AnchorDensifier(pc, opt, voxel_size=0.01, seed=5)
        arena = GradArena(params)
        res = []
        for it in range(2):
            loss, out, _ = collaborative_step(pc, cams, gts, pipe, bg, optimizer=opt, consistency_weight=0.05, densifier=den,
                                              arena=arena, iteration=4 * (it + 1), tv_weight=1e-3)
            res += [loss, out["render"]]
        seen["visible"] = int((out["radii"] > 0).sum())
        res += [p.detach() for p in params]
        res += [opt.state[p][name] for p in params if p in opt.state for name in ("exp_avg", "exp_avg_sq")]
        return res + [den.opacity_accum, den.anchor_demon, den.offset_gradient_accum, den.offset_denom]

    out = _check("step", "two collaborative steps, 2 views 160x96, 3000 anchors", fn)
    assert seen["visible"] > 100 and float(out[-3].sum()) > 0 and float(out[-1].sum()) > 0
    assert not torch.equal(out[1], out[3])                   # the second step rendered other parameters


# ============================================================================================ parity at the small shapes
_TRIPLANE_FIGURES = {}
COORD_EPS = 1.25e-7       # bound of the float32 error of ((x + 1) / 2) per unit of (B - 1), |x| <= 1.08: half an ulp of x + 1 <= 2.08
                          # (1.2e-7, halved by the / 2) plus 2^-24 of the product with (B - 1)


def _bounded_triple(R, sizes, g):
    """Planes whose neighbouring texels -- the zero padding around the plane included -- differ by at most
    4 / ((A - 1) + (B - 1)): uniform in +-2 / ((A - 1) + (B - 1)).  See _conditioning."""
    X, Y, Z = sizes
    return [(torch.rand(1, R, a, b, device=DEV, generator=g) * 2 - 1) * (2.0 / (a + b - 2)) for a, b in ((X, Y), (X, Z), (Y, Z))]


def _conditioning(p):
    """What the float32 rounding of the two cell coordinates can move a bilinear sample of plane p by, at most: the coordinate
    errors COORD_EPS (B - 1) and COORD_EPS (A - 1) times the steepest slope per cell, i.e. the largest difference of
    neighbouring texels, the zero padding included (a sample within one cell outside the border interpolates towards 0)."""
    q = torch.nn.functional.pad(p.detach().double(), (1, 1, 1, 1))
    dmax = max(float((q[..., 1:, :] - q[..., :-1, :]).abs().max()), float((q[..., :, 1:] - q[..., :, :-1]).abs().max()))
    return COORD_EPS * (p.shape[2] - 1 + p.shape[3] - 1) * dmax


def _triplane_figures(V, layout, bounded):
    """triplane_sample (one grid) and multi_triplane_sample (attention grid + two plain grids, R = 5: column blocks at every
    16-byte phase) once per (V, layout, kind of planes), shared by the tests below.  Per case (random / edge points) and
    plane: the forward excess max(|e| - 1e-5 |ref|) (allclose(rtol 1e-5, atol 1e-6) asks <= 1e-6) and the backward max |e| and
    scale, for [kernel vs float64, torch's float32 grid_sample vs float64, kernel vs torch's float32], and the plane's
    _conditioning.  Points exactly on the plane corners and borders, and points outside the planes, are among the samples at
    every V: V = 1 and 2 run once with random points and once with a corner and a border point.
    bounded: planes of _bounded_triple; otherwise 0.5 x standard normal, as the existing tri-plane tests take them."""
    import torch.nn.functional as F
    from splatco_amd.triplane import multi_triplane_sample, triplane_sample
    if (V, layout, bounded) in _TRIPLANE_FIGURES:
        return _TRIPLANE_FIGURES[V, layout, bounded]
    R, rows = 5, []
    excess = lambda a, ref: float(((a - ref).abs() - 1e-5 * ref.abs()).max())
    for edge in ((False, True) if V <= 2 else (True,)):
        g = _gen(V * 7 + int(edge))
        ind = torch.tensor([[1.0, -1.0, 1.0], [-1.0, 0.25, 1.0]], device=DEV)[:V] if edge and V <= 2 else _points(V, V + 41, lim=1.0 if V <= 2 else 1.08)
        mk = lambda n, sizes: [p.requires_grad_() for _ in range(n // 3) for p in (_bounded_triple if bounded else _triple)(R, sizes, g)]
        single = mk(3, PLANES)
        grids = [(mk(6, (40, 40, 40)), tuple(c * R for c in (0, 2, 4, 1, 3, 5))),
                 (mk(3, (40, 48, 56)), tuple(6 * R + c * R for c in range(3))),
                 (mk(3, (24, 20, 28)), tuple(9 * R + c * R for c in range(3)))]
        w1, w = torch.randn(V, 3 * R, device=DEV, generator=g), torch.randn(V, 12 * R, device=DEV, generator=g)
        out1 = triplane_sample(ind, single)
        (out1 * w1).sum().backward()
        out = multi_triplane_sample([(ind, tuple(pl), cols) for pl, cols in grids])
        assert out.shape == (V, 12 * R) and out1.shape == (V, 3 * R)
        (out * w).sum().backward()
        todo = [("one grid", single, tuple(R * j for j in range(3)), out1, w1)] + [(f"grid {k} of 3", pl, cols, out, w) for k, (pl, cols) in enumerate(grids)]
        for name, pl, cols, o, wt in todo:
            for j, p in enumerate(pl):
                res = []
                for dtype in (torch.float64, torch.float32):
                    q = p.detach().to(dtype).requires_grad_()
                    grid = ind[:, list(_PAIRS[j % 3])].to(dtype).view(1, 1, V, 2)
                    samp = F.grid_sample(q, grid, mode="bilinear", align_corners=True).flatten(0, 2).T
                    (samp * wt[:, cols[j]:cols[j] + R].to(dtype)).sum().backward()
                    res.append((samp.detach().double(), q.grad.double()))
                (s64, g64), (s32, g32) = res
                got, ggot = o[:, cols[j]:cols[j] + R].detach().double(), p.grad.double()
                rows.append(dict(case=f"edge={int(edge)} {name} plane {j}", cond=_conditioning(p), amplitude=float(s64.abs().max()),
                                 fwd=[excess(got, s64), excess(s32, s64), excess(got, s32)],
                                 bwd=[float((x - y).abs().max()) for x, y in ((ggot, g64), (g32, g64), (ggot, g32))],
                                 scale=[float(g64.abs().max()), float(g64.abs().max()), float(g32.abs().max())]))
    worst = lambda key, i: max(r[key][i] / (max(r["scale"][i], 1e-30) if key == "bwd" else 1.0) for r in rows)
    _log(f"parity triplane V={V:3d} {layout:11s} {'bounded' if bounded else 'normal':7s} planes (coordinate rounding moves a sample by <= {max(r['cond'] for r in rows):.1e}) "
         f"forward max(|e| - 1e-5 |ref|), bar 1e-6: kernel/f64 {worst('fwd', 0):.2e}  torch32/f64 "
         f"{worst('fwd', 1):.2e}  kernel/torch32 {worst('fwd', 2):.2e};  backward max |e| / scale, bar 5e-5: {worst('bwd', 0):.2e}  "
         f"{worst('bwd', 1):.2e}  {worst('bwd', 2):.2e}")
    _TRIPLANE_FIGURES[V, layout, bounded] = rows
    return rows


SMALL_V = [1, 2, 63, 64, 65, 257]


@pytest.mark.parametrize("V", SMALL_V)
def test_triplane_forward_parity_with_float64_grid_sample_at_small_sizes(V, layout):
    """Forward against F.grid_sample per plane in float64 at rtol 1e-5 / atol 1e-6 (the forward bar of
    test_multi_grid_sampling_into_one_matrix_all_alignments, whose reference is torch's float32 grid_sample).

    The planes' contents are chosen for the reference.  The operator is defined in float32: the cell coordinate
    ((x + 1) / 2) (B - 1) carries a float32 rounding error of up to COORD_EPS (B - 1) cells, which moves the sample by that
    times the difference of the neighbouring texels -- in ANY float32 evaluation, torch's own included, and whatever the
    kernel does with the texels.  An absolute bar of 1e-6 against float64 can therefore only be asked of planes whose
    _conditioning is below it; with 0.5 x standard normal texels (differences up to 3 across a cell) on planes of 20 to 56
    nodes it is 1e-5 to 4e-5, and both the kernel and torch's float32 grid_sample are off from float64 by the same
    2.6e-6 to 5.5e-6 at V >= 63 (profiles/r15_fresh_memory.txt; they agree with each other to 1.5e-8, the test below).  So
    this test takes the LARGEST texel differences at which the bar can be asked at all: uniform texels of amplitude
    2 / ((A - 1) + (B - 1)), which bounds the coordinate's share by 5e-7, half the bar (asserted on the planes, before
    anything is compared), and leaves the other half to the arithmetic on the texels.  At that amplitude (0.02 to 0.05) a
    wrong node, a swapped weight or a missed border still shows as 1e-2, four orders above the bar."""
    rows = _triplane_figures(V, layout, True)
    assert all(r["cond"] <= 0.5e-6 * (1 + 1e-6) for r in rows), max(r["cond"] for r in rows)
    assert max(r["amplitude"] for r in rows) > 0.01 or V <= 2          # the samples are not all padding
    bad = [(r["case"], r["fwd"][0]) for r in rows if not r["fwd"][0] <= 1e-6]
    assert not bad, (V, layout, bad)


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("V", SMALL_V)
def test_triplane_plane_gradient_parity_with_float64_grid_sample_at_small_sizes(V, layout, bounded):
    """Plane gradients against float64 autograd through F.grid_sample: 5e-5 x scale + 1e-7, the backward bar of
    test_multi_grid_sampling_into_one_matrix_all_alignments.  The gradient of a plane does not depend on its texels, and the
    coordinate's rounding is at most COORD_EPS x 55 = 7e-6 of a weight: inside the bar for either kind of plane."""
    bad = [(r["case"], r["bwd"][0], r["scale"][0]) for r in _triplane_figures(V, layout, bounded) if not r["bwd"][0] <= 5e-5 * r["scale"][0] + 1e-7]
    assert not bad, (V, layout, bad)


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("V", SMALL_V)
def test_triplane_parity_with_float32_grid_sample_at_small_sizes(V, layout, bounded):
    """The same samples and gradients against torch's float32 grid_sample, the reference and both bars of
    test_multi_grid_sampling_into_one_matrix_all_alignments, whose smallest V is 70 001: here the coordinate's rounding is
    common to both sides, so the bar holds on 0.5 x standard normal planes too."""
    rows = _triplane_figures(V, layout, bounded)
    bad = [(r["case"], r["fwd"][2], r["bwd"][2]) for r in rows if not (r["fwd"][2] <= 1e-6 and r["bwd"][2] <= 5e-5 * r["scale"][2] + 1e-7)]
    assert not bad, (V, layout, bad)


@pytest.mark.parametrize("V", [1, 25, 300])
@pytest.mark.parametrize("k", [1, 9, 10])
def test_training_statis_parity_at_small_sizes(k, V):
    """training_statis against training_statis_torch (rtol 1e-6, atol 1e-6), over three views, and statis_increments +
    statis_apply bit-equal to it; once more with the two per-candidate accumulators starting 4 bytes into an allocation
    (with k = 10 that sends the one-candidate kernels down the path for unaligned accumulators)."""
    from splatco_amd.stats import statis_apply, statis_increments, training_statis
    from torch_restatements import training_statis_torch
    N = V + 7
    for offset in (0, 1):
        acc0 = _statis_inputs(N, V, k, 7 * k + V)[0]

        def fresh():
            acc = [a.clone() for a in acc0]
            if offset:
                for i in (2, 3):
                    buf = torch.zeros(N * k + 1, device=DEV)
                    buf[1:] = acc0[i].view(-1)
                    acc[i] = buf[1:].view(N * k, 1)
                    assert acc[i].data_ptr() % 8 == 4 and acc[i].is_contiguous()
            return acc
        a1, a2, a3 = fresh(), [a.clone() for a in acc0], fresh()
        for view in range(3):
            _, vis, no, sel, upd, grad = _statis_inputs(N, V, k, 1000 * view + 7 * k + V)
            training_statis(*a1, k, grad, no, upd, sel, vis)
            training_statis_torch(*a2, k, grad, no, upd, sel, vis)
            statis_apply(*a3, k, vis.nonzero().squeeze(1), *statis_increments(k, grad, no, upd, sel))
        for name, x, y, z in zip(("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom"), a1, a2, a3):
            assert torch.allclose(x, y, rtol=1e-6, atol=1e-6), (name, k, V, offset, float((x - y).abs().max()))
            assert torch.equal(x, z), (name, k, V, offset)
