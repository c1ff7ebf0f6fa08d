"""The forward blend's per-pixel update runs under the live-lane mask (blend.hip masked_blend): lanes that take no part in
a splat -- not hit, finished, or finished by this very splat -- are not written.  What that has to keep:

  1. the stop lands on the right list entry wherever it falls in a pair, a group of four, a 64-entry chunk and the
     one-pair tail of a chunk;
  2. the SAFE instantiation (a colour that is not finite among the visible Gaussians) and the plain one give the same bits;
  3. lanes outside a ragged image stay out of the result;
  4. run to run the bits are the same.

No exp() threshold is involved where a comparison is exact: the Gaussians of such a pixel are centred exactly on the pixel
centre, where power is exactly 0, exp exactly 1 and alpha = min(0.99, opacity) on both sides.
"""
import math

import numpy as np
import pytest
import torch

from util import oracle_settings, small_scene
from splatco_amd.cameras import make_camera

pytestmark = pytest.mark.gpu

IMG_TOL = 1e-4        # the suite's image bar (max-abs against the fp32 oracle)
MARGIN = 1e-3         # test 3: a pixel is compared exactly when every decision it took lies this far (relative) from its threshold


def _dev():
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    return torch.device("cuda:0")


def _settings(cam, bg):
    from splatco_amd.rasterizer import GaussianRasterizationSettings
    d = _dev()
    return GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=torch.tensor(bg, dtype=torch.float32, device=d), scale_modifier=1.0,
        viewmatrix=cam.world_view_transform.to(d), projmatrix=cam.full_proj_transform.to(d), sh_degree=1,
        campos=cam.camera_center.to(d), prefiltered=False, debug=False)


def _t(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=_dev(), requires_grad=grad)


def _forward(cam, g):
    """One forward pass; (image, final_T, n_contrib, radii, per-instance quadrant masks, tile ranges, sorted ids) on the device."""
    from splatco_amd import rasterizer as R
    from splatco_amd import _C
    with torch.no_grad():
        color, radii, st = R.rasterize_forward(R._CSettings(_settings(cam, g["bg"])), _t(g["means3D"]), _t(g["opacities"]),
                                               _t(g["scales"]), _t(g["rotations"]), None, None, _t(g["colors"]))
        out = dict(color=color, radii=radii, final_T=st.debug(_C.DBG_FINAL_T).clone(), n_contrib=st.debug(_C.DBG_N_CONTRIB).clone(),
                   qmask=st.debug(_C.DBG_QMASK).clone(), ranges=st.debug(_C.DBG_RANGES).clone(),
                   point_list=st.debug(_C.DBG_POINT_LIST).clone())
    torch.cuda.synchronize()
    return out


def _oracle_forward(oracle, cam, g):
    return oracle.forward(oracle_settings(oracle, cam, g["bg"]), g["means3D"], g["opacities"], g["scales"], g["rotations"],
                          colors_precomp=g["colors"])


# ------------------------------------------------------------------ 1. stop position against list position
STACK = 16                 # opacity-0.5 Gaussians on the pixel: 13 contribute (0.5^13 * 0.5 < 1e-4 <= 0.5^13), the 14th is the stop
PIXEL = (16, 16)           # first pixel of quadrant 0 of tile (1, 1) of the 32x32 image
SIDE = (19, 19)            # another pixel of the same quadrant ("offset" fillers)
FRONT = (0, 1, 2, 3, 49, 50, 51, 52, 61, 62, 63, 64)


def stack_scene(m, filler):
    """STACK isotropic Gaussians of opacity 0.5 centred on PIXEL at increasing depth, m fillers in front of them that are in the
    tile's list and never reach alpha >= 1/255 at PIXEL:
      "faint"  : same centre, opacity 1/300.  (Their quadrant masks are empty -- no pixel can reach 1/255 -- so the waves skip
                 them while compacting the list: they move the stop through the LANES of the 64-entry chunks, not through
                 the staged pairs.)
      "offset" : opacity 0.8, a fraction of a pixel wide, centred on SIDE: staged by the wave of PIXEL, out of reach of PIXEL
                 itself (alpha there is below 1e-9) -- they move the stop through the staged pairs and groups, and the
                 pixels around SIDE finish on them, so the wave carries finished lanes while PIXEL is still live."""
    cam = make_camera(np.eye(3), np.zeros(3), math.pi / 2, math.pi / 2, 32, 32)
    n = m + STACK
    rng = np.random.default_rng(m)
    z = (3.0 + 0.02 * np.arange(n)).astype(np.float32)
    ndc = lambda p: np.float32((2 * p + 1) / 32.0 - 1.0)          # ((ndc + 1) * 32 - 1) / 2 = p
    cx = np.full(n, ndc(PIXEL[0]), np.float32)
    cy = np.full(n, ndc(PIXEL[1]), np.float32)
    op = np.full((n, 1), 0.5, np.float32)
    sc = np.full((n, 3), 0.25, np.float32)
    if filler == "faint":
        op[:m] = np.float32(1.0 / 300.0)
    else:
        cx[:m], cy[:m] = ndc(SIDE[0]), ndc(SIDE[1])
        op[:m] = 0.8
        sc[:m] = 0.02
    means = np.stack([cx * z, cy * z, z], 1).astype(np.float32)
    rot = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    g = dict(means3D=means, scales=sc, rotations=rot, opacities=op, colors=rng.uniform(0, 1, (n, 3)).astype(np.float32),
             bg=np.array([0.2, 0.5, 0.9], np.float32))
    return cam, g


@pytest.mark.parametrize("filler", ["faint", "offset"])
@pytest.mark.parametrize("m", FRONT)
def test_stop_position_against_list_position(oracle, m, filler):
    cam, g = stack_scene(m, filler)
    f = _oracle_forward(oracle, cam, g)
    x, y = PIXEL
    # what makes the comparison exact: every Gaussian of the stack sits exactly on the pixel centre, the stack is the tail
    # of the tile's list in depth order, and 13 of its members contribute
    assert np.array_equal(f["xy"][m:], np.tile(np.array([x, y], np.float32), (STACK, 1)))
    assert f["n_contrib"][y, x] == m + 13 and f["final_T"][y, x] == np.float32(0.5 ** 13)
    o = _forward(cam, g)
    lo, hi = (int(v) for v in o["ranges"][1 * 2 + 1])                 # tile (1, 1) of the 2 x 2 grid
    assert hi - lo == m + STACK and np.array_equal(o["point_list"][lo:hi].cpu().numpy(), np.arange(m + STACK))
    staged = (o["qmask"][lo:hi].cpu().numpy() & 1) != 0               # quadrant 0: the wave of PIXEL
    assert staged[m:].all()
    assert staged[:m].all() if filler == "offset" else not staged[:m].any()
    n_contrib, final_T = o["n_contrib"].cpu().numpy(), o["final_T"].cpu().numpy()
    print(f"[mask] m={m} {filler}: n_contrib {n_contrib[y, x]} (oracle {f['n_contrib'][y, x]}), final_T {final_T[y, x]!r}")
    assert n_contrib[y, x] == f["n_contrib"][y, x]
    assert final_T[y, x].tobytes() == np.float32(f["final_T"][y, x]).tobytes()
    assert np.abs(o["color"].cpu().numpy() - f["color"]).max() <= IMG_TOL


# ------------------------------------------------------------------ scene S
SEED, SPREAD = 13, 3.0     # chosen on the CPU with the oracle alone: at 40x24 99.3 % of the pixels keep every decision MARGIN away
                           # from its threshold (test 3 needs 99 %); spread 1.0 gives lists of 1500 entries per pixel and
                           # 96 - 98 % for every seed of 0..59, spread 3.0 lists of 370 and 98.9 - 99.3 % for the best seeds of 0..29


def scene_s(W=64, H=48, seed=SEED):
    """2000 Gaussians of small_scene, a fifth of the colour components negative, a fifth exactly zero, black background."""
    cam, g = small_scene(P=2000, W=W, H=H, seed=seed, spread=SPREAD)
    rng = np.random.default_rng(seed + 1000)
    kind = rng.random(g["colors"].shape)
    g["colors"][kind < 0.2] *= -1.0
    g["colors"][kind > 0.8] = 0.0
    g["bg"] = np.zeros(3, np.float32)
    return cam, g


# ------------------------------------------------------------------ 2. both instantiations give the same bits
def test_safe_and_plain_instantiations_give_the_same_bits():
    cam, g = scene_s()
    plain = _forward(cam, g)
    # one more Gaussian straight ahead of the camera, behind everything: visible, last in every list it is in (so no other
    # entry moves), too faint to contribute anywhere, with a NaN colour -- the library picks the SAFE kernels for the call
    wvt = cam.world_view_transform.numpy().astype(np.float64)
    eye = cam.camera_center.numpy().astype(np.float64)
    fwd = wvt[:3, 2] / np.linalg.norm(wvt[:3, 2])
    depth = g["means3D"].astype(np.float64) @ wvt[:3, 2] + wvt[3, 2]
    far = (eye + 50.0 * fwd).astype(np.float32)
    assert 50.0 > depth.max() + 1.0
    g2 = {k: v.copy() for k, v in g.items()}
    g2["means3D"] = np.concatenate([g["means3D"], far[None]])
    g2["scales"] = np.concatenate([g["scales"], np.full((1, 3), 0.3, np.float32)])
    g2["rotations"] = np.concatenate([g["rotations"], np.array([[1, 0, 0, 0]], np.float32)])
    g2["opacities"] = np.concatenate([g["opacities"], np.array([[1.0 / 300.0]], np.float32)])
    g2["colors"] = np.concatenate([g["colors"], np.array([[np.nan, 0.5, np.nan]], np.float32)])
    safe = _forward(cam, g2)
    assert int(safe["radii"][-1]) > 0, "the NaN-coloured Gaussian must be visible"
    assert torch.equal(safe["radii"][:-1], plain["radii"])
    assert not torch.isnan(safe["color"]).any()
    assert torch.equal(safe["color"], plain["color"])
    assert torch.equal(safe["final_T"], plain["final_T"])
    assert torch.equal(safe["n_contrib"], plain["n_contrib"])


# ------------------------------------------------------------------ 3. ragged image
def single_gaussian_16():
    cam, g = small_scene(P=1, W=16, H=16, seed=SEED)
    g["means3D"][:] = np.array([0.1, 0.05, 0.0], np.float32)      # the camera's target: the middle of the image
    g["scales"][:] = 0.3
    g["opacities"][:] = 0.7
    g["colors"][:] = np.array([0.9, -0.3, 0.0], np.float32)
    g["bg"] = np.zeros(3, np.float32)
    return cam, g


@pytest.mark.parametrize("scene", ["S_40x24", "single_16x16"])
def test_ragged_image(oracle, scene):
    cam, g = scene_s(40, 24) if scene == "S_40x24" else single_gaussian_16()
    f = _oracle_forward(oracle, cam, g)
    assert (f["radii"] > 0).any()
    o = _forward(cam, g)
    err = float(np.abs(o["color"].cpu().numpy() - f["color"]).max())
    # by the oracle's own numbers: every decision of the pixel (alpha against 1/255, T (1 - alpha) against 1e-4, for every
    # splat it evaluated) lies at least MARGIN, relative to the threshold, away from it
    clear = f["margin"] >= MARGIN
    same = o["n_contrib"].cpu().numpy().astype(np.int64) == f["n_contrib"].astype(np.int64)
    print(f"[mask] {scene}: image max-abs {err:.2e}, {clear.mean():.2%} of the pixels clear of every threshold, "
          f"n_contrib equal on {same.mean():.2%}")
    assert err <= IMG_TOL
    assert clear.mean() >= 0.99
    assert same[clear].all()


# ------------------------------------------------------------------ 4. run to run
def test_run_to_run_bits():
    from splatco_amd.rasterizer import GaussianRasterizer
    cam, g = scene_s()
    dL = _t(np.random.default_rng(1).standard_normal((3, cam.image_height, cam.image_width)).astype(np.float32))
    runs = []
    for _ in range(2):
        leaves = dict(means3D=_t(g["means3D"], True), opacities=_t(g["opacities"], True), colors_precomp=_t(g["colors"], True),
                      scales=_t(g["scales"], True), rotations=_t(g["rotations"], True))
        m2d = torch.zeros(len(g["means3D"]), 3, device=_dev(), requires_grad=True)
        img, _ = GaussianRasterizer(_settings(cam, g["bg"]))(means2D=m2d, **leaves)
        (img * dL).sum().backward()
        torch.cuda.synchronize()
        runs.append(dict(image=img.detach(), means2D=m2d.grad, **{k: v.grad for k, v in leaves.items()}))
    for k in runs[0]:
        assert runs[0][k] is not None and torch.equal(runs[0][k], runs[1][k]), k
