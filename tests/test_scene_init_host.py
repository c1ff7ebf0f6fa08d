"""CPU tests of splatco_amd.scene_init (voxelize, dist2, create_from_pcd): the plain torch branch against the reference's
own voxelize_sample / create_from_pcd output (tests/golden/scene_init.npz, tools/make_golden_scene_init.py) and against
the float64 brute force stored there.  The device branch is compared bit for bit with this one in
tests/test_gpu_scene_init.py.

Bound of dist2 against float64, derived: one rounding in each difference (3 u after squaring), two in the sum of squares,
two in the sum of three, one in the division -- 8 u, u = 2^-24."""
import os

import numpy as np
import pytest
import torch

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_init.npz"))
U = 2.0 ** -24
DIST2_BOUND = 8 * U


def _points():
    return torch.tensor(GOLDEN["points"])


def _reference_expression(p, v):
    return np.unique(np.round(p / np.float32(v)), axis=0) * np.float32(v)


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(got[want == 0], want[want == 0])
    return float((np.abs(got - want)[want > 0] / want[want > 0]).max())


@pytest.mark.parametrize("i", range(2))
def test_voxelize_equals_the_reference_rows_in_order(i):
    from splatco_amd.scene_init import voxelize
    v = float(GOLDEN["voxel_sizes"][i])
    got = voxelize(_points(), v)
    want = GOLDEN[f"vox{i}"]
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.numpy(), want)
    assert np.array_equal(voxelize(_points().double(), v).numpy(), want)       # float64 input is converted first


def test_fixture_has_the_cases_it_promises():
    p = GOLDEN["points"]
    assert p.dtype == np.float32 and (p < 0).any() and len(np.unique(p, axis=0)) < len(p)
    for v in GOLDEN["voxel_sizes"]:
        t = p / np.float32(v)
        half = t - np.floor(t) == 0.5
        k = np.floor(t[half])
        assert (k % 2 == 0).any() and (k % 2 == 1).any(), "half-way cases with even and odd floor"


def test_dist2_against_float64():
    from splatco_amd.scene_init import dist2
    a = torch.tensor(GOLDEN["_anchor"])
    got = dist2(a)
    assert got.dtype == torch.float32 and got.shape == (a.shape[0],)
    rel = _rel(got.numpy(), GOLDEN["dist2_f64"])
    print(f"dist2 vs float64 on the anchors: max relative error {rel:.3e} = {rel / U:.2f} u")
    assert rel <= DIST2_BOUND
    # the raw cloud has exact duplicates: a duplicate is another point at distance 0
    p = _points()
    d = dist2(p)
    brute = ((p.double()[None] - p.double()[:, None]) ** 2).sum(-1)
    brute.fill_diagonal_(float("inf"))
    want = brute.topk(3, dim=1, largest=False).values.sum(1) / 3.0
    assert (brute.min(dim=1).values == 0).any()
    assert _rel(d.numpy(), want.numpy()) <= DIST2_BOUND


def test_create_from_pcd_reproduces_the_fixture():
    from splatco_amd.scene_init import create_from_pcd, dist2
    from splatco_amd.scene_model import AnchorGaussianModel
    pc = AnchorGaussianModel(plane_size=8, num_channels=15)
    v = float(GOLDEN["voxel_sizes"][0])
    used, n_points, n_anchors = create_from_pcd(pc, GOLDEN["points"], v)
    assert used == v and pc.voxel_size == v and n_points == len(GOLDEN["points"]) and n_anchors == len(GOLDEN["_anchor"])
    assert np.array_equal(pc._anchor.detach().numpy(), GOLDEN["_anchor"])
    own = torch.log(torch.sqrt(torch.clamp_min(dist2(pc._anchor.detach()), 1e-7)))[:, None].repeat(1, 6)
    assert torch.equal(pc._scaling.detach(), own)
    # the bound of dist2 through log(sqrt(.)): half of 8 u absolute, one rounding of sqrt (u relative, u in the
    # logarithm) and one of the logarithm (u of its value)
    want = GOLDEN["_scaling"].astype(np.float64)
    err = np.abs(pc._scaling.detach().numpy().astype(np.float64) - want)
    tol = 0.5 * DIST2_BOUND + U + U * np.abs(want)
    print(f"_scaling vs fixture: max |d| {err.max():.3e}, max d / tol {float((err / tol).max()):.3f}")
    assert (err <= tol).all()
    assert np.array_equal(pc._rotation.numpy(), GOLDEN["_rotation"]) and np.array_equal(pc._opacity.numpy(), GOLDEN["_opacity"])
    assert pc._offset.shape == (n_anchors, pc.n_offsets, 3) and not pc._offset.any()
    assert pc._anchor_feat.shape == (n_anchors, pc.feat_dim) and not pc._anchor_feat.any()
    assert pc._scaling.shape == (n_anchors, 6) and pc._rotation.shape == (n_anchors, 4) and pc._opacity.shape == (n_anchors, 1)
    assert [getattr(pc, n).requires_grad for n in ("_anchor", "_offset", "_anchor_feat", "_scaling", "_rotation", "_opacity")] == \
        [True, True, True, True, False, False]
    assert all(getattr(pc, n).dtype == torch.float32 for n in ("_anchor", "_offset", "_anchor_feat", "_scaling"))

    # voxel_size <= 0: the kthvalue of the raw cloud's dist2 (a squared distance used as a length)
    used, n_points, _ = create_from_pcd(pc, GOLDEN["points"], 0)
    want = float(GOLDEN["auto_voxel_size"])
    print(f"auto voxel size {used!r} vs fixture {want!r}: relative {abs(used - want) / want:.3e}")
    assert abs(used - want) <= DIST2_BOUND * want and pc.voxel_size == used
    assert np.array_equal(pc._anchor.detach().numpy(), _reference_expression(GOLDEN["points"], used))
    # ratio: points[::ratio]
    _, n_points, _ = create_from_pcd(pc, GOLDEN["points"], v, ratio=3)
    assert n_points == len(GOLDEN["points"][::3])
    assert np.array_equal(pc._anchor.detach().numpy(), _reference_expression(GOLDEN["points"][::3], v))


def test_bad_input_raises():
    from splatco_amd.scene_init import dist2, voxelize
    p = _points()
    with pytest.raises(ValueError):
        dist2(p[:3])
    bad = p.clone()
    bad[17, 1] = float("nan")
    with pytest.raises(ValueError):
        dist2(bad)
    with pytest.raises(ValueError):
        voxelize(bad, 0.05)
    bad[17, 1] = float("inf")
    with pytest.raises(ValueError):
        voxelize(bad, 0.05)
    with pytest.raises(ValueError):
        voxelize(p * 1000, 1e-7)            # |rint(x / v)| ~ 2e10 does not fit int32
    with pytest.raises(ValueError):
        voxelize(p, 0.0)
    with pytest.raises(ValueError):
        voxelize(p[:, :2], 0.05)


def test_wide_extent_fallback():
    from splatco_amd.scene_init import voxelize
    p = _points()
    for v in (0.05, 0.01):
        assert torch.equal(voxelize(p, v, _force_rows=True), voxelize(p, v))
    # two clusters 3000 units apart at v = 0.001: 3e6 > 2^21 voxels along x, the packed key cannot hold it
    g = torch.Generator().manual_seed(5)
    a = torch.randn(3000, 3, generator=g) * 0.02
    wide = torch.cat([a + torch.tensor([-1500.0, 0.3, -0.2]), a.flip(0) + torch.tensor([1500.0, -0.1, 0.4]), a[:200] + torch.tensor([-1500.0, 0.3, -0.2])])
    got = voxelize(wide, 0.001)
    want = _reference_expression(wide.numpy(), 0.001)
    assert 0 < len(want) < len(wide) and np.array_equal(got.numpy(), want)


def test_simple_knn_drop_in():
    from simple_knn._C import distCUDA2
    from splatco_amd.scene_init import dist2
    a = torch.tensor(GOLDEN["_anchor"][:500])
    assert torch.equal(distCUDA2(a), dist2(a))
