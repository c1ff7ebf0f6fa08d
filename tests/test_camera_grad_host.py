"""Host-side checks of the camera gradients (no GPU): the C-ABI additions, cameras.pose_delta_camera, and the reference-side
conditions test_gpu_camera_grad.py relies on -- asserted here so that a later change of small_scene() cannot hollow those tests.
"""
import numpy as np
import pytest
import torch

import camera_grad_refs as R
from util import rel_l2, small_scene


def test_abi_has_the_camera_entry_points():
    from splatco_amd import _C
    assert _C.ABI_VERSION >= 34 and _C.lib.scr_abi_version() == _C.ABI_VERSION
    for name in ("scr_backward", "scr_backward_scratch_bytes"):      # the camera outputs and the `camera` flag are theirs
        assert name in _C.SYMBOLS and hasattr(_C.lib, name), name
    size = _C.lib.scr_backward_scratch_bytes
    # the records, the depth sums and one 128-byte row per 256 Gaussians, each part 256-byte aligned
    base = size(1000, 0, 1, 0)
    assert size(1000, 1, 0, 1) == size(1000, 1, 1, 1) == base + 256      # the depth sums are reserved whatever `maps` says
    assert size(1000, 70000, 0, 1) == size(1000, 70000, 1, 1) == base + 274 * 128
    assert size(0, 0, 0, 1) >= size(0, 0, 1, 0) + 128


def test_pose_delta_camera_at_zero_is_the_camera():
    from splatco_amd.cameras import pose_delta_camera
    cam, _ = small_scene()
    c = pose_delta_camera(cam, torch.zeros(6))
    assert torch.equal(c.world_view_transform, cam.world_view_transform)
    assert float((c.full_proj_transform - cam.full_proj_transform).abs().max()) <= 1e-6
    assert float((c.camera_center - cam.camera_center).abs().max()) <= 1e-6
    assert (c.image_width, c.image_height, c.FoVx, c.FoVy, c.znear, c.zfar) == (
        cam.image_width, cam.image_height, cam.FoVx, cam.FoVy, cam.znear, cam.zfar)
    assert all(t.dtype == torch.float32 for t in (c.world_view_transform, c.full_proj_transform, c.camera_center))


def test_pose_delta_camera_jacobian():
    """The autograd Jacobian of the three tensors at a seeded xi against a float64 central difference of the same function."""
    from splatco_amd.cameras import pose_delta_camera, pose_tensors
    cam, _ = small_scene()
    gen = torch.Generator(device="cpu").manual_seed(3)
    xi = (torch.rand(6, generator=gen) - 0.5) * 0.2
    outs = lambda c: (c.world_view_transform, c.full_proj_transform, c.camera_center)
    jac = torch.autograd.functional.jacobian(lambda x: tuple(t.reshape(-1) for t in outs(pose_delta_camera(cam, x))), xi)
    h = 1e-6
    cols = []
    for k in range(6):
        e = torch.zeros(6, dtype=torch.float64)
        e[k] = h
        hi, lo = pose_tensors(cam, xi.double() + e, torch.float64), pose_tensors(cam, xi.double() - e, torch.float64)
        cols.append([(a - b).reshape(-1) / (2 * h) for a, b in zip(hi, lo)])
    for i, name in enumerate(("world_view_transform", "full_proj_transform", "camera_center")):
        want = torch.stack([c[i] for c in cols], dim=1)
        err = rel_l2(jac[i].numpy(), want.numpy())
        print(f"[camera] d {name} / d xi: rel-L2 autograd (float32) vs central difference (float64) {err:.2e}")
        assert jac[i].shape == want.shape and float(want.abs().max()) > 0
        assert err <= 1e-6, (name, err)


CASES = ["base", "clamped", "shs", "shs_cov3D", "cov3D"] + [f"P={p}" for p in R.EDGE_P]


@pytest.mark.parametrize("name", CASES)
def test_reference_conditions(name):
    """float32 and float64 torch_ref agree on the radii and to e32 <= 1e-5 on every camera gradient; the gradients are dense
    but for the columns the forward never reads; campos gets a gradient exactly when the colours are SH."""
    r64, r32, e32 = R.reference(name)
    print(f"[camera] {name}: e32 " + ", ".join(f"{n} {e:.2e}" for n, e in e32.items()))
    assert torch.equal(r64["radii"], r32["radii"]) and int((r64["radii"] > 0).sum()) > 0
    assert all(e <= 1e-5 for e in e32.values()), e32
    V, M, C = (r64[n] for n in R.NAMES)
    assert torch.all(V[:, 3] == 0) and torch.all(M[:, 2] == 0)
    assert int((V[:, :3] != 0).sum()) == 12 and int((M[:, [0, 1, 3]] != 0).sum()) == 12
    assert bool(C.any()) == name.startswith("shs")


def test_clamped_scene_has_clamped_jacobians():
    cam, g, _ = R.case("clamped")
    radii = R.reference("clamped")[0]["radii"].numpy()
    n = R.clamped_and_visible(cam, g, radii)
    print(f"[camera] clamped scene: {int((radii > 0).sum())} visible, {n} of them with a clamped Jacobian")
    assert n >= 10


def test_culled_gaussians_change_nothing():
    """What case 4 of the GPU tests relies on: the gradients of a set with culled Gaussians in between are those of its
    visible subset (a small instance of scattered_scene: 160 among 400)."""
    cam, g, rows = R.scattered_scene(P=400)
    assert rows[0] == 0 and rows[-1] == 399 and np.all(np.diff(rows) > 0)
    full = R.torch_ref_run(cam, g, R.weights(cam)[0], torch.float64)
    radii = full["radii"].numpy()
    culled = np.ones(400, bool)
    culled[rows] = False
    assert not radii[culled].any() and np.array_equal(radii[rows], R.reference("subset160")[0]["radii"].numpy())
    for n in ("viewmatrix", "projmatrix"):
        err = rel_l2(full[n].numpy(), R.reference("subset160")[0][n].numpy())
        print(f"[camera] full set vs visible subset, {n}: {err:.2e}")
        assert err <= 1e-12
