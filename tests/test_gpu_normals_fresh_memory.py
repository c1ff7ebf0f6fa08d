"""The normals family on the poison ladder (tests/poison.py): no result of depth_normals, normal_loss, their backward passes or
the training step's normal term may depend on what its uninitialised buffers held -- the scratch of the loss records, the
(L, n_valid) pair, the normal map and both gradient maps are all torch.empty.  Each case runs unpatched, then with every such
buffer pre-filled with zero bytes, int64 ones and 0xFF bytes (NaN / -1), in that order, and every run must give the bits of
the zero-filled one.  52 x 70: two tiles across, seven down, the last of each partly filled, guarded dword accesses."""
import math
import types

import pytest
import torch

import normals_ref as ref
import poison
import splatco_amd.normals                    # noqa: F401  (the module under test: without it nothing here can run)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W = 52, 70


def _check(fn):
    rep = poison.check(fn, sync=torch.cuda.synchronize)
    for pattern in poison.PATTERNS:
        assert rep[pattern].bytes > 0 and rep[pattern].count > 0, pattern
    return rep


def _camera():
    from splatco_amd.cameras import look_at_camera
    return look_at_camera(eye=(0.3, -0.2, 0.1), target=(1.0, 0.7, -0.4), up=(0, -1, 0), FoVx=math.radians(60), width=W, height=H).to(
        torch.device(DEV))


@pytest.mark.parametrize("frame", ("camera", "world"))
def test_normal_map_and_its_backward(frame):
    from splatco_amd.normals import depth_normals
    D, A, _, _, _ = ref.recipe(H, W, 1, device=DEV)
    cam = _camera()
    G = torch.randn(3, H, W, generator=torch.Generator().manual_seed(2)).to(DEV)

    def fn():
        D_, A_ = D.clone().requires_grad_(), A.clone().requires_grad_()
        n, valid = depth_normals(D_, A_, cam, frame=frame, return_valid=True)
        (n * G).sum().backward()
        only = A.clone().requires_grad_()
        (depth_normals(D, only, cam, frame=frame) * G).sum().backward()         # one map only: the other pointer is NULL
        return [n, valid, D_.grad, A_.grad, only.grad]

    p = _check(fn)["nan"]
    assert p.bytes > 0


@pytest.mark.parametrize("mk", (None, "f32", "u8", "bool"))
def test_normal_loss_and_its_backward(mk):
    from splatco_amd.normals import normal_loss
    D, A, prior, mask, intr = ref.recipe(H, W, 1, device=DEV, mask_kind=mk)

    def fn():
        D_, A_ = D.clone().requires_grad_(), A.clone().requires_grad_()
        loss, stats = normal_loss(D_, A_, prior, intr, mask, return_stats=True)
        (loss * 1.5).backward()
        only = D.clone().requires_grad_()
        normal_loss(only, A, prior, intr, mask).backward()                        # one map only: the other pointer is NULL
        return [loss, stats, D_.grad, A_.grad, only.grad]

    p = _check(fn)["nan"]
    assert p.bytes > 0


def test_training_step_with_a_normal_term():
    """One collaborative_step on a 70 x 52 view with normal_weight > 0, the model rebuilt from the same seed in every run."""
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.synthetic import synthetic_anchor_model
    from splatco_amd.train_step import collaborative_step
    cams = [look_at_camera(eye=(0.3, -0.2, -6.0), target=(0, 0, 0), up=(0, -1, 0), FoVx=math.radians(60), width=W, height=H).to(DEV)]
    gts = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(4)).to(DEV)]
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    bg = torch.ones(3, device=DEV)
    targets = [torch.tensor([0.3, 0.2, -0.5]).reshape(3, 1, 1).expand(3, H, W).contiguous()]
    seen = {}

    def fn():
        torch.manual_seed(11)
        pc = synthetic_anchor_model(3000, 9, DEV, plane_size=64)
        loss, out, _ = collaborative_step(pc, cams, gts, pipe, bg, normal_targets=targets, normal_weight=0.5,
                                          normal_options=dict(min_alpha=0.2))
        seen["alpha"] = out["alpha"].detach()
        return [loss, out["render"], out["depth"], out["alpha"]] + [p.grad for p in pc.parameters() if p.grad is not None]

    p = _check(fn)["nan"]
    assert p.bytes > 0
    assert int((seen["alpha"] >= 0.2).sum()) >= 64, "the view shows too little of the model for the normal term to act"
