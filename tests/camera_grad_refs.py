"""Reference side of the camera-gradient tests (test_gpu_camera_grad.py, test_camera_grad_host.py): the scenes, the fixed
dL/dimage and oracle/torch_ref.py::rasterize differentiated in the camera on the CPU.

viewmatrix, projmatrix and campos are leaves that require grad; the loss is <G, image> with a seeded G.  A gradient autograd
returns as None (campos with colors_precomp) counts as zeros.  Results are cached per case: the float64 run of a case is
computed once per process and shared, never modified.
"""
import functools
import math

import numpy as np
import torch

from oracle import torch_ref
from util import rel_l2, small_scene

NAMES = ("viewmatrix", "projmatrix", "campos")
GRAD_TOL = 1e-4            # the project's gradient bar against its oracle (test_gpu_parity.py)
EDGE_P = (1, 255, 256, 257, 700)


def weights(cam, seed=11):
    """Fixed random dL/dimage, dL/ddepth, dL/dalpha (test_gpu_aux_maps.py::_weights, on the CPU)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    H, W = cam.image_height, cam.image_width
    return torch.randn(3, H, W, generator=gen), torch.randn(H, W, generator=gen), torch.randn(H, W, generator=gen)


def sh_coefficients(P, seed=5):
    """Degree-3 SH coefficients [P, 16, 3], seeded normal, sigma 0.4."""
    return (np.random.default_rng(seed).standard_normal((P, 16, 3)) * 0.4).astype(np.float32)


def cov3d(g):
    """Sigma = (R S)(R S)^T as the operator forms it (quaternions as given), upper triangle."""
    q, s = g["rotations"].astype(np.float64), g["scales"].astype(np.float64)
    r, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    L = R * s[:, None, :]
    S = L @ L.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)


def case(name):
    """(cam, g, extra) of a named case; extra: dict(shs=..., cov=..., sh_degree=...) for the other input forms."""
    if name == "base":
        return (*small_scene(), {})
    if name.startswith("P="):
        return (*small_scene(P=int(name[2:])), {})
    if name == "clamped":
        return (*small_scene(P=300, spread=2.0), {})
    if name == "subset160":
        return (*small_scene(P=160), {})
    if name == "recovery":
        return (*small_scene(P=300), {})
    if name in ("shs", "shs_cov3D", "cov3D"):
        cam, g = small_scene()
        extra = {}
        if name != "cov3D":
            extra.update(shs=sh_coefficients(g["means3D"].shape[0]), sh_degree=3)
        if name != "shs":
            extra.update(cov=cov3d(g))
        return cam, g, extra
    raise KeyError(name)


def torch_ref_run(cam, g, G, dtype, shs=None, cov=None, sh_degree=1, camera=None):
    """oracle/torch_ref.py::rasterize in `dtype` with the camera tensors as leaves.  camera: (V, M, campos) to use instead
    of the camera's own (for the pose tests).  Returns dict(image, radii, viewmatrix, projmatrix, campos [gradients])."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    V, M, C = (x.detach().to(dtype).clone().requires_grad_() for x in
               (camera or (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)))
    kw = dict(means3D=t(g["means3D"]), opacities=t(g["opacities"]))
    if cov is None:
        kw.update(scales=t(g["scales"]), rotations=t(g["rotations"]))
    else:
        kw.update(cov3D_precomp=t(cov))
    kw.update(shs=t(shs)) if shs is not None else kw.update(colors_precomp=t(g["colors"]))
    img, radii, _ = torch_ref.rasterize(cam.image_height, cam.image_width, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5),
                                        t(g["bg"]), 1.0, V, M, sh_degree, C, **kw)
    grads = torch.autograd.grad((img * G.to(dtype)).sum(), (V, M, C), allow_unused=True)
    out = dict(image=img.detach(), radii=radii)
    for n, x, gr in zip(NAMES, (V, M, C), grads):
        out[n] = torch.zeros_like(x) if gr is None else gr
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 result, float32 result, e32 per camera tensor) of a named case.  e32: rel-L2 of the float32 torch_ref's
    gradient against the float64 one (0 where both are exactly zero)."""
    cam, g, extra = case(name)
    G = weights(cam)[0]
    r64, r32 = torch_ref_run(cam, g, G, torch.float64, **extra), torch_ref_run(cam, g, G, torch.float32, **extra)
    e32 = {n: (0.0 if not r64[n].any() and not r32[n].any() else rel_l2(r32[n].numpy(), r64[n].numpy())) for n in NAMES}
    return r64, r32, e32


def bar(e32):
    return max(GRAD_TOL, 1.5 * e32)


def clamped_and_visible(cam, g, radii):
    """Number of visible Gaussians whose t.x / t.z or t.y / t.z lies outside 1.3 tan(fov / 2): the clamped Jacobians."""
    V = cam.world_view_transform.numpy().astype(np.float64)
    t = np.concatenate([g["means3D"].astype(np.float64), np.ones((g["means3D"].shape[0], 1))], 1) @ V
    limx, limy = 1.3 * math.tan(cam.FoVx * 0.5), 1.3 * math.tan(cam.FoVy * 0.5)
    cl = (np.abs(t[:, 0] / t[:, 2]) > limx) | (np.abs(t[:, 1] / t[:, 2]) > limy)
    return int((cl & (np.asarray(radii) > 0)).sum())


def scattered_scene(P=70000, n=160, seed=17):
    """Case 4: the n Gaussians of small_scene(P=n) at seeded random rows (0 and P - 1 among them, ascending: the subset
    keeps its index order) of a set of P; every other Gaussian lies behind the camera and is culled.  Returns
    (cam, g of the P, rows [n])."""
    cam, sub = small_scene(P=n)
    rng = np.random.default_rng(seed)
    rows = np.sort(np.concatenate([[0, P - 1], rng.choice(np.arange(1, P - 1), n - 2, replace=False)]))
    f = np.float32
    q = rng.standard_normal((P, 4))
    g = dict(means3D=(rng.uniform(-1, 1, (P, 3)) + np.array([0.6, -0.4, -9.0])).astype(f),
             scales=np.exp(rng.uniform(math.log(0.03), math.log(0.35), (P, 3))).astype(f),
             rotations=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f),
             opacities=rng.uniform(0.05, 0.95, (P, 1)).astype(f), colors=rng.uniform(0, 1, (P, 3)).astype(f), bg=sub["bg"])
    for k in ("means3D", "scales", "rotations", "opacities", "colors"):
        g[k][rows] = sub[k]
    return cam, g, rows
