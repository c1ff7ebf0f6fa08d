"""Per-view bilateral grids (host side of csrc/bilagrid.hip): a remedy for training photographs that disagree photometrically.

Exposure, white balance and vignetting drift from view to view in every captured dataset, and a scene model that has to
explain the drift does so with floaters and view-dependent haze.  A bilateral grid ("Bilateral Guided Radiance Field
Processing"; gsplat's use_bilateral_grid) leaves the scene model alone: every TRAINING view owns a small learnable lattice
G[12, L, Gh, Gw] of 3x4 affine colour transforms, indexed by pixel position and luminance, that is applied to the RENDERED
image before the loss and dropped at test time.  The definition (normative; include/splatco_bilagrid.h and
tests/bilagrid_ref.py restate it), all float32:

  u = (px + 0.5) / W (Gw - 1),  v = (py + 0.5) / H (Gh - 1),  z = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1) (L - 1)
  A(px, py) = the trilinear interpolation of G at (z, v, u)  (grid_sample: align_corners=True, padding_mode="border")
  out = A[:, :3] rgb + A[:, 3]
  tv(grids) = (1 / N) sum over d in {L, Gh, Gw} of S_d / c_d,  S_d = the squared differences of neighbours along d over all
              views and channels, c_d = the number of such pairs in one view's grid

The grids start as the identity (A = [I | 0] at every vertex).  In a training step (train_step.collaborative_step,
`bilateral_grid=`) they get their data gradient from the views of the step and the total-variation gradient in closed form,
and an optimizer that holds them steps them:

    bil = BilateralGrid(len(train_views), device="cuda")
    opt = FusedAdam(model_groups + [{"params": [bil.grids], "lr": 2e-3, "name": "bilateral_grids"}], eps=1e-15)
    collaborative_step(pc, views, gts, pipe, bg, optimizer=opt, bilateral_grid=bil)

Every launch goes through _C.family_call.  There is no CPU path."""
import torch

from . import _C

CHANNELS = 12
LEVELS = (2, 16)            # supported L
VERTICES = (2, 64)          # supported Gh, Gw


def _check_lattice(fn, L, Gh, Gw):
    if not (LEVELS[0] <= L <= LEVELS[1] and VERTICES[0] <= Gh <= VERTICES[1] and VERTICES[0] <= Gw <= VERTICES[1]):
        raise ValueError(f"{fn}: (L, Gh, Gw) = {(L, Gh, Gw)} is outside L in {LEVELS}, Gh and Gw in {VERTICES}")


def _check_operands(fn, grid, image):
    """What is wrong with the tensors themselves first (that holds on any device), where they live last."""
    if grid.dtype != torch.float32 or image.dtype != torch.float32:
        raise ValueError(f"{fn}: expected a float32 grid and image, got {grid.dtype} and {image.dtype}")
    if grid.dim() != 4 or grid.shape[0] != CHANNELS:
        raise ValueError(f"{fn}: expected a [12, L, Gh, Gw] grid, got {tuple(grid.shape)}")
    _check_lattice(fn, *grid.shape[1:])
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"{fn}: expected a [3, H, W] image, got {tuple(image.shape)}")
    if image.shape[1] * image.shape[2] >= 2 ** 31:
        raise ValueError(f"{fn}: H W = {image.shape[1] * image.shape[2]} is not below 2^31")
    if not grid.is_cuda or not image.is_cuda:
        raise RuntimeError(f"{fn}: grid and image must live on the GPU (csrc/bilagrid.hip; there is no CPU path)")
    if image.device != grid.device:
        raise ValueError(f"{fn}: the image is on {image.device}, the grid on {grid.device}")


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, image):
        grid, image = grid.detach().contiguous(), image.detach().contiguous()
        _, L, Gh, Gw = grid.shape
        _, H, W = image.shape
        out = torch.empty_like(image)
        _C.family_call("scr_bilagrid_slice", grid, L, Gh, Gw, _C.ptr(image), H, W, _C.ptr(out), device=grid.device)
        ctx.save_for_backward(grid, image)
        return out

    @staticmethod
    def backward(ctx, g_out):
        grid, image = ctx.saved_tensors
        _, L, Gh, Gw = grid.shape
        _, H, W = image.shape
        want_grid, want_image = ctx.needs_input_grad
        g_out = g_out.contiguous().float()
        d_grid = torch.empty_like(grid) if want_grid else None
        d_image = torch.empty_like(image) if want_image else None
        if H * W == 0:
            return (None if d_grid is None else d_grid.zero_()), d_image
        nbytes = _C.lib.scr_bilagrid_scratch_bytes(L, Gh, Gw, H, W) if want_grid else 0
        scratch = _C.scratch(nbytes, grid.device) if want_grid else None
        _C.family_call("scr_bilagrid_slice_backward", grid, L, Gh, Gw, image, g_out, H, W, d_image, d_grid, scratch, nbytes,
                       device=grid.device)
        return d_grid, d_image


def slice_apply(grid, image):
    """The bare operator: `image` [3, H, W] corrected by `grid` [12, L, Gh, Gw]; gradients flow to both."""
    _check_operands("slice_apply", grid, image)
    return _Slice.apply(grid, image)


def tv_add_grad(grids, weight):
    """Adds d/dgrids of weight * tv(grids) into grids.grad (allocated as zeros where there is none) in closed form: no
    autograd graph, no loss value.  grids: [N, 12, L, Gh, Gw]."""
    if not grids.is_cuda:
        raise RuntimeError("tv_add_grad: the grids must live on the GPU (csrc/bilagrid.hip; there is no CPU path)")
    if grids.dtype != torch.float32 or grids.dim() != 5 or grids.shape[1] != CHANNELS or not grids.is_contiguous():
        raise ValueError(f"tv_add_grad: expected contiguous float32 [N, 12, L, Gh, Gw] grids, got {grids.dtype} {tuple(grids.shape)}")
    N, _, L, Gh, Gw = grids.shape
    _check_lattice("tv_add_grad", L, Gh, Gw)
    if grids.grad is None:
        grids.grad = torch.zeros_like(grids)
    g = grids.grad
    if g.dtype != torch.float32 or g.shape != grids.shape or not g.is_contiguous() or g.device != grids.device:
        raise ValueError("tv_add_grad: grids.grad must be a contiguous float32 tensor of the grids' shape on their device")
    if N == 0:
        return
    _C.family_call("scr_bilagrid_tv_add_grad", grids.detach(), g, N, L, Gh, Gw, float(weight) / N, device=grids.device)


class BilateralGrid(torch.nn.Module):
    """One grid per training view: `grids` [num_views, 12, grid_w, grid_y, grid_x] (grid_w luminance levels), the identity at
    the start.  `bil(image, view_index)` is the corrected image of that view.  Test views have no grid: evaluate on the
    uncorrected render."""

    def __init__(self, num_views, grid_x=16, grid_y=16, grid_w=8, device="cuda"):
        super().__init__()
        num_views, L, Gh, Gw = int(num_views), int(grid_w), int(grid_y), int(grid_x)
        if num_views < 1:
            raise ValueError(f"BilateralGrid: num_views = {num_views}")
        _check_lattice("BilateralGrid", L, Gh, Gw)
        identity = torch.eye(3, 4, dtype=torch.float32, device=device).reshape(1, CHANNELS, 1, 1, 1)
        self.grids = torch.nn.Parameter(identity.repeat(num_views, 1, L, Gh, Gw).contiguous())

    @property
    def num_views(self):
        return self.grids.shape[0]

    def forward(self, image, view_index):
        view_index = int(view_index)
        if not 0 <= view_index < self.grids.shape[0]:
            raise IndexError(f"BilateralGrid: view index {view_index} is outside 0 .. {self.grids.shape[0] - 1}")
        return slice_apply(self.grids[view_index], image)

    def tv_add_grad(self, weight):
        tv_add_grad(self.grids, weight)
