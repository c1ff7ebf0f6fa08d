"""Host side of the rasterizer operator: the reference's `diff_gaussian_rasterization` API
(GaussianRasterizationSettings / GaussianRasterizer, imported at gaussian_renderer/__init__.py:15)
over the C-ABI of include/splatco_raster.h.

Autograd contract: differentiable w.r.t. means3D, colors_precomp | shs, opacities,
scales + rotations | cov3D_precomp; `means2D` receives the NDC-space mean gradient although its
value is unused (read back through .grad at scene/gaussian_model.py:779); radii is int32 and
non-differentiable.  Saved state is per call, so the mv live graphs of train.py:171-240 coexist.
With return_aux=True the same pass also returns the depth map sum_i w_i z_i and the accumulated opacity sum_i w_i
(w_i = alpha_i T_i, z_i the view-space depth; background excluded, depth not normalised), both differentiable.
The camera is differentiable too: when raster_settings.viewmatrix, .projmatrix or .campos requires grad (and gradient mode is
on) the backward also returns dL/dviewmatrix, dL/dprojmatrix [4, 4] and dL/dcampos [3] (scr_backward's camera outputs), each in the
shape of the tensor given and only for those that require grad.  The two matrices are independent inputs, as the kernels
read them: a full projection built in torch from the view matrix gets the composed gradient from autograd.  Columns the
forward never reads (viewmatrix[:, 3], projmatrix[:, 2]) get exact zeros, campos gets zeros with colors_precomp.  tanfovx /
tanfovy stay Python floats.  Without such a tensor nothing changes: the same kernels and bits.
With antialiased=True (upstream 3DGS `antialiasing`, gsplat rasterize_mode="antialiased") every splat's opacity is multiplied
by h = sqrt(max(0.000025, det(Sigma2D) / det(Sigma2D + 0.3 I))), which keeps its integrated opacity independent of the
0.3 px^2 dilation; h is differentiated with respect to the means, the covariance inputs and the view matrix.  Radii, tile
rects and the sort do not depend on the mode; the default (False) is the same kernels and bits as before.
PyTorch is used for device memory and streams only.
"""
from typing import NamedTuple

import ctypes as C
import os

import torch
import torch.nn as nn

from . import _C


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _dev_f32(t, name):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a device tensor (the rasterizer has no CPU path)")
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.contiguous().float()
    return t


class _CSettings:
    """Keeps the device tensors alive next to the C struct that points at them."""

    def __init__(self, rs: GaussianRasterizationSettings):
        self.bg = _dev_f32(rs.bg, "bg")
        self.view = _dev_f32(rs.viewmatrix, "viewmatrix")
        self.proj = _dev_f32(rs.projmatrix, "projmatrix")
        self.campos = _dev_f32(rs.campos, "campos")
        s = _C.Settings()
        s.image_height, s.image_width = int(rs.image_height), int(rs.image_width)
        s.tanfovx, s.tanfovy = float(rs.tanfovx), float(rs.tanfovy)
        s.bg, s.viewmatrix, s.projmatrix, s.campos = (self.bg.data_ptr(), self.view.data_ptr(),
                                                      self.proj.data_ptr(), self.campos.data_ptr())
        s.scale_modifier = float(rs.scale_modifier)
        s.sh_degree = int(rs.sh_degree)
        s.prefiltered, s.debug = int(bool(rs.prefiltered)), int(bool(rs.debug))
        self.c = s
        self.H, self.W = s.image_height, s.image_width

    def ref(self):
        return C.byref(self.c)


class RasterState:
    """Per-call saved buffers (opaque to Python) + what the debug getters need."""
    __slots__ = ("P", "M", "I", "max_tile", "flags", "cs", "geom", "binning", "image", "radii", "aux")

    def debug(self, which):
        """Integer / float intermediates for the parity tests (SCR_DBG_* selectors)."""
        dev = self.geom.device
        tiles = ((self.cs.W + 15) // 16) * ((self.cs.H + 15) // 16)
        shapes = {
            _C.DBG_TILES_TOUCHED: ((self.P,), torch.int32), _C.DBG_POINT_OFFSETS: ((self.P,), torch.int32),
            _C.DBG_RANGES: ((tiles, 2), torch.int32), _C.DBG_POINT_LIST: ((self.I,), torch.int32),
            _C.DBG_N_CONTRIB: ((self.cs.H, self.cs.W), torch.int32),
            _C.DBG_FINAL_T: ((self.cs.H, self.cs.W), torch.float32),
            _C.DBG_SPLAT_RECORDS: ((self.P, 12), torch.float32),
            _C.DBG_QMASK: ((self.I,), torch.uint8), _C.DBG_GM_INDEX: ((self.I,), torch.int32),
        }
        shape, dt = shapes[which]
        out = torch.empty(shape, dtype=dt, device=dev)
        if out.numel():
            _C.call("scr_debug_get", which, self.P, self.I, self.cs.H, self.cs.W, _C.ptr(self.geom), _C.ptr(self.binning),
                    _C.ptr(self.image), out)
        return out


SPECULATE = os.environ.get("SPLATCO_SPECULATIVE_BINNING", "1") != "0"
_plan_guess = {}           # (device, H, W) -> (P, instances, largest tile) of the last forward at that resolution: sizes the speculative binning buffer


def rasterize_forward(cs, means3D, opacities, scales, rotations, cov3D_precomp, shs, colors_precomp, aux=False,
                      antialiased=False):
    """plan + run through the C-ABI.  Returns (color, radii, RasterState).  aux: the blend also writes the depth and
    opacity maps, two [H, W] tensors left in RasterState.aux for the caller to take.  antialiased: the opacity compensation
    (SCR_MODE_ANTIALIASED); RasterState.flags then carries PLAN_ANTIALIASED to the backward."""
    dev = means3D.device
    P = means3D.shape[0]
    M = 0 if shs is None else shs.shape[1]
    st = RasterState()
    st.P, st.M, st.cs = P, M, cs
    st.geom = _C.scratch(_C.lib.scr_geom_bytes(P, cs.H, cs.W), dev)
    st.image = _C.scratch(_C.lib.scr_image_bytes(cs.H, cs.W), dev)
    radii = torch.empty(P, dtype=torch.int32, device=dev)      # every entry is written by preprocess_kernel
    color = torch.empty(3, cs.H, cs.W, dtype=torch.float32, device=dev)
    st.aux = None
    if aux:
        st.aux = (torch.empty(cs.H, cs.W, dtype=torch.float32, device=dev), torch.empty(cs.H, cs.W, dtype=torch.float32, device=dev))
    maps = st.aux or (None, None)
    mode = _C.MODE_ANTIALIASED if antialiased else 0
    plan = (C.c_int64 * 4)(0, 0, 0, 0)   # (tile instances, largest per-tile instance count, phase 2 already ran, plan flags)
    # The binning buffer's size is only known after the plan phase.  A guess from the previous call of this size (the
    # instance count of a training loop moves by a few per cent per step) lets both phases go out in ONE call: the GPU
    # does not wait for this thread's allocation and second call in the middle of every forward pass.
    key = (dev.index, cs.H, cs.W)
    guess = _plan_guess.get(key)      # (P, instances, largest tile) of the last forward at this resolution
    spec = None
    if SPECULATE and guess is not None and guess[0] > 0 and 0.5 <= P / guess[0] <= 2.0:
        scale = 1.06 * P / guess[0]
        cap = _C.lib.scr_binning_bytes(min(int(guess[1] * scale) + 4096, (1 << 32) - 2), max(int(guess[2] * 1.25), guess[2] + 64))
        spec = _C.scratch(cap, dev)
    _C.call("scr_forward_plan_run", mode, P, M, _C.ptr(means3D), _C.ptr(scales), _C.ptr(rotations), _C.ptr(cov3D_precomp),
            _C.ptr(opacities), _C.ptr(shs), _C.ptr(colors_precomp), cs.ref(), st.geom, _C.ptr(radii), plan, spec,
            0 if spec is None else spec.numel(), st.image, color, *maps)
    st.I, st.max_tile, st.flags = int(plan[0]), int(plan[1]), int(plan[3])
    _plan_guess[key] = (P, st.I, st.max_tile)
    if plan[2]:
        st.binning = spec
    else:
        del spec
        st.binning = _C.scratch(_C.lib.scr_binning_bytes(st.I, st.max_tile), dev)
        _C.call("scr_forward_run", P, st.I, st.max_tile, st.flags, cs.ref(), st.geom, st.binning, st.image, color, *maps)
    st.radii = radii
    return color, radii, st


def _debug_dump(path, raster_settings, **tensors):
    """debug=True (pipe.debug, switched on by --debug_from, train.py:179-180): the C-ABI synchronises and checks
    after every kernel; when a call fails the operator's inputs are written to `path` (snapshot_fw.dump /
    snapshot_bw.dump in the working directory, the operator family's convention) before the error propagates."""
    try:
        blob = {"raster_settings": {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v)
                                    for k, v in raster_settings._asdict().items()}}
        blob.update({k: (None if v is None else v.detach().cpu()) for k, v in tensors.items()})
        torch.save(blob, path)
        return f" (inputs written to {path})"
    except Exception as e:       # a faulted device may refuse the copies
        return f" (could not write {path}: {e})"


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, return_aux=False, antialiased=False, *camera):
        # camera: () or (viewmatrix, projmatrix, campos) -- the tensors of raster_settings once more, as inputs autograd sees
        ctx.camera = [(tuple(t.shape), t.dtype) for t in camera]
        cs = _CSettings(raster_settings)
        # no zero tensors for outputs that received no gradient: autograd filled an int32 [P] "gradient" of radii with
        # zeros before every backward (88 M elements at configs[4]); backward() treats a missing dL/dcolor as zero
        ctx.set_materialize_grads(False)
        means3D = _dev_f32(means3D, "means3D")
        none_if_empty = lambda t, n: None if t is None or t.numel() == 0 else _dev_f32(t, n)
        sh, colors_precomp = none_if_empty(sh, "shs"), none_if_empty(colors_precomp, "colors_precomp")
        scales, rotations = none_if_empty(scales, "scales"), none_if_empty(rotations, "rotations")
        cov3Ds_precomp = none_if_empty(cov3Ds_precomp, "cov3D_precomp")
        opacities = _dev_f32(opacities, "opacities")
        P = means3D.shape[0]
        if P == 0:  # nothing to launch: background only
            color = cs.bg.reshape(3, 1, 1).expand(3, cs.H, cs.W).contiguous()
            radii = torch.zeros(0, dtype=torch.int32, device=means3D.device)
            ctx.state = None
            ctx.shapes = (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
            ctx.mark_non_differentiable(radii)
            if return_aux:      # the background adds nothing to either map
                zero = torch.zeros(cs.H, cs.W, dtype=torch.float32, device=means3D.device)
                return color, radii, zero, torch.zeros_like(zero)
            return color, radii
        try:
            color, radii, st = rasterize_forward(cs, means3D, opacities, scales, rotations, cov3Ds_precomp, sh,
                                                 colors_precomp, **({"aux": True} if return_aux else {}),
                                                 **({"antialiased": True} if antialiased else {}))
        except RuntimeError as e:
            if raster_settings.debug:
                raise RuntimeError(str(e) + _debug_dump("snapshot_fw.dump", raster_settings, means3D=means3D, sh=sh,
                                                        colors_precomp=colors_precomp, opacities=opacities, scales=scales,
                                                        rotations=rotations, cov3Ds_precomp=cov3Ds_precomp)) from e
            raise
        ctx.state = st
        ctx.raster_settings = raster_settings
        ctx.save_for_backward(means3D, scales, rotations, cov3Ds_precomp, sh, colors_precomp, opacities)
        ctx.m2d_shape = tuple(means2D.shape)
        ctx.mark_non_differentiable(radii)
        if return_aux:
            (depth, alpha), st.aux = st.aux, None      # the state keeps what the backward needs, not the outputs
            return color, radii, depth, alpha
        return color, radii

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, grad_out_depth=None, grad_out_alpha=None):
        st = ctx.state
        # the camera tensors' gradients: asked of the kernel only where the tensor requires grad, None for the rest
        want_cam = [bool(w) for w in ctx.needs_input_grad[11:]]
        if st is None:
            zeros_cam = tuple(torch.zeros(shape, dtype=dt, device=ctx.shapes[0].device) if w else None
                              for (shape, dt), w in zip(ctx.camera, want_cam))
            return tuple(None if t is None else torch.zeros_like(t) for t in ctx.shapes) + (None, None, None) + zeros_cam
        if grad_out_color is None and grad_out_depth is None and grad_out_alpha is None:
            return (None,) * (11 + len(ctx.camera))      # no output took part in the loss: every gradient is zero
        means3D, scales, rotations, cov3D, sh, colors, opacities = ctx.saved_tensors
        dev, P, cs = means3D.device, st.P, st.cs
        # with a gradient for one of the maps the blend backward carries two more channels; without, this is the
        # colour-only backward whichever forward ran.  A missing dL/dcolor is zeros then: the kernels always read it
        aux = grad_out_depth is not None or grad_out_alpha is not None
        g = (_dev_f32(grad_out_color, "grad_out_color") if grad_out_color is not None
             else torch.zeros(3, cs.H, cs.W, dtype=torch.float32, device=dev))
        g_depth, g_alpha = _dev_f32(grad_out_depth, "grad_out_depth"), _dev_f32(grad_out_alpha, "grad_out_alpha")
        # All per-Gaussian PARAMETER gradients are carved from ONE arena, adjacent (means2D, a per-view statistic, is a
        # tensor of its own): when the operator's inputs are leaves their .grad tensors
        # alias the arena, and multiview.allreduce_gradients reduces it in place without packing copies.
        widths = [3, 3 if colors is not None else 0, 3 * st.M if sh is not None else 0, 1,
                  3 if cov3D is None else 0, 4 if cov3D is None else 0, 6 if cov3D is not None else 0]
        arena = torch.empty(P * sum(widths), dtype=torch.float32, device=dev)
        parts, off = [], 0
        for w in widths:
            parts.append(arena[off:off + P * w].view(P, w) if w else None)
            off += P * w
        g_means3D, g_col, g_sh, g_op, g_scales, g_rot, g_cov = parts
        # a tensor of its own: the caller may KEEP it as viewspace_points.grad (renderer.keep_grad) without pinning the arena
        g_means2D = torch.empty(P, 3, dtype=torch.float32, device=dev)
        if g_sh is not None:
            g_sh = g_sh.view(P, st.M, 3)
        del arena, parts
        g_cam = ()
        if any(want_cam):      # [16 | 16 | 3]: dL/dviewmatrix, dL/dprojmatrix, dL/dcampos, row-major like the settings' tensors
            cam_buf = torch.empty(35, dtype=torch.float32, device=dev)
            g_cam = tuple(cam_buf[lo:hi] if w else None for (lo, hi), w in zip(((0, 16), (16, 32), (32, 35)), want_cam))
        scratch = _C.scratch(_C.lib.scr_backward_scratch_bytes(st.I, P, int(aux), int(bool(g_cam))), dev)
        try:
            _C.call("scr_backward", P, st.M, st.I, st.flags, _C.ptr(means3D), _C.ptr(scales), _C.ptr(rotations), _C.ptr(cov3D),
                    _C.ptr(sh), cs.ref(), st.radii, st.geom, st.binning, st.image, g, _C.ptr(g_depth), _C.ptr(g_alpha), scratch,
                    g_means3D, g_means2D, _C.ptr(g_col), _C.ptr(g_sh), g_op, _C.ptr(g_scales), _C.ptr(g_rot), _C.ptr(g_cov),
                    *(_C.ptr(t) for t in g_cam or (None,) * 3))
        except RuntimeError as e:
            if ctx.raster_settings.debug:
                raise RuntimeError(str(e) + _debug_dump("snapshot_bw.dump", ctx.raster_settings, means3D=means3D, sh=sh,
                                                        colors_precomp=colors, opacities=opacities, scales=scales,
                                                        rotations=rotations, cov3Ds_precomp=cov3D, radii=st.radii,
                                                        grad_out_color=g, grad_out_depth=g_depth,
                                                        grad_out_alpha=g_alpha)) from e
            raise
        g_op = g_op.reshape(opacities.shape)
        if ctx.m2d_shape != (P, 3):
            g_means2D = g_means2D[:, :ctx.m2d_shape[1]].reshape(ctx.m2d_shape) if len(ctx.m2d_shape) == 2 else None
        # the camera gradients in the shape (and dtype) of the tensors given: autograd needs no more of a strided view
        g_cam = tuple(None if t is None else t.reshape(shape).to(dt) for t, (shape, dt) in zip(g_cam, ctx.camera))
        if len(g_cam) < len(ctx.camera):
            g_cam = (None,) * len(ctx.camera)
        # order: means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings, return_aux,
        # antialiased, camera
        return (g_means3D, g_means2D, g_sh, g_col, g_op, g_scales, g_rot, g_cov, None, None, None) + g_cam


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, return_aux=False, antialiased=False):
    camera = (raster_settings.viewmatrix, raster_settings.projmatrix, raster_settings.campos)
    if not (torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in camera)):
        camera = ()      # the default: the camera is a constant, nothing about the call changes
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, bool(return_aux), bool(antialiased), *camera)


class GaussianRasterizer(nn.Module):
    """Same constructor / forward / visible_filter / markVisible as the reference operator."""

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        with torch.no_grad():
            positions = _dev_f32(positions, "positions")
            P = positions.shape[0]
            out = torch.zeros(P, dtype=torch.uint8, device=positions.device)
            view = _dev_f32(self.raster_settings.viewmatrix, "viewmatrix")
            if P:
                _C.call("scr_mark_visible", P, positions, view, out)
            return out.bool()

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, antialiased=False, return_aux=False):
        """(image, radii); with return_aux=True (image, radii, depth, alpha): the [H, W] maps sum_i w_i z_i and sum_i w_i over
        the image's contributors (module docstring), differentiable like the image.  antialiased=True: every opacity is
        compensated for the 0.3 px^2 dilation of its splat (module docstring); radii are the same either way.  Pass both
        switches by keyword."""
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise ValueError('GaussianRasterizer: pass either shs or colors_precomp (one of them, not both, not neither)')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise ValueError('GaussianRasterizer: pass either scales + rotations or cov3D_precomp (one form of the covariance, not both, not neither)')
        empty = torch.Tensor([])
        return rasterize_gaussians(
            means3D, means2D, empty if shs is None else shs, empty if colors_precomp is None else colors_precomp,
            opacities, empty if scales is None else scales, empty if rotations is None else rotations,
            empty if cov3D_precomp is None else cov3D_precomp, self.raster_settings, return_aux, antialiased)

    def visible_filter(self, means3D, scales=None, rotations=None, cov3D_precomp=None):
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise ValueError('GaussianRasterizer: pass either scales + rotations or cov3D_precomp (one form of the covariance, not both, not neither)')
        with torch.no_grad():
            cs = _CSettings(self.raster_settings)
            means3D = _dev_f32(means3D, "means3D")
            scales, rotations = _dev_f32(scales, "scales"), _dev_f32(rotations, "rotations")
            cov3D_precomp = _dev_f32(cov3D_precomp, "cov3D_precomp")
            P = means3D.shape[0]
            radii = torch.empty(P, dtype=torch.int32, device=means3D.device)  # filter_kernel writes every entry
            if P:
                _C.call("scr_visible_filter", P, means3D, _C.ptr(scales), _C.ptr(rotations), _C.ptr(cov3D_precomp), cs.ref(), radii)
            return radii
