"""TSDF fusion of rendered depth maps into a dense volume and mesh extraction from it, on the device (host side of
csrc/tsdf.hip).

2DGS, PGSR, GOF and DN-Splatter all end in a triangle mesh fused from the rendered depth maps; this is that last step, without
Open3D.  The definition (normative; include/splatco_tsdf.h and tests/tsdf_ref.py restate it):

Volume.  Nodes p(i, j, k) = lo + h (i, j, k), 0 <= i < nx, 0 <= j < ny, 0 <= k < nz, every dimension >= 2, nx ny nz < 2^31;
linear node index n = (k ny + j) nx + i; tsdf [nz, ny, nx], weight [nz, ny, nx], optionally color [3, nz, ny, nx], float32.  A
fresh volume has tsdf = 1, weight = 0, color = 0.  lo and h are float32 values; all arithmetic between the float32 inputs and
the float32 outputs is binary64 in the written order.

Integrating one view (depth D = sum w z and alpha A = sum w [H, W] of render(aux=True), optionally the image [3, H, W] and a
mask; intrinsics fx, fy, cx, cy; W2C = world_view_transform^T).  Per node:
  1. pc = R p + t, row by row, left to right; zc = pc.z; skip the node if zc <= near
  2. u = fx pc.x / zc + cx, v = fy pc.y / zc + cy; px = floor(u), py = floor(v) (pixel px covers [px, px + 1), the
     rasterizer's convention and normals.intrinsics'); skip if the pixel is outside the image
  3. ok: D, A finite, A >= min_alpha, D > 0, the mask (if given) positive; skip otherwise; z = D / A, ONE binary32 division
  4. sdf = z - zc; skip if sdf < -trunc; d = min(1, sdf / trunc)
  5. with Wt the stored weight and w = 1: tsdf <- (tsdf Wt + d w) / (Wt + w); color_c <- (color_c Wt + image_c w) / (Wt + w)
     where an image was given and its three values at the pixel are finite; weight <- min(Wt + w, max_weight); each rounded
     to float32 once per view
Views are applied in list order; a batch of views in one launch gives the bits of the same views one launch each.

Extraction: marching tetrahedra at level 0 on the six Kuhn tetrahedra of every cube whose 8 nodes have weight > min_weight
(tetrahedron q = 0..5: axis permutation pi in lexicographic order, nodes corner, + e_pi1, + e_pi2, corner + (1, 1, 1)); a node
is inside when tsdf < 0; one vertex per lattice edge (id 7 n + dir) whose nodes differ and that lies in a valid cube, in
ascending id, at p_a + (p_b - p_a) s_a / (s_a - s_b) with a the node of lower linear index; faces by cube, tetrahedron,
triangle, wound counter-clockwise seen from the free-space side.  The mesh is indexed and welded.

    vol = TSDFVolume.from_bounds(lo, hi, voxel_size)
    out = render(cam, pc, pipe, bg, aux=True)
    vol.integrate(out["depth"], out["alpha"], cam, image=out["render"])
    vertices, faces, colors = vol.extract()
    scene_io.write_ply_mesh("mesh.ply", vertices, faces, colors)

or extract_mesh(views, pc, pipe, bg, voxel_size) for all of it.  Component filtering and vertex normals of the extracted mesh
are splatco_amd.mesh's (extract_mesh(..., keep_largest=50, min_faces=50) ends in its clean_mesh).  Scenes too large for a dense
volume go to splatco_amd.tsdf_sparse (extract_mesh(..., sparse=True)), which stores 8 x 8 x 8-node blocks near the surface only.
Not built: hashed volumes, decimation, smoothing, texture baking, a weight other than 1 per observation, bilinear depth lookup,
gradients, multi-rank fusion.

Every launch goes through _C.family_call.  There is no CPU path: a CPU tensor is a ValueError."""
import ctypes
import math

import numpy as np
import torch

from . import _C
from .normals import _mask_operand, _resolve

BATCH = _C.TSDF_MAX_VIEWS


def _finite_positive(fn, name, x):
    x = float(x)
    if not (0.0 < x < float("inf")):
        raise ValueError(f"{fn}: {name} = {x} must be finite and > 0")
    return x


def _check_dims(fn, dims):
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3 or min(dims) < 2:
        raise ValueError(f"{fn}: dims {dims} must be three sizes (nx, ny, nz), each >= 2")
    if dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError(f"{fn}: dims {dims}: the node count {dims[0] * dims[1] * dims[2]} is not below 2^31")
    return dims


def _device_only(fn, name, t):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{fn}: {name} is not a tensor")
    if not t.is_cuda:
        raise ValueError(f"{fn}: {name} is on {t.device}; the TSDF volume lives on the GPU and there is no CPU path")


def _camera(fn, cam):
    """(intrinsics, 12 floats of the world-to-camera rows, znear or None)"""
    if hasattr(cam, "FoVx"):
        intr, wvt, znear = _resolve(fn, cam), cam.world_view_transform.detach().t(), getattr(cam, "znear", None)
    else:
        if len(cam) != 2:
            raise ValueError(f"{fn}: cam must be a camera or ((fx, fy, cx, cy), w2c [4, 4])")
        intr, wvt, znear = _resolve(fn, cam[0]), torch.as_tensor(cam[1]).detach(), None
    if tuple(wvt.shape) != (4, 4):
        raise ValueError(f"{fn}: the world-to-camera matrix has shape {tuple(wvt.shape)}, not (4, 4)")
    rows = [float(x) for x in wvt.double().cpu()[:3].reshape(-1).tolist()]
    if not all(math.isfinite(x) for x in rows):
        raise ValueError(f"{fn}: the world-to-camera matrix is not finite")
    return intr, rows, znear


class TSDFVolume:
    """A dense truncated signed distance volume on one GPU (see the module's definition).

    lo: the position of node (0, 0, 0); voxel_size: the node spacing h; dims = (nx, ny, nz); trunc: the truncation distance
    (default 4 h); color: also fuse the rendered images; max_weight: the weight's cap.  The tensors tsdf [nz, ny, nx],
    weight [nz, ny, nx] and color [3, nz, ny, nx] (or None) are the volume itself, updated in place."""

    def __init__(self, lo, voxel_size, dims, trunc=None, color=True, max_weight=255.0, device="cuda"):
        fn = "TSDFVolume"
        self._geometry(fn, lo, voxel_size, dims, trunc, max_weight)
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"{fn}: device {device}: the TSDF volume lives on the GPU and there is no CPU path")
        nx, ny, nz = self.dims
        self.tsdf = torch.empty(nz, ny, nx, dtype=torch.float32, device=device).fill_(1.0)
        self.weight = torch.empty(nz, ny, nx, dtype=torch.float32, device=device).zero_()
        self.color = torch.empty(3, nz, ny, nx, dtype=torch.float32, device=device).zero_() if color else None

    def _geometry(self, fn, lo, voxel_size, dims, trunc, max_weight):
        self.dims = _check_dims(fn, dims)
        self.voxel_size = float(np.float32(_finite_positive(fn, "voxel_size", voxel_size)))
        if not self.voxel_size > 0.0:
            raise ValueError(f"{fn}: voxel_size = {voxel_size} is not a positive float32 value")
        lo = [float(x) for x in (lo.detach().cpu().reshape(-1).tolist() if isinstance(lo, torch.Tensor) else np.asarray(lo).reshape(-1))]
        if len(lo) != 3 or not all(math.isfinite(x) for x in lo):
            raise ValueError(f"{fn}: lo {lo} must be three finite coordinates")
        self.lo = tuple(float(np.float32(x)) for x in lo)
        self.trunc = _finite_positive(fn, "trunc", 4.0 * self.voxel_size if trunc is None else trunc)
        self.max_weight = float(np.float32(_finite_positive(fn, "max_weight", max_weight)))

    @classmethod
    def from_bounds(cls, lo, hi, voxel_size, **kw):
        """The smallest volume of spacing voxel_size from lo that covers [lo, hi]: dims = ceil((hi - lo) / h) + 1."""
        h = _finite_positive("TSDFVolume.from_bounds", "voxel_size", voxel_size)
        lo_, hi_ = (np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64).reshape(-1) for x in (lo, hi))
        if lo_.shape != (3,) or hi_.shape != (3,) or not (np.isfinite(lo_).all() and np.isfinite(hi_).all()) or (hi_ < lo_).any():
            raise ValueError(f"TSDFVolume.from_bounds: bounds {lo_.tolist()} .. {hi_.tolist()} are not two finite corners lo <= hi")
        dims = [max(int(math.ceil(float(e) / h)) + 1, 2) for e in hi_ - lo_]
        return cls(lo_, h, dims, **kw)

    @classmethod
    def from_tensors(cls, lo, voxel_size, tsdf, weight, color=None, trunc=None, max_weight=255.0):
        """A volume over existing tensors (not copied): tsdf, weight [nz, ny, nx], color [3, nz, ny, nx] or None, float32,
        contiguous, on one GPU.  trunc and max_weight as in the constructor: what the volume was, or is to be, fused with."""
        fn = "TSDFVolume.from_tensors"
        for name, t in (("tsdf", tsdf), ("weight", weight), ("color", color)):
            if not isinstance(t, torch.Tensor) and not (t is None and name == "color"):
                raise ValueError(f"{fn}: {name} is not a tensor")
        if tsdf.dim() != 3:
            raise ValueError(f"{fn}: tsdf {tuple(tsdf.shape)} is not [nz, ny, nx]")
        nz, ny, nx = tsdf.shape
        _check_dims(fn, (nx, ny, nz))
        given = [("tsdf", tsdf, (nz, ny, nx)), ("weight", weight, (nz, ny, nx))]
        given += [] if color is None else [("color", color, (3, nz, ny, nx))]
        for name, t, shape in given:
            if tuple(t.shape) != shape or t.dtype != torch.float32:
                raise ValueError(f"{fn}: {name} {tuple(t.shape)} {t.dtype} is not float32 {shape}")
            if not t.is_contiguous():
                raise ValueError(f"{fn}: {name} is not contiguous")
        for name, t, _ in given:
            _device_only(fn, name, t)
            if t.device != tsdf.device:
                raise ValueError(f"{fn}: {name} is on {t.device}, tsdf on {tsdf.device}")
        self = cls.__new__(cls)
        self._geometry(fn, lo, voxel_size, (nx, ny, nz), trunc, max_weight)
        self.tsdf, self.weight, self.color = tsdf, weight, color
        return self

    @property
    def device(self):
        return self.tsdf.device

    def _check_volume(self, fn):
        nx, ny, nz = self.dims
        held = [("tsdf", self.tsdf, (nz, ny, nx)), ("weight", self.weight, (nz, ny, nx))]
        held += [] if self.color is None else [("color", self.color, (3, nz, ny, nx))]
        for name, t, shape in held:
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.float32:
                raise ValueError(f"{fn}: the volume's {name} is not a float32 tensor of shape {shape}")
            if not t.is_contiguous():
                raise ValueError(f"{fn}: the volume's {name} is not contiguous")
        for name, t, _ in held:
            _device_only(fn, "the volume's " + name, t)
            if t.device != self.tsdf.device:
                raise ValueError(f"{fn}: the volume's {name} is on {t.device}, tsdf on {self.tsdf.device}")

    # ------------------------------------------------------------------ integration
    def _view(self, fn, depth, alpha, cam, image, mask, min_alpha, near):
        """One checked view: (TsdfView fields, the tensors it points into).  Shapes and scalars first, devices last."""
        for name, t in (("depth", depth), ("alpha", alpha), ("image", image), ("mask", mask)):
            if t is not None and not isinstance(t, torch.Tensor):
                raise ValueError(f"{fn}: {name} is not a tensor")
        if depth is None or alpha is None:
            raise ValueError(f"{fn}: depth and alpha are both needed")
        min_alpha = float(min_alpha)
        if not (0.0 <= min_alpha < float("inf")):
            raise ValueError(f"{fn}: min_alpha {min_alpha} must be finite and >= 0")
        if depth.dim() != 2 or depth.numel() == 0:
            raise ValueError(f"{fn}: depth {tuple(depth.shape)} is not a non-empty [H, W] map")
        if depth.numel() >= 2 ** 31:
            raise ValueError(f"{fn}: H W = {depth.numel()} is not below 2^31")
        for name, t, lead in (("alpha", alpha, ()), ("image", image, (3,)), ("mask", mask, ())):
            if t is not None and tuple(t.shape) != lead + tuple(depth.shape):
                raise ValueError(f"{fn}: {name} {tuple(t.shape)} does not match depth {tuple(depth.shape)}")
        if image is not None and self.color is None:
            raise ValueError(f"{fn}: an image was given, but the volume was made with color=False")
        intr, rows, znear = _camera(fn, cam)
        near = float(near)
        if not (0.0 <= near < float("inf")):
            raise ValueError(f"{fn}: near {near} must be finite and >= 0")
        if znear is not None:
            near = max(near, float(znear))
        for name, t in (("depth", depth), ("alpha", alpha), ("image", image), ("mask", mask)):
            if t is not None:
                _device_only(fn, name, t)
                if t.device != self.device:
                    raise ValueError(f"{fn}: {name} is on {t.device}, the volume on {self.device}")
        c = lambda t: None if t is None else t.detach().contiguous().float()
        depth, alpha, image = c(depth), c(alpha), c(image)
        mask, kind = _mask_operand(mask)
        H, W = depth.shape
        view = _C.TsdfView(depth.data_ptr(), alpha.data_ptr(), None if image is None else image.data_ptr(),
                           None if mask is None else mask.data_ptr(), H, W, kind, min_alpha, *intr, (ctypes.c_double * 12)(*rows), near)
        return view, (depth, alpha, image, mask)

    def integrate(self, depth, alpha, cam, image=None, mask=None, min_alpha=0.5, near=0.05):
        """Fuse one view.  cam: a camera (image_width, image_height, FoVx, FoVy, world_view_transform; a `near` below its znear
        is raised to it) or ((fx, fy, cx, cy), w2c [4, 4])."""
        self._integrate("TSDFVolume.integrate", [depth], [alpha], [cam], None if image is None else [image],
                        None if mask is None else [mask], min_alpha, near, 1)

    def integrate_views(self, depths, alphas, cams, images=None, masks=None, min_alpha=0.5, near=0.05, batch=1):
        """Fuse lists of views in list order, `batch` (1 to 16) views per pass over the volume; whatever the batch, the result
        is the same bits.  The default of one view per pass is the fastest setting measured at 256^3 and 512^3 nodes
        (DESIGN.md section 3).  images / masks: None, or lists with None for the views that have none.  Everything is checked
        before the first launch."""
        self._integrate("TSDFVolume.integrate_views", depths, alphas, cams, images, masks, min_alpha, near, batch)

    def _integrate(self, fn, depths, alphas, cams, images, masks, min_alpha, near, batch):
        n = len(depths)
        batch = int(batch)
        if not 1 <= batch <= BATCH:
            raise ValueError(f"{fn}: batch {batch} is not in 1 .. {BATCH}")
        for name, lst in (("alphas", alphas), ("cams", cams), ("images", images), ("masks", masks)):
            if lst is not None and len(lst) != n:
                raise ValueError(f"{fn}: {len(lst)} {name} for {n} depths")
        views, keep = [], []
        for i in range(n):
            v, held = self._view(fn, depths[i], alphas[i], cams[i], None if images is None else images[i],
                                 None if masks is None else masks[i], min_alpha, near)
            views.append(v)
            keep.append(held)
        self._check_volume(fn)
        nx, ny, nz = self.dims
        lo = _C.host_array(self.lo, _C.f32)
        for first in range(0, n, batch):
            chunk = views[first:first + batch]
            _C.family_call("scr_tsdf_integrate", nx, ny, nz, lo, self.voxel_size, self.trunc, self.max_weight, self.tsdf, self.weight,
                           self.color, len(chunk), (_C.TsdfView * len(chunk))(*chunk), device=self.device)
        del keep                    # the maps outlived the launches that read them (same stream: the allocator orders reuse)

    # ------------------------------------------------------------------ extraction
    def extract(self, min_weight=0.0):
        """-> (vertices [Nv, 3] float32, faces [Nf, 3] int32, colors [Nv, 3] float32 or None) on the device: marching tetrahedra
        at level 0 over the cubes whose 8 nodes have weight > min_weight.  Two host reads (the two counts)."""
        fn = "TSDFVolume.extract"
        min_weight = float(min_weight)
        if math.isnan(min_weight):
            raise ValueError(f"{fn}: min_weight is NaN")
        nx, ny, nz = self.dims
        if 7 * nx * ny * nz >= 2 ** 31:
            raise ValueError(f"{fn}: 7 nx ny nz = {7 * nx * ny * nz} edge ids are not below 2^31")
        self._check_volume(fn)
        dev = self.device
        empty = lambda dt: torch.zeros(0, 3, dtype=dt, device=dev)
        scratch = _C.scratch(_C.lib.scr_tsdf_extract_scratch_bytes(nx, ny, nz), dev)
        count = ctypes.c_int64(0)
        _C.family_call("scr_tsdf_extract_vertices_plan", nx, ny, nz, self.tsdf, self.weight, min_weight, scratch, ctypes.byref(count),
                       device=dev)
        nv = count.value
        if nv == 0:
            return empty(torch.float32), empty(torch.int32), None if self.color is None else empty(torch.float32)
        ids = torch.empty(nv, dtype=torch.int32, device=dev)
        vertices = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        colors = None if self.color is None else torch.empty(nv, 3, dtype=torch.float32, device=dev)
        _C.family_call("scr_tsdf_extract_vertices_run", nx, ny, nz, _C.host_array(self.lo, _C.f32), self.voxel_size, self.tsdf, self.weight,
                       self.color, min_weight, scratch, nv, ids, vertices, colors, device=dev)
        _C.family_call("scr_tsdf_extract_faces_plan", nx, ny, nz, self.tsdf, self.weight, min_weight, scratch, ctypes.byref(count),
                       device=dev)
        nf = count.value
        faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        if nf:
            _C.family_call("scr_tsdf_extract_faces_run", nx, ny, nz, self.tsdf, self.weight, min_weight, scratch, nv, ids, nf, faces,
                           device=dev)
        return vertices, faces, colors


def extract_mesh(views, pc, pipe, bg, voxel_size, bounds=None, trunc=None, min_alpha=0.5, antialiased=None, filter_3d=None,
                 color=True, sparse=False, keep_largest=None, min_faces=None):
    """Render every view in evaluation mode (evaluate._eval_mode, no_grad, prefilter_voxel then render(aux=True), as
    evaluate.render_views does), fuse depth, alpha and (color=True) the image of each into one volume as it is rendered, and
    extract the mesh: (vertices [Nv, 3] float32, faces [Nf, 3] int32, colors [Nv, 3] float32 or None) on the device.
    bounds: (lo, hi); None takes the bounding box of the anchors padded by trunc (default 4 voxel_size).  keep_largest /
    min_faces: where either is given, the mesh goes through mesh.clean_mesh (2DGS's post_process_mesh uses 50) before it is
    returned; with both None nothing of that module runs.  sparse=True fuses into a tsdf_sparse.SparseTSDFVolume over the same
    bounds instead: every rendered view allocates its blocks and is integrated as it comes, so a block holds the views from
    its first sighting on (that module's ORDER DEPENDENCE), and bounds beyond the dense volume's 2^31 nodes are accepted."""
    from . import knn_grid
    from .evaluate import _eval_mode
    from .renderer import prefilter_voxel, render
    h = _finite_positive("extract_mesh", "voxel_size", voxel_size)
    trunc = _finite_positive("extract_mesh", "trunc", 4.0 * h if trunc is None else trunc)
    if bounds is None:
        lo, hi = knn_grid.bounds(pc.get_anchor.detach())
        lo, hi = np.asarray(lo, np.float64) - trunc, np.asarray(hi, np.float64) + trunc
    else:
        lo, hi = bounds
    if sparse:
        from .tsdf_sparse import SparseTSDFVolume
        vol = SparseTSDFVolume.from_bounds(lo, hi, h, trunc=trunc, color=color, device=pc.get_anchor.device)
    else:
        vol = TSDFVolume.from_bounds(lo, hi, h, trunc=trunc, color=color, device=pc.get_anchor.device)
    extra = {} if antialiased is None else {"antialiased": antialiased}
    if filter_3d is not None:
        extra["filter_3d"] = filter_3d
    with _eval_mode(pc), torch.no_grad():
        for view in views:
            vis = prefilter_voxel(view, pc, pipe, bg)
            out = render(view, pc, pipe, bg, visible_mask=vis, aux=True, **extra)
            if sparse:
                vol.integrate(out["depth"], out["alpha"], view, image=out["render"] if color else None, min_alpha=min_alpha, near=0.05)
                continue
            vol._integrate("extract_mesh", [out["depth"]], [out["alpha"]], [view], [out["render"]] if color else None, None,
                           min_alpha, 0.05, 1)
    if keep_largest is None and min_faces is None:
        return vol.extract()
    from .mesh import clean_mesh
    return clean_mesh(*vol.extract(), keep_largest=keep_largest, min_faces=min_faces)[:3]
