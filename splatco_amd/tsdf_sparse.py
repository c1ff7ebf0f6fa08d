"""A block-sparse TSDF volume: fuse and mesh scenes too large for the dense TSDFVolume (host side of csrc/tsdf_sparse.hip).

The volume is a virtual lattice of splatco_amd.tsdf's kind (lo, voxel_size, dims, trunc, max_weight; every dimension >= 2 and
< 2^20, the node count may exceed 2^31) that stores 8 x 8 x 8-node blocks only where a depth map puts a surface.  The
definition is include/splatco_tsdf_sparse.h's (normative; tests/tsdf_sparse_ref.py restates the allocation rule):

Blocks.  nb? = ceil(n? / 8); block (bi, bj, bk) has the int32 key (bk nby + bj) nbx + bi (nbx nby nbz < 2^31); a node's local
index is l = (lk 8 + lj) 8 + li.  keys [Nb] ascending, slots [Nb] the storage row of each key, tsdf / weight [cap, 512],
color [cap, 3, 512] or None.  A new block holds tsdf 1, weight 0, colour 0; the new blocks of one allocation take the rows
Nb_old + rank, rank their position among the new keys in ascending order.  Growing the capacity copies rows.

Allocation for one view: every pixel that passes the dense family's pixel test (D, A finite, A >= min_alpha, D > 0, mask) takes
z = D / A, the depth slab [max(z - trunc, near), z + trunc] of its pixel frustum, the world box of the slab's 8 corners padded
by h / 8, and allocates every block that box meets.  Every node the dense update would move with |sdf| <= trunc is covered;
free space in front of the band is deliberately not allocated.

Integration of one view: every node of every allocated block gets the dense family's update, by the same device code, so the
bits are the dense volume's.

ORDER DEPENDENCE (inherent): a block allocated at view a has missed the views before a; its nodes hold what a dense volume
fused from the views a, a + 1, ... holds.  integrate_views(..., two_pass=True) allocates for all views first and integrates
them afterwards, which gives exactly the dense volume on every allocated block.

Extraction: the dense family's marching tetrahedra over the cubes whose corner is in an allocated block and whose 8 nodes lie
inside dims, in allocated blocks, with weight > min_weight.  Vertices come in ascending (block key, local edge id), faces in
ascending (block key, local cube, tetrahedron, triangle); the mesh is indexed and welded.  The two compactions run over
3584 Nb edge ids and 6144 Nb triangle slots, in passes of at most 349525 blocks (6144 per block, below 2^31 per pass) with one
host read per pass and compaction; Nv and Nf stay below 2^31.

    vol = SparseTSDFVolume.from_bounds(lo, hi, voxel_size)
    vol.integrate(out["depth"], out["alpha"], cam, image=out["render"])         # allocates, then fuses
    vertices, faces, colors = vol.extract()

Not built: hashing, block eviction or streaming to the host, multi-rank fusion, gradients, bilinear depth lookup, weights other
than 1, decimation and smoothing.  Every launch goes through _C.family_call; a CPU tensor is a ValueError."""
import ctypes
import math

import numpy as np
import torch

from . import _C
from .tsdf import TSDFVolume, _finite_positive

B = _C.TSDFS_BLOCK
NODES = B * B * B
MAX_EXTRACT_BLOCKS = (2 ** 31 - 1) // (12 * NODES)


def _check_dims(fn, dims):
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3 or min(dims) < 2:
        raise ValueError(f"{fn}: dims {dims} must be three sizes (nx, ny, nz), each >= 2")
    if max(dims) >= 2 ** 20:
        raise ValueError(f"{fn}: dims {dims}: every dimension must be below 2^20")
    nb = tuple((d + B - 1) // B for d in dims)
    if nb[0] * nb[1] * nb[2] >= 2 ** 31:
        raise ValueError(f"{fn}: dims {dims}: the block count {nb[0] * nb[1] * nb[2]} is not below 2^31")
    return dims, nb


class SparseTSDFVolume:
    """A block-sparse truncated signed distance volume on one GPU (see the module's definition).

    lo, voxel_size, dims, trunc, color, max_weight: as TSDFVolume's.  capacity: storage rows to start with (the storage doubles
    when it runs out); max_blocks: an allocation that would take the volume beyond it raises and allocates nothing."""

    def __init__(self, lo, voxel_size, dims, trunc=None, color=True, max_weight=255.0, device="cuda", capacity=None, max_blocks=None):
        fn = "SparseTSDFVolume"
        checked = _check_dims(fn, dims)
        TSDFVolume._geometry(self, fn, lo, voxel_size, (2, 2, 2), trunc, max_weight)      # lo, voxel_size, trunc, max_weight: the dense volume's rules
        self.dims, self.block_dims = checked
        virtual = self.block_dims[0] * self.block_dims[1] * self.block_dims[2]
        self.max_blocks = virtual if max_blocks is None else int(max_blocks)
        if self.max_blocks < 1:
            raise ValueError(f"{fn}: max_blocks {max_blocks} must be >= 1")
        capacity = min(1024, virtual) if capacity is None else int(capacity)
        if capacity < 1:
            raise ValueError(f"{fn}: capacity {capacity} must be >= 1")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"{fn}: device {device}: the TSDF volume lives on the GPU and there is no CPU path")
        self._color = bool(color)
        self.keys = torch.zeros(0, dtype=torch.int32, device=device)
        self.slots = torch.zeros(0, dtype=torch.int32, device=device)
        self._marks = torch.empty(virtual, dtype=torch.uint8, device=device).zero_()
        self._store(capacity, device)

    def _store(self, capacity, device, old=None):
        """Storage of `capacity` rows, uninitialised but for the rows copied from `old` = (tsdf, weight, color, rows)."""
        tsdf = torch.empty(capacity, NODES, dtype=torch.float32, device=device)
        weight = torch.empty(capacity, NODES, dtype=torch.float32, device=device)
        color = torch.empty(capacity, 3, NODES, dtype=torch.float32, device=device) if self._color else None
        if old is not None and old[3]:
            n = old[3]
            tsdf[:n].copy_(old[0][:n])
            weight[:n].copy_(old[1][:n])
            if color is not None:
                color[:n].copy_(old[2][:n])
        self._tsdf, self._weight, self._colors = tsdf, weight, color

    @classmethod
    def from_bounds(cls, lo, hi, voxel_size, **kw):
        """The smallest volume of spacing voxel_size from lo that covers [lo, hi]: dims = ceil((hi - lo) / h) + 1."""
        h = _finite_positive("SparseTSDFVolume.from_bounds", "voxel_size", voxel_size)
        lo_, hi_ = (np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64).reshape(-1) for x in (lo, hi))
        if lo_.shape != (3,) or hi_.shape != (3,) or not (np.isfinite(lo_).all() and np.isfinite(hi_).all()) or (hi_ < lo_).any():
            raise ValueError(f"SparseTSDFVolume.from_bounds: bounds {lo_.tolist()} .. {hi_.tolist()} are not two finite corners lo <= hi")
        dims = [max(int(math.ceil(float(e) / h)) + 1, 2) for e in hi_ - lo_]
        return cls(lo_, h, dims, **kw)

    # ------------------------------------------------------------------ what the volume holds
    @property
    def device(self):
        return self._marks.device

    @property
    def num_blocks(self):
        return int(self.keys.shape[0])

    @property
    def capacity(self):
        return int(self._tsdf.shape[0])

    @property
    def tsdf(self):
        """[cap, 512]: row slots[r] is the block keys[r]."""
        return self._tsdf

    @property
    def weight(self):
        return self._weight

    @property
    def color(self):
        """[cap, 3, 512], or None for a volume made with color=False."""
        return self._colors

    def block_coords(self):
        """[Nb, 3] int32 (bi, bj, bk) of the allocated blocks, in key order."""
        nbx, nby, _ = self.block_dims
        k = self.keys
        rest = torch.div(k, nbx, rounding_mode="floor")
        return torch.stack((k % nbx, rest % nby, torch.div(rest, nby, rounding_mode="floor")), dim=1).to(torch.int32)

    def bytes_held(self):
        """Device bytes of the storage, the key lists and the mark array."""
        held = [self._tsdf, self._weight, self._colors, self.keys, self.slots, self._marks]
        return sum(t.numel() * t.element_size() for t in held if t is not None)

    # ------------------------------------------------------------------ views
    def _view(self, fn, depth, alpha, cam, image, mask, min_alpha, near):
        """One checked view: (TsdfsView, the tensors it points into): TSDFVolume's own checks, camera forms, mask kinds and near
        rule, and the binary64 inverse of the world-to-camera matrix."""
        view, held = TSDFVolume._view(self, fn, depth, alpha, cam, image, mask, min_alpha, near)
        w2c = np.eye(4)
        w2c[:3] = np.array(list(view.w2c), np.float64).reshape(3, 4)
        try:
            c2w = np.linalg.inv(w2c)
        except np.linalg.LinAlgError:
            raise ValueError(f"{fn}: the world-to-camera matrix is singular") from None
        if not np.isfinite(c2w).all():
            raise ValueError(f"{fn}: the inverse of the world-to-camera matrix is not finite")
        return _C.TsdfsView(view, (ctypes.c_double * 12)(*c2w[:3].reshape(-1).tolist())), held

    def _views(self, fn, depths, alphas, cams, images, masks, min_alpha, near):
        n = len(depths)
        for name, lst in (("alphas", alphas), ("cams", cams), ("images", images), ("masks", masks)):
            if lst is not None and len(lst) != n:
                raise ValueError(f"{fn}: {len(lst)} {name} for {n} depths")
        return [self._view(fn, depths[i], alphas[i], cams[i], None if images is None else images[i],
                           None if masks is None else masks[i], min_alpha, near) for i in range(n)]

    # ------------------------------------------------------------------ allocation
    def allocate(self, depth, alpha, cam, mask=None, min_alpha=0.5, near=0.05):
        """Allocate the blocks this view's depth band touches; -> the number of new blocks.  Raises, before anything grows,
        when max_blocks would be exceeded."""
        view, held = self._view("SparseTSDFVolume.allocate", depth, alpha, cam, None, mask, min_alpha, near)
        n = self._allocate("SparseTSDFVolume.allocate", view)
        del held
        return n

    def _allocate(self, fn, view):
        nx, ny, nz = self.dims
        dev = self.device
        scratch = _C.scratch(_C.lib.scr_tsdfs_alloc_scratch_bytes(nx, ny, nz), dev)
        count = ctypes.c_int64(0)
        _C.family_call("scr_tsdfs_alloc_plan", nx, ny, nz, _C.host_array(self.lo, _C.f32), self.voxel_size, self.trunc, ctypes.byref(view),
                       self._marks, scratch, ctypes.byref(count), device=dev)
        new, old = count.value, self.num_blocks
        if new == 0:
            return 0
        if old + new > self.max_blocks:
            self._marks.mul_(self._marks == 2)          # forget the marks of the refused view
            raise RuntimeError(f"{fn}: {new} new blocks on top of {old} exceed max_blocks = {self.max_blocks}")
        if old + new > self.capacity:
            self._store(max(2 * self.capacity, old + new), dev, old=(self._tsdf, self._weight, self._colors, old))
        new_keys = torch.empty(new, dtype=torch.int32, device=dev)
        keys = torch.empty(old + new, dtype=torch.int32, device=dev)
        slots = torch.empty(old + new, dtype=torch.int32, device=dev)
        _C.family_call("scr_tsdfs_alloc_run", nx, ny, nz, self._marks, scratch, old, _C.ptr(self.keys), _C.ptr(self.slots), new, new_keys,
                       keys, slots, device=dev)
        _C.family_call("scr_tsdfs_init_blocks", old, new, self._tsdf, self._weight, self._colors, device=dev)
        self.keys, self.slots = keys, slots
        return new

    # ------------------------------------------------------------------ integration
    def integrate(self, depth, alpha, cam, image=None, mask=None, min_alpha=0.5, near=0.05, allocate=True):
        """Fuse one view into the allocated blocks, after allocating for it (allocate=True).  cam: as TSDFVolume.integrate's."""
        fn = "SparseTSDFVolume.integrate"
        view, held = self._view(fn, depth, alpha, cam, image, mask, min_alpha, near)
        if allocate:
            self._allocate(fn, view)
        self._integrate(view)
        del held

    def integrate_views(self, depths, alphas, cams, images=None, masks=None, min_alpha=0.5, near=0.05, allocate=True, two_pass=False):
        """Fuse lists of views in list order, one view per pass over the blocks.  two_pass=True allocates for all views first:
        every allocated block then holds what the dense volume holds (see ORDER DEPENDENCE in the module's text).  Everything
        is checked before the first launch."""
        fn = "SparseTSDFVolume.integrate_views"
        views = self._views(fn, depths, alphas, cams, images, masks, min_alpha, near)
        if two_pass:
            for view, _ in views:
                self._allocate(fn, view)
        for view, _ in views:
            if allocate and not two_pass:
                self._allocate(fn, view)
            self._integrate(view)
        del views                   # the maps outlived the launches that read them (same stream: the allocator orders reuse)

    def _integrate(self, view):
        nx, ny, nz = self.dims
        if self.num_blocks:
            _C.family_call("scr_tsdfs_integrate", nx, ny, nz, _C.host_array(self.lo, _C.f32), self.voxel_size, self.trunc, self.max_weight,
                           self.num_blocks, self.keys, self.slots, self._tsdf, self._weight, self._colors, ctypes.byref(view),
                           device=self.device)

    # ------------------------------------------------------------------ to and from the dense volume (torch indexing)
    def _padded(self, t):
        """[(3,) nbz 8, nby 8, nbx 8] seen as blocks [(3,) nbz nby nbx, 512] (a copy)."""
        nbx, nby, nbz = self.block_dims
        lead = t.shape[:-3]
        return t.reshape(*lead, nbz, B, nby, B, nbx, B).permute(*range(len(lead)), -6, -4, -2, -5, -3, -1).reshape(*lead, nbz * nby * nbx, NODES)

    def _unpadded(self, blocks):
        nbx, nby, nbz = self.block_dims
        nx, ny, nz = self.dims
        lead = blocks.shape[:-2]
        t = blocks.reshape(*lead, nbz, nby, nbx, B, B, B).permute(*range(len(lead)), -6, -3, -5, -2, -4, -1)
        return t.reshape(*lead, nbz * B, nby * B, nbx * B)[..., :nz, :ny, :nx].contiguous()

    def to_dense(self):
        """A TSDFVolume of the same lattice: the allocated blocks' nodes, every other node fresh.  Refused at >= 2^31 nodes."""
        fn = "SparseTSDFVolume.to_dense"
        nx, ny, nz = self.dims
        if nx * ny * nz >= 2 ** 31:
            raise ValueError(f"{fn}: dims {self.dims}: the node count {nx * ny * nz} is not below 2^31")
        nbx, nby, nbz = self.block_dims
        dev, virtual = self.device, nbx * nby * nbz
        keys, slots = self.keys.long(), self.slots.long()
        tsdf = torch.ones(virtual, NODES, dtype=torch.float32, device=dev)
        weight = torch.zeros(virtual, NODES, dtype=torch.float32, device=dev)
        tsdf[keys] = self._tsdf[slots]
        weight[keys] = self._weight[slots]
        color = None
        if self._colors is not None:
            color = torch.zeros(3, virtual, NODES, dtype=torch.float32, device=dev)
            color[:, keys] = self._colors[slots].permute(1, 0, 2)
            color = self._unpadded(color)
        return TSDFVolume.from_tensors(self.lo, self.voxel_size, self._unpadded(tsdf), self._unpadded(weight), color, trunc=self.trunc,
                                       max_weight=self.max_weight)

    @classmethod
    def from_dense(cls, volume, blocks=None, capacity=None, max_blocks=None):
        """The blocks `blocks` of a TSDFVolume: a bool [nbz, nby, nbx] mask or a tensor of keys; None takes the blocks that
        contain a node with weight > 0."""
        fn = "SparseTSDFVolume.from_dense"
        if not isinstance(volume, TSDFVolume):
            raise ValueError(f"{fn}: volume is not a TSDFVolume")
        volume._check_volume(fn)
        nx, ny, nz = volume.dims
        dev = volume.device
        self = cls.__new__(cls)
        self.dims, self.block_dims = _check_dims(fn, volume.dims)
        self.voxel_size, self.lo, self.trunc, self.max_weight = volume.voxel_size, volume.lo, volume.trunc, volume.max_weight
        nbx, nby, nbz = self.block_dims
        virtual = nbx * nby * nbz
        pad = (0, nbx * B - nx, 0, nby * B - ny, 0, nbz * B - nz)
        tsdf = self._padded(torch.nn.functional.pad(volume.tsdf, pad, value=1.0))
        weight = self._padded(torch.nn.functional.pad(volume.weight, pad, value=0.0))
        if blocks is None:
            keys = torch.nonzero((weight > 0).any(dim=1)).reshape(-1)
        else:
            if not isinstance(blocks, torch.Tensor):
                raise ValueError(f"{fn}: blocks is not a tensor")
            if blocks.device != dev:
                raise ValueError(f"{fn}: blocks is on {blocks.device}, the volume on {dev}")
            if blocks.dtype == torch.bool:
                if tuple(blocks.shape) != (nbz, nby, nbx):
                    raise ValueError(f"{fn}: the block mask {tuple(blocks.shape)} is not [nbz, nby, nbx] = {(nbz, nby, nbx)}")
                keys = torch.nonzero(blocks.reshape(-1)).reshape(-1)
            else:
                keys = torch.unique(blocks.reshape(-1).long())
                if keys.numel() and (int(keys[0]) < 0 or int(keys[-1]) >= virtual):
                    raise ValueError(f"{fn}: block keys must lie in 0 .. {virtual - 1}")
        n = int(keys.numel())
        self.max_blocks = virtual if max_blocks is None else int(max_blocks)
        if n > self.max_blocks:
            raise RuntimeError(f"{fn}: {n} blocks exceed max_blocks = {self.max_blocks}")
        self._color = volume.color is not None
        self._store(max(n, 1 if capacity is None else int(capacity)), dev)
        self._tsdf[:n] = tsdf[keys]
        self._weight[:n] = weight[keys]
        if self._color:
            self._colors[:n] = self._padded(torch.nn.functional.pad(volume.color, pad, value=0.0))[:, keys].permute(1, 0, 2)
        self.keys = keys.to(torch.int32)
        self.slots = torch.arange(n, dtype=torch.int32, device=dev)
        self._marks = torch.empty(virtual, dtype=torch.uint8, device=dev).zero_()
        self._marks[keys] = 2
        return self

    # ------------------------------------------------------------------ extraction
    def extract(self, min_weight=0.0, pass_blocks=MAX_EXTRACT_BLOCKS):
        """-> (vertices [Nv, 3] float32, faces [Nf, 3] int32, colors [Nv, 3] float32 or None) on the device.  The two
        compactions run in passes of at most pass_blocks (<= 349525) blocks in key order, one host read per pass and
        compaction: two host reads for a volume of up to 349525 blocks.  Whatever pass_blocks, the result is the same bits."""
        fn = "SparseTSDFVolume.extract"
        min_weight = float(min_weight)
        if math.isnan(min_weight):
            raise ValueError(f"{fn}: min_weight is NaN")
        pass_blocks = int(pass_blocks)
        if not 1 <= pass_blocks <= MAX_EXTRACT_BLOCKS:
            raise ValueError(f"{fn}: pass_blocks {pass_blocks} is not in 1 .. {MAX_EXTRACT_BLOCKS} (6144 slots per block, below 2^31 per pass)")
        nb = self.num_blocks
        nx, ny, nz = self.dims
        dev = self.device
        empty = lambda dt: torch.zeros(0, 3, dtype=dt, device=dev)
        none = (empty(torch.float32), empty(torch.int32), None if self._colors is None else empty(torch.float32))
        if nb == 0:
            return none
        table = torch.empty(nb, 27, dtype=torch.int32, device=dev)
        _C.family_call("scr_tsdfs_neighbors", nx, ny, nz, nb, self.keys, table, device=dev)
        passes = [(first, min(pass_blocks, nb - first)) for first in range(0, nb, pass_blocks)]
        scratch = _C.scratch(_C.lib.scr_tsdfs_extract_scratch_bytes(passes[0][1]), dev)
        count = ctypes.c_int64(0)
        held = (self.keys, self.slots, table, self._tsdf, self._weight)
        join = lambda parts: parts[0] if len(parts) == 1 else torch.cat(parts)
        ids, vertices, colors = [], [], []
        for first, n in passes:
            _C.family_call("scr_tsdfs_extract_vertices_plan", nx, ny, nz, nb, first, n, *held, min_weight, scratch, ctypes.byref(count), device=dev)
            nv = count.value
            if nv == 0:
                continue
            if sum(t.shape[0] for t in ids) + nv >= 2 ** 31:
                raise ValueError(f"{fn}: the vertex count is not below 2^31")
            ids.append(torch.empty(nv, dtype=torch.int64, device=dev))
            vertices.append(torch.empty(nv, 3, dtype=torch.float32, device=dev))
            colors.append(None if self._colors is None else torch.empty(nv, 3, dtype=torch.float32, device=dev))
            _C.family_call("scr_tsdfs_extract_vertices_run", nx, ny, nz, _C.host_array(self.lo, _C.f32), self.voxel_size, nb, first, n, *held,
                           self._colors, min_weight, scratch, nv, ids[-1], vertices[-1], colors[-1], device=dev)
        if not ids:
            return none
        ids, vertices, colors = join(ids), join(vertices), None if self._colors is None else join(colors)
        nv = ids.shape[0]
        faces = []
        for first, n in passes:
            _C.family_call("scr_tsdfs_extract_faces_plan", nx, ny, nz, nb, first, n, *held, min_weight, scratch, ctypes.byref(count), device=dev)
            nf = count.value
            if nf == 0:
                continue
            if sum(t.shape[0] for t in faces) + nf >= 2 ** 31:
                raise ValueError(f"{fn}: the face count is not below 2^31")
            faces.append(torch.empty(nf, 3, dtype=torch.int32, device=dev))
            _C.family_call("scr_tsdfs_extract_faces_run", nx, ny, nz, nb, first, n, *held, min_weight, scratch, nv, ids, nf, faces[-1], device=dev)
        return vertices, join(faces) if faces else empty(torch.int32), colors
