"""Clean-up of an indexed triangle mesh on the device: connected components, the size filter of 2DGS's post_process_mesh, and
vertex normals (host side of csrc/mesh.hip).

What 2DGS, PGSR, GOF and DN-Splatter run right after the TSDF extraction, without Open3D or scipy.  The definition (normative;
include/splatco_mesh.h and tests/mesh_ref.py restate it):

Components.  Two vertices are connected when some face contains both: VERTEX connectivity.  (Open3D's
cluster_connected_triangles clusters triangles by shared EDGES, so two shells that touch in a single vertex are one component
here and two there.)  labels[v] (int32 [Nv]) is the smallest vertex index of v's component; a vertex that no face references is
a component of its own with 0 faces; roots (int32 [Nc]) lists the vertices with labels[v] == v in ascending order;
face_counts[c] (int32) is the number of faces whose first index lies in component roots[c].  Degenerate faces (repeated
indices) are legal and count as faces.  Every output is an integer that the definition fixes uniquely.

Size filter.  t = max(1, min_faces or 1, k), k the keep_largest-th largest value of face_counts, taken only when keep_largest
is given and Nc >= keep_largest (2DGS's semantics: ties at the K-th place are all kept).  A component is kept when its face
count is >= t; a vertex or a face is kept when its component is.  Kept vertices and faces keep their relative order, faces are
re-indexed, positions and colours are copied bit for bit.  Vertices that no face references are always dropped.

Vertex normals.  For vertex v the sum, over the faces containing v in ascending face index (a face that contains v twice is
added once), of (p1 - p0) x (p2 - p0), in binary64 in the written order, divided by its binary64 norm sqrt((x x + y y) + z z)
and rounded to float32 once; exactly (0, 0, 0) where the sum is zero or not finite or the vertex has no face.  No atomics: the
same bits run after run.

    labels, roots, face_counts = connected_components(faces, num_vertices)
    vertices, faces, colors, info = clean_mesh(vertices, faces, colors, keep_largest=50, min_faces=50)
    normals = vertex_normals(vertices, faces)
    scene_io.write_ply_mesh("mesh.ply", vertices, faces, colors, normals=normals)

Not built: decimation, smoothing, edge-connectivity clustering, texture baking.

Every launch goes through _C.family_call.  There is no CPU path: a CPU tensor is a ValueError.  The face indices are checked
against [0, Nv) before anything is launched (one aminmax, one host read): the kernels index with them."""
import ctypes

import torch

from . import _C


def _device_only(fn, name, t):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{fn}: {name} is not a tensor")
    if not t.is_cuda:
        raise ValueError(f"{fn}: {name} is on {t.device}; the mesh operators run on the GPU and there is no CPU path")


def _count(fn, name, x, least):
    if x is None:
        return None
    if isinstance(x, bool) or not isinstance(x, int) or x < least:
        raise ValueError(f"{fn}: {name} = {x!r} must be an int >= {least} or None")
    return x


def _faces_shape(fn, faces, nv):
    if not isinstance(faces, torch.Tensor):
        raise ValueError(f"{fn}: faces is not a tensor")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{fn}: faces {tuple(faces.shape)} {faces.dtype} is not an int32 or int64 [Nf, 3] tensor")
    if isinstance(nv, bool) or not isinstance(nv, int) or not 0 <= nv < 2 ** 31:
        raise ValueError(f"{fn}: num_vertices = {nv!r} must be an int in 0 .. 2^31 - 1")
    if 3 * faces.shape[0] >= 2 ** 31:
        raise ValueError(f"{fn}: 3 Nf = {3 * faces.shape[0]} is not below 2^31")


def _vertices_shape(fn, vertices, colors):
    for name, t in (("vertices", vertices), ("colors", colors)):
        if t is None and name == "colors":
            continue
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{fn}: {name} is not a tensor")
        if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32:
            raise ValueError(f"{fn}: {name} {tuple(t.shape)} {t.dtype} is not a float32 [Nv, 3] tensor")
    if vertices.shape[0] >= 2 ** 31:
        raise ValueError(f"{fn}: Nv = {vertices.shape[0]} is not below 2^31")
    if colors is not None and colors.shape[0] != vertices.shape[0]:
        raise ValueError(f"{fn}: {colors.shape[0]} colors for {vertices.shape[0]} vertices")


def _faces_on_device(fn, faces, nv, like=None):
    """The faces as contiguous int32 on their device, after the device checks and, last, the index range: one host read, and
    the only thing between a bad mesh and an out-of-bounds access."""
    _device_only(fn, "faces", faces)
    if like is not None and faces.device != like.device:
        raise ValueError(f"{fn}: faces is on {faces.device}, vertices on {like.device}")
    if faces.shape[0]:
        lo, hi = (int(x) for x in torch.stack(torch.aminmax(faces.detach())).tolist())
        if lo < 0 or hi >= nv:
            raise ValueError(f"{fn}: face indices span {lo} .. {hi}, outside [0, {nv})")
    return faces.detach().to(torch.int32).contiguous()


def _check_mesh(fn, vertices, faces, colors=None):
    """Shapes, dtypes and sizes first, devices next, the index range last.  -> (vertices, faces int32, colors), contiguous."""
    _vertices_shape(fn, vertices, colors)
    _faces_shape(fn, faces, vertices.shape[0])
    _device_only(fn, "vertices", vertices)
    if colors is not None:
        _device_only(fn, "colors", colors)
        if colors.device != vertices.device:
            raise ValueError(f"{fn}: colors is on {colors.device}, vertices on {vertices.device}")
    faces = _faces_on_device(fn, faces, vertices.shape[0], vertices)
    return vertices.detach().contiguous(), faces, None if colors is None else colors.detach().contiguous()


def _components(faces, nv):
    """faces: checked int32 [Nf, 3].  -> (labels [Nv], vertex_faces [Nv], roots [Nc], face_counts [Nc], scratch)."""
    dev, nf = faces.device, faces.shape[0]
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    scratch = _C.scratch(_C.lib.scr_mesh_scratch_bytes(nv, nf), dev)
    if nv == 0:
        return i32(0), i32(0), i32(0), i32(0), scratch
    parent, labels, vertex_faces, status = i32(nv), i32(nv), i32(nv), i32(1)
    _C.family_call("scr_mesh_components", nv, nf, faces if nf else None, parent, labels, vertex_faces, status, device=dev)
    count = ctypes.c_int64(0)
    _C.family_call("scr_mesh_roots_plan", nv, labels, status, scratch, ctypes.byref(count), device=dev)    # RuntimeError: status
    nc = count.value
    roots, face_counts = i32(nc), i32(nc)
    _C.family_call("scr_mesh_roots_run", nv, labels, vertex_faces, scratch, nc, roots, face_counts, device=dev)
    return labels, vertex_faces, roots, face_counts, scratch


def connected_components(faces, num_vertices):
    """-> (labels [Nv] int32, roots [Nc] int32, face_counts [Nc] int32) on the device (see the module's definition).
    faces: [Nf, 3] int32 or int64 on the GPU, every index in [0, num_vertices).  Two host reads: the index range and Nc."""
    _faces_shape("connected_components", faces, num_vertices)
    faces = _faces_on_device("connected_components", faces, num_vertices)
    labels, _, roots, face_counts, _ = _components(faces, num_vertices)
    return labels, roots, face_counts


def clean_mesh(vertices, faces, colors=None, keep_largest=None, min_faces=None):
    """Drop the components with fewer than t = max(1, min_faces or 1, the keep_largest-th largest face count) faces, and every
    vertex that no face references.  -> (vertices [Nv', 3] float32, faces [Nf', 3] int32, colors [Nv', 3] float32 or None, info)
    on the device; info: components, components_kept, threshold, vertices_before, vertices_after, faces_before, faces_after.
    The result may be empty ([0, 3] tensors)."""
    fn = "clean_mesh"
    keep_largest, min_faces = _count(fn, "keep_largest", keep_largest, 1), _count(fn, "min_faces", min_faces, 0)
    vertices, faces, colors = _check_mesh(fn, vertices, faces, colors)
    dev, nv, nf = vertices.device, vertices.shape[0], faces.shape[0]
    empty = lambda dt: torch.zeros(0, 3, dtype=dt, device=dev)
    base = max(1, min_faces or 1)
    info = {"components": nv if nf == 0 else 0, "components_kept": 0, "threshold": base, "vertices_before": nv, "vertices_after": 0,
            "faces_before": nf, "faces_after": 0}
    if nv == 0 or nf == 0:
        return empty(torch.float32), empty(torch.int32), None if colors is None else empty(torch.float32), info
    labels, vertex_faces, roots, face_counts, scratch = _components(faces, nv)
    nc = roots.shape[0]
    # the K-th largest count and the number of kept components: one host read for both
    if keep_largest is not None and nc >= keep_largest:
        kth = torch.topk(face_counts, keep_largest, sorted=True).values[-1].to(torch.int64)
    else:
        kth = torch.zeros((), dtype=torch.int64, device=dev)
    kth, kept = (int(x) for x in torch.stack((kth, (face_counts.to(torch.int64) >= torch.clamp(kth, min=base)).sum())).tolist())
    t = max(base, kth)
    info.update(components=nc, components_kept=kept, threshold=t)
    if t >= 2 ** 31:
        return empty(torch.float32), empty(torch.int32), None if colors is None else empty(torch.float32), info
    count = ctypes.c_int64(0)
    _C.family_call("scr_mesh_vertices_plan", nv, labels, vertex_faces, t, scratch, ctypes.byref(count), device=dev)
    nv2 = count.value
    if nv2 == 0:
        return empty(torch.float32), empty(torch.int32), None if colors is None else empty(torch.float32), info
    out_v = torch.empty(nv2, 3, dtype=torch.float32, device=dev)
    out_c = None if colors is None else torch.empty(nv2, 3, dtype=torch.float32, device=dev)
    remap = torch.empty(nv, dtype=torch.int32, device=dev)
    _C.family_call("scr_mesh_vertices_run", nv, labels, vertex_faces, t, scratch, nv2, vertices, colors, out_v, out_c, remap, device=dev)
    _C.family_call("scr_mesh_faces_plan", nf, faces, labels, vertex_faces, t, scratch, ctypes.byref(count), device=dev)
    nf2 = count.value
    out_f = torch.empty(nf2, 3, dtype=torch.int32, device=dev)
    _C.family_call("scr_mesh_faces_run", nf, faces, labels, vertex_faces, t, scratch, nf2, remap, out_f, device=dev)
    info.update(vertices_after=nv2, faces_after=nf2)
    return out_v, out_f, out_c, info


def normal_keys(faces, num_vertices):
    """The sorted int64 keys v Nf + f [3 Nf] of scr_mesh_vertex_normals: one per (face, distinct index of the face), and the
    value Nv Nf, which follows every real key, in the slots that within-face duplicates leave over.  No host read."""
    nf = faces.shape[0]
    f = torch.arange(nf, dtype=torch.int64, device=faces.device)
    i0, i1, i2 = (faces[:, e].to(torch.int64) for e in range(3))
    last = num_vertices * nf
    k0 = i0 * nf + f
    k1 = torch.where(i1 != i0, i1 * nf + f, last)
    k2 = torch.where((i2 != i0) & (i2 != i1), i2 * nf + f, last)
    return torch.sort(torch.cat((k0, k1, k2))).values


def vertex_normals(vertices, faces):
    """-> normals [Nv, 3] float32 on the device: area-weighted, binary64 inside, unit length or exactly 0 (see the module's
    definition).  One host read (the index range)."""
    fn = "vertex_normals"
    vertices, faces, _ = _check_mesh(fn, vertices, faces)
    dev, nv, nf = vertices.device, vertices.shape[0], faces.shape[0]
    if nv == 0:
        return torch.zeros(0, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    keys = normal_keys(faces, nv) if nf else None
    _C.family_call("scr_mesh_vertex_normals", nv, nf, vertices, faces if nf else None, keys, normals, device=dev)
    return normals
