"""The definitions of splatco_amd.mesh (include/splatco_mesh.h) restated in plain numpy and Python: what the kernels are tested
against, and the mesh recipes the tests share.

Components.  Two vertices are connected when some face contains both (vertex connectivity; Open3D clusters triangles by shared
edges).  labels[v] = the smallest vertex index of v's component; an unreferenced vertex is a component of its own; roots = the
vertices with labels[v] == v, ascending; face_counts[c] = the number of faces whose FIRST index lies in component roots[c].
Degenerate faces count as faces.

Size filter.  t = max(1, min_faces or 1, k), k = the keep_largest-th largest face count, taken only when keep_largest is given
and Nc >= keep_largest.  A component is kept when its face count >= t; kept vertices and faces keep their order; faces are
re-indexed; unreferenced vertices (count 0 < t) always go.

Vertex normals.  For vertex v: the sum over the faces containing v, in ascending face index, each face once, of
(p1 - p0) x (p2 - p0) in float64 (every product and difference rounded on its own), divided by sqrt((x x + y y) + z z), rounded
to float32 once; (0, 0, 0) where the sum is zero or not finite, or the vertex has no face."""
import numpy as np


# ------------------------------------------------------------------ the definitions
def components_ref(faces, nv):
    """-> (labels [nv] int32, roots [nc] int32, face_counts [nc] int32): union-find in Python, then the smallest index."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    parent = list(range(nv))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in faces.tolist():
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    labels = np.array([find(v) for v in range(nv)], np.int32).reshape(nv)
    roots = np.nonzero(labels == np.arange(nv))[0].astype(np.int32)
    per_vertex = np.bincount(labels[faces[:, 0]], minlength=nv) if len(faces) else np.zeros(nv, np.int64)
    return labels, roots, per_vertex[roots].astype(np.int32)


def threshold_ref(face_counts, keep_largest=None, min_faces=None):
    t = max(1, min_faces or 1)
    if keep_largest is not None and len(face_counts) >= keep_largest:
        t = max(t, int(np.sort(np.asarray(face_counts))[::-1][keep_largest - 1]))
    return t


def clean_ref(vertices, faces, colors=None, keep_largest=None, min_faces=None):
    """-> (vertices, faces int32, colors or None, info) as splatco_amd.mesh.clean_mesh returns them."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    nv, nf = len(vertices), len(faces)
    labels, roots, counts = components_ref(faces, nv)
    t = threshold_ref(counts, keep_largest, min_faces)
    info = dict(components=len(roots), components_kept=int((counts >= t).sum()), threshold=t, vertices_before=nv, vertices_after=0,
                faces_before=nf, faces_after=0)
    if nv == 0 or nf == 0:
        info.update(components=nv if nf == 0 else 0, components_kept=0)
        return vertices[:0], np.zeros((0, 3), np.int32), None if colors is None else np.asarray(colors, np.float32)[:0], info
    per_vertex = np.zeros(nv, np.int64)
    per_vertex[roots] = counts
    keep_v = per_vertex[labels] >= t
    keep_f = keep_v[faces[:, 0]]
    remap = np.cumsum(keep_v) - 1
    info.update(vertices_after=int(keep_v.sum()), faces_after=int(keep_f.sum()))
    return (vertices[keep_v], remap[faces[keep_f]].astype(np.int32).reshape(-1, 3),
            None if colors is None else np.asarray(colors, np.float32)[keep_v], info)


def normals_ref(vertices, faces):
    """-> [nv, 3] float32.  np.add.at applies its updates in index order, i.e. in ascending face index per vertex."""
    p = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    acc = np.zeros((len(p), 3), np.float64)
    with np.errstate(all="ignore"):
        if len(faces):
            p0, p1, p2 = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
            u, w = p1 - p0, p2 - p0
            c = np.stack((u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]),
                         axis=1)
            f = np.arange(len(faces))
            second = faces[:, 1] != faces[:, 0]
            third = (faces[:, 2] != faces[:, 0]) & (faces[:, 2] != faces[:, 1])
            # one pass per corner would add a vertex's faces corner by corner; merge the three lists by face index instead
            idx = np.concatenate((faces[:, 0], faces[second, 1], faces[third, 2]))
            fid = np.concatenate((f, f[second], f[third]))
            order = np.argsort(fid, kind="stable")
            for ch in range(3):
                np.add.at(acc[:, ch], idx[order], c[fid[order], ch])
        norm = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
        ok = np.isfinite(acc).all(1) & np.isfinite(norm) & (norm > 0)
        out = np.where(ok[:, None], acc / np.where(ok, norm, 1.0)[:, None], 0.0)
    return out.astype(np.float32)


def normals_loop_ref(vertices, faces):
    """The same in a Python loop, face by face (small meshes: what normals_ref's np.add.at is checked against)."""
    p = [[float(x) for x in row] for row in np.asarray(vertices, np.float32).reshape(-1, 3)]
    acc = [[0.0, 0.0, 0.0] for _ in p]
    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        u = [p[b][k] - p[a][k] for k in range(3)]
        w = [p[c][k] - p[a][k] for k in range(3)]
        n = (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])
        for v in dict.fromkeys((a, b, c)):
            for k in range(3):
                acc[v][k] += n[k]
    out = np.zeros((len(p), 3), np.float32)
    for v, (x, y, z) in enumerate(acc):
        norm = float(np.sqrt(np.float64((x * x + y * y) + z * z)))
        if np.isfinite([x, y, z, norm]).all() and norm > 0:
            out[v] = [np.float32(x / norm), np.float32(y / norm), np.float32(z / norm)]
    return out


# ------------------------------------------------------------------ mesh recipes
TETRA = (4, [(0, 1, 2), (0, 3, 1), (1, 3, 2), (0, 2, 3)])
STRIP = (6, [(0, 1, 2), (1, 3, 2), (2, 3, 4), (3, 5, 4)])                          # open
TRIANGLE = (3, [(0, 1, 2)])
DEGENERATE = (1, [(0, 0, 0)])                                                     # one face on one vertex
TEMPLATES = (TETRA, STRIP, TRIANGLE, DEGENERATE)


def assemble(parts, unreferenced=0, seed=0, shuffle=True):
    """Disjoint copies of templates (nv, faces) as ONE mesh, vertex numbering and face order shuffled by `seed`, plus
    `unreferenced` vertices no face uses.  -> (vertices float32 [Nv, 3], faces int32 [Nf, 3], part [Nv] int: the copy a vertex
    came from, -1 for an unreferenced one, faces_of_part [len(parts)])."""
    gen = np.random.default_rng(seed)
    faces, part = [], []
    base = 0
    for i, (nv, fs) in enumerate(parts):
        faces += [(a + base, b + base, c + base) for a, b, c in fs]
        part += [i] * nv
        base += nv
    part = np.array(part + [-1] * unreferenced, np.int64)
    nv = len(part)
    faces = np.array(faces, np.int64).reshape(-1, 3)
    if shuffle:
        perm = gen.permutation(nv)                       # old index -> new index
        faces = perm[faces][gen.permutation(len(faces))] if len(faces) else faces
        new_part = np.empty_like(part)
        new_part[perm] = part
        part = new_part
    vertices = gen.uniform(-1.0, 1.0, size=(nv, 3)).astype(np.float32)
    return vertices, faces.astype(np.int32).reshape(-1, 3), part, np.array([len(fs) for _, fs in parts], np.int64)


def labels_by_construction(part):
    """What the definition gives for a mesh of assemble(): the smallest vertex index of each copy; unreferenced: itself."""
    part = np.asarray(part)
    labels = np.arange(len(part), dtype=np.int32)
    for i in np.unique(part[part >= 0]):
        members = np.nonzero(part == i)[0]
        labels[members] = members.min()
    return labels


def mixed_mesh(n_parts, unreferenced, seed):
    """n_parts copies of the four templates in turn."""
    return assemble([TEMPLATES[i % 4] for i in range(n_parts)], unreferenced, seed)


def deep_strip(n_tri):
    """An open strip of n_tri triangles over n_tri + 2 vertices whose numbering makes a hooking union-find build a deep tree:
    position k along the strip carries index k // 2 for even k and Nv - 1 - k // 2 for odd k (descending and interleaved),
    faces listed from the strip's far end."""
    nv = n_tri + 2
    k = np.arange(nv)
    index = np.where(k % 2 == 0, k // 2, nv - 1 - k // 2)
    faces = np.stack((index[:-2], index[1:-1], index[2:]), axis=1)[::-1]
    gen = np.random.default_rng(11)
    return gen.uniform(-1, 1, size=(nv, 3)).astype(np.float32), np.ascontiguousarray(faces, np.int32)


def octahedron():
    v = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float32)
    f = np.array([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], np.int32)
    return v, f


def fan(n, seed=4):
    """A vertex of degree n (> 64 wanted): n triangles around vertex 0 on a bumpy disc."""
    gen = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n) / n
    rim = np.stack((np.cos(ang), np.sin(ang), 0.2 * gen.standard_normal(n)), axis=1)
    v = np.concatenate((np.array([[0.0, 0.0, 0.3]]), rim)).astype(np.float32)
    i = np.arange(n)
    f = np.stack((np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n), axis=1)
    return v, f.astype(np.int32)


# ------------------------------------------------------------------ the end-to-end scene
def blob_scene(dims=(40, 40, 40), h=0.06, n_views=24, H=160, W=160):
    """Two spheres of different size and one tiny blob, far enough apart that their truncation bands do not meet, seen from
    n_views cameras around the volume through tsdf_ref's pinhole conventions (pixel centres; depth = alpha z, alpha = 1 on a
    hit and 0 elsewhere).  -> (views for tsdf_ref.integrate_views_ref / TSDFVolume.integrate_views, lo float32 [3], h float32,
    dims, [(centre, radius)] largest first)."""
    import math
    import tsdf_ref as T
    h = np.float32(h)
    ext = float(h) * (np.array(dims) - 1)
    lo = (-0.5 * ext + float(h) * np.array([0.13, -0.21, 0.07])).astype(np.float32)
    mid = lo.astype(np.float64) + 0.5 * ext
    blobs = [(mid + np.array([-0.42, -0.30, 0.02]), 0.50), (mid + np.array([0.60, 0.52, 0.14]), 0.29),
             (mid + np.array([0.55, -0.72, -0.50]), 0.10)]
    intr = T.intrinsics_fov(H, W)
    fx, fy, cx, cy = intr
    views = []
    for i in range(n_views):
        ang = 2.0 * math.pi * (i + 0.3) / n_views
        eye = mid + 3.0 * np.array([math.cos(ang), math.sin(ang), 0.9 * math.sin(2.5 * ang + 0.4)])
        w2c = T.look_at(eye, mid)
        R, t = w2c[:3, :3], w2c[:3, 3]
        origin = -R.T @ t
        px, py = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
        ray = np.stack(((px - cx) / fx, (py - cy) / fy, np.ones_like(px)), axis=-1) @ R
        z = np.full((H, W), np.inf)
        for c, r in blobs:
            oc = origin - c
            a, b, cc = (ray * ray).sum(-1), 2.0 * (ray @ oc), oc @ oc - r * r
            disc = b * b - 4 * a * cc
            with np.errstate(all="ignore"):
                ts = np.where(disc > 0, (-b - np.sqrt(np.abs(disc))) / (2 * a), np.inf)
            z = np.minimum(z, np.where(ts > 0, ts, np.inf))
        hit = np.isfinite(z)
        views.append(dict(depth=np.where(hit, z, 0.0).astype(np.float32), alpha=hit.astype(np.float32), image=None, mask=None,
                          intr=intr, w2c=w2c))
    return views, lo, h, tuple(dims), blobs


def sized_mesh(n, seed):
    """A mesh with Nv = Nf = n exactly: tetrahedra (4 vertices, 4 faces) and single degenerate faces (1, 1), shuffled."""
    k = n // 6
    return assemble([TETRA] * k + [DEGENERATE] * (n - 4 * k), 0, seed)


def triangle_soup(n_tri, unreferenced, seed):
    """n_tri single-triangle components under a random vertex numbering, plus unreferenced vertices; everything the
    definition gives follows from the construction.  -> (vertices, faces int32, labels int32)."""
    gen = np.random.default_rng(seed)
    nv = 3 * n_tri + unreferenced
    perm = gen.permutation(nv).astype(np.int32)
    faces = perm[:3 * n_tri].reshape(n_tri, 3)
    labels = np.arange(nv, dtype=np.int32)
    labels[faces.reshape(-1)] = np.repeat(faces.min(1), 3)
    return gen.uniform(-1.0, 1.0, size=(nv, 3)).astype(np.float32), np.ascontiguousarray(faces), labels
