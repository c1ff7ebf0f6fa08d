"""The definition of splatco_amd.tsdf (include/splatco_tsdf.h) restated in numpy float64, one loop-free function per step: what
the host and GPU tests of the TSDF family compare against, the input recipe they share and the mesh checks they run.

Volume: nodes p(i, j, k) = lo + h (i, j, k), linear index n = (k ny + j) nx + i, tsdf / weight [nz, ny, nx] float32, colour
[3, nz, ny, nx] float32; lo, h float32 VALUES, every operation between the float32 inputs and the float32 outputs binary64 in
the written order.  integrate_ref applies ONE view, extract_ref is marching tetrahedra at level 0 on the six Kuhn tetrahedra of
every valid cube.  The only Python loops here run over the 6 x 16 cases of a tetrahedron (tables built at import) and over the
views of a list."""
import itertools
import math

import numpy as np

EDGE_OFFSETS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)], dtype=np.int64)
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]        # lexicographic: xyz xzy yxz yzx zxy zyx
_DIR = {tuple(o): d for d, o in enumerate(EDGE_OFFSETS.tolist())}


def tet_nodes(q):
    """[4, 3] node offsets of Kuhn tetrahedron q inside its cube: corner, + e_pi1, + e_pi2, corner + (1, 1, 1)."""
    v = np.zeros((4, 3), dtype=np.int64)
    for m, axis in enumerate(PERMS[q]):
        v[m + 1] = v[m]
        v[m + 1, axis] += 1
    return v


def _case_triangles(inside):
    """The triangles of one tetrahedron before winding: lists of three local edges (x, y), x < y."""
    ins = [m for m in range(4) if inside[m]]
    out = [m for m in range(4) if not inside[m]]
    e = lambda x, y: (min(x, y), max(x, y))
    if len(ins) == 1:
        a = ins[0]
        return [[e(a, out[0]), e(a, out[1]), e(a, out[2])]]
    if len(ins) == 3:
        a = out[0]
        return [[e(a, ins[0]), e(a, ins[1]), e(a, ins[2])]]
    if len(ins) == 2:
        (a, b), (c, d) = ins, out
        quad = [e(a, c), e(a, d), e(b, d), e(b, c)]
        return [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return []


def _build_tables():
    """TRI_NODE [6, 16, 2, 3] (local node x of the edge), TRI_DIR (its lattice direction), TRI_USED [6, 16, 2], the winding
    already decided: by the sign of (v1 - v0) x (v2 - v0) . (p_outside - p_inside), evaluated with every vertex at the MIDPOINT
    of its edge and p the centroids of the outside and inside nodes.  The sign does not depend on where on its edge a vertex
    lies (the cut is a plane section of the tetrahedron, and it never degenerates while inside values are < 0 <= outside), so
    the midpoints decide it without the zero-area triangles that a vertex sitting on a node produces."""
    node = np.zeros((6, 16, 2, 3), dtype=np.int64)
    dirs = np.zeros((6, 16, 2, 3), dtype=np.int64)
    used = np.zeros((6, 16, 2), dtype=bool)
    flip = np.zeros((6, 16), dtype=bool)
    for q in range(6):
        v = tet_nodes(q).astype(np.float64)
        for mask in range(16):
            inside = [(mask >> m) & 1 for m in range(4)]
            tris = _case_triangles(inside)
            if not tris:
                continue
            p_in = np.mean([v[m] for m in range(4) if inside[m]], axis=0)
            p_out = np.mean([v[m] for m in range(4) if not inside[m]], axis=0)
            for t, tri in enumerate(tris):
                mid = [0.5 * (v[x] + v[y]) for x, y in tri]
                s = float(np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), p_out - p_in))
                assert abs(s) > 1e-9
                if s < 0:
                    tri = [tri[0], tri[2], tri[1]]
                    flip[q, mask] = True
                else:
                    assert not (t == 1 and flip[q, mask]), "both triangles of a quad wind alike"
                for m, (x, y) in enumerate(tri):
                    node[q, mask, t, m] = x
                    dirs[q, mask, t, m] = _DIR[tuple((tet_nodes(q)[y] - tet_nodes(q)[x]).tolist())]
                used[q, mask, t] = True
    return node, dirs, used, flip


TRI_NODE, TRI_DIR, TRI_USED, TRI_FLIP = _build_tables()
TET_NODES = np.stack([tet_nodes(q) for q in range(6)])                            # [6, 4, 3]


# ------------------------------------------------------------------ the volume
def fresh(dims, color=True):
    nx, ny, nz = dims
    return dict(tsdf=np.ones((nz, ny, nx), np.float32), weight=np.zeros((nz, ny, nx), np.float32),
                color=np.zeros((3, nz, ny, nx), np.float32) if color else None)


def node_positions(lo, h, dims):
    """[nz, ny, nx, 3] float64: lo + h (i, j, k), lo and h taken as float32 values."""
    nx, ny, nz = dims
    lo = np.asarray(lo, np.float32).astype(np.float64)
    h = float(np.float32(h))
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack((lo[0] + h * i, lo[1] + h * j, lo[2] + h * k), axis=-1)


def project(p, intr, w2c):
    """(pc.x, pc.y, zc, u, v) float64 of the points p [..., 3]; rows left to right; u, v NaN-free only where zc > 0."""
    fx, fy, cx, cy = (float(x) for x in intr)
    M = np.asarray(w2c, np.float64)
    row = lambda r: ((M[r, 0] * p[..., 0] + M[r, 1] * p[..., 1]) + M[r, 2] * p[..., 2]) + M[r, 3]
    x, y, z = row(0), row(1), row(2)
    with np.errstate(all="ignore"):
        u = fx * x / z + cx
        v = fy * y / z + cy
    return x, y, z, u, v


def mask_positive(mask, shape):
    if mask is None:
        return np.ones(shape, bool)
    mask = np.asarray(mask)
    return (mask > 0) if mask.dtype.kind == "f" else (mask != 0)


def integrate_ref(vol, lo, h, depth, alpha, intr, w2c, trunc, image=None, mask=None, min_alpha=0.5, near=0.05, max_weight=255.0,
                  details=False):
    """One view into the volume dict (tsdf, weight, color): returns a new dict.  details=True: also the per-node float64
    quantities the tests' exclusions are made of."""
    nz, ny, nx = vol["tsdf"].shape
    H, W = depth.shape
    D, A = np.asarray(depth, np.float32), np.asarray(alpha, np.float32)
    p = node_positions(lo, h, (nx, ny, nz))
    _, _, zc, u, v = project(p, intr, w2c)
    front = zc > float(near)
    with np.errstate(all="ignore"):
        fu, fv = np.floor(u), np.floor(v)
        inimg = front & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
    px = np.where(inimg, fu, 0).astype(np.int64)
    py = np.where(inimg, fv, 0).astype(np.int64)
    d_, a_ = D[py, px], A[py, px]
    ok = inimg & np.isfinite(d_) & np.isfinite(a_) & (a_ >= np.float32(min_alpha)) & (d_ > 0) & mask_positive(mask, (H, W))[py, px]
    with np.errstate(all="ignore"):
        z = (np.where(ok, d_, np.float32(1)) / np.where(ok, a_, np.float32(1))).astype(np.float32).astype(np.float64)
    sdf = z - zc
    trunc = float(trunc)
    upd = ok & ~(sdf < -trunc)
    d = np.minimum(1.0, sdf / trunc)
    Wt = vol["weight"].astype(np.float64)
    w = 1.0
    out = dict(tsdf=np.where(upd, (vol["tsdf"].astype(np.float64) * Wt + d * w) / (Wt + w), vol["tsdf"]).astype(np.float32),
               weight=np.where(upd, np.minimum(Wt + w, float(np.float32(max_weight))), vol["weight"]).astype(np.float32), color=None)
    if vol["color"] is not None:
        out["color"] = vol["color"].copy()
        if image is not None:
            img = np.asarray(image, np.float32)[:, py, px]                         # [3, nz, ny, nx]
            cu = upd & np.isfinite(img).all(0)
            img = np.where(cu, img, np.float32(0)).astype(np.float64)
            out["color"] = np.where(cu, (vol["color"].astype(np.float64) * Wt + img * w) / (Wt + w), vol["color"]).astype(np.float32)
    if details:
        out["details"] = dict(zc=zc, u=u, v=v, front=front, ok=ok, sdf=sdf, upd=upd)
    return out


def fragile_nodes(det, trunc, near):
    """Nodes whose verdicts hang on the last bit of the reference's own u, v, sdf or zc (left out of a comparison)."""
    with np.errstate(all="ignore"):
        near_int = lambda x: np.abs(x - np.rint(x)) < 1e-6
        f = (np.abs(det["zc"] - near) < 1e-6) | (det["front"] & (near_int(det["u"]) | near_int(det["v"])))
        f |= det["ok"] & (np.abs(det["sdf"] + trunc) < 1e-6 * trunc)
    return f


def integrate_views_ref(vol, lo, h, views, trunc, **kw):
    """views: dicts with depth, alpha, intr, w2c and optionally image, mask, near.  Returns (volume, fragile [nz, ny, nx])."""
    fragile = np.zeros(vol["tsdf"].shape, bool)
    for view in views:
        near = view.get("near", kw.get("near", 0.05))
        o = integrate_ref(vol, lo, h, view["depth"], view["alpha"], view["intr"], view["w2c"], trunc, image=view.get("image"),
                          mask=view.get("mask"), details=True, **dict(kw, near=near))
        fragile |= fragile_nodes(o.pop("details"), float(trunc), float(near))
        vol = o
    return vol, fragile


# ------------------------------------------------------------------ extraction
def _shift(a, off):
    """a[k + oz, j + oy, i + ox] over the cube corners (k < nz - 1 ...)."""
    ox, oy, oz = off
    nz, ny, nx = a.shape
    return a[oz:nz - 1 + oz, oy:ny - 1 + oy, ox:nx - 1 + ox]


def valid_cubes(weight, min_weight=0.0):
    ok = weight > np.float32(min_weight)
    corners = [_shift(ok, o) for o in itertools.product((0, 1), repeat=3)]
    return np.logical_and.reduce(corners)


def extract_ref(vol, lo, h, min_weight=0.0):
    """-> dict(vertices [Nv, 3] float32, faces [Nf, 3] int32, colors [Nv, 3] float32 or None, edge_ids [Nv] int64,
    vertices64 / colors64 the unrounded float64 values)."""
    s = vol["tsdf"]
    nz, ny, nx = s.shape
    N = nx * ny * nz
    inside = s < 0
    cubes = valid_cubes(vol["weight"], min_weight)                                   # [nz-1, ny-1, nx-1]
    used = np.zeros((nz, ny, nx, 7), bool)
    for q in range(6):                                                               # 6 x 6 table entries, not data
        tn = TET_NODES[q]
        for x, y in itertools.combinations(range(4), 2):
            ox, oy, oz = tn[x]
            used[oz:nz - 1 + oz, oy:ny - 1 + oy, ox:nx - 1 + ox, _DIR[tuple((tn[y] - tn[x]).tolist())]] |= cubes
    differs = np.zeros((nz, ny, nx, 7), bool)
    for d, (ox, oy, oz) in enumerate(EDGE_OFFSETS.tolist()):
        differs[:nz - oz, :ny - oy, :nx - ox, d] = inside[:nz - oz, :ny - oy, :nx - ox] != inside[oz:, oy:, ox:]
    ids = np.nonzero((used & differs).reshape(-1))[0].astype(np.int64)                # ascending 7 n + dir
    na, d = ids // 7, ids % 7
    ia = np.stack((na % nx, (na // nx) % ny, na // (nx * ny)), axis=1)
    ib = ia + EDGE_OFFSETS[d]
    nb = (ib[:, 2] * ny + ib[:, 1]) * nx + ib[:, 0]
    lo64 = np.asarray(lo, np.float32).astype(np.float64)
    h64 = float(np.float32(h))
    pa, pb = lo64 + h64 * ia, lo64 + h64 * ib
    sa, sb = s.reshape(-1)[na].astype(np.float64), s.reshape(-1)[nb].astype(np.float64)
    t = sa / (sa - sb)
    v64 = pa + (pb - pa) * t[:, None]
    c64 = None
    if vol.get("color") is not None:
        c = vol["color"].reshape(3, N).astype(np.float64)
        c64 = (c[:, na] + (c[:, nb] - c[:, na]) * t).T
    # faces: per cube, tetrahedron, triangle slot
    kc, jc, ic = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    corner = np.stack((ic, jc, kc), axis=-1).reshape(-1, 3)                           # ascending cube index
    tn = corner[:, None, None, :] + TET_NODES[None]                                   # [Nc, 6, 4, 3]
    tlin = (tn[..., 2] * ny + tn[..., 1]) * nx + tn[..., 0]
    mask = (inside.reshape(-1)[tlin] * (1 << np.arange(4))).sum(-1)                   # [Nc, 6]
    qq = np.arange(6)[None, :]
    keep = TRI_USED[qq, mask] & cubes.reshape(-1)[:, None, None]                      # [Nc, 6, 2]
    local = TRI_NODE[qq, mask]                                                        # [Nc, 6, 2, 3]
    ea = np.take_along_axis(tlin[:, :, None, :].repeat(2, 2), local, axis=-1)
    eid = 7 * ea + TRI_DIR[qq, mask]
    eid = eid[keep]                                                                   # [Nf, 3], cube, q, triangle order
    faces = np.searchsorted(ids, eid).astype(np.int32).reshape(-1, 3)
    assert eid.size == 0 or np.array_equal(ids[faces], eid), "a face names an edge that carries no vertex"
    return dict(vertices=v64.astype(np.float32).reshape(-1, 3), faces=faces, edge_ids=ids, vertices64=v64.reshape(-1, 3),
                colors=None if c64 is None else c64.astype(np.float32).reshape(-1, 3), colors64=c64)


# ------------------------------------------------------------------ comparisons and mesh checks
def ulp_distance(a, b):
    """Per element: how many float32 values lie between a and b (0 = same value; -0.0 and 0.0 count as equal)."""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def canonical_faces(faces):
    """Each triple rotated to start at its smallest index (the winding kept), the list sorted."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return f
    r = np.argmin(f, axis=1)
    f = np.stack([np.take_along_axis(f, ((r + m) % 3)[:, None], 1)[:, 0] for m in range(3)], axis=1)
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]


def mesh_report(vertices, faces):
    """dict: V, E, F, euler, duplicate vertices, unreferenced vertices, degenerate index triples, boundary (directed edges with
    no opposite, [Nb, 2]), nonmanifold (directed edges that occur twice), signed volume."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = v.shape[0]
    de = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))
    key = de[:, 0] * max(V, 1) + de[:, 1]
    opp = de[:, 1] * max(V, 1) + de[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    und = np.unique(np.minimum(key, opp))
    vol = float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0) if len(f) else 0.0
    return dict(V=V, E=len(und), F=len(f), euler=V - len(und) + len(f),
                duplicates=V - len(np.unique(v.astype(np.float32).view(np.int32).reshape(-1, 3), axis=0)) if V else 0,
                unreferenced=V - len(np.unique(f)), degenerate=int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum()),
                boundary=de[~np.isin(opp, uniq)], nonmanifold=int((counts > 1).sum()), volume=vol)


def assert_closed_manifold(vertices, faces):
    r = mesh_report(vertices, faces)
    assert r["F"] > 0 and r["nonmanifold"] == 0 and len(r["boundary"]) == 0, (r["nonmanifold"], len(r["boundary"]))
    assert r["euler"] == 2, r["euler"]
    assert r["unreferenced"] == 0 and r["degenerate"] == 0
    return r


def on_lattice_edges(vertices, edge_ids, lo, h, dims, tol):
    """Largest distance of a vertex from the segment of its lattice edge."""
    nx, ny, nz = dims
    ids = np.asarray(edge_ids, np.int64)
    na, d = ids // 7, ids % 7
    ia = np.stack((na % nx, (na // nx) % ny, na // (nx * ny)), axis=1)
    lo64, h64 = np.asarray(lo, np.float32).astype(np.float64), float(np.float32(h))
    pa, pb = lo64 + h64 * ia, lo64 + h64 * (ia + EDGE_OFFSETS[d])
    v = np.asarray(vertices, np.float64)
    ab = pb - pa
    t = np.einsum("ij,ij->i", v - pa, ab) / np.einsum("ij,ij->i", ab, ab)
    off = np.linalg.norm(v - (pa + ab * t[:, None]), axis=1)
    assert ((t >= -tol) & (t <= 1 + tol)).all()
    return float(off.max()) if len(off) else 0.0


def sphere_volume(dims=(24, 24, 24), h=0.05, radius_cells=8.0, slab=None):
    """The analytic test volume: tsdf = clamp((|p - c| - r) / trunc, -1, 1), trunc = 4 h, weight 1 (0 on the nodes of `slab`,
    a slice of i), a colour that is linear in p.  Returns (vol, lo, h, centre, r)."""
    lo = np.array([-0.61, -0.57, -0.63], np.float32)
    h = np.float32(h)
    p = node_positions(lo, h, dims)
    centre = lo.astype(np.float64) + float(h) * (np.array(dims) - 1) * 0.5 + float(h) * np.array([0.137, -0.211, 0.319])
    r = radius_cells * float(h)
    tsdf = np.clip((np.linalg.norm(p - centre, axis=-1) - r) / (4.0 * float(h)), -1.0, 1.0).astype(np.float32)
    weight = np.ones_like(tsdf)
    if slab is not None:
        weight[:, :, slab] = 0.0
    color = np.moveaxis(((p - lo.astype(np.float64)) / (float(h) * np.array(dims))), -1, 0).astype(np.float32)
    return dict(tsdf=tsdf, weight=weight, color=np.ascontiguousarray(color)), lo, h, centre, r


# ------------------------------------------------------------------ the scene recipe
def look_at(eye, target, down=(0.0, 0.0, -1.0)):
    """World-to-camera [4, 4] of a COLMAP camera (+x right, +y down, +z forward), its entries rounded to float32 values."""
    eye, target, down = (np.asarray(x, np.float64) for x in (eye, target, down))
    f = (target - eye) / np.linalg.norm(target - eye)
    d = down - np.dot(down, f) * f
    d /= np.linalg.norm(d)
    r = np.cross(d, f)
    M = np.eye(4)
    M[:3, :3] = np.stack((r, d, f))
    M[:3, 3] = -M[:3, :3] @ eye
    return M.astype(np.float32).astype(np.float64)


def intrinsics_fov(H, W, fov_x=math.radians(60.0)):
    fx = W / (2.0 * math.tan(fov_x * 0.5))
    return (fx, fx, W * 0.5, H * 0.5)


SCENE = dict(centre=np.array([0.08, -0.03, 0.02]), radius=0.33, plane_z=-0.27)      # a sphere over the plane z = plane_z


def render_scene(H, W, intr, w2c, seed, holes=True, mask_kind=None):
    """Depth, alpha, image and mask of the analytic scene through the pixel centres: D = float32(A z), A in [0.6, 1), the
    image a smooth function of the hit point; alpha 0 where the ray hits nothing.  holes=True plants every kind of hole the
    definition names at fixed pixels of the part of the image that sees the scene."""
    fx, fy, cx, cy = intr
    gen = np.random.default_rng(seed)
    R, t = w2c[:3, :3], w2c[:3, 3]
    eye = -R.T @ t
    px, py = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    ray = np.stack(((px - cx) / fx, (py - cy) / fy, np.ones_like(px)), axis=-1) @ R      # world direction, z_cam component 1
    oc = eye - SCENE["centre"]
    a, b, c = (ray * ray).sum(-1), 2.0 * (ray @ oc), oc @ oc - SCENE["radius"] ** 2
    disc = b * b - 4 * a * c
    with np.errstate(all="ignore"):
        ts = np.where(disc > 0, (-b - np.sqrt(np.abs(disc))) / (2 * a), np.inf)
        ts = np.where(ts > 0, ts, np.inf)
        tp = (SCENE["plane_z"] - eye[2]) / ray[..., 2]
        tp = np.where(np.isfinite(tp) & (tp > 0), tp, np.inf)
    z = np.minimum(ts, tp)
    hit = np.isfinite(z) & (z < 50.0)
    z = np.where(hit, z, 1.0)
    P = eye + ray * z[..., None]
    A = np.where(hit, 0.6 + 0.4 * gen.random((H, W)), 0.0)
    D = (A * z).astype(np.float32)
    A = A.astype(np.float32)
    image = (0.5 + 0.5 * np.sin(np.moveaxis(P, -1, 0) * np.array([3.0, 4.0, 5.0])[:, None, None] + np.array([0.1, 0.7, 1.3])[:, None, None]))
    image = np.ascontiguousarray(image, np.float32)
    m = (0.25 + gen.random((H, W))).astype(np.float32)
    m[gen.random((H, W)) < 0.1] = 0.0
    if holes:
        ys, xs = np.nonzero(hit)
        pick = gen.permutation(len(ys))[:9 * 4].reshape(9, 4)
        at = lambda r: (ys[pick[r]], xs[pick[r]])
        A[at(0)] = 0.3                      # below min_alpha
        D[at(1)] = np.nan
        D[at(2)] = np.inf
        A[at(3)] = np.nan
        A[at(4)] = np.inf
        D[at(5)] = 0.0
        D[at(6)] = -1.5
        image[0][at(7)] = np.nan            # a non-finite image value: the colour stays, tsdf and weight move
        image[2][at(8)] = np.inf
    mask = {None: None, "f32": m, "u8": (m > 0).astype(np.uint8) * 3, "bool": m > 0}[mask_kind]
    return dict(depth=D, alpha=A, image=image, mask=mask, intr=intr, w2c=w2c)


def volume_geometry(dims, h=0.1):
    """(lo float32 [3], h float32) of a volume of `dims` nodes centred a generic fraction of a cell off the scene's centre."""
    h = np.float32(h)
    lo = (SCENE["centre"] - 0.5 * float(h) * (np.array(dims) - 1) + float(h) * np.array([0.13, -0.21, 0.07])).astype(np.float32)
    return lo, h


def parity_views(dims, H=37, W=29, h=0.1, corner_shift=0.6):
    """The three views of the integration-parity test, float32 mask / uint8 mask / bool mask in turn: one that sees the whole
    volume, one inside it (part of the volume behind `near`), one that sees only a corner of it (20 x 13 x 9: 13 % of the
    nodes; the flat 64 x 4 x 3 volume wants corner_shift = 0.4 for 11 %)."""
    lo, h = volume_geometry(dims, h)
    ext = float(h) * (np.array(dims) - 1)
    mid = lo.astype(np.float64) + 0.5 * ext
    far = float(np.linalg.norm(ext))
    intr = intrinsics_fov(H, W)
    corner = lo.astype(np.float64) + ext                                           # the last node of the volume
    away = np.array([1.0, 0.8, 0.9]) / np.linalg.norm([1.0, 0.8, 0.9])
    aside = np.cross(away, [0.3, -0.5, 1.0])
    aside /= np.linalg.norm(aside)
    cams = [look_at(mid + far * np.array([0.55, -0.9, 0.6]), mid + np.array([0.01, 0.02, -0.03])),
            look_at(mid + ext * np.array([0.21, -0.17, 0.3]), mid + ext * np.array([-0.45, 0.4, -0.6])),
            look_at(corner + 0.8 * far * away, corner + corner_shift * far * aside)]   # looks past the corner
    kinds = ("f32", "u8", "bool")
    return [render_scene(H, W, intr, cams[i], seed=20 + i, mask_kind=kinds[i]) for i in range(3)]


def orbit_views(n, H, W, dims, h, seed=5, holes=False):
    """n views on a circle around the volume (the batching test's)."""
    lo, h = volume_geometry(dims, h)
    ext = float(h) * (np.array(dims) - 1)
    mid = lo.astype(np.float64) + 0.5 * ext
    rad = 1.4 * float(np.linalg.norm(ext))
    intr = intrinsics_fov(H, W)
    out = []
    for i in range(n):
        ang = 2.0 * math.pi * (i + 0.3) / n
        eye = mid + rad * np.array([math.cos(ang), math.sin(ang), 0.35 + 0.2 * math.sin(3 * ang)])
        out.append(render_scene(H, W, intr, look_at(eye, mid), seed=seed + i, holes=holes))
    return out
