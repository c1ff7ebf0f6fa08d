"""The definitions of splatco_amd.tsdf_sparse (include/splatco_tsdf_sparse.h) that the dense family does not already state,
restated in numpy float64: the block lattice and the allocation rule of one view.  Integration and extraction are the dense
family's (tests/tsdf_ref.py), applied to the allocated blocks.

Blocks have B = 8 nodes per side, nb? = ceil(n? / 8); block (bi, bj, bk) has the key (bk nby + bj) nbx + bi; block masks here
are bool [nbz, nby, nbx], so mask.reshape(-1) is indexed by key.

Allocation for one view.  For every pixel (px, py) that passes the dense pixel test (D, A finite, A >= min_alpha, D > 0, mask
positive):
  1. z = (double)(float)(D / A), z0 = max(z - trunc, near), z1 = z + trunc; z0 > z1 allocates nothing
  2. the 8 camera-space corners ((px + dx - cx) / fx zc, (py + dy - cy) / fy zc, zc), dx, dy in {0, 1}, zc in {z0, z1}
  3. moved to world space with c2w, the binary64 inverse of the 4 x 4 world-to-camera matrix
  4. their axis-aligned box padded by `pad` (h / 8 in the definition) on every side
  5. block ranges floor((min - lo) / (8 h)) .. floor((max - lo) / (8 h)) per axis, clipped to the grid
  6. every block in the range is allocated
The only Python loop runs over the passing pixels, to mark each one's range."""
import numpy as np

import tsdf_ref as ref

B = 8


def block_dims(dims):
    """(nbx, nby, nbz)"""
    return tuple((int(d) + B - 1) // B for d in dims)


def blocks_of(nodes):
    """bool [nz, ny, nx] -> bool [nbz, nby, nbx]: the blocks that contain a marked node."""
    nz, ny, nx = nodes.shape
    nbx, nby, nbz = block_dims((nx, ny, nz))
    padded = np.zeros((nbz * B, nby * B, nbx * B), bool)
    padded[:nz, :ny, :nx] = nodes
    return padded.reshape(nbz, B, nby, B, nbx, B).any(axis=(1, 3, 5))


def nodes_of(blocks, dims):
    """bool [nbz, nby, nbx] -> bool [nz, ny, nx]: the nodes of the marked blocks."""
    nx, ny, nz = dims
    return np.repeat(np.repeat(np.repeat(blocks, B, 0), B, 1), B, 2)[:nz, :ny, :nx]


def allocate_ref(dims, lo, h, trunc, view, pad=None, min_alpha=0.5, near=0.05):
    """The blocks one view allocates: bool [nbz, nby, nbx].  view: a dict of tsdf_ref.render_scene.  pad: the padding of the
    world box, h / 8 unless given (the GPU test brackets the device's rounding with h / 8 -+ 1e-6 h)."""
    nbx, nby, nbz = block_dims(dims)
    lo = np.asarray(lo, np.float32).astype(np.float64)
    h = float(np.float32(h))
    trunc = float(trunc)
    pad = h / 8.0 if pad is None else float(pad)
    near = float(view.get("near", near))
    D, A = np.asarray(view["depth"], np.float32), np.asarray(view["alpha"], np.float32)
    H, W = D.shape
    fx, fy, cx, cy = (float(x) for x in view["intr"])
    c2w = np.linalg.inv(np.asarray(view["w2c"], np.float64))
    ok = np.isfinite(D) & np.isfinite(A) & (A >= np.float32(min_alpha)) & (D > 0) & ref.mask_positive(view.get("mask"), (H, W))
    with np.errstate(all="ignore"):
        z = (np.where(ok, D, np.float32(1)) / np.where(ok, A, np.float32(1))).astype(np.float32).astype(np.float64)
    z0, z1 = np.maximum(z - trunc, near), z + trunc
    ok &= ~(z0 > z1)
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    mn, mx = np.full((3, H, W), np.inf), np.full((3, H, W), -np.inf)
    for dx in (0.0, 1.0):
        for dy in (0.0, 1.0):
            for zc in (z0, z1):
                xc, yc = (px + dx - cx) / fx * zc, (py + dy - cy) / fy * zc
                for a in range(3):
                    w = ((c2w[a, 0] * xc + c2w[a, 1] * yc) + c2w[a, 2] * zc) + c2w[a, 3]
                    mn[a], mx[a] = np.minimum(mn[a], w), np.maximum(mx[a], w)
    side = 8.0 * h
    b0 = np.floor(((mn - pad) - lo[:, None, None]) / side)
    b1 = np.floor(((mx + pad) - lo[:, None, None]) / side)
    nb = np.array([nbx, nby, nbz], np.float64)[:, None, None]
    b0, b1 = np.maximum(b0, 0.0), np.minimum(b1, nb - 1.0)
    ok &= (b0 <= b1).all(0)
    out = np.zeros((nbz, nby, nbx), bool)
    for y, x in zip(*np.nonzero(ok)):
        i0, j0, k0 = (int(v) for v in b0[:, y, x])
        i1, j1, k1 = (int(v) for v in b1[:, y, x])
        out[k0:k1 + 1, j0:j1 + 1, i0:i1 + 1] = True
    return out


def band_blocks(dims, lo, h, trunc, view, **kw):
    """The blocks that contain a node the dense update moves with sdf <= trunc (tsdf_ref.integrate_ref's details)."""
    o = ref.integrate_ref(ref.fresh(dims, color=False), lo, h, view["depth"], view["alpha"], view["intr"], view["w2c"], trunc,
                          mask=view.get("mask"), details=True, **kw)
    det = o["details"]
    return blocks_of(det["upd"] & (det["sdf"] <= float(trunc)))
