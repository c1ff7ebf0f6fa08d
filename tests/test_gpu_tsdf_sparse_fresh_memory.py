"""The block-sparse TSDF family on the poison ladder (tests/poison.py): no result of allocation, integration or extraction may
depend on what its uninitialised buffers held.  The block storage (grown from one row, so that copied and fresh rows mix), the
mark array, the key lists, the neighbour table, the compaction scratch, the kept edge ids, the vertices, the colours and the
faces are all torch.empty.  Each case runs unpatched, then with every such buffer pre-filled with zero bytes, int64 ones and
0xFF bytes (NaN / -1), in that order, and every run must give the bits of the zero-filled one."""
import numpy as np
import pytest
import torch

import poison
import tsdf_ref as ref
import splatco_amd.tsdf_sparse                # noqa: F401  (the module under test: without it nothing here can run)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _check(fn):
    rep = poison.check(fn, sync=torch.cuda.synchronize)
    for pattern in poison.PATTERNS:
        assert rep[pattern].bytes > 0 and rep[pattern].count > 0, pattern
    return rep


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


@pytest.mark.parametrize("dims", [(40, 27, 19), (17, 9, 10)])
def test_allocation_and_integration(dims):
    """Streaming from a capacity of one row, with colour and masks, and a two-pass volume without colour."""
    from splatco_amd.tsdf_sparse import SparseTSDFVolume
    lo, h = ref.volume_geometry(dims)
    views = ref.parity_views(dims)
    D, A, images, masks = ([_dev(v[k]) for v in views] for k in ("depth", "alpha", "image", "mask"))
    cams = [(v["intr"], torch.from_numpy(v["w2c"])) for v in views]
    seen = {}

    def fn():
        vol = SparseTSDFVolume(lo, float(h), dims, device=DEV, capacity=1)
        for i in (2, 1, 0):
            vol.integrate(D[i], A[i], cams[i], image=images[i], mask=masks[i])
        plain = SparseTSDFVolume(lo, float(h), dims, color=False, device=DEV)
        plain.integrate_views(D, A, cams, masks=masks, two_pass=True)
        n, m = vol.num_blocks, plain.num_blocks
        seen["n"] = (n, m)
        return [vol.keys, vol.slots, vol.tsdf[:n], vol.weight[:n], vol.color[:n], vol._marks, plain.keys, plain.slots, plain.tsdf[:m], plain.weight[:m]]

    rep = _check(fn)
    n, m = seen["n"]
    assert n > 2 and m == n                              # the same views: the same blocks, whatever the order
    assert rep["nan"].bytes >= (5 * n + 2 * m) * 512 * 4
    out = rep["outputs"]
    assert bool((out[3] > 0).any()) and bool((out[2] < 1).any()) and bool((out[4] > 0).any())


def test_extraction():
    """The fused orbit volume: neighbour table, scratch, ids, vertices, colours and faces are all taken uninitialised."""
    from splatco_amd.tsdf_sparse import SparseTSDFVolume
    dims = (20, 20, 20)
    lo, h = ref.volume_geometry(dims, 0.06)
    views = ref.orbit_views(5, 30, 40, dims, 0.06)
    D, A, images = ([_dev(v[k]) for v in views] for k in ("depth", "alpha", "image"))
    cams = [(v["intr"], torch.from_numpy(v["w2c"])) for v in views]
    seen = {}

    def fn():
        vol = SparseTSDFVolume(lo, float(h), dims, device=DEV, capacity=3)
        vol.integrate_views(D, A, cams, images)
        v, f, col = vol.extract()
        v1, f1, _ = vol.extract(min_weight=2.0, pass_blocks=7)          # several passes: joined lists
        seen["n"] = (vol.num_blocks, v.shape[0], f.shape[0], v1.shape[0])
        return [v, f, col, v1, f1]

    p = _check(fn)["nan"]
    nb, nv, nf, nv1 = seen["n"]
    assert nv > 100 and nf > 100 and 0 < nv1 < nv
    assert p.bytes >= nv * (8 + 12 + 12) + nf * 12 + nb * 27 * 4
