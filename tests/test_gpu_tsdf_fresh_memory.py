"""The TSDF family on the poison ladder (tests/poison.py): no result of integration or extraction may depend on what its
uninitialised buffers held.  The volume's own tensors are torch.empty filled by the constructor; the compaction scratch, the
kept edge ids, the vertices, the colours and the faces are torch.empty and handed to the kernels as they are.  Each case runs
unpatched, then with every such buffer pre-filled with zero bytes, int64 ones and 0xFF bytes (NaN / -1), in that order, and
every run must give the bits of the zero-filled one."""
import numpy as np
import pytest
import torch

import poison
import tsdf_ref as ref
import splatco_amd.tsdf                       # noqa: F401  (the module under test: without it nothing here can run)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _check(fn):
    rep = poison.check(fn, sync=torch.cuda.synchronize)
    for pattern in poison.PATTERNS:
        assert rep[pattern].bytes > 0 and rep[pattern].count > 0, pattern
    return rep


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


@pytest.mark.parametrize("dims,shift", [((2, 5, 7), 0.6), ((64, 4, 3), 0.4)])
def test_integration(dims, shift):
    """The two small parity volumes: guarded dword accesses with a partial last run, and 16-byte accesses."""
    from splatco_amd.tsdf import TSDFVolume
    lo, h = ref.volume_geometry(dims)
    views = ref.parity_views(dims, corner_shift=shift)
    D, A, images, masks = ([_dev(v[k]) for v in views] for k in ("depth", "alpha", "image", "mask"))
    cams = [(v["intr"], torch.from_numpy(v["w2c"])) for v in views]

    def fn():
        vol = TSDFVolume(lo, float(h), dims, device=DEV)
        vol.integrate_views(D, A, cams, images, masks, batch=16)
        plain = TSDFVolume(lo, float(h), dims, color=False, device=DEV)
        plain.integrate(D[0], A[0], cams[0], mask=masks[0])
        return [vol.tsdf, vol.weight, vol.color, plain.tsdf, plain.weight]

    rep = _check(fn)
    assert rep["nan"].bytes >= 5 * 4 * dims[0] * dims[1] * dims[2]
    out = rep["outputs"]
    assert bool((out[1] > 0).any()) and bool((out[0] < 1).any())


def test_extraction():
    """The integrated 20 x 13 x 9 volume: scratch, ids, vertices, colours and faces are all taken uninitialised."""
    from splatco_amd.tsdf import TSDFVolume
    dims = (20, 13, 9)
    lo, h = ref.volume_geometry(dims)
    vol, _ = ref.integrate_views_ref(ref.fresh(dims), lo, h, ref.parity_views(dims), 4.0 * float(h))
    t, w, c = _dev(vol["tsdf"]), _dev(vol["weight"]), _dev(vol["color"])
    seen = {}

    def fn():
        v, f, col = TSDFVolume.from_tensors(lo, float(h), t, w, c).extract()
        v1, f1, _ = TSDFVolume.from_tensors(lo, float(h), t, w).extract(min_weight=1.0)
        seen["n"] = (v.shape[0], f.shape[0], v1.shape[0])
        return [v, f, col, v1, f1]

    p = _check(fn)["nan"]
    nv, nf, nv1 = seen["n"]
    assert nv > 100 and nf > 100 and 0 < nv1 < nv
    assert p.bytes >= nv * (4 + 12 + 12) + nf * 12 and p.count >= 9
