"""The mesh-evaluation family on the poison ladder (tests/poison.py): no result of the sampler, the nearest-neighbour search or
the score may depend on what its uninitialised buffers held.  The face counts, the samples and their face indices, the cell
keys, the distances and indices, the score's workgroup records and its output record are torch.empty and handed to the kernels
as they are.  Each case runs unpatched, then with every such buffer pre-filled with zero bytes, int64 ones and 0xFF bytes
(NaN / -1), in that order, and every run must give the bits of the zero-filled one."""
import numpy as np
import pytest
import torch

import poison
import surfeval_ref as ref
import splatco_amd.surface_eval                # noqa: F401  (the module under test: without it nothing here can run)
from splatco_amd.surface_eval import THREADS as T, _reduce, nearest, sample_surface, score

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
bits = lambda a: np.ascontiguousarray(a).view(np.int32)


def _check(fn):
    rep = poison.check(fn, sync=torch.cuda.synchronize)
    for pattern in poison.PATTERNS:
        assert rep[pattern].bytes > 0 and rep[pattern].count > 0, pattern
    return rep


def test_sampler():
    v, f = ref.small_faces(3 * T + 5, 1)                     # four workgroups of faces, partial last; degenerate faces among them
    f[7], f[300] = (3, 3, 4), (9, 9, 9)
    density = 2.5 / float(ref.areas_ref(v, f).mean())
    vd, fd = dev(v), dev(f)
    rep = _check(lambda: list(sample_surface(vd, fd, density=density, seed=4)))
    pts, fi = (x.cpu().numpy() for x in rep["outputs"])
    want = ref.sample_ref(v, f, density, 4)
    assert np.array_equal(bits(pts), bits(want[0])) and np.array_equal(fi, want[1]) and len(fi) > 2 * T
    # counts [Nf] int64, points [Ns, 3], face_index [Ns], and the bounds' scratch and record
    assert rep["nan"].count >= 4 and rep["nan"].bytes >= 8 * len(f) + 16 * len(fi)


def test_nearest():
    t = ref.targets("clusters", 1000, 2)
    q = ref.queries(t, 2 * T + 3, 3)
    td, qd = dev(t), dev(q)
    rep = _check(lambda: list(nearest(qd, td)) + list(nearest(qd, td, max_dist=0.3)))
    got = [x.cpu().numpy() for x in rep["outputs"]]
    for (d2, idx), want in ((got[:2], ref.nearest_ref(q, t)), (got[2:], ref.nearest_ref(q, t, 0.3))):
        assert np.array_equal(bits(d2), bits(want[0])) and np.array_equal(idx, want[1])
    # per call: the keys of both sets, dist2 and index [Nq]
    assert rep["nan"].bytes >= 2 * (8 * len(t) + 8 * len(q) + 8 * len(q))


def test_score():
    gen = np.random.default_rng(5)
    a = (gen.uniform(0, 2, size=3 * 4096 + 17) ** 2).astype(np.float32)             # four workgroups of items, partial last
    b = (gen.uniform(0, 1, size=T + 1) ** 2).astype(np.float32)
    ad, bd = dev(a), dev(b)
    seen = {}

    def fn():
        seen["res"] = score(ad, bd, (0.5, 1.0, 0.25))
        return [_reduce(ad, [0.5, 1.0, 0.25]), _reduce(bd, [])]

    rep = _check(fn)
    want = ref.score_ref(a, b, (0.5, 1.0, 0.25))
    rec = rep["outputs"][0].cpu().numpy()
    assert rec[2:5].tolist() == want["count_pred_to_gt"] and not rec[5:].any() and rec[1] == want["max_pred_to_gt"]
    assert not rep["outputs"][1].cpu().numpy()[2:].any()
    assert seen["res"]["count_gt_to_pred"] == want["count_gt_to_pred"] and seen["res"]["accuracy"] == rec[0] / len(a)
    # per reduction: ten binary64 per workgroup (256-byte aligned) and the record
    assert rep["nan"].bytes >= 2 * (4 * 80 + 80 + 256 + 80)
