"""The mesh family on the poison ladder (tests/poison.py): no result of the components, the filter or the normals may depend on
what its uninitialised buffers held.  parent, labels, the per-vertex face counts, the status word, the compaction scratch,
roots, face counts, remap and every output are torch.empty and handed to the kernels as they are.  Each case runs unpatched,
then with every such buffer pre-filled with zero bytes, int64 ones and 0xFF bytes (NaN / -1), in that order, and every run must
give the bits of the zero-filled one."""
import numpy as np
import pytest
import torch

import mesh_ref as ref
import poison
import splatco_amd.mesh                       # noqa: F401  (the module under test: without it nothing here can run)
from splatco_amd.mesh import clean_mesh, connected_components, vertex_normals

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _check(fn):
    rep = poison.check(fn, sync=torch.cuda.synchronize)
    for pattern in poison.PATTERNS:
        assert rep[pattern].bytes > 0 and rep[pattern].count > 0, pattern
    return rep


def _mesh():
    v, f, *_ = ref.mixed_mesh(700, 41, 21)                  # 2491 vertices, 1750 faces: three workgroups of items, partial last
    c = np.random.default_rng(2).random(v.shape).astype(np.float32)
    return v, f, tuple(torch.from_numpy(x).to(DEV) for x in (v, f, c))


def test_components():
    v, f, (vd, fd, cd) = _mesh()
    rep = _check(lambda: list(connected_components(fd, len(v))))
    labels, roots, counts = (x.cpu().numpy() for x in rep["outputs"])
    want = ref.components_ref(f, len(v))
    assert np.array_equal(labels, want[0]) and np.array_equal(roots, want[1]) and np.array_equal(counts, want[2])
    # parent, labels, vertex_faces [Nv], status, the scratch, roots and face_counts [Nc]
    assert rep["nan"].count >= 7 and rep["nan"].bytes >= 3 * 4 * len(v) + 4 + 2 * 4 * len(roots)


def test_filter():
    v, f, (vd, fd, cd) = _mesh()
    seen = {}

    def fn():
        v2, f2, c2, info = clean_mesh(vd, fd, cd, keep_largest=200, min_faces=2)
        v3, f3, _, _ = clean_mesh(vd, fd, None)
        seen["info"] = info
        return [v2, f2, c2, v3, f3]

    rep = _check(fn)
    want = ref.clean_ref(v, f, v * 0, keep_largest=200, min_faces=2)
    assert seen["info"] == want[3] and 0 < want[3]["vertices_after"] < len(v)
    assert np.array_equal(rep["outputs"][1].cpu().numpy(), want[1])
    nv2, nf2 = want[3]["vertices_after"], want[3]["faces_after"]
    assert rep["nan"].bytes >= 4 * 4 * len(v) + 2 * 12 * nv2 + 12 * nf2


def test_normals():
    v, f, (vd, fd, cd) = _mesh()
    rep = _check(lambda: [vertex_normals(vd, fd)])
    assert np.array_equal(rep["outputs"][0].cpu().numpy().view(np.int32), ref.normals_ref(v, f).view(np.int32))
    assert rep["nan"].bytes >= 12 * len(v)
