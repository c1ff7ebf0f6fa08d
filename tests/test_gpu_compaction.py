"""GPU tests of the shared count / scan / write compaction (csrc/compact.h) through its three users -- the mask -> index
list, the neural-Gaussian expansion (csrc/expand.hip) and the distinct voxel keys (csrc/scene_init.hip) -- at the smallest
sizes at which each part of the scheme can go wrong: the edge of a wave (64 items), of a round (256), of a workgroup (1024),
and of the scan kernel's chunks of 1024 workgroup counts (1 048 576 items per chunk; the carry between chunks).  Every
comparison is exact."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNK = 1_048_576                  # items behind one chunk of the scan: 1024 workgroups of 1024 items
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, CHUNK, CHUNK + 1, 2 * CHUNK + 1]


def _keep_patterns(n, seed):
    """(name, bool[n] on the device): none, all, random at 0.37, only the last item, only the first item of the scan's
    second chunk (where it exists: the carry alone then decides its position)."""
    z = torch.zeros(n, dtype=torch.bool, device=DEV)
    out = [("none", z), ("all", ~z),
           ("random", (torch.rand(n, generator=torch.Generator().manual_seed(seed)) < 0.37).to(DEV))]
    if n:
        last = z.clone()
        last[n - 1] = True
        out.append(("last", last))
    if n > CHUNK:
        one = z.clone()
        one[CHUNK] = True
        out.append(("carry", one))
    return out


@pytest.mark.parametrize("n", [0] + SIZES)
def test_mask_indices_at_every_edge_of_the_scheme(n):
    """mask_indices(mask) == mask.nonzero().squeeze(1), and its inverse map == the fill / arange / index_put it replaces."""
    from splatco_amd.expand import mask_indices
    for name, mask in _keep_patterns(n, n):
        idx = mask_indices(mask)
        ref = mask.nonzero(as_tuple=False).squeeze(1)
        assert idx.dtype == torch.int64 and idx.shape == ref.shape, name
        assert torch.equal(idx, ref), name
        if n:
            inv = torch.full((n,), -1, dtype=torch.int64, device=DEV)
            inv.index_put_((ref,), torch.arange(ref.shape[0], dtype=torch.int64, device=DEV))
            assert torch.equal(idx._scr_inverse, inv), name


@pytest.mark.parametrize("V,k", [(1, 1), (65, 1), (257, 1), (103, 10), (1025, 1), (CHUNK + 1, 1), (104_858, 10)])
def test_expand_compact_at_every_edge_of_the_scheme(V, k):
    """expand_compact keeps exactly the candidates with neural_opacity > 0, in order: mask, the copied-through opacity and
    colour (bit for bit), the position of every candidate, and the same bits from a second call."""
    from splatco_amd.expand import expand_compact
    n = V * k
    g = torch.Generator().manual_seed(V + k)
    mag = (torch.rand(n, 1, generator=g) + 0.01).to(DEV)
    color = torch.rand(n, 3, generator=g).to(DEV)
    scale_rot = torch.randn(n, 7, generator=g).to(DEV)
    offsets = torch.randn(V, k, 3, generator=g).to(DEV)
    grid_scaling = (torch.rand(V, 6, generator=g) + 0.1).to(DEV)
    anchor = torch.randn(V, 3, generator=g).to(DEV)
    for name, keep in _keep_patterns(n, n):
        neural_opacity = torch.where(keep[:, None], mag, -mag)
        if name == "random":
            neural_opacity[::7] = 0.0                  # a zero opacity is not kept
        runs = [expand_compact(neural_opacity, color, scale_rot, offsets, grid_scaling, anchor, k) for _ in range(2)]
        xyz, col, opa, sca, rot, mask = runs[0]
        ref_mask = neural_opacity.reshape(-1) > 0
        nz = ref_mask.nonzero(as_tuple=False).squeeze(1)
        assert mask.dtype == torch.bool and torch.equal(mask, ref_mask), name
        assert opa.shape == (nz.shape[0], 1) and torch.equal(opa, neural_opacity[nz]), name
        assert torch.equal(col, color[nz]), name
        assert xyz.shape == (nz.shape[0], 3) and sca.shape == (nz.shape[0], 3) and rot.shape == (nz.shape[0], 4), name
        pos = torch.where(ref_mask, torch.cumsum(ref_mask, 0) - 1, -1).to(torch.int32)
        assert torch.equal(mask._scr_out_index, pos), name
        for a, b in zip(runs[0], runs[1]):
            assert torch.equal(a, b), name


def _voxel_unique(keys, v, lo):
    """scr_voxel_unique_plan + scr_voxel_unique_run on sorted packed keys -> (count, [count, 3] float32)."""
    from splatco_amd import _C
    N, st = keys.shape[0], _C.stream(torch.device(DEV))
    lo_host = _C.host_array(lo, _C.i32)
    with torch.cuda.device(DEV):
        scratch = _C.scratch(_C.lib.scr_voxel_unique_scratch_bytes(N), torch.device(DEV))
        cnt = C.c_int64(-1)
        _C.check(_C.lib.scr_voxel_unique_plan(N, keys.data_ptr(), scratch.data_ptr(), C.byref(cnt), st))
        out = torch.empty(cnt.value, 3, dtype=torch.float32, device=DEV)
        _C.check(_C.lib.scr_voxel_unique_run(N, keys.data_ptr(), scratch.data_ptr(), float(v), lo_host, out.data_ptr(), st))
    return cnt.value, out


@pytest.mark.parametrize("n", SIZES)
def test_voxel_unique_at_every_edge_of_the_scheme(n):
    """The distinct keys of a sorted packed key list: as many as torch.unique_consecutive finds, decoded to
    float32(q) * v in binary32."""
    lo, v = (-3, 5, -100_000), torch.tensor(0.01, dtype=torch.float32, device=DEV)
    g = torch.Generator().manual_seed(n)
    pack = lambda x, y, z: (x << 42) | (y << 21) | z
    rnd = pack(torch.randint(0, 3, (n,), generator=g), torch.randint(0, 5, (n,), generator=g),
               torch.randint(0, n // 16 + 2, (n,), generator=g))
    cases = [("equal", torch.full((n,), pack(7, 2_000_000, 11), dtype=torch.int64)),
             ("distinct", torch.arange(n, dtype=torch.int64)),       # the largest size carries from the z field into y
             ("random", torch.sort(rnd).values)]
    if n > CHUNK:        # two runs, the second begins with the scan's second chunk: the carry alone decides its position
        cases.append(("carry", (torch.arange(n, dtype=torch.int64) >= CHUNK).long() * pack(1, 2, 3)))
    for name, keys in cases:
        keys = keys.to(DEV)
        u = torch.unique_consecutive(keys)
        ref = torch.stack(((u >> 42) + lo[0], ((u >> 21) & 0x1FFFFF) + lo[1], (u & 0x1FFFFF) + lo[2]), 1).float() * v
        count, out = _voxel_unique(keys, v.item(), lo)
        assert count == u.shape[0], name
        assert torch.equal(out, ref), name
