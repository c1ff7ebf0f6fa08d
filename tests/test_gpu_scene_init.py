"""GPU tests of scene initialisation from a point cloud (csrc/scene_init.hip, splatco_amd.scene_init): the device branch
against the CPU branch BIT FOR BIT (the CPU branch itself is tied to the reference's output and to float64 by
tests/test_scene_init_host.py), at full size against torch.unique and a brute force with the specified arithmetic, and
end to end into the existing training step."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_init.npz"))
DEV = "cuda:0"


TIME_LIMIT = 300      # seconds per test; the slowest takes a few seconds


@pytest.fixture(autouse=True)
def _time_limit_and_fault_guard(request):
    """Every test here runs under its own time limit, and a test that leaves the device unusable ends the run: nothing
    more is started on a GPU that has faulted or hung."""
    import signal

    def expired(signum, frame):
        pytest.exit(f"{request.node.name} exceeded its time limit of {TIME_LIMIT} s: stopping the run", returncode=1)

    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(TIME_LIMIT)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reports an error after {request.node.name}: {e}; stopping the run", returncode=1)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _sphere(n, seed, radius=1.5):
    x = torch.randn(n, 3, generator=_gen(seed))
    return (x / x.norm(dim=1, keepdim=True) * radius).float().contiguous()


def _clustered(n, seed, dup=0.1):
    g = _gen(seed)
    c = torch.rand(8, 3, generator=g) * 3 - 1.5
    s = torch.tensor([0.01, 0.03, 0.05, 0.1, 0.2, 0.3, 0.02, 0.5])
    k = torch.randint(0, 8, (n,), generator=g)
    p = c[k] + torch.randn(n, 3, generator=g) * s[k, None]
    nd = int(n * dup)
    p[torch.randperm(n, generator=g)[:nd]] = p[torch.randint(0, n, (nd,), generator=g)]      # exact duplicates
    return p.contiguous()


def _wide(seed=5):
    """the cloud of tests/test_scene_init_host.py::test_wide_extent_fallback: two clusters 3000 units apart"""
    a = torch.randn(3000, 3, generator=_gen(seed)) * 0.02
    return torch.cat([a + torch.tensor([-1500.0, 0.3, -0.2]), a.flip(0) + torch.tensor([1500.0, -0.1, 0.4]),
                      a[:200] + torch.tensor([-1500.0, 0.3, -0.2])])


def _dist2_clouds():
    from splatco_amd.scene_init import voxelize
    uniform = torch.rand(20011, 3, generator=_gen(1)) * 4 - 2
    line = torch.zeros(5000, 3)
    line[:, 1] = torch.rand(5000, generator=_gen(2)) * 7 - 3
    line += torch.tensor([0.25, 0.0, -1.0])
    small = torch.rand(257, 3, generator=_gen(3)) * 2 - 1
    clouds = {"uniform 20011": uniform, "clustered, 10 % duplicates": _clustered(20000, 4),
              "lattice": voxelize(_clustered(30000, 6, dup=0.0), 0.05), "sheet 20000": _sphere(20000, 7), "line": line}
    clouds.update({f"N = {n}": small[:n].contiguous() for n in (4, 63, 64, 65, 257)})
    return clouds


DIST2_CLOUDS = ("uniform 20011", "clustered, 10 % duplicates", "lattice", "sheet 20000", "line", "N = 4", "N = 63", "N = 64",
                "N = 65", "N = 257")


@pytest.mark.parametrize("name", DIST2_CLOUDS)
def test_dist2_device_equals_cpu_bit_for_bit(name):
    from splatco_amd.scene_init import dist2
    clouds = _dist2_clouds()
    assert tuple(clouds) == DIST2_CLOUDS
    p = clouds[name]
    want = dist2(p)
    got = dist2(p.to(DEV))
    torch.cuda.synchronize()
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape
    bad = int((got.cpu() != want).sum())
    print(f"[{name}] N = {p.shape[0]}: {bad} of {want.numel()} values differ")
    assert torch.equal(got.cpu(), want)


KNN_KS = (1, 3, 10, 11, 16)          # 10 takes knn_kernel<10>; 11 and 16 take knn_kernel<16>
KNN_REF = 17                          # reference distances kept per query: k + 1 at the largest k
# cloud -> N.  The members of _dist2_clouds() ("N = 257" is small[:257]), then: the two far clusters (the per-axis bound sets
# h, the walk crosses many empty shells), clusters without duplicates, one point 300 times (the [1, 1, 1] grid, every
# distance 0), small[:k + 1] (every other point is a neighbour: rmax ends the walk, not the stop test) and the edges of the
# 256-thread workgroup.
KNN_CLOUDS = {"uniform 20011": 20011, "clustered, 10 % duplicates": 20000, "lattice": None, "sheet 20000": 20000, "line": 5000,
              "N = 4": 4, "N = 63": 63, "N = 64": 64, "N = 65": 65, "N = 257": 257, "two clusters 3000 apart": 6200,
              "clustered": 20000, "300 identical points": 300, "N = 255": 255, "N = 256": 256,
              **{f"N = {k + 1}": k + 1 for k in KNN_KS if k != 3}}
# (c) leaves out a row whose k + 1 smallest distances tie; on these clouds at most 1 % of the rows may be left out (the
# reference alone has ties on 0.01 %, 0 %, 0.36 %, 0.01 % and 0 % of their rows, with 17 distances per row)
KNN_FEW_TIES = ("uniform 20011", "sheet 20000", "line", "clustered") + tuple(n for n in KNN_CLOUDS if n.startswith("N = "))
KNN_CASES = [(name, k) for name, n in KNN_CLOUDS.items() for k in KNN_KS if n is None or n > k]
_knn_cache = {}


def _knn_cloud(name):
    """(points, the KNN_REF smallest squared distances of every query ascending, their indices): a float32 brute force on
    the CPU with the kernel's arithmetic, the query masked by index; computed once per cloud."""
    if name not in _knn_cache:
        if not _knn_cache:
            small = torch.rand(257, 3, generator=_gen(3)) * 2 - 1          # the `small` of _dist2_clouds()
            _knn_cache[None] = {**_dist2_clouds(), "two clusters 3000 apart": _wide(), "clustered": _clustered(20000, 4, dup=0.0),
                                "300 identical points": torch.tensor([[0.3, -1.2, 2.5]]).repeat(300, 1),
                                **{f"N = {n}": small[:n].contiguous() for n in (2, 11, 12, 17, 255, 256)}}
            assert torch.equal(_knn_cache[None]["N = 257"], small)
        p = _knn_cache[None][name].float().contiguous()
        N = p.shape[0]
        m = min(KNN_REF, N)
        ref_d, ref_i = torch.empty(N, m), torch.empty(N, m, dtype=torch.long)
        x, y, z = p[:, 0].contiguous(), p[:, 1].contiguous(), p[:, 2].contiguous()
        step = max(1, (1 << 23) // N)
        for s in range(0, N, step):
            e = min(s + step, N)
            ex, ey, ez = x[None, :] - x[s:e, None], y[None, :] - y[s:e, None], z[None, :] - z[s:e, None]
            d = (ex * ex + ey * ey) + ez * ez                     # separate torch ops: nothing is contracted
            d[torch.arange(e - s), torch.arange(s, e)] = float("inf")
            ref_d[s:e], ref_i[s:e] = d.topk(m, dim=1, largest=False, sorted=True)
        _knn_cache[name] = (p, ref_d, ref_i)
    return _knn_cache[name]


@pytest.mark.parametrize("name,k", KNN_CASES)
def test_knn_indices_device_equals_brute_force(name, k):
    """densify._knn_indices on the device against the brute force: (a) well-formed indices, (b) the k distances bit for bit
    and in order, (c) the indices themselves wherever the k + 1 smallest distances are distinct, (d) at k = 3 the mean of
    (b)'s distances is dist2 on the device, bit for bit -- the two kernels share the search of csrc/knn_grid.h."""
    from splatco_amd.densify import _knn_indices
    from splatco_amd.scene_init import dist2
    p, ref_d, ref_i = _knn_cloud(name)
    N = p.shape[0]
    assert KNN_CLOUDS[name] in (None, N) and N > k
    got = _knn_indices(p.to(DEV), k)
    torch.cuda.synchronize()
    assert got.is_cuda and got.dtype == torch.long and tuple(got.shape) == (N, k)                     # (a)
    idx = got.cpu()
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    assert not bool((idx == torch.arange(N)[:, None]).any())
    s = idx.sort(dim=1).values
    assert not bool((s[:, 1:] == s[:, :-1]).any())
    e = p[idx] - p[:, None, :]                                                                         # (b)
    ex, ey, ez = e[..., 0], e[..., 1], e[..., 2]
    d = (ex * ex + ey * ey) + ez * ez
    bad = int((d != ref_d[:, :k]).any(dim=1).sum())
    distinct = (ref_d[:, 1:k + 1] != ref_d[:, :k]).all(dim=1)                                          # (c)
    tied = N - int(distinct.sum())
    wrong = int((idx[distinct] != ref_i[distinct, :k]).any(dim=1).sum())
    print(f"[{name}, k = {k}] N = {N}: {bad} rows differ in a distance; {tied} rows ({100 * tied / N:.2f} %) have a tie among "
          f"their {k + 1} smallest; {wrong} of the others differ in an index")
    assert torch.equal(d, ref_d[:, :k])
    assert torch.equal(idx[distinct], ref_i[distinct, :k])
    if name in KNN_FEW_TIES:
        assert tied <= 0.01 * N
    if k == 3:                                                                                         # (d)
        t = (d[:, 0] + d[:, 1]) + d[:, 2]
        assert torch.equal(t / torch.full_like(t, 3.0), dist2(p.to(DEV)).cpu())


def test_knn_indices_refuses_non_finite_points():
    from splatco_amd.densify import _knn_indices
    p = _clustered(5000, 51, dup=0.0).to(DEV)
    for bad_value in (float("nan"), float("inf"), -float("inf")):
        bad = p.clone()
        bad[4097, 2] = bad_value
        with pytest.raises(ValueError):
            _knn_indices(bad, 10)


def _voxel_clouds():
    clouds = {"fixture": (torch.tensor(GOLDEN["points"]), [float(v) for v in GOLDEN["voxel_sizes"]])}
    clouds["uniform 200 k"] = (torch.rand(200_000, 3, generator=_gen(11)) * 4 - 2, [0.05, 0.01, 0.001])
    clouds["clustered 200 k"] = (_clustered(200_000, 12), [0.05, 0.01, 0.001])
    clouds["two clusters 3000 apart"] = (_wide(), [0.001, 0.01])           # 0.001: the three-column path
    return clouds


VOXEL_CLOUDS = ("fixture", "uniform 200 k", "clustered 200 k", "two clusters 3000 apart")


@pytest.mark.parametrize("name", VOXEL_CLOUDS)
def test_voxelize_device_equals_cpu(name):
    from splatco_amd.scene_init import voxelize
    clouds = _voxel_clouds()
    assert tuple(clouds) == VOXEL_CLOUDS
    p, sizes = clouds[name]
    for v in sizes:
        want = voxelize(p, v)
        got = voxelize(p.to(DEV), v)
        torch.cuda.synchronize()
        print(f"[{name}] v = {v}: {p.shape[0]} -> {want.shape[0]} rows")
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape
        assert torch.equal(got.cpu(), want)
    if name == "fixture":
        assert torch.equal(voxelize(p.to(DEV), sizes[0], _force_rows=True).cpu(), voxelize(p, sizes[0]))


def _brute_dist2(anchors, rows, chunk=1 << 16):
    """dist2 of anchors[rows] by brute force over ALL anchors, on the device, with the specified arithmetic (separate
    torch ops: nothing is contracted)."""
    q = anchors[rows]
    best = torch.full((rows.shape[0], 3), float("inf"), device=anchors.device)
    ar = torch.arange(rows.shape[0], device=anchors.device)
    for c0 in range(0, anchors.shape[0], chunk):
        a = anchors[c0:c0 + chunk]
        ex, ey, ez = a[None, :, 0] - q[:, None, 0], a[None, :, 1] - q[:, None, 1], a[None, :, 2] - q[:, None, 2]
        d = (ex * ex + ey * ey) + ez * ez
        inside = (rows >= c0) & (rows < c0 + a.shape[0])
        d[ar[inside], rows[inside] - c0] = float("inf")                       # the query itself, by index
        best = torch.cat([best, d], dim=1).topk(3, dim=1, largest=False, sorted=True).values
    s = (best[:, 0] + best[:, 1]) + best[:, 2]
    return s / torch.full_like(s, 3.0)      # a tensor divisor: torch multiplies by the reciprocal of a scalar one on the device


@pytest.mark.parametrize("shape", ["uniform", "sheet"])
def test_full_size_5m_points(shape):
    from splatco_amd.scene_init import dist2, voxelize
    n, v = 5_000_000, 0.01
    p = torch.rand(n, 3, generator=_gen(21)) * 4 - 2 if shape == "uniform" else _sphere(n, 22)
    q = torch.round(p / torch.full_like(p, v)).long().to(DEV)                # float32 division on the host: IEEE
    want = torch.unique(q, dim=0).float() * torch.full((), v, dtype=torch.float32, device=DEV)
    got = voxelize(p.to(DEV), v)
    torch.cuda.synchronize()
    print(f"[5 M {shape}] survivors {got.shape[0]} (torch.unique: {want.shape[0]})")
    assert got.shape == want.shape
    assert torch.equal(got, want)
    del q, want
    d = dist2(got)
    rows = torch.randperm(got.shape[0], generator=_gen(23))[:1024].to(DEV)
    brute = _brute_dist2(got, rows)
    torch.cuda.synchronize()
    bad = int((d[rows] != brute).sum())
    print(f"[5 M {shape}] dist2 of 1024 sampled anchors: {bad} differ from the brute force")
    assert torch.equal(d[rows], brute)


def test_two_calls_give_identical_bits():
    from splatco_amd.scene_init import dist2, voxelize
    p = _clustered(300_000, 31).to(DEV)
    a, b = voxelize(p, 0.01), voxelize(p, 0.01)
    assert torch.equal(a, b)
    assert torch.equal(dist2(a), dist2(a))
    assert torch.equal(dist2(p), dist2(p))


def test_bad_input_raises_on_the_device():
    from splatco_amd.scene_init import dist2, voxelize
    p = _clustered(5000, 51, dup=0.0).to(DEV)
    for bad_value in (float("nan"), float("inf"), -float("inf")):
        bad = p.clone()
        bad[4097, 2] = bad_value
        with pytest.raises(ValueError):
            dist2(bad)
        with pytest.raises(ValueError):
            voxelize(bad, 0.05)
    with pytest.raises(ValueError):
        dist2(p[:3])
    with pytest.raises(ValueError):
        voxelize(p * 1000, 1e-7)


def _box_surfaces(n, seed):
    """n points on the faces of three boxes inside the [-2, 2]^3 scene box that synthetic_views look at"""
    g = _gen(seed)
    centre = torch.tensor([[-0.9, 0.1, 0.2], [0.6, -0.3, -0.4], [0.2, 0.8, 0.9]])
    half = torch.tensor([[0.5, 0.6, 0.4], [0.6, 0.4, 0.5], [0.3, 0.3, 0.6]])
    b = torch.randint(0, 3, (n,), generator=g)
    u = torch.rand(n, 3, generator=g) * 2 - 1
    axis = torch.randint(0, 3, (n,), generator=g)
    side = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    u[torch.arange(n), axis] = side
    return (centre[b] + u * half[b]).contiguous()


def test_create_from_pcd_feeds_the_training_step():
    from splatco_amd.adam import FusedAdam
    from splatco_amd.densify import AnchorDensifier
    from splatco_amd.renderer import prefilter_voxel, render
    from splatco_amd.scene_init import create_from_pcd
    from splatco_amd.synthetic import synthetic_anchor_model, synthetic_views
    from splatco_amd.train_step import collaborative_step
    dev = torch.device(DEV)
    W, H = 480, 270
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    bg = torch.ones(3, device=dev)
    views = [v.to(dev) for v in synthetic_views(2, W, H)]
    pc = synthetic_anchor_model(16, 7, dev, plane_size=256)          # seeded heads and planes; the anchors are replaced
    used, n_points, n_anchors = create_from_pcd(pc, _box_surfaces(200_000, 41), 0.02)
    print(f"create_from_pcd: {n_points} points -> {n_anchors} anchors at voxel size {used}")
    assert used == 0.02 and n_points == 200_000 and 1000 < n_anchors < n_points and pc._anchor.shape == (n_anchors, 3)
    assert pc._anchor.is_cuda and bool(torch.isfinite(pc._scaling).all())
    with torch.no_grad():
        vis = prefilter_voxel(views[0], pc, pipe, bg)
        assert vis.shape == (n_anchors,) and int(vis.sum()) > 100
        img = render(views[0], pc, pipe, bg, visible_mask=vis)["render"]
    assert img.shape == (3, H, W) and bool(torch.isfinite(img).all())
    groups = [{"params": [getattr(pc, "_" + n)], "lr": lr, "name": n}
              for n, lr in (("anchor", 0.0), ("offset", 1e-3), ("anchor_feat", 7.5e-3), ("scaling", 7e-3))]
    groups.append({"params": [p for n, p in pc.named_parameters() if not n.startswith("_") and p.requires_grad], "lr": 2e-3,
                   "name": "mlp_and_feat_planes"})
    opt = FusedAdam(groups, eps=1e-15)
    den = AnchorDensifier(pc, opt, voxel_size=used, seed=3)
    gts = [torch.rand(3, H, W, generator=_gen(42 + i)).to(dev) for i in range(2)]
    loss, out, _ = collaborative_step(pc, views, gts, pipe, bg, optimizer=opt, densifier=den)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    for name in ("_anchor_feat", "_offset", "_scaling"):
        g = getattr(pc, name).grad
        assert g is not None and bool(torch.isfinite(g).all()) and bool(g.any()), name
    assert all(bool(torch.isfinite(p).all()) for p in pc.parameters())
