#!/usr/bin/env python3
"""Time the mesh clean-up (splatco_amd/mesh.py, csrc/mesh.hip) on one MI355X:

  meshes    the 256^3 and 512^3 meshes of tools/time_tsdf.py (its scene, its 64 views of 1920x1080 maps, fused with colour
            and extracted), and a floater-rich variant of the largest: the same mesh with --floaters small closed shells
            (octahedra of 8 faces, edge about one voxel) appended at random places;
  timed     connected_components, clean_mesh(keep_largest=50, min_faces=50) and vertex_normals, each a whole call as a user
            makes it (validation, host reads and allocations included), and of the normals the key sort alone;
  baselines the device-to-host copy of the faces plus scipy.sparse.csgraph.connected_components where scipy imports, and a
            float32 torch restatement of the normals (index_add_ of the face normals, then normalize).

Every call ends in host reads or is closed by a device synchronise, so the clock is the host's (time.perf_counter around the
call and a synchronise).  Every figure is the median of --rounds rounds after a warm-up call and settled clocks
(bench.settle_clocks); min and max are printed next to it.  The table goes to stdout and into --out, where it replaces the
section under SECTION (the file's other sections are kept).  No test asserts a speed."""
import argparse
import importlib.util
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECTION = "## timing (tools/time_mesh.py)"


def _time_tsdf():
    spec = importlib.util.spec_from_file_location("time_tsdf", os.path.join(ROOT, "tools", "time_tsdf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def torch_normals(vertices, faces):
    """Area-weighted vertex normals in float32 torch ops: what a caller writes without the fused op.  Sums with atomics (the
    order of index_add_ is not fixed), adds a face twice to a vertex it holds twice."""
    f = faces.long()
    p0, p1, p2 = vertices[f[:, 0]], vertices[f[:, 1]], vertices[f[:, 2]]
    n = torch.linalg.cross(p1 - p0, p2 - p0)
    acc = torch.zeros_like(vertices)
    for e in range(3):
        acc.index_add_(0, f[:, e], n)
    return torch.nn.functional.normalize(acc, dim=1, eps=0.0).nan_to_num_(0.0, 0.0, 0.0)


def add_floaters(vertices, faces, colors, count, size, seed):
    gen = torch.Generator(device=vertices.device).manual_seed(seed)
    dev = vertices.device
    lo, hi = vertices.amin(0), vertices.amax(0)
    centre = lo + (hi - lo) * torch.rand(count, 3, device=dev, generator=gen)
    octa_v = torch.tensor([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=torch.float32, device=dev) * size
    octa_f = torch.tensor([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], dtype=torch.int32, device=dev)
    fv = (centre[:, None, :] + octa_v[None]).reshape(-1, 3)
    ff = (octa_f[None] + (vertices.shape[0] + 6 * torch.arange(count, device=dev, dtype=torch.int32))[:, None, None]).reshape(-1, 3)
    fc = None if colors is None else torch.rand(fv.shape[0], 3, device=dev, generator=gen)
    return torch.cat((vertices, fv)), torch.cat((faces, ff)), None if colors is None else torch.cat((colors, fc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--floaters", type=int, default=20000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_mesh.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_mesh.py needs an MI355X: there is no CPU timing"
    assert args.rounds >= 5, "medians of at least 5 rounds"
    import bench
    from splatco_amd.mesh import clean_mesh, connected_components, normal_keys, vertex_normals
    from splatco_amd.tsdf import TSDFVolume
    tt = _time_tsdf()
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components as scipy_cc
    except ImportError:
        scipy_cc = None
    dev = torch.device("cuda:0")
    H, W, V = args.height, args.width, args.views
    fx = W / (2.0 * math.tan(math.radians(60.0) * 0.5))
    intr = (fx, fx, W * 0.5, H * 0.5)
    gen = torch.Generator(device=dev).manual_seed(0)
    cams, D, A, I = [], [], [], []
    for i in range(V):
        ang = 2.0 * math.pi * (i + 0.3) / V
        eye = (tt.CENTRE[0] + 3.0 * math.cos(ang), tt.CENTRE[1] + 3.0 * math.sin(ang), tt.CENTRE[2] + 0.9 + 0.5 * math.sin(3 * ang))
        w2c = tt.look_at(eye, tt.CENTRE, dev)
        d, a, img = tt.render_view(H, W, intr, w2c, dev, gen)
        cams.append((intr, w2c)); D.append(d); A.append(a); I.append(img)
    med = lambda ms: statistics.median(ms)
    fmt = lambda ms: f"{med(ms):9.3f} ms ({min(ms):.3f} - {max(ms):.3f})"

    def measure(fn, rounds=None):
        fn()
        bench.settle_clocks(fn, 1, dev)
        return [wall(fn) for _ in range(rounds or args.rounds)]

    lines = [f"Mesh clean-up on the meshes of tools/time_tsdf.py ({V} views of {W}x{H} maps, sphere over a plane, fused with colour), host clock around "
             f"each whole call and a device synchronise, median (min - max) of {args.rounds} rounds after a warm-up call and settled clocks; "
             f"host baselines {args.host_rounds} rounds", "components algorithm: single-pass lock-free union-find (init, hook with compare-and-swap, flatten)"]
    lo_w, hi_w = [c - 1.0 for c in tt.CENTRE], [c + 1.0 for c in tt.CENTRE]
    meshes = []
    for n in args.sizes:
        vol = TSDFVolume(lo_w, 2.0 / (n - 1), (n, n, n), color=True, device=dev)
        vol.integrate_views(D, A, cams, I)
        meshes.append((f"{n}^3", 2.0 / (n - 1)) + vol.extract())
        del vol
        torch.cuda.empty_cache()
    del D, A, I
    tag, h, v, f, c = meshes[-1]
    meshes.append((f"{tag} + {args.floaters} floaters", h) + add_floaters(v, f, c, args.floaters, 0.7 * h, seed=1))
    for tag, h, v, f, c in meshes:
        nv, nf = v.shape[0], f.shape[0]
        labels, roots, counts = connected_components(f, nv)
        top = torch.sort(counts, descending=True).values[:4].tolist()
        v2, f2, c2, info = clean_mesh(v, f, c, keep_largest=50, min_faces=50)
        lines.append(f"[{tag}] {nv} vertices, {nf} faces, {roots.shape[0]} components (largest face counts {top}); "
                     f"clean_mesh(keep_largest=50, min_faces=50): threshold {info['threshold']}, {info['components_kept']} components, "
                     f"{info['vertices_after']} vertices and {info['faces_after']} faces kept")
        ms_cc = measure(lambda: connected_components(f, nv))
        ms_cl = measure(lambda: clean_mesh(v, f, c, keep_largest=50, min_faces=50))
        ms_vn = measure(lambda: vertex_normals(v, f))
        ms_keys = measure(lambda: normal_keys(f, nv))
        ms_tn = measure(lambda: torch_normals(v, f))
        lines.append(f"[{tag}] connected_components: {fmt(ms_cc)}")
        lines.append(f"[{tag}] clean_mesh(50, 50):   {fmt(ms_cl)}")
        lines.append(f"[{tag}] vertex_normals:       {fmt(ms_vn)}; of it the {3 * nf} keys (build + torch.sort): {fmt(ms_keys)} = "
                     f"{100 * med(ms_keys) / med(ms_vn):.0f} %")
        lines.append(f"[{tag}] float32 torch normals (index_add_): {fmt(ms_tn)}; fused / torch = {med(ms_vn) / med(ms_tn):.2f}")
        got, want = vertex_normals(v, f), torch_normals(v, f)
        both = (got.abs().sum(1) > 0) & (want.abs().sum(1) > 0)
        lines.append(f"[{tag}] fused against float32 torch normals: max |difference| {float((got - want)[both].abs().max()):.2e} over {int(both.sum())} "
                     f"vertices where both are non-zero ({nv - int(both.sum())} others)")
        if scipy_cc is None:
            lines.append(f"[{tag}] host baseline: scipy absent")
        else:
            def host():
                fh = f.cpu().numpy().astype(np.int64)
                i, j = np.concatenate((fh[:, 0], fh[:, 1])), np.concatenate((fh[:, 1], fh[:, 2]))
                g = coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(nv, nv))
                return scipy_cc(g, directed=False)
            ncomp, _ = host()
            ms_h = [wall(host) for _ in range(args.host_rounds)]
            ms_copy = [wall(lambda: f.cpu()) for _ in range(args.host_rounds)]
            lines.append(f"[{tag}] host baseline (faces to the host + scipy connected_components, {ncomp} components): {fmt(ms_h)}, of it the copy "
                         f"{fmt(ms_copy)}; host / device = {med(ms_h) / med(ms_cc):.0f}")
        del labels, roots, counts, v2, f2, c2
    text = "\n".join(lines)
    print(text)
    tt.SECTION = SECTION
    tt.write_section(args.out, text)


if __name__ == "__main__":
    main()
