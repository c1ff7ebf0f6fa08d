#!/usr/bin/env python3
"""Time the mesh evaluation (splatco_amd/surface_eval.py, csrc/surfeval.hip) on one MI355X:

  meshes    the 256^3 and 512^3 meshes of tools/time_tsdf.py (its scene, its 64 views of 1920x1080 maps, fused and extracted);
  timed     sample_surface at the spacing that yields about as many samples as the mesh has vertices, nearest from those samples
            into a ground-truth cloud of the same size (the same surface sampled under another seed), score of the two distance
            lists, and the whole evaluate_mesh, each a whole call as a user makes it (validation, host reads, bucketing and
            allocations included);
  floaters  nearest with 1 % of the queries moved 50 extents away, without and with max_dist: what a floater costs;
  baselines the same float32 definition as chunked torch ops on the device (differences, squares, amin over chunks of queries),
            on growing subsets until the next size would take more than a minute, and scipy.spatial.cKDTree on the host where
            scipy imports, device-to-host copies included.

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

SECTION = "## timing (tools/time_surfeval.py)"


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


def torch_nearest(query, target, chunk_elems=1 << 28):
    """The definition in float32 torch ops, chunked over the queries: what a caller writes without the fused search."""
    nq, nt = query.shape[0], target.shape[0]
    chunk = max(1, chunk_elems // nt)
    d2 = torch.empty(nq, dtype=torch.float32, device=query.device)
    idx = torch.empty(nq, dtype=torch.int64, device=query.device)
    tx, ty, tz = (target[:, k].contiguous()[None, :] for k in range(3))
    for s in range(0, nq, chunk):
        q = query[s:s + chunk]
        ex, ey, ez = tx - q[:, 0:1], ty - q[:, 1:2], tz - q[:, 2:3]
        d = (ex * ex + ey * ey) + ez * ez
        d2[s:s + chunk], idx[s:s + chunk] = torch.min(d, dim=1)
    return d2, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=1)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_surfeval.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_surfeval.py needs an MI355X: there is no CPU timing"
    assert args.rounds >= 5, "medians of at least 5 rounds"
    import bench
    from splatco_amd.surface_eval import evaluate_mesh, nearest, sample_surface, score
    from splatco_amd.tsdf import TSDFVolume
    tt = _time_tsdf()
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    dev = torch.device("cuda:0")
    H, W, V = args.height, args.width, args.views
    fx = W / (2.0 * math.tan(math.radians(60.0) * 0.5))
    intr = (fx, fx, W * 0.5, H * 0.5)
    gen = torch.Generator(device=dev).manual_seed(0)
    cams, D, A = [], [], []
    for i in range(V):
        ang = 2.0 * math.pi * (i + 0.3) / V
        eye = (tt.CENTRE[0] + 3.0 * math.cos(ang), tt.CENTRE[1] + 3.0 * math.sin(ang), tt.CENTRE[2] + 0.9 + 0.5 * math.sin(3 * ang))
        w2c = tt.look_at(eye, tt.CENTRE, dev)
        d, a, _ = tt.render_view(H, W, intr, w2c, dev, gen)
        cams.append((intr, w2c)); D.append(d); A.append(a)
    med = lambda ms: statistics.median(ms)
    fmt = lambda ms: f"{med(ms):9.3f} ms ({min(ms):.3f} - {max(ms):.3f})"

    def measure(fn, rounds=None):
        first = wall(fn)
        if first > 5000.0:                                  # seconds per call: three rounds, no clock settling
            return [first] + [wall(fn) for _ in range(2)]
        bench.settle_clocks(fn, 1, dev)
        return [wall(fn) for _ in range(rounds or args.rounds)]

    lines = [f"Mesh evaluation on the meshes of tools/time_tsdf.py ({V} views of {W}x{H} maps, sphere over a plane), host clock around each whole "
             f"call and a device synchronise, median (min - max) of {args.rounds} rounds after a warm-up call and settled clocks (3 rounds, the "
             f"warm-up among them, where a call takes more than 5 s); host baselines {args.host_rounds} round(s)"]
    lo_w = [c - 1.0 for c in tt.CENTRE]
    for n in args.sizes:
        vol = TSDFVolume(lo_w, 2.0 / (n - 1), (n, n, n), color=False, device=dev)
        vol.integrate_views(D, A, cams, None)
        v, f = vol.extract()[:2]
        del vol
        torch.cuda.empty_cache()
        tag, nv, nf = f"{n}^3", v.shape[0], f.shape[0]
        p = [v[f[:, k].long()] for k in range(3)]
        area = float(0.5 * torch.linalg.cross(p[1] - p[0], p[2] - p[0]).double().norm(dim=1).sum())
        del p
        spacing = math.sqrt(area / nv)
        pred, _ = sample_surface(v, f, spacing=spacing, seed=0)
        gt, _ = sample_surface(v, f, spacing=spacing, seed=1)
        ns, ng = pred.shape[0], gt.shape[0]
        tau = (2.0 * spacing, 5.0 * spacing)
        lines.append(f"[{tag}] {nv} vertices, {nf} faces, area {area:.4f}; spacing {spacing:.6f}: {ns} samples (seed 0) against a cloud of {ng} "
                     f"(the same surface, seed 1); thresholds 2 and 5 spacings")
        print(lines[-1], flush=True)
        a, _ = nearest(pred, gt)
        b, _ = nearest(gt, pred)
        res = evaluate_mesh(v, f, gt, spacing, thresholds=tau)
        lines.append(f"[{tag}] evaluate_mesh: accuracy {res['accuracy']:.6f}, completeness {res['completeness']:.6f}, chamfer {res['chamfer']:.6f}, "
                     f"fscore {res['fscore'][0]:.4f} / {res['fscore'][1]:.4f}")
        ms_s = measure(lambda: sample_surface(v, f, spacing=spacing, seed=0))
        ms_n = measure(lambda: nearest(pred, gt))
        ms_sc = measure(lambda: score(a, b, tau))
        ms_e = measure(lambda: evaluate_mesh(v, f, gt, spacing, thresholds=tau))
        lines.append(f"[{tag}] sample_surface ({ns} samples):       {fmt(ms_s)}")
        lines.append(f"[{tag}] nearest ({ns} into {ng}):    {fmt(ms_n)}")
        lines.append(f"[{tag}] score ({ns} + {ng} distances): {fmt(ms_sc)}")
        lines.append(f"[{tag}] evaluate_mesh (sample, nearest both ways, score): {fmt(ms_e)}")
        print("\n".join(lines[-4:]), flush=True)
        # floaters: 1 % of the queries 50 extents away, in random directions
        ext = float((gt.amax(0) - gt.amin(0)).max())
        fl = pred.clone()
        step = torch.arange(0, ns, 100, device=dev)
        g = torch.randn(step.shape[0], 3, device=dev, generator=gen)
        fl[step] += 50.0 * ext * g / g.norm(dim=1, keepdim=True)
        cap = 10.0 * spacing
        ms_f = measure(lambda: nearest(fl, gt))
        ms_fc = measure(lambda: nearest(fl, gt, max_dist=cap))
        ms_nc = measure(lambda: nearest(pred, gt, max_dist=cap))
        lines.append(f"[{tag}] nearest, {step.shape[0]} of the queries (1 %) moved 50 extents away: {fmt(ms_f)} without max_dist, {fmt(ms_fc)} with "
                     f"max_dist = 10 spacings; without floaters and with that max_dist: {fmt(ms_nc)}")
        print(lines[-1], flush=True)
        # chunked torch ops: growing subsets, until the next would take more than a minute
        size, last = min(50000, ns), None
        while True:
            q, t = pred[:size], gt[:min(size, ng)]
            ms = wall(lambda: torch_nearest(q, t))
            ms = min(ms, wall(lambda: torch_nearest(q, t)))
            fused = measure(lambda: nearest(q, t))
            same = bool(torch.equal(torch_nearest(q, t)[0], nearest(q, t)[0]))
            last = (size, ms, med(fused), same)
            print(f"[{tag}] chunked torch at {size}: {ms:.1f} ms", flush=True)
            nxt = min(2 * size, ns)
            if nxt == size or ms * (nxt / size) ** 2 > 60000.0:
                break
            size = nxt
        lines.append(f"[{tag}] chunked float32 torch ops (differences, squares, min over chunks of 2^28 pairs) at {last[0]} into {last[0]}, the largest "
                     f"size it finishes in under a minute (quadratic: twice the size is four times the time): {last[1]:.1f} ms (best of 2); the "
                     f"fused search at that size: {last[2]:.3f} ms; torch / fused = {last[1] / last[2]:.0f}; distances equal bit for bit: {last[3]}")
        if cKDTree is None:
            lines.append(f"[{tag}] host baseline: scipy absent")
        else:
            def host():
                ph, gh = pred.cpu().numpy().astype(np.float64), gt.cpu().numpy().astype(np.float64)
                return cKDTree(gh).query(ph)[0], cKDTree(ph).query(gh)[0]
            ms_h = [wall(host) for _ in range(args.host_rounds)]
            both = measure(lambda: (nearest(pred, gt), nearest(gt, pred)))
            lines.append(f"[{tag}] host baseline (both clouds to the host, two scipy cKDTree builds and queries, one thread): {fmt(ms_h)}; nearest both ways "
                         f"on the device: {fmt(both)}; host / device = {med(ms_h) / med(both):.0f}")
        print("\n".join(lines[-2:]), flush=True)
        del v, f, pred, gt, a, b, fl
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    tt.SECTION = SECTION
    tt.write_section(args.out, text)


if __name__ == "__main__":
    main()
