#!/usr/bin/env python3
"""Time scene initialisation from a point cloud on the GPU with device events (splatco_amd.scene_init, csrc/scene_init.hip)
for a uniform cloud in [-2, 2]^3 and a sheet (a sphere of radius 1.5) of the same N:

  voxelize   the whole call and its three stages (key pass, torch.sort, unique plan + run), each stage's share of the copy
             peak (scr_copy_probe, measured here) from its algorithmic bytes, next to the host expression
             np.unique(np.round(p / v), axis=0) * v on this box's CPU (the only baseline that exists; run once, it takes
             tens of seconds);
  dist2      the fused 3-NN kernel alone and the whole call (bucketing included), alternated in one process with what the
             library could do for the same result before: densify._knn_indices(points, 3), a torch gather and a mean;
  kNN        densify._knn_indices(points, 10), the curvature pass's search: the whole call and scr_knn alone.

Every device time is the median of --reps runs after --warmup; min and max are printed next to it.  Prints one line
per measurement, the first a provenance stamp (tools/provenance.py).  No test asserts a speed."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def timed(fn, reps, warmup):
    """[ms] of `reps` separately timed runs of fn (device events), after `warmup` untimed ones."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def fmt(ms):
    return f"{statistics.median(ms):9.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, n = {len(ms)})"


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def clouds(n, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    uniform = torch.rand(n, 3, device=dev, generator=g) * 4 - 2
    x = torch.randn(n, 3, device=dev, generator=g)
    sheet = (x / x.norm(dim=1, keepdim=True) * 1.5).contiguous()
    return {"uniform": uniform, "sheet": sheet}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy baseline")
    args = ap.parse_args()
    import provenance
    from splatco_amd import _C, knn_grid, scene_init as si
    from splatco_amd.densify import _knn_indices
    print("# provenance: " + json.dumps(provenance.stamp(" ".join(["tools/time_scene_init.py"] + sys.argv[1:]))))
    dev = torch.device("cuda:0")
    N, v = args.points, args.voxel_size
    st = _C.stream(dev)
    print(f"# {torch.cuda.get_device_name(0)}; host {cpu_model()}, {os.cpu_count()} logical CPUs, torch threads {torch.get_num_threads()}, "
          f"numpy {np.__version__}; N = {N}, v = {v}")

    a = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    ms = timed(lambda: _C.check(_C.lib.scr_copy_probe(a.data_ptr(), b.data_ptr(), a.numel(), st)), args.reps, args.warmup)
    peak = 2 * a.numel() / (statistics.median(ms) * 1e-3)                 # bytes / s, read + write
    print(f"copy probe 256 MiB: {fmt(ms)} -> {peak / 1e12:.2f} TB/s (read + write)")
    del a, b

    def share(nbytes, ms):
        return f"{nbytes / (statistics.median(ms) * 1e-3) / 1e12:.2f} TB/s, {100 * nbytes / (statistics.median(ms) * 1e-3) / peak:.0f} % of the copy peak"

    for name, p in clouds(N, dev).items():
        t_bounds = timed(lambda: knn_grid.bounds(p), args.reps, args.warmup)
        print(f"[{name}] bounding box + finite check (read back): {fmt(t_bounds)}  12 B / point: {share(12 * N, t_bounds)}")
        # ---- voxelize
        vv, lo, ext = si._voxel_range(p, v)
        assert (ext < (1 << si._PACK_BITS)).all()
        lo_host = _C.host_array([int(x) for x in lo], _C.i32)
        keys = torch.empty(N, dtype=torch.long, device=dev)
        key_pass = lambda: _C.check(_C.lib.scr_voxel_keys(N, p.data_ptr(), float(vv), lo_host, 1, keys.data_ptr(), st))
        t_keys = timed(key_pass, args.reps, args.warmup)
        t_sort = timed(lambda: torch.sort(keys).values, args.reps, args.warmup)
        skeys = torch.sort(keys).values
        scratch = _C.scratch(_C.lib.scr_voxel_unique_scratch_bytes(N), dev)
        cnt = C.c_int64(0)
        _C.check(_C.lib.scr_voxel_unique_plan(N, skeys.data_ptr(), scratch.data_ptr(), C.byref(cnt), st))
        M = cnt.value
        out = torch.empty(M, 3, device=dev)

        def unique():
            _C.check(_C.lib.scr_voxel_unique_plan(N, skeys.data_ptr(), scratch.data_ptr(), C.byref(cnt), st))
            _C.check(_C.lib.scr_voxel_unique_run(N, skeys.data_ptr(), scratch.data_ptr(), float(vv), lo_host, out.data_ptr(), st))

        t_uniq = timed(unique, args.reps, args.warmup)
        t_all = timed(lambda: si.voxelize(p, v), args.reps, args.warmup)
        print(f"[{name}] voxelize {N} -> {M} rows: whole call {fmt(t_all)}")
        print(f"[{name}]   key pass          {fmt(t_keys)}  20 B / point: {share(20 * N, t_keys)}")
        print(f"[{name}]   torch.sort (int64) {fmt(t_sort)}")
        print(f"[{name}]   unique plan + run {fmt(t_uniq)}  16 B / key + 12 B / row: {share(16 * N + 12 * M, t_uniq)}")
        del keys, skeys, out
        if not args.no_host:
            ph = p.cpu().numpy()
            t0 = time.perf_counter()
            ref = np.unique(np.round(ph / np.float32(v)), axis=0) * np.float32(v)
            t_host = time.perf_counter() - t0
            same = np.array_equal(ref, si.voxelize(p, v).cpu().numpy())
            print(f"[{name}]   host np.unique(np.round(p / v), axis=0) * v: {t_host:.2f} s, once ({cpu_model()}); "
                  f"device call / host = 1 / {t_host * 1e3 / statistics.median(t_all):.0f}; same rows: {same}")
            del ref, ph

        # ---- dist2: fused against _knn_indices + gather + mean, alternating
        def parent():
            idx = _knn_indices(p, 3)
            e = p[idx] - p[:, None, :]
            return (e * e).sum(-1).mean(-1)

        grid, spts, order, cell_start = knn_grid.buckets(p)
        res = torch.empty(N, device=dev)
        kernel = lambda: _C.check(_C.lib.scr_knn3_dist2(N, grid, spts.data_ptr(), order.data_ptr(), cell_start.data_ptr(),
                                                        res.data_ptr(), st))
        t_kernel = timed(kernel, args.reps, args.warmup)
        del spts, order, cell_start
        t_new, t_old = [], []
        si.dist2(p), parent()
        for _ in range(args.reps):
            t_new += timed(lambda: si.dist2(p), 1, 0)
            t_old += timed(parent, 1, 0)
        d_new, d_old = si.dist2(p), parent()
        rel = float(((d_new - d_old).abs() / d_old.clamp_min(1e-30)).max())
        print(f"[{name}] dist2 {N} points: fused kernel alone {fmt(t_kernel)}  ({N / statistics.median(t_kernel) / 1e6:.2f} G points / s)")
        print(f"[{name}]   whole call (bucketing + kernel) {fmt(t_new)}")
        print(f"[{name}]   _knn_indices(p, 3) + gather + mean {fmt(t_old)}  -> {statistics.median(t_old) / statistics.median(t_new):.2f} x the fused call; "
              f"max relative difference of the two results {rel:.2e}")
        # ---- the curvature pass's kNN, k = 10 (the same buckets, the same search, another policy of what to keep)
        grid, spts, order, cell_start = knn_grid.buckets(p)
        idx = torch.empty(N, 10, dtype=torch.long, device=dev)
        knn = lambda: _C.check(_C.lib.scr_knn(N, 10, grid, spts.data_ptr(), order.data_ptr(), cell_start.data_ptr(),
                                              idx.data_ptr(), st))
        t_knn = timed(knn, args.reps, args.warmup)
        del spts, order, cell_start, idx
        t_knn_all = timed(lambda: _knn_indices(p, 10), args.reps, args.warmup)
        print(f"[{name}] kNN k = 10, {N} points: scr_knn alone {fmt(t_knn)}  ({N / statistics.median(t_knn) / 1e6:.2f} G points / s)")
        print(f"[{name}]   whole call _knn_indices(p, 10) {fmt(t_knn_all)}")
        del p
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
