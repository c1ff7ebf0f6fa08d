#!/usr/bin/env python3
"""Time the block-sparse TSDF volume (splatco_amd/tsdf_sparse.py, csrc/tsdf_sparse.hip) against the dense one on one MI355X with
HIP events, on the scene, the maps and the 64 views of tools/time_tsdf.py (a sphere of radius 0.8 over a plane, 1920x1080):

  sizes    256^3 and 512^3 virtual nodes, with colour: allocated blocks and their share of the nodes, bytes held against the
           dense volume's, allocation per view (plan + run + block initialiser, one host read; on a volume that already holds
           the blocks, and the first pass that creates them), integration per view of the sparse and of the dense volume on
           the same maps, extraction of both, and the neighbour table alone;
  virtual  volumes the dense family refuses (default 1344^3 and 2048^3 nodes): blocks, bytes, the streaming pass
           (allocate + integrate per view), integration alone, extraction (in passes above 349525 blocks).

Every figure is the median of --rounds rounds after a warm-up and settled clocks (bench.settle_clocks); min and max are
printed next to it.  The table goes to stdout and into --out under SECTION.  No test asserts a speed."""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_tsdf import CENTRE, look_at, render_view, timed      # noqa: E402  (the same scene and maps)
import time_tsdf                                                # noqa: E402

SECTION = "## timing (tools/time_tsdf_sparse.py)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--virtual", type=int, nargs="*", default=[1344, 2048])
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_tsdf_sparse.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_tsdf_sparse.py needs an MI355X: there is no CPU timing"
    import bench
    from splatco_amd import _C
    from splatco_amd.tsdf import TSDFVolume, _check_dims as dense_dims
    from splatco_amd.tsdf_sparse import MAX_EXTRACT_BLOCKS, SparseTSDFVolume
    dev = torch.device("cuda:0")
    H, W, V = args.height, args.width, args.views
    fx = W / (2.0 * math.tan(math.radians(60.0) * 0.5))
    intr = (fx, fx, W * 0.5, H * 0.5)
    gen = torch.Generator(device=dev).manual_seed(0)
    cams, D, A, I = [], [], [], []
    for i in range(V):
        ang = 2.0 * math.pi * (i + 0.3) / V
        eye = (CENTRE[0] + 3.0 * math.cos(ang), CENTRE[1] + 3.0 * math.sin(ang), CENTRE[2] + 0.9 + 0.5 * math.sin(3 * ang))
        w2c = look_at(eye, CENTRE, dev)
        d, a, img = render_view(H, W, intr, w2c, dev, gen)
        cams.append((intr, w2c)); D.append(d); A.append(a); I.append(img)
    torch.cuda.synchronize()

    med = lambda ms: statistics.median(ms)
    fmt = lambda ms: f"{med(ms):9.3f} ms ({min(ms):.3f} - {max(ms):.3f})"
    lines = [f"Block-sparse TSDF volume against the dense one: {V} views of {W}x{H} maps (sphere over a plane, FoVx 60 degrees, trunc 4 h, "
             f"min_alpha 0.5, colour), HIP events, median (min - max) of {args.rounds} rounds after a warm-up pass and settled clocks"]
    lo_w = [c - 1.0 for c in CENTRE]

    def sparse_figures(n, tag):
        """Allocation, integration and extraction of the sparse volume of n^3 virtual nodes; -> (volume, ms per view of integrate)."""
        h = 2.0 / (n - 1)
        first = []

        def stream():
            vol = SparseTSDFVolume(lo_w, h, (n, n, n), device=dev)
            vol.integrate_views(D, A, cams, I)
            first.append(vol)
        stream()
        bench.settle_clocks(lambda: first[-1].integrate_views(D[:1], A[:1], cams[:1], I[:1], allocate=False), 1, dev)
        del first[:]
        ms = [timed(stream) for _ in range(max(3, args.rounds // 2))]
        vol = first[-1]
        del first[:-1]
        nb = vol.num_blocks
        share = nb * 512 / n ** 3
        lines.append(f"[{tag}] {nb} of {vol.block_dims[0] * vol.block_dims[1] * vol.block_dims[2]} blocks allocated = {100 * share:.2f} % of the "
                     f"{n ** 3} nodes; held {vol.bytes_held() / 2 ** 20:.1f} MiB (capacity {vol.capacity} rows, marks {vol._marks.numel() / 2 ** 20:.1f} MiB); "
                     f"a dense volume: {5 * 4 * n ** 3 / 2 ** 20:.1f} MiB")
        lines.append(f"[{tag}] streaming from an empty volume (allocate + integrate per view, storage grown by doubling): {fmt(ms)} for {V} views "
                     f"= {med(ms) / V:8.4f} ms per view")
        alloc = lambda: [vol.allocate(D[i], A[i], cams[i]) for i in range(V)]
        alloc()
        ms = [timed(alloc) for _ in range(args.rounds)]
        lines.append(f"[{tag}] allocation with every block already there (mark, count, one host read): {fmt(ms)} for {V} views = {med(ms) / V:8.4f} ms per view")
        run = lambda: vol.integrate_views(D, A, cams, I, allocate=False)
        run()
        ms = [timed(run) for _ in range(args.rounds)]
        moved = V * (2 * 5 * 4 * 512 * nb + 5 * 4 * H * W)
        lines.append(f"[{tag}] sparse integration, blocks given: {fmt(ms)} for {V} views = {med(ms) / V:8.4f} ms per view "
                     f"(at most {moved / 1e9:.2f} GB moved -> {moved / (med(ms) * 1e-3) / 1e12:.2f} TB/s if no block left early)")
        per_view = med(ms) / V
        table = torch.empty(nb, 27, dtype=torch.int32, device=dev)
        nbr = lambda: _C.family_call("scr_tsdfs_neighbors", n, n, n, nb, vol.keys, table, device=dev)
        nbr()
        tms = [timed(nbr) for _ in range(args.rounds)]
        ex = lambda: vol.extract()
        v, f, c = ex()
        ms = [timed(ex) for _ in range(args.rounds)]
        passes = (nb + MAX_EXTRACT_BLOCKS - 1) // MAX_EXTRACT_BLOCKS
        lines.append(f"[{tag}] sparse extract ({passes} pass{'es' if passes > 1 else ''} of at most {MAX_EXTRACT_BLOCKS} blocks): {fmt(ms)}; {v.shape[0]} vertices, "
                     f"{f.shape[0]} faces; of that the neighbour table [{nb}, 27]: {fmt(tms)}")
        del v, f, c, table
        return vol, per_view

    for n in args.sizes:
        tag = f"{n}^3"
        vol, sparse_ms = sparse_figures(n, tag)
        del vol
        torch.cuda.empty_cache()
        h = 2.0 / (n - 1)
        dense = TSDFVolume(lo_w, h, (n, n, n), device=dev)
        run = lambda: dense.integrate_views(D, A, cams, I)
        run()
        bench.settle_clocks(lambda: dense.integrate_views(D[:1], A[:1], cams[:1], I[:1]), 1, dev)
        ms = [timed(run) for _ in range(args.rounds)]
        lines.append(f"[{tag}] dense integration, one view per pass: {fmt(ms)} for {V} views = {med(ms) / V:8.4f} ms per view; "
                     f"dense / sparse = {med(ms) / V / sparse_ms:.2f}")
        ex = lambda: dense.extract()
        v, f, c = ex()
        ms = [timed(ex) for _ in range(args.rounds)]
        lines.append(f"[{tag}] dense extract: {fmt(ms)}; {v.shape[0]} vertices, {f.shape[0]} faces")
        del dense, v, f, c
        torch.cuda.empty_cache()
    for n in args.virtual:
        tag = f"{n}^3 virtual"
        try:
            dense_dims("TSDFVolume", (n, n, n))
            lines.append(f"[{tag}] the dense family accepts these dims")
        except ValueError as e:
            lines.append(f"[{tag}] dense: refused ({str(e).split(': ', 1)[1]})")
        vol, _ = sparse_figures(n, tag)
        del vol
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    time_tsdf.SECTION = SECTION
    time_tsdf.write_section(args.out, text)


if __name__ == "__main__":
    main()
