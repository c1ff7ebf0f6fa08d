#!/usr/bin/env python3
"""Time the dense optimizer step `FusedAdam.step()` against the row-sparse one `FusedAdam.step(visible=mask)` (csrc/adam.hip:
adam_kernel / adam_rows_kernel) on the per-anchor parameters of the cfg3 scene -- 5 M anchors in Morton order, `_anchor_feat`
[N,32], `_anchor` [N,3], `_offset` [N,10,3], `_scaling` [N,6] -- with HIP events, in ONE process, the two steps alternating
block by block for every mask:

  none      no row visible;
  all       every row visible (the dense step's work plus the mask lookups);
  cam1/cam4 the prefilter_voxel mask of one camera / the union of four cameras standing INSIDE the [-2,2]^3 box (the bench
            cameras stand outside it and see nearly everything);
  rnd1/rnd4 random masks of the same visible fractions: no runs, the stated worst case.

Per mask it prints the visible fraction, per tensor the share of its 128-byte lines that hold a visible element, the bytes
the step has to move under the model "seven streams (four read, three written) of every touched line, plus the mask once
per tensor", the median time per step of both steps with the spread of the blocks, and the masked step's rate under that
model.  The process warms up and lets the clocks settle under load (bench.settle_clocks) first.  With --once a few steps
of each case run and one line per case is printed (what a kernel trace would wrap).  --out writes the same text to a file
with a provenance stamp.  No test asserts a speed."""
import argparse
import json
import math
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("anchor_feat", "anchor", "offset", "scaling")
CAMERAS = (((0.0, 0.0, 0.0), (1.0, 0.2, 0.3)), ((0.5, -0.3, 0.2), (-1.0, 0.0, 0.5)),
           ((-0.6, 0.4, -0.5), (0.2, 1.5, -1.0)), ((0.2, 0.6, 0.9), (0.0, -0.5, -2.0)))      # (eye, target), all inside the box


def timed(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def lines_touched(torch, mask, width):
    """(lines that hold an element of a visible row, lines of the tensor) for a row-major fp32 [N, width] tensor on a
    128-byte boundary."""
    N = mask.numel()
    total = (N * width * 4 + 127) // 128
    rows = torch.nonzero(mask).reshape(-1)
    first, last = rows * (width * 4) // 128, ((rows + 1) * (width * 4) - 1) // 128
    d = torch.zeros(total + 1, dtype=torch.int32, device=mask.device)
    one = torch.ones_like(first, dtype=torch.int32)
    d.index_add_(0, first, one)
    d.index_add_(0, last + 1, -one)
    return int((torch.cumsum(d[:total], 0) > 0).sum()), total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=20, help="steps per block")
    ap.add_argument("--blocks", type=int, default=9, help="interleaved blocks per step kind and mask")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="a few steps of each case, clocks not settled (for a kernel trace)")
    ap.add_argument("--out", default=None, help="also write the table, with a provenance stamp, to this file")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import types
    import torch
    import bench
    from provenance import stamp
    from splatco_amd.adam import FusedAdam
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.renderer import prefilter_voxel
    from splatco_amd.synthetic import ANCHOR_CONFIGS, synthetic_anchor_model
    dev = torch.device("cuda:0")
    N, W, H = args.anchors, 1920, 1080
    # the cfg3 anchors (the planes play no part in the optimizer step of the per-anchor groups: kept small)
    pc = synthetic_anchor_model(N, ANCHOR_CONFIGS["cfg3"][2], dev, plane_size=64)
    pc.sort_anchors()
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    bg = torch.ones(3, device=dev)
    cams = [look_at_camera(eye, target, (0.0, -1.0, 0.0), math.radians(60.0), W, H, uid=i).to(dev)
            for i, (eye, target) in enumerate(CAMERAS)]
    with torch.no_grad():
        vis = [prefilter_voxel(c, pc, pipe, bg) for c in cams]
    cam1, cam4 = vis[0], vis[0] | vis[1] | vis[2] | vis[3]
    gen = torch.Generator(device=dev).manual_seed(12)
    rnd = lambda m: torch.rand(N, device=dev, generator=gen) < float(m.float().mean())
    masks = [("none", torch.zeros(N, dtype=torch.bool, device=dev)), ("all", torch.ones(N, dtype=torch.bool, device=dev)),
             ("cam1", cam1), ("cam4", cam4), ("rnd1", rnd(cam1)), ("rnd4", rnd(cam4))]
    params = [getattr(pc, "_" + n) for n in NAMES]
    widths = [p.numel() // N for p in params]
    opt = FusedAdam([{"params": [p], "lr": 1e-4, "name": n, "row_sparse": True} for n, p in zip(NAMES, params)], eps=1e-15)
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
    dense = lambda: opt.step()
    for _ in range(args.warmup):
        dense()
        for _, m in masks:
            opt.step(visible=m)
    torch.cuda.synchronize()
    lines = []
    say = lambda s="": (print(s), lines.append(s))
    if args.once:
        print(f"dense: {timed(torch, dense, args.steps):.4f} ms per step ({args.steps} steps, clocks not settled)")
        for name, m in masks:
            print(f"{name}: {timed(torch, lambda: opt.step(visible=m), args.steps):.4f} ms per step")
        return
    bench.settle_clocks(dense, 1, dev)
    dense_bytes = 7 * 4 * sum(p.numel() for p in params)
    say(f"FusedAdam.step() against step(visible=mask): {N} anchors in Morton order, widths "
        f"{' / '.join(f'{n} {w}' for n, w in zip(NAMES, widths))} ({dense_bytes / 1e9:.2f} GB per dense step), one process, "
        f"{args.blocks} alternating blocks of {args.steps} steps per step kind and mask; cameras inside the box at {W}x{H}")
    say(f"{'mask':5s} {'visible':>8s}  128-B lines touched: {' '.join(f'{n:>11s}' for n in NAMES)}  {'model GB':>8s}  "
        f"{'dense ms (spread)':>18s}  {'masked ms (spread)':>18s}  {'masked/dense':>12s}  {'model TB/s':>10s}")
    for name, m in masks:
        share, model = [], 0
        for w in widths:
            hit, total = lines_touched(torch, m, w)
            share.append(hit / total)
            model += 7 * 128 * hit + N                      # seven streams of every touched line + the mask once per tensor
        sparse = lambda: opt.step(visible=m)
        td, ts = [], []
        for _ in range(args.blocks):
            td.append(timed(torch, dense, args.steps))
            ts.append(timed(torch, sparse, args.steps))
        d, s = statistics.median(td), statistics.median(ts)
        say(f"{name:5s} {float(m.float().mean()):8.4f}  {'':21s}{' '.join(f'{x:11.4f}' for x in share)}  {model / 1e9:8.3f}  "
            f"{d:9.4f} ({max(td) - min(td):.4f})  {s:9.4f} ({max(ts) - min(ts):.4f})  {s / d:12.3f}  {model / s / 1e9:10.2f}")
    say(f"(dense step under the same model: {dense_bytes / 1e9:.3f} GB; model TB/s = model bytes / masked time)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n\nprovenance: " + json.dumps(stamp("python tools/time_sparse_adam.py " + " ".join(sys.argv[1:]))) + "\n")


if __name__ == "__main__":
    main()
