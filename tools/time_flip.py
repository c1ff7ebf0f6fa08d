#!/usr/bin/env python3
"""Time LDR-FLIP on the GPU with HIP events: the fused HIP pass (splatco_amd.metrics.flip, csrc/flip.hip) at 1920x1080
for N = 1 and N = 8, next to the reference-shaped float32 torch restatement (tests/flip_restatement.py: 2-D conv2d,
elementwise ops), and evaluate_views' per-view split between rendering and scoring on a synthetic anchor scene.
Prints one line per measurement.  No test asserts a speed."""
import argparse
import math
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--anchors", type=int, default=200_000)
    args = ap.parse_args()
    import flip_restatement as fr
    from splatco_amd.metrics import flip, flip_and_mse
    dev = torch.device("cuda:0")
    H, W = 1080, 1920
    g = torch.Generator(device=dev).manual_seed(0)
    ref = torch.nn.functional.avg_pool2d(torch.rand(8, 3, H + 4, W + 4, device=dev, generator=g), 5, stride=1).contiguous()
    test = (ref + 0.05 * torch.randn(ref.shape, device=dev, generator=g)).contiguous()
    for N in (1, 8):
        t, r = test[:N], ref[:N]
        ms = timed(lambda: flip(t, r), args.reps, args.warmup)
        ms_map = timed(lambda: flip(t, r, return_map=True), args.reps, args.warmup)
        print(f"flip HIP         N={N} {W}x{H}: {ms:8.3f} ms per call ({ms / N:.3f} ms per image); with map {ms_map:.3f} ms")
    for N in (1, 8):
        t, r = test[:N], ref[:N]
        ms = timed(lambda: fr.flip_map(t, r, dtype=torch.float32).mean((1, 2)), max(3, args.reps // 4), 1)
        print(f"flip torch fp32  N={N} {W}x{H}: {ms:8.3f} ms per call ({ms / N:.3f} ms per image)")

    # evaluate_views' split: render (prefilter + render, synchronised per view as render.py times it) vs scoring
    from splatco_amd.evaluate import render_views, score_views
    from splatco_amd.synthetic import synthetic_anchor_model, synthetic_views
    pc = synthetic_anchor_model(args.anchors, seed=1, device=dev)
    views = [v.to(dev) for v in synthetic_views(args.views, width=W, height=H)]
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False, mv=1)
    bg = torch.zeros(3, device=dev)
    render_views(views[:2], pc, pipe, bg)
    imgs, times, fps = render_views(views, pc, pipe, bg)
    gts = [im.flip(-1).contiguous() for im in imgs]
    score_views(imgs[:2], gts[:2])
    torch.cuda.synchronize()
    ms_score = timed(lambda: score_views(imgs, gts), 3, 1) / len(imgs)
    ms_flip = timed(lambda: [flip_and_mse(a, b, quantize=True) for a, b in zip(imgs, gts)], 3, 1) / len(imgs)
    tail = times[5:] if len(times) > 5 else times
    print(f"evaluate_views {args.anchors} anchors {W}x{H}, {len(views)} views: render {1e3 * sum(tail) / len(tail):.3f} ms "
          f"per view (FPS {fps:.1f}), scoring {ms_score:.3f} ms per view (of which FLIP + MSE {ms_flip:.3f} ms)")


if __name__ == "__main__":
    main()
