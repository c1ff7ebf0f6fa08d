#!/usr/bin/env python3
"""Time forward + backward of the rasterizer WITH the depth and opacity maps at the cfg1 scene (1 M synthetic Gaussians, one
1920x1080 view) with HIP events, against two baselines in the same process:

  colour only : the benchmark's step (image, loss on the image);
  two passes  : what a caller had to do before return_aux -- the colour-only operator twice, the second time on the colours
                (z, 1, 0) over a black background, z formed in torch; loss on image, depth and alpha;
  fused       : one call with return_aux=True, the same loss.

The three are timed in interleaved rounds after the clocks have settled under load (bench.settle_clocks); per variant the
median over the rounds and the spread (max - min) of its rounds are printed.  No test asserts a speed."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="steps per round and variant")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import bench
    from splatco_amd.rasterizer import GaussianRasterizer
    from splatco_amd.synthetic import synthetic_gaussians
    dev = torch.device("cuda:0")
    P, W, H = bench.P_CFG1, bench.W_CFG1, bench.H_CFG1
    g = synthetic_gaussians(P, W, H, seed=0)
    cam = bench.make_view(0, W, H)
    rs = bench.settings_for(cam, g["bg"], dev)
    rast, rast_black = GaussianRasterizer(rs), GaussianRasterizer(rs._replace(bg=torch.zeros(3, device=dev)))
    t = lambda a: torch.tensor(a, device=dev, requires_grad=True)
    params = dict(means3D=t(g["means3D"]), opacities=t(g["opacities"]), colors_precomp=t(g["colors"]),
                  scales=t(g["scales"]), rotations=t(g["rotations"]))
    means2D = torch.zeros(P, 3, device=dev, requires_grad=True)
    leaves = list(params.values()) + [means2D]
    gen = torch.Generator(device=dev).manual_seed(1)
    Gc, Gd, Ga = (torch.randn(3, H, W, device=dev, generator=gen), torch.randn(H, W, device=dev, generator=gen),
                  torch.randn(H, W, device=dev, generator=gen))
    view = rs.viewmatrix

    def clear():
        for p in leaves:
            p.grad = None

    def colour_only():
        clear()
        img, _ = rast(means2D=means2D, **params)
        img.backward(Gc)

    def two_passes():
        clear()
        img, _ = rast(means2D=means2D, **params)
        z = params["means3D"] @ view[:3, 2] + view[3, 2]
        aux_colours = torch.stack((z, torch.ones_like(z), torch.zeros_like(z)), dim=1)
        aux, _ = rast_black(means2D=means2D, **{**params, "colors_precomp": aux_colours})
        torch.autograd.backward((img, aux), (Gc, torch.stack((Gd, Ga, torch.zeros_like(Gd)))))

    def fused():
        clear()
        img, _, depth, alpha = rast(means2D=means2D, return_aux=True, **params)
        torch.autograd.backward((img, depth, alpha), (Gc, Gd, Ga))

    variants = (("colour only", colour_only), ("two passes", two_passes), ("fused", fused))
    for _, fn in variants:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    bench.settle_clocks(fused, 1, dev)
    ms = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            ms[name].append(timed(fn, args.steps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(f"cfg1 scene, {P} Gaussians {W}x{H}, forward + backward, {args.rounds} interleaved rounds of {args.steps} steps")
    for name, _ in variants:
        v = ms[name]
        print(f"{name:12s}: median {med[name]:.4f} ms per step, spread {max(v) - min(v):.4f} ms "
              f"(rounds: {' '.join(f'{x:.4f}' for x in v)})")
    print(f"fused / two passes  = {med['fused'] / med['two passes']:.3f}   "
          f"(two passes - fused = {med['two passes'] - med['fused']:.4f} ms)")
    print(f"fused / colour only = {med['fused'] / med['colour only']:.3f}")


if __name__ == "__main__":
    main()
