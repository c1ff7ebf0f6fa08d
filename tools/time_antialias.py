#!/usr/bin/env python3
"""Time forward + backward of the rasterizer at the cfg1 scene (1 M synthetic Gaussians, one 1920x1080 view) with HIP
events, in ONE process, three cases interleaved block by block:

  (off)  loss on the image, the mode off -- the default call;
  (on)   the same with antialiased=True;
  (all)  antialiased=True together with return_aux (loss on image, depth and alpha) and the camera's gradients.

The process warms up, lets the clocks settle under load (bench.settle_clocks) and prints per case the median of its
blocks and their spread (max - min), then (on) - (off).  With --kernels the two per-Gaussian kernels are also timed per
case through the library's own event brackets (scr_profile_*: preprocess_kernel, preprocess_backward_kernel), in extra
blocks that do not enter the step times (an event pair costs a few microseconds of stream time).  With --once a few steps
of each case run and one line per case is printed: what a `rocprofv3 --kernel-trace --stats -- python
tools/time_antialias.py --once` run traces.  No test asserts a speed."""
import argparse
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="steps per block")
    ap.add_argument("--blocks", type=int, default=9, help="interleaved blocks per case")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernels", action="store_true", help="also time the two per-Gaussian kernels per case")
    ap.add_argument("--once", action="store_true", help="a few steps of each case, clocks not settled (for a kernel trace)")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    import bench
    from splatco_amd import _C
    from splatco_amd.rasterizer import GaussianRasterizer
    from splatco_amd.synthetic import synthetic_gaussians
    dev = torch.device("cuda:0")
    P, W, H = bench.P_CFG1, bench.W_CFG1, bench.H_CFG1
    g = synthetic_gaussians(P, W, H, seed=0)
    rs = bench.settings_for(bench.make_view(0, W, H), g["bg"], dev)
    t = lambda a: torch.tensor(a, device=dev, requires_grad=True)
    params = dict(means3D=t(g["means3D"]), opacities=t(g["opacities"]), colors_precomp=t(g["colors"]),
                  scales=t(g["scales"]), rotations=t(g["rotations"]))
    means2D = torch.zeros(P, 3, device=dev, requires_grad=True)
    gen = torch.Generator(device=dev).manual_seed(1)
    Gc, Gd, Ga = (torch.randn(*s, device=dev, generator=gen) for s in ((3, H, W), (H, W), (H, W)))
    camera = [x.detach().clone().requires_grad_() for x in (rs.viewmatrix, rs.projmatrix, rs.campos)]
    rast = GaussianRasterizer(rs)
    rast_cam = GaussianRasterizer(rs._replace(viewmatrix=camera[0], projmatrix=camera[1], campos=camera[2]))

    def clear():
        for p in list(params.values()) + [means2D] + camera:
            p.grad = None

    def colour(**mode):
        clear()
        img, _ = rast(means2D=means2D, **mode, **params)
        img.backward(Gc)

    def everything():
        clear()
        img, _, depth, alpha = rast_cam(means2D=means2D, return_aux=True, antialiased=True, **params)
        torch.autograd.backward((img, depth, alpha), (Gc, Gd, Ga))

    cases = [("off", lambda: colour()), ("on", lambda: colour(antialiased=True)), ("all", everything)]
    for _, fn in cases:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    assert all(c.grad is not None and torch.isfinite(c.grad).all() for c in camera)
    if args.once:
        for name, fn in cases:
            print(f"{name}: {timed(torch, fn, args.steps):.4f} ms per step ({args.steps} steps, clocks not settled)")
        return
    bench.settle_clocks(cases[-1][1], 1, dev)
    ms = {name: [] for name, _ in cases}
    for _ in range(args.blocks):
        for name, fn in cases:
            ms[name].append(timed(torch, fn, args.steps))
    print(f"cfg1 scene ({P} Gaussians, {W}x{H}), forward + backward, one process, {args.blocks} interleaved blocks of "
          f"{args.steps} steps per case")
    names = {"off": "(off) mode off", "on": "(on)  antialiased", "all": "(all) antialiased + aux maps + camera gradients"}
    med = {}
    for k, v in ms.items():
        med[k] = statistics.median(v)
        print(f"{names[k]:48s}: median {med[k]:.4f} ms per step, spread {max(v) - min(v):.4f} ms "
              f"(blocks: {' '.join(f'{x:.4f}' for x in v)})")
    print(f"(on) - (off) = {med['on'] - med['off']:+.4f} ms   per block: "
          f"{' '.join(f'{b - a:+.4f}' for a, b in zip(ms['off'], ms['on']))}")
    if args.kernels:
        kernels = ("preprocess_kernel", "preprocess_backward_kernel")
        known = [_C.lib.scr_profile_kernel_name(i).decode() for i in range(_C.PROF_COUNT)]
        mask = sum(1 << known.index(k) for k in kernels)
        print("the per-Gaussian kernels (library event brackets, us per launch; extra blocks outside the step times):")
        per = {}
        for name, fn in cases:
            _C.profile_enable(mask)
            _C.profile_read()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            got = _C.profile_read()
            _C.profile_enable(0)
            per[name] = {k: 1000.0 * got[k][0] / max(got[k][1], 1) for k in kernels}
            print(f"  {names[name]:48s}: " + ", ".join(f"{k} {per[name][k]:.1f}" for k in kernels))
        for k in kernels:
            print(f"  {k}: (on) / (off) = {per['on'][k] / per['off'][k]:.3f}")


if __name__ == "__main__":
    main()
