#!/usr/bin/env python3
"""Time forward + backward of the rasterizer at the cfg1 scene (1 M synthetic Gaussians, one 1920x1080 view, loss on the
image) with HIP events, three ways:

  (a) colour only, on ANOTHER tree's build (--parent-root: a checkout of the parent commit with its library built);
  (b) colour only, on this build;
  (c) this build with all three camera tensors requiring grad (dL/dviewmatrix, dL/dprojmatrix, dL/dcampos).

Two builds of the library cannot share a process, so every round starts one fresh process per tree, one after the other
(the way tools/ab.sh interleaves builds): the parent's measures (a), this tree's measures (b) and (c) interleaved.  Each
process warms up, lets the clocks settle under load (bench.settle_clocks) and prints the median of its blocks.  The
summary has per variant the median over the rounds and the spread (max - min) of its rounds, (b) - (a) and (c) - (b).
Without --parent-root only (b) and (c) are measured.  With --once the worker runs a few steps of (b) and (c) and prints
nothing but a line per variant: what a `rocprofv3 --kernel-trace --stats -- python tools/time_camera_grad.py --once` run
traces (preprocess_backward_kernel<false, false> against <false, true>, camera_grad_finish_kernel).  No test asserts a speed."""
import argparse
import json
import os
import statistics
import subprocess
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


def worker(args):
    """One process on one tree (args.root): the median ms per step of each variant that tree has, as one JSON line."""
    sys.path.insert(0, args.root)
    import torch
    import bench
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
    Gc = torch.randn(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    camera = [x.detach().clone().requires_grad_() for x in (rs.viewmatrix, rs.projmatrix, rs.campos)]
    rast = GaussianRasterizer(rs)
    rast_cam = GaussianRasterizer(rs._replace(viewmatrix=camera[0], projmatrix=camera[1], campos=camera[2]))

    def step(r):
        for p in list(params.values()) + [means2D] + camera:
            p.grad = None
        img, _ = r(means2D=means2D, **params)
        img.backward(Gc)

    variants = [("colour", lambda: step(rast))]
    if args.camera:
        variants.append(("camera", lambda: step(rast_cam)))
    for _, fn in variants:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    if args.camera:
        assert all(c.grad is not None and torch.isfinite(c.grad).all() for c in camera) and float(camera[0].grad.abs().max()) > 0
    if args.once:
        for name, fn in variants:
            print(f"{name}: {timed(torch, fn, args.steps):.4f} ms per step ({args.steps} steps, clocks not settled)")
        return
    bench.settle_clocks(variants[-1][1], 1, dev)
    ms = {name: [] for name, _ in variants}
    for _ in range(args.blocks):
        for name, fn in variants:
            ms[name].append(timed(torch, fn, args.steps))
    print(json.dumps({name: statistics.median(v) for name, v in ms.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit, library built: measures (a)")
    ap.add_argument("--steps", type=int, default=20, help="steps per block")
    ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per process")
    ap.add_argument("--rounds", type=int, default=4, help="processes per tree")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="a few steps of (b) and (c) in this process (for a kernel trace)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--camera", type=int, default=1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker or args.once:
        return worker(args)

    def run(root, camera):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", os.path.abspath(root), "--camera", str(camera),
               "--steps", str(args.steps), "--blocks", str(args.blocks), "--warmup", str(args.warmup)]
        env = {k: v for k, v in os.environ.items() if k != "SPLATCO_RASTER_LIB"}
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=os.path.abspath(root))
        if r.returncode != 0:      # nothing more is started on the GPU after a failed process
            raise SystemExit(f"worker on {root} failed with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])

    ms = {"a": [], "b": [], "c": []}
    for _ in range(args.rounds):
        if args.parent_root:
            ms["a"].append(run(args.parent_root, 0)["colour"])
        here = run(HERE, 1)
        ms["b"].append(here["colour"])
        ms["c"].append(here["camera"])
    names = {"a": "(a) colour only, parent build", "b": "(b) colour only, this build", "c": "(c) camera gradients    "}
    print(f"cfg1 scene, forward + backward, {args.rounds} rounds of one process per tree, {args.blocks} blocks of "
          f"{args.steps} steps each (median per process)")
    med = {}
    for k, v in ms.items():
        if v:
            med[k] = statistics.median(v)
            print(f"{names[k]:32s}: median {med[k]:.4f} ms per step, spread {max(v) - min(v):.4f} ms "
                  f"(rounds: {' '.join(f'{x:.4f}' for x in v)})")
    if "a" in med:
        print(f"(b) - (a) = {med['b'] - med['a']:+.4f} ms")
    print(f"(c) - (b) = {med['c'] - med['b']:+.4f} ms   per round: {' '.join(f'{c - b:+.4f}' for b, c in zip(ms['b'], ms['c']))}")


if __name__ == "__main__":
    main()
