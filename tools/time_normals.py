#!/usr/bin/env python3
"""Time forward + backward of the depth-map normals (normals.depth_normals, normals.normal_loss, csrc/normals.hip) at 1920x1080
with HIP events, against the float32 torch-op chain of the same definition on the same inputs, in the same process:

  chain : what a caller writes without the fused op -- the ok mask, the where-guarded division, rays, points, the sliced
          differences, cross, the guarded normalisation, pad (normals._normals_torch / _normal_loss_torch, the package's own
          torch path); autograd for the backward;
  fused : depth_normals(...) / normal_loss(...) and their backward passes.

The map in both frames under a fixed upstream [3, H, W], the loss with and without a float32 mask.  The variants are timed in
interleaved rounds after the clocks have settled under load (bench.settle_clocks); per variant the median over the rounds and
the spread (max - min) of its rounds are printed, and the two results side by side.  The table goes to stdout and into --out,
where it replaces the section under SECTION (the file's other sections -- parity figures -- are kept).  No test asserts a
speed."""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECTION = "## timing (tools/time_normals.py)"


def write_section(path, text):
    """Replace the lines from SECTION up to the next '## ' heading (or the end) of `path` by SECTION + text; create or append
    where there is no such section."""
    old = open(path).read().split("\n") if os.path.exists(path) else []
    if SECTION in old:
        i = old.index(SECTION)
        j = next((k for k in range(i + 1, len(old)) if old[k].startswith("## ")), len(old))
        new = old[:i] + [SECTION] + text.split("\n") + [""] + old[j:]
    else:
        new = old + [SECTION] + text.split("\n") + [""]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(new).rstrip("\n") + "\n")


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
    ap.add_argument("--steps", type=int, default=2000, help="steps per round and variant (0.2 s of the fused op per window)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_normals.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_normals.py needs an MI355X: there is no CPU timing"
    import bench
    from splatco_amd import normals
    from splatco_amd.cameras import look_at_camera
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    cam = look_at_camera(eye=(0.3, -0.2, 0.1), target=(1.0, 0.7, -0.4), up=(0, -1, 0), FoVx=math.radians(60), width=W, height=H).to(dev)
    intr = normals.intrinsics(cam)
    rot = cam.world_view_transform[:3, :3]
    gen = torch.Generator(device=dev).manual_seed(0)
    U = lambda *s: torch.rand(*s, device=dev, generator=gen)
    u = ((torch.arange(W, device=dev) + 0.5) / W * 2 - 1)[None, :]
    v = ((torch.arange(H, device=dev) + 0.5) / H * 2 - 1)[:, None]
    z = 2 + 0.3 * u + 0.2 * v + 0.1 * torch.sin(3 * u + 1) * torch.cos(2 * v) + 1e-3 * (U(H, W) - 0.5)
    A = 0.55 + 0.45 * U(H, W)
    A = torch.where(U(H, W) < 0.1, torch.full_like(A, 0.2), A)
    D = (A * z).requires_grad_()
    A.requires_grad_()
    with torch.no_grad():
        n0 = normals.depth_normals(D, A, cam)
        prior = n0 + 0.3 * (U(3, H, W) - 0.5) ** 3
        m = 0.25 + U(H, W)
        m = torch.where(U(H, W) < 0.2, torch.zeros_like(m), m)
        G = torch.randn(3, H, W, device=dev, generator=gen)

    def variant(kind, op, arg):
        def run():
            D.grad = A.grad = None
            if op == "map":
                if kind == "fused":
                    out = (normals.depth_normals(D, A, cam, frame=arg) * G).sum()
                else:
                    n, _ = normals._normals_torch(D, A, intr, 0.5)
                    out = ((torch.einsum("ij,jhw->ihw", rot, n) if arg == "world" else n) * G).sum()
            elif kind == "fused":
                out = normals.normal_loss(D, A, prior, cam, arg)
            else:
                out = normals._normal_loss_torch(D, A, prior, intr, arg, 0.5)[0]
            out.backward()
            return out
        return run

    cases = [("map", "camera"), ("map", "world"), ("loss", None), ("loss", m)]
    label = lambda op, arg: f"{op} {arg if isinstance(arg, str) else ('mask f32' if arg is not None else 'no mask')}"
    variants = [((kind, label(op, arg)), variant(kind, op, arg)) for op, arg in cases for kind in ("chain", "fused")]
    results = {}
    for key, fn in variants:
        for _ in range(args.warmup):
            results[key] = float(fn().detach())
    torch.cuda.synchronize()
    bench.settle_clocks(variants[0][1], 1, dev)
    ms = {key: [] for key, _ in variants}
    for _ in range(args.rounds):
        for key, fn in variants:
            ms[key].append(timed(fn, args.steps))
    lines = [f"depth normals forward + backward at {W}x{H} (min_alpha 0.5; map: sum(n * G) under a fixed G), HIP events, {args.rounds} "
             f"interleaved rounds of {args.steps} steps after {args.warmup} warm-up steps per variant and settled clocks; ms per step",
             f"{'case':14s} {'chain median':>12s} {'spread':>8s} {'fused median':>12s} {'spread':>8s} {'chain/fused':>11s}   "
             f"{'chain result':>13s} {'fused result':>13s}"]
    for op, arg in cases:
        c, f = ms[("chain", label(op, arg))], ms[("fused", label(op, arg))]
        mc, mf = statistics.median(c), statistics.median(f)
        lines.append(f"{label(op, arg):14s} {mc:12.4f} {max(c) - min(c):8.4f} {mf:12.4f} {max(f) - min(f):8.4f} {mc / mf:11.2f}   "
                     f"{results[('chain', label(op, arg))]:13.6e} {results[('fused', label(op, arg))]:13.6e}")
    text = "\n".join(lines)
    print(text)
    write_section(args.out, text)


if __name__ == "__main__":
    main()
