#!/usr/bin/env python3
"""Time the bilateral-grid operators (splatco_amd.bilagrid, csrc/bilagrid.hip) with HIP events, in one process:

  slice      forward + backward (gradients to the image and to the grid) at 1920x1080 with the default (8, 16, 16) grid:
             `fused` = bilagrid.slice_apply, `chain` = the same definition in float32 torch ops (a 5-D F.grid_sample with
             align_corners=True and border padding, then the affine transform; autograd for the backward);
  tv         bilagrid.tv_add_grad on N = 300 grids against the float32 autograd of the term as written;
  indexing   BilateralGrid(300)(image, i) -- the operator on grids[i], whose backward has autograd build a full-size zero
             gradient of all N grids (29 MB at N = 300) -- against the operator on a stand-alone grid.

The variants of a group are timed in interleaved rounds after the clocks have settled under load (bench.settle_clocks); per
variant the median over the rounds and the spread (max - min) of its rounds are printed.  The table goes to stdout and into
--out, where it replaces the section under SECTION (the file's other sections are kept).  No test asserts a speed."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECTION = "## timing (tools/time_bilagrid.py)"


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


def chain_slice(grid, rgb):
    """The definition in float32 framework ops."""
    _, H, W = rgb.shape
    x = (torch.arange(W, dtype=rgb.dtype, device=rgb.device) + 0.5) / W
    y = (torch.arange(H, dtype=rgb.dtype, device=rgb.device) + 0.5) / H
    z = ((0.299 * rgb[0] + 0.587 * rgb[1]) + 0.114 * rgb[2]).clamp(0, 1)
    pts = torch.stack([(2 * x - 1).reshape(1, W).expand(H, W), (2 * y - 1).reshape(H, 1).expand(H, W), 2 * z - 1], dim=-1)
    A = F.grid_sample(grid.unsqueeze(0), pts.reshape(1, 1, H, W, 3), mode="bilinear", padding_mode="border", align_corners=True)
    A = A.reshape(3, 4, H, W)
    return (A[:, :3] * rgb.unsqueeze(0)).sum(1) + A[:, 3]


def chain_tv(grids):
    N = grids.shape[0]
    total = 0
    for dim in (2, 3, 4):
        n = grids.shape[dim]
        diff = grids.narrow(dim, 1, n - 1) - grids.narrow(dim, 0, n - 1)
        total = total + (diff * diff).sum() / (diff.numel() // N)
    return total / N


def measure(group, variants, args, dev, bench):
    """[(name, median ms, spread ms)] of one group's variants, interleaved."""
    for _, fn in variants:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    bench.settle_clocks(variants[0][1], 1, dev)
    ms = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            ms[name].append(timed(fn, args.steps))
    return [(f"{group} {name}", statistics.median(v), max(v) - min(v)) for name, v in ms.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per round and variant")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--views", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_bilagrid.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_bilagrid.py needs an MI355X: there is no CPU timing"
    import bench
    from splatco_amd.bilagrid import BilateralGrid, slice_apply, tv_add_grad
    dev = torch.device("cuda:0")
    H, W, N = args.height, args.width, args.views
    gen = torch.Generator(device=dev).manual_seed(0)
    rgb = (1.2 * torch.rand(3, H, W, device=dev, generator=gen) - 0.1).requires_grad_()
    dout = torch.randn(3, H, W, device=dev, generator=gen)
    bil = BilateralGrid(N, device=dev)
    with torch.no_grad():
        bil.grids.add_(0.05 * torch.randn(bil.grids.shape, device=dev, generator=gen))
    grid = bil.grids[N // 2].detach().clone().requires_grad_()

    def slice_variant(op):
        def run():
            rgb.grad = grid.grad = None
            op(grid, rgb).backward(dout)
        return run

    def indexed():
        rgb.grad = bil.grids.grad = None
        bil(rgb, N // 2).backward(dout)

    def tv_fused():
        tv_add_grad(bil.grids, 10.0)

    def tv_chain():
        bil.grids.grad = None
        (10.0 * chain_tv(bil.grids)).backward()

    rows = measure("slice", [("chain", slice_variant(chain_slice)), ("fused", slice_variant(slice_apply))], args, dev, bench)
    rows += measure("indexing", [("stand-alone grid", slice_variant(slice_apply)), (f"grids[i] of {N}", indexed)], args, dev, bench)
    bil.grids.grad = None
    rows += measure("tv", [("chain", tv_chain), ("fused", tv_fused)], args, dev, bench)
    with torch.no_grad():
        diff = float((slice_apply(grid, rgb) - chain_slice(grid, rgb)).abs().max())
    lines = [f"bilateral grid (8, 16, 16) at {W}x{H}, N = {N} views for tv / indexing, HIP events, {args.rounds} interleaved rounds of "
             f"{args.steps} steps after {args.warmup} warm-up steps per variant and settled clocks; ms per step",
             f"{'variant':34s} {'median':>10s} {'spread':>10s}"]
    lines += [f"{name:34s} {med:10.4f} {spread:10.4f}" for name, med, spread in rows]
    by = {name: med for name, med, _ in rows}
    lines.append(f"slice chain / fused {by['slice chain'] / by['slice fused']:.2f}; tv chain / fused {by['tv chain'] / by['tv fused']:.2f}; "
                 f"indexing overhead {by[f'indexing grids[i] of {N}'] - by['indexing stand-alone grid']:.4f} ms per view; "
                 f"largest |fused - chain| of the output {diff:.3e}")
    text = "\n".join(lines)
    print(text)
    write_section(args.out, text)


if __name__ == "__main__":
    main()
