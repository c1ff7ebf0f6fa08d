#!/usr/bin/env python3
"""Time forward + backward of the fused depth term (losses.depth_loss, csrc/depth_loss.hip) at 1920x1080 with HIP events,
against the float32 torch-op chain of the same definition on the same inputs, in the same process:

  chain : what a caller writes without the fused op -- validity mask, where-guarded division, the five moment sums and the
          closed-form fit (with alignment), the masked L1 mean; autograd for the backward;
  fused : depth_loss(...) and its backward.

Both with and without alignment, with and without a float32 mask.  The variants are timed in interleaved rounds after the
clocks have settled under load (bench.settle_clocks); per variant the median over the rounds and the spread (max - min) of its
rounds are printed, and the two losses side by side.  The table goes to stdout and into --out, where it replaces the
section under SECTION (the file's other sections -- parity figures, compiler resource figures -- are kept).  No test
asserts a speed."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


SECTION = "## timing (tools/time_depth_loss.py)"


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


def chain_loss(D, A, g, m, align, min_alpha=0.5):
    """The definition in float32 framework ops ("inverse" mode)."""
    valid = torch.isfinite(g) & torch.isfinite(D) & torch.isfinite(A) & (A >= min_alpha) & (D > 0)
    if m is not None:
        valid = valid & (m > 0)
    one, zero = torch.ones_like(D), torch.zeros_like(D)
    p = torch.where(valid, A, one) / torch.where(valid, D, one)
    gv = torch.where(valid, g, zero)
    w = valid.float() if m is None else torch.where(valid, m, zero)
    r = p - gv
    if align:
        with torch.no_grad():
            S0, Sp, Spp, Sg, Spg = w.sum(), (w * p).sum(), (w * p * p).sum(), (w * gv).sum(), (w * p * gv).sum()
            det = S0 * Spp - Sp * Sp
            ok = (valid.sum() >= 2) & (det > 1e-12 * S0 * Spp)
            s = torch.where(ok, (S0 * Spg - Sp * Sg) / torch.where(ok, det, torch.ones_like(det)), torch.ones_like(det))
            t = torch.where(ok, (Sg - s * Sp) / torch.where(ok, S0, torch.ones_like(S0)), torch.zeros_like(det))
        r = s * p + t - gv
    return (w * r.abs()).sum() / D.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500, help="steps per round and variant")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_depth_loss.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_depth_loss.py needs an MI355X: there is no CPU timing"
    import bench
    from splatco_amd.losses import depth_loss
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    gen = torch.Generator(device=dev).manual_seed(0)
    U = lambda: torch.rand(H, W, device=dev, generator=gen)
    A = 0.05 + 0.95 * U()
    D = (A * (0.5 + 7.5 * U())).requires_grad_()
    A.requires_grad_()
    with torch.no_grad():
        p = A / D
        noise = (0.05 + 0.15 * U()) * torch.where(U() < 0.5, -1.0, 1.0)
        targets = {True: 1.7 * p - 0.08 + noise, False: p + noise}        # the line each setting assumes: no residual at the kink
        m = 0.25 + U()
        m = torch.where(U() < 0.2, torch.zeros_like(m), m)

    def variant(kind, align, mask):
        g = targets[align]

        def run():
            D.grad = A.grad = None
            loss = depth_loss(D, A, g, mask, align=align) if kind == "fused" else chain_loss(D, A, g, mask, align)
            loss.backward()
            return loss
        return run

    cases = [(align, mask) for align in (True, False) for mask in (None, m)]
    variants = [((kind, align, mask is not None), variant(kind, align, mask)) for align, mask in cases for kind in ("chain", "fused")]
    losses = {}
    for key, fn in variants:
        for _ in range(args.warmup):
            losses[key] = float(fn().detach())
    torch.cuda.synchronize()
    bench.settle_clocks(variants[0][1], 1, dev)
    ms = {key: [] for key, _ in variants}
    for _ in range(args.rounds):
        for key, fn in variants:
            ms[key].append(timed(fn, args.steps))
    lines = [f"depth_loss forward + backward at {W}x{H} (inverse mode, min_alpha 0.5), HIP events, {args.rounds} interleaved rounds of "
             f"{args.steps} steps after {args.warmup} warm-up steps per variant and settled clocks; ms per step",
             f"{'align':5s} {'mask':5s} {'chain median':>12s} {'spread':>8s} {'fused median':>12s} {'spread':>8s} {'chain/fused':>11s}   "
             f"{'chain loss':>13s} {'fused loss':>13s}"]
    for align, mask in cases:
        c, f = ms[("chain", align, mask is not None)], ms[("fused", align, mask is not None)]
        mc, mf = statistics.median(c), statistics.median(f)
        lines.append(f"{str(align):5s} {'f32' if mask is not None else 'none':5s} {mc:12.4f} {max(c) - min(c):8.4f} {mf:12.4f} {max(f) - min(f):8.4f} "
                     f"{mc / mf:11.2f}   {losses[('chain', align, mask is not None)]:13.6e} {losses[('fused', align, mask is not None)]:13.6e}")
    text = "\n".join(lines)
    print(text)
    write_section(args.out, text)


if __name__ == "__main__":
    main()
