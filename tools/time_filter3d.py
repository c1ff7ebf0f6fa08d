#!/usr/bin/env python3
"""Time the 3D smoothing filter (splatco_amd/filter3d.py, csrc/filter3d.hip) with HIP events against the float32 torch-op
chains it replaces, in the same process on the same inputs:

  distance : filter3d.sampling_distance at --points points x --cameras cameras against upstream Mip-Splatting's
             compute_3D_filter, a loop of torch ops per camera (tests/filter3d_ref.py: upstream_loop);
  apply    : filter3d.apply_filter_3d forward + backward at the cfg2 scene's own V, k and P (the mask and the Gaussians of one
             render of that scene) against the same definition in float32 torch ops with autograd (filter3d_ref.apply on the
             per-Gaussian filter, an index_select of the row filter); also the bytes of the two passes computed from the
             shapes and their share of the rate scr_copy_probe reaches in this process;
  render   : render() forward + backward at cfg2 with the filter and without it.

The variants of a pair alternate round by round after a warm-up of each and settled clocks (bench.settle_clocks); per variant
the median over the rounds and the spread (max - min) are printed.  The table goes to stdout and into --out, where it
replaces the section under SECTION (the file's other sections -- the compiler's resource figures -- are kept).  No test
asserts a speed."""
import argparse
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SECTION = "## timing (tools/time_filter3d.py)"


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


def alternate(pairs, rounds, reps, warmup):
    """{name: [ms per call of every round]} of the variants, alternating round by round after `warmup` calls of each."""
    for _, fn in pairs:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in pairs}
    for _ in range(rounds):
        for name, fn in pairs:
            ms[name].append(timed(fn, reps[name] if isinstance(reps, dict) else reps))
    return ms


def row(name, v):
    return f"  {name:34s} median {statistics.median(v):10.4f} ms   spread {max(v) - min(v):8.4f} ms"


def apply_bytes(V, k, P):
    """(forward, backward) bytes the apply passes move, from the shapes: the candidates' index and the row filter in both;
    scaling + opacity read and written in the forward; scaling + opacity and both upstream gradients read and both
    gradients written in the backward."""
    head = 4 * V * k + 4 * V
    return head + 16 * P + 16 * P, head + 16 * P + 16 * P + 16 * P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=5_000_000)
    ap.add_argument("--cameras", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="calls per round of the apply pair and of the kernel of the distance pair")
    ap.add_argument("--render-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--anchors", type=int, default=0, help="anchors of the scene (default: cfg2's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_filter3d.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_filter3d.py needs an MI355X: there is no CPU timing"
    import bench
    import filter3d_ref as ref
    from test_filter3d_host import scene_cameras
    from splatco_amd import filter3d
    from splatco_amd.losses import scaling_reg
    from splatco_amd.renderer import prefilter_voxel, render
    from splatco_amd.synthetic import ANCHOR_CONFIGS, synthetic_anchor_model, synthetic_views
    dev = torch.device("cuda:0")
    lines = []
    peak = bench.hbm_copy_peak(dev)
    lines.append(f"scr_copy_probe in this process: {peak:.0f} GB/s (read + write)")

    # ---- sampling distance
    N, C = args.points, args.cameras
    gen = torch.Generator(device=dev).manual_seed(0)
    pts = (torch.rand(N, 3, device=dev, generator=gen) * 2 - 1) * 1.5
    cams = scene_cameras(C, seed=1, focal=(1000.0, 1000.0), width=1920, height=1080).to(dev)      # one focal length: upstream's case
    pairs = [("upstream's per-camera torch loop", lambda: ref.upstream_loop(pts, cams)),
             ("scr_filter3d_distance + amax/where", lambda: filter3d.compute_filter_3d(pts, cams))]
    ours, theirs = pairs[1][1](), pairs[0][1]()
    agree = float((ours - theirs).abs().max() / theirs.abs().max())
    ms = alternate(pairs, args.rounds, {pairs[0][0]: 1, pairs[1][0]: args.steps}, 1)
    lines.append(f"sampling distance, {N} points x {C} cameras (max relative difference of the two results {agree:.2e}):")
    lines += [row(name, v) for name, v in ms.items()]
    a, b = (statistics.median(ms[p[0]]) for p in pairs)
    lines.append(f"  loop / kernel = {a / b:.1f}")
    del pts, ours, theirs

    # ---- the cfg2 scene: one render gives V, k, P and the tensors of the apply pair
    n_anchors, _, seed = ANCHOR_CONFIGS["cfg2"]
    n_anchors = args.anchors or n_anchors
    W, H = 1920, 1080
    pc = synthetic_anchor_model(n_anchors, seed, dev)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    bg = torch.ones(3, device=dev)
    views = [v.to(dev) for v in synthetic_views(8, W, H)]
    target = torch.rand(3, H, W, device=dev, generator=gen)
    flt = filter3d.Filter3D(views)
    flt.update(pc)
    with torch.no_grad():
        vis = prefilter_voxel(views[0], pc, pipe, bg)
        out = render(views[0], pc, pipe, bg, visible_mask=vis)
    mask, k = out["selection_mask"], pc.n_offsets
    V, P = mask.numel() // k, out["scaling"].shape[0]
    from splatco_amd.expand import visible_indices
    row_filter = flt.values.index_select(0, visible_indices(vis))
    s = out["scaling"].detach().clone().requires_grad_()
    o = torch.rand(P, 1, device=dev, generator=gen).requires_grad_()
    gs, go = torch.randn(P, 3, device=dev, generator=gen), torch.randn(P, 1, device=dev, generator=gen)

    def fused():
        s.grad = o.grad = None
        s2, o2 = filter3d.apply_filter_3d(s, o, row_filter, mask, k)
        torch.autograd.backward((s2, o2), (gs, go))

    def chain():
        s.grad = o.grad = None
        fg = row_filter.repeat_interleave(k)[mask]
        s2, o2 = ref.apply(s, o, fg, torch.float32)
        torch.autograd.backward((s2, o2), (gs, go))

    fused()
    d_fused = (s.grad.clone(), o.grad.clone())
    chain()
    agree = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(d_fused, (s.grad, o.grad)))
    pairs = [("float32 torch ops + autograd", chain), ("scr_filter3d_apply + _backward", fused)]
    bench.settle_clocks(fused, 1, dev)
    ms = alternate(pairs, args.rounds, args.steps, args.warmup)
    fb, bb = apply_bytes(V, k, P)
    mf = statistics.median(ms[pairs[1][0]])
    lines.append(f"apply forward + backward at cfg2 ({n_anchors} anchors): V = {V}, k = {k}, P = {P} "
                 f"(max relative difference of the gradients {agree:.2e}):")
    lines += [row(name, v) for name, v in ms.items()]
    lines.append(f"  chain / fused = {statistics.median(ms[pairs[0][0]]) / mf:.1f}")
    lines.append(f"  bytes from shapes: forward {fb}, backward {bb}; both over the fused median: {(fb + bb) / (mf * 1e-3) / 1e9:.0f} GB/s "
                 f"= {100 * (fb + bb) / (mf * 1e-3) / 1e9 / peak:.0f} % of the copy rate (the median holds two launches, the autograd "
                 f"nodes and four output allocations)")
    del s, o, gs, go, d_fused

    # ---- render forward + backward with and without the filter
    def step(**kw):
        for p in pc.parameters():
            p.grad = None
        vis = prefilter_voxel(views[0], pc, pipe, bg)
        out = render(views[0], pc, pipe, bg, visible_mask=vis, retain_grad=True, **kw)
        ((out["render"] - target).abs().mean() + 0.01 * scaling_reg(out["scaling"])).backward()

    pairs = [("render() without the filter", lambda: step()), ("render(filter_3d=...)", lambda: step(filter_3d=flt))]
    ms = alternate(pairs, args.rounds, args.render_steps, args.warmup)
    lines.append(f"render() forward + backward at cfg2, {W}x{H}, prefilter included:")
    lines += [row(name, v) for name, v in ms.items()]
    a, b = (statistics.median(ms[p[0]]) for p in pairs)
    lines.append(f"  with - without = {b - a:+.4f} ms")
    head = (f"HIP events, one process, {args.rounds} alternating rounds per pair after warm-up and settled clocks; "
            f"{args.steps} calls per round (torch loop of the distance pair: 1, render: {args.render_steps})")
    text = "\n".join([head] + lines)
    print(text)
    write_section(args.out, text)


if __name__ == "__main__":
    main()
