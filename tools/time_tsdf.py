#!/usr/bin/env python3
"""Time the TSDF fusion and the mesh extraction (splatco_amd/tsdf.py, csrc/tsdf.hip) on one MI355X with HIP events:

  volumes  256^3 and 512^3 nodes around a synthetic scene (a sphere of radius 0.8 over a plane), 64 views of 1920x1080 maps on
           an orbit, rendered here in torch ops (depth = alpha z, alpha in [0.6, 1), a smooth image);
  fused    TSDFVolume.integrate_views over the 64 views, 16 per pass (and 1 per pass), with and without colour: ms per view,
           and per pass the bytes the definition moves (volume read + written once, the maps of the batch read once) over the
           time, against the copy peak (scr_copy_probe, measured in the same run);
  chain    the same definition in float32 torch ops, one view at a time (chain_integrate below: what a caller writes without
           the fused op), on the first --chain-views views;
  extract  TSDFVolume.extract of the fused volume: ms, vertices, faces.

Every figure is the median of --rounds rounds after a warm-up and settled clocks (bench.settle_clocks); min and max are
printed next to it.  The table goes to stdout and into --out, where it replaces the section under SECTION (the file's other
sections are kept).  No test asserts a speed."""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECTION = "## timing (tools/time_tsdf.py)"
CENTRE, RADIUS, PLANE_Z = (0.05, -0.03, 0.1), 0.8, -0.7


def write_section(path, text):
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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def look_at(eye, target, dev):
    """World-to-camera [4, 4] float64 (COLMAP: +x right, +y down, +z forward), world z up."""
    eye, target = torch.tensor(eye, dtype=torch.float64), torch.tensor(target, dtype=torch.float64)
    f = (target - eye) / (target - eye).norm()
    down = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64)
    d = down - (down @ f) * f
    d = d / d.norm()
    r = torch.linalg.cross(d, f)
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3] = torch.stack((r, d, f))
    M[:3, 3] = -M[:3, :3] @ eye
    return M.float().double()


def render_view(H, W, intr, w2c, dev, gen):
    """(depth, alpha, image) of the analytic scene through the pixel centres, float32 on the device."""
    fx, fy, cx, cy = intr
    R, t = w2c[:3, :3].to(dev), w2c[:3, 3].to(dev)
    eye = -(R.T @ t)
    px = (torch.arange(W, device=dev, dtype=torch.float64) + 0.5 - cx) / fx
    py = (torch.arange(H, device=dev, dtype=torch.float64) + 0.5 - cy) / fy
    ray = torch.stack((px[None, :].expand(H, W), py[:, None].expand(H, W), torch.ones(H, W, device=dev, dtype=torch.float64)), -1) @ R
    oc = eye - torch.tensor(CENTRE, device=dev, dtype=torch.float64)
    a, b, c = (ray * ray).sum(-1), 2.0 * (ray @ oc), oc @ oc - RADIUS ** 2
    disc = b * b - 4 * a * c
    inf = torch.full_like(a, float("inf"))
    ts = torch.where(disc > 0, (-b - disc.abs().sqrt()) / (2 * a), inf)
    ts = torch.where(ts > 0, ts, inf)
    tp = (PLANE_Z - eye[2]) / ray[..., 2]
    tp = torch.where(torch.isfinite(tp) & (tp > 0), tp, inf)
    z = torch.minimum(ts, tp)
    hit = torch.isfinite(z) & (z < 50.0)
    z = torch.where(hit, z, torch.ones_like(z))
    P = eye + ray * z[..., None]
    A = torch.where(hit, 0.6 + 0.4 * torch.rand(H, W, device=dev, generator=gen, dtype=torch.float64), torch.zeros_like(z))
    image = 0.5 + 0.5 * torch.sin(P.permute(2, 0, 1) * torch.tensor([3.0, 4.0, 5.0], device=dev, dtype=torch.float64)[:, None, None])
    return (A * z).float().contiguous(), A.float().contiguous(), image.float().contiguous()


def chain_integrate(tsdf, weight, color, lo, h, trunc, depth, alpha, image, intr, w2c, min_alpha=0.5, near=0.05, max_weight=255.0):
    """One view into the volume, the module's definition in float32 torch ops (in place through torch.where + copy_)."""
    nz, ny, nx = tsdf.shape
    dev = tsdf.device
    H, W = depth.shape
    fx, fy, cx, cy = intr
    M = w2c.float().to(dev)
    x = (lo[0] + h * torch.arange(nx, device=dev, dtype=torch.float32))[None, None, :]
    y = (lo[1] + h * torch.arange(ny, device=dev, dtype=torch.float32))[None, :, None]
    z = (lo[2] + h * torch.arange(nz, device=dev, dtype=torch.float32))[:, None, None]
    row = lambda r: ((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]
    xc, yc, zc = row(0), row(1), row(2)
    front = zc > near
    zs = torch.where(front, zc, torch.ones_like(zc))
    u = torch.floor(fx * xc / zs + cx)
    v = torch.floor(fy * yc / zs + cy)
    ok = front & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    pix = torch.where(ok, v * W + u, torch.zeros_like(u)).long().reshape(-1)
    d_ = depth.reshape(-1)[pix].reshape(nz, ny, nx)
    a_ = alpha.reshape(-1)[pix].reshape(nz, ny, nx)
    ok = ok & torch.isfinite(d_) & torch.isfinite(a_) & (a_ >= min_alpha) & (d_ > 0)
    one = torch.ones_like(d_)
    sdf = torch.where(ok, d_, one) / torch.where(ok, a_, one) - zc
    upd = ok & (sdf >= -trunc)
    d = torch.clamp(sdf / trunc, max=1.0)
    den = weight + 1.0
    tsdf.copy_(torch.where(upd, (tsdf * weight + d) / den, tsdf))
    if color is not None and image is not None:
        img = image.reshape(3, -1)[:, pix].reshape(3, nz, ny, nx)
        cu = upd & torch.isfinite(img).all(0)
        color.copy_(torch.where(cu, (color * weight + img) / den, color))
    weight.copy_(torch.where(upd, torch.clamp(den, max=max_weight), weight))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--chain-views", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_tsdf.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_tsdf.py needs an MI355X: there is no CPU timing"
    import bench
    from splatco_amd import _C
    from splatco_amd.tsdf import TSDFVolume
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
    a8 = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
    b8 = torch.empty_like(a8)
    st = torch.cuda.current_stream().cuda_stream
    probe = lambda: _C.check(_C.lib.scr_copy_probe(a8.data_ptr(), b8.data_ptr(), a8.numel(), st))
    bench.settle_clocks(probe, 1, dev)
    pm = [timed(probe) for _ in range(9)]
    peak = 2 * a8.numel() / (med(pm) * 1e-3)
    del a8, b8
    lines = [f"TSDF fusion of {V} views of {W}x{H} maps (sphere over a plane, FoVx 60 degrees, trunc 4 h, min_alpha 0.5), HIP events, "
             f"median (min - max) of {args.rounds} rounds after a warm-up pass and settled clocks",
             f"copy probe 256 MiB: {fmt(pm)} -> {peak / 1e12:.2f} TB/s read + write (the copy peak below)"]
    lo_w, hi_w = [c - 1.0 for c in CENTRE], [c + 1.0 for c in CENTRE]
    for n in args.sizes:
        h = 2.0 / (n - 1)
        N = n ** 3
        for color in (True, False):
            planes = 5 if color else 2
            images = I if color else None
            vol = TSDFVolume(lo_w, h, (n, n, n), color=color, device=dev)
            tag = f"{n}^3 {'colour' if color else 'no colour'}"
            per_view = {}
            for batch in (16, 1):
                run = lambda: vol.integrate_views(D, A, cams, images, batch=batch)
                some = lambda: vol.integrate_views(D[:batch], A[:batch], cams[:batch], None if images is None else images[:batch], batch=batch)
                run()
                bench.settle_clocks(some, 1, dev)
                ms = [timed(run) for _ in range(args.rounds)]
                passes = (V + batch - 1) // batch
                moved = passes * 2 * planes * 4 * N + V * (2 + (3 if color else 0)) * 4 * H * W
                rate = moved / (med(ms) * 1e-3)
                lines.append(f"[{tag}] fused, {batch:2d} views per pass: {fmt(ms)} for {V} views = {med(ms) / V:8.4f} ms per view; "
                             f"{moved / 1e9:.2f} GB moved -> {rate / 1e12:.2f} TB/s = {100 * rate / peak:.0f} % of the copy peak")
                per_view[batch] = med(ms) / V
            # the float32 torch chain, one view at a time, into a fresh volume
            K = min(args.chain_views, V)
            ct, cw = torch.ones(n, n, n, device=dev), torch.zeros(n, n, n, device=dev)
            cc = torch.zeros(3, n, n, n, device=dev) if color else None
            lo32 = [float(torch.tensor(x, dtype=torch.float32)) for x in lo_w]
            h32 = float(torch.tensor(h, dtype=torch.float32))

            def chain():
                for i in range(K):
                    chain_integrate(ct, cw, cc, lo32, h32, vol.trunc, D[i], A[i], None if images is None else images[i], intr, cams[i][1])
            chain()
            ms = [timed(chain) for _ in range(max(3, args.rounds // 2))]
            lines.append(f"[{tag}] float32 torch chain, one view per call: {fmt(ms)} for {K} views = {med(ms) / K:8.4f} ms per view; "
                         f"chain / fused = {med(ms) / K / per_view[16]:.1f} (16 per pass), {med(ms) / K / per_view[1]:.1f} (1 per pass)")
            # agreement of the two on a fresh pair of volumes and the same K views (the chain rounds in float32)
            fresh = TSDFVolume(lo_w, h, (n, n, n), color=color, device=dev)
            fresh.integrate_views(D[:K], A[:K], cams[:K], None if images is None else images[:K])
            ct.fill_(1.0); cw.zero_()
            if cc is not None:
                cc.zero_()
            chain()
            same = fresh.weight == cw
            diff = (fresh.tsdf - ct)[same].abs()
            lines.append(f"[{tag}] chain against fused after {K} views: weights differ at {int((~same).sum())} of {N} nodes; where they "
                         f"agree |tsdf difference| > 1e-4 at {int((diff > 1e-4).sum())} nodes (max {float(diff.max()):.2e}; supposed: float32 u, v "
                         f"fall into the neighbouring pixel at a depth edge), max {float(diff[diff <= 1e-4].max()):.2e} at the others")
            del ct, cw, cc, fresh
            if color:
                ex = lambda: vol.extract()
                v, f, c = ex()
                ms = [timed(ex) for _ in range(args.rounds)]
                lines.append(f"[{tag}] extract: {fmt(ms)}; {v.shape[0]} vertices, {f.shape[0]} faces "
                             f"({(v.numel() + f.numel() + c.numel()) * 4 / 1e6:.1f} MB)")
                del v, f, c
            del vol
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    write_section(args.out, text)


if __name__ == "__main__":
    main()
