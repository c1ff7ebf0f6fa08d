"""csrc/mlp_heads.hip, csrc/attention.hip, csrc/expand.hip, csrc/ssim.hip, csrc/anchor_gather.hip and csrc/normlinear.hip
against float64, at the edges of their launch shapes.

Every case runs, on the same packed fp32 inputs (drawn on the CPU, tests/f64_refs.py):
  the kernel, through the product wrapper (mlp_heads.mlp_heads, plane_attention.attended_pair_planes,
  expand.expand_compact), twice -- the second run must give the same bits;
  the fp32 framework chain on the GPU (the reference's ops in float32);
  the float64 reference on the CPU (autograd for the gradients).
For every tensor e = max|got - ref| / max|ref|; for per-anchor / per-candidate / per-pixel tensors the same ratio per
row with the row's scale floored at 1e-3 of the tensor's (f64_refs.err).  The bar is max(floor, c * e_chain), e_chain
being the same figure of the fp32 chain against the same float64 result in the same process: floor 2e-5, c = 1.5 (the
constants of test_fused_norm_linear_matches_batchnorm_linear_chain).  Every figure is printed before anything is
asserted (and appended to the file $SPLATCO_F64_PARITY_LOG names, if set); profiles/r08_f64_parity.txt is one such run,
profiles/r13_loss_f64_parity.txt one of the image losses (l1_ssim, scaling_reg, pair_l1), profiles/r22_gather_f64_parity.txt
one of csrc/anchor_gather.hip at its C ABI (the end of this file) and of the heads and the expansion reading feat /
offsets in place from the gather's [V,72] matrix (layout `gather` of their tests), profiles/r23_norm_linear_f64_parity.txt one of
csrc/normlinear.hip at its C ABI (the last section: every element against an a-priori bound, no chain).
"""
import copy
import functools
import os

import pytest
import torch

import f64_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


class Report:
    """Collects (tensor, e, e_chain, bar) of one case; prints all of them, then asserts."""

    def __init__(self, op, case):
        self.op, self.case, self.lines, self.failed = op, case, [], []

    def add(self, name, got, chain, ref, rows=False, keep=None, floor=R.FLOOR, scale_floor=None, row_floor=None):
        e, e_chain = R.err(got, ref, rows, keep, scale_floor, row_floor), R.err(chain, ref, rows, keep, scale_floor, row_floor)
        b = R.bar(e_chain, floor)
        self.lines.append(f"{self.op:9s} {self.case:16s} {name:22s} e {e:9.3e}  e_chain {e_chain:9.3e}  bar {b:9.3e}"
                          f"{'' if e <= b else '   <-- FAIL'}")
        if not e <= b:
            self.failed.append((name, e, e_chain, b))

    def require(self, ok, what):
        self.lines.append(f"{self.op:9s} {self.case:16s} {what:22s} {'ok' if ok else 'FAIL'}")
        if not ok:
            self.failed.append((what,))

    def within(self, name, d, bound):
        """A figure with an a-priori bound (no chain to compare with)."""
        self.lines.append(f"{self.op:9s} {self.case:16s} {name:22s} e {d:9.3e}  bound {bound:9.3e}{'' if d <= bound else '   <-- FAIL'}")
        if not d <= bound:
            self.failed.append((name, d, bound))

    def finish(self):
        text = "\n".join(self.lines)
        print(text)
        log = os.environ.get("SPLATCO_F64_PARITY_LOG")
        if log:
            with open(log, "a") as f:
                f.write(text + "\n")
        assert not self.failed, self.failed


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------- heads
# Raised floor (every other tensor: 2e-5).  d anchor = (d ob - ob <ob, d ob>) / |o| takes the radial part out of d ob, a
# 96-term fp32 dot product: where d ob is nearly radial the row keeps the rounding of the whole and loses its size.  At
# V = 32769 the kernel's worst row holds 1/119 of |d ob| / |o| and is off by 3.42e-5 of itself = 2.9e-7 of |d ob| / |o|
# (two ulps); the chain is off by 7.9e-6 at that row and by 1.43e-5 at its own worst one, and by 2.18e-5 / 2.92e-5 at
# V = 49153 / 100003 where the kernel stays below 2e-5: rounding, which row it hits differs between the two.  Floor =
# that measured kernel error x 2 (profiles/r08_f64_parity.txt, "heads V=32769 d anchor" and the probe below the table).
HEADS_FLOOR = {"anchor": 6.9e-5}


def _in_gather_layout(t, col0):
    """t [V, w] as columns col0 .. col0 + w - 1 of a [V,72] leaf whose other columns are NaN: what csrc/anchor_gather.hip
    hands the readers of feat (col0 = 0) and offsets (col0 = 35, rows 140 bytes into 288: 4-byte aligned only).
    -> (the leaf, the view)"""
    g72 = torch.full((t.shape[0], 72), float("nan"), device=t.device)
    g72[:, col0:col0 + t.shape[1]] = t
    g72.requires_grad_()
    return g72, g72[:, col0:col0 + t.shape[1]]


def _gather_layout_grad(g72, col0, w):
    """(the gradient of the view, whether every other column of the leaf's gradient is exactly 0)"""
    rest = g72.grad.clone()
    rest[:, col0:col0 + w] = 0
    return g72.grad[:, col0:col0 + w], float(rest.abs().max()) == 0


HEADS_GATHER_V = [1, 17, 65, 1025, 16385]                    # V = 1: the wrapper copies (a row stride means nothing there)


@pytest.mark.parametrize("V,layout", [pytest.param(V, "packed", id=str(V)) for V in R.HEADS_V]
                         + [pytest.param(V, "gather", id=f"gather-{V}") for V in HEADS_GATHER_V])
def test_mlp_heads_against_float64(V, layout):
    """layout `gather`: feat is columns 0..31 of a [V,72] matrix (row stride 72, as the anchor gather leaves it), every
    other column NaN -- an over-read shows in the values; same references and bars.
    16-row tiles, 4 tiles per workgroup, backward grid capped at 256 workgroups, forward at 512: the row counts give
    4, 60, 64, 68, 128 and 1024 weight-gradient partials (the unrolled loop of mlp_heads_reduce_kernel alone, its tail
    alone, both), a last tile of 1, 15 and 16 rows alone and behind full workgroups, the first backward grid-stride
    (16385) and the first forward one (32769).  geo_fea arrives as one [V,64] matrix or as its two halves, alternating.
    The two largest sizes carry the edge rows of f64_refs.heads_inputs: a hidden unit that is exactly 0, second-layer
    pre-activations of +-40, +-100 (saturated tanh / sigmoid) and +-1e-4 (where 1 - 2 / (1 + e^2z) cancels)."""
    from splatco_amd.mlp_heads import mlp_heads, supported
    d = R.heads_inputs(V)
    rep = Report("heads", f"V={V}" + (" gather" if layout == "gather" else ""))
    two_parts = R.HEADS_V.index(V) % 2 == 1
    f64 = lambda t: t.double()
    ref_o, ref_g = R.heads_run(f64(d["feat"]), f64(d["anchor"]), f64(d["campos"]), f64(d["geo"]), [f64(u) for u in d["up"]],
                               R.weights_of(d["pc"], requires_grad=True))
    g = lambda t: t.to(DEV)
    feat, anchor, campos, geo, up = g(d["feat"]), g(d["anchor"]), g(d["campos"]), g(d["geo"]), [g(u) for u in d["up"]]
    ch_o, ch_g = R.heads_run(feat, anchor, campos, geo, up, R.weights_of(d["pc"], torch.float32, DEV, requires_grad=True))
    pc = copy.deepcopy(d["pc"]).to(DEV)
    runs = []
    for _ in range(2):
        f, a, ge = (t.clone().requires_grad_() for t in (feat, anchor, geo))
        if layout == "gather":
            g72, f = _in_gather_layout(feat, 0)
            assert f.stride() == (72, 1) and f.shape == feat.shape
        for p in pc.parameters():
            p.grad = None
        assert supported(pc, f, ge)
        if two_parts:
            outs = mlp_heads(pc, f, a, campos, ge[:, :32].contiguous(), ge[:, 32:].contiguous())
        else:
            outs = mlp_heads(pc, f, a, campos, ge)
        sum((o * u).sum() for o, u in zip(outs, up)).backward()
        grads = {"feat": f.grad, "anchor": a.grad, "geo": ge.grad}
        if layout == "gather":
            grads["feat"], clean = _gather_layout_grad(g72, 0, 32)
            rep.require(clean, "d g72: 0 elsewhere")
        grads.update({n: p.grad.clone() for n, p in pc.named_parameters() if n.startswith("mlp_")})
        runs.append(([o.detach() for o in outs], grads))
    (k_o, k_g), (k_o2, k_g2) = runs
    assert set(k_g) == set(ref_g) and len(k_g) == 15
    for name, a_, b_, c_ in zip(R.HEAD_NAMES, k_o, ch_o, ref_o):
        rep.add(name, a_, b_, c_, rows=True)
    for name in ref_g:
        rep.add("d " + name, k_g[name], ch_g[name], ref_g[name], rows=name in ("feat", "anchor", "geo"),
                floor=HEADS_FLOOR.get(name, R.FLOOR))
    rep.require(_same_bits(k_o, k_o2) and all(torch.equal(k_g[n], k_g2[n]) for n in k_g), "bit-reproducible")
    rep.require(all(bool(torch.isfinite(t).all()) for t in list(k_o) + list(k_g.values())), "finite")
    for row, (head, z) in d["edge_rows"].items():
        got = float(k_o[head][row, 0])
        if abs(z) < 1:                                         # +-1e-4: the right side of tanh(0) = 0 / sigmoid(0) = 0.5 (the value: rows above)
            ok = (got if head == 0 else got - 0.5) * z > 0
        elif head == 0:                                        # tanh(+-40), tanh(+-100) = +-1 in fp32, overflowing exp included
            ok = got == (1.0 if z > 0 else -1.0)
        else:                                                  # sigmoid(40) = 1; sigmoid(-40) = 4e-18; sigmoid(-100): exp overflows, 0
            ok = got == 1.0 if z > 0 else (0.0 <= got <= 1e-17 and (z > -100 or got == 0.0))
        rep.require(ok, f"edge row {row} z={z:g}")
    if d["edge_rows"]:
        unit = 64 + R.ZERO_UNIT                                # relu'(0) = 0: nothing flows through the zero unit
        rep.require(float(k_g["mlp_cov.0.weight"][R.ZERO_UNIT].abs().max()) == 0
                    and float(k_g["mlp_cov.0.bias"][R.ZERO_UNIT]) == 0 and unit == 69, "zero unit: no gradient")
    rep.finish()


# ---------------------------------------------------------------------------------------------------------- attention
def _pixels(t):
    """[1, C, H, W] -> [H*W, C]: one row per pixel."""
    return t[0].reshape(t.shape[1], -1).T


def _kernel_arg(planes):
    """The pool pass alone (scr_tpa_stats, as plane_attention._AttendedPairs.forward calls it): the pixel of every
    channel's maximum."""
    from splatco_amd import _C
    Rr, H, W = planes[0].shape[1:]
    scratch = torch.empty(_C.lib.scr_tpa_scratch_bytes(Rr, H, W), dtype=torch.uint8, device=DEV)
    avg, mx = torch.empty(3 * Rr, device=DEV), torch.empty(3 * Rr, device=DEV)
    arg = torch.empty(3 * Rr, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        _C.check(_C.lib.scr_tpa_stats(Rr, H, W, *(p.data_ptr() for p in planes), avg.data_ptr(), mx.data_ptr(),
                                      arg.data_ptr(), scratch.data_ptr(), _C.stream()))
    torch.cuda.synchronize()
    return arg.cpu(), mx.cpu()


@pytest.mark.parametrize("name,Rr,H,W,tie", R.ATTN_CASES, ids=[c[0] for c in R.ATTN_CASES])
def test_plane_attention_against_float64(name, Rr, H, W, tie):
    """R = 2..8 at 37 x 91 (every instantiation of tpa_bwd_apply_kernel the module can reach); R = 5 at planes smaller
    than the 3-pixel halo, thinner than it, exact multiples of the 16 x 64 tile and one off, with fewer pixels than the
    64 pooling blocks, and at the product's 700 x 700; three planes with a tied channel maximum (the whole plane; twice
    in different pooling blocks; twice in one block): kernel and reference send the pool's gradient to the first one.
    The gradient of a pixel whose two largest channels of y = ca * x are closer than 1e-5 max|y| (f64_refs.
    attention_undecided; at most 0.1 % of the pixels, tests/test_f64_refs_host.py) is left out of the per-pixel
    comparison of dx; the outputs are continuous there and stay in."""
    from splatco_amd import plane_attention
    d = R.attention_inputs(Rr, H, W, tie)
    rep = Report("attention", name)
    f64 = lambda ts: [t.double() for t in ts]
    ref_o, ref_y, ref_dx, ref_dw = R.attention_run(f64(d["planes"]), f64(d["up"]), R.attention_weights(d["ta"], requires_grad=True))
    keep = ~R.attention_undecided(ref_y).reshape(-1)
    planes, up = [p.to(DEV) for p in d["planes"]], [u.to(DEV) for u in d["up"]]
    ch_o, _, ch_dx, ch_dw = R.attention_run(planes, up, R.attention_weights(d["ta"], torch.float32, DEV, requires_grad=True))
    ta = copy.deepcopy(d["ta"]).to(DEV)
    arg, mx = _kernel_arg(planes)
    x = torch.cat(d["planes"], dim=1)[0].reshape(3 * Rr, -1)
    rep.require(torch.equal(arg, d["arg"]), "arg == first maximum")
    rep.require(torch.equal(mx, x.amax(dim=1)), "max exact")
    runs = []
    for _ in range(2):
        ps = [p.clone().requires_grad_(True) for p in planes]
        for p in ta.parameters():
            p.grad = None
        assert plane_attention.fused_ok(*ps, ta)
        out = plane_attention.attended_pair_planes(*ps, ta)
        sum((o * u).sum() for o, u in zip(out, up)).backward()
        runs.append(([o.detach() for o in out], [p.grad for p in ps],
                     [ta.ca.sharedMLP[0].weight.grad.clone(), ta.ca.sharedMLP[2].weight.grad.clone(), ta.sa.conv.weight.grad.clone()]))
    (k_o, k_dx, k_dw), (k_o2, k_dx2, k_dw2) = runs
    for j, pl in enumerate(("xy", "xz", "yz")):
        assert k_o[j].shape == ref_o[j].shape == (1, 2 * Rr, H, W)
        rep.add("pair " + pl, _pixels(k_o[j]), _pixels(ch_o[j]), _pixels(ref_o[j]), rows=True)
    for j, pl in enumerate(("xy", "xz", "yz")):
        rep.add("d " + pl, _pixels(k_dx[j]), _pixels(ch_dx[j]), _pixels(ref_dx[j]), rows=True, keep=keep)
    for n, a_, b_, c_ in zip(("d mlp.0", "d mlp.2", "d conv7x7"), k_dw, ch_dw, ref_dw):
        rep.add(n, a_, b_, c_)
    rep.lines.append(f"attention {name:16s} pixels left out of dx  {int((~keep).sum())} of {keep.numel()}")
    rep.require(_same_bits(k_o, k_o2) and _same_bits(k_dx, k_dx2) and _same_bits(k_dw, k_dw2), "bit-reproducible")
    rep.finish()


# ---------------------------------------------------------------------------------------------------------- expansion
EXPAND_GRADS = ("d neural_opacity", "d color", "d scale_rot", "d offsets", "d grid_scaling", "d anchor")
EXPAND_OUTS = ("xyz", "color", "opacity", "scaling", "rot")


@pytest.mark.parametrize("name,V,k,select,edges,layout", [pytest.param(*c, "packed", id=c[0]) for c in R.EXPAND_CASES]
                         + [pytest.param(*c, "gather", id="gather-" + c[0]) for c in R.EXPAND_CASES if c[2] == 10])
def test_expand_compact_against_float64(name, V, k, select, edges, layout):
    """layout `gather` (the k = 10 cases): the offsets are columns 35..64 of a [V,72] matrix whose other columns are NaN,
    rows 288 bytes apart and 140 bytes in; same references and bars.
    k = 1, 5, 10, 33 offsets per anchor; n = V k candidates on both sides of the first workgroup (1024) and of the
    1024 and 2048 workgroups after which compact_scan_kernel carries its running total into the next chunk; everything
    kept, nothing kept, every other candidate kept.  The k cases carry the edge rows of f64_refs.expand_inputs: zero
    and 1e-20 quaternions (the clamped branch of the normalisation, forward and backward), scale_rot[:, :3] = +-90
    (saturated sigmoid), neural_opacity +0.0, -0.0 and the smallest subnormal (the mask is `> 0`).  The mask is exact
    on identical inputs: indices and mask are compared with torch.nonzero for equality, nothing is left out."""
    from splatco_amd.expand import expand_compact
    from splatco_amd.losses import scaling_reg
    d = R.expand_inputs(V, k, select, edges)
    rep = Report("expand", name + (" gather" if layout == "gather" else ""))
    n = V * k
    want_mask = (d["args"][0] > 0).view(-1)
    want_idx = want_mask.nonzero().view(-1)
    P = int(want_mask.sum())
    rank = torch.cumsum(want_mask.long(), 0) - 1
    clamped = [int(rank[i]) for q, i in d["edge"].items() if q.startswith("quat_")]
    up = R.expand_upstream(P, clamped, n)
    args64, up64 = [t.double() for t in d["args"]], [u.double() for u in up]
    args, upd = [t.to(DEV) for t in d["args"]], [u.to(DEV) for u in up]
    for reg in (0.0, 700.0):
        tag = " +reg" if reg else ""
        ref_o, ref_m, ref_g = R.expand_run(args64, k, up64, reg)
        ch_o, ch_m, ch_g = R.expand_run(args, k, upd, reg)
        runs = []
        for _ in range(2):
            ins = [t.clone().requires_grad_(True) for t in args]
            if layout == "gather":
                g72, off = _in_gather_layout(args[3].reshape(V, 30), 35)
                ins[3] = off.unflatten(1, (10, 3))
                assert (V == 1 or ins[3].stride() == (72, 3, 1)) and ins[3].data_ptr() % 16 == 12      # (one row: no stride)
            *outs, mask = expand_compact(*ins, k)
            loss = sum((o * u).sum() for o, u in zip(outs, upd))
            if reg and P:
                loss = loss + reg * scaling_reg(outs[3])
            loss.backward()
            grads = [t.grad for t in ins]
            if layout == "gather":
                d_off, clean = _gather_layout_grad(g72, 35, 30)
                grads[3] = d_off.reshape(V, 10, 3)
                rep.require(clean, "d g72: 0 elsewhere" + tag)
            runs.append(([o.detach() for o in outs], mask, mask._scr_out_index, grads))
        (k_o, k_m, k_i, k_g), (k_o2, k_m2, k_i2, k_g2) = runs
        if not reg:
            rep.require(torch.equal(ref_m, want_mask) and torch.equal(ch_m.cpu(), want_mask), "reference masks")
            rep.require(k_m.dtype == torch.bool and torch.equal(k_m.nonzero().view(-1).cpu(), want_idx), "mask == nonzero")
            want_index = torch.where(want_mask, rank, torch.full_like(rank, -1)).to(torch.int32)
            rep.require(torch.equal(k_i.cpu(), want_index), "compaction index")
            rep.require(all(o.shape[0] == P for o in k_o), "P rows")
            rep.require(torch.equal(k_o[2].cpu().view(-1), d["args"][0].view(-1)[want_idx])
                        and torch.equal(k_o[1].cpu(), d["args"][1][want_idx]), "copies exact")
            for nm, a_, b_, c_ in zip(EXPAND_OUTS, k_o, ch_o, ref_o):
                rep.add(nm, a_, b_, c_, rows=True)
        for nm, a_, b_, c_ in zip(EXPAND_GRADS, k_g, ch_g, ref_g):
            rows = lambda t: t.reshape(n, -1) if nm != "d grid_scaling" and nm != "d anchor" else t
            rep.add(nm + tag, rows(a_), rows(b_), rows(c_), rows=True)
        rep.require(_same_bits(k_o, k_o2) and _same_bits(k_g, k_g2) and torch.equal(k_m, k_m2) and torch.equal(k_i, k_i2),
                    "bit-reproducible" + tag)
        rep.require(all(bool(torch.isfinite(t).all()) for t in k_o + k_g), "finite" + tag)
    rep.finish()


# ---------------------------------------------------------------------------------------------------------- image losses
def _l1_ssim_run(fn, x, y, up):
    """(L1, SSIM, dx) of fn(x, y) -> (L1, SSIM) with x a fresh leaf; only the outputs `up` weights are in the graph."""
    x = x.detach().clone().requires_grad_(True)
    l1, s = fn(x, y)
    R._ssim_loss(l1, s, up).backward()
    return l1.detach(), s.detach(), x.grad


@pytest.mark.parametrize("name", R.SSIM_IDS)
def test_l1_ssim_against_float64(name):
    """l1_ssim_forward / _reduce / _backward_kernel (16 x 16 tiles with a 5-pixel halo, 256 threads, the reduce workgroup
    striding by 1024 tiles).  Shapes: images thinner or smaller than the window and the halo, around the 11 taps, exact
    tiles and one off, a last tile that is exactly the halo and one more, C = 1, 2, 4 (the maps are indexed
    (m * C + c) * plane) and 1083 tiles.  Content at 3 x 33 x 37: the noise of test_fused_l1_ssim_matches_torch, y == x
    everywhere / on half the pixels (sign(0) = 0), flat and smooth images where s11 = E11 - mu1^2 cancels, zero images,
    a negative SSIM, values outside [0, 1], and two pixels whose gradient footprint crosses four tiles.  Upstream
    gradients of both signs and sizes, and graphs that use one output only.  A NaN or +Inf pixel: the values are
    non-finite as in float64 (NaN; L1 of inf_x is +Inf in float64 itself), dx is non-finite on float64's set of pixels
    and meets the bar elsewhere.  L1, SSIM, dx and dx per image row against max(2e-5, 1.5 e_chain); the scale of dx is
    floored at (|g_l1| + |g_ssim|) / n (f64_refs.ssim_dx_floor), on `identical` that of every row too
    (f64_refs.SSIM_ROW_FLOOR_CASES).  tests/test_f64_refs_host.py shows that correct fp32
    arithmetic meets these bars on every case and six wrong kernels do not."""
    from splatco_amd.losses import l1_loss, l1_ssim, ssim
    d = R.ssim_inputs(name)
    rep = Report("l1_ssim", name)
    up = d["up"]
    ref = R.ssim_f64(d["x"], d["y"], up)
    floor = R.ssim_dx_floor(up, d["x"].numel())
    finite = torch.isfinite(ref[2])
    x, y = d["x"].to(DEV), d["y"].to(DEV)
    chain = _l1_ssim_run(lambda a, b: (l1_loss(a, b), ssim(a, b)), x, y, up)
    k1, k2 = _l1_ssim_run(l1_ssim, x, y, up), _l1_ssim_run(l1_ssim, x, y, up)
    assert k1[2].shape == x.shape and k1[2].dtype == torch.float32 and k1[0].shape == k1[1].shape == ()
    zero = torch.zeros(())
    dxs = [torch.where(finite, R._f64(t[2]), zero) for t in (k1, chain, ref)]
    if d["nonfinite"]:
        same = lambda got, want: bool(torch.isnan(got)) if bool(torch.isnan(want)) else float(got) == float(want)
        rep.require(same(k1[0], ref[0]) and not bool(torch.isfinite(ref[0])), "L1 non-finite as f64")
        rep.require(bool(torch.isnan(k1[1])) and bool(torch.isnan(ref[1])), "SSIM is NaN")
        rep.require(torch.equal(torch.isfinite(k1[2]).cpu(), finite), "non-finite set of dx")
        rep.lines.append(f"l1_ssim   {name:16s} non-finite elements of dx  {int((~finite).sum())} of {finite.numel()}")
    else:
        rep.add("L1", k1[0], chain[0], ref[0])
        rep.add("SSIM", k1[1], chain[1], ref[1])
        rep.require(all(bool(torch.isfinite(t).all()) for t in k1) and bool(finite.all()), "finite")
    W = x.shape[-1]
    rep.add("dx", *dxs, scale_floor=floor)
    rep.add("dx rows", *(t.reshape(-1, W) for t in dxs), rows=True, scale_floor=floor,
            row_floor=R.ssim_row_floor(name, up, d["x"].numel()))
    rep.require(all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(k1, k2)), "bit-reproducible")
    if name == "identical":
        rep.require(float(k1[0]) == 0.0, "L1 == 0")
        rep.within("|SSIM - 1|", abs(float(k1[1].double()) - 1.0), 2.0 ** -22)
    rep.finish()


def test_l1_ssim_entry_points():
    """The ways into the forward kernel other than a packed fp32 leaf, on 3 x 33 x 37 noise: without the derivative maps
    (with_grad = 0: under no_grad, metrics.ssim_value, multiview.pair_similarity) the SSIM has the bits of the
    differentiable run; a non-contiguous crop of a leaf and float64 / float16 leaves are converted inside the autograd
    function and get the gradient of the packed fp32 run, in their own layout and dtype; a backward after a forward
    that did not write the maps raises."""
    from splatco_amd.losses import _L1Ssim, l1_ssim
    from splatco_amd.metrics import ssim_value
    from splatco_amd.multiview import pair_similarity
    d = R.ssim_inputs("noise")
    x, y, up = d["x"].to(DEV), d["y"].to(DEV), d["up"]
    l1, s, dx = _l1_ssim_run(l1_ssim, x, y, up)
    bits = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    with torch.no_grad():
        l1n, sn = l1_ssim(x, y)
    assert bits(sn, s) and bits(l1n, l1)
    assert bits(ssim_value(x, y), s) and bits(pair_similarity(x, y), s)
    big = torch.full((3, 40, 48), 7.0, device=DEV)
    big[:, 3:36, 5:42] = x
    big.requires_grad_(True)
    crop = big[:, 3:36, 5:42]
    assert not crop.is_contiguous() and crop.shape == x.shape
    l1c, sc = l1_ssim(crop, y)
    R._ssim_loss(l1c, sc, up).backward()
    assert bits(l1c.detach(), l1) and bits(sc.detach(), s) and bits(big.grad[:, 3:36, 5:42].contiguous(), dx)
    outside = big.grad.clone()
    outside[:, 3:36, 5:42] = 0
    assert float(big.grad.abs().sum()) > 0 and float(outside.abs().max()) == 0
    for dtype in (torch.float64, torch.float16):
        leaf = x.to(dtype).requires_grad_(True)
        lo, so = l1_ssim(leaf, y)
        R._ssim_loss(lo, so, up).backward()
        l1f, sf, dxf = _l1_ssim_run(l1_ssim, leaf.detach().float(), y, up)
        assert lo.dtype == so.dtype == torch.float32 and bits(lo.detach(), l1f) and bits(so.detach(), sf)
        assert leaf.grad.dtype == dtype and torch.equal(leaf.grad, dxf.to(dtype))
        if dtype == torch.float64:
            assert bits(so.detach(), s)
    gt = y.clone().requires_grad_(True)                              # the graph reaches the op through y only: no maps
    l1y, _ = _L1Ssim.apply(x, gt)
    with pytest.raises(RuntimeError, match="without the derivative maps"):
        l1y.backward()


@pytest.mark.parametrize("shape", R.L1_ORDER_SHAPES, ids=["%dx%dx%d" % s for s in R.L1_ORDER_SHAPES])
def test_l1_has_the_documented_summation_order(shape):
    """The L1 of l1_ssim equals f64_refs.l1_tile_order bit for bit: the order of csrc/wg.h (butterfly per wave, waves
    ascending) and of l1_ssim_reduce_kernel, on one live pixel, one tile, ragged tiles, 45 tiles and 1083 tiles.  The
    inputs' seeds are those on which a pairwise wave combine and a serial sum end in other bits
    (tests/test_f64_refs_host.py checks that they do), so a changed order fails here, not only a wrong sum."""
    import numpy as np
    from splatco_amd.losses import l1_ssim
    x, y = R.l1_order_inputs(shape)
    want = R.l1_tile_order(x, y)
    with torch.no_grad():
        got = l1_ssim(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))[0].cpu().numpy()
    print(f"l1 order {shape}: kernel {float(got):.9g} ({int(got.view(np.uint32)):#010x}), emulator {float(want):.9g} "
          f"({int(want.view(np.uint32)):#010x})")
    assert got.dtype == np.float32 and got.shape == () and got.view(np.uint32) == want.view(np.uint32)


def test_l1_ssim_wrapper_refuses_a_mismatched_ground_truth(monkeypatch):
    """losses.l1_ssim hands the kernel gt_image as a bare pointer with image's extents.  A gt_image of another shape or
    on another device is a ValueError naming both, and one that requires grad goes to the framework chain and gets its
    gradient -- all before any launch: the forward entry is replaced by one that fails the test."""
    from splatco_amd import _C
    from splatco_amd.losses import l1_loss, l1_ssim, ssim
    d = R.ssim_inputs("noise")
    x, y = d["x"].to(DEV), d["y"].to(DEV)
    launched = []
    monkeypatch.setattr(_C.lib, "scr_l1_ssim_forward", lambda *a: launched.append(a) or pytest.fail("the kernel was launched"))
    cases = {"another H": y[:, :-1], "another C": y[:2], "on the CPU": d["y"]}
    if torch.cuda.device_count() > 1:
        cases["on another GPU"] = d["y"].to("cuda:1")
    for what, gt in cases.items():
        for image in (x, x.clone().requires_grad_(True)):
            with pytest.raises(ValueError) as e:
                l1_ssim(image, gt)
            msg = str(e.value)
            assert str(tuple(x.shape)) in msg and str(tuple(gt.shape)) in msg and str(x.device) in msg and str(gt.device) in msg, (what, msg)
    a, gt = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    l1, s = l1_ssim(a, gt)
    (0.8 * l1 + 0.2 * (1.0 - s)).backward()
    a2, gt2 = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    (0.8 * l1_loss(a2, gt2) + 0.2 * (1.0 - ssim(a2, gt2))).backward()
    assert gt.grad is not None and float(gt.grad.abs().max()) > 0
    assert torch.equal(gt.grad, gt2.grad) and torch.equal(a.grad, a2.grad)
    assert not launched


@pytest.mark.parametrize("P", R.SREG_P)
def test_scaling_reg_against_float64(P):
    """scaling_reg_partial / _finish / _backward_kernel (2048 rows per workgroup, 256 threads, the finish workgroup
    striding by 1024 partials): one row, around a wave-set of 256 and a workgroup of 2048 rows, and 1024 / 1025
    partials.  The first rows hold one, two and three zeros (where torch.prod's backward takes its own path), a
    negative entry and (1e-20, 1e-20, 1) (a subnormal product).
    Value: within 2^-23 of the float64 mean of the binary32 products (the order the kernel documents) + 1e-12.
    Gradient: d s[r,0] = w (b c) with w = fl(g fl(1/P)), four roundings -- 1/P, g/P, b c, their product -- each 2^-24:
    (1 + 2^-24)^4 - 1 < 4.5 * 2^-24 of float64 autograd of prod(dim=1).mean(), + 2^-126 where the result is subnormal;
    the rows with a zero get exactly the product of the other two entries times w."""
    from splatco_amd.losses import scaling_reg
    s = R.sreg_inputs(P)
    rep = Report("sreg", f"P={P}")
    g = float(torch.tensor(0.37, dtype=torch.float32))               # the upstream gradient as the kernel sees it
    exact = float(((s[:, 0] * s[:, 1]) * s[:, 2]).double().mean())
    s64 = s.double().requires_grad_(True)
    (g * s64.prod(dim=1).mean()).backward()
    runs = []
    for _ in range(2):
        a = s.to(DEV).clone().requires_grad_(True)
        v = scaling_reg(a)
        (v * 0.37).backward()
        runs.append((v.detach().cpu(), a.grad.cpu()))
    (v, ds), (v2, ds2) = runs
    assert v.dtype == torch.float32 and ds.dtype == torch.float32 and ds.shape == (P, 3)
    rep.within("value", abs(float(v.double()) - exact), 2.0 ** -23 * abs(exact) + 1e-12)
    over = ((ds.double() - s64.grad).abs() - (4.5 * 2.0 ** -24 * s64.grad.abs() + 2.0 ** -126)).max()
    rep.within("d scaling (excess)", float(over), 0.0)
    k = min(P, R.SREG_ZERO_ROWS)
    w = torch.tensor(0.37, dtype=torch.float32) * torch.tensor(1.0 / P, dtype=torch.float64).float()
    z = s[:k]
    want = torch.stack([w * (z[:, 1] * z[:, 2]), w * (z[:, 0] * z[:, 2]), w * (z[:, 0] * z[:, 1])], dim=1)
    rep.require(torch.equal(ds[:k], want) and int((want != 0).sum()) == 1, "zero rows exact")
    rep.require(bool(torch.isfinite(v)) and bool(torch.isfinite(ds).all()), "finite")
    rep.require(torch.equal(v, v2) and torch.equal(ds, ds2), "bit-reproducible")
    rep.finish()


@pytest.mark.parametrize("n", R.PAIR_N)
def test_pair_l1_at_workgroup_edges(n):
    """pair_l1_partial / _backward_kernel and the finish kernel it shares with scaling_reg: one element, around the 4096
    elements of a workgroup, and 1024 / 1025 partials.  The assertions of test_fused_pair_l1_matches_the_reference_ops:
    the value within 2^-23 of the double mean of the binary32 residuals and no further from it than the framework's,
    the gradients with the framework's signs (sign(0) = 0; every 53rd residual is at or next to zero) and within 2^-22."""
    from splatco_amd.losses import l1_loss, pair_l1
    a0, b0, r1, r2 = R.pair_inputs(n)
    rep = Report("pair_l1", f"n={n}")
    exact = float(((r1 - r2) - (a0 - b0)).abs().double().mean())
    a0, b0, r1, r2 = (t.to(DEV) for t in (a0, b0, r1, r2))
    for need in ((True, True), (True, False), (False, True)):
        tag = " d" + "".join(str(i + 1) for i in range(2) if need[i])
        outs = []
        for fused in (True, True, False):
            a, b = a0.clone().requires_grad_(need[0]), b0.clone().requires_grad_(need[1])
            loss = pair_l1(a, b, r1, r2) if fused else l1_loss(r1 - r2, a - b)
            (loss * 0.37).backward()
            outs.append((loss.detach(), a.grad, b.grad))
        (lf, af, bf), (lf2, af2, bf2), (lt, at, bt) = outs
        e, e_t = abs(float(lf.double()) - exact), abs(float(lt.double()) - exact)
        rep.within("value" + tag, e, 2.0 ** -23 * exact + 1e-12)
        rep.within("value vs torch's" + tag, e, e_t + 2.0 ** -24 * exact + 1e-12)
        ok = lf.dtype == torch.float32 and torch.equal(lf, lf2)
        for got, got2, want, needed in ((af, af2, at, need[0]), (bf, bf2, bt, need[1])):
            ok = ok and (got is None) == (not needed) and (want is None) == (not needed)
            if needed:
                ok = ok and torch.equal(got, got2)
                rep.require(torch.equal(got.sign(), want.sign()) and torch.allclose(got, want, rtol=2.0 ** -22, atol=0),
                            "gradient" + tag + (" (gen1)" if got is af else " (gen2)"))
        rep.require(bool(ok), "bit-reproducible" + tag)
    rep.finish()


# ---------------------------------------------------------------------------------------------------------- anchor gather
# csrc/anchor_gather.hip at its own C ABI (include/splatco_raster.h: scr_anchor_gather, scr_anchor_gather_backward), on the
# cases of f64_refs.GATHER_CASES: what each block of every case makes the kernel do is asserted from the index alone in
# tests/test_f64_refs_host.py, which also shows that plain fp32 arithmetic meets every bound used here and three wrong
# kernels do not.  profiles/r22_gather_f64_parity.txt is one run of this section.
AG_WIDTHS = (32, 3, 30, 6)
AG_ALL = frozenset(R.GATHER_UP)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


@functools.lru_cache(maxsize=None)
def _gather_case(case):
    """(the CPU inputs, their device copies with the fp32 framework chain's grid_scaling `gs` and g_fea `x`, the float64
    forward): made once per case, shared by the tests below and never modified."""
    d = R.gather_inputs(case)
    g = lambda t: t.to(DEV)
    dev = dict(idx=g(d["idx"]), inv=g(d["inv"]), params=[g(p) for p in d["params"]], up={n: g(t) for n, t in d["up"].items()},
               coef=g(d["coef"]), dy=g(d["dy"]), old=[g(t) for t in d["old"]])
    dev["up71"] = dev["up"]["g_fea"][:, :71].contiguous()
    chain = R.gather_f64(dev["idx"], *dev["params"])
    dev["gs"], dev["x"] = chain[3].contiguous(), chain[4].contiguous()
    return d, dev, R.gather_f64(d["idx"], *(p.double() for p in d["params"]))


@functools.lru_cache(maxsize=None)
def _gather_bwd_ref(case, names, dx=False, old=False):
    """(float64 gradients [N, width] x 4, the sums of |terms| their bounds are multiples of): once per set of operands."""
    d, dev, _ = _gather_case(case)
    f = lambda t: None if t is None else t.double()
    up = {n: (d["up"][n] if n in names else None) for n in R.GATHER_UP}
    dx3 = (d["coef"], d["dy"], dev["x"].cpu()) if dx else None
    dx64 = R.gather_dx_f64(*(f(t) for t in dx3)) if dx else None
    _, ref = R.gather_run(d["idx"], [f(p) for p in d["params"]], {n: f(t) for n, t in up.items()}, dx64)
    ref = [r.reshape(d["N"], -1) for r in ref]
    if old:
        ref = [r + f(o) for r, o in zip(ref, d["old"])]
    return ref, R.gather_terms(d, up, dx3, d["old"] if old else None)


def _gather_backward(case, names, ldg, dxa=None, old=False, ranges=None, gs=True):
    """scr_anchor_gather_backward into NaN-filled (old: copies of the case's old) buffers, one call per anchor range on
    offset addresses as anchor_gather._AnchorGather.backward makes them.  names: the upstream gradients that are given."""
    from splatco_amd import _C
    d, dev, _ = _gather_case(case)
    N, V = d["N"], d["V"]
    outs = [o.clone() for o in dev["old"]] if old else [_nan(N, w) for w in AG_WIDTHS]
    u = lambda n: _C.ptr(dev["up"][n]) if n in names else None
    gf = _C.ptr(dev["up"]["g_fea"] if ldg == 72 else dev["up71"]) if "g_fea" in names else None
    nl = dxa if dxa is not None else (None, None, 0, None, 0)
    for n0, n1 in ranges or [(0, N)]:
        _C.call("scr_anchor_gather_backward", n1 - n0, V, dev["inv"].data_ptr() + 8 * n0, _C.ptr(dev["gs"]) if gs else None,
                u("feat"), u("anchor"), u("offsets"), u("scaling"), gf, ldg,
                *(o.data_ptr() + 4 * w * n0 for o, w in zip(outs, AG_WIDTHS)), 1 if old else 0, *nl, device=DEV)
    return outs


def _gather_ranges(N):
    """64-aligned ranges of [0, N): the first block, the full blocks behind it, the last (shorter) block."""
    cuts = sorted({0, min(64, N), N // 64 * 64, N})
    return [(a, b) for a, b in zip(cuts, cuts[1:]) if b > a]


@pytest.mark.parametrize("ld,split", [(71, True), (72, True), (72, False)], ids=["ld71", "ld72", "ld72-inplace"])
@pytest.mark.parametrize("case", R.GATHER_CASES)
def test_anchor_gather_forward_against_float64(case, ld, split):
    """scr_anchor_gather with packed (71) and padded (72) g_fea rows, with feat / offsets written or left to their readers
    (NULL, 72 only), into NaN-filled buffers: the copied columns and the split outputs are the inputs' rows bit for bit, the
    pad column is 0, exp(scaling) is within max(2^-23, 1.5 e_chain) of float64 (relative, per element; e_chain: fp32
    torch.exp on the device), the per-workgroup column sums of (x - x[0]) and (x - x[0])^2 add up to the float64 sums over
    the same fp32 matrix within 512 x 2^-24 of sum |x - x[0]| / sum (x - x[0])^2 (an fp32 sum of at most 512 terms per
    partial, any order), their columns 71.. are 0, and everything the call owns is NaN-free.  V = 511, 512, 513, 1025: one
    workgroup owns 8 x 64 rows and one statistics row."""
    from splatco_amd import _C
    d, dev, ref = _gather_case(case)
    rep = Report("gather fw", f"{case} ld{ld}" + ("" if split else " in place"))
    V = d["V"]
    rows = _C.lib.scr_anchor_gather_stat_rows(V)
    rep.require(rows == R.gather_stat_rows(V) == R.GATHER_STAT_ROWS.get(case, 1), f"{rows} stat rows")
    runs = []
    for _ in range(2):
        g, anc, gs = _nan(V, ld), _nan(V, 3), _nan(V, 6)
        feat, off = (_nan(V, 32), _nan(V, 30)) if split else (None, None)
        st = _nan(_C.lib.scr_anchor_gather_stat_buffer_rows(V), 2, 80)
        _C.call("scr_anchor_gather", V, _C.ptr(dev["idx"]), *dev["params"], _C.ptr(feat), anc, _C.ptr(off), gs, g, ld, st, device=DEV)
        runs.append([t.cpu() for t in (g, anc, gs, st[:rows]) + ((feat, off) if split else ())])
    g, anc, gs, st = runs[0][:4]
    if V:
        want = [p[d["idx"]].reshape(V, -1) for p in d["params"][:3]]
        rep.require(torch.equal(g[:, :32], want[0]) and torch.equal(g[:, 32:35], want[1]) and torch.equal(g[:, 35:65], want[2]),
                    "g_fea copies exact")
        rep.require(torch.equal(anc, want[1]) and torch.equal(gs, g[:, 65:71]), "anchor, scaling exact")
        if split:
            rep.require(torch.equal(runs[0][4], want[0]) and torch.equal(runs[0][5], want[2]), "feat, offsets exact")
        if ld == 72:
            rep.require(bool((g[:, 71] == 0).all()), "pad column == 0")
        rep.require(all(bool(torch.isfinite(t).all()) for t in runs[0]), "NaN-free")
        rel = lambda t: float(((t.double() - ref[3]).abs() / ref[3]).max())
        e, e_chain = rel(gs), rel(dev["gs"].cpu())
        rep.lines.append(f"gather fw {rep.case:16s} exp: e_chain {e_chain:9.3e}")
        rep.within("exp(scaling)", e, max(R.GATHER_EXP_FLOOR, 1.5 * e_chain))
        excess, zeros = R.gather_stats_excess(st, g)
        rep.within("column sums / bound", excess, 1.0)
        rep.require(zeros, "stat columns 71.. == 0")
        if V == 1:
            rep.require(bool((st == 0).all()), "V = 1: sums exactly 0")
    rep.require(all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*runs)), "bit-reproducible")
    rep.finish()


def _gather_check(rep, tag, case, got, names, tol, dx=False, old=False):
    d = _gather_case(case)[0]
    ref, terms = _gather_bwd_ref(case, frozenset(names), dx, old)
    rep.within(tag, R.gather_excess(got, ref, terms, tol), 1.0)
    hidden = ~d["mask"]
    want = d["old"] if old else [torch.zeros(d["N"], w) for w in AG_WIDTHS]
    rep.require(all(torch.equal(a.cpu()[hidden], b[hidden]) for a, b in zip(got, want)),
                tag + (": hidden == old" if old else ": hidden == 0"))


@pytest.mark.parametrize("ldg", [71, 72], ids=["ld71", "ld72"])
@pytest.mark.parametrize("case", R.GATHER_BWD_CASES)
def test_anchor_gather_backward_against_float64(case, ldg):
    """scr_anchor_gather_backward without dx, d g_fea packed (71) and padded (72, the pad column random: ignored).  Per
    element |got - ref| <= 4 x 2^-24 x ((|d part| + |d g_fea|) exp(s) + |old|) -- at most three additions and one multiply;
    the factor exp(s) is 1 outside d scaling, and |old| (accumulate only) is added behind the multiplication, so it does
    not carry that factor (with |old| exp(s) in its place plain fp32 arithmetic itself stands at 5.7 x / 6.8 x the bound on
    `mixed` / `tail_edge`: exp(s) = 0.05 and the last addition rounds to 2^-24 |old + new|; tests/test_f64_refs_host.py
    has it at 0.43 of this one) -- against float64 autograd of the torch chain; invisible anchors exactly 0 (accumulate:
    exactly the old value); a second run gives the same bits.  On `mixed` and `tail_edge` also: each upstream pointer NULL
    on its own; all five and grid_scaling NULL (all zeros); accumulate = 1 over a random old buffer; the call split into
    64-aligned ranges with a last range shorter than 64 and V larger than every range (the whole call's bits)."""
    d = _gather_case(case)[0]
    rep = Report("gather bw", f"{case} ld{ldg}")
    got, got2 = _gather_backward(case, AG_ALL, ldg), _gather_backward(case, AG_ALL, ldg)
    _gather_check(rep, "all upstreams", case, got, AG_ALL, R.GATHER_BWD_TOL)
    rep.require(_same_bits(got, got2), "bit-reproducible")
    if d["V"] == 0:                                            # upstream pointers NULL (nothing to point at), no grid_scaling
        rep.require(all(float(t.abs().max()) == 0 for t in _gather_backward(case, (), ldg, gs=False)), "V = 0: all zeros")
    if case in R.GATHER_SUB_CASES:
        for n in R.GATHER_UP:
            _gather_check(rep, "no d " + n, case, _gather_backward(case, AG_ALL - {n}, ldg), AG_ALL - {n}, R.GATHER_BWD_TOL)
        rep.require(all(float(t.abs().max()) == 0 for t in _gather_backward(case, (), ldg, gs=False)), "no upstream: zeros")
        _gather_check(rep, "accumulate", case, _gather_backward(case, AG_ALL, ldg, old=True), AG_ALL, R.GATHER_BWD_TOL, old=True)
        ranges = _gather_ranges(d["N"])
        assert len(ranges) == 3 and ranges[-1][1] - ranges[-1][0] < 64 and all(b - a < d["V"] for a, b in ranges[::2])
        rep.require(_same_bits(_gather_backward(case, AG_ALL, ldg, ranges=ranges), got), "ranges: the call's bits")
    rep.finish()


@pytest.mark.parametrize("off", [0, 1], ids=["x0", "x1"])
@pytest.mark.parametrize("ldx", [71, 72, 76], ids=["ldx71", "ldx72", "ldx76"])
@pytest.mark.parametrize("case", R.GATHER_DX_CASES)
def test_anchor_gather_backward_with_fused_dx_against_float64(case, ldx, off):
    """scr_anchor_gather_backward forming d g_fea = k0 + x k1 + dy Gi itself (nl_coef given): x with packed rows (71), padded
    rows (72) and a wider matrix (76), at a 16-byte aligned address and one float behind it (x0 / x1) -- the row pointers are
    then 16-byte aligned on every row, every fourth row, or never; dy with row strides 32 and 36; d g_fea absent or given
    (added on top).  The unused floats of x and dy are NaN.  Reference: float64 autograd of the torch chain fed d g_fea +
    gather_dx_f64.  Per element |got - ref| <= 40 x 2^-24 x S exp(s), S the sum of the absolute values of all terms (32
    products, x k1, k0, the other upstream parts): HEADS_TOL's rule for an fp32 MFMA dot product.  The call split into
    64-aligned ranges gives the whole call's bits, a second run too."""
    d, dev, _ = _gather_case(case)
    rep = Report("gather dx", f"{case} ldx{ldx}+{off}")
    V = d["V"]
    xb = _nan(off + V * ldx + 3)
    xb[off:off + V * ldx].view(V, ldx)[:, :71] = dev["x"]
    assert xb.data_ptr() % 16 == 0
    for with_gf in (False, True):
        for lddy in (32, 36):
            dyb = _nan(V, lddy)
            dyb[:, :32] = dev["dy"]
            dxa = (dev["coef"], dyb, lddy, xb.data_ptr() + 4 * off, ldx)
            names, ldg = (AG_ALL if with_gf else AG_ALL - {"g_fea"}), (72 if lddy == 32 else 71)
            tag = f"{'d g_fea ' if with_gf else ''}lddy {lddy}"
            got = _gather_backward(case, names, ldg, dxa)
            _gather_check(rep, tag, case, got, names, R.GATHER_DX_TOL, dx=True)
            rep.require(_same_bits(_gather_backward(case, names, ldg, dxa), got), tag + ": bit-reproducible")
            rep.require(_same_bits(_gather_backward(case, names, ldg, dxa, ranges=_gather_ranges(d["N"])), got),
                        tag + ": ranges: the call's bits")
    rep.finish()


@pytest.mark.parametrize("N", R.GATHER_WRAPPER_N)
def test_gather_wrappers_against_float64(N, monkeypatch):
    """The product path: anchor_gather.gather_anchors -> scene_model._NormLinearFn with the deferred-dx box -> a weighted
    sum of y and the four split outputs.  The gradients of the four parameters, of G and of c against float64 autograd of
    the torch chain (f64_refs.gather_norm_linear_run), bar max(2e-5, 1.5 e_chain) with e_chain from the same chain in
    fp32 on the device.  The backward call is watched: dx is formed inside the gather's kernel, no d g_fea arrives."""
    from splatco_amd import _C
    from splatco_amd import anchor_gather as ag
    from splatco_amd import scene_model as sm
    w = R.gather_wrapper_inputs(N)
    rep = Report("gather wr", f"N={N}")
    f, g = (lambda t: t.double()), (lambda t: t.to(DEV))
    ref = R.gather_norm_linear_run(w["idx"], [f(p) for p in w["params"]], f(w["G"]), f(w["c"]), [f(u) for u in w["w"]])
    chain = R.gather_norm_linear_run(g(w["idx"]), [g(p) for p in w["params"]], g(w["G"]), g(w["c"]), [g(u) for u in w["w"]])
    calls, call = [], _C.call
    monkeypatch.setattr(_C, "call", lambda name, *a, **k: (calls.append((name, a)), call(name, *a, **k))[1])
    runs = []
    for _ in range(2):
        pc = sm.AnchorGaussianModel(plane_size=16, num_channels=15).to(DEV)
        p_feat, p_anchor, p_offset, p_scaling = (g(p).clone() for p in w["params"])
        pc.set_anchors(p_anchor, p_offset, p_feat, p_scaling)
        G, c = g(w["G"]).clone().requires_grad_(), g(w["c"]).clone().requires_grad_()
        feat, anc, off, gs, g_fea = ag.gather_anchors(pc, g(w["idx"]))
        assert feat.stride() == (72, 1) and off.stride() == (72, 3, 1) and g_fea.stride() == (72, 1)
        y, _, _ = sm._NormLinearFn.apply(g_fea, G, c, 1e-5, g_fea._scr_col_stats, g_fea._scr_deferred_dx)
        sum((o * u).sum() for o, u in zip((y, feat, anc, off, gs), (g(u) for u in w["w"]))).backward()
        runs.append([t.grad.clone() for t in (pc._anchor_feat, pc._anchor, pc._offset, pc._scaling, G, c)])
    bw = [a for name, a in calls if name == "scr_anchor_gather_backward"]
    rep.require(len(bw) == 2 and all(a[15] is not None and a[8] is None and a[19] == 72 for a in bw), "dx formed in the gather")
    for name, a_, b_, c_ in zip(("d anchor_feat", "d anchor", "d offset", "d scaling", "d G", "d c"), runs[0], chain, ref):
        rep.add(name, a_, b_, c_, rows=not name.endswith((" G", " c")))
    rep.require(_same_bits(*runs), "bit-reproducible")
    rep.finish()


# ---------------------------------------------------------------------------------------------------------- norm-linear
# csrc/normlinear.hip at its own C ABI (include/splatco_raster.h: scr_norm_linear_forward / _backward / _dx, scr_norm_fold*),
# on the shapes of f64_refs.NL_*: what each reaches (template instantiation, loop form, slabs, partials, grid rounds) is
# asserted from the shapes alone in tests/test_f64_refs_host.py, which also shows that plain fp32 arithmetic meets every
# bound used here and six wrong kernels do not.  (The statistics are held to 2 fp32 roundings per slab sum: the kernel's
# lanes sum in fp64.  The host restatement meets that bound with its slab sums formed in float64 and rounded once, and on the
# col_stats cases; with fp32 slab sums it is held to the 516- / 1026-term bound of such a lane instead.)  Every figure is |got - ref| / bound, the bound a-priori and per element
# (f64_refs.nl_*_bounds): at most 1.  profiles/r23_norm_linear_f64_parity.txt is one run of this section.
NL_SENTINEL = 0x7FC12345                                    # a quiet NaN with a payload: shows in a value, and its bits are checked


def _sent(*shape):
    return torch.full(shape, NL_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _kept(t, used=None):
    """Whether every element of t outside the boolean mask `used` (None: all of t) still holds the sentinel's bits."""
    bits = t.view(torch.int32)
    return bool((bits == NL_SENTINEL).all()) if used is None else bool((bits[~used] == NL_SENTINEL).all())


def _nl_forward(xv, ld, G, c, eps, stats=None):
    """scr_norm_linear_forward into sentinel-filled buffers: y [V + 1, 32] (one row to spare), mean / var / inv [80]."""
    from splatco_amd import _C
    V, d = xv.shape
    y, mean, var, inv = _sent(V + 1, 32), _sent(R.NL_DP), _sent(R.NL_DP), _sent(R.NL_DP)
    scratch = _C.scratch(_C.lib.scr_norm_linear_scratch_bytes(V), DEV)
    _C.call("scr_norm_linear_forward", V, d, xv.data_ptr(), ld, G, c, float(eps), y, mean, var, inv, scratch,
            stats, 0 if stats is None else stats.shape[0], device=DEV)
    return y, mean, var, inv


def _nl_backward(xv, ld, dyv, lddy, G, mean, inv, lddx, with_dx, with_coef):
    """scr_norm_linear_backward into sentinel-filled buffers: dx [V + 1, lddx] or NULL, dG [32 d + 4], dc [36], coef_out
    [34 x 80 + 4] or NULL."""
    from splatco_amd import _C
    V, d = xv.shape
    dx = _sent(V + 1, lddx) if with_dx else None
    dG, dc = _sent(32 * d + 4), _sent(36)
    coef = _sent(34 * R.NL_DP + 4) if with_coef else None
    scratch = _C.scratch(_C.lib.scr_norm_linear_scratch_bytes(V), DEV)
    _C.call("scr_norm_linear_backward", V, d, xv.data_ptr(), ld, dyv.data_ptr(), lddy, G, mean, inv, _C.ptr(dx), lddx, dG, dc,
            scratch, _C.ptr(coef), device=DEV)
    return dx, dG, dc, coef


def _nl_dx(xv, ld, dyv, lddy, coef, lddx):
    from splatco_amd import _C
    V, d = xv.shape
    dx = _sent(V + 1, lddx)
    _C.call("scr_norm_linear_dx", V, d, xv.data_ptr(), ld, dyv.data_ptr(), lddy, coef, dx, lddx, device=DEV)
    return dx


def _dx_kept(dx, V, d):
    used = torch.zeros(dx.shape, dtype=torch.bool, device=dx.device)
    used[:V, :d] = True
    return _kept(dx, used)


def _nl_drive(rep, inp, xlayout="packed", eps=1e-5, lddy=32, lddx=None, stats=None, backward=True, rows=()):
    """One case through forward, backward with dx (+ coef_out), backward with dx = NULL + coef_out, scr_norm_linear_dx on that
    block -- each call twice.  Adds every figure to rep; -> the forward's (y, mean, var, inv) on the CPU."""
    V, d = inp["V"], inp["d"]
    x, G, c = inp["x"], inp["G"].to(DEV), inp["c"].to(DEV)
    _leaf, xv, ld, _off = R.nl_layout(x.to(DEV), xlayout)
    fw = [_nl_forward(xv, ld, G, c, eps, stats) for _ in range(2)]
    y, mean, var, inv = fw[0]
    rep.require(_same_bits([t.view(torch.int32) for t in fw[0]], [t.view(torch.int32) for t in fw[1]]), "forward: same bits twice")
    rep.require(_kept(y[V:]) and all(_kept(t[d:]) for t in (mean, var, inv)), "forward: sentinels kept")
    yc, mc, vc, ic = y[:V].cpu(), mean[:d].cpu(), var[:d].cpu(), inv[:d].cpu()
    for name, e in R.nl_forward_figures(x, inp["G"], inp["c"], eps, yc, mc, vc, ic, R.NL_STAT_COMBINE):
        rep.within(name + " / bound", e, 1.0)
    if backward:
        lddx = lddx or R.nl_lddx(d)[1]
        _dyleaf = torch.full((V, lddy), float("nan"), device=DEV)
        _dyleaf[:, :32] = inp["dy"].to(DEV)
        dyv = _dyleaf[:, :32]
        mean_d, inv_d = mean[:d].clone(), inv[:d].clone()
        bw = [_nl_backward(xv, ld, dyv, lddy, G, mean_d, inv_d, lddx, True, True) for _ in range(2)]
        dx, dG, dc, coef = bw[0]
        rep.require(_same_bits([t.view(torch.int32) for t in bw[0]], [t.view(torch.int32) for t in bw[1]]), "backward: same bits twice")
        rep.require(_dx_kept(dx, V, d) and _kept(dG[32 * d:]) and _kept(dc[32:]) and _kept(coef[34 * R.NL_DP:]), "backward: sentinels kept")
        cf = coef[:34 * R.NL_DP].view(34, R.NL_DP).cpu()
        for name, e in R.nl_backward_figures(x, inp["dy"], inp["G"], mc, ic, dG[:32 * d].view(32, d).cpu(), dc[:32].cpu(), cf):
            rep.within(name + " / bound", e, 1.0)
        rep.require(bool((cf[:, d:] == 0).all()), "coef_out pads == 0")
        for name, e in R.nl_dx_figures(x, inp["dy"], cf, dx[:V, :d].cpu(), rows):
            rep.within(name + " / bound", e, 1.0)
        # the split route: no dx here, the coefficients out, pass 3 on its own
        sp = [_nl_backward(xv, ld, dyv, lddy, G, mean_d, inv_d, lddx, False, True) for _ in range(2)]
        rep.require(all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for a in sp for b in (bw[0],) for k in (1, 2, 3)),
                    "dx = NULL: dG, dc, coef same bits")
        dx2 = [_nl_dx(xv, ld, dyv, lddy, sp[0][3], lddx) for _ in range(2)]
        rep.require(torch.equal(dx2[0].view(torch.int32), dx.view(torch.int32)) and torch.equal(dx2[1].view(torch.int32), dx.view(torch.int32)),
                    "split route: the call's dx bits")
    return yc, mc, vc, ic


@pytest.mark.parametrize("V", R.NL_ROW_V)
@pytest.mark.parametrize("d,ld", R.NL_ROW_DL, ids=["d60", "d71ld72"])
def test_norm_linear_row_edges_against_float64(d, ld, V):
    """Row counts around the 16-row MFMA tile, the 64-row workgroup and 7 / 8 / 9 reduction partials (V = 448, 512, 513), x
    packed (60) and padded (71 in 72).  V = 1: var == 0 exactly and mean == x[0] bit for bit; y inside its bound, which is what
    counts there -- inv = 1 / sqrt(eps) amplifies the difference of two differently ordered sums."""
    inp = R.nl_inputs(V, d)
    rep = Report("nl rows", f"V={V} d={d}")
    y, mean, var, inv = _nl_drive(rep, inp, "packed" if ld == d else "padded")
    if V == 1:
        rep.require(bool((var == 0).all()) and torch.equal(mean, inp["x"][0]), "V = 1: var == 0, mean == x[0]")
    rep.finish()


@pytest.mark.parametrize("layout", R.NL_LAYOUTS)
@pytest.mark.parametrize("d", R.NL_COL_D)
def test_norm_linear_column_edges_against_float64(d, layout):
    """Every width next to a switch of Q = NT = ceil(d / 16) and of the statistics kernel's 64 / 128 lanes per row, x in all
    five layouts (NaN around it: an unmasked over-read meets 0 x NaN in the MFMA), V = 193."""
    rep = Report("nl cols", f"d={d} {layout}")
    _nl_drive(rep, R.nl_inputs(R.NL_COL_V, d), layout)
    rep.finish()


def _nl_grad_cases():
    return [pytest.param(d, lddy, k, xl, id=f"d{d}-lddy{lddy}-lddx{k}-{xl}") for d in R.NL_GRAD_D for lddy in R.NL_GRAD_LDDY
            for k in range(3) for xl in R.NL_GRAD_X]


@pytest.mark.parametrize("d,lddy,k,xlayout", _nl_grad_cases())
def test_norm_linear_gradient_layouts_against_float64(d, lddy, k, xlayout):
    """dy with row strides 32, 36 and 64 (NaN pads), dx with row strides d, roundup4(d) and roundup4(d) + 4 (the pads keep the
    sentinel), x padded and one float behind a 16-byte boundary: both ALIGNED instantiations of the dx kernel, left from the
    side of x and from the side of dx."""
    rep = Report("nl grads", f"d={d} dy{lddy} dx{R.nl_lddx(d)[k]} {xlayout}")
    _nl_drive(rep, R.nl_inputs(R.NL_COL_V, d, seed=1), xlayout, lddy=lddy, lddx=R.nl_lddx(d)[k])
    rep.finish()


@pytest.mark.parametrize("d,lddy,k,xlayout", _nl_grad_cases())
def test_norm_linear_dx_on_a_free_standing_block_against_float64(d, lddy, k, xlayout):
    """scr_norm_linear_dx on a drawn (not derived) Gi | k0 | k1 whose columns d.. are NaN: neither csrc/anchor_gather.hip (it
    drops column 71 of its tile) nor csrc/triplane.hip (it reads its span's columns only) relies on those pads being 0, so
    the kernel must not let them reach a stored column."""
    inp = R.nl_inputs(R.NL_COL_V, d, seed=2)
    V, lddx = inp["V"], R.nl_lddx(d)[k]
    rep = Report("nl dx", f"d={d} dy{lddy} dx{lddx} {xlayout}")
    coef = R.nl_coef_block(d, lddy + k)
    _leaf, xv, ld, _off = R.nl_layout(inp["x"].to(DEV), xlayout)
    dyl = torch.full((V, lddy), float("nan"), device=DEV)
    dyl[:, :32] = inp["dy"].to(DEV)
    runs = [_nl_dx(xv, ld, dyl[:, :32], lddy, coef.to(DEV), lddx) for _ in range(2)]
    for name, e in R.nl_dx_figures(inp["x"], inp["dy"], coef, runs[0][:V, :d].cpu()):
        rep.within(name + " / bound", e, 1.0)
    rep.require(_dx_kept(runs[0], V, d), "sentinels kept")
    rep.require(torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "same bits twice")
    rep.finish()


@pytest.mark.parametrize("V,d,ld", R.NL_STRIDE_CASES, ids=lambda v: str(v))
def test_norm_linear_grid_strides_against_float64(V, d, ld):
    """V = 70 001: the reduction's grid is capped (1024 workgroups of 64 rows) and strides.  V = 140 001: more rows than one
    round of the forward and dx grids holds (8 workgroups x 256 CUs x 64 rows).  Every element is inside its own bound; the
    first row of the second round and the last row are shown on their own."""
    rep = Report("nl stride", f"V={V} d={d}")
    rows = tuple(r for r in (R.NL_FWD_GRID_ROWS, V - 1) if r < V)
    _nl_drive(rep, R.nl_inputs(V, d), "packed" if ld == d else "padded", rows=rows)
    rep.finish()


@pytest.mark.parametrize("V,d,ld", R.NL_SLAB_CASES, ids=lambda v: str(v))
def test_norm_linear_statistics_slabs_against_float64(V, d, ld):
    """The built-in statistics pass: a last slab of 2047, 2048 and 1 rows, of 15 .. 33 rows (in and out of the eight-fold
    unrolled row loop for 2 and 4 row groups), 9 and 65 partials (the unrolled loop of the finish kernel and its tail)."""
    rep = Report("nl slabs", f"V={V} d={d}")
    _nl_drive(rep, R.nl_inputs(V, d), "packed" if ld == d else "padded", backward=False)
    rep.finish()


@pytest.mark.parametrize("rows", R.NL_COLSTAT_ROWS)
def test_norm_linear_caller_statistics_against_float64(rows):
    """col_stats: fp32 roundings of float64 sums over a random partition of the 4099 rows into `rows` sets.  mean / var / inv
    against the bound of sums rounded to fp32 once (the only fp32 roundings are the caller's), y against its own."""
    inp = R.nl_inputs(R.NL_COLSTAT_V, 71)
    rep = Report("nl cstats", f"rows={rows}")
    _nl_drive(rep, inp, "padded", stats=R.nl_col_stats(inp["x"], rows).to(DEV), backward=False)
    rep.finish()


@pytest.mark.parametrize("path", ["builtin", "col_stats"])
@pytest.mark.parametrize("eps", R.NL_EPS)
def test_norm_linear_statistics_regimes_against_float64(eps, path):
    """One [4099,8] matrix, a column per regime (f64_refs.nl_regime_matrix); the error of every column beside its bound.  The
    constant column: var == 0 and mean == 3.25 exactly, inv within an ulp of 1 / sqrt(eps).  The column whose first row -- the
    shift -- lies a thousand deviations off shows what the one-pass formula loses there: E t^2 = 1e6 is rounded to fp32 once
    per slab before mean^2 is taken off a variance of 245."""
    x = R.nl_regime_matrix()
    g = torch.Generator().manual_seed(8)
    inp = dict(V=x.shape[0], d=8, x=x, G=torch.randn(32, 8, generator=g), c=torch.randn(32, generator=g))
    rep = Report("nl regime", f"eps={eps:g} {path}")
    stats = R.nl_col_stats(x, 9).to(DEV) if path == "col_stats" else None
    _, mean, var, inv = _nl_drive(rep, inp, "packed", eps=eps, stats=stats, backward=False)
    sb = R.nl_stats_bounds(x, eps, R.NL_STAT_COMBINE)
    for j, name in enumerate(R.NL_REGIME_COLUMNS):
        for what, got in (("mean", mean), ("var", var), ("inv", inv)):
            ref, b = sb[what]
            rep.within(f"{what} {name}", abs(float(got[j].double() - ref[j])), float(b[j]))
    k = R.NL_REGIME_COLUMNS.index("constant")
    want = 1.0 / float(torch.tensor(eps, dtype=torch.float32)) ** 0.5
    rep.require(float(var[k]) == 0.0 and float(mean[k]) == 3.25, "constant: var == 0, mean == 3.25")
    rep.within("constant: inv, ulps", abs(float(inv[k].double()) - want) / (2.0 ** -23 * want), 1.0)
    rep.require(float(mean[6]) != 0 and float(mean[7]) != 0, "single-row columns: mean != 0")
    rep.finish()


@pytest.mark.parametrize("name", [c[0] for c in R.NL_FOLD_CASES])
def test_norm_fold_kernels_against_float64(name):
    """scr_norm_fold, scr_norm_fold_backward and scr_norm_running_stats (n = 1 and 2 rows; with and without the batch
    counters) against float64, per element: (L + 2) u sum |W gamma| for G, (sum d_i + L) u (sum |W beta| + |b|) for c, 3 u
    of the two products for dW, 34 u of the 32 for the column sums, db == dc, 6 u of the two terms for the running
    statistics; the counters advance by one."""
    from splatco_amd import _C
    p = R.nl_fold_inputs(name)
    rep = Report("nl fold", name)
    d, L = p["d"], len(p["widths"])
    dev = lambda ts: [t.to(DEV) for t in ts]
    f64 = lambda ts: [t.double() for t in ts]
    W, b, ga, be = dev(p["W"]), dev(p["b"]), dev(p["gamma"]), dev(p["beta"])
    wi, ci = _C.host_array(p["widths"]), _C.host_array(p["cols"])
    at = None if p["col_at"] is None else _C.host_array(p["col_at"], _C.u8)
    runs = []
    for _ in range(2):
        G, c = _sent(32 * d + 4), _sent(36)
        _C.call("scr_norm_fold", L, d, wi, ci, at, _C.ptr_array(W), _C.ptr_array(b), _C.ptr_array(ga), _C.ptr_array(be), G, c, device=DEV)
        dW, db = [_sent(32 * w + 4) for w in p["widths"]], [_sent(36) for _ in range(L)]
        dga, dbe = [_sent(w + 4) for w in p["widths"]], [_sent(w + 4) for w in p["widths"]]
        _C.call("scr_norm_fold_backward", L, d, wi, ci, at, _C.ptr_array(W), _C.ptr_array(ga), _C.ptr_array(be), p["dG"].to(DEV),
                p["dc"].to(DEV), _C.ptr_array(dW), _C.ptr_array(db), _C.ptr_array(dga), _C.ptr_array(dbe), device=DEV)
        runs.append([G, c, *dW, *db, *dga, *dbe])
    rep.require(_same_bits([t.view(torch.int32) for t in runs[0]], [t.view(torch.int32) for t in runs[1]]), "same bits twice")
    sizes = [32 * d, 32] + [32 * w for w in p["widths"]] + [32] * L + list(p["widths"]) * 2
    rep.require(all(_kept(t[n:]) for t, n in zip(runs[0], sizes)), "sentinels kept")
    G64, c64 = R.nl_fold_f64(f64(p["W"]), f64(p["b"]), f64(p["gamma"]), f64(p["beta"]), p["widths"], p["cols"], d, p["col_at"])
    bG, bc = R.nl_fold_bounds(p)
    rep.within("G / bound", R.nl_excess(G[:32 * d].view(32, d), G64, bG), 1.0)
    rep.within("c / bound", R.nl_excess(c[:32], c64, bc), 1.0)
    ref = R.nl_fold_backward_f64(p["dG"].double(), p["dc"].double(), f64(p["W"]), f64(p["gamma"]), f64(p["beta"]), p["widths"],
                                 p["cols"], p["col_at"])
    for i, (r4, b4) in enumerate(zip(ref, R.nl_fold_backward_bounds(p))):
        w = p["widths"][i]
        got = (dW[i][:32 * w].view(32, w), db[i][:32], dga[i][:w], dbe[i][:w])
        for tag, g_, r_, b_ in zip(("dW", "db", "dgamma", "dbeta"), got, r4, b4):
            rep.within(f"{tag}[{i}] / bound", R.nl_excess(g_, r_, b_), 1.0)
    mom = _C.host_array(p["momentum"], _C.f32)
    for n in (1, 2):
        for counters in (False, True):
            rm, rv = [_sent(w + 4) for w in p["widths"]], [_sent(w + 4) for w in p["widths"]]
            for t, s in zip(rm + rv, p["run_mean"] + p["run_var"]):
                t[:s.numel()] = s.to(DEV)
            nb = [torch.full((1,), 41 + i, dtype=torch.int64, device=DEV) for i in range(L)]
            _C.call("scr_norm_running_stats", L, d, wi, ci, at, mom, _C.ptr_array(rm), _C.ptr_array(rv),
                    _C.ptr_array(nb) if counters else None, p["mean"].to(DEV), p["var"].to(DEV), n, device=DEV)
            want = R.nl_running_f64(f64(p["run_mean"]), f64(p["run_var"]), p["momentum"], p["mean"].double(), p["var"].double(), n,
                                    p["widths"], p["cols"], p["col_at"])
            e = max(max(R.nl_excess(rm[i][:w], want[i][0], bd[0]), R.nl_excess(rv[i][:w], want[i][1], bd[1]))
                    for i, (w, bd) in enumerate(zip(p["widths"], R.nl_running_bounds(p, n))))
            tag = f"n={n}{' counters' if counters else ''}"
            rep.within(f"running {tag} / bound", e, 1.0)
            rep.require(all(_kept(t[w:]) for ts in (rm, rv) for t, w in zip(ts, p["widths"]))
                        and all(int(t) == 41 + i + (1 if counters else 0) for i, t in enumerate(nb)), f"running {tag}: pads, counters")
    rep.finish()
