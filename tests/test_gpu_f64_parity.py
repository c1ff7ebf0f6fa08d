"""csrc/mlp_heads.hip, csrc/attention.hip and csrc/expand.hip against float64, at the edges of their launch shapes.

Every case runs, on the same packed fp32 inputs (drawn on the CPU, tests/f64_refs.py):
  the kernel, through the product wrapper (mlp_heads.mlp_heads, plane_attention.attended_pair_planes,
  expand.expand_compact), twice -- the second run must give the same bits;
  the fp32 framework chain on the GPU (the reference's ops in float32);
  the float64 reference on the CPU (autograd for the gradients).
For every tensor e = max|got - ref| / max|ref|; for per-anchor / per-candidate / per-pixel tensors the same ratio per
row with the row's scale floored at 1e-3 of the tensor's (f64_refs.err).  The bar is max(floor, c * e_chain), e_chain
being the same figure of the fp32 chain against the same float64 result in the same process: floor 2e-5, c = 1.5 (the
constants of test_fused_norm_linear_matches_batchnorm_linear_chain).  Every figure is printed before anything is
asserted (and appended to the file $SPLATCO_F64_PARITY_LOG names, if set); profiles/r08_f64_parity.txt is one such run.
"""
import copy
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

    def add(self, name, got, chain, ref, rows=False, keep=None, floor=R.FLOOR):
        e, e_chain = R.err(got, ref, rows, keep), R.err(chain, ref, rows, keep)
        b = R.bar(e_chain, floor)
        self.lines.append(f"{self.op:9s} {self.case:16s} {name:22s} e {e:9.3e}  e_chain {e_chain:9.3e}  bar {b:9.3e}"
                          f"{'' if e <= b else '   <-- FAIL'}")
        if not e <= b:
            self.failed.append((name, e, e_chain, b))

    def require(self, ok, what):
        self.lines.append(f"{self.op:9s} {self.case:16s} {what:22s} {'ok' if ok else 'FAIL'}")
        if not ok:
            self.failed.append((what,))

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


@pytest.mark.parametrize("V", R.HEADS_V)
def test_mlp_heads_against_float64(V):
    """16-row tiles, 4 tiles per workgroup, backward grid capped at 256 workgroups, forward at 512: the row counts give
    4, 60, 64, 68, 128 and 1024 weight-gradient partials (the unrolled loop of mlp_heads_reduce_kernel alone, its tail
    alone, both), a last tile of 1, 15 and 16 rows alone and behind full workgroups, the first backward grid-stride
    (16385) and the first forward one (32769).  geo_fea arrives as one [V,64] matrix or as its two halves, alternating.
    The two largest sizes carry the edge rows of f64_refs.heads_inputs: a hidden unit that is exactly 0, second-layer
    pre-activations of +-40, +-100 (saturated tanh / sigmoid) and +-1e-4 (where 1 - 2 / (1 + e^2z) cancels)."""
    from splatco_amd.mlp_heads import mlp_heads, supported
    d = R.heads_inputs(V)
    rep = Report("heads", f"V={V}")
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
        for p in pc.parameters():
            p.grad = None
        assert supported(pc, f, ge)
        if two_parts:
            outs = mlp_heads(pc, f, a, campos, ge[:, :32].contiguous(), ge[:, 32:].contiguous())
        else:
            outs = mlp_heads(pc, f, a, campos, ge)
        sum((o * u).sum() for o, u in zip(outs, up)).backward()
        grads = {"feat": f.grad, "anchor": a.grad, "geo": ge.grad}
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


@pytest.mark.parametrize("name,V,k,select,edges", R.EXPAND_CASES, ids=[c[0] for c in R.EXPAND_CASES])
def test_expand_compact_against_float64(name, V, k, select, edges):
    """k = 1, 5, 10, 33 offsets per anchor; n = V k candidates on both sides of the first workgroup (1024) and of the
    1024 and 2048 workgroups after which expand_scan_kernel carries its running total into the next chunk; everything
    kept, nothing kept, every other candidate kept.  The k cases carry the edge rows of f64_refs.expand_inputs: zero
    and 1e-20 quaternions (the clamped branch of the normalisation, forward and backward), scale_rot[:, :3] = +-90
    (saturated sigmoid), neural_opacity +0.0, -0.0 and the smallest subnormal (the mask is `> 0`).  The mask is exact
    on identical inputs: indices and mask are compared with torch.nonzero for equality, nothing is left out."""
    from splatco_amd.expand import expand_compact
    from splatco_amd.losses import scaling_reg
    d = R.expand_inputs(V, k, select, edges)
    rep = Report("expand", name)
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
            *outs, mask = expand_compact(*ins, k)
            loss = sum((o * u).sum() for o, u in zip(outs, upd))
            if reg and P:
                loss = loss + reg * scaling_reg(outs[3])
            loss.backward()
            runs.append(([o.detach() for o in outs], mask, mask._scr_out_index, [t.grad for t in ins]))
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
