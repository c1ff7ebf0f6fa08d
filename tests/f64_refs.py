"""Float64 references of the three anchor-path operators between the sampler and the rasterizer and of the image losses
behind it, and the inputs the parity tests feed them.  TEST INFRASTRUCTURE ONLY; nothing here imports the native library.

  heads_f64       the three Linear-ReLU-Linear heads on x = cat(feat, ob_view, geo_fea)      -> checker of csrc/mlp_heads.hip
  attention_f64   TriPlaneAttention + chunk + cat(plane, attended plane)                     -> checker of csrc/attention.hip
  expand_f64      torch_restatements.expand_torch_chain on double inputs                     -> checker of csrc/expand.hip
  ssim_f64        losses.l1_loss + losses.ssim in float64 (and the inputs of pair_l1 / scaling_reg) -> checker of csrc/ssim.hip
  gather_f64      the four visible-anchor gathers, exp and cat; gather_dx_f64 the fused dx         -> checker of csrc/anchor_gather.hip

The references are plain torch op chains, written from scene_model.py / torch_restatements.py, dtype- and device-agnostic:
on float64 CPU tensors they are the reference, on float32 device tensors the "framework chain" whose own error against
the float64 result sets the bar of the kernel (tests/test_gpu_f64_parity.py).  Every input is drawn on the CPU from a
seeded generator, so the host tests (tests/test_f64_refs_host.py) see exactly the inputs the GPU tests use.

Decisive inputs.  A float64 reference and an fp32 kernel may legitimately disagree where a discrete choice hangs on
rounding: a ReLU whose pre-activation is a rounding error away from 0, a channel maximum with a runner-up a rounding
error below it.  Whether an input is decisive is decided here, by the reference alone.
"""
import torch
import torch.nn.functional as F

from torch_restatements import expand_torch_chain

# ---------------------------------------------------------------------------------------------------------- comparison
FLOOR, C_CHAIN = 2e-5, 1.5      # bar = max(FLOOR, C_CHAIN * e_chain): test_fused_norm_linear_matches_batchnorm_linear_chain


def _f64(t):
    return t.detach().to("cpu", torch.float64)


def err(got, ref, rows=False, keep=None, scale_floor=None, row_floor=None):
    """max|got - ref| / max|ref|.  rows: `got` / `ref` are [rows, ...]; the ratio is taken per row, the row's scale
    floored at 1e-3 of the tensor's, and the largest row is returned (>= the tensor-level ratio by construction): a
    wrong tail row cannot hide behind 1e5 good ones.  keep: bool [rows], rows that take part.  scale_floor: an absolute
    floor under the tensor's scale, row_floor: one under each row's (for a reference that may be zero throughout)."""
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.numel() == 0:
        return 0.0
    scale = float(ref.abs().max())
    if scale_floor is not None:
        scale = max(scale, scale_floor)
    if not rows:
        d = float((got - ref).abs().max())
        return d / scale if scale > 0 else (0.0 if d == 0 else float("inf"))
    got, ref = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    d = (got - ref).abs().amax(dim=1)
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    s = ref.abs().amax(dim=1).clamp_min(1e-3 * scale)
    if row_floor is not None:
        s = s.clamp_min(row_floor)
    if keep is not None:
        d, s = d[keep], s[keep]
        if d.numel() == 0:
            return 0.0
    if scale == 0:
        return 0.0 if float(d.max()) == 0 else float("inf")
    return float((d / s).max())


def bar(e_chain, floor=FLOOR, c=C_CHAIN):
    return max(floor, c * e_chain)


# ---------------------------------------------------------------------------------------------------------- heads
HEADS_V = [1, 15, 16, 17, 63, 64, 65, 960, 961, 1025, 1985, 16383, 16384, 16385, 32768, 32769, 49153, 100003]
HEADS_EDGE_V = (49153, 100003)                  # the two largest sizes also carry the edge rows
HEADS_TOL = 100 * 2.0 ** -24                    # a-priori bound of a 100-term fp32 dot product, relative to sum |w x| + |b|
HEADS_CAP, HEADS_ROUNDS = 0.01, 8
HEAD_NAMES = ("opacity", "color", "cov")
HEAD_OUT = (10, 30, 70)
# second-layer pre-activations planted in output 0 of the tanh (opacity) and sigmoid (colour) heads of the edge rows
EDGE_Z = (40.0, -40.0, 100.0, -100.0, 1e-4, -1e-4)
ZERO_UNIT = 5                                   # hidden unit of the covariance head that is exactly 0 on every row


def heads_weights(seed, edges=False):
    """A model whose three heads carry the modules' init plus 0.2 randn (as test_fused_mlp_heads_match_the_torch_chain).
    edges: the weights that let heads_inputs plant its edge rows, and the zero unit."""
    from splatco_amd.scene_model import AnchorGaussianModel
    torch.manual_seed(seed)
    pc = AnchorGaussianModel(plane_size=16, num_channels=15)
    heads = (pc.mlp_opacity, pc.mlp_color, pc.mlp_cov)
    with torch.no_grad():
        for h in heads:
            for p in h.parameters():
                p.add_(0.2 * torch.randn_like(p))
        if edges:
            for h in heads[:2]:
                # feat column 0 feeds only the hidden units 0 (+) and 1 (-), and these feed only output 0:
                # z[0] = relu(t) - relu(-t) + rest = t + rest with t = feat[v, 0]
                h[0].weight[:, 0] = 0
                h[0].weight[:2] = 0
                h[0].bias[:2] = 0
                h[0].weight[0, 0], h[0].weight[1, 0] = 1.0, -1.0
                h[2].weight[:, :2] = 0
                h[2].weight[0, 0], h[2].weight[0, 1] = 1.0, -1.0
            heads[2][0].weight[ZERO_UNIT] = 0       # pre-activation exactly 0: relu'(0) = 0
            heads[2][0].bias[ZERO_UNIT] = 0
    return pc


def weights_of(pc, dtype=torch.float64, device="cpu", requires_grad=False):
    """{'w1': 3 x [32,99], 'b1': 3 x [32], 'w2': 3 x [n,32], 'b2': 3 x [n]} (opacity, colour, cov): copies of the heads' weights."""
    heads = (pc.mlp_opacity, pc.mlp_color, pc.mlp_cov)
    c = lambda t: t.detach().to(device, dtype).clone().requires_grad_(requires_grad)
    return {"w1": [c(h[0].weight) for h in heads], "b1": [c(h[0].bias) for h in heads],
            "w2": [c(h[2].weight) for h in heads], "b2": [c(h[2].bias) for h in heads]}


def _heads_layers(feat, anchor, campos, geo, w):
    ob = anchor - campos
    ob = ob / ob.norm(dim=1, keepdim=True)
    x = torch.cat([feat, ob, geo], dim=1)
    zs, pres, bounds = [], [], []
    for i in range(3):
        pre = F.linear(x, w["w1"][i], w["b1"][i])
        zs.append(F.linear(F.relu(pre), w["w2"][i], w["b2"][i]))
        pres.append(pre)
        bounds.append(x.detach().abs() @ w["w1"][i].detach().abs().T + w["b1"][i].detach().abs())
    return zs, torch.cat(pres, dim=1), torch.cat(bounds, dim=1)


def heads_f64(feat, anchor, campos, geo, w):
    """((opacity [V,10], color [V,30], cov [V,70]), pre [V,96], bound [V,96]): the heads, the stacked hidden
    pre-activations and per hidden unit sum_i |w_i x_i| + |b| (the scale its rounding error is relative to)."""
    zs, pre, bound = _heads_layers(feat, anchor, campos, geo, w)
    return (torch.tanh(zs[0]), torch.sigmoid(zs[1]), zs[2]), pre, bound


def heads_undecided(feat, anchor, campos, geo, w64):
    """bool [V]: rows with a hidden unit whose sign the fp32 rounding could flip.  A unit whose terms are all exactly 0
    is exact in every precision and counts as decided."""
    with torch.no_grad():
        _, pre, bound = heads_f64(feat.double(), anchor.double(), campos.double(), geo.double(), w64)
    return ((pre.abs() <= HEADS_TOL * bound) & (bound > 0)).any(dim=1)


def heads_inputs(V):
    """fp32 CPU inputs of one heads case: dict(pc, feat, anchor, campos, geo, up (upstream gradients), flagged (share of
    rows the first draw flagged), rounds, edge_rows).  Rows with an undecided unit are replaced: their feat is redrawn
    from the same generator, at most HEADS_ROUNDS times."""
    edges = V in HEADS_EDGE_V
    pc = heads_weights(V, edges)
    w64 = weights_of(pc)
    g = torch.Generator().manual_seed(V + 1)
    r = lambda *s: torch.randn(*s, generator=g)
    feat, anchor, geo, campos = r(V, 32), r(V, 3) * 2, r(V, 64), torch.tensor([0.3, -0.2, -5.0])
    up = [r(V, n) for n in HEAD_OUT]
    bad = heads_undecided(feat, anchor, campos, geo, w64)
    flagged, rounds = float(bad.float().mean()), 0
    while bad.any() and rounds < HEADS_ROUNDS:
        feat[bad] = r(int(bad.sum()), 32)
        bad = heads_undecided(feat, anchor, campos, geo, w64)
        rounds += 1
    edge_rows = {}
    if edges:
        # one row per planted value and head, spread over the first and last tiles and both sides of the grid-stride onsets
        rows = [0, 15, 16, 4095, 16383, 16384, 32767, 32768, V - 17, V - 16, V - 2, V - 1]
        with torch.no_grad():
            f0 = feat.clone()
            f0[:, 0] = 0
            zs, _, _ = _heads_layers(f0.double(), anchor.double(), campos.double(), geo.double(), w64)
            rest = {0: zs[0][:, 0], 1: zs[1][:, 0]}                     # z[0] at t = 0
        for j, row in enumerate(rows):
            head, z = j // len(EDGE_Z), EDGE_Z[j % len(EDGE_Z)]
            feat[row, 0] = float(z - rest[head][row])
            edge_rows[row] = (head, z)
        bad = heads_undecided(feat, anchor, campos, geo, w64)
    assert not bad.any(), f"V={V}: {int(bad.sum())} undecided rows left after {rounds} rounds"
    return dict(pc=pc, feat=feat, anchor=anchor, campos=campos, geo=geo, up=up, flagged=flagged, rounds=rounds,
                edge_rows=edge_rows)


def heads_run(feat, anchor, campos, geo, up, w):
    """Forward + backward of heads_f64 in the dtype / on the device of its arguments: (outs, grads dict)."""
    f, a, ge = (t.detach().clone().requires_grad_(True) for t in (feat, anchor, geo))
    outs, _, _ = heads_f64(f, a, campos, ge, w)
    sum((o * u).sum() for o, u in zip(outs, up)).backward()
    grads = {"feat": f.grad, "anchor": a.grad, "geo": ge.grad}
    for i, h in enumerate(("mlp_opacity", "mlp_color", "mlp_cov")):
        grads.update({f"{h}.0.weight": w["w1"][i].grad, f"{h}.0.bias": w["b1"][i].grad,
                      f"{h}.2.weight": w["w2"][i].grad, f"{h}.2.bias": w["b2"][i].grad})
    return [o.detach() for o in outs], grads


# ---------------------------------------------------------------------------------------------------------- attention
ATTN_R = [2, 3, 4, 5, 6, 7, 8]                                       # at (37, 91): every instantiation the module reaches
ATTN_HW = [(1, 1), (2, 3), (3, 200), (200, 3), (5, 5), (16, 64), (15, 63), (17, 65), (32, 128), (700, 700)]
ATTN_TIES = ("constant", "two_blocks", "one_block")                  # at 5 x 48 x 130
ATTN_TIE_SHAPE = (5, 48, 130)
ATTN_CASES = ([("R%d" % R, R, 37, 91, None) for R in ATTN_R] + [("%dx%d" % hw, 5, hw[0], hw[1], None) for hw in ATTN_HW]
              + [("tie_" + t, *ATTN_TIE_SHAPE, t) for t in ATTN_TIES])
ATTN_TOL, ATTN_CAP = 1e-5, 1e-3
STAT_BLOCKS = 64                                                     # pooling blocks per channel (TPA_STAT_BLOCKS)


def attention_f64(planes, w1, w2, wc):
    """planes: three [1,R,H,W]; w1 [C//5,C,1,1], w2 [C,C//5,1,1] the shared MLP, wc [1,2,7,7] the window.
    -> (pairs: three [1,2R,H,W] = cat(plane, attended plane), y = ca * x [1,C,H,W]).  The pools are the reference's
    AdaptiveAvgPool2d(1) / AdaptiveMaxPool2d(1): a tied maximum belongs to its first pixel, in value and in gradient."""
    x = torch.cat(planes, dim=1)
    mlp = lambda t: F.conv2d(F.relu(F.conv2d(t, w1)), w2)
    ca = torch.sigmoid(mlp(F.adaptive_avg_pool2d(x, 1)) + mlp(F.adaptive_max_pool2d(x, 1)))
    y = ca * x
    s = torch.cat([y.mean(dim=1, keepdim=True), torch.max(y, dim=1, keepdim=True)[0]], dim=1)
    tri = torch.sigmoid(F.conv2d(s, wc, padding=3)) * y
    return [torch.cat((p, a), dim=1) for p, a in zip(planes, torch.chunk(tri, 3, dim=1))], y


def attention_undecided(y):
    """bool [H,W]: pixels whose two largest channels of y are closer than ATTN_TOL * max|y| (the fp32 kernel may route
    the max gradient of such a pixel to the other channel)."""
    top = torch.topk(y.detach()[0], 2, dim=0)[0]
    return (top[0] - top[1]) <= ATTN_TOL * float(y.detach().abs().max())


def attention_inputs(R, H, W, tie=None):
    """fp32 CPU inputs of one attention case: dict(ta (the module), planes, up, arg (first maximum of every channel))."""
    from splatco_amd.scene_model import TriPlaneAttention
    torch.manual_seed(R * 1000 + H)
    ta = TriPlaneAttention(3 * R)
    g = torch.Generator().manual_seed(R * 100003 + H * 1009 + W)
    planes = [torch.randn(1, R, H, W, generator=g) * 0.5 for _ in range(3)]
    HW = H * W
    per = (HW + STAT_BLOCKS - 1) // STAT_BLOCKS                      # pixels per pooling block
    if tie == "constant":
        planes[1][:] = 0.25                                          # every pixel of R channels is the maximum
    elif tie == "two_blocks":
        p = planes[0][0, 2].view(-1)
        p[3 * per + 7] = p[40 * per + 1] = float(p.max()) + 1.0
    elif tie == "one_block":
        p = planes[2][0, 1].view(-1)
        p[10 * per + 70] = p[10 * per + 5] = float(p.max()) + 1.0
        assert per > 70
    up = [torch.randn(1, 2 * R, H, W, generator=g) for _ in range(3)]
    x = torch.cat(planes, dim=1)[0].reshape(3 * R, HW)
    mx = x.amax(dim=1, keepdim=True)
    arg = (x == mx).int().argmax(dim=1).to(torch.int32)              # first maximum
    return dict(ta=ta, planes=planes, up=up, arg=arg)


def attention_weights(ta, dtype=torch.float64, device="cpu", requires_grad=False):
    c = lambda t: t.detach().to(device, dtype).clone().requires_grad_(requires_grad)
    return [c(ta.ca.sharedMLP[0].weight), c(ta.ca.sharedMLP[2].weight), c(ta.sa.conv.weight)]


def attention_run(planes, up, ws):
    """Forward + backward of attention_f64 in the dtype / on the device of its arguments:
    (pairs, y, plane gradients, [d w1, d w2, d wc])."""
    ps = [p.detach().clone().requires_grad_(True) for p in planes]
    pairs, y = attention_f64(ps, *ws)
    sum((o * u).sum() for o, u in zip(pairs, up)).backward()
    return [o.detach() for o in pairs], y.detach(), [p.grad for p in ps], [w.grad for w in ws]


# ---------------------------------------------------------------------------------------------------------- expansion
EXPAND_K = [1, 5, 10, 33]                                            # at V = 4099, with the edge rows
EXPAND_V_K = 4099
EXPAND_N = [10, 1020, 1030, 1_048_570, 1_048_580, 2_100_010]         # k = 10: first workgroup, 1024 and 2048 workgroups of the scan
EXPAND_SELECT = ("all", "none", "alternating")                       # at n = 1030
EXPAND_CASES = ([("k%d" % k, EXPAND_V_K, k, "random", True) for k in EXPAND_K]
                + [("n%d" % n, n // 10, 10, "random", False) for n in EXPAND_N]
                + [("sel_" + s, 103, 10, s, False) for s in EXPAND_SELECT])
SUBNORMAL = 2.0 ** -149


def expand_f64(neural_opacity, color, scale_rot, grid_offsets, grid_scaling, anchor, k):
    return expand_torch_chain(neural_opacity, color, scale_rot, grid_offsets, grid_scaling, anchor, k)


def expand_inputs(V, k, select="random", edges=False):
    """fp32 CPU inputs of one expansion case: dict(args (the six tensors), k, edge (candidate index by name))."""
    g = torch.Generator().manual_seed(V * 131 + k)
    r = lambda *s: torch.randn(*s, generator=g)
    n = V * k
    no, color, sr, off = r(n, 1), r(n, 3), r(n, 7), r(V, k, 3)
    gs, anchor = torch.rand(V, 6, generator=g) + 0.1, r(V, 3)
    if select == "all":
        no = no.abs() + 0.01
    elif select == "none":
        no = -no.abs()
    elif select == "alternating":
        no = (no.abs() + 0.01) * (1.0 - 2.0 * (torch.arange(n) % 2)).view(n, 1)
    edge = {}
    if edges:
        # candidates spread over the first, a middle and the last workgroup; all of them kept unless the row is about
        # the mask itself
        at = [1, 2, 3, 4, 5, 6, n // 2, n // 2 + 1, n - 2, n - 1] if n >= 64 else None
        assert at is not None
        names = ["quat_zero", "quat_tiny", "sig_hi", "sig_lo", "op_pzero", "op_nzero", "op_subnormal", "quat_zero2",
                 "sig_mixed", "quat_tiny2"]
        edge = dict(zip(names, at))
        no[at] = no[at].abs() + 0.01
        sr[edge["quat_zero"], 3:] = 0.0
        sr[edge["quat_zero2"], 3:] = 0.0
        sr[edge["quat_tiny"], 3:] = 1e-20 * torch.tensor([1.0, -2.0, 0.5, 3.0])
        sr[edge["quat_tiny2"], 3:] = 1e-20 * torch.tensor([0.0, 0.0, 1.0, 0.0])
        sr[edge["sig_hi"], :3] = 90.0
        sr[edge["sig_lo"], :3] = -90.0
        sr[edge["sig_mixed"], :3] = torch.tensor([90.0, -90.0, 0.0])
        no[edge["op_pzero"]] = 0.0
        no[edge["op_nzero"]] = -0.0
        no[edge["op_subnormal"]] = SUBNORMAL
    return dict(args=[no, color, sr, off, gs, anchor], k=k, edge=edge)


def expand_upstream(P, edge_pos, seed):
    """Upstream gradients of the five outputs for P kept candidates.  The rot gradient of the clamped-quaternion rows
    (positions edge_pos among the kept) is scaled by 1e-12: d scale_rot = g / 1e-12 there, and O(1) values keep the
    tensor's scale -- and with it the bar of every other row -- where it is without them."""
    g = torch.Generator().manual_seed(seed)
    up = [torch.randn(P, c, generator=g) for c in (3, 3, 1, 3, 4)]
    for p in edge_pos:
        up[4][p] *= 1e-12
    return up


def expand_run(args, k, up, reg=0.0):
    """Forward + backward of expand_f64 in the dtype / on the device of its arguments; reg: weight of the regulariser
    mean(prod(scaling, 1)).  -> (outputs, mask, gradients of the six inputs)."""
    ins = [t.detach().clone().requires_grad_(True) for t in args]
    *outs, mask = expand_f64(*ins, k)
    loss = sum((o * u).sum() for o, u in zip(outs, up))
    if reg and outs[3].shape[0]:
        loss = loss + reg * outs[3].prod(dim=1).mean()
    if loss.requires_grad:
        loss.backward()
    grads = [t.grad if t.grad is not None else torch.zeros_like(t) for t in ins]
    return [o.detach() for o in outs], mask, grads


# ---------------------------------------------------------------------------------------------------------- image losses
# csrc/ssim.hip: l1_ssim (16 x 16 tiles, window radius 5, 256 threads, one reduce workgroup striding by 1024), pair_l1
# (4096 elements per workgroup) and scaling_reg (2048 rows per workgroup); the last two share a finish kernel striding
# by 1024 partials.
SSIM_TILE, SSIM_RADIUS, SSIM_REDUCE = 16, 5, 1024
SSIM_SHAPES = ([(3, h, w) for h, w in [(1, 1), (1, 40), (40, 1), (5, 7), (10, 10), (11, 11), (12, 12), (16, 16), (32, 48),
                                       (15, 17), (17, 15), (33, 37), (21, 21), (22, 22)]]
               + [(1, 17, 33), (2, 17, 33), (4, 17, 33), (3, 300, 300)])
SSIM_CONTENT = ("noise", "identical", "ties", "flat", "flat_both", "ramp", "zeros", "anti", "range", "impulse")
SSIM_CONTENT_SHAPE = (3, 33, 37)
# (g_l1, g_ssim); None: the graph does not use that output (autograd hands the kernel a zero for it)
SSIM_UPSTREAM = [(0.8, -0.2), (1.0, 0.0), (0.0, 1.0), (-3.5, 7e3), (1.0, None), (None, 1.0)]
SSIM_NONFINITE = {"nan_x": ("x", (1, 16, 16), float("nan")), "nan_y": ("y", (1, 3, 35), float("nan")),
                  "inf_x": ("x", (0, 0, 0), float("inf"))}
SSIM_FAULTS = ("reach4_right", "clamp", "no_mu2_dE12", "map_index", "reduce_1024", "sign0_is_1", "tap_sum_ulp")


def _up_name(up):
    return "up_" + "_".join("none" if g is None else "%g" % g for g in up)


# (name, (C, H, W), content, (g_l1, g_ssim), non-finite key or None)
SSIM_CASES = ([("%s%dx%d" % ("" if s[0] == 3 else "c%d_" % s[0], s[1], s[2]), s, "noise", SSIM_UPSTREAM[0], None)
               for s in SSIM_SHAPES]
              + [(c, SSIM_CONTENT_SHAPE, c, (0.0, -0.2) if c == "impulse" else SSIM_UPSTREAM[0], None) for c in SSIM_CONTENT]
              + [(_up_name(u), SSIM_CONTENT_SHAPE, "noise", u, None) for u in SSIM_UPSTREAM[1:]]
              + [(k, SSIM_CONTENT_SHAPE, "noise", SSIM_UPSTREAM[0], k) for k in SSIM_NONFINITE])
SSIM_IDS = [c[0] for c in SSIM_CASES]


def ssim_inputs(name):
    """fp32 CPU inputs of one l1_ssim case: dict(x, y, up, nonfinite)."""
    _, (C, H, W), content, up, nonfinite = SSIM_CASES[SSIM_IDS.index(name)]
    g = torch.Generator().manual_seed(1000 * C + 37 * H + W)
    rand, randn = lambda: torch.rand(C, H, W, generator=g), lambda: torch.randn(C, H, W, generator=g)
    x = rand()                                                         # noise: what test_fused_l1_ssim_matches_torch draws
    y = (x + 0.15 * randn()).clamp(0, 1)
    if content == "identical":
        y = x.clone()
    elif content == "ties":
        y = torch.where(rand() < 0.5, x, y)
    elif content == "flat":
        x, y = 0.9 + 1e-3 * randn(), torch.full((C, H, W), 0.9)
    elif content == "flat_both":
        x, y = 1.0 + 1e-3 * randn(), 1.0 + 1e-3 * randn()
    elif content == "ramp":
        ramp = torch.linspace(0, 1, W).expand(C, H, W)
        x, y = ramp + 1e-3 * randn(), 0.95 * ramp + 0.02
    elif content == "zeros":
        x, y = torch.zeros(C, H, W), torch.zeros(C, H, W)
    elif content == "anti":
        y = 1.0 - x
    elif content == "range":
        x, y = 4.0 * rand() - 1.0, 4.0 * rand() - 1.0
    elif content == "impulse":                                         # the two pixels sit in the four tiles' common corner
        y = x.clone()
        x[:, 15, 15] += 0.25
        x[:, 16, 16] -= 0.25
    if nonfinite:
        which, at, value = SSIM_NONFINITE[nonfinite]
        (x if which == "x" else y)[at] = value
    return dict(x=x.contiguous(), y=y.contiguous(), up=up, nonfinite=nonfinite)


def ssim_window():
    """The 11 taps as the reference project and make_window() of csrc/ssim.hip have them: built and normalised in fp32,
    their sum the correctly rounded one (equal to torch's g.sum() for these taps, losses._window; spelled out here so
    that the reference does not hang on a summation order).  An ulp on that sum is 1.5e-7 on the window's total and, on a flat
    image, 3.3e-4 of the gradient: the `flat` cases see it."""
    from math import exp
    g = torch.tensor([exp(-(i - SSIM_RADIUS) ** 2 / float(2 * 1.5 ** 2)) for i in range(2 * SSIM_RADIUS + 1)])
    return g / g.double().sum().float()


def _ssim_loss(l1, s, up):
    terms = [g * v for g, v in zip(up, (l1, s)) if g is not None]
    return terms[0] if len(terms) == 1 else terms[0] + terms[1]


def ssim_f64(x, y, up=None):
    """losses.ssim and losses.l1_loss restated in float64 on the CPU (the fp32 taps cast up, the 2-D window their outer
    product in double): (mean |x - y|, mean SSIM, d (g_l1 L1 + g_ssim SSIM) / dx by autograd, or None without `up`)."""
    x, y = _f64(x).requires_grad_(up is not None), _f64(y)
    C = x.shape[0]
    g = ssim_window().double()
    w = torch.outer(g, g).expand(C, 1, g.numel(), g.numel()).contiguous()
    conv = lambda t: F.conv2d(t.unsqueeze(0), w, padding=SSIM_RADIUS, groups=C).squeeze(0)
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = conv(x * x) - mu1_sq, conv(y * y) - mu2_sq, conv(x * y) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    s = (((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s11 + s22 + C2))).mean()
    l1 = (x - y).abs().mean()
    dx = torch.autograd.grad(_ssim_loss(l1, s, up), x)[0] if up is not None else None
    return l1.detach(), s.detach(), dx


def ssim_chain(x, y, up):
    """The fp32 framework chain (losses.l1_loss, losses.ssim) on the device of its arguments: (L1, SSIM, dx)."""
    from splatco_amd.losses import l1_loss, ssim
    x = x.detach().clone().requires_grad_(True)
    l1, s = l1_loss(x, y), ssim(x, y)
    _ssim_loss(l1, s, up).backward()
    return l1.detach(), s.detach(), x.grad


def ssim_restated_f32(x, y, g_l1, g_ssim, fault=None, with_maps=False):
    """csrc/ssim.hip's arithmetic in plain fp32 torch on the CPU: zero-padded halo, separable window (horizontal pass,
    then vertical, taps added in order), the moments, A1 A2 B1 B2, the two reciprocals and the three derivative maps in
    the kernel's order, the same window over the maps, c0 + 2 x c1 + y c2; sums in double (with_maps: the maps
    [3,C,H,W] as a fourth result).  (The device contracts
    g * a + acc to one fma and adds a tile in fp32 before the double sum: neither is restated.)  -> (L1, SSIM, dx).
    fault: one of SSIM_FAULTS, a deliberate error --
      reach4_right   the staged tile is one column short on the right: the last tap of the horizontal pass reads 0 at
                     the pixels of a tile's last column (forward and backward)
      clamp          clamp-to-edge instead of zero padding (images and maps)
      no_mu2_dE12    dmu1 without its - mu2 dE12 term
      map_index      the backward reads map m of channel c at (c * 3 + m) where the forward wrote it at (m * C + c)
      reduce_1024    tiles with index >= 1024 are left out of the two sums
      sign0_is_1     sign(0) = 1 in the L1 gradient
      tap_sum_ulp    the taps divided by their sum added one by one in fp32, an ulp below the correctly rounded one"""
    assert fault is None or fault in SSIM_FAULTS, fault
    x, y = x.detach().float().cpu(), y.detach().float().cpu()
    C, H, W = x.shape
    T, Rr, g = SSIM_TILE, SSIM_RADIUS, ssim_window()
    if fault == "tap_sum_ulp":
        from math import exp
        raw = torch.tensor([exp(-(i - Rr) ** 2 / float(2 * 1.5 ** 2)) for i in range(2 * Rr + 1)])
        total = torch.zeros(())
        for v in raw:
            total = total + v
        g = raw / total
    taps = 2 * Rr + 1
    last_col = (torch.arange(W) % T == T - 1)

    def pad(t):
        if fault == "clamp":
            return F.pad(t.unsqueeze(0), (Rr, Rr, Rr, Rr), mode="replicate").squeeze(0)
        return F.pad(t, (Rr, Rr, Rr, Rr))

    def window(t):                                                     # [..., H + 10, W + 10] -> [..., H, W]
        hz = torch.zeros(*t.shape[:-1], W)
        for k in range(taps):
            term = g[k] * t[..., k:k + W]
            if fault == "reach4_right" and k == taps - 1:
                term = torch.where(last_col, torch.zeros(()), term)
            hz = hz + term
        out = torch.zeros(*t.shape[:-2], H, W)
        for k in range(taps):
            out = out + g[k] * hz[..., k:k + H, :]
        return out
    a, b = pad(x), pad(y)
    mu1, mu2, e11, e22, e12 = window(torch.stack([a, b, a * a, b * b, a * b]))
    C1, C2 = torch.tensor(0.01) * torch.tensor(0.01), torch.tensor(0.03) * torch.tensor(0.03)
    mu1s, mu2s, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = e11 - mu1s, e22 - mu2s, e12 - mu12
    A1, A2, B1, B2 = 2.0 * mu12 + C1, 2.0 * s12 + C2, mu1s + mu2s + C1, s11 + s22 + C2
    iB1, iB2 = 1.0 / B1, 1.0 / B2
    ss = (A1 * A2) * (iB1 * iB2)
    l1 = (x - y).abs()
    dE11 = -ss * iB2
    dE12 = 2.0 * A1 * (iB1 * iB2)
    dmu1 = 2.0 * mu2 * A2 * (iB1 * iB2) - 2.0 * mu1 * ss * iB1
    if fault != "no_mu2_dE12":
        dmu1 = dmu1 - mu2 * dE12
    dmu1 = dmu1 - 2.0 * mu1 * dE11
    n = C * H * W
    keep = torch.ones(C, H, W, dtype=torch.bool)
    if fault == "reduce_1024":
        gy, gx = (H + T - 1) // T, (W + T - 1) // T
        tile = ((torch.arange(C).view(C, 1, 1) * gy + torch.arange(H).view(1, H, 1) // T) * gx
                + torch.arange(W).view(1, 1, W) // T)
        keep = tile < SSIM_REDUCE
    inv = 1.0 / float(n)
    L1 = (l1.double()[keep].sum() * inv).float()
    S = (ss.double()[keep].sum() * inv).float()
    maps = torch.stack([dmu1, dE11, dE12])                             # [3, C, H, W]: (m * C + c) * plane
    if fault == "map_index":
        flat = maps.reshape(3 * C, H, W)
        maps = torch.stack([torch.stack([flat[c * 3 + m] for c in range(C)]) for m in range(3)])
    c0, c1, c2 = window(pad(maps.reshape(3 * C, H, W)).reshape(3, C, H + 2 * Rr, W + 2 * Rr))
    d = x - y
    one = torch.ones(())
    sgn = torch.where(d > 0, one, torch.where(d < 0, -one, one if fault == "sign0_is_1" else torch.zeros(())))
    inv_n = torch.tensor(inv, dtype=torch.float64).float()
    gl = torch.tensor(0.0 if g_l1 is None else g_l1, dtype=torch.float32)
    gs = torch.tensor(0.0 if g_ssim is None else g_ssim, dtype=torch.float32)
    dx = (gl * inv_n) * sgn + (gs * inv_n) * (c0 + 2.0 * x * c1 + y * c2)
    return (L1, S, dx, maps) if with_maps else (L1, S, dx)


# The summation order of csrc/wg.h, pinned where binary32 shows it: the L1 output of scr_l1_ssim_forward.  Shapes with
# one live pixel, one tile, ragged tiles, several tiles, and 1083 tiles (the reduce workgroup's second stride).  For
# every shape with more than one wave of live pixels the seed was chosen by a CPU search (lowest seed from 0) so that the
# final bits under the documented order differ from those under BOTH alternatives of L1_ORDER_ALTERNATIVES: the final
# rounding to binary32 hides most changes of order, and a test on a seed that hides them would pin nothing.
# (3, 1, 1) has one live lane per tile: no order can differ, only equality is asked (seed None: no condition).
L1_ORDER_SHAPES = [(3, 1, 1), (1, 16, 16), (3, 17, 33), (3, 48, 80), (3, 304, 304)]
L1_ORDER_SEEDS = {(3, 1, 1): None, (1, 16, 16): 6, (3, 17, 33): 10, (3, 48, 80): 30, (3, 304, 304): 6}
L1_ORDER_ALTERNATIVES = ("pairwise", "serial")


def l1_order_inputs(shape):
    """fp32 numpy (x, y) of one order-pin case: uniform noise and a noisy copy, from the shape's recorded seed."""
    import numpy as np
    rng = np.random.default_rng(L1_ORDER_SEEDS[shape] or 0)
    x = rng.random(shape, dtype=np.float32)
    y = np.clip(x + np.float32(0.15) * rng.standard_normal(shape, dtype=np.float32), 0, 1).astype(np.float32)
    return x, y


def l1_tile_order(x, y, order="wg.h"):
    """numpy emulation of the L1 half of scr_l1_ssim_forward on fp32 [C,H,W] arrays, operation by operation: per 16 x 16
    tile and channel thread ly * 16 + lx holds fabsf(x - y) in binary32 (0 outside the image); each of the 4 waves sums
    by the xor butterfly over 32 .. 1; the waves are added in ascending order; tile partial ((c * gy + by) * gx + bx);
    thread t of 1024 adds partials t, t + 1024, ... in binary64; the LDS tree over 512 .. 1; times 1 / (C H W), rounded
    once to binary32.  order: "wg.h" (the documented one), or a tile sum the kernel must NOT have -- "pairwise"
    ((w0 + w1) + (w2 + w3)) or "serial" (the 256 threads in ascending order)."""
    import numpy as np
    C, H, W = x.shape
    T = SSIM_TILE
    gy, gx = -(-H // T), -(-W // T)
    d = np.zeros((C, gy * T, gx * T), np.float32)
    d[:, :H, :W] = np.abs(x.astype(np.float32) - y.astype(np.float32))
    v = d.reshape(C, gy, T, gx, T).transpose(0, 1, 3, 2, 4).reshape(C * gy * gx, 4, 64)     # [tile, wave, lane]
    if order == "serial":
        part = np.add.accumulate(v.reshape(-1, 256), axis=1, dtype=np.float32)[:, -1]
    else:
        lane = np.arange(64)
        for s in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, lane ^ s]
        w = v[:, :, 0]
        part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3]) if order == "pairwise" else ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    assert part.dtype == np.float32
    rows = -(-part.size // SSIM_REDUCE)
    rec = np.zeros(rows * SSIM_REDUCE, np.float64)
    rec[:part.size] = part
    a = np.zeros(SSIM_REDUCE, np.float64)
    for r in rec.reshape(rows, SSIM_REDUCE):
        a = a + r
    s = SSIM_REDUCE // 2
    while s > 0:
        a[:s] = a[:s] + a[s:2 * s]
        s //= 2
    return np.float32(a[0] * (1.0 / (float(C) * H * W)))


def ssim_dx_floor(up, n):
    """Floor of the scale d x is measured against: (|g_l1| + |g_ssim|) / n, the size of a gradient that is not there.
    On identical images the true gradient is 1e-16 and a ratio to it is noise over nothing."""
    return sum(abs(g) for g in up if g is not None) / n


# Cases whose image rows take the same floor under their own scale; every other case keeps the module's rule (a row's
# scale floored at 1e-3 of the tensor's).  On `identical` d x = x (2 G*dE11 + G*dE12) with the two terms
# +-2 x G*(1 / B2) = +-12 / n cancelling, so correct fp32 leaves 6e-7 of the floor in every row, which the module's
# rule reports as 6e-4: the exact restatement 5.7e-4 against 1.5 x 3.0e-4 of the chain, a coin toss between two noises.
# No image with y = x avoids it (the terms scale with x / B2), so the case cannot be changed to meet the rule.  A wrong
# halo or index moves a row by 1e-3 .. 1 of the floor (test_f64_refs_host.py), fifty times the bar and more.
SSIM_ROW_FLOOR_CASES = ("identical",)


def ssim_row_floor(name, up, n):
    return ssim_dx_floor(up, n) if name in SSIM_ROW_FLOOR_CASES else None


def ssim_figures(got, ref, finite=None):
    """{L1, SSIM, dx, dx rows: e} of (L1, SSIM, dx) triples; `ref` carries the floor of dx's scale as a fourth entry and
    that of its rows' scale (or None) as a fifth.
    finite: bool [C,H,W], the elements of dx that take part (the others are compared as sets by the caller)."""
    gd, rd = _f64(got[2]), _f64(ref[2])
    if finite is not None:
        gd, rd = torch.where(finite, gd, torch.zeros(())), torch.where(finite, rd, torch.zeros(()))
    W = rd.shape[-1]
    return {"L1": err(got[0], ref[0]), "SSIM": err(got[1], ref[1]), "dx": err(gd, rd, scale_floor=ref[3]),
            "dx rows": err(gd.reshape(-1, W), rd.reshape(-1, W), rows=True, scale_floor=ref[3], row_floor=ref[4])}


# scaling regulariser: rows per workgroup 2048, so the last two sizes give 1024 and 1025 partials
SREG_P = [1, 255, 256, 257, 2047, 2048, 2049, 2_097_152, 2_097_153]
SREG_EDGE_ROWS = [(0.0, 0.7, 1.3), (0.0, 0.0, 0.4), (0.0, 0.0, 0.0), (-0.5, 0.7, 1.2), (1e-20, 1e-20, 1.0)]
SREG_ZERO_ROWS = 3                                                    # the first three edge rows hold a zero


def sreg_inputs(P):
    """fp32 CPU scaling [P,3]: uniform in [0.01, 2], the first min(P, 5) rows the edge rows."""
    g = torch.Generator().manual_seed(P)
    s = 0.01 + 1.99 * torch.rand(P, 3, generator=g)
    k = min(P, len(SREG_EDGE_ROWS))
    s[:k] = torch.tensor(SREG_EDGE_ROWS[:k])
    return s


# pair L1: 4096 elements per workgroup, so the last two sizes give 1024 and 1025 partials
PAIR_N = [1, 4095, 4096, 4097, 4_194_304, 4_194_305]
PAIR_ZERO_STRIDE = 53                                                # the column 0 of the (3, 37, 53) case, flattened


def pair_inputs(n):
    """fp32 CPU (gen1, gen2, real1, real2) of n elements; every 53rd residual (real1 - real2) - (gen1 - gen2) is at or
    next to zero, as column 0 of test_fused_pair_l1_matches_the_reference_ops."""
    g = torch.Generator().manual_seed(n)
    r1, r2, a0, b0 = (torch.rand(n, generator=g) for _ in range(4))
    z = slice(0, None, PAIR_ZERO_STRIDE)
    b0[z] = a0[z] - (r1[z] - r2[z])
    return a0, b0, r1, r2


# ---------------------------------------------------------------------------------------------------------- anchor gather
# csrc/anchor_gather.hip: the forward owns 64 rows of the OUTPUT per tile, 8 tiles and one statistics row per workgroup; the
# backward owns 64 consecutive ANCHORS per block, whose visible ones own consecutive upstream rows fv .. fv + nv - 1.  Every
# upstream chunk is loaded as 16-byte pieces from the aligned address below it (h = fv * width mod 4 floats in front), without
# a guard while fv + nv + 1 < V and element by element otherwise.
AG_ROWS, AG_TPW, AG_COLS, AG_LD, AG_DP = 64, 8, 71, 72, 80
AG_PARTS = (("feat", 0, 32), ("anchor", 32, 3), ("offsets", 35, 30), ("scaling", 65, 6))       # name, first column, width
AG_U = 2.0 ** -24
GATHER_BWD_TOL, GATHER_DX_TOL = 4 * AG_U, 40 * AG_U
GATHER_STAT_TOL = AG_ROWS * AG_TPW * AG_U                            # an fp32 sum of at most 512 terms per partial, any order
GATHER_EXP_FLOOR = 2.0 ** -23
GATHER_FWD_V = {"fwd511": 511, "fwd512": 512, "fwd513": 513, "fwd1025": 1025}
GATHER_STAT_ROWS = {"fwd511": 1, "fwd512": 1, "fwd513": 2, "fwd1025": 3}
GATHER_TAIL_FRONT = 3                                                # blocks in front of tail_edge's last 3 * 64 + 1 anchors
GATHER_MIXED_SEED = 2                # the lowest for which the blocks' h takes every value (test_f64_refs_host.py asserts it)
GATHER_CASES = ("one", "one_hidden", "b63", "b64", "b65", "b129", "only_last", "only_first", "hole", "tail_edge", "mixed",
                *GATHER_FWD_V)
GATHER_BWD_CASES = tuple(c for c in GATHER_CASES if c not in GATHER_FWD_V)
GATHER_DX_CASES = ("b65", "hole", "tail_edge", "mixed")
GATHER_SUB_CASES = ("mixed", "tail_edge")
GATHER_UP = ("feat", "anchor", "offsets", "scaling", "g_fea")        # the five upstream gradients
GATHER_FAULTS = ("no_xk1_col3", "first_v_plus_1", "no_exp")


def gather_mask(case):
    """bool [N]: the visible anchors of a case."""
    full = {"one": 1, "b63": 63, "b64": 64, "b65": 65, "b129": 129}
    if case in full:
        return torch.ones(full[case], dtype=torch.bool)
    if case == "one_hidden":
        return torch.zeros(1, dtype=torch.bool)
    g = torch.Generator().manual_seed(GATHER_CASES.index(case) + 7 + (GATHER_MIXED_SEED if case == "mixed" else 0))
    if case in ("only_last", "only_first"):
        m = torch.zeros(200, dtype=torch.bool)
        m[199 if case == "only_last" else 0] = True
        return m
    if case == "hole":
        m = torch.rand(256, generator=g) < 0.7
        m[64:128] = False
        return m
    if case == "tail_edge":
        f = GATHER_TAIL_FRONT * AG_ROWS
        m = torch.zeros(f + 3 * AG_ROWS + 1, dtype=torch.bool)
        m[:f] = torch.rand(f, generator=g) < 0.7
        m[f + 17] = m[f + AG_ROWS + 63] = m[f + 3 * AG_ROWS] = True      # alone in their blocks; the third block is empty
        return m
    if case == "mixed":
        return torch.rand(AG_ROWS * 9 + 7, generator=g) < 0.5
    V = GATHER_FWD_V[case]
    m = torch.zeros(V + V // 3, dtype=torch.bool)
    m[torch.randperm(m.numel(), generator=g)[:V]] = True
    return m


def gather_blocks(inv, V, n0=0, n1=None):
    """What the backward kernel derives per block of 64 anchors, from `inv` alone: dict(fv, nv, h {width: floats between
    the 16-byte boundary below the chunk and the chunk}, path: "none" (nv = 0), "vector" (unguarded 16-byte loads) or
    "tail" (element-wise, guarded))."""
    n1 = inv.numel() if n1 is None else n1
    out = []
    for b0 in range(n0, n1, AG_ROWS):
        rows = inv[b0:min(b0 + AG_ROWS, n1)]
        vis = rows[rows >= 0]
        nv = int(vis.numel())
        fv = int(vis[0]) if nv else -1
        assert not nv or torch.equal(vis, torch.arange(fv, fv + nv)), "the index list is not ascending"
        out.append(dict(fv=fv, nv=nv, h={w: (fv * w) % 4 if nv else None for w in (3, 6, 30, 32, 71, 72)},
                        path="none" if not nv else "vector" if fv + nv + 1 < V else "tail"))
    return out


def gather_stat_rows(V):
    return max(1, -(-V // (AG_ROWS * AG_TPW)))


def gather_inputs(case):
    """fp32 CPU inputs of one gather case: dict(N, V, mask, idx [V], inv [N] (row of every anchor, -1 = invisible), params
    (anchor_feat [N,32], anchor [N,3], offset [N,10,3], scaling [N,6]), up {name: upstream gradient; g_fea as [V,72] with
    a pad column the kernel must ignore}, coef [34,80] = Gi [32] | k0 | k1 with columns 71.. zero, dy [V,32], old (four
    buffers to accumulate into), blocks (gather_blocks)).  Scalings randn 0.3 - 3 and features randn 3 + 0.5 as in
    test_fused_anchor_gather_matches_the_torch_ops; upstreams and coefficients O(1)."""
    mask = gather_mask(case)
    N, idx = mask.numel(), mask.nonzero().view(-1)
    V = idx.numel()
    inv = torch.full((N,), -1, dtype=torch.long)
    inv[idx] = torch.arange(V)
    g = torch.Generator().manual_seed(1000 + GATHER_CASES.index(case))
    r = lambda *s: torch.randn(*s, generator=g)
    params = (r(N, 32) * 3 + 0.5, r(N, 3) * 2, r(N, 10, 3), r(N, 6) * 0.3 - 3)
    up = {"feat": r(V, 32), "anchor": r(V, 3), "offsets": r(V, 30), "scaling": r(V, 6), "g_fea": r(V, AG_LD)}
    coef = torch.zeros(34, AG_DP)
    coef[:, :AG_COLS] = r(34, AG_COLS)
    coef[:32] *= 0.3
    old = tuple(r(N, w) for _, _, w in AG_PARTS)
    return dict(case=case, N=N, V=V, mask=mask, idx=idx, inv=inv, params=params, up=up, coef=coef, dy=r(V, 32), old=old,
                blocks=gather_blocks(inv, V))


def gather_f64(idx, anchor_feat, anchor, offset, scaling):
    """The head of generate_neural_gaussians as the reference writes it: (feat [V,32], anchor [V,3], grid_offsets
    [V,10,3], grid_scaling [V,6] = exp(scaling)[idx], g_fea [V,71])."""
    feat, anc = anchor_feat.index_select(0, idx), anchor.index_select(0, idx)
    off, gs = offset.index_select(0, idx), torch.exp(scaling).index_select(0, idx)
    return feat, anc, off, gs, torch.cat((feat, anc, off.flatten(1), gs), dim=1)


def gather_stats_f64(g_fea):
    """Per column of the fp32 matrix g_fea [V, >= 71], in float64: (sum (x - x[0]), sum (x - x[0])^2, sum |x - x[0]|)."""
    x = _f64(g_fea)[:, :AG_COLS]
    t = x - x[0]
    return t.sum(dim=0), (t * t).sum(dim=0), t.abs().sum(dim=0)


def gather_stats_excess(stats, g_fea):
    """stats [rows, 2, 80]: the partial sums of disjoint row sets.  -> (excess of the two sums over GATHER_STAT_TOL times
    sum |x - x[0]| / sum (x - x[0])^2, 0 / 0 = 0; whether columns 71.. are exactly 0)."""
    s = _f64(stats).sum(dim=0)
    s1, s2, sa = gather_stats_f64(g_fea)
    worst = 0.0
    for got, ref, scale in ((s[0, :AG_COLS], s1, sa), (s[1, :AG_COLS], s2, s2)):
        dlt = (got - ref).abs()
        dlt = torch.where(torch.isnan(dlt), torch.full_like(dlt, float("inf")), dlt)
        worst = max(worst, float(torch.where(dlt == 0, torch.zeros_like(dlt), dlt / (GATHER_STAT_TOL * scale)).max()))
    return worst, bool((_f64(stats)[:, :, AG_COLS:] == 0).all())


def gather_dx_f64(coef, dy, x):
    """d g_fea [V,71] as the BatchNorm-Linear's backward ends: k0 + x k1 + dy Gi, coef = Gi [32][80] | k0 | k1."""
    c = coef[:, :AG_COLS]
    return c[32] + x[:, :AG_COLS] * c[33] + dy @ c[:32]


def gather_run(idx, params, up, dx=None):
    """Forward + backward of gather_f64 in the dtype / on the device of its arguments.  up: {name: gradient or None} of the
    five outputs (offsets as [V,30], g_fea with 71 or 72 columns: the pad is dropped); dx: a further gradient of g_fea
    [V,71].  -> (the five outputs, the gradients of the four parameters [N,32] / [N,3] / [N,10,3] / [N,6])."""
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    outs = gather_f64(idx, *ps)
    loss = outs[4].sum() * 0
    for name, o, w in zip(GATHER_UP, outs, (32, 3, 30, 6, AG_COLS)):
        u = up.get(name)
        if u is not None:
            loss = loss + (o.reshape(o.shape[0], w) * u[:, :w]).sum()
    if dx is not None:
        loss = loss + (outs[4] * dx).sum()
    loss.backward()
    return [o.detach() for o in outs], [p.grad for p in ps]


def gather_terms(d, up, dx=None, old=None, n0=0, n1=None):
    """Sum of the absolute values of every term that enters an element of the four gradients, d exp applied to the new
    ones: ((|d part| + |d g_fea| + dx's terms) exp(s), + |old| where the call accumulates).  float64, [n1 - n0, width]
    each; the bounds of the parity tests are multiples of 2^-24 of it.  dx: (coef, dy, x) -- 32 products, x k1 and k0."""
    f = lambda t: t.detach().to("cpu", torch.float64)
    V, N = d["V"], d["N"]
    n1 = N if n1 is None else n1
    A = torch.zeros(V, AG_COLS, dtype=torch.float64)
    if up.get("g_fea") is not None:
        A += f(up["g_fea"])[:, :AG_COLS].abs()
    for name, c0, w in AG_PARTS:
        if up.get(name) is not None:
            A[:, c0:c0 + w] += f(up[name]).abs()
    if dx is not None:
        coef, dy, x = (f(t) for t in dx)
        c = coef[:, :AG_COLS].abs()
        A += c[32] + x[:, :AG_COLS].abs() * c[33] + dy.abs() @ c[:32]
    A[:, 65:] *= torch.exp(f(d["params"][3]))[d["idx"]]
    full = torch.zeros(N, AG_COLS, dtype=torch.float64)
    full[d["idx"]] = A
    outs = [full[n0:n1, c0:c0 + w].clone() for _, c0, w in AG_PARTS]
    if old is not None:
        outs = [o + f(b).reshape(N, -1)[n0:n1].abs() for o, b in zip(outs, old)]
    return outs


def gather_restated_f32(d, up, dx=None, old=None, fault=None):
    """csrc/anchor_gather.hip's backward in plain fp32 torch on the CPU, in the kernel's order: the rows of dx (k0 + x k1,
    then the 32 products) or of d g_fea, the four parts added, (with dx: d g_fea added last,) times exp(s) as the forward
    left it, rows scattered to their anchors (zeros elsewhere), added to `old`.  -> the four gradients [N, width].
    fault: one of GATHER_FAULTS, a deliberate error --
      no_xk1_col3     the x k1 term is missing in columns 3, 7, .., 67 of dx
      first_v_plus_1  every block takes its upstream rows from first_v + 1 (the last row from itself)
      no_exp          d scaling without the factor exp(s)"""
    assert fault is None or fault in GATHER_FAULTS, fault
    V, N, idx = d["V"], d["N"], d["idx"]
    rows = torch.arange(V)
    if fault == "first_v_plus_1":
        rows = (rows + 1).clamp(max=max(V - 1, 0))
    g = lambda t: None if t is None else t.detach().float().cpu()[rows]
    T = torch.zeros(V, AG_COLS)
    gf = g(up.get("g_fea"))
    if dx is not None:
        coef, dy, x = dx[0].float()[:, :AG_COLS], g(dx[1]), g(dx[2])[:, :AG_COLS]
        k1 = coef[33].clone()
        xk1 = x * k1
        if fault == "no_xk1_col3":
            xk1[:, 3:68:4] = 0
        T = (coef[32] + xk1) + dy @ coef[:32]
    elif gf is not None:
        T = T + gf[:, :AG_COLS]
    for name, c0, w in AG_PARTS:
        if up.get(name) is not None:
            T[:, c0:c0 + w] += g(up[name])
    if dx is not None and gf is not None:
        T = T + gf[:, :AG_COLS]
    if fault != "no_exp":
        T[:, 65:] *= torch.exp(d["params"][3].float())[idx]
    full = torch.zeros(N, AG_COLS)
    full[idx] = T
    outs = [full[:, c0:c0 + w].clone() for _, c0, w in AG_PARTS]
    if old is not None:
        outs = [b.float().reshape(N, -1) + o for o, b in zip(outs, old)]
    return outs


def gather_excess(got, ref, terms, tol):
    """max over the four gradients of |got - ref| / (tol * terms), 0 / 0 = 0: at most 1 when every element is inside its
    bound.  An element whose terms are all zero (an invisible anchor, an absent upstream) must be exact."""
    worst = 0.0
    for a, b, s in zip(got, ref, terms):
        a, b = a.detach().to("cpu", torch.float64).reshape(s.shape), b.detach().to("cpu", torch.float64).reshape(s.shape)
        dlt = (a - b).abs()
        dlt = torch.where(torch.isnan(dlt), torch.full_like(dlt, float("inf")), dlt)
        ratio = torch.where(dlt == 0, torch.zeros_like(dlt), dlt / (tol * s))
        if ratio.numel():
            worst = max(worst, float(ratio.max()))
    return worst


GATHER_WRAPPER_N = (130, 2051)


def gather_wrapper_inputs(N):
    """fp32 CPU inputs of the wrapper check: dict(idx (80 % of N anchors), params, G [32,71], c [32], w (weights of the
    sum over y, feat, anchor, offsets, scaling))."""
    g = torch.Generator().manual_seed(N + 17)
    r = lambda *s: torch.randn(*s, generator=g)
    params = (r(N, 32) * 3 + 0.5, r(N, 3) * 2, r(N, 10, 3), r(N, 6) * 0.3 - 3)
    idx = (torch.rand(N, generator=g) < 0.8).nonzero().view(-1)
    V = idx.numel()
    return dict(idx=idx, params=params, G=r(32, 71) * 0.2, c=r(32), w=(r(V, 32), r(V, 32), r(V, 3), r(V, 10, 3), r(V, 6)))


def gather_norm_linear_run(idx, params, G, c, w, eps=1e-5):
    """gather_f64 -> BatchNorm1d in training mode (no affine part) folded into a Linear, y = xhat G^T + c -> the sum of
    y, feat, anchor, offsets and scaling weighted by w, in the dtype / on the device of its arguments.
    -> gradients of the four parameters, of G and of c."""
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    G, c = G.detach().clone().requires_grad_(True), c.detach().clone().requires_grad_(True)
    feat, anc, off, gs, x = gather_f64(idx, *ps)
    y = ((x - x.mean(dim=0)) / torch.sqrt(x.var(dim=0, unbiased=False) + eps)) @ G.T + c
    sum((o * u).sum() for o, u in zip((y, feat, anc, off, gs), w)).backward()
    return [p.grad for p in ps] + [G.grad, c.grad]
