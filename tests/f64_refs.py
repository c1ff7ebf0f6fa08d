"""Float64 references of the three anchor-path operators between the sampler and the rasterizer and of the image losses
behind it, and the inputs the parity tests feed them.  TEST INFRASTRUCTURE ONLY; nothing here imports the native library.

  heads_f64       the three Linear-ReLU-Linear heads on x = cat(feat, ob_view, geo_fea)      -> checker of csrc/mlp_heads.hip
  attention_f64   TriPlaneAttention + chunk + cat(plane, attended plane)                     -> checker of csrc/attention.hip
  expand_f64      torch_restatements.expand_torch_chain on double inputs                     -> checker of csrc/expand.hip
  ssim_f64        losses.l1_loss + losses.ssim in float64 (and the inputs of pair_l1 / scaling_reg) -> checker of csrc/ssim.hip
  gather_f64      the four visible-anchor gathers, exp and cat; gather_dx_f64 the fused dx         -> checker of csrc/anchor_gather.hip
  nl_*_f64        BatchNorm1d (batch statistics) folded into Linear(d, 32), launch by launch, and the parameter fold;
                  nl_*_bounds the a-priori bound of every output element                          -> checker of csrc/normlinear.hip

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


# ---------------------------------------------------------------------------------------------------------- norm-linear
# csrc/normlinear.hip at its own C ABI: BatchNorm1d (batch statistics) folded into Linear(d, 32).  Every launch is checked
# against float64 ON THAT LAUNCH'S OWN INPUTS (the forward GEMM takes the kernel's fp32 mean / inv as exact numbers, the dx
# pass the coefficient block it was handed), so every bound below is rounding alone plus one stated conditioning term.
# u = 2^-24; a bound is u times the number of fp32 operations on the longest chain into an element times the sum of the
# absolute values of the terms.  The chain lengths, read from the kernels:
NL_U = 2.0 ** -24
NL_OUT, NL_DP, NL_SLAB = 32, 80, 2048            # output features; padded coefficient rows; rows per statistics workgroup
NL_STAT_EXTRA = 3                                # an fp32 lane's x - shift, t * t and the rounding of its partial (nl_n_s's companion)
NL_STAT_COMBINE = 2                              # the kernel's statistics: nl_stats_partial_kernel subtracts, squares and adds in fp64
                                                 # and rounds a slab's two sums to fp32 once (1) + slack (1); a caller's col_stats are
                                                 # roundings of exact sums in the same way; nl_stats_finish_kernel adds them in fp64
NL_INV_ROUNDINGS = 2                             # 1 / sqrtf(vf + eps): the sum's rounding is halved by the root; the root and the division
                                                 # are correctly rounded (half an ulp each, at most u of the result)
NL_Y_EXTRA = 4                                   # G * inv, Gs * mean, c - acc, the accumulator's start: nl_stats_finish_kernel + nl_forward_kernel
NL_FINISH_TERMS = NL_OUT + 2                     # nl_bwd_finish_kernel: u and w are 32-term sums of two-factor products
NL_DX_TERMS = NL_OUT + 4                         # nl_bwd_dx_kernel: k0 + x k1 (2 roundings), 32 MFMA products, slack 2
NL_BWD_CAP, NL_BWD_LOW = 1024, 256               # nl_bwd_wgs: at most 1024 workgroups of 64 rows; never fewer resident than one per CU
NL_FWD_GRID_ROWS = 8 * 256 * 64                  # the most rows one round of nl_forward / nl_bwd_dx holds (8 workgroups x 256 CUs x 64)


def nl_cw(d):
    """Lanes per row of nl_stats_partial_kernel."""
    return 64 if d <= 64 else 128


def nl_n_s(d):
    """Terms a lane of nl_stats_partial_kernel adds one after the other (slab / RG rows) plus the RG groups it folds: the
    chain an fp32 lane would carry into a partial (nl_restated_f32 sums in fp32; the kernel's lanes in fp64, NL_STAT_COMBINE)."""
    rg = 256 // nl_cw(d)
    return NL_SLAB // rg + rg


def nl_slabs(V):
    return -(-V // NL_SLAB)


def nl_partials(V):
    """Workgroups (= partials) of nl_bwd_reduce_kernel when the chip holds them all: min(ceil(V / 64), 1024)."""
    return max(1, min(-(-V // 64), NL_BWD_CAP))


def nl_n_h(V):
    """Worst chain into an element of Hraw / sdy: (rows a wave walks) / 4 MFMA steps, 4 waves, partials / 8 per lane of
    nl_bwd_sum_kernel, its 8 groups (the 8 also covers the three roundings of (Hraw - sdy mean) inv in the finish kernel).
    The grid is min(nl_partials, what the chip holds): both ends are taken."""
    worst = 0
    for g in {nl_partials(V), min(nl_partials(V), NL_BWD_LOW)}:
        rows = -(-(-(-V // 16)) // (4 * g)) * 16
        worst = max(worst, rows // 4 + 4 + -(-g // 8) + 8)
    return worst


def nl_loop_forms(n, first, step):
    """{'unrolled', 'tail'}: the forms lane-group 0 of a `for (; i + first < n; i += step) ...; for (; i < n; ...)` pair runs."""
    forms, i = set(), 0
    while i + first < n:
        forms.add("unrolled")
        i += step
    if i < n:
        forms.add("tail")
    return forms


def nl_case_facts(V, d, ldx, off=0, lddx=None, dx_off=0, stat_rows=0):
    """What a call makes the kernels do, from its shapes alone: dict(Q (= NT), CW, aligned (forward), aligned_dx, slabs,
    partials, finish (loop forms of nl_stats_finish_kernel), slab_tail (loop forms the row groups of nl_stats_partial_kernel run on the
    last slab, together), strides (rounds of the forward / dx grid-stride loop)).  off / dx_off: floats between a 16-byte boundary and x / dx."""
    rg = 256 // nl_cw(d)
    al = ldx % 4 == 0 and off % 4 == 0
    nwg = stat_rows or nl_slabs(V)
    last = (V - 1) % NL_SLAB + 1                 # rows of the last slab; row group g of rg owns rows g, g + rg, ...
    return dict(Q=-(-d // 16), CW=nl_cw(d), aligned=al,
                aligned_dx=None if lddx is None else al and lddx % 4 == 0 and dx_off % 4 == 0,
                slabs=nl_slabs(V), partials=nl_partials(V), finish=nl_loop_forms(nwg, 56, 64),
                slab_tail=set().union(*(nl_loop_forms(max(0, -(-(last - g) // rg)), 7, 8) for g in range(rg))),
                strides=-(-V // NL_FWD_GRID_ROWS))


NL_LAYOUTS = ("packed", "padded", "block", "off1", "odd")


def _up4(n):
    return (n + 3) // 4 * 4


def nl_layout(t, layout, fill=float("nan")):
    """t [V,w] inside a `fill`-filled allocation on t's device -> (the flat leaf, the view, its row stride, floats from the
    leaf's 16-byte aligned start to the view).  packed: ld = w; padded: ld = roundup4(w); block: columns 4 .. 4 + w - 1 of a
    [V, roundup4(w) + 8] matrix (aligned, NaN on both sides); off1: columns 1 .. w of a [V, roundup4(w + 1)] matrix (stride a
    multiple of 4, rows 4-byte aligned only); odd: ld = w + 1 if that is odd, else w + 3 (never w itself; odd for an even
    w, and for w = 1 mod 4 a multiple of 4 with three pad columns)."""
    V, w = t.shape
    ld, off = {"packed": (w, 0), "padded": (_up4(w), 0), "block": (_up4(w) + 8, 4), "off1": (_up4(w + 1), 1),
               "odd": (w + 1 if (w + 1) % 2 else w + 3, 0)}[layout]
    leaf = torch.full((V * ld + 4,), fill, dtype=t.dtype, device=t.device)
    view = leaf[off:off + (V - 1) * ld + w].as_strided((V, w), (ld, 1))
    view.copy_(t)
    return leaf, view, ld, off


def nl_inputs(V, d, seed=0):
    """fp32 CPU inputs of one case: x [V,d] (the first d // 2 columns -5 +- 0.3, the log-scalings; the rest N(0,1)), G [32,d]
    (0.2 randn), c [32], dy [V,32] -- what test_fused_norm_linear_matches_batchnorm_linear_chain draws."""
    g = torch.Generator().manual_seed(V * 131 + d + 7919 * seed)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(V, d)
    x[:, : d // 2] = x[:, : d // 2] * 0.3 - 5.0
    return dict(V=V, d=d, x=x, G=r(NL_OUT, d) * 0.2, c=r(NL_OUT), dy=r(V, NL_OUT))


def nl_coef_block(d, seed, pad=float("nan")):
    """A free-standing coefficient block [34,80] = Gi [32] | k0 | k1, drawn (Gi 0.3 randn, k0 / k1 randn), columns d.. = pad."""
    g = torch.Generator().manual_seed(50_000 + 97 * d + seed)
    coef = torch.full((NL_OUT + 2, NL_DP), pad)
    coef[:, :d] = torch.randn(NL_OUT + 2, d, generator=g)
    coef[:NL_OUT, :d] *= 0.3
    return coef


NL_REGIME_COLUMNS = ("normal", "minus5", "constant", "1e4", "outlier_first", "alternating", "last_row_only", "row2048_only")
NL_REGIME_V = 4099


def nl_regime_matrix():
    """[4099,8] fp32, one column per statistics regime (NL_REGIME_COLUMNS)."""
    V = NL_REGIME_V
    g = torch.Generator().manual_seed(4099)
    r = lambda: torch.randn(V, generator=g)
    x = torch.zeros(V, 8)
    x[:, 0] = r()
    x[:, 1] = r() * 0.3 - 5.0
    x[:, 2] = 3.25
    x[:, 3] = r() * 1e-2 + 1e4
    x[:, 4] = r()
    x[0, 4] = 1e3                                                      # the shift is a thousand deviations from the mean
    x[:, 5] = 1.0 - 2.0 * (torch.arange(V) % 2)
    x[V - 1, 6] = 1.0
    x[NL_SLAB, 7] = 1.0
    return x


def nl_col_stats(x, rows, seed=0):
    """[rows,2,80] fp32: roundings of the float64 sums of (x - x[0]) and (x - x[0])^2 over a seeded random partition of the
    rows of x into `rows` non-empty disjoint sets; columns d.. are 0."""
    V, d = x.shape
    assert 1 <= rows <= V
    g = torch.Generator().manual_seed(rows * 1009 + V + seed)
    owner = torch.cat([torch.arange(rows), torch.randint(0, rows, (V - rows,), generator=g)])[torch.randperm(V, generator=g)]
    t = _f64(x) - _f64(x)[0]
    st = torch.zeros(rows, 2, NL_DP, dtype=torch.float64)
    st[:, 0, :d].index_add_(0, owner, t)
    st[:, 1, :d].index_add_(0, owner, t * t)
    return st.float()


# ---- references (dtype-agnostic op chains)
def nl_stats_f64(x):
    """(mean, biased variance) per column."""
    m = x.mean(dim=0)
    return m, ((x - m) ** 2).mean(dim=0)


def nl_forward_f64(x, G, c, mean, inv):
    return ((x - mean) * inv) @ G.T + c


def nl_backward_f64(x, dy, G, mean, inv):
    """(dG, dc, Gi, k0, k1) by the algebra in csrc/normlinear.hip's header: dG = (dy^T x - sdy mean^T) inv, dc = sdy,
    u = G^T sdy, w = sum_m G dG, k1 = -inv^2 w / V, k0 = -inv u / V - mean k1, Gi = G inv."""
    V = x.shape[0]
    sdy = dy.sum(dim=0)
    dG = (dy.T @ x - sdy[:, None] * mean) * inv
    u, w = G.T @ sdy, (G * dG).sum(dim=0)
    k1 = -(inv * inv) * w / V
    return dG, sdy, G * inv, -inv * u / V - mean * k1, k1


def nl_dx_f64(x, dy, Gi, k0, k1):
    return k0 + x * k1 + dy @ Gi


def nl_fold_f64(W, b, gamma, beta, widths, cols, d, col_at=None):
    """(G [32,d], c [32]) of sum_i Linear_i(BatchNorm_i(.)) as scene_model._norm_linear's non-device branch folds them:
    G_ref[:, cols_i + j] += W_i[:, j] gamma_i[j], c = sum_i (W_i beta_i + b_i); col_at: G[:, col_at[j]] = G_ref[:, j]."""
    G = torch.zeros(NL_OUT, d, dtype=W[0].dtype)
    for Wi, gi, c0, w in zip(W, gamma, cols, widths):
        G[:, c0:c0 + w] = G[:, c0:c0 + w] + Wi * gi
    c = sum(Wi @ bi + b_ for Wi, bi, b_ in zip(W, beta, b))
    if col_at is not None:
        G = torch.zeros_like(G).index_copy(1, torch.as_tensor(list(col_at), dtype=torch.long), G)
    return G, c


def nl_fold_backward_f64(dG, dc, W, gamma, beta, widths, cols, col_at=None, apply_at=True):
    """[(dW_i, db_i, dgamma_i, dbeta_i)]: dW_i = dG_ref[:, block i] gamma_i + dc beta_i^T, db_i = dc, dgamma_i = sum_r
    dG_ref W_i, dbeta_i = W_i^T dc, with dG_ref[:, j] = dG[:, col_at[j]].  apply_at=False: the planted fault (dG read as it lies)."""
    if col_at is not None and apply_at:
        dG = dG.index_select(1, torch.as_tensor(list(col_at), dtype=torch.long))
    out = []
    for Wi, gi, bi, c0, w in zip(W, gamma, beta, cols, widths):
        blk = dG[:, c0:c0 + w]
        out.append((blk * gi + dc[:, None] * bi, dc.clone(), (blk * Wi).sum(dim=0), Wi.T @ dc))
    return out


def nl_running_f64(run_mean, run_var, momentum, mean, var, n, widths, cols, col_at=None, unbiased=True):
    """[(running_mean_i, running_var_i)] after nn.BatchNorm1d's update: (1 - m) old + m new, the variance times n / (n - 1)
    (n = 1: times 1).  unbiased=False: the planted fault n / n."""
    if col_at is not None:
        at = torch.as_tensor(list(col_at), dtype=torch.long)
        mean, var = mean.index_select(0, at), var.index_select(0, at)
    f = n / max(n - 1, 1) if unbiased else 1.0
    return [(rm * (1 - m) + m * mean[c0:c0 + w], rv * (1 - m) + m * (var[c0:c0 + w] * f))
            for rm, rv, m, c0, w in zip(run_mean, run_var, momentum, cols, widths)]


# ---- a-priori bounds, per element, float64, from the inputs alone
def nl_excess(got, ref, bound):
    """max |got - ref| / bound over the elements, 0 / 0 = 0, NaN = inf: at most 1 when every element is inside its bound."""
    got, ref, bound = _f64(got), _f64(ref), _f64(bound)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.numel() == 0:
        return 0.0
    dlt = (got - ref).abs()
    dlt = torch.where(torch.isnan(dlt), torch.full_like(dlt, float("inf")), dlt)
    return float(torch.where(dlt == 0, torch.zeros_like(dlt), dlt / bound).max())


def nl_stats_bounds(x, eps, n_s):
    """{'mean' | 'var' | 'inv': (float64 reference, bound)} of the shifted one-pass statistics of the fp32 matrix x, shift
    x0 = x[0], n_s fp32 terms per partial sum (NL_STAT_COMBINE for the kernel on either path: its lanes sum in fp64; nl_n_s(d)
    for sums formed in fp32, f64_refs.nl_restated_f32):
      shifted mean m = mean - x0:  bm = (n_s + 3) u mean_v |x - x0|;   mean = fl(x0 + m):  bm + u |mean|
      var = E t^2 - m^2:           (n_s + 3) u (var + m^2) + 2 |m| bm + bm^2 + u var
    var + m^2 = E t^2 is the CONDITIONING of a shifted one-pass variance: the rounding of the raw second moment stays when
    m^2 is taken off, so a shift |m| / sigma deviations from the mean costs (|m| / sigma)^2 in relative accuracy.
    (2 |m| bm, not 2 |m| times the whole mean bound: the variance is formed from m before x0 is added and rounded.)
      inv = 1 / sqrt(var + eps):   the interval [var - b, var + b] mapped through it, plus 2 u inv (the addition of eps -- half of its
                                   error passes the root --, the correctly rounded root and division)"""
    x = _f64(x)
    eps = float(torch.tensor(eps, dtype=torch.float32))
    mean, var = nl_stats_f64(x)
    t = x - x[0]
    m = mean - x[0]
    k = (n_s + NL_STAT_EXTRA) * NL_U
    bm = k * t.abs().mean(dim=0)
    bv = k * (var + m * m) + 2 * m.abs() * bm + bm * bm + NL_U * var
    inv = 1.0 / torch.sqrt(var + eps)
    hi, lo = 1.0 / torch.sqrt((var - bv).clamp_min(0) + eps), 1.0 / torch.sqrt(var + bv + eps)
    return {"mean": (mean, bm + NL_U * mean.abs()), "var": (var, bv),
            "inv": (inv, torch.maximum(hi - inv, inv - lo) + NL_INV_ROUNDINGS * NL_U * hi)}


def nl_y_bound(x, G, c, mean, inv):
    """(d + 4) u (sum_n |G_mn inv_n| (|x_vn| + |mean_n|) + |c_m|)  [V,32]; d products each in the bias and in the GEMM."""
    x, G, c, mean, inv = (_f64(t) for t in (x, G, c, mean, inv))
    Ga = (G * inv).abs()
    return (x.shape[1] + NL_Y_EXTRA) * NL_U * (x.abs() @ Ga.T + Ga @ mean.abs() + c.abs())


def nl_backward_bounds(x, dy, G, mean, inv):
    """{'dG' | 'dc' | 'Gi' | 'k0' | 'k1': (reference, bound)}: dc and the raw moment with N_H = nl_n_h(V) terms,
      dc: N_H u sum_v |dy_vm|;   dG: inv_n N_H u (sum_v |dy_vm x_vn| + |mean_n| sum_v |dy_vm|)
    (the raw moment dy^T x is centred only afterwards: sum_v |dy x| stands where a centred sum would have sum_v |dy (x - mean)|
    -- the conditioning term of this pass), and the finish kernel's 32-term sums over them:
      u: sum_m |G| b_dc + 34 u sum_m |G sdy|;  w: sum_m |G| b_dG + 34 u sum_m |G dG|
      k1: inv^2 b_w / V + 4 u |k1|;  k0: inv b_u / V + |mean| b_k1 + 4 u (|inv u / V| + |mean k1|);  Gi: u |Gi|"""
    x, dy, G, mean, inv = (_f64(t) for t in (x, dy, G, mean, inv))
    V = x.shape[0]
    dG, dc, Gi, k0, k1 = nl_backward_f64(x, dy, G, mean, inv)
    nh = nl_n_h(V) * NL_U
    sa = dy.abs().sum(dim=0)
    b_dc = nh * sa
    b_dG = inv * nh * (dy.abs().T @ x.abs() + sa[:, None] * mean.abs())
    ft = NL_FINISH_TERMS * NL_U
    b_u = G.abs().T @ b_dc + ft * (G.abs().T @ dc.abs())
    b_w = (G.abs() * b_dG).sum(dim=0) + ft * (G * dG).abs().sum(dim=0)
    b_k1 = inv * inv * b_w / V + 4 * NL_U * k1.abs()
    b_k0 = inv * b_u / V + mean.abs() * b_k1 + 4 * NL_U * ((inv * (G.T @ dc) / V).abs() + (mean * k1).abs())
    return {"dG": (dG, b_dG), "dc": (dc, b_dc), "Gi": (Gi, NL_U * Gi.abs()), "k0": (k0, b_k0), "k1": (k1, b_k1)}


def nl_dx_bound(x, dy, Gi, k0, k1):
    """36 u (|k0| + |x k1| + sum_m |dy_vm Gi_mn|)  [V,d]."""
    x, dy, Gi, k0, k1 = (_f64(t) for t in (x, dy, Gi, k0, k1))
    return NL_DX_TERMS * NL_U * (k0.abs() + x.abs() * k1.abs() + dy.abs() @ Gi.abs())


def nl_forward_figures(x, G, c, eps, y, mean, var, inv, n_s):
    """[(name, |got - ref| / bound)] of one forward launch's four outputs (fp32 tensors on any device)."""
    sb = nl_stats_bounds(x, eps, n_s)
    out = [(n, nl_excess(t, *sb[n])) for n, t in (("mean", mean), ("var", var), ("inv", inv))]
    y64 = nl_forward_f64(_f64(x), _f64(G), _f64(c), _f64(mean), _f64(inv))
    return out + [("y", nl_excess(y, y64, nl_y_bound(x, G, c, mean, inv)))]


def nl_backward_figures(x, dy, G, mean, inv, dG, dc, coef):
    """[(name, excess)] of dG, dc and, with a coefficient block [34,80], of Gi / k0 / k1."""
    bb = nl_backward_bounds(x, dy, G, mean, inv)
    d = x.shape[1]
    out = [("dG", nl_excess(dG, *bb["dG"])), ("dc", nl_excess(dc, *bb["dc"]))]
    if coef is not None:
        out += [("Gi", nl_excess(coef[:NL_OUT, :d], *bb["Gi"])), ("k0", nl_excess(coef[NL_OUT, :d], *bb["k0"])),
                ("k1", nl_excess(coef[NL_OUT + 1, :d], *bb["k1"]))]
    return out


def nl_dx_figures(x, dy, coef, dx, rows=()):
    """[('dx', excess over all elements)] + [('dx row r', excess of that row)]: the block's values taken as exact."""
    d = x.shape[1]
    Gi, k0, k1 = coef[:NL_OUT, :d], coef[NL_OUT, :d], coef[NL_OUT + 1, :d]
    ref, b = nl_dx_f64(_f64(x), _f64(dy), _f64(Gi), _f64(k0), _f64(k1)), nl_dx_bound(x, dy, Gi, k0, k1)
    return [("dx", nl_excess(dx, ref, b))] + [(f"dx row {r}", nl_excess(dx[r], ref[r], b[r])) for r in rows]


NL_FAULTS = ("stats_drop_last_row", "pad_column_read", "k1_without_inv2", "dG_without_sdy_mean", "fold_bwd_ignores_at",
             "unbias_n_over_n")


def nl_restated_f32(x, G, c, dy, eps, fault=None, pad=None, col_stats=None, lanes="fp32"):
    """csrc/normlinear.hip's three launches in plain fp32 torch on the CPU, the same formulas in torch's own summation
    order: shifted sums per 2048-row slab combined in float64 (or the caller's col_stats), Gs = G inv and the folded bias
    c - Gs mean, the raw moment dy^T x centred afterwards, the finish algebra, dx = (k0 + x k1) + dy Gi.
    lanes: "fp32" -- the slab sums formed in fp32 (bound: nl_n_s(d) terms); "fp64" -- as nl_stats_partial_kernel forms them:
    difference, square and sums in float64, a slab's two sums rounded to fp32 once (bound: NL_STAT_COMBINE).
    -> dict(mean, var, inv, y, dG, dc, coef [34,80] (pads 0), dx).  pad: [V] fp32, the column behind x's last one in memory
    (only the fault reads it).  fault: one of NL_FAULTS[:4], a deliberate error --
      stats_drop_last_row   the statistics sums stop one row early (still divided by V)
      pad_column_read       the forward contraction runs over d + 1 columns: x's pad times the weight of column 0
      k1_without_inv2       k1 = -w / V
      dG_without_sdy_mean   dG = Hraw inv"""
    assert fault is None or fault in NL_FAULTS[:4], fault
    x, G, c, dy = (t.detach().float().cpu() for t in (x, G, c, dy))
    V, d = x.shape
    if col_stats is None:
        assert lanes in ("fp32", "fp64"), lanes
        t = x - x[0] if lanes == "fp32" else x.double() - x[0].double()
        if fault == "stats_drop_last_row":
            t = t[:V - 1]
        parts = [torch.stack((s.sum(dim=0), (s * s).sum(dim=0))) for s in t.split(NL_SLAB)]
        st = torch.stack(parts).float().double().sum(dim=0) if parts else torch.zeros(2, d, dtype=torch.float64)
    else:
        st = col_stats.double().sum(dim=0)[:, :d]
    m = st[0] / V
    v = (st[1] / V - m * m).clamp_min(0)
    mean, var = (x[0].double() + m).float(), v.float()
    inv = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    Gs = G * inv
    cb = c - (Gs * mean).sum(dim=1)
    y = x @ Gs.T + cb
    if fault == "pad_column_read":
        y = y + pad.float()[:, None] * Gs[:, 0]
    sdy = dy.sum(dim=0)
    h = dy.T @ x
    dG = (h if fault == "dG_without_sdy_mean" else h - sdy[:, None] * mean) * inv
    u, w = (G * sdy[:, None]).sum(dim=0), (G * dG).sum(dim=0)
    k1 = -w / V if fault == "k1_without_inv2" else -(inv * inv) * w / V
    k0 = -inv * u / V - mean * k1
    coef = torch.zeros(NL_OUT + 2, NL_DP)
    coef[:NL_OUT, :d], coef[NL_OUT, :d], coef[NL_OUT + 1, :d] = Gs, k0, k1
    return dict(mean=mean, var=var, inv=inv, y=y, dG=dG, dc=sdy, coef=coef, dx=(k0 + x * k1) + dy @ Gs)


# ---- the parameter fold
# (name, d, widths, cols, col_at kind): L = 1; 4 pairs on the whole input; 4 blocks side by side; 3 blocks under a column map
NL_FOLD_CASES = (("L1_w80", 80, (80,), (0,), None), ("L4_shared71", 71, (71,) * 4, (0,) * 4, None),
                 ("L4_blocks", 60, (1, 30, 15, 14), (0, 1, 31, 46), None),
                 ("L3_planes", 60, (30, 15, 15), (0, 30, 45), "planes"), ("L3_random", 60, (30, 15, 15), (0, 30, 45), "random"))


def nl_fold_col_at(kind, d=60, r=5):
    """None, the interleaving FeaturePlanes._sample_all gives two same-size grids sampled as one (r channels: grid 0's plane q
    at 3 r q .., grid 1's behind it) followed by the identity, or a seeded random permutation."""
    if kind is None:
        return None
    if kind == "random":
        return [int(v) for v in torch.randperm(d, generator=torch.Generator().manual_seed(d))]
    at = [(j // (2 * r)) * 3 * r + j % (2 * r) for j in range(6 * r)] + [q * 3 * r + 2 * r + k for q in range(3) for k in range(r)]
    return at + list(range(len(at), d))


def nl_fold_inputs(name):
    """fp32 CPU inputs of one fold case: dict(d, widths, cols, col_at, W, b, gamma, beta, dG, dc, run_mean, run_var,
    momentum, mean, var)."""
    _, d, widths, cols, kind = NL_FOLD_CASES[[c[0] for c in NL_FOLD_CASES].index(name)]
    g = torch.Generator().manual_seed(len(name) * 1000 + d)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(d=d, widths=widths, cols=cols, col_at=nl_fold_col_at(kind, d),
                W=[r(NL_OUT, w) * 0.3 for w in widths], b=[r(NL_OUT) for _ in widths], gamma=[1 + 0.2 * r(w) for w in widths],
                beta=[0.3 * r(w) for w in widths], dG=r(NL_OUT, d), dc=r(NL_OUT), run_mean=[r(w) for w in widths],
                run_var=[r(w).abs() + 0.5 for w in widths], momentum=[0.1, 0.25, 0.5, 1.0][:len(widths)], mean=r(d),
                var=r(d).abs() + 0.1)


def nl_fold_bounds(p):
    """(G, c) bounds: (L + 2) u sum_i |W gamma| per element of G (placed by col_at); (sum_i d_i + L) u (sum |W beta| + |b|)."""
    W, ga, be, b = ([_f64(t).abs() for t in p[k]] for k in ("W", "gamma", "beta", "b"))
    L = len(W)
    bG, bc = nl_fold_f64(W, b, ga, be, p["widths"], p["cols"], p["d"], p["col_at"])
    return (L + 2) * NL_U * bG, (sum(p["widths"]) + L) * NL_U * bc


def nl_fold_backward_bounds(p):
    """[(b dW, b db = 0, b dgamma, b dbeta)] per pair: 3 u (|dG gamma| + |dc beta|); 34-term column sums."""
    a = lambda k: [_f64(t).abs() for t in p[k]]
    terms = nl_fold_backward_f64(_f64(p["dG"]).abs(), _f64(p["dc"]).abs(), a("W"), a("gamma"), a("beta"), p["widths"], p["cols"],
                                 p["col_at"])
    ft = NL_FINISH_TERMS * NL_U
    return [(3 * NL_U * t[0], 0 * t[1], ft * t[2], ft * t[3]) for t in terms]


def nl_running_bounds(p, n):
    """6 u ((1 - m) |old| + m |new|) per element: 1 - m, two products, the sum, the unbias factor and its rounding."""
    a = lambda k: [_f64(t).abs() for t in p[k]]
    terms = nl_running_f64(a("run_mean"), a("run_var"), p["momentum"], _f64(p["mean"]).abs(), _f64(p["var"]).abs(), n,
                           p["widths"], p["cols"], p["col_at"])
    return [(6 * NL_U * t[0], 6 * NL_U * t[1]) for t in terms]


# ---- the cases of tests/test_gpu_f64_parity.py (shapes alone; tests/test_f64_refs_host.py asserts what each reaches)
NL_ROW_DL = ((60, 60), (71, 72))
NL_ROW_V = (1, 2, 15, 16, 17, 63, 64, 65, 129, 448, 512, 513, 1025)
NL_COL_V, NL_COL_D = 193, (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 71, 79, 80)
NL_GRAD_D, NL_GRAD_LDDY, NL_GRAD_X = (17, 60, 71), (32, 36, 64), ("padded", "off1")
NL_STRIDE_CASES = ((70_001, 60, 60), (140_001, 60, 60), (140_001, 71, 72))
NL_SLAB_DL = ((7, 7), (71, 72))
NL_SLAB_V = (2047, 2048, 2049, 2048 + 15, 2048 + 16, 2048 + 17, 2048 + 31, 2048 + 32, 2048 + 33, 8 * 2048 + 1)
NL_SLAB_CASES = tuple((V, d, ld) for d, ld in NL_SLAB_DL for V in NL_SLAB_V) + ((64 * 2048 + 1, 7, 7),)
NL_COLSTAT_V, NL_COLSTAT_ROWS = 4099, (1, 7, 8, 9, 56, 57, 58, 64, 65, 121, 2048)
NL_EPS = (1e-5, 1e-3)


def nl_lddx(d):
    return (d, _up4(d), _up4(d) + 4)
