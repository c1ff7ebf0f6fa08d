"""The float64 references of tests/f64_refs.py, checked on the CPU: they reproduce the golden fixtures captured from
the reference's own Python, they are differentiable where the parity tests differentiate them, a tied pool maximum
belongs to its first pixel, and the inputs of every GPU case stay inside the caps on replaced / excluded elements.  For the
image losses: correct fp32 arithmetic (a restatement of csrc/ssim.hip's, and the framework chain) meets the bars of the GPU
test on every case, and six deliberately wrong restatements each miss them on the cases chosen to see them."""
import functools
import os

import numpy as np
import pytest
import torch

import f64_refs as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _npz(name):
    return np.load(os.path.join(GOLD, name))


def test_heads_and_expansion_references_reproduce_the_golden_anchor_path():
    """neural_gaussians.npz (level 0, training): heads_f64 on the fixture's anchors gives its neural_opacity, expand_f64
    on the heads' outputs its mask, xyz, color, opacity, scaling and rot -- to the bars of
    test_host_golden.test_generate_neural_gaussians."""
    from test_host_golden import _model_from_fixture
    d = _npz("neural_gaussians.npz")
    pc = _model_from_fixture(d)
    pc.feat_planes._feat.activate_level = 0
    pc.train(True)
    cam = torch.tensor(d["camera_center"])
    with torch.no_grad():
        idx = torch.tensor(d["visible_mask"]).nonzero().squeeze(1)
        feat, anchor = pc._anchor_feat.index_select(0, idx), pc.get_anchor.index_select(0, idx)
        offsets, scaling = pc._offset.index_select(0, idx), pc.get_scaling.index_select(0, idx)
        V, k = anchor.shape[0], pc.n_offsets
        g_fea = torch.concat((feat, anchor, offsets.reshape(V, -1), scaling), dim=1)
        geo = pc.feat_planes.inference(anchor, g_fea, 0)
        (o, c, v), _, _ = R.heads_f64(feat.double(), anchor.double(), cam.double(), geo.double(), R.weights_of(pc))
        no, color, sr = o.reshape(-1, 1), c.reshape(V * k, 3), v.reshape(V * k, 7)
        res = R.expand_f64(no, color, sr, offsets.double(), scaling.double(), anchor.double(), k)
    np.testing.assert_allclose(no.numpy(), d["L0_train.neural_opacity"], rtol=2e-5, atol=2e-6)
    np.testing.assert_array_equal(res[5].numpy(), d["L0_train.mask"])
    for n, t in zip(["xyz", "color", "opacity", "scaling", "rot"], res):
        assert tuple(t.shape) == d[f"L0_train.{n}"].shape, n
        np.testing.assert_allclose(t.numpy(), d[f"L0_train.{n}"], rtol=2e-5, atol=2e-6, err_msg=n)


def test_attention_reference_reproduces_the_golden_plane_grid():
    """planegrid.npz (`ta`): PlaneGrid in float64 with attention_f64 in the place of its attention module gives the
    fixture's samples, to the bars of test_host_golden.test_planegrid."""
    from test_host_golden import _load_prefixed
    from splatco_amd.scene_model import PlaneGrid
    d = _npz("planegrid.npz")
    pg = PlaneGrid(15, [24, 24, 24], [-2.0, -2.0, -2.0], [2.0, 2.0, 2.0], TAflag=True)
    _load_prefixed(pg, d, "ta.")
    ws = R.attention_weights(pg.TA)
    pg = pg.double()

    class RefTA(torch.nn.Module):
        def forward(self, x):
            pairs, _ = R.attention_f64(list(torch.chunk(x, 3, dim=1)), *ws)
            return torch.cat([p[:, p.shape[1] // 2:] for p in pairs], dim=1)
    pg.TA = RefTA()
    with torch.no_grad():
        y = pg(torch.tensor(d["xyz"]).double(), 0)
    assert y.shape == (1000, 30)
    np.testing.assert_allclose(y.numpy(), d["ta.out"], rtol=1e-5, atol=1e-6)


def test_references_pass_gradcheck():
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    pc = R.heads_weights(3)
    w = R.weights_of(pc, requires_grad=True)
    flat = w["w1"] + w["b1"] + w["w2"] + w["b2"]
    feat, anchor, geo, cam = r(3, 32).requires_grad_(), (r(3, 3) * 2).requires_grad_(), r(3, 64).requires_grad_(), r(3)
    assert not R.heads_undecided(feat, anchor, cam, geo, R.weights_of(pc)).any()

    def heads(feat, anchor, geo, *flat):
        ww = {"w1": flat[0:3], "b1": flat[3:6], "w2": flat[6:9], "b2": flat[9:12]}
        return R.heads_f64(feat, anchor, cam, geo, ww)[0]
    assert torch.autograd.gradcheck(heads, (feat, anchor, geo, *flat), eps=1e-6, atol=1e-6, rtol=1e-5)

    from splatco_amd.scene_model import TriPlaneAttention
    torch.manual_seed(9)
    ta = TriPlaneAttention(6)
    ws = R.attention_weights(ta, requires_grad=True)
    planes = [(r(1, 2, 4, 5) * 0.5).requires_grad_() for _ in range(3)]
    with torch.no_grad():
        y = R.attention_f64(planes, *ws)[1]
        top = torch.topk(y[0], 2, dim=0)[0]
        assert (top[0] - top[1]).min() > 1e-4            # no channel maximum within the finite-difference step
    att = lambda p0, p1, p2, w1, w2, wc: tuple(R.attention_f64([p0, p1, p2], w1, w2, wc)[0])
    assert torch.autograd.gradcheck(att, (*planes, *ws), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_a_tied_pool_maximum_sends_its_gradient_to_the_first_pixel():
    """Two equal maxima in one channel: the whole gradient of the max pool goes to the first of them (the reference's
    AdaptiveMaxPool2d(1), and csrc/attention.hip).  Stated without a tie: lowering the SECOND maximum by 1e-9 leaves
    the gradient where it was, lowering the FIRST moves the pool's share to the second."""
    from splatco_amd.scene_model import TriPlaneAttention
    R_, H, W = 4, 12, 20            # (the max branch of the shared MLP is alive for this seed: the share is not 0)
    d = R.attention_inputs(R_, H, W)
    ws = R.attention_weights(d["ta"])
    p1, p2 = 3 * W + 4, 9 * W + 17

    def dx(delta1, delta2):
        planes = [p.double().clone() for p in d["planes"]]
        flat = planes[1][0, 3].view(-1)
        top = float(flat.max()) + 1.0
        flat[p1], flat[p2] = top - delta1, top - delta2
        _, _, grads, _ = R.attention_run(planes, [u.double() for u in d["up"]], ws)
        return grads[1][0, 3].reshape(-1)
    tie, second_lower, first_lower = dx(0, 0), dx(0, 1e-9), dx(1e-9, 0)
    assert (tie - second_lower).abs().max() < 1e-7
    moved = first_lower - tie
    share = float(moved[p2])                                   # the pool's gradient of this channel
    assert abs(share) > 1e-3 and abs(float(moved[p1]) + share) < 1e-7
    rest = moved.clone()
    rest[p1] = rest[p2] = 0
    assert rest.abs().max() < 1e-7
    # the module's amax would split the share between the two pixels: it cannot stand in for the reference here
    planes = [p.double().clone().requires_grad_(True) for p in d["planes"]]
    with torch.no_grad():
        flat = planes[1][0, 3].view(-1)
        flat[p1] = flat[p2] = float(flat.max()) + 1.0
    ta = TriPlaneAttention(3 * R_).double()
    ta.load_state_dict({k: v.double() for k, v in d["ta"].state_dict().items()})
    tri = ta(torch.cat(planes, dim=1))
    pairs = [torch.cat((p, a), dim=1) for p, a in zip(planes, torch.chunk(tri, 3, dim=1))]
    sum((o * u.double()).sum() for o, u in zip(pairs, d["up"])).backward()
    split = planes[1].grad[0, 3].reshape(-1) - tie
    assert abs(float(split[p2]) - 0.5 * share) < 1e-7 and abs(float(split[p1]) + 0.5 * share) < 1e-7


@pytest.mark.parametrize("V", R.HEADS_V)
def test_heads_inputs_stay_inside_the_replacement_cap(V):
    d = R.heads_inputs(V)                                      # asserts that no undecided row is left
    print(f"heads V={V}: first draw flagged {100 * d['flagged']:.3f} % of the rows, {d['rounds']} redraw rounds")
    assert d["flagged"] <= R.HEADS_CAP
    if V in R.HEADS_EDGE_V:
        w = R.weights_of(d["pc"])
        f64 = lambda t: t.double()
        zs, pre, _ = R._heads_layers(f64(d["feat"]), f64(d["anchor"]), f64(d["campos"]), f64(d["geo"]), w)
        assert len(d["edge_rows"]) == 2 * len(R.EDGE_Z)
        for row, (head, z) in d["edge_rows"].items():          # the planted pre-activations are there
            assert abs(float(zs[head][row, 0]) - z) <= 1e-6 + 1e-6 * abs(z), (row, head, z)   # fp32 rounding of feat[row, 0]
        assert (pre[:, 64 + R.ZERO_UNIT] == 0).all()


@pytest.mark.parametrize("name,R_,H,W,tie", R.ATTN_CASES, ids=[c[0] for c in R.ATTN_CASES])
def test_attention_inputs_stay_inside_the_exclusion_cap(name, R_, H, W, tie):
    d = R.attention_inputs(R_, H, W, tie)
    with torch.no_grad():
        _, y = R.attention_f64([p.double() for p in d["planes"]], *R.attention_weights(d["ta"]))
    share = float(R.attention_undecided(y).float().mean())
    print(f"attention {name} {R_}x{H}x{W}: {100 * share:.4f} % of the pixels excluded from dx")
    assert share <= R.ATTN_CAP
    if tie:
        x = torch.cat(d["planes"], dim=1)[0].reshape(3 * R_, -1)
        tied = ((x == x.amax(dim=1, keepdim=True)).sum(dim=1) > 1)
        assert int(tied.sum()) == (R_ if tie == "constant" else 1)
        per = (H * W + R.STAT_BLOCKS - 1) // R.STAT_BLOCKS
        c = int(tied.nonzero()[-1])
        at = (x[c] == x[c].max()).nonzero().squeeze(1)
        if tie == "two_blocks":
            assert int(at[0]) // per != int(at[1]) // per
        if tie == "one_block":
            assert int(at[0]) // per == int(at[1]) // per and int(at[0]) != int(at[1])
        assert int(d["arg"][c]) == int(at[0])
        # the case is about something: the pool's gradient of the tied channel is not 0 (lowering the first maximum by
        # 1e-9 moves it to the second)
        ws, up = R.attention_weights(d["ta"]), [u.double() for u in d["up"]]
        planes = [p.double() for p in d["planes"]]
        g0 = R.attention_run(planes, up, ws)[2][c // R_][0, c % R_].reshape(-1)
        planes[c // R_] = planes[c // R_].clone()
        planes[c // R_][0, c % R_].view(-1)[at[0]] -= 1e-9
        g1 = R.attention_run(planes, up, ws)[2][c // R_][0, c % R_].reshape(-1)
        share = float((g1 - g0)[at[1]])
        print(f"attention {name}: pool gradient of the tied channel {share:.3e} (max |dx| {float(g0.abs().max()):.3e})")
        assert abs(share) > 1e-3 * float(g0.abs().max())


@pytest.mark.parametrize("name,V,k,select,edges", R.EXPAND_CASES, ids=[c[0] for c in R.EXPAND_CASES])
def test_expansion_inputs_hold_what_the_case_is_about(name, V, k, select, edges):
    d = R.expand_inputs(V, k, select, edges)
    no, sr = d["args"][0], d["args"][2]
    mask = (no > 0).view(-1)
    n = V * k
    assert {"all": int(mask.sum()) == n, "none": not mask.any(), "alternating": bool((mask == (torch.arange(n) % 2 == 0)).all()),
            "random": 0 < int(mask.sum()) < n}[select]
    if edges:
        e = d["edge"]
        assert not mask[e["op_pzero"]] and not mask[e["op_nzero"]] and mask[e["op_subnormal"]]
        assert torch.signbit(no[e["op_nzero"]]).all() and float(no[e["op_subnormal"]]) == R.SUBNORMAL
        for q in ("quat_zero", "quat_zero2", "quat_tiny", "quat_tiny2"):
            assert mask[e[q]] and float(sr[e[q], 3:].double().norm()) < 1e-12
        assert float(sr[e["quat_tiny"], 3:].abs().max()) > 0
        assert mask[e["sig_hi"]] and mask[e["sig_lo"]] and mask[e["sig_mixed"]]


# ---------------------------------------------------------------------------------------------------------- image losses
def test_ssim_reference_reproduces_the_golden_losses():
    """losses.npz (captured from the reference's own loss functions in fp32): ssim_f64 / its L1 on the fixture's second
    image pair, to the fp32 rounding of the recorded values (the bars of test_fused_l1_ssim_matches_torch)."""
    d = _npz("losses.npz")
    l1, s, dx = R.ssim_f64(torch.tensor(d["a1"]), torch.tensor(d["b1"]))
    assert dx is None
    assert abs(float(s) - float(d["ssim_1"])) <= 1e-5 * abs(float(d["ssim_1"]))
    assert abs(float(l1) - float(d["l1_1"])) <= 1e-6


@functools.lru_cache(maxsize=None)
def _ssim_case(name):
    """(inputs, float64 result + the floor of dx's scale, finite elements of the float64 dx, the chain's result, its
    figures): computed once per case, shared by the tests below and never modified."""
    d = R.ssim_inputs(name)
    n = d["x"].numel()
    ref = (*R.ssim_f64(d["x"], d["y"], d["up"]), R.ssim_dx_floor(d["up"], n), R.ssim_row_floor(name, d["up"], n))
    finite = torch.isfinite(ref[2])
    chain = R.ssim_chain(d["x"], d["y"], d["up"])
    return d, ref, finite, chain, R.ssim_figures(chain, ref, finite)


def _same_class(got, ref):
    """A non-finite value: NaN where the reference is NaN, the same infinity where it is infinite."""
    got, ref = float(got), float(ref)
    return got != got if ref != ref else got == ref


@pytest.mark.parametrize("name", R.SSIM_IDS)
def test_correct_fp32_arithmetic_meets_the_bars_of_the_gpu_test(name):
    """The condition under which test_gpu_f64_parity.test_l1_ssim_against_float64 may ask what it asks: on every case
    the plain fp32 restatement of the kernel's arithmetic stays within max(2e-5, 1.5 e_chain) of float64, e_chain being
    the fp32 framework chain's figure on the CPU (which is within its own bar by construction: what is asserted of it
    is that it is finite where float64 is).  On the non-finite cases the three non-finite sets of dx are equal, the
    finite rest meets the bar, and the two values are non-finite in float64's way: NaN, except L1 of `inf_x`, which is
    +Inf in float64 itself (mean |Inf - y|).
    Measured here: noise 3.3e-7 against 9.9e-7 (dx), flat 2.0e-4 against 4.8e-4, flat_both 8.6e-5 against 2.0e-4, ramp
    1.8e-5 against 5.4e-5; non-finite elements 441, 168 and 121 in all three.  One thing had to give: on `identical`
    the floor of dx's scale goes under every row's scale too (f64_refs.SSIM_ROW_FLOOR_CASES says why)."""
    d, ref, finite, chain, f_chain = _ssim_case(name)
    got = R.ssim_restated_f32(d["x"], d["y"], *d["up"])
    f = R.ssim_figures(got, ref, finite)
    values = ("L1", "SSIM")
    for k in f:
        if d["nonfinite"] and k in values:
            continue
        print(f"l1_ssim {name:16s} {k:8s} restated {f[k]:9.3e}  chain {f_chain[k]:9.3e}  bar {R.bar(f_chain[k]):9.3e}")
    print(f"l1_ssim {name:16s} non-finite elements of dx: {int((~finite).sum())}")
    if d["nonfinite"]:
        assert int((~finite).sum()) == {"nan_x": 441, "nan_y": 168, "inf_x": 121}[name]   # 21 x 21, 14 x 12, 11 x 11
        for r in (got, chain):
            assert torch.equal(torch.isfinite(r[2]), finite)
            assert _same_class(r[0], ref[0]) and _same_class(r[1], ref[1])
        assert float(ref[1]) != float(ref[1]) and not torch.isfinite(ref[0])
        assert (float(ref[0]) == float("inf")) == (name == "inf_x")
    else:
        assert finite.all()
        for r in (got, chain):
            assert all(bool(torch.isfinite(t).all()) for t in r)
    for k in f:
        if not (d["nonfinite"] and k in values):
            assert f[k] <= R.bar(f_chain[k]) and f_chain[k] <= R.bar(f_chain[k]), (k, f[k], f_chain[k])
    if name == "identical":
        assert float(got[0]) == 0 and abs(float(got[1]) - 1) <= 2.0 ** -22
    if name == "anti":
        assert float(ref[1]) < 0


_FINITE = {n for n in R.SSIM_IDS if n not in R.SSIM_NONFINITE}
_USES_DSSIM = _FINITE - {"up_1_0", "up_1_none"}                        # the SSIM gradient reaches dx
_W21 = {c[0] for c in R.SSIM_CASES if c[1][2] >= 21}                   # a full tile column with five pixels to its right
SSIM_FAULT_SEEN_BY = {
    # under any window the maps of x == y cancel (identical) or vanish (zeros); L1-only graphs never read the maps, and the
    # value moves by the last tap (1e-3) on two columns of 37, below the floor; W < 21: the sixth pixel right of column
    # 15 is outside the image and 0 either way
    "reach4_right": (_USES_DSSIM & _W21) - {"identical", "zeros"},
    # x == y at the border (impulse: the two pixels are interior): SSIM = 1 and cancelling maps under any padding
    "clamp": _FINITE - {"identical", "zeros", "impulse"},
    "no_mu2_dE12": _USES_DSSIM - {"zeros"},                            # mu2 = 0
    "map_index": _USES_DSSIM - {"c1_17x33"},                           # c * 3 + m == m * C + c at C = 1
    "reduce_1024": {"300x300"},                                        # the only case with more than 1024 tiles (1083)
    "sign0_is_1": {"identical", "ties", "zeros"},                      # the cases with x == y where g_l1 != 0
}


@pytest.mark.parametrize("fault", sorted(SSIM_FAULT_SEEN_BY))
def test_a_wrong_restatement_misses_the_bars_on_the_cases_chosen_for_it(fault):
    """Each deliberate error of f64_refs.ssim_restated_f32 fails the bars of the GPU test on exactly the cases named in
    SSIM_FAULT_SEEN_BY, which say why the others cannot see it: the cases see the errors they were chosen for."""
    missed = set()
    for name in sorted(_FINITE):
        d, ref, finite, _, f_chain = _ssim_case(name)
        f = R.ssim_figures(R.ssim_restated_f32(d["x"], d["y"], *d["up"], fault=fault), ref, finite)
        bad = {k: f[k] / R.bar(f_chain[k]) for k in f if not f[k] <= R.bar(f_chain[k])}
        if bad:
            missed.add(name)
            print(f"{fault:13s} {name:16s} " + "  ".join(f"{k} {v:.3g} x bar" for k, v in bad.items()))
    assert missed and missed == SSIM_FAULT_SEEN_BY[fault], (sorted(missed - SSIM_FAULT_SEEN_BY[fault]),
                                                            sorted(SSIM_FAULT_SEEN_BY[fault] - missed))


def test_an_ulp_on_the_sum_of_the_taps_shows_on_flat_images():
    """The seventh fault, tap_sum_ulp: the taps divided by their sum added one by one in fp32 (3.7592325, an ulp below the
    correctly rounded 3.7592328).  The 2-D window then sums to 1 + 8.9e-8 where the reference's sums to 1 - 6.2e-8, and
    s11 = E11 - mu1^2 and s22 each move by 1.5e-7 mu^2: 3e-7 on B2 = s11 + s22 + C2 = 9.0e-4, that is 3.3e-4 of the
    maps and of dx, on `flat_both` (level 1).  The exact restatement is at 8.6e-5 there.  (The GPU test's bar on that
    case, 1.5 x the chain's 1.8e-4 .. 2.0e-4, lies between the two.)"""
    d, ref, finite, _, _ = _ssim_case("flat_both")
    good = R.ssim_figures(R.ssim_restated_f32(d["x"], d["y"], *d["up"]), ref, finite)["dx"]
    bad = R.ssim_figures(R.ssim_restated_f32(d["x"], d["y"], *d["up"], fault="tap_sum_ulp"), ref, finite)["dx"]
    print(f"flat_both dx: exact restatement {good:.3e}, an ulp on the tap sum {bad:.3e}")
    assert good <= 1.5e-4 and 2.5e-4 <= bad <= 4.5e-4
    total = lambda g: float(torch.outer(g.double(), g.double()).sum()) - 1.0
    assert abs(total(R.ssim_window()) + 6.2e-8) < 1e-8


def test_the_reference_taps_are_the_chain_taps():
    """f64_refs.ssim_window() fixes its own summation order; losses._window leaves it to torch's sum.  Bit for bit the
    same taps: an ulp between them is the 3.3e-4 of the test above, and would be charged to the kernel."""
    from splatco_amd.losses import _window
    g = R.ssim_window()
    assert g.dtype == torch.float32
    assert torch.equal(_window(11, 3, torch.zeros(1)), g.unsqueeze(1).mm(g.unsqueeze(0)).expand(3, 1, 11, 11))


def test_image_loss_inputs_hold_what_the_case_is_about():
    T = R.SSIM_TILE
    tiles = lambda s: s[0] * ((s[1] + T - 1) // T) * ((s[2] + T - 1) // T)
    assert [tiles(s) > R.SSIM_REDUCE for s in R.SSIM_SHAPES] == [False] * (len(R.SSIM_SHAPES) - 1) + [True]
    assert tiles(R.SSIM_SHAPES[-1]) == 1083
    assert len(set(R.SSIM_IDS)) == len(R.SSIM_IDS)
    d = R.ssim_inputs("identical")
    assert torch.equal(d["x"], d["y"])
    d = R.ssim_inputs("ties")
    assert 0.4 < float((d["x"] == d["y"]).float().mean()) < 0.6
    d = R.ssim_inputs("impulse")
    assert (d["x"] != d["y"]).nonzero().tolist() == [[c, p, p] for c in range(3) for p in (15, 16)] and d["up"][0] == 0
    d = R.ssim_inputs("range")
    assert float(d["x"].min()) < -0.9 and float(d["x"].max()) > 2.9
    for name, (which, at, value) in R.SSIM_NONFINITE.items():
        d = R.ssim_inputs(name)
        bad = ~torch.isfinite(d[which])
        assert int(bad.sum()) == 1 and bool(bad[at]) and torch.isfinite(d["y" if which == "x" else "x"]).all()
    nb = lambda n, per: (n + per - 1) // per
    assert [nb(P, 2048) for P in R.SREG_P[-2:]] == [1024, 1025] and [nb(n, 4096) for n in R.PAIR_N[-2:]] == [1024, 1025]
    for P in R.SREG_P:
        s = R.sreg_inputs(P)
        k = min(P, len(R.SREG_EDGE_ROWS))
        assert s.shape == (P, 3) and torch.equal(s[:k], torch.tensor(R.SREG_EDGE_ROWS[:k]))
        assert float(s[k:].min() if P > k else 1) >= 0.01 and [int((r == 0).sum()) for r in s[:3]] == [1, 2, 3][:k]
    for n in R.PAIR_N[:4]:
        a, b, r1, r2 = R.pair_inputs(n)
        res = (r1 - r2) - (a - b)
        assert float(res[::R.PAIR_ZERO_STRIDE].abs().max()) <= 2.0 ** -22 and (n < 2 or float(res.abs().max()) > 0.1)


@pytest.mark.parametrize("shape", R.L1_ORDER_SHAPES, ids=["%dx%dx%d" % s for s in R.L1_ORDER_SHAPES])
def test_the_l1_order_emulator_is_a_mean_and_its_seeds_tell_the_orders_apart(shape):
    """f64_refs.l1_tile_order (what test_gpu_f64_parity asks of the kernel bit for bit) is within 2^-22 mean + 1e-12 of the
    float64 mean (a tile's 256 binary32 terms pass 8 tree levels of 2^-25 each at most, then one rounding of the mean;
    the float64 fold adds nothing visible; these inputs come to 0.08 .. 0.15 of the bound) -- and on the recorded seeds
    the two orders the kernel must not have end in other bits, so the GPU test's equality pins the order.  A shape
    without a recorded seed has one live pixel per tile: no order can show."""
    x, y = R.l1_order_inputs(shape)
    assert x.dtype == y.dtype == np.float32 and x.shape == y.shape == shape
    got = R.l1_tile_order(x, y)
    mean = np.abs(x - y).astype(np.float64).mean()
    print(f"l1 order {shape}: emulator {float(got):.9g}, float64 mean {mean:.9g}, |diff| {abs(float(got) - mean) / mean * 2 ** 22:.3f} x 2^-22 mean")
    assert got.dtype == np.float32 and abs(float(got) - mean) <= 2.0 ** -22 * mean + 1e-12
    others = [R.l1_tile_order(x, y, o) for o in R.L1_ORDER_ALTERNATIVES]
    if R.L1_ORDER_SEEDS[shape] is None:
        assert shape[1] * shape[2] == 1 and all(o.view(np.uint32) == got.view(np.uint32) for o in others)
    else:
        assert all(o.view(np.uint32) != got.view(np.uint32) for o in others), [float(o) for o in others]


# ---------------------------------------------------------------------------------------------------------- anchor gather
def test_gather_reference_is_the_literal_chain_and_passes_gradcheck():
    """gather_f64 / gather_run on float64 give what autograd gives of the reference's own lines (boolean-mask gathers,
    get_scaling = exp(_scaling), the concatenation), and gather_f64 with gather_dx_f64 behind it passes gradcheck."""
    d = R.gather_inputs("b65")
    mask = torch.rand(65, generator=torch.Generator().manual_seed(3)) < 0.6
    idx = mask.nonzero().view(-1)
    V = idx.numel()
    ps = [p.double().requires_grad_(True) for p in d["params"]]
    up = {n: t[:V].double() for n, t in d["up"].items()}
    feat, anchor, offs, gs = ps[0][mask], ps[1][mask], ps[2][mask], torch.exp(ps[3])[mask]
    g_fea = torch.cat([feat, anchor, offs.view(V, -1), gs], dim=1)
    outs = (feat, anchor, offs.view(V, -1), gs, g_fea)
    sum((o * up[n][:, :o.shape[1]]).sum() for n, o in zip(R.GATHER_UP, outs)).backward()
    got_o, got_g = R.gather_run(idx, [p.detach() for p in ps], up)
    assert got_o[4].shape == (V, 71) and got_o[2].shape == (V, 10, 3)
    for a, b in zip(got_o, (feat, anchor, offs, gs, g_fea)):
        assert torch.equal(a, b.detach())
    for a, p in zip(got_g, ps):
        assert a.shape == p.shape and torch.allclose(a, p.grad, rtol=1e-14, atol=1e-14)
    assert float(got_g[0][~mask].abs().max()) == 0 and float(got_g[3][mask].abs().min()) > 0
    g = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    idx = torch.tensor([0, 2, 3])
    ps = [r(5, 32).requires_grad_(), r(5, 3).requires_grad_(), r(5, 10, 3).requires_grad_(), (r(5, 6) * 0.3 - 3).requires_grad_()]
    coef, dy = r(34, 80), r(3, 32)

    def fn(*p):
        outs = R.gather_f64(idx, *p)
        return (*outs, R.gather_dx_f64(coef, dy, outs[4]))
    assert torch.autograd.gradcheck(fn, ps, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_gather_inputs_hold_what_the_case_is_about():
    """From `inv` alone: what each block of 64 anchors of every case makes the backward kernel do."""
    ds = {c: R.gather_inputs(c) for c in R.GATHER_CASES}
    for c, d in ds.items():
        assert d["inv"].shape == (d["N"],) and int((d["inv"] >= 0).sum()) == d["V"] and d["N"] <= 2100
        assert torch.equal(d["inv"][d["idx"]], torch.arange(d["V"])) and float(d["coef"][:, 71:].abs().max()) == 0
        assert d["blocks"] == R.gather_blocks(d["inv"], d["V"]) and len(d["blocks"]) == -(-d["N"] // 64)
    facts = lambda c: [(b["fv"], b["nv"], b["path"]) for b in ds[c]["blocks"]]
    assert facts("one") == [(0, 1, "tail")] and facts("one_hidden") == [(-1, 0, "none")] and ds["one_hidden"]["V"] == 0
    assert facts("b63") == [(0, 63, "tail")] and facts("b64") == [(0, 64, "tail")]
    assert facts("b65") == [(0, 64, "tail"), (64, 1, "tail")]
    assert facts("b129") == [(0, 64, "vector"), (64, 64, "tail"), (128, 1, "tail")]
    assert facts("only_last") == [(-1, 0, "none")] * 3 + [(0, 1, "tail")] and ds["only_last"]["idx"].tolist() == [199]
    assert facts("only_first") == [(0, 1, "tail")] + [(-1, 0, "none")] * 3
    hole = facts("hole")
    assert hole[1] == (-1, 0, "none") and all(f[1] > 0 for f in hole[:1] + hole[2:]) and not ds["hole"]["mask"][64:128].any()
    te, V = facts("tail_edge"), ds["tail_edge"]["V"]
    assert ds["tail_edge"]["N"] == (R.GATHER_TAIL_FRONT + 3) * 64 + 1 and len(te) == R.GATHER_TAIL_FRONT + 4
    assert all(f[2] == "vector" and f[0] + f[1] <= V - 3 for f in te[:R.GATHER_TAIL_FRONT])
    assert te[-4:] == [(V - 3, 1, "vector"), (V - 2, 1, "tail"), (-1, 0, "none"), (V - 1, 1, "tail")]
    assert [f[0] + f[1] for f in te if f[1]][-3:] == [V - 2, V - 1, V]
    mixed = ds["mixed"]
    assert mixed["N"] == 64 * 9 + 7 and 0.4 < mixed["V"] / mixed["N"] < 0.6
    hs = lambda w: {b["h"][w] for b in mixed["blocks"] if b["nv"]}
    assert hs(3) == hs(71) == {0, 1, 2, 3} and hs(6) == hs(30) == {0, 2} and hs(32) == hs(72) == {0}
    assert {b["path"] for b in mixed["blocks"]} == {"vector", "tail"}
    for c, V in R.GATHER_FWD_V.items():
        assert ds[c]["V"] == V and R.gather_stat_rows(V) == R.GATHER_STAT_ROWS[c]
    assert [R.gather_stat_rows(V) for V in (1, 511, 512, 513, 1025)] == [1, 1, 1, 2, 3]


def _gather_variants(d):
    """(name, upstreams, dx, old) the GPU tests run on a case: everything, without dx; accumulating; with dx, with and
    without a gradient that did arrive for g_fea."""
    up = d["up"]
    x = R.gather_f64(d["idx"], *d["params"])[4]
    dx = (d["coef"], d["dy"], x)
    out = [("all", up, None, None), ("accumulate", up, None, d["old"])]
    if d["case"] in R.GATHER_DX_CASES:
        out += [("dx", {**up, "g_fea": None}, dx, None), ("dx + d g_fea", up, dx, None)]
    return out


def _gather_ref(d, up, dx, old):
    f = lambda t: None if t is None else t.double()
    dx64 = None if dx is None else R.gather_dx_f64(*(f(t) for t in dx))
    _, ref = R.gather_run(d["idx"], [f(p) for p in d["params"]], {n: f(t) for n, t in up.items()}, dx64)
    if old is not None:
        ref = [r.reshape(d["N"], -1) + f(o) for r, o in zip(ref, old)]
    return ref, R.gather_terms(d, up, dx, old)


@pytest.mark.parametrize("case", R.GATHER_BWD_CASES)
def test_correct_fp32_gather_arithmetic_meets_the_a_priori_bounds(case):
    """The condition under which the gather tests of test_gpu_f64_parity may ask what they ask: the backward's
    arithmetic in plain fp32 (f64_refs.gather_restated_f32) is inside 4 x 2^-24 / 40 x 2^-24 of the sum of its terms on
    every element of every case, fp32 exp inside 2^-23, and fp32 column sums of 512 rows inside 512 x 2^-24."""
    d = R.gather_inputs(case)
    for name, up, dx, old in _gather_variants(d):
        ref, terms = _gather_ref(d, up, dx, old)
        tol = R.GATHER_DX_TOL if dx is not None else R.GATHER_BWD_TOL
        e = R.gather_excess(R.gather_restated_f32(d, up, dx, old), ref, terms, tol)
        print(f"gather {case:10s} {name:14s} worst |got - ref| / bound {e:.3f}")
        assert e <= 1
        assert old is not None or all(float(r.reshape(d["N"], -1)[~d["mask"]].abs().sum()) == 0 for r in ref)
    outs = R.gather_f64(d["idx"], *d["params"])
    if d["V"]:
        e64 = torch.exp(d["params"][3].double())[d["idx"]]
        assert float(((outs[3].double() - e64).abs() / e64).max()) <= R.GATHER_EXP_FLOOR
        g = outs[4]
        t = g - g[0]
        parts = [torch.stack((c.sum(dim=0), (c * c).sum(dim=0))) for c in t.split(512)]
        stats = torch.zeros(len(parts), 2, 80)
        stats[:, :, :71] = torch.stack(parts)
        e, zeros = R.gather_stats_excess(stats, g)
        print(f"gather {case:10s} statistics     worst |got - ref| / bound {e:.3f}")
        assert e <= 1 and zeros


@pytest.mark.parametrize("case", R.GATHER_SUB_CASES)
def test_the_old_value_of_an_accumulating_call_stands_outside_exp_s(case):
    """Why gather_terms adds |old| BEHIND the factor exp(s): the kernel multiplies the new gradient by exp(s) = 0.05 and
    then adds it to the old value, and that addition alone rounds to 2^-24 |old + new|.  With the bound written as
    4 x 2^-24 (|d part| + |d g_fea| + |old|) exp(s), plain fp32 arithmetic is several times outside it on d scaling
    (5.7 x on `mixed`, 6.8 x on `tail_edge`); the other three gradients have exp(s) = 1 and are the same either way."""
    d = R.gather_inputs(case)
    ref, terms = _gather_ref(d, d["up"], None, d["old"])
    got = R.gather_restated_f32(d, d["up"], None, d["old"])
    e_s = torch.zeros(d["N"], 6, dtype=torch.float64)
    e_s[d["idx"]] = torch.exp(d["params"][3].double())[d["idx"]]
    new = R.gather_terms(d, d["up"])[3]
    inside = new + d["old"][3].double().abs() * e_s
    vis = d["mask"]
    e_in = R.gather_excess([got[3][vis]], [ref[3][vis]], [inside[vis]], R.GATHER_BWD_TOL)
    e_out = R.gather_excess([got[3]], [ref[3]], [terms[3]], R.GATHER_BWD_TOL)
    print(f"gather {case}: d scaling, accumulate: {e_in:.2f} x the bound with |old| exp(s), {e_out:.2f} x with |old|")
    assert e_in > 3 and e_out <= 1


# `one` and the two `only_` cases have one upstream row: a block that starts a row late reads that row again
_GATHER_V2 = {c for c in R.GATHER_BWD_CASES if R.gather_mask(c).sum() >= 2}
GATHER_FAULT_SEEN_BY = {
    "no_xk1_col3": set(R.GATHER_DX_CASES),                               # the cases that run with dx
    "first_v_plus_1": _GATHER_V2,
    "no_exp": set(R.GATHER_BWD_CASES) - {"one_hidden"},                  # V = 0: nothing to scale
}


@pytest.mark.parametrize("fault", R.GATHER_FAULTS)
def test_a_wrong_gather_restatement_misses_the_bounds_on_the_cases_chosen_for_it(fault):
    """Each deliberate error of f64_refs.gather_restated_f32 leaves the a-priori bounds on exactly the cases named in
    GATHER_FAULT_SEEN_BY."""
    missed = set()
    for case in R.GATHER_BWD_CASES:
        d = R.gather_inputs(case)
        for name, up, dx, old in _gather_variants(d):
            ref, terms = _gather_ref(d, up, dx, old)
            tol = R.GATHER_DX_TOL if dx is not None else R.GATHER_BWD_TOL
            e = R.gather_excess(R.gather_restated_f32(d, up, dx, old, fault=fault), ref, terms, tol)
            if e > 1:
                missed.add(case)
                print(f"{fault:15s} {case:10s} {name:14s} {e:.3g} x bound")
    assert missed == GATHER_FAULT_SEEN_BY[fault], (sorted(missed - GATHER_FAULT_SEEN_BY[fault]),
                                                   sorted(GATHER_FAULT_SEEN_BY[fault] - missed))


# ---------------------------------------------------------------------------------------------------------- norm-linear
def _bn_linear_chain(xs, bns, linears):
    return sum(lin(bn(x)) for x, bn, lin in zip(xs, bns, linears))


def test_norm_linear_references_are_the_module_chain_and_pass_gradcheck():
    """At float64 statistics nl_forward_f64 / nl_backward_f64 / nl_dx_f64 are BatchNorm1d(affine=False, training) -> Linear
    and its autograd to 1e-12; nl_fold_f64 (+ the forward on the column-mapped input) is the chain of modules FeaturePlanes
    sums, with and without col_at; the backward algebra passes gradcheck."""
    torch.manual_seed(3)
    V, d, eps = 257, 23, 1e-5
    inp = R.nl_inputs(V, d)
    x, G, c, dy = (inp[k].double() for k in ("x", "G", "c", "dy"))
    bn, lin = torch.nn.BatchNorm1d(d, eps=eps, affine=False).double().train(), torch.nn.Linear(d, 32).double()
    with torch.no_grad():
        lin.weight.copy_(G)
        lin.bias.copy_(c)
    xa = x.clone().requires_grad_()
    ya = lin(bn(xa))
    (ya * dy).sum().backward()
    mean, var = R.nl_stats_f64(x)
    inv = 1.0 / torch.sqrt(var + eps)
    dG, dc, Gi, k0, k1 = R.nl_backward_f64(x, dy, G, mean, inv)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    figures = {"y": rel(R.nl_forward_f64(x, G, c, mean, inv), ya.detach()), "dx": rel(R.nl_dx_f64(x, dy, Gi, k0, k1), xa.grad),
               "dG": rel(dG, lin.weight.grad), "dc": rel(dc, lin.bias.grad)}
    print(figures)
    assert max(figures.values()) <= 1e-12

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x_, G_, c_):
            m, v = R.nl_stats_f64(x_)
            iv = 1.0 / torch.sqrt(v + eps)
            ctx.save_for_backward(x_, G_, m, iv)
            return R.nl_forward_f64(x_, G_, c_, m, iv)

        @staticmethod
        def backward(ctx, dy_):
            x_, G_, m, iv = ctx.saved_tensors
            dG_, dc_, Gi_, k0_, k1_ = R.nl_backward_f64(x_, dy_, G_, m, iv)
            return R.nl_dx_f64(x_, dy_, Gi_, k0_, k1_), dG_, dc_
    small = [t.clone().requires_grad_() for t in (x[:9, :5], G[:, :5], c)]
    assert torch.autograd.gradcheck(Fn.apply, small, eps=1e-6, atol=1e-7)

    for name, _, widths, cols, _ in R.NL_FOLD_CASES:
        p = R.nl_fold_inputs(name)
        dd, at = p["d"], p["col_at"]
        bns = [torch.nn.BatchNorm1d(w, eps=eps).double().train() for w in widths]
        lins = [torch.nn.Linear(w, 32).double() for w in widths]
        with torch.no_grad():
            for i in range(len(widths)):
                bns[i].weight.copy_(p["gamma"][i]); bns[i].bias.copy_(p["beta"][i])
                lins[i].weight.copy_(p["W"][i]); lins[i].bias.copy_(p["b"][i])
        xr = torch.randn(64, dd, dtype=torch.float64)                   # the reference's column order
        want = _bn_linear_chain([xr[:, c0:c0 + w] for c0, w in zip(cols, widths)], bns, lins).detach()
        xk = xr if at is None else torch.zeros_like(xr).index_copy(1, torch.as_tensor(at), xr)   # column j kept at col_at[j]
        f = lambda k: [t.double() for t in p[k]]
        G_, c_ = R.nl_fold_f64(f("W"), f("b"), f("gamma"), f("beta"), widths, cols, dd, at)
        m, v = R.nl_stats_f64(xk)
        e = rel(R.nl_forward_f64(xk, G_, c_, m, 1.0 / torch.sqrt(v + eps)), want)
        print(f"fold {name}: {e:.2e}")
        assert e <= 1e-12
        # the fold's backward is the autograd of the fold
        leaves = [[t.clone().requires_grad_() for t in f(k)] for k in ("W", "b", "gamma", "beta")]
        Ga, ca = R.nl_fold_f64(*leaves, widths, cols, dd, at)
        ((Ga * p["dG"].double()).sum() + (ca * p["dc"].double()).sum()).backward()
        got = R.nl_fold_backward_f64(p["dG"].double(), p["dc"].double(), f("W"), f("gamma"), f("beta"), widths, cols, at)
        for i, (dW, db, dga, dbe) in enumerate(got):
            for a, b_ in ((dW, leaves[0][i].grad), (db, leaves[1][i].grad), (dga, leaves[2][i].grad), (dbe, leaves[3][i].grad)):
                assert float((a - b_).abs().max()) <= 1e-12 * max(1.0, float(b_.abs().max()))
        # running statistics: nn.BatchNorm1d's own update (identity column map; the modules saw xr's blocks)
        if at is None:
            n = xr.shape[0]
            m_, v_ = R.nl_stats_f64(xr)
            old = [(torch.zeros(w, dtype=torch.float64), torch.ones(w, dtype=torch.float64)) for w in widths]
            upd = R.nl_running_f64([o[0] for o in old], [o[1] for o in old], [0.1] * len(widths), m_, v_, n, widths, cols)
            for bn_, (rm, rv) in zip(bns, upd):
                assert float((bn_.running_mean - rm).abs().max()) <= 1e-12 and float((bn_.running_var - rv).abs().max()) <= 1e-12


def _nl_host_cases():
    """(name, inputs, eps, col_stats rows): every GPU case with V <= 4099 (x's layout changes no arithmetic)."""
    out = [(f"rows V={V} d={d}", R.nl_inputs(V, d), 1e-5, 0) for d, _ in R.NL_ROW_DL for V in R.NL_ROW_V]
    out += [(f"cols d={d}", R.nl_inputs(R.NL_COL_V, d), 1e-5, 0) for d in R.NL_COL_D]
    out += [(f"grads d={d}", R.nl_inputs(R.NL_COL_V, d, seed=1), 1e-5, 0) for d in R.NL_GRAD_D]
    out += [(f"slabs V={V} d={d}", R.nl_inputs(V, d), 1e-5, 0) for V, d, _ in R.NL_SLAB_CASES if V <= 4099]
    out += [(f"cstats rows={r}", R.nl_inputs(R.NL_COLSTAT_V, 71), 1e-5, r) for r in R.NL_COLSTAT_ROWS]
    x = R.nl_regime_matrix()
    g = torch.Generator().manual_seed(8)
    reg = dict(V=x.shape[0], d=8, x=x, G=torch.randn(32, 8, generator=g), c=torch.randn(32, generator=g),
               dy=torch.randn(x.shape[0], 32, generator=g))
    out += [(f"regime eps={eps:g} {'col_stats' if r else 'builtin'}", reg, eps, r) for eps in R.NL_EPS for r in (0, 9)]
    return out


def _nl_restated_figures(inp, eps, rows, fault=None, lanes="fp32"):
    """{name: |got - ref| / bound} of f64_refs.nl_restated_f32 on one case, each launch against float64 on its own inputs.
    lanes = "fp64": the slab sums as the kernel forms them, judged at the kernel's NL_STAT_COMBINE roundings."""
    x, d = inp["x"], inp["d"]
    stats = R.nl_col_stats(x, rows) if rows else None
    pad = torch.full((inp["V"],), float("nan"))
    o = R.nl_restated_f32(x, inp["G"], inp["c"], inp["dy"], eps, fault=fault, pad=pad, col_stats=stats, lanes=lanes)
    n_s = R.NL_STAT_COMBINE if rows or lanes == "fp64" else R.nl_n_s(d)
    fig = dict(R.nl_forward_figures(x, inp["G"], inp["c"], eps, o["y"], o["mean"], o["var"], o["inv"], n_s))
    fig.update(R.nl_backward_figures(x, inp["dy"], inp["G"], o["mean"], o["inv"], o["dG"], o["dc"], o["coef"]))
    fig.update(R.nl_dx_figures(x, inp["dy"], o["coef"], o["dx"]))
    return fig


@functools.lru_cache(maxsize=None)
def _nl_all_restated():
    """Every host case with fp32 slab sums; the built-in statistics cases again with the kernel's fp64 lanes."""
    cases = _nl_host_cases()
    return ([(name, _nl_restated_figures(inp, eps, rows)) for name, inp, eps, rows in cases]
            + [(name + " fp64 lanes", _nl_restated_figures(inp, eps, rows, lanes="fp64")) for name, inp, eps, rows in cases if not rows])


def test_correct_fp32_norm_linear_arithmetic_meets_the_a_priori_bounds():
    """The condition under which the norm-linear tests of test_gpu_f64_parity may ask what they ask: the three launches in
    plain fp32 torch (f64_refs.nl_restated_f32: the kernels' formulas, torch's summation order) are inside every bound on
    every case with V <= 4099.  The statistics are judged twice: slab sums formed in fp32 against the 516- / 1026-term bound
    of such a lane (nl_n_s), and slab sums formed in float64 and rounded to fp32 once -- what nl_stats_partial_kernel does and
    what a caller's col_stats are -- against the NL_STAT_COMBINE = 2 roundings the GPU tests hold the kernel to.  The worst
    ratio per bound is printed."""
    worst = {}
    for name, fig in _nl_all_restated():
        for k, e in fig.items():
            if e > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (e, name)
    for k, (e, name) in worst.items():
        print(f"norm-linear {k:5s} worst |got - ref| / bound {e:.3f}  ({name})")
    assert all(e <= 1 for e, _ in worst.values()), worst


def test_constant_and_single_row_columns_are_exact_in_the_restatement():
    """What the regime test asks of the kernel holds for the formulas: a constant column has var == 0 and mean == the
    constant, a one-row matrix var == 0 and mean == x[0], bit for bit."""
    x = R.nl_regime_matrix()
    z = torch.zeros(32, 8)
    o = R.nl_restated_f32(x, z, z[:, 0], torch.zeros(x.shape[0], 32), 1e-5)
    k = R.NL_REGIME_COLUMNS.index("constant")
    assert float(o["var"][k]) == 0.0 and float(o["mean"][k]) == 3.25
    inp = R.nl_inputs(1, 60)
    o = R.nl_restated_f32(inp["x"], inp["G"], inp["c"], inp["dy"], 1e-5)
    assert bool((o["var"] == 0).all()) and torch.equal(o["mean"], inp["x"][0])


# fault -> (the case named for it, the figure that must leave its bound there).  The last two are faults of the parameter
# fold: test_fp32_fold_arithmetic_meets_its_bounds_and_two_wrong_folds_do_not runs them on every fold case and asserts from
# this table which see them (the cases of NL_FOLD_CASES; the row counts n of the running-statistics update)
NL_FAULT_SEEN_BY = {
    "stats_drop_last_row": ("regime eps=1e-05 builtin", "mean"),         # the last-row-only column: mean == 0
    "pad_column_read": ("cols d=71", "y"),
    "k1_without_inv2": ("grads d=60", "k1"),                              # inv = 3.3 in the log-scaling columns
    "dG_without_sdy_mean": ("grads d=60", "dG"),                          # mean = -5 there
    "fold_bwd_ignores_at": ({"L3_planes", "L3_random"}, "fold backward"),  # the cases with a column map, and no other
    "unbias_n_over_n": ({1: False, 2: True}, "running statistics"),      # n / (n - 1) = 2 at n = 2; n = 1 has no factor
}
assert set(NL_FAULT_SEEN_BY) == set(R.NL_FAULTS)


@pytest.mark.parametrize("fault", R.NL_FAULTS[:4])
def test_a_wrong_norm_linear_restatement_misses_the_bounds_on_the_case_named_for_it(fault):
    case, figure = NL_FAULT_SEEN_BY[fault]
    name, inp, eps, rows = next(c for c in _nl_host_cases() if c[0] == case)
    good, bad = _nl_restated_figures(inp, eps, rows), _nl_restated_figures(inp, eps, rows, fault=fault)
    print(f"{fault}: {case}: {figure} {good[figure]:.3f} -> {bad[figure]:.3g} x bound")
    assert good[figure] <= 1 < bad[figure]


def test_fp32_fold_arithmetic_meets_its_bounds_and_two_wrong_folds_do_not():
    """The fold launches in plain fp32 torch are inside the bounds of test_norm_fold_kernels_against_float64 on every case;
    a backward that reads dG as it lies (col_at not applied) leaves them on the two cases with a column map and on no
    other; running statistics with n / n in place of n / (n - 1) leave them at n = 2 and not at n = 1."""
    for name, *_ in R.NL_FOLD_CASES:
        p = R.nl_fold_inputs(name)
        w, cols, at = p["widths"], p["cols"], p["col_at"]
        f64 = lambda k: [t.double() for t in p[k]]
        G32, c32 = R.nl_fold_f64(p["W"], p["b"], p["gamma"], p["beta"], w, cols, p["d"], at)
        G64, c64 = R.nl_fold_f64(f64("W"), f64("b"), f64("gamma"), f64("beta"), w, cols, p["d"], at)
        bG, bc = R.nl_fold_bounds(p)
        eG, ec = R.nl_excess(G32, G64, bG), R.nl_excess(c32, c64, bc)
        ref = R.nl_fold_backward_f64(p["dG"].double(), p["dc"].double(), f64("W"), f64("gamma"), f64("beta"), w, cols, at)
        bnd = R.nl_fold_backward_bounds(p)
        worst = {}
        for apply_at in (True, False):
            got = R.nl_fold_backward_f64(p["dG"], p["dc"], p["W"], p["gamma"], p["beta"], w, cols, at, apply_at=apply_at)
            worst[apply_at] = max(R.nl_excess(a, r, b) for g4, r4, b4 in zip(got, ref, bnd) for a, r, b in zip(g4, r4, b4))
        print(f"fold {name:12s} G {eG:.3f} c {ec:.3f} backward {worst[True]:.3f}; col_at ignored: {worst[False]:.3g}")
        assert eG <= 1 and ec <= 1 and worst[True] <= 1
        assert (worst[False] > 1) == (name in NL_FAULT_SEEN_BY["fold_bwd_ignores_at"][0]) == (at is not None)
        for n in (1, 2):
            want = R.nl_running_f64(f64("run_mean"), f64("run_var"), p["momentum"], p["mean"].double(), p["var"].double(), n, w, cols, at)
            bd = R.nl_running_bounds(p, n)
            for unbiased in (True, False):
                got = R.nl_running_f64(p["run_mean"], p["run_var"], [torch.tensor(m) for m in p["momentum"]], p["mean"], p["var"], n,
                                       w, cols, at, unbiased=unbiased)
                e = max(max(R.nl_excess(g[0], r[0], b[0]), R.nl_excess(g[1], r[1], b[1])) for g, r, b in zip(got, want, bd))
                print(f"fold {name:12s} running n={n} unbiased={unbiased}: {e:.3g}")
                assert (e > 1) == (not unbiased and NL_FAULT_SEEN_BY["unbias_n_over_n"][0][n])


def test_norm_linear_cases_reach_every_instantiation_and_loop_form():
    """From the shapes alone (f64_refs.nl_case_facts): the column-edge cases reach Q = NT = 1 .. 5 of the forward, reduce and dx
    kernels with aligned and unaligned rows and both statistics kernels; the gradient-layout cases leave the aligned dx kernel
    from x's side and from dx's side; the row, slab and col_stats cases give the partial counts and loop forms named below."""
    ld_off = lambda d, layout: R.nl_layout(torch.zeros(2, d), layout)[2:]
    cols = {(d, l): R.nl_case_facts(R.NL_COL_V, d, *ld_off(d, l), lddx=R.nl_lddx(d)[1]) for d in R.NL_COL_D for l in R.NL_LAYOUTS}
    assert {(f["Q"], f["aligned"]) for f in cols.values()} == {(q, a) for q in range(1, 6) for a in (True, False)}
    assert {(f["Q"], f["aligned_dx"]) for f in cols.values()} == {(q, a) for q in range(1, 6) for a in (True, False)}
    assert all(cols[(d, l)]["aligned"] == (l in ("padded", "block") or (l == "packed" and d % 4 == 0) or (l == "odd" and d % 4 == 1))
               for d in R.NL_COL_D for l in R.NL_LAYOUTS)
    for a, b in ((16, 17), (32, 33), (48, 49), (64, 65)):
        assert cols[(a, "padded")]["Q"] + 1 == cols[(b, "padded")]["Q"]
    assert cols[(64, "padded")]["CW"] == 64 and cols[(65, "padded")]["CW"] == 128
    grads = {(d, k, xl): R.nl_case_facts(R.NL_COL_V, d, *ld_off(d, xl), lddx=R.nl_lddx(d)[k])
             for d in R.NL_GRAD_D for k in range(3) for xl in R.NL_GRAD_X}
    for d in R.NL_GRAD_D:
        assert [grads[(d, k, "padded")]["aligned_dx"] for k in range(3)] == [d % 4 == 0, True, True]
        assert not any(grads[(d, k, "off1")]["aligned_dx"] for k in range(3)) and not grads[(d, 1, "off1")]["aligned"]
    assert [R.nl_partials(V) for V in (448, 512, 513)] == [7, 8, 9]
    strides = [R.nl_case_facts(V, d, ld) for V, d, ld in R.NL_STRIDE_CASES]
    assert [f["partials"] for f in strides] == [1024] * 3 and -(-70_001 // 64) > 1024
    assert [f["strides"] for f in strides] == [1, 2, 2]
    slabs = {(V, d): R.nl_case_facts(V, d, ld) for V, d, ld in R.NL_SLAB_CASES}
    assert [slabs[(V, 7)]["slabs"] for V in (2047, 2048, 2049, 8 * 2048 + 1, 64 * 2048 + 1)] == [1, 1, 2, 9, 65]
    assert slabs[(8 * 2048 + 1, 71)]["finish"] == {"tail"} and slabs[(64 * 2048 + 1, 7)]["finish"] == {"unrolled", "tail"}
    # the row loop of the statistics kernel on the last slab: a row group unrolls once it owns 8 rows -- all 4 groups (d = 7) at
    # 32 rows and the first of them at 29, both groups (d = 71) at 16 and the first at 15
    want7 = {2047: {"unrolled", "tail"}, 2048: {"unrolled"}, 2049: {"tail"}, 2063: {"tail"}, 2064: {"tail"}, 2065: {"tail"},
             2079: {"unrolled", "tail"}, 2080: {"unrolled"}, 2081: {"unrolled", "tail"}}
    want71 = {2047: {"unrolled", "tail"}, 2048: {"unrolled"}, 2049: {"tail"}, 2063: {"unrolled", "tail"}, 2064: {"unrolled"},
              2065: {"unrolled", "tail"}, 2079: {"unrolled", "tail"}, 2080: {"unrolled"}, 2081: {"unrolled", "tail"}}
    assert {V: slabs[(V, 7)]["slab_tail"] for V in want7} == want7
    assert {V: slabs[(V, 71)]["slab_tail"] for V in want71} == want71
    # (an fp32 lane's chain: the restatement's bound; the kernel's lanes sum in fp64 and answer to NL_STAT_COMBINE)
    fin = {r: R.nl_case_facts(R.NL_COLSTAT_V, 71, 72, stat_rows=r)["finish"] for r in R.NL_COLSTAT_ROWS}
    assert fin[8] == fin[9] == fin[56] == {"tail"} and fin[57] == fin[58] == fin[64] == {"unrolled"}
    assert fin[65] == {"unrolled", "tail"} and fin[2048] == fin[121] == {"unrolled"}       # (lane-group 0's view: partials 0, 8, .., 120)
    assert R.nl_n_s(7) == 516 and R.nl_n_s(71) == 1026
