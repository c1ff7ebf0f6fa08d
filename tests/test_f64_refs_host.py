"""The float64 references of tests/f64_refs.py, checked on the CPU: they reproduce the golden fixtures captured from
the reference's own Python, they are differentiable where the parity tests differentiate them, a tied pool maximum
belongs to its first pixel, and the inputs of every GPU case stay inside the caps on replaced / excluded elements."""
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
