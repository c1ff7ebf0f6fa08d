"""splatco_amd.adam.FusedAdam.step(visible=...) (csrc/adam.hip adam_rows_kernel, scr_adam_step_rows): visible rows get the
dense kernel's bits, every other row keeps its own whatever its gradient holds; several steps against the torch
restatement (tests/sparse_adam_ref.py); mixed groups; the optimizer surgery of densification; and two training steps whose
cameras look in opposite directions from the centre of the scene."""
import math
import types

import pytest
import torch

from sparse_adam_ref import SparseAdamRef
from splatco_amd.adam import FusedAdam

SIZES = (1, 5, 341, 342, 1023, 1025, 4097)      # 341 x 3 = 1023 and 342 x 3 = 1026 lie around the workgroup's 1024 elements


def _tensors(N, dev, seed):
    """The row-sparse tensors of one case: widths 1 (as [N] and as [N,1]), 3, 6, 30 as [N,10,3], 32, 71, one that starts
    4 bytes into an allocation (the scalar path), an empty one, and 26 more of width 2 so that the group needs a second
    launch (ADAM_MAX = 24).  Returns a factory of identical copies."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    shapes = [(N,), (N, 1), (N, 3), (N, 6), (N, 10, 3), (N, 32), (N, 71), (N, 0)] + [(N, 2)] * 26
    base = [torch.randn(s, generator=g) for s in shapes]
    off = torch.randn(N * 3 + 1, generator=g)

    def make():
        ps = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
        ps.append(torch.nn.Parameter(off.clone().to(dev)[1:].view(N, 3)))
        assert ps[-1].data_ptr() % 16 == 4 and ps[-1].is_contiguous()
        return ps
    return make


def _masks(N, dev):
    """name -> mask.  `runs`: rows [3,9), [341,343), [1021,1030) and [N-3,N-1): for every width of _tensors some run starts
    or ends inside a float4 and one crosses a multiple of 1024 elements (width 3: 341 x 3 = 1023; width 6: 2046..2057;
    width 30: 10230..10289; width 71: 72491..73129 around 71 x 1024; width 1: 1021..1029)."""
    z = lambda dtype=torch.bool: torch.zeros(N, dtype=dtype, device=dev)
    out = {"ones": ~z(), "zeros": z()}
    for name, r in (("first", 0), ("last", N - 1), ("middle", N // 2)):
        out[name] = z()
        out[name][r] = True
    out["alternating"] = z()
    out["alternating"][::2] = True
    out["runs"] = z()
    for a, b in ((3, 9), (341, 343), (1021, 1030), (N - 3, N - 1)):
        out["runs"][max(a, 0):max(min(b, N), 0)] = True
    rnd = torch.rand(N, generator=torch.Generator().manual_seed(N)) < 0.3
    out["random"] = rnd.to(dev)
    out["random_u8"] = (rnd.to(torch.uint8) * (2 + 253 * (torch.arange(N) % 2).to(torch.uint8))).to(dev)      # 0 / 2 / 255
    out["ones_u8"] = torch.full((N,), 128, dtype=torch.uint8, device=dev)
    return out


def _snapshot(opt, ps):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), float(opt.state[p]["step"]))
            for p in ps]


def _restore(opt, ps, snap):
    for p, (a, m, v, t) in zip(ps, snap):
        p.data.copy_(a)
        opt.state[p]["exp_avg"].copy_(m)
        opt.state[p]["exp_avg_sq"].copy_(v)
        opt.state[p]["step"].fill_(t)


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_visible_rows_get_the_dense_kernels_bits_and_the_others_keep_theirs(N):
    """From one state (two dense steps in), one dense step gives the reference bits; the same state stepped with a mask
    must hold those bits on the visible rows and the bits from before on every other row -- parameter and both moments, all
    widths, masks of both dtypes with values other than 1."""
    dev = torch.device("cuda:0")
    ps = _tensors(N, dev, seed=N)()
    opt = FusedAdam([{"params": ps, "lr": 1e-2, "row_sparse": True}], eps=1e-15)
    gen = torch.Generator(device=dev).manual_seed(N + 1)
    grads = [[torch.randn(p.shape, device=dev, generator=gen) * 10.0 ** ((i % 5) - 3) for i, p in enumerate(ps)] for _ in range(3)]
    for k in range(2):
        for p, g in zip(ps, grads[k]):
            p.grad = g.clone()
        opt.step()
    before = _snapshot(opt, ps)
    for p, g in zip(ps, grads[2]):
        p.grad = g.clone()
    opt.step()
    dense = _snapshot(opt, ps)
    for name, mask in _masks(N, dev).items():
        _restore(opt, ps, before)
        for p, g in zip(ps, grads[2]):
            p.grad = g.clone()                 # (a fresh copy: nothing may depend on what a step leaves in the gradient)
        opt.step(visible=mask)
        vis = mask != 0
        for i, (p, b, d) in enumerate(zip(ps, before, dense)):
            got = (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
            assert float(opt.state[p]["step"]) == d[3] == 3.0
            for what, x, xb, xd in zip(("param", "exp_avg", "exp_avg_sq"), got, b, d):
                where = f"mask {name}, tensor {i} {tuple(p.shape)}, {what}"
                assert torch.equal(_bits(x[vis]), _bits(xd[vis])), where + ": a visible row differs from the dense step"
                assert torch.equal(_bits(x[~vis]), _bits(xb[~vis])), where + ": an invisible row changed"
                if name in ("ones", "ones_u8"):
                    assert torch.equal(_bits(x), _bits(xd)), where
        if name != "zeros" and N > 1:
            assert any(not torch.equal(p.detach(), b[0]) for p, b in zip(ps, before))     # something did move


@pytest.mark.gpu
@pytest.mark.parametrize("N", (5, 342, 4097))
def test_invisible_rows_keep_their_bits_whatever_they_and_their_gradients_hold(N):
    """Invisible rows of parameter and moments hold a NaN with a payload, -0.0, a denormal and 1e30, their gradients NaN and
    +-Inf: their int32 images are the same after the step, and no visible row holds a NaN."""
    dev = torch.device("cuda:0")
    ps = _tensors(N, dev, seed=100 + N)()
    opt = FusedAdam([{"params": ps, "lr": 1e-2, "row_sparse": True}], eps=1e-15)
    gen = torch.Generator(device=dev).manual_seed(7)
    for p in ps:
        p.grad = torch.randn(p.shape, device=dev, generator=gen)
    opt.step()                                                       # moments exist and are ordinary numbers
    sentinels = torch.tensor([0x7fc12345, -0x80000000, 0x00000123, 0x7149f2ca], dtype=torch.int32, device=dev)   # NaN+payload, -0.0, denormal, 1e30
    assert sentinels.view(torch.float32)[3] == 1e30 and sentinels.view(torch.float32)[1].signbit()
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")], device=dev)
    for name, mask in _masks(N, dev).items():
        if name in ("ones", "ones_u8"):
            continue
        vis = mask != 0
        images = []
        for k, p in enumerate(ps):
            st = opt.state[p]
            p.grad = torch.randn(p.shape, device=dev, generator=gen)
            for j, x in enumerate((p.data, st["exp_avg"], st["exp_avg_sq"])):
                x[vis] = torch.rand_like(x[vis]) + 0.5                # ordinary values on the visible rows
                fill = sentinels[(torch.arange(x[~vis].numel(), device=dev) + j + k) % 4].view(x[~vis].shape)
                _bits(x)[~vis] = fill                                 # (x is contiguous: a view, written in place)
            g_inv = p.grad[~vis]
            p.grad[~vis] = bad[torch.arange(g_inv.numel(), device=dev) % 3].view(g_inv.shape)
            images.append([_bits(x).clone() for x in (p.data, st["exp_avg"], st["exp_avg_sq"])])
        opt.step(visible=mask)
        for i, (p, img) in enumerate(zip(ps, images)):
            st = opt.state[p]
            for what, x, xb in zip(("param", "exp_avg", "exp_avg_sq"), (p.data, st["exp_avg"], st["exp_avg_sq"]), img):
                where = f"mask {name}, tensor {i} {tuple(p.shape)}, {what}"
                assert torch.equal(_bits(x)[~vis], xb[~vis]), where + ": an invisible row changed"
                assert not x[vis].isnan().any() and x[vis].isfinite().all(), where + ": a visible row caught a NaN / Inf"
                if x[vis].numel():
                    assert not torch.equal(_bits(x)[vis], xb[vis]), where + ": the visible rows were not stepped"


def _multi_step(dev, make, n_rows, kind):
    """12 steps: a mask that changes every step, gradients from 1e-4 to 1e2, the learning rates halved at step 6, one
    parameter without a gradient in every third step, one dense group beside two row-sparse ones."""
    ps = make()
    dense = [torch.nn.Parameter(torch.linspace(-1, 1, 777, device=dev))]
    groups = [{"params": ps[:4], "lr": 1e-2, "row_sparse": True}, {"params": ps[4:], "lr": 3e-4, "row_sparse": True},
              {"params": dense, "lr": 1e-3}]
    opt = FusedAdam(groups, lr=0.0, eps=1e-15) if kind == "ours" else SparseAdamRef(groups, eps=1e-15)
    gen = torch.Generator(device=dev).manual_seed(3)
    mgen = torch.Generator().manual_seed(4)
    for it in range(12):
        for i, p in enumerate(ps + dense):
            if i == 2 and it % 3 == 0:
                p.grad = None
                continue
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 10.0 ** ((i % 7) - 4)
        if it == 6:
            for grp in opt.param_groups:
                grp["lr"] *= 0.5
        mask = (torch.rand(n_rows, generator=mgen) < (0.1, 0.5, 0.9)[it % 3]).to(dev)
        opt.step(visible=mask)
    return ps + dense, opt


@pytest.mark.gpu
def test_twelve_masked_steps_match_the_torch_restatement_and_repeat_bit_for_bit():
    dev = torch.device("cuda:0")
    N = 1025
    make = _tensors(N, dev, seed=11)
    pa, ours = _multi_step(dev, make, N, "ours")
    pb, ref = _multi_step(dev, make, N, "ref")
    for i, (a, b) in enumerate(zip(pa, pb)):
        # the tolerances of test_fused_adam_matches_torch_adam
        torch.testing.assert_close(a, b, rtol=2e-6, atol=2e-7, msg=lambda m: f"param {i} {tuple(a.shape)}: {m}")
        sa, sb = ours.state[a], ref.state[b]
        assert float(sa["step"]) == float(sb["step"]) == (8.0 if i == 2 else 12.0)
        if a.numel():
            assert float((sa["exp_avg"] - sb["exp_avg"]).abs().max()) <= 2e-6 * float(sb["exp_avg"].abs().max()), i
        torch.testing.assert_close(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=2e-6, atol=1e-30)
    pc, again = _multi_step(dev, make, N, "ours")
    for a, c in zip(pa, pc):
        assert torch.equal(a, c) and torch.equal(ours.state[a]["exp_avg"], again.state[c]["exp_avg"])
        assert torch.equal(ours.state[a]["exp_avg_sq"], again.state[c]["exp_avg_sq"])


@pytest.mark.gpu
def test_a_dense_group_beside_a_row_sparse_one_takes_the_dense_step():
    dev = torch.device("cuda:0")
    N = 342
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(N, 6, generator=g), torch.randn(N, 10, 3, generator=g), torch.randn(N, generator=g), torch.randn(2050, generator=g)]
    grads = [[torch.randn(b.shape, generator=g).to(dev) for b in base] for _ in range(3)]
    mask = (torch.rand(N, generator=g) < 0.4).to(dev)
    out = []
    for masked in (False, True):
        ps = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
        # the third tensor has N elements and sits in the DENSE group: its first dimension must not make it row-sparse
        opt = FusedAdam([{"params": ps[:2], "lr": 1e-2, "row_sparse": True}, {"params": ps[2:], "lr": 1e-3}], eps=1e-15)
        for gs in grads:
            for p, gr in zip(ps, gs):
                p.grad = gr.clone()
            opt.step(visible=mask if masked else None)
        out.append((ps, opt))
    (pd, od), (pm, om) = out
    for d, m in zip(pd[2:], pm[2:]):
        assert torch.equal(_bits(d), _bits(m)) and torch.equal(_bits(od.state[d]["exp_avg"]), _bits(om.state[m]["exp_avg"]))
        assert torch.equal(_bits(od.state[d]["exp_avg_sq"]), _bits(om.state[m]["exp_avg_sq"]))
    for d, m in zip(pd[:2], pm[:2]):
        assert torch.equal(d[mask], m[mask]) and not torch.equal(d[~mask], m[~mask])
    # a group without the key (as one loaded from a torch state_dict) is a dense group: with it gone from the only group
    # that had it, a mask is refused rather than ignored
    om.param_groups[0].pop("row_sparse")
    with pytest.raises(ValueError, match="row_sparse"):
        om.step(visible=mask)


@pytest.mark.gpu
def test_masked_step_after_densifier_surgery_equals_the_dense_twin_on_visible_rows():
    """adjust_anchor grows / prunes the per-anchor parameters and their moments inside an optimizer whose groups are
    row-sparse (the key rides along), then a step with a mask of the NEW anchor count: visible rows as the dense twin's,
    the others untouched."""
    from splatco_amd.densify import AnchorDensifier
    from splatco_amd.synthetic import synthetic_anchor_model
    dev = torch.device("cuda:0")
    out = []
    for masked in (False, True):
        pc = synthetic_anchor_model(20_000, 9, dev, plane_size=64)
        groups = [{"params": [getattr(pc, "_" + n)], "lr": 1e-3, "name": n, "row_sparse": True}
                  for n in ("anchor", "offset", "anchor_feat", "scaling")]
        opt = FusedAdam(groups, eps=1e-15)
        den = AnchorDensifier(pc, opt, voxel_size=0.01, seed=5)
        gen = torch.Generator(device=dev).manual_seed(6)
        for _ in range(2):
            for grp in groups:
                p = grp["params"][0]
                p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-2
            opt.step()
        N, k = pc._anchor.shape[0], pc.n_offsets
        den.offset_gradient_accum[:] = torch.rand(N * k, 1, device=dev, generator=gen)
        den.offset_denom[:] = 60
        den.opacity_accum[:] = torch.rand(N, 1, device=dev, generator=gen) * 2
        den.anchor_demon[:] = 100
        den.adjust_anchor(iteration=100, check_interval=100, grad_threshold=0.012)
        N2 = pc._anchor.shape[0]
        assert N2 != 20_000 and all(grp["row_sparse"] is True and grp["params"][0].shape[0] == N2 for grp in opt.param_groups)
        mask = (torch.rand(N2, device=dev, generator=gen) < 0.25)
        before = {}
        for grp in opt.param_groups:
            p = grp["params"][0]
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
            before[grp["name"]] = (p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
        if masked:
            with pytest.raises(ValueError, match="mask of"):
                opt.step(visible=torch.ones(20_000, dtype=torch.bool, device=dev))          # the old anchor count
        opt.step(visible=mask if masked else None)
        after = {grp["name"]: (grp["params"][0].detach().clone(), opt.state[grp["params"][0]]["exp_avg"].clone(),
                               opt.state[grp["params"][0]]["exp_avg_sq"].clone()) for grp in opt.param_groups}
        out.append((mask, before, after))
    (mask_d, before_d, dense), (mask, before, sparse) = out
    assert torch.equal(mask_d, mask) and 0 < int(mask.sum()) < mask.numel()
    for name in dense:
        for b_d, b, d, s in zip(before_d[name], before[name], dense[name], sparse[name]):
            assert torch.equal(b_d, b)                                   # the twins went through the same surgery
            assert torch.equal(_bits(s[mask]), _bits(d[mask])), name
            assert torch.equal(_bits(s[~mask]), _bits(b[~mask])), name
            assert not torch.equal(d[~mask], b[~mask]), name


@pytest.mark.gpu
def test_two_training_steps_with_cameras_looking_opposite_ways_step_only_what_they_see():
    """collaborative_step(sparse_adam=True) against a dense twin: a camera at the centre of the box looking along +x, then one
    looking along -x.  After step 1 the twins are bit-equal (zero moments and zero gradients leave an unseen row where it is
    under dense Adam too).  In step 2 the sparse run leaves every anchor the second camera does not see exactly where it was,
    while the dense twin moves the ones the FIRST camera saw along their momentum; what the second camera sees, and every
    MLP / plane parameter, is bit-equal between the twins."""
    from splatco_amd.cameras import look_at_camera
    from splatco_amd.renderer import prefilter_voxel
    from splatco_amd.synthetic import synthetic_anchor_model
    from splatco_amd.train_step import collaborative_step
    dev = torch.device("cuda:0")
    W, H = 160, 96
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
    bg = torch.ones(3, device=dev)
    cams = [look_at_camera(eye=(0.0, 0.0, 0.0), target=(x, 0.0, 0.0), up=(0, -1, 0), FoVx=math.radians(60), width=W, height=H,
                           uid=i).to(dev) for i, x in enumerate((1.0, -1.0))]
    gts = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(i)).to(dev) for i in range(2)]
    names = ("anchor", "offset", "anchor_feat", "scaling")

    def make():
        pc = synthetic_anchor_model(20_000, 7, dev, plane_size=64)
        groups = [{"params": [getattr(pc, "_" + n)], "lr": lr, "name": n, "row_sparse": True}
                  for n, lr in zip(names, (1e-5, 1e-3, 7.5e-3, 7e-3))]
        groups.append({"params": [p for n, p in pc.named_parameters() if not n.startswith("_") and p.requires_grad], "lr": 2e-3,
                       "name": "mlp_and_feat_planes"})
        return pc, FusedAdam(groups, eps=1e-15)

    def state_of(opt):
        """[[param, exp_avg, exp_avg_sq]] in group order (a parameter that never had a gradient has no moments yet)."""
        return [[p.detach().clone()] + [opt.state[p][k].clone() for k in ("exp_avg", "exp_avg_sq") if p in opt.state]
                for grp in opt.param_groups for p in grp["params"]]

    (pc_s, opt_s), (pc_d, opt_d) = make(), make()
    unions, states = [], []
    for k in range(2):
        with torch.no_grad():
            u_s, u_d = prefilter_voxel(cams[k], pc_s, pipe, bg), prefilter_voxel(cams[k], pc_d, pipe, bg)
        assert torch.equal(u_s, u_d)
        unions.append(u_s)
        before = state_of(opt_s) if k else None
        loss_s, _, _ = collaborative_step(pc_s, cams[k:k + 1], gts[k:k + 1], pipe, bg, optimizer=opt_s, sparse_adam=True)
        loss_d, _, _ = collaborative_step(pc_d, cams[k:k + 1], gts[k:k + 1], pipe, bg, optimizer=opt_d)
        assert torch.equal(loss_s, loss_d) and torch.isfinite(loss_s)
        states.append((before, state_of(opt_s), state_of(opt_d)))
    u1, u2 = unions
    N = u1.numel()
    # conditions of the test itself
    assert 0 < int(u1.sum()) < N and 0 < int(u2.sum()) < N
    only_first = u1 & ~u2
    assert int(only_first.sum()) >= 100
    # step 1: everything bit-equal to the dense twin
    _, s1, d1 = states[0]
    assert len(s1) == len(d1) > 4
    for a, b in zip(s1, d1):
        for x, y in zip(a, b):
            assert torch.equal(_bits(x), _bits(y))
    before2, s2, d2 = states[1]
    moved_dense, moved_sparse = 0, 0
    for i in range(4):                                   # the per-anchor groups, in the order of `names`
        assert len(before2[i]) == len(s2[i]) == len(d2[i])
        for xb, xs, xd in zip(before2[i], s2[i], d2[i]):
            assert torch.equal(_bits(xs[~u2]), _bits(xb[~u2])), names[i] + ": a row the second camera does not see changed"
            assert torch.equal(_bits(xs[u2]), _bits(xd[u2])), names[i] + ": a row the second camera sees differs from the dense twin"
        # (before2 is also the dense twin's state before step 2: the twins were bit-equal after step 1)
        moved_dense += int(((d2[i][0] != before2[i][0]).reshape(N, -1).any(dim=1) & only_first).sum())
        moved_sparse += int(((s2[i][0] != before2[i][0]).reshape(N, -1).any(dim=1) & u2).sum())
    assert moved_sparse > 0                              # the second camera's anchors were stepped
    for a, b in zip(s2[4:], d2[4:]):                     # MLP and plane parameters
        for x, y in zip(a, b):
            assert torch.equal(_bits(x), _bits(y))
    # the test discriminates: the dense twin DID move rows only the first camera saw (stale momentum)
    assert moved_dense > 0
