"""Row-sparse Adam, everything that needs no device: the host-side validation of scr_adam_step_rows (include/splatco_raster.h),
the ABI version, the argument checks of FusedAdam.step(visible=...) and collaborative_step(sparse_adam=True), the torch
restatement the GPU tests compare against (tests/sparse_adam_ref.py) against torch.optim.Adam, and the state_dict of an
optimizer that never uses the feature."""
import pytest
import torch

from sparse_adam_ref import SparseAdamRef
from splatco_amd.adam import FusedAdam


def test_scr_adam_step_rows_rejects_bad_arguments_without_a_gpu():
    """Validated before anything is launched; each message names its argument."""
    from splatco_amd import _C
    lib = _C.lib
    err = lambda: lib.scr_last_error().decode()
    call = lambda n, t, mask, rows, b1=0.9, b2=0.999, eps=1e-15: lib.scr_adam_step_rows(n, t, mask, rows, b1, b2, eps, None)
    assert call(-1, None, None, 0) != 0 and "n_tensors" in err()
    assert call(1, None, 16, 4) != 0 and "tensors is NULL" in err()
    assert call(0, None, None, 0) == 0                                            # nothing to do
    t = (_C.AdamTensor * 2)()
    for x in t:
        x.numel, x.step_size, x.bias_correction2_sqrt = 12, 1e-2, 0.03
    assert call(2, t, 16, 4) != 0 and "NULL tensor" in err()
    for x in t:
        x.param = x.grad = x.exp_avg = x.exp_avg_sq = 16                          # non-null: the checks below come first
    for b1, b2, eps in ((1.0, 0.999, 1e-15), (0.9, -0.1, 1e-15), (0.9, 0.999, -1.0)):
        assert call(2, t, 16, 4, b1, b2, eps) != 0 and "beta" in err()
    t[1].step_size = float("inf")                                                 # step 0: lr / (1 - beta1^0) does not exist
    assert call(2, t, 16, 4) != 0 and "step_size" in err() and "bias" in err()
    t[1].step_size = float("nan")
    assert call(2, t, 16, 4) != 0 and "step_size" in err()
    t[1].step_size, t[1].bias_correction2_sqrt = 1e-2, 0.0
    assert call(2, t, 16, 4) != 0 and "bias_correction2_sqrt" in err()
    t[1].bias_correction2_sqrt = 0.03
    assert call(2, t, 16, -1) != 0 and "n_rows" in err()
    assert call(2, t, None, 4) != 0 and "row_mask" in err()
    assert call(2, t, 16, 5) != 0 and "multiple of n_rows" in err()               # 12 elements in 5 rows
    t[1].numel = 13
    assert call(2, t, 16, 4) != 0 and "multiple of n_rows" in err()               # the second tensor
    assert call(2, t, None, 0) != 0 and "multiple of n_rows" in err()             # elements but no rows
    t[1].numel = 1 << 32
    assert call(2, t, 16, 4) != 0 and "2^32" in err()
    t[0].numel = t[1].numel = 0
    assert call(2, t, None, 0) == 0                                               # no rows, no elements: nothing launched
    assert call(2, t, 16, 7) == 0                                                 # empty tensors of 7 rows: nothing launched


def test_abi_version_is_33_in_binding_and_library():
    from splatco_amd import _C
    assert _C.ABI_VERSION >= 33 and _C.lib.scr_abi_version() == _C.ABI_VERSION
    assert "scr_adam_step_rows" in _C.SYMBOLS


def test_step_visible_argument_checks_need_no_device():
    N = 6
    p, q = torch.nn.Parameter(torch.zeros(N, 3)), torch.nn.Parameter(torch.zeros(5))
    opt = FusedAdam([{"params": [p], "row_sparse": True}, {"params": [q]}], lr=1e-3)
    p.grad, q.grad = torch.ones(N, 3), torch.ones(5)
    for bad in (torch.ones(N), torch.ones(N, dtype=torch.int32), torch.ones(N, dtype=torch.int64), [True] * N):
        with pytest.raises(ValueError, match="bool or torch.uint8"):
            opt.step(visible=bad)
    for bad in (torch.ones(N, 1, dtype=torch.bool), torch.ones((), dtype=torch.bool), torch.ones(2 * N, dtype=torch.uint8)[::2]):
        with pytest.raises(ValueError, match=r"contiguous \[N\]"):
            opt.step(visible=bad)
    for n in (N - 1, N + 1, 0):
        with pytest.raises(ValueError, match="mask of"):
            opt.step(visible=torch.ones(n, dtype=torch.bool))
    with pytest.raises(ValueError, match="lives on"):
        opt.step(visible=torch.ones(N, dtype=torch.bool, device="meta"))
    # nothing was stepped by the refused calls
    assert len(opt.state) == 0
    # a scalar parameter cannot be row-sparse
    s = torch.nn.Parameter(torch.zeros(()))
    with pytest.raises(ValueError, match="mask of"):
        FusedAdam([{"params": [s], "row_sparse": True}]).step(visible=torch.ones(1, dtype=torch.bool))
    # visible without a row-sparse group: refused, not a silent dense step -- also for groups that carry the key as False
    # or (as after load_state_dict of a torch optimizer) not at all
    for groups in ([{"params": [p]}, {"params": [q]}], [{"params": [p], "row_sparse": False}]):
        with pytest.raises(ValueError, match="row_sparse"):
            FusedAdam(groups, lr=1e-3).step(visible=torch.ones(N, dtype=torch.bool))
    # there is no CPU path behind a well-formed call either
    with pytest.raises(ValueError, match="no CPU path"):
        opt.step(visible=torch.ones(N, dtype=torch.bool))


def test_state_dict_without_row_sparse_has_todays_keys():
    p = torch.nn.Parameter(torch.zeros(4))
    opt = FusedAdam([{"params": [p], "lr": 1e-2, "name": "a"}], eps=1e-15)
    ref = torch.optim.Adam([{"params": [p], "lr": 1e-2, "name": "a"}], eps=1e-15)
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and len(sd["param_groups"]) == 1
    assert set(sd["param_groups"][0]) == {"params", "lr", "name", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach",
                                          "capturable", "differentiable", "fused", "decoupled_weight_decay"}
    assert set(sd["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])
    assert "row_sparse" not in opt.defaults
    # a group that asks for it keeps the key through state_dict, one loaded from torch's optimizer does not grow it
    marked = FusedAdam([{"params": [p], "row_sparse": True}])
    assert marked.state_dict()["param_groups"][0]["row_sparse"] is True
    opt.load_state_dict(ref.state_dict())
    assert "row_sparse" not in opt.param_groups[0]


def test_collaborative_step_sparse_adam_refuses_other_optimizers_and_ranks(monkeypatch):
    from splatco_amd import train_step
    from splatco_amd.adam import ShardedFusedAdam
    p = torch.nn.Parameter(torch.zeros(4, 3))
    args = (None, [], [], None, None)                       # refused before the model or a view is looked at
    with pytest.raises(TypeError, match="FusedAdam"):
        train_step.collaborative_step(*args, optimizer=torch.optim.Adam([p]), sparse_adam=True)
    with pytest.raises(TypeError, match="FusedAdam"):
        train_step.collaborative_step(*args, optimizer=None, sparse_adam=True)
    with pytest.raises(NotImplementedError, match="row origin"):
        train_step.collaborative_step(*args, optimizer=object.__new__(ShardedFusedAdam), sparse_adam=True)
    monkeypatch.setattr(train_step, "world_info", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="SAME union"):
        train_step.collaborative_step(*args, optimizer=FusedAdam([{"params": [p], "row_sparse": True}]), sparse_adam=True)


def test_restatement_with_all_ones_mask_is_torch_adam():
    """tests/sparse_adam_ref.py with every row visible against torch.optim.Adam(foreach=False, fused=False) on the CPU, several
    steps, a learning-rate change and a parameter that gets no gradient in some steps (tolerances: test_gpu_adam.py's)."""
    g = torch.Generator().manual_seed(0)
    N = 37
    shapes = [(N,), (N, 3), (N, 10, 3), (N, 32), (N, 6)]
    base = [torch.randn(s, generator=g) for s in shapes] + [torch.randn(11, generator=g)]

    def make():
        ps = [torch.nn.Parameter(b.clone()) for b in base]
        return ps, [{"params": ps[:3], "lr": 1e-2, "row_sparse": True}, {"params": ps[3:5], "lr": 3e-4, "row_sparse": True},
                    {"params": ps[5:], "lr": 1e-3}]
    pa, ga = make()
    pb, gb = make()
    ours = SparseAdamRef(ga, eps=1e-15)
    ref = torch.optim.Adam([{k: v for k, v in grp.items() if k != "row_sparse"} for grp in gb], lr=0.0, eps=1e-15, foreach=False,
                           fused=False)
    ones = torch.ones(N, dtype=torch.bool)
    for it in range(8):
        for i, (a, b) in enumerate(zip(pa, pb)):
            if i == 1 and it % 3 == 0:
                a.grad = b.grad = None
                continue
            grad = torch.randn(a.shape, generator=g) * 10.0 ** ((i % 7) - 4)
            a.grad, b.grad = grad.clone(), grad.clone()
        if it == 4:
            for grp in ours.param_groups + ref.param_groups:
                grp["lr"] *= 0.5
        ours.step(ones)
        ref.step()
    for a, b in zip(pa, pb):
        torch.testing.assert_close(a, b, rtol=2e-6, atol=2e-7)
        assert float(ours.state[a]["step"]) == float(ref.state[b]["step"])
        torch.testing.assert_close(ours.state[a]["exp_avg"], ref.state[b]["exp_avg"], rtol=2e-6, atol=2e-7)
        torch.testing.assert_close(ours.state[a]["exp_avg_sq"], ref.state[b]["exp_avg_sq"], rtol=2e-6, atol=2e-7)
    # and a masked step leaves the other rows alone, bit for bit
    vis = torch.zeros(N, dtype=torch.uint8)
    vis[::3] = 5
    before = [a.detach().clone() for a in pa]
    for a in pa:
        a.grad = torch.full_like(a, float("nan"))
    for a in pa[:5]:
        a.grad[vis != 0] = 1.0
    ours.step(vis)
    for a, b in zip(pa[:5], before[:5]):
        assert torch.equal(a[vis == 0], b[vis == 0]) and not torch.equal(a[vis != 0], b[vis != 0]) and not a[vis != 0].isnan().any()
    assert pa[5].isnan().all()                              # the dense group saw its whole gradient
