"""Depth supervision, everything that needs no device: the C-ABI surface of scr_depth_loss_* (include/splatco_raster.h) and
its argument checks, the restatement the GPU tests compare against (tests/depth_loss_ref.py) against the closed-form gradient
of the definition, the CPU fallback of splatco_amd.losses.depth_loss against the restatement, and the definition's edge
cases: an exact affine target, holes that hold NaN / Inf, degenerate fits."""
import inspect
import os
import re

import pytest
import torch

from depth_loss_ref import closed_form_grads, depth_loss_ref, recipe, valid_pixels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scr_depth_loss_scratch_bytes", "scr_depth_loss_forward", "scr_depth_loss_backward")


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def test_binding_and_header_declare_the_three_entry_points_at_abi_35():
    from splatco_amd import _C
    hdr = open(os.path.join(ROOT, "include", "splatco_raster.h")).read()
    assert _C.ABI_VERSION >= 35 and _C.lib.scr_abi_version() == _C.ABI_VERSION
    assert f"#define SCR_ABI_VERSION {_C.ABI_VERSION}" in hdr
    sig = {s[0]: s for s in _C.SIGNATURES}
    for name in NAMES:
        assert hasattr(_C.lib, name) and name in _C.SYMBOLS and re.search(rf"\b{name}\s*\(", hdr), name
    # in header order, behind the pair-L1 family
    assert _C.SYMBOLS[_C.SYMBOLS.index("scr_pair_l1_backward") + 1:][:3] == list(NAMES)
    assert len(sig["scr_depth_loss_forward"]) - 2 == 13 and len(sig["scr_depth_loss_backward"]) - 2 == 14
    assert sig["scr_depth_loss_forward"][11] is _C.f32 and sig["scr_depth_loss_backward"][10] is _C.f32       # min_alpha


def test_scratch_bytes_is_positive_and_monotone_in_the_pixel_count():
    from splatco_amd import _C
    f = _C.lib.scr_depth_loss_scratch_bytes
    sizes = [(1, 1), (1, 4096), (1, 4097), (52, 70), (513, 512), (1080, 1920), (4320, 7680), (46340, 46340), (1, 2 ** 31 - 1)]
    got = [f(h, w) for h, w in sizes]
    assert all(b > 0 and b % 256 == 0 for b in got)
    assert got == sorted(got) and got[0] < got[4] < got[5] < got[6] < got[-1]
    assert f(1080, 1920) == f(1920, 1080)                  # a function of H W alone
    assert got[5] < (1 << 16)                              # 1080p: a few records, not a map


def test_c_abi_rejects_bad_arguments_without_a_device():
    """Validated before anything is launched; 16 stands for any non-null device address (never dereferenced on the host)."""
    from splatco_amd import _C
    lib = _C.lib
    err = lambda: lib.scr_last_error().decode()
    ok = dict(H=4, W=5, depth=16, alpha=16, target=16, mask=None, mask_kind=0, mode=0, align=1, min_alpha=0.5, scratch=16, out=16,
              g=16, d_depth=16, d_alpha=16)

    def fwd(**kw):
        a = {**ok, **kw}
        return lib.scr_depth_loss_forward(a["H"], a["W"], a["depth"], a["alpha"], a["target"], a["mask"], a["mask_kind"], a["mode"],
                                          a["align"], a["min_alpha"], a["scratch"], a["out"], None)

    def bwd(**kw):
        a = {**ok, **kw}
        return lib.scr_depth_loss_backward(a["H"], a["W"], a["depth"], a["alpha"], a["target"], a["mask"], a["mask_kind"], a["mode"],
                                           a["min_alpha"], a["scratch"], a["g"], a["d_depth"], a["d_alpha"], None)

    for call, ptrs in ((fwd, ("depth", "alpha", "target", "scratch", "out")), (bwd, ("depth", "alpha", "target", "scratch", "g"))):
        for name in ptrs:
            assert call(**{name: None}) != 0 and "NULL" in err(), name
        for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(W=-1)):
            assert call(**kw) != 0 and "image size" in err(), kw
        assert call(H=65536, W=32768) != 0 and "2^31" in err()
        for mode in (-1, 2, 7):
            assert call(mode=mode) != 0 and "mode" in err()
        for kind in (-1, 3):
            assert call(mask_kind=kind, mask=16) != 0 and "mask_kind" in err()
        for kind in (1, 2):
            assert call(mask_kind=kind, mask=None) != 0 and "mask is NULL" in err()
        for bad in (-0.25, float("nan"), float("inf"), float("-inf")):
            assert call(min_alpha=bad) != 0 and "min_alpha" in err(), bad
    # both gradient maps absent: nothing to do, nothing launched
    assert bwd(d_depth=None, d_alpha=None) == 0


def test_python_surface():
    from splatco_amd import losses, train_step
    p = inspect.signature(losses.depth_loss).parameters
    assert list(p) == ["depth", "alpha", "target", "mask", "mode", "align", "min_alpha", "return_stats"]
    assert (p["mask"].default, p["mode"].default, p["align"].default, p["min_alpha"].default, p["return_stats"].default) == \
        (None, "inverse", True, 0.5, False)
    assert "detached" in losses.depth_loss.__doc__
    q = inspect.signature(train_step.collaborative_step).parameters
    assert [q[k].default for k in ("depth_targets", "depth_masks", "depth_weight", "depth_options")] == [None, None, 0.0, None]
    assert list(q)[-4:] == ["depth_targets", "depth_masks", "depth_weight", "depth_options"]


def test_depth_loss_refuses_mismatched_arguments_before_any_launch():
    from splatco_amd.losses import depth_loss
    D, A, g, m = recipe(6, 7, 0)
    with pytest.raises(ValueError, match="mode"):
        depth_loss(D, A, g, m, mode="disparity")
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_alpha"):
            depth_loss(D, A, g, m, min_alpha=bad)
    with pytest.raises(ValueError, match="alpha"):
        depth_loss(D, A[:5], g, m)
    with pytest.raises(ValueError, match="target"):
        depth_loss(D, A, g.t(), m)
    with pytest.raises(ValueError, match="mask"):
        depth_loss(D, A, g, m[:, :6])
    with pytest.raises(ValueError, match="target"):
        depth_loss(D, A, g.to("meta"), m)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        depth_loss(D[None], A[None], g[None], m[None])


def test_collaborative_step_depth_error_cases_need_no_device():
    from splatco_amd import train_step
    args = (None, [1, 2], [None, None], None, None)         # refused before the model or a view is looked at
    with pytest.raises(ValueError, match="depth_targets"):
        train_step.collaborative_step(*args, depth_weight=0.3)
    with pytest.raises(ValueError, match="1 depth_targets for 2 views"):
        train_step.collaborative_step(*args, depth_weight=0.3, depth_targets=[torch.zeros(2, 2)])
    with pytest.raises(ValueError, match="3 depth_masks for 2 views"):
        train_step.collaborative_step(*args, depth_weight=0.3, depth_targets=[torch.zeros(2, 2)] * 2, depth_masks=[None] * 3)


CASES = [(mode, align, mk) for mode in ("inverse", "expected") for align in (True, False) for mk in (None, "f32", "u8", "bool")]


@pytest.mark.parametrize("mode,align,mk", CASES)
def test_cpu_fallback_equals_the_restatement(mode, align, mk):
    """Value, (s, t, n_valid) and both gradients; 37 x 7 and 52 x 70.  Bar 2e-6: the fallback forms the division's derivative
    in float32 (two roundings per pixel), the sums in float64."""
    from splatco_amd.losses import depth_loss
    for H, W in ((7, 37), (52, 70)):
        D, A, g, m = recipe(H, W, 1, mask_kind=mk, mode=mode, line=(1.7, -0.08) if align else (1.0, 0.0))
        D.requires_grad_()
        A.requires_grad_()
        ref = depth_loss_ref(D, A, g, m, mode, align)
        assert int(ref["n_valid"]) >= 64 and float(ref["residual"][ref["valid"]].abs().min()) > 1e-3
        rd, ra = torch.autograd.grad(ref["loss"], (D, A))
        loss, stats = depth_loss(D, A, g, m, mode=mode, align=align, return_stats=True)
        assert loss.dtype == torch.float32 and stats.shape == (3,) and not stats.requires_grad
        gd, ga = torch.autograd.grad(loss, (D, A))
        loss, ref["loss"] = loss.detach(), ref["loss"].detach()
        assert abs(float(loss) - float(ref["loss"])) <= 2e-6 * float(ref["loss"])
        assert abs(float(stats[0]) - float(ref["s"])) <= 2e-6 * abs(float(ref["s"]))
        assert abs(float(stats[1]) - float(ref["t"])) <= 2e-6 * max(abs(float(ref["t"])), 1e-2)
        assert int(stats[2]) == int(ref["n_valid"])
        assert rel(gd, rd) <= 2e-6 and rel(ga, ra) <= 2e-6
        holes = ~ref["valid"]
        assert not gd[holes].any() and not ga[holes].any()
        if not align:
            assert float(stats[0]) == 1.0 and float(stats[1]) == 0.0
        # without return_stats: the loss alone
        assert torch.equal(depth_loss(D, A, g, m, mode=mode, align=align), loss)


def test_fallback_sends_gradients_to_target_and_mask_when_they_want_one():
    from splatco_amd.losses import depth_loss
    D, A, g, m = recipe(9, 11, 2)
    g.requires_grad_()
    m.requires_grad_()
    depth_loss(D, A, g, m).backward()
    valid = valid_pixels(D, A, g.detach(), m.detach(), 0.5)
    assert g.grad is not None and m.grad is not None and g.grad[valid].abs().min() > 0 and not g.grad[~valid].any()


@pytest.mark.parametrize("mode", ("inverse", "expected"))
@pytest.mark.parametrize("align", (True, False))
def test_restatement_gradient_is_the_closed_form_and_passes_gradcheck(mode, align):
    """float64 inputs bounded away from the kinks (|residual| >= 0.05 by construction, alpha >= 0.6 > min_alpha, depth > 0,
    mask weights >= 0.25 or exactly 0); (s, t) detached, so the gradient is the definition's q formulas."""
    D, A, g, m = (x.double() for x in recipe(5, 9, 3, mode=mode, line=(1.7, -0.08) if align else (1.0, 0.0)))
    z = D / A
    A = 0.6 + 0.4 * (A - 0.05) / 0.95                       # the same z, so the same p up to rounding and the same residuals
    D = (A * z).detach()
    D.requires_grad_()
    A.requires_grad_()
    ref = depth_loss_ref(D, A, g, m, mode, align)
    assert int(ref["n_valid"]) >= 20 and float(ref["residual"][ref["valid"]].abs().min()) > 1e-3
    gd, ga = torch.autograd.grad(2.5 * ref["loss"], (D, A))
    cd, ca = closed_form_grads(D.detach(), A.detach(), g, m, mode, ref["s"], ref["t"], g_up=2.5)
    assert rel(gd, cd) <= 1e-12 and rel(ga, ca) <= 1e-12
    assert not gd[~ref["valid"]].any() and not ga[~ref["valid"]].any()
    # numerical derivative with (s, t) held at the values of the fit
    s, t = float(ref["s"]), float(ref["t"])

    def f(D_, A_):
        p = A_ / D_ if mode == "inverse" else D_ / A_
        return (torch.where(ref["valid"], m, torch.zeros_like(m)) * (s * p + t - g).abs()).sum() / D_.numel()
    assert torch.autograd.gradcheck(f, (D, A), eps=1e-6, atol=1e-8, rtol=1e-6)
    nd, na = torch.autograd.grad(2.5 * f(D, A), (D, A))
    assert rel(gd, nd) <= 1e-12 and rel(ga, na) <= 1e-12


@pytest.mark.parametrize("mode", ("inverse", "expected"))
def test_an_affine_target_is_fitted_exactly(mode):
    from splatco_amd.losses import depth_loss
    D, A, g, m = recipe(20, 31, 4, mode=mode)
    a, b = 2.25, -0.4
    p = (A / D if mode == "inverse" else D / A).double()
    g = (a * p + b).float()
    ref = depth_loss_ref(D, A, g, m, mode, True)
    loss, stats = depth_loss(D, A, g, m, mode=mode, return_stats=True)
    for s, t, L in ((float(ref["s"]), float(ref["t"]), float(ref["loss"])), (float(stats[0]), float(stats[1]), float(loss))):
        # g is rounded to float32: 6e-8 relative on values up to 18, spread over the fit
        assert abs(s - a) <= 1e-6 and abs(t - b) <= 1e-6 and 0 <= L <= 1e-6


def _poisoned(mode, seed=5):
    """The recipe with every kind of hole written into pixels that were valid: NaN / +-Inf in each of the four maps, depth <= 0,
    alpha < min_alpha.  Returns the maps and the bool map of the poisoned pixels."""
    D, A, g, m = recipe(12, 17, seed, mode=mode)
    valid = valid_pixels(D, A, g, m, 0.5).flatten().nonzero().flatten()
    assert valid.numel() >= 40
    nan, inf = float("nan"), float("inf")
    D, A, g, m = D.flatten().clone(), A.flatten().clone(), g.flatten().clone(), m.flatten().clone()
    k = iter(valid.tolist())
    hit = []
    for x in (D, A, g, m):
        for v in (nan, inf, -inf):
            i = next(k)
            x[i] = v
            hit.append(i)
    for v in (0.0, -1.5):
        i = next(k)
        D[i] = v
        hit.append(i)
    for v in (0.0, 0.4999):
        i = next(k)
        A[i] = v
        hit.append(i)
    i = next(k)                                            # everything at once
    D[i], A[i], g[i], m[i] = nan, inf, -inf, nan
    hit.append(i)
    bad = torch.zeros(12 * 17, dtype=torch.bool)
    bad[hit] = True
    r = lambda x: x.reshape(12, 17)
    return r(D), r(A), r(g), r(m), r(bad)


@pytest.mark.parametrize("mode", ("inverse", "expected"))
@pytest.mark.parametrize("align", (True, False))
def test_holes_with_nan_or_inf_leak_nowhere(mode, align):
    """An Inf mask WEIGHT is not a hole by the definition (m > 0): the +Inf written into the mask is the one poisoned pixel
    that stays valid, so it is kept out of this test's mask (the other mask poisons, NaN and -Inf, are holes)."""
    from splatco_amd.losses import depth_loss
    D, A, g, m, bad = _poisoned(mode)
    m = torch.where(m == float("inf"), torch.zeros_like(m), m)
    clean = recipe(12, 17, 5, mode=mode)
    m_clean = torch.where(bad, torch.zeros_like(m), clean[3])            # the same pixels masked out by hand
    want = depth_loss_ref(*clean[:3], m_clean, mode, align)
    for fn in ("ref", "fallback"):
        D_, A_ = D.clone().requires_grad_(), A.clone().requires_grad_()
        if fn == "ref":
            out = depth_loss_ref(D_, A_, g, m, mode, align)
            loss, s, t, n = out["loss"], float(out["s"]), float(out["t"]), int(out["n_valid"])
        else:
            loss, st = depth_loss(D_, A_, g, m, mode=mode, align=align, return_stats=True)
            s, t, n = float(st[0]), float(st[1]), int(st[2])
        gd, ga = torch.autograd.grad(loss, (D_, A_))
        loss = loss.detach()
        assert torch.isfinite(loss) and torch.isfinite(gd).all() and torch.isfinite(ga).all()
        assert not gd[bad].any() and not ga[bad].any()
        assert n == int(want["n_valid"]) and abs(float(loss) - float(want["loss"])) <= 2e-6 * float(want["loss"])
        assert abs(s - float(want["s"])) <= 2e-6 * abs(float(want["s"])) and abs(t - float(want["t"])) <= 2e-6


@pytest.mark.parametrize("mode", ("inverse", "expected"))
def test_degenerate_fits_fall_back_to_the_identity(mode):
    from splatco_amd.losses import depth_loss
    D, A, g, m = recipe(8, 9, 6, mode=mode)
    none = torch.zeros_like(m)
    one = none.clone()
    one[3, 4] = 1.0
    A1 = A.clone()
    A1[3, 4] = 0.9
    flat_D, flat_A = torch.full_like(D, 1.75), torch.full_like(A, 0.875)         # constant p
    for (D_, A_, m_, n_want) in ((D, A1, none, 0), (D, A1, one, 1), (flat_D, flat_A, None, 72)):
        D_ = D_.clone().requires_grad_()
        ref = depth_loss_ref(D_, A_, g, m_, mode, True)
        loss, st = depth_loss(D_, A_, g, m_, mode=mode, return_stats=True)
        (gd,) = torch.autograd.grad(loss, D_)
        loss, want = float(loss.detach()), float(ref["loss"].detach())
        assert st.tolist() == [1.0, 0.0, float(n_want)] and float(ref["s"]) == 1.0 and float(ref["t"]) == 0.0
        assert int(ref["n_valid"]) == n_want and abs(loss - want) <= 2e-6 * want
        if n_want == 0:
            assert loss == 0.0 and not gd.any()
