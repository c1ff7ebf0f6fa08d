"""GPU tests of the fused LDR-FLIP pass (csrc/flip.hip, splatco_amd.metrics.flip) against the float64 restatement of
tests/flip_restatement.py and the reference's own maps (tests/golden/flip.npz).

Bars (per pixel): max |d| <= 1e-3, 99.9 % of pixels <= 1e-4, mean |d| <= 1e-5 -- the reference's own float32 maps
meet them against the float64 restatement (tests/test_flip_host.py)."""
import os

import numpy as np
import pytest
import torch

import flip_restatement as fr

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flip.npz"))
MAX_BAR, P999_BAR, MEAN_BAR = 1e-3, 1e-4, 1e-5
DEV = "cuda:0"


def _check(got, want, what):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    assert d.max() <= MAX_BAR, (what, "max", d.max())
    assert np.quantile(d, 0.999) <= P999_BAR, (what, "p99.9", np.quantile(d, 0.999))
    assert d.mean() <= MEAN_BAR, (what, "mean", d.mean())


def _pair(i):
    return torch.tensor(GOLDEN[f"test{i}"], device=DEV), torch.tensor(GOLDEN[f"ref{i}"], device=DEV)


def _smooth_pair(N, H, W, seed, noise=0.05):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.rand(N, 3, H + 4, W + 4, device=DEV, generator=g)
    ref = torch.nn.functional.avg_pool2d(x, 5, stride=1)
    test = ref + noise * torch.randn(ref.shape, device=DEV, generator=g)
    return test.contiguous(), ref.contiguous()


@pytest.mark.parametrize("i", range(4))
def test_flip_matches_golden_and_restatement(i):
    from splatco_amd.metrics import flip
    t, r = _pair(i)
    mean, fmap = flip(t, r, return_map=True)
    torch.cuda.synchronize()
    want = fr.flip_map(t.cpu(), r.cpu()).numpy()
    _check(fmap.cpu().numpy(), want, f"pair {i} vs restatement")
    _check(fmap.cpu().numpy(), GOLDEN[f"map{i}"], f"pair {i} vs golden")
    assert abs(float(mean) - float(GOLDEN[f"mean{i}"])) <= MEAN_BAR
    assert mean.shape == () and fmap.shape == t.shape[1:]


def test_flip_1080p_pair_matches_restatement():
    from splatco_amd.metrics import flip
    t, r = _smooth_pair(1, 1080, 1920, seed=3)
    mean, fmap = flip(t, r, return_map=True)
    want = fr.flip_map(t, r)                       # float64 on the device
    _check(fmap.cpu().numpy(), want.cpu().numpy(), "1080p")
    assert abs(float(mean) - float(want.mean())) <= MEAN_BAR


@pytest.mark.parametrize("ppd", [40.0, 100.0])
def test_flip_other_pixels_per_degree(ppd):
    from splatco_amd.metrics import flip
    t, r = _smooth_pair(2, 75, 101, seed=5)
    mean, fmap = flip(t, r, pixels_per_degree=ppd, return_map=True)
    want = fr.flip_map(t, r, ppd=ppd)
    _check(fmap.cpu().numpy(), want.cpu().numpy(), f"ppd {ppd}")
    assert torch.allclose(mean.double().cpu(), want.mean((1, 2)).cpu(), rtol=0, atol=MEAN_BAR)


def test_flip_one_pixel_and_one_row_images():
    from splatco_amd.metrics import flip
    for H, W in ((1, 1), (1, 37), (29, 1), (2, 3)):
        t, r = _smooth_pair(1, H, W, seed=H * 100 + W, noise=0.2)
        mean, fmap = flip(t, r, return_map=True)
        _check(fmap.cpu().numpy(), fr.flip_map(t, r).cpu().numpy(), f"{H}x{W}")


def test_flip_batch_equals_single_calls_and_repeats_bitwise():
    from splatco_amd.metrics import flip
    t, r = _smooth_pair(3, 90, 70, seed=11)
    mean, fmap = flip(t, r, return_map=True)
    mean2, fmap2 = flip(t, r, return_map=True)
    assert torch.equal(mean, mean2) and torch.equal(fmap, fmap2)
    for n in range(3):
        m1, f1 = flip(t[n], r[n], return_map=True)
        assert torch.equal(m1, mean[n]) and torch.equal(f1, fmap[n])
    # the mean is the map's mean (the kernel sums in a fixed order, torch in its own)
    assert torch.allclose(fmap.double().mean((1, 2)), mean.double(), rtol=1e-6, atol=0)


def test_flip_quantize_is_the_8bit_round_trip():
    from splatco_amd.metrics import flip, quantize8
    t, r = _smooth_pair(2, 50, 66, seed=13)
    qt, qr = quantize8(t), quantize8(r)
    m_q, f_q = flip(t, r, quantize=True, return_map=True)
    m_p, f_p = flip(qt, qr, return_map=True)
    assert torch.equal(m_q, m_p) and torch.equal(f_q, f_p)
    _check(f_q.cpu().numpy(), fr.flip_map(qt, qr).cpu().numpy(), "quantized")
    _check(f_q.cpu().numpy(), fr.flip_map(t, r, quantize=True).cpu().numpy(), "quantize flag")
    m3, f3 = flip(GOLDEN_T3(), GOLDEN_R3(), quantize=True, return_map=True)        # already on the 8-bit grid
    _check(f3.cpu().numpy(), GOLDEN["map3"], "golden pre-quantized pair")


def GOLDEN_T3():
    return torch.tensor(GOLDEN["test3"], device=DEV)


def GOLDEN_R3():
    return torch.tensor(GOLDEN["ref3"], device=DEV)


def test_psnr_from_mse_equals_losses_psnr():
    from splatco_amd import losses
    from splatco_amd.metrics import flip_and_mse, psnr_from_mse
    t, r = _smooth_pair(3, 64, 80, seed=17)
    t = t.clamp(0, 1)
    _, mse = flip_and_mse(t, r)
    want = losses.psnr(t, r).reshape(-1)
    assert torch.allclose(psnr_from_mse(mse), want, rtol=0, atol=2e-4), (psnr_from_mse(mse), want)
    for i in range(3):   # golden pairs: the reference's psnr of the clamped pair
        a, b = _pair(i)
        _, mse = flip_and_mse(a, b)
        assert abs(float(psnr_from_mse(mse)) - float(GOLDEN[f"psnr{i}"])) <= 2e-4


def test_ssim_value_matches_losses_ssim_and_golden():
    from splatco_amd import losses
    from splatco_amd.metrics import ssim_value
    for i in range(4):
        a, b = (x.clamp(0, 1) for x in _pair(i))
        v = ssim_value(a, b)
        assert v.shape == () and v.is_cuda
        assert abs(float(v) - float(losses.ssim(a, b))) <= 1e-5
        assert abs(float(v) - float(GOLDEN[f"ssim{i}"])) <= 1e-5


def test_identical_images_score_zero():
    from splatco_amd.metrics import flip_and_mse
    t, _ = _smooth_pair(2, 40, 52, seed=19)
    mean, mse = flip_and_mse(t, t.clone())
    assert float(mean.abs().max()) <= 1e-6 and float(mse.abs().max()) == 0.0


def test_flip_refuses_bad_arguments():
    from splatco_amd.metrics import flip
    t, r = _smooth_pair(1, 20, 24, seed=23)
    for ppd in (0.5, 119.0, float("nan")):
        with pytest.raises(ValueError, match="pixels_per_degree"):
            flip(t, r, pixels_per_degree=ppd)
    with pytest.raises(ValueError):
        flip(t, r[:, :, :-1])                        # shape mismatch
    with pytest.raises(ValueError):
        flip(t[:, :2], r[:, :2])                     # not 3 channels
    with pytest.raises(ValueError):
        flip(t[0, 0], r[0, 0])                       # 2-D
    with pytest.raises(ValueError):
        flip(t[:, :, :0], r[:, :, :0])               # empty
    with pytest.raises(ValueError):
        flip(t.cpu(), r.cpu())                       # host tensors: no fallback
    with pytest.raises(TypeError):
        flip(t.double(), r.double())
    g = t.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="no backward"):
        flip(g, r)
    with torch.no_grad():
        assert flip(g, r).requires_grad is False
