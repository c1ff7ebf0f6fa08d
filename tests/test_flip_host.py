"""CPU tests of the LDR-FLIP host side: the 1-D filters the HIP kernel receives (splatco_amd.metrics.flip_filters, from
the library's host code) rebuild the reference's 2-D kernels, and the float64 restatement of tests/flip_restatement.py
reproduces the reference's maps (tests/golden/flip.npz) within the bars the GPU tests hold the kernel to."""
import os

import numpy as np
import pytest
import torch

import flip_restatement as fr

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flip.npz"))
PAIRS = range(4)

# bars of tests/test_gpu_flip.py: per-pixel max |d|, the 99.9th percentile of |d|, the mean |d|
MAX_BAR, P999_BAR, MEAN_BAR = 1e-3, 1e-4, 1e-5


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_flip_filters_rebuild_the_golden_2d_kernels():
    from splatco_amd.metrics import DEFAULT_PPD, flip_filters
    f = flip_filters(DEFAULT_PPD)
    assert f["csf_radius"] == 10 and f["feature_radius"] == 9
    assert abs(f["cmax"] - float(GOLDEN["cmax"])) <= 1e-6 * float(GOLDEN["cmax"])
    assert abs(DEFAULT_PPD - float(GOLDEN["ppd"])) < 1e-12
    for name in ("a", "rg", "by1", "by2", "edge", "point", "gauss"):
        assert f[name].dtype == np.float64
        assert len(f[name]) == 2 * (f["csf_radius"] if name in ("a", "rg", "by1", "by2") else f["feature_radius"]) + 1
    # the golden kernels are binary32: 1e-7 of the kernel's largest weight is within their own rounding
    assert _rel(np.outer(f["a"], f["a"]), GOLDEN["csf_a"]) <= 1e-7
    assert _rel(np.outer(f["rg"], f["rg"]), GOLDEN["csf_rg"]) <= 1e-7
    by = f["by_c1"] * np.outer(f["by1"], f["by1"]) + f["by_c2"] * np.outer(f["by2"], f["by2"])
    assert _rel(by, GOLDEN["csf_by"]) <= 1e-7
    # the reference rounds the detectors to binary32 and then divides by the weight sums in binary32: two roundings,
    # so per weight up to 2^-23 of its value (1.06e-7 of the largest weight measured) -- the bar is that bound
    for kind in ("edge", "point"):
        kx = np.outer(f["gauss"], f[kind])                  # rows y, columns x
        for got, want in ((kx, GOLDEN[kind + "_x"]), (kx.T, GOLDEN[kind + "_y"])):
            assert np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(got)), _rel(got, want)
        assert abs(kx[kx > 0].sum() - 1) < 1e-12 and abs(kx[kx < 0].sum() + 1) < 1e-12
    for k in (f["a"], f["rg"], f["by1"], f["by2"], f["gauss"]):
        assert abs(k.sum() - 1) < 1e-12 and np.allclose(k, k[::-1], rtol=0, atol=1e-17)


@pytest.mark.parametrize("ppd,rc,rf", [(40.0, 6, 5), (100.0, 14, 13), (1.0, 1, 1), (118.0, 16, 15)])
def test_flip_filter_radii_follow_the_reference(ppd, rc, rf):
    from splatco_amd.metrics import flip_filters
    f = flip_filters(ppd)
    assert (f["csf_radius"], f["feature_radius"]) == (rc, rf)
    ks, r = fr.csf_kernels(ppd)
    assert r == rc
    assert _rel(np.outer(f["a"], f["a"]), ks[0].numpy()) <= 1e-12
    by = f["by_c1"] * np.outer(f["by1"], f["by1"]) + f["by_c2"] * np.outer(f["by2"], f["by2"])
    assert _rel(by, ks[2].numpy()) <= 1e-12
    fk, r = fr.feature_kernels(ppd)
    assert r == rf
    assert _rel(np.outer(f["gauss"], f["point"]), fk["point"].numpy()) <= 1e-12


@pytest.mark.parametrize("ppd", [0.5, 0.0, -3.0, 119.0, 1000.0, float("nan"), float("inf")])
def test_flip_filters_refuse_out_of_range_ppd(ppd):
    from splatco_amd.metrics import flip_filters
    with pytest.raises(ValueError, match="pixels_per_degree"):
        flip_filters(ppd)


def test_cmax_restatement_matches_the_golden():
    assert abs(fr.cmax() - float(GOLDEN["cmax"])) <= 1e-6 * float(GOLDEN["cmax"])


@pytest.mark.parametrize("i", PAIRS)
def test_fp64_restatement_reproduces_the_golden_maps(i):
    t, r = torch.tensor(GOLDEN[f"test{i}"]), torch.tensor(GOLDEN[f"ref{i}"])
    m = fr.flip_map(t, r).numpy()
    g = GOLDEN[f"map{i}"].astype(np.float64)
    d = np.abs(m - g)
    assert d.max() <= MAX_BAR, d.max()
    assert np.quantile(d, 0.999) <= P999_BAR, np.quantile(d, 0.999)
    assert abs(m.mean() - float(GOLDEN[f"mean{i}"])) <= MEAN_BAR
    assert d.mean() <= MEAN_BAR, d.mean()


def test_restatement_quantize_is_the_8bit_round_trip():
    t, r = torch.tensor(GOLDEN["test0"]), torch.tensor(GOLDEN["ref0"])
    q = lambda x: (torch.floor(x.clamp(0, 1) * 255 + 0.5).double() / 255).float()
    a = fr.flip_map(t, r, quantize=True)
    b = fr.flip_map(q(t), q(r))
    assert torch.equal(a, b)
    assert not torch.equal(a, fr.flip_map(t, r))
