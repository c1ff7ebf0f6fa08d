"""GPU tests of test-view evaluation (splatco_amd.evaluate: render.py + metrics.py of the reference) on a small seeded
anchor model; the ground truths are renders of a perturbed copy of the model."""
import json
import math
import types

import pytest
import torch

import flip_restatement as fr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PIPE = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False, mv=1)


def _scene(n_views=7, W=96, H=64):
    from splatco_amd.synthetic import synthetic_anchor_model, synthetic_views
    pc = synthetic_anchor_model(3000, seed=5, device=DEV, plane_size=64)
    views = [v.to(DEV) for v in synthetic_views(n_views, width=W, height=H)]
    gt_pc = synthetic_anchor_model(3000, seed=5, device=DEV, plane_size=64)
    with torch.no_grad():
        g = torch.Generator(device=DEV).manual_seed(9)
        gt_pc._anchor_feat.add_(0.3 * torch.randn(gt_pc._anchor_feat.shape, device=DEV, generator=g))
        gt_pc._offset.add_(0.05 * torch.randn(gt_pc._offset.shape, device=DEV, generator=g))
    bg = torch.tensor([0.0, 0.0, 0.0], device=DEV)
    from splatco_amd.evaluate import render_views
    gts, _, _ = render_views(views, gt_pc, PIPE, bg)
    return pc, views, gts, bg


def test_evaluate_views_equals_per_view_scores():
    from splatco_amd import losses
    from splatco_amd.evaluate import evaluate_views
    pc, views, gts, bg = _scene()
    pc.train()
    pc.feat_planes.Q0 = 0.03
    res = evaluate_views(views, pc, PIPE, bg, gts=gts, quantize=True)
    # keys and shape of metrics.py's results.json entry (LPIPS absent: no weights), plus FPS
    assert set(res) == {"SSIM", "PSNR", "FLIPS", "NUM", "FPS", "per_view"}
    assert set(res["per_view"]) == {"SSIM", "PSNR", "FLIPS"}
    names = ["{0:05d}.png".format(i) for i in range(len(views))]
    assert all(list(res["per_view"][k]) == names for k in ("SSIM", "PSNR", "FLIPS"))
    assert res["NUM"] == 3000
    assert math.isfinite(res["FPS"]) and res["FPS"] > 0
    # mode and plane noise restored
    assert pc.get_color_mlp.training and pc.feat_planes.Q0 == 0.03
    # no gradient anywhere, no graph kept
    assert all(p.grad is None for p in pc.parameters())
    # the same numbers from the torch ops: renders of the eval-mode model (Q0 = 0), 8-bit round trip, losses.ssim,
    # losses.psnr and the float64 FLIP restatement
    pc.eval()
    pc.feat_planes.Q0 = 0
    from splatco_amd.renderer import prefilter_voxel, render
    q = lambda x: (torch.floor(x.clamp(0, 1) * 255 + 0.5).double() / 255).float()
    for i, (view, gt) in enumerate(zip(views, gts)):
        with torch.no_grad():
            img = render(view, pc, PIPE, bg, visible_mask=prefilter_voxel(view, pc, PIPE, bg))["render"]
        a, b = q(img), q(gt)
        name = names[i]
        assert abs(res["per_view"]["SSIM"][name] - float(losses.ssim(a, b))) <= 1e-5
        assert abs(res["per_view"]["PSNR"][name] - float(losses.psnr(a[None], b[None]))) <= 2e-4
        assert abs(res["per_view"]["FLIPS"][name] - float(fr.flip_map(a, b).mean())) <= 1e-5
    pc.train()
    for k in ("SSIM", "PSNR", "FLIPS"):
        v = list(res["per_view"][k].values())
        assert abs(res[k] - sum(v) / len(v)) <= 1e-5 * max(1.0, abs(res[k]))
    assert 0 < res["FLIPS"] < 1 and 0 < res["SSIM"] < 1 and res["PSNR"] > 5


def test_evaluate_reads_original_image_and_restores_mode_on_error():
    from splatco_amd.evaluate import evaluate_views, render_views
    pc, views, gts, bg = _scene(n_views=3, W=48, H=40)
    for v, g in zip(views, gts):
        v.original_image = torch.cat((g, torch.ones_like(g[:1])))        # RGBA: the scores read [0:3]
    pc.eval()
    pc.feat_planes.Q0 = 0.5
    res = evaluate_views(views, pc, PIPE, bg, names=["a", "b", "c"], quantize=False)
    assert list(res["per_view"]["FLIPS"]) == ["a", "b", "c"]
    assert not pc.get_color_mlp.training and pc.feat_planes.Q0 == 0.5
    # with 5 views or fewer every view is timed
    imgs, times, fps = render_views(views, pc, PIPE, bg)
    assert len(times) == 3 and abs(fps - 3 / sum(times)) <= 1e-9 * fps
    assert all(not im.requires_grad and im.grad_fn is None for im in imgs)
    pc.train()
    bad = types.SimpleNamespace(debug=False, compute_cov3D_python=True)              # prefilter_voxel refuses this
    with pytest.raises(NotImplementedError):
        render_views(views, pc, bad, bg)
    assert pc.get_color_mlp.training and pc.feat_planes.Q0 == 0.5


def test_write_results_round_trips(tmp_path):
    from splatco_amd.evaluate import write_results
    res = {"SSIM": 0.9, "PSNR": 31.5, "FLIPS": 0.1, "NUM": 12, "FPS": 250.0,
           "per_view": {"SSIM": {"00000.png": 0.9}, "PSNR": {"00000.png": 31.5}, "FLIPS": {"00000.png": 0.1}}}
    full, per = write_results(str(tmp_path / "m"), res, method="ours_30000")
    assert json.load(open(full)) == {"ours_30000": {"SSIM": 0.9, "PSNR": 31.5, "FLIPS": 0.1, "NUM": 12, "FPS": 250.0}}
    assert json.load(open(per)) == {"ours_30000": res["per_view"]}
