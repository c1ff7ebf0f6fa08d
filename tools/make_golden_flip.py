#!/usr/bin/env python3
"""Generate tests/golden/flip.npz by IMPORTING the reference's own Python (utils/flip.py LDRFLIPLoss, utils/loss_utils.py
ssim, utils/image_utils.py psnr; build container only) and recording seeded inputs -> outputs on the CPU.  Only arrays
are written.  The reference hard-codes .cuda() and device='cuda': tools/make_golden.py's stubs make .cuda() the identity,
and torch.zeros drops a cuda device while this runs (restored afterwards).

  pairs    smooth random 64x64; ragged 70x133; tiny 23x17 (smaller than the 21-tap CSF filter); one pair already on
           the 8-bit grid (what save_image + to_tensor give) -- each `test{i}` / `ref{i}` [3,H,W]
  outputs  `map{i}` the reference's per-pixel LDR-FLIP [H,W] at the default pixels per degree, `mean{i}` its mean,
           `ssim{i}`, `psnr{i}` (of the pair clamped to [0,1]); the 2-D kernels at the default ppd: `csf_a`, `csf_rg`,
           `csf_by`, `edge_x`, `edge_y`, `point_x`, `point_y`; `ppd`, `cmax`
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402


def smooth(g, H, W, k=5):
    x = torch.rand(1, 3, H + k - 1, W + k - 1, generator=g, dtype=torch.float64)
    return torch.nn.functional.avg_pool2d(x, k, stride=1)[0]


def make_flip():
    fl = mg._load("utils/flip.py", "ref_flip")
    lu = mg._load("utils/loss_utils.py", "ref_loss_utils")
    iu = mg._load("utils/image_utils.py", "ref_image_utils")
    zeros = torch.zeros

    def zeros_host(*a, **k):
        if str(k.get("device", "")).startswith("cuda"):
            k.pop("device")
        return zeros(*a, **k)

    torch.zeros = zeros_host
    try:
        g = torch.Generator().manual_seed(0)
        pairs = []
        ref = smooth(g, 64, 64)
        pairs.append((ref + 0.08 * torch.randn(3, 64, 64, generator=g, dtype=torch.float64), ref))
        ref = smooth(g, 70, 133, 3)
        test = ref.clone()
        test[:, 20:50, 40:90] = test[:, 20:50, 40:90].flip(-1)       # a mirrored block: edges and points differ
        pairs.append((test + 0.03 * torch.randn(3, 70, 133, generator=g, dtype=torch.float64), ref))
        ref = torch.rand(3, 23, 17, generator=g, dtype=torch.float64)
        pairs.append((ref * 0.8 + 0.1 + 0.05 * torch.randn(3, 23, 17, generator=g, dtype=torch.float64), ref))
        ref = smooth(g, 48, 40)
        test = ref + 0.06 * torch.randn(3, 48, 40, generator=g, dtype=torch.float64)
        q = lambda x: torch.floor(x.clamp(0, 1).float() * 255 + 0.5) / 255
        pairs.append((q(test), q(ref)))
        out = {}
        loss = fl.LDRFLIPLoss()
        for i, (t, r) in enumerate(pairs):
            t, r = t.float(), r.float()          # float32 inputs, as the reference receives them (values may leave [0,1])
            m = loss(t[None], r[None])[0, 0]
            tc, rc = t.clamp(0, 1), r.clamp(0, 1)
            out.update({f"test{i}": t.numpy(), f"ref{i}": r.numpy(), f"map{i}": m.numpy(),
                        f"mean{i}": np.float32(m.mean().item()),
                        f"ssim{i}": np.float32(lu.ssim(tc, rc).item()),
                        f"psnr{i}": np.float32(iu.psnr(tc[None], rc[None]).item())})
        ppd = (0.7 * 3840 / 0.7) * np.pi / 180
        out["ppd"] = np.float64(ppd)
        for name in ("A", "RG", "BY"):
            k, _ = fl.generate_spatial_filter(ppd, name)
            out["csf_" + name.lower()] = k[0, 0].numpy()
        # feature_detection builds its kernel inline: record it from the response to a unit impulse (conv2d correlates,
        # so the response is the kernel mirrored in both axes; mirror it back)
        rf = int(np.ceil(3 * 0.5 * 0.082 * ppd))
        n = 2 * rf + 1
        c = 3 * n // 2
        imp = torch.zeros(1, 1, 3 * n, 3 * n)
        imp[0, 0, c, c] = 1.0
        for kind in ("edge", "point"):
            resp = fl.feature_detection(imp, ppd, kind)[0]
            out[kind + "_x"] = resp[0, c - rf:c + rf + 1, c - rf:c + rf + 1].flip(0).flip(1).numpy()
            out[kind + "_y"] = resp[1, c - rf:c + rf + 1, c - rf:c + rf + 1].flip(0).flip(1).numpy()
        unit = lambda ch: torch.tensor([[[float(ch == 0)]], [[float(ch == 1)]], [[float(ch == 2)]]]).unsqueeze(0)
        green = fl.hunt_adjustment(fl.color_space_transform(unit(1), "linrgb2lab"))
        blue = fl.hunt_adjustment(fl.color_space_transform(unit(2), "linrgb2lab"))
        out["cmax"] = np.float32(torch.pow(fl.hyab(green, blue, 1e-15), 0.7).item())
    finally:
        torch.zeros = zeros
    np.savez_compressed(os.path.join(mg.OUT, "flip.npz"), **out)


if __name__ == "__main__":
    mg.install_stubs()
    make_flip()
    print("flip.npz", os.path.getsize(os.path.join(mg.OUT, "flip.npz")))
