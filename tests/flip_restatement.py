"""LDR-FLIP restated in torch (Andersson et al., "FLIP: A Difference Evaluator for Alternating Images", HPG 2020; the
reference's utils/flip.py LDRFLIPLoss at its defaults), in the reference's structure: full 2-D conv2d kernels with
replicate padding, one elementwise step per formula.  Runs in float64 by default (the checker of the GPU tests) or in
float32 (the reference-shaped baseline of tools/time_flip.py), on any device."""
import math

import numpy as np
import torch
import torch.nn.functional as F

DEFAULT_PPD = (0.7 * 3840 / 0.7) * math.pi / 180
QC, QF, PC, PT, EPS = 0.7, 0.5, 0.4, 0.95, 1e-15

_RGB2XYZ = [[10135552 / 24577794, 8788810 / 24577794, 4435075 / 24577794],
            [2613072 / 12288897, 8788810 / 12288897, 887015 / 12288897],
            [1425312 / 73733382, 8788810 / 73733382, 70074185 / 73733382]]
_XYZ2RGB = [[3.241003275, -1.537398934, -0.498615861],
            [-0.969224334, 1.875930071, 0.041554224],
            [0.055639423, -0.204011202, 1.057148933]]
_WHITE = [0.950428545, 1.0, 1.088900371]
_INV_WHITE = [1.052156925, 1.0, 0.918357670]


def csf_kernels(ppd, dtype=torch.float64):
    """The three 2-D contrast sensitivity kernels (A, RG, BY), each summing to 1, and their common radius."""
    r = int(np.ceil(3 * np.sqrt(0.04 / (2 * np.pi ** 2)) * ppd))
    d = np.arange(-r, r + 1) / ppd
    z = d[None, :] ** 2 + d[:, None] ** 2
    out = []
    for terms in (((1.0, 0.0047),), ((1.0, 0.0053),), ((34.1, 0.04), (13.5, 0.025))):
        k = sum(a * np.sqrt(np.pi / b) * np.exp(-np.pi ** 2 * z / b) for a, b in terms)
        out.append(torch.tensor(k / k.sum(), dtype=dtype))
    return out, r


def feature_kernels(ppd, dtype=torch.float64):
    """2-D edge and point detectors along x (rows = y, columns = x): positive weights sum to 1, negative to -1."""
    sd = 0.5 * 0.082 * ppd
    r = int(np.ceil(3 * sd))
    x = np.arange(-r, r + 1, dtype=np.float64)[None, :]
    y = x.T
    g = np.exp(-(x ** 2 + y ** 2) / (2 * sd * sd))
    out = {}
    for kind, k in (("edge", -x * g), ("point", (x ** 2 / (sd * sd) - 1) * g)):
        pos, neg = k[k > 0].sum(), -k[k < 0].sum()
        out[kind] = torch.tensor(np.where(k > 0, k / pos, np.where(k < 0, k / neg, 0.0)), dtype=dtype)
    return out, r


def _mat(m, img):
    A = torch.tensor(m, dtype=img.dtype, device=img.device)
    return torch.einsum("ij,njhw->nihw", A, img)


def _col(v, img):
    return torch.tensor(v, dtype=img.dtype, device=img.device).view(1, 3, 1, 1)


def srgb_to_ycxcz(img):
    lin = torch.where(img > 0.04045, ((img.clamp(min=0.04045) + 0.055) / 1.055) ** 2.4, img / 12.92)
    xyz = _mat(_RGB2XYZ, lin) * _col(_INV_WHITE, img)
    X, Y, Z = xyz[:, 0:1], xyz[:, 1:2], xyz[:, 2:3]
    return torch.cat((116 * Y - 16, 500 * (X - Y), 200 * (Y - Z)), 1)


def ycxcz_to_linrgb(img):
    y = (img[:, 0:1] + 16) / 116
    xyz = torch.cat((y + img[:, 1:2] / 500, y, y - img[:, 2:3] / 200), 1) * _col(_WHITE, img)
    return _mat(_XYZ2RGB, xyz)


def linrgb_to_hunt_lab(img):
    xyz = _mat(_RGB2XYZ, img) * _col(_INV_WHITE, img)
    d = 6 / 29
    f = torch.where(xyz > d ** 3, xyz.clamp(min=d ** 3) ** (1 / 3), xyz / (3 * d * d) + 4 / 29)
    L = 116 * f[:, 1:2] - 16
    a = 500 * (f[:, 0:1] - f[:, 1:2])
    b = 200 * (f[:, 1:2] - f[:, 2:3])
    return torch.cat((L, 0.01 * L * a, 0.01 * L * b), 1)


def hyab(x, y):
    d = x - y
    return torch.sqrt((d[:, 0:1] ** 2).clamp(min=EPS)) + torch.sqrt(d[:, 1:2] ** 2 + d[:, 2:3] ** 2)


def cmax(dtype=torch.float64):
    g = linrgb_to_hunt_lab(torch.tensor([0.0, 1.0, 0.0], dtype=dtype).view(1, 3, 1, 1))
    b = linrgb_to_hunt_lab(torch.tensor([0.0, 0.0, 1.0], dtype=dtype).view(1, 3, 1, 1))
    return float(hyab(g, b).pow(QC))


def _conv(x, k, r):
    return F.conv2d(F.pad(x, (r, r, r, r), mode="replicate"), k.to(x)[None, None])


def flip_map(test, reference, ppd=DEFAULT_PPD, quantize=False, dtype=torch.float64):
    """Per-pixel LDR-FLIP [N,H,W] of [N,3,H,W] (or [3,H,W] -> [H,W]) sRGB images."""
    single = test.dim() == 3
    t = (test[None] if single else test).to(dtype).clamp(0, 1)
    r = (reference[None] if single else reference).to(dtype).clamp(0, 1)
    if quantize:
        # k / 255 correctly rounded to binary32, as a PNG reader forms it
        t, r = [(torch.floor(x.float() * 255 + 0.5).double() / 255).float().to(dtype) for x in (t, r)]
    ks, rc = csf_kernels(ppd, dtype)
    fk, rf = feature_kernels(ppd, dtype)
    yt, yr = srgb_to_ycxcz(t), srgb_to_ycxcz(r)

    def colour(y):
        filt = torch.cat([_conv(y[:, c:c + 1], ks[c], rc) for c in range(3)], 1)
        return linrgb_to_hunt_lab(ycxcz_to_linrgb(filt).clamp(0, 1))

    cm = cmax(dtype)
    p = hyab(colour(yr), colour(yt)).pow(QC)
    pcc = PC * cm
    dEc = torch.where(p < pcc, (PT / pcc) * p, PT + ((p - pcc) / (cm - pcc)) * (1 - PT))

    def norms(y):
        yn = (y[:, 0:1] + 16) / 116
        e = torch.cat((_conv(yn, fk["edge"], rf), _conv(yn, fk["edge"].T, rf)), 1).norm(dim=1, keepdim=True)
        q = torch.cat((_conv(yn, fk["point"], rf), _conv(yn, fk["point"].T, rf)), 1).norm(dim=1, keepdim=True)
        return e, q

    er, pr = norms(yr)
    et, pt = norms(yt)
    dEf = torch.maximum((er - et).abs(), (pt - pr).abs()).clamp(min=EPS)
    dEf = (dEf / math.sqrt(2)) ** QF
    out = dEc.pow(1 - dEf)[:, 0]
    return out[0] if single else out
