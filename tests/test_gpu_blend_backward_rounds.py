"""The blend backward settles per-lane and per-round facts once (blend.hip): a reducing lane reads the list position of its
column's splat from the staging block, the cross-wave combine loads every wave's part and adds under lane masks, and the
transposition block is laid out for the hardware's ds_read_b128 lane groups.  None of that may change a value, and neither
may any form of the contributor cut-off j < last (per entry today; per round was tried); what these tests pin:

  1. the cut-off at the edges of a round (last = 64, 65, 127, 128, 129; a quadrant that is live to the end; one that is
     finished inside the first round), Gaussians behind every last contributor with gradients that are exactly zero;
  2. the position read where slot != list position, with partial groups of one, two and three splats;
  3. the combine over entries that one, two, three, four and no quadrants reach, with a quadrant that finishes early (its
     parts are stale bits in the later rounds);
  4. a ragged image, the depth / opacity maps (AUX) and a colour that is not finite (SAFE);
  5. the deep-list variants;  6. run-to-run bits.

Scenes are hand-built on one to six 16x16 tiles with a narrow, axis-aligned camera, so that a splat's pixel position, size
and list position are what the builder says.  Bars are the parity suite's: integers exact, image 1e-4 max-abs, gradients
1e-4 rel-L2 per tensor against the CPU oracle.  Single rows are compared at ROW_TOL = 1e-3: a sum sent to the wrong record
is an error of order one, three orders above it, and a single row may lose a digit to cancellation that a tensor norm
does not see.  Every test first asserts, from the oracle's n_contrib and the tile lists, that its situation occurs.
"""
import functools
import math

import numpy as np
import pytest
import torch

from util import oracle_settings, rel_l2
from splatco_amd.cameras import make_camera

pytestmark = pytest.mark.gpu

IMG_TOL, GRAD_TOL, ROW_TOL = 1e-4, 1e-4, 1e-3
NAMES = ["means3D", "means2D", "colors_precomp", "opacities", "scales", "rotations"]
TAN = 0.01           # tan(FoVx / 2): a narrow camera, so that an isotropic Gaussian projects to a circle wherever it stands
BCH = 64             # list entries per round of the backward kernel
POSITION_SEED, RAGGED_SEED = 10, 48     # chosen on the CPU with the oracle alone, for the margins asserted below
MARGIN = 1e-4        # every decision of a scene (alpha against 1/255, T against 1e-4) lies this far, relatively, from its threshold by
                     # the oracle's own numbers: 400 x the 2 ulp the device's exp() may differ by, so n_contrib must agree everywhere


def _dev():
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    return torch.device("cuda:0")


def _t(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=_dev(), requires_grad=grad)


def _settings(cam, bg):
    from splatco_amd.rasterizer import GaussianRasterizationSettings
    d = _dev()
    return GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=torch.tensor(bg, dtype=torch.float32, device=d), scale_modifier=1.0,
        viewmatrix=cam.world_view_transform.to(d), projmatrix=cam.full_proj_transform.to(d), sh_degree=1,
        campos=cam.camera_center.to(d), prefiltered=False, debug=False)


# ------------------------------------------------------------------ scene builder
def build(W, H, entries, seed):
    """entries: (x, y, sigma, opacity[, z]) per splat in pixel units, in LIST ORDER (depth 3 + 0.01 index unless given): a Gaussian whose
    centre projects to pixel position (x, y) and whose screen-space standard deviations are (sigma, 0.8 sigma) before the
    0.3 px^2 dilation.  sigma = 0.05 ("tiny"): the dilation alone, alpha = opacity * exp(-d^2 / 0.6) -- at opacity 0.5 it
    reaches the 3x3 pixels around its centre pixel, at 0.08 the pixel and its four neighbours, at 0.015 that pixel alone."""
    cam = make_camera(np.eye(3), np.zeros(3), 2 * math.atan(TAN), 2 * math.atan(TAN * H / W), W, H)
    e = np.asarray([t[:4] for t in entries], np.float64)
    n = len(e)
    z = np.array([t[4] if len(t) > 4 else 3.0 + 0.01 * i for i, t in enumerate(entries)])
    focal = W / (2 * TAN)
    x = ((2 * e[:, 0] + 1) / W - 1) * TAN * z
    y = ((2 * e[:, 1] + 1) / H - 1) * (TAN * H / W) * z
    s = e[:, 2] * z / focal
    rng = np.random.default_rng(seed)
    f = np.float32
    g = dict(means3D=np.stack([x, y, z], 1).astype(f), scales=np.stack([s, 0.8 * s, s], 1).astype(f),
             rotations=np.tile(np.array([1, 0, 0, 0], f), (n, 1)), opacities=e[:, 3:4].astype(f),
             colors=rng.uniform(0, 1, (n, 3)).astype(f), bg=np.array([0.2, 0.5, 0.9], f))
    return cam, g


tiny = lambda x, y, op=0.5: (float(x), float(y), 0.05, op)
full = lambda: (7.5, 7.5, 40.0, 0.5)                              # half opacity over the whole tile
Q3_BLOCK = [(9.5, 9.5), (13.5, 9.5), (9.5, 13.5), (13.5, 13.5)]    # opaque blobs that finish quadrant 3 (x, y = 8..15)


def blockers(per_centre):
    return [(cx, cy, 1.92, 0.99) for _ in range(per_centre) for cx, cy in Q3_BLOCK]


# scene 1: quadrant 1 (x 8..15, y 0..7) holds the pixels whose last contributor sits at a round's edge, quadrant 0 is live to
# the end of the list, quadrant 3 is finished inside round 0, quadrant 2 mixes pixels that finish in round 0 (stacks of
# opaque tiny splats) with pixels that a late blob keeps alive: its round 1 has no boundary lane and both kinds of lane
EDGE = {64: (11, 0), 65: (14, 0), 127: (11, 3), 128: (14, 3), 129: (12, 6)}      # last -> pixel
DONE2 = [(1, 9), (1, 13)]           # pixels of quadrant 2 that finish in round 0
LIVE2 = [(4, 10), (5, 13), (3, 14)]


def cutoff_entries():
    E = blockers(12) + [full()] * 4                               # 0..51
    for p in DONE2:
        E += [tiny(*p, 0.9)] * 5                                  # ..61
    E += [tiny(9, 6, 0.08)]                                       # 62
    assert len(E) == 63
    E.append(tiny(*EDGE[64]))                                     # entry 63 = contributor 64
    E.append(tiny(*EDGE[65]))
    fill = [tiny(*LIVE2[0], 0.08), tiny(*DONE2[0], 0.015), tiny(9, 6, 0.08), tiny(*LIVE2[1], 0.08), tiny(*DONE2[1], 0.015), tiny(15, 6, 0.08),
            tiny(*LIVE2[2], 0.08)]
    while len(E) < 126:
        E.append(fill[len(E) % len(fill)])
    E += [tiny(*EDGE[127]), tiny(*EDGE[128]), tiny(*EDGE[129])]   # entries 126, 127, 128
    E += [(3.5, 11.5, 1.92, 0.2)] * 4                             # the blob that keeps quadrant 2 alive into round 2
    while len(E) < 192:
        E.append(fill[len(E) % len(fill)] if len(E) % 3 else tiny(15, 6, 0.08))
    E += [(3.5, 3.5, 1.92, 0.2)] * 8                              # quadrant 0: contributors 193..200
    E += [tiny(*DONE2[0], 0.015), tiny(12, 12, 0.8), tiny(*DONE2[1], 0.015), tiny(13, 13, 0.8), tiny(12, 12, 0.8), tiny(*DONE2[0], 0.015)]
    return E


# scene 2: quadrant 0 stages 8, 9, 10 and 11 blobs in rounds 0..3, scattered between tiny splats of the other quadrants
def position_entries():
    rng = np.random.default_rng(POSITION_SEED)
    E = []
    for r, cnt in enumerate((8, 9, 10, 11)):
        mine = set(rng.choice(BCH, cnt, replace=False).tolist())
        for j in range(BCH):
            if j in mine:
                E.append((rng.uniform(2, 5), rng.uniform(2, 5), 1.2, 0.08))
            else:
                x, y = rng.integers(11, 15, 2)
                E.append(tiny(x, y if rng.random() < 0.5 else y - 9, 0.1) if rng.random() < 0.6 else tiny(x - 9, y, 0.1))
    return E


# scene 3: entries that four, two, three, one and no quadrants reach; quadrant 3 finishes inside round 0
def combine_entries():
    rng = np.random.default_rng(9)
    kinds = [lambda: (7.5, 7.5, 3.0, 0.05),                         # all four
             lambda: (7.5, 3.5, 0.85, 0.3),                         # quadrants 0 and 1
             lambda: (5.5, 5.5, 0.85, 0.3),                         # 0, 1 and 2
             lambda: (3.5, 7.5, 0.85, 0.3),                         # 0 and 2
             lambda: tiny(rng.integers(1, 6), rng.integers(1, 6), 0.3),
             lambda: tiny(rng.integers(10, 14), rng.integers(1, 6), 0.3),
             lambda: tiny(rng.integers(10, 14), rng.integers(10, 14), 0.3),      # quadrant 3 alone: behind its last contributor
             lambda: (11.5, 11.5, 1.5, 0.3),                        # quadrant 3 and its neighbours' edges, likewise
             lambda: (rng.uniform(0, 15), rng.uniform(0, 15), 1.0, 1.0 / 300.0)]    # no quadrant: below 1/255 everywhere
    E = blockers(11) + [full()] * 3
    while len(E) < 4 * BCH:
        E.append(kinds[rng.integers(len(kinds))]())
    return E


# scene 4: 40x24 (2.5 x 1.5 tiles), random blobs
def ragged_entries():
    rng = np.random.default_rng(RAGGED_SEED)
    return [(rng.uniform(-2, 42), rng.uniform(-2, 26), float(np.exp(rng.uniform(math.log(0.3), math.log(5.0)))), rng.uniform(0.05, 0.9))
            for _ in range(320)]


SCENES = {"cutoff": (16, 16, cutoff_entries, 1), "position": (16, 16, position_entries, 2), "combine": (16, 16, combine_entries, 3),
          "ragged": (40, 24, ragged_entries, 4)}


@functools.lru_cache(maxsize=None)
def scene(name):
    W, H, entries, seed = SCENES[name]
    return build(W, H, entries(), seed)


def _dL(cam, seed=1):
    return np.random.default_rng(seed).standard_normal((3, cam.image_height, cam.image_width)).astype(np.float32)


_ORACLE = {}


def reference(oracle, name):
    """(forward results, gradients) of the CPU oracle for a scene, computed once."""
    if name not in _ORACLE:
        cam, g = scene(name)
        st = oracle_settings(oracle, cam, g["bg"])
        f = oracle.forward(st, g["means3D"], g["opacities"], g["scales"], g["rotations"], colors_precomp=g["colors"])
        b = oracle.backward(st, f, _dL(cam), g["means3D"], g["scales"], g["rotations"], colors_precomp=g["colors"])
        _ORACLE[name] = (f, b)
    return _ORACLE[name]


def run(name, aux_loss=None, g=None):
    """Forward + backward on the device; numpy results and the tile lists.  aux_loss: (dL/ddepth, dL/dalpha) -> return_aux."""
    from splatco_amd import _C
    from splatco_amd import rasterizer as R
    cam, g0 = scene(name)
    g = g or g0
    rs = _settings(cam, g["bg"])
    with torch.no_grad():
        color, radii, st = R.rasterize_forward(R._CSettings(rs), _t(g["means3D"]), _t(g["opacities"]), _t(g["scales"]),
                                               _t(g["rotations"]), None, None, _t(g["colors"]))
        out = dict(n_contrib=st.debug(_C.DBG_N_CONTRIB).cpu().numpy().view(np.uint32), qmask=st.debug(_C.DBG_QMASK).cpu().numpy(),
                   ranges=st.debug(_C.DBG_RANGES).cpu().numpy().view(np.uint32),
                   point_list=st.debug(_C.DBG_POINT_LIST).cpu().numpy().view(np.uint32))
    leaves = dict(means3D=_t(g["means3D"], True), opacities=_t(g["opacities"], True), colors_precomp=_t(g["colors"], True),
                  scales=_t(g["scales"], True), rotations=_t(g["rotations"], True))
    m2d = torch.zeros(len(g["means3D"]), 3, device=_dev(), requires_grad=True)
    res = R.GaussianRasterizer(rs)(means2D=m2d, return_aux=aux_loss is not None, **leaves)
    loss = (res[0] * _t(_dL(cam))).sum()
    if aux_loss is not None:
        loss = loss + (res[2] * _t(aux_loss[0])).sum() + (res[3] * _t(aux_loss[1])).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(res[0].detach(), color) and torch.equal(res[1], radii)
    out.update(color=color.cpu().numpy(), radii=radii.cpu().numpy(),
               grads=dict(means2D=m2d.grad.cpu().numpy(), **{k: v.grad.cpu().numpy() for k, v in leaves.items()}))
    return out


def check(f, b, o, tag):
    """The parity suite's bars: integers exact, image 1e-4, gradients 1e-4 rel-L2 per tensor."""
    assert np.array_equal(o["radii"], f["radii"]) and np.array_equal(o["point_list"], f["point_list"])
    live = f["ranges"][:, 1] > f["ranges"][:, 0]
    assert np.array_equal(o["ranges"].astype(np.int64)[live], f["ranges"].astype(np.int64)[live])
    assert np.array_equal(o["n_contrib"], f["n_contrib"]), "n_contrib"
    err = float(np.abs(o["color"] - f["color"]).max())
    errs = {n: rel_l2(o["grads"][n], b[n]) for n in NAMES}
    print(f"[rounds] {tag}: image max-abs {err:.2e}; gradient rel-L2 " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert err <= IMG_TOL
    for n in NAMES:
        assert float(np.abs(b[n]).max()) > 0, n
        assert errs[n] <= GRAD_TOL, (n, errs[n])


def check_rows(o, b, rows, tag):
    """Single rows (Gaussians) of the well-conditioned gradients."""
    worst = {}
    for n in ("colors_precomp", "opacities", "means2D"):
        want, got = b[n][rows].astype(np.float64), o["grads"][n][rows].astype(np.float64)
        norm = np.linalg.norm(want, axis=1)
        keep = norm > 1e-3 * norm.max()
        assert keep.sum() >= 0.5 * len(rows), (n, keep.sum())
        worst[n] = float((np.linalg.norm(got - want, axis=1)[keep] / norm[keep]).max())
    print(f"[rounds] {tag}: worst single row of {len(rows)}: " + ", ".join(f"{n} {e:.2e}" for n, e in worst.items()))
    assert all(e <= ROW_TOL for e in worst.values()), worst


def quadrant_last(f, q):
    """n_contrib of the 64 pixels of quadrant q of the 16x16 tile (0, 0)."""
    x0, y0 = 8 * (q & 1), 8 * (q >> 1)
    return f["n_contrib"][y0:y0 + 8, x0:x0 + 8].astype(np.int64)


def staged(o, f, q):
    """List positions of tile 0 that wave q stages: its mask bit is set and the position lies in front of the wave's last."""
    lo, hi = (int(v) for v in o["ranges"][0])
    pos = np.arange(hi - lo)
    return pos[((o["qmask"][lo:hi] >> q) & 1).astype(bool) & (pos < quadrant_last(f, q).max())]


def contributes(f):
    """Per Gaussian of a one-tile scene: does it contribute to any pixel (alpha >= 1/255 by the oracle's records, taken 1 %
    generously, at a pixel whose last contributor is not in front of it)?"""
    H, W = f["n_contrib"].shape
    xy, co = f["xy"].astype(np.float64), f["conic_opacity"].astype(np.float64)
    py, px = np.mgrid[0:H, 0:W]
    pos_of = np.full(len(xy), -1)
    pos_of[f["point_list"]] = np.arange(len(f["point_list"]))
    out = np.zeros(len(xy), bool)
    for i in range(len(xy)):
        if pos_of[i] < 0:
            continue
        dx, dy = xy[i, 0] - px, xy[i, 1] - py
        power = -0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy
        alpha = co[i, 3] * np.exp(power)
        out[i] = bool(((alpha >= 0.99 / 255.0) & (power <= 0) & (pos_of[i] < f["n_contrib"])).any())
    return out


# ------------------------------------------------------------------ 1. cut-off edges
def cutoff_situation(f):
    assert f["ranges"].shape[0] == 1 and int(f["ranges"][0, 1]) >= 200 and np.array_equal(f["point_list"], np.arange(len(f["point_list"])))
    assert float(f["margin"].min()) > MARGIN, "a decision of this scene sits on its threshold"
    for last, (x, y) in EDGE.items():
        assert 8 <= x < 16 and y < 8 and f["n_contrib"][y, x] == last, (last, f["n_contrib"][y, x])
    assert quadrant_last(f, 0).min() >= 192
    assert quadrant_last(f, 3).max() <= 64
    l2 = quadrant_last(f, 2)       # round 1 of quadrant 2: every lane in front of it or behind it, both kinds
    assert ((l2 <= 64) | (l2 >= 128)).all() and (l2 <= 64).any() and (l2 >= 128).any()
    assert all(f["n_contrib"][y, x] <= 64 for x, y in DONE2)


def test_cutoff_edges(oracle):
    f, b = reference(oracle, "cutoff")
    cutoff_situation(f)
    o = run("cutoff")
    lo, hi = (int(v) for v in o["ranges"][0])
    # quadrant 2 stages entries of round 1 that only its finished pixels could take: cut by the cut-off, not by geometry
    st2 = staged(o, f, 2)
    dead = [p for p in st2 if BCH <= p < 2 * BCH and float(scene("cutoff")[1]["opacities"][p, 0]) == np.float32(0.015)]
    assert len(dead) >= 4, dead
    check(f, b, o, "cut-off edges")
    live = contributes(f)
    behind = np.arange(len(live)) >= int(f["n_contrib"].max())          # behind every pixel's last contributor
    assert behind.sum() >= 4 and not live[behind].any() and not live[dead].any() and (~live).sum() >= 20
    for n in NAMES:
        assert not o["grads"][n][~live].any(), (n, np.nonzero(o["grads"][n][~live].any(axis=1))[0])
    lasts = np.unique(f["point_list"][f["n_contrib"][f["n_contrib"] > 0].astype(np.int64) - 1])
    assert len(lasts) >= 10 and (o["grads"]["opacities"][lasts, 0] != 0).all()


# ------------------------------------------------------------------ 2. position read, tail groups
def test_position_read_and_tail_groups(oracle):
    f, b = reference(oracle, "position")
    assert f["ranges"].shape[0] == 1 and int(f["ranges"][0, 1]) == 4 * BCH and float(f["margin"].min()) > MARGIN
    o = run("position")
    st0 = staged(o, f, 0)
    per_round = [int(((st0 >= r * BCH) & (st0 < (r + 1) * BCH)).sum()) for r in range(4)]
    print(f"[rounds] position: entries quadrant 0 stages per round {per_round}")
    assert sorted(c % 4 for c in per_round) == [0, 1, 2, 3] and min(per_round) >= 4
    slots = np.concatenate([np.arange(c) for c in per_round])
    assert (slots != st0 % BCH).mean() > 0.9, "slot == list position"
    check(f, b, o, "position read")
    check_rows(o, b, st0, "position read")


# ------------------------------------------------------------------ 3. combine
def test_combine(oracle):
    f, b = reference(oracle, "combine")
    assert f["ranges"].shape[0] == 1 and int(f["ranges"][0, 1]) == 4 * BCH and float(f["margin"].min()) > MARGIN
    wave_max = [int(quadrant_last(f, q).max()) for q in range(4)]
    assert wave_max[3] <= 64 and min(wave_max[:3]) > 192, wave_max
    o = run("combine")
    lo, hi = (int(v) for v in o["ranges"][0])
    m = o["qmask"][lo:hi].astype(np.int64)
    took = sum(((m >> q) & 1) * (np.arange(hi - lo) < wave_max[q]) for q in range(4))      # waves that add a part
    print(f"[rounds] combine: wave_max {wave_max}; entries by number of waves taking part {np.bincount(took, minlength=5).tolist()}, "
          f"mask 0: {(m == 0).sum()}, bit 3 set behind quadrant 3's last: {(((m >> 3) & 1) * (np.arange(hi - lo) >= wave_max[3])).sum()}")
    assert all((took[64:] == k).sum() >= 3 for k in range(4)) and (took == 4).sum() >= 3 and (m == 0).sum() >= 3
    assert (((m >> 3) & 1) * (np.arange(hi - lo) >= 128)).sum() >= 10      # stale parts of wave 3 in the later rounds
    check(f, b, o, "combine")
    check_rows(o, b, np.nonzero(took >= 1)[0], "combine")


# ------------------------------------------------------------------ 4. instantiations and edges
def test_ragged_image(oracle):
    f, b = reference(oracle, "ragged")
    assert f["ranges"].shape[0] == 6 and float(f["margin"].min()) > MARGIN
    check(f, b, run("ragged"), "ragged 40x24")


def test_ragged_image_with_depth_loss(oracle):
    """AUX: the blend is linear in (colour, dL/dpixel), so the oracle run a second time on the colours (z, 1, 0) over a black
    background, with (dL/ddepth, dL/dalpha, 0) as its image gradient, gives the maps' share; z = means3D.z for this camera."""
    cam, g = scene("ragged")
    f, b = reference(oracle, "ragged")
    H, W = cam.image_height, cam.image_width
    rng = np.random.default_rng(23)
    Gd, Ga = rng.standard_normal((H, W)).astype(np.float32), rng.standard_normal((H, W)).astype(np.float32)
    z = g["means3D"][:, 2:3]
    col2 = np.concatenate([z, np.ones_like(z), np.zeros_like(z)], 1).astype(np.float32)
    st2 = oracle_settings(oracle, cam, np.zeros(3, np.float32))
    f2 = oracle.forward(st2, g["means3D"], g["opacities"], g["scales"], g["rotations"], colors_precomp=col2)
    assert np.array_equal(f2["n_contrib"], f["n_contrib"])
    b2 = oracle.backward(st2, f2, np.stack([Gd, Ga, np.zeros_like(Gd)]), g["means3D"], g["scales"], g["rotations"], colors_precomp=col2)
    want = {n: b[n] + b2[n] for n in NAMES if n != "colors_precomp"}
    want["means3D"] = want["means3D"] + np.concatenate([np.zeros((len(z), 2), np.float32), b2["colors_precomp"][:, :1]], 1)
    want["colors_precomp"] = b["colors_precomp"]
    o = run("ragged", aux_loss=(Gd, Ga))
    assert float(np.abs(b2["colors_precomp"][:, 0]).max()) > 0
    check(f, want, o, "ragged 40x24, depth + opacity loss")


def test_ragged_image_with_a_colour_that_is_not_finite(oracle):
    """SAFE: one more splat in the middle of a tile's list, whose alpha >= 1/255 ellipse lies between four pixel centres of a
    quadrant -- staged by that wave, contributing to no pixel -- with a colour that is not finite.  The oracle skips it; the
    image keeps its bits (the forward has no groups), the gradients meet the oracle's at the usual bar (a list entry more
    moves the groups of four of the backward, and with them its rounding) and stay finite, the splat's own are zero."""
    cam, g = scene("ragged")
    f, _ = reference(oracle, "ragged")
    cam2, g2 = build(40, 24, ragged_entries() + [(20.5, 10.5, 0.05, 0.0045, 3.0 + 0.01 * 40.5)], SCENES["ragged"][3])
    assert all(np.array_equal(g2[k][:-1], g[k]) for k in ("means3D", "scales", "opacities", "colors"))
    g2["colors"][-1] = np.array([np.nan, 0.5, np.inf], np.float32)
    st = oracle_settings(oracle, cam2, g2["bg"])
    f2 = oracle.forward(st, g2["means3D"], g2["opacities"], g2["scales"], g2["rotations"], colors_precomp=g2["colors"])
    b2 = oracle.backward(st, f2, _dL(cam2), g2["means3D"], g2["scales"], g2["rotations"], colors_precomp=g2["colors"])
    assert np.array_equal(f2["color"], f["color"]) and float(f2["margin"].min()) > MARGIN
    o = run("ragged", g=g2)
    lo, hi = (int(v) for v in o["ranges"][1])                     # tile (1, 0) of the 3 x 2 grid holds pixel (20, 10), in its quadrant 2
    n = len(g2["means3D"]) - 1
    at = np.nonzero(o["point_list"][lo:hi] == n)[0]
    assert len(at) == 1 and (o["qmask"][lo + at[0]] >> 2) & 1 and at[0] < int(f2["n_contrib"][8:16, 16:24].max()), "not staged"
    assert np.array_equal(o["color"], run("ragged")["color"])
    check(f2, b2, o, "ragged 40x24, one colour not finite")
    for k in NAMES:
        assert np.isfinite(o["grads"][k]).all() and not o["grads"][k][n].any(), k


# ------------------------------------------------------------------ 5. deep-list variants
def test_deep_list_variants_keep_the_bits(oracle):
    from splatco_amd import _C
    cutoff_situation(reference(oracle, "cutoff")[0])
    base = run("cutoff")
    _C.check(_C.lib.scr_debug_force_deep_lists(1))
    try:
        deep = run("cutoff")
    finally:
        _C.check(_C.lib.scr_debug_force_deep_lists(-1))
    assert np.array_equal(deep["color"], base["color"]) and np.array_equal(deep["n_contrib"], base["n_contrib"])
    for k in NAMES:
        assert np.array_equal(deep["grads"][k], base["grads"][k]), k


# ------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("name", ["cutoff", "position", "combine"])
def test_run_to_run_bits(name):
    a, b = run(name), run(name)
    assert np.array_equal(a["color"], b["color"])
    for k in NAMES:
        assert a["grads"][k].tobytes() == b["grads"][k].tobytes(), k
