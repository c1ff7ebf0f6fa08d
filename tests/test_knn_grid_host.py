"""CPU tests of the host half of the grid-bucketed neighbour search (splatco_amd/knn_grid.py) and of the validation the
C-ABI does on its one grid descriptor before anything is launched.  The searches themselves are compared with a brute
force in tests/test_gpu_scene_init.py."""
import ast

import numpy as np
import pytest
import torch

from test_gpu_scene_init import _gen, _wide


def _grid_clouds():
    line = torch.zeros(5000, 3)
    line[:, 1] = torch.rand(5000, generator=_gen(2)) * 7 - 3
    plane = torch.rand(40000, 3, generator=_gen(3)) * 4 - 2
    plane[:, 2] = 0.75
    box = torch.rand(30000, 3, generator=_gen(4)) * torch.tensor([1.0e6, 1.0, 1.0])
    return {"line": line, "plane": plane, "1e6 : 1 box": box, "two clusters 3000 apart": _wide()}


def test_identical_points_give_one_cell_and_no_slack():
    from splatco_amd.knn_grid import bounds, grid
    p = torch.full((300, 3), 0.37)
    h, n, slack = grid(*bounds(p), p.shape[0])
    assert n == [1, 1, 1] and slack == 0.0 and isinstance(h, np.float32) and h > 0


@pytest.mark.parametrize("name", ["line", "plane", "1e6 : 1 box", "two clusters 3000 apart"])
def test_grid_respects_its_caps_and_derives_the_slack(name):
    from splatco_amd.knn_grid import bounds, grid
    p = _grid_clouds()[name]
    N = p.shape[0]
    h, n, slack = grid(*bounds(p), N)
    print(f"[{name}] N = {N}: h = {h}, n = {n}, slack = {slack}")
    assert len(n) == 3 and all(isinstance(v, int) and 1 <= v <= 2 ** 18 for v in n)
    assert n[0] * n[1] * n[2] <= min(8 * N + 64, 2 ** 31 - 2)
    assert isinstance(h, np.float32) and np.isfinite(h) and h > 0
    assert slack == float(h) * (8.0 * max(n) * 2.0 ** -23 + 1e-4)


def test_grid_descriptor_is_validated_before_anything_is_launched():
    """ABI 36: scr_knn, scr_knn_cell_keys and scr_knn3_dist2 check the same grid_host[8] and N.  Host-side checks, no
    device needed."""
    from splatco_amd import _C
    lib = _C.lib
    err = lambda: lib.scr_last_error().decode()
    p = 4096                                   # a non-null stand-in address: the checks below come first
    calls = {"scr_knn": lambda N, g: lib.scr_knn(N, 3, g, p, p, p, p, None),
             "scr_knn_cell_keys": lambda N, g: lib.scr_knn_cell_keys(N, g, p, p, None),
             "scr_knn3_dist2": lambda N, g: lib.scr_knn3_dist2(N, g, p, p, p, p, None)}
    good = (0.0, 0.0, 0.0, 0.5, 4, 4, 4, 1e-4)
    at = lambda i=None, v=None: _C.host_array([v if j == i else w for j, w in enumerate(good)], _C.f32)   # good, but for [i]
    bad_grids = {"h = 0": at(3, 0.0), "h < 0": at(3, -0.5), "h NaN": at(3, float("nan")), "nx = 0": at(4, 0), "ny = 0": at(5, 0),
                 "nz = 0": at(6, 0), "2^31 cells on one axis": at(4, 2.0 ** 31),
                 "2^31 cells": _C.host_array((0.0, 0.0, 0.0, 0.5, 2048, 1024, 1024, 1e-4), _C.f32),
                 "negative slack": at(7, -1e-6), "slack NaN": at(7, float("nan"))}
    for name, call in calls.items():
        for what, g in bad_grids.items():
            assert call(1000, g) == 1 and name + ":" in err(), (name, what, err())
        for N in (0, -5, 2 ** 31, 2 ** 40):
            assert call(N, at()) == 1 and name + ":" in err(), (name, N, err())
        assert call(1000, None) == 1 and name + ":" in err(), (name, "NULL grid", err())
    g = at()
    for N, k in ((1000, 0), (1000, 17), (1000, -1), (3, 3), (16, 16)):
        assert lib.scr_knn(N, k, g, p, p, p, p, None) == 1 and "scr_knn:" in err(), (N, k, err())
    assert lib.scr_knn3_dist2(3, g, p, p, p, p, None) == 1 and "scr_knn3_dist2:" in err()


def test_both_searches_bucket_with_the_one_module():
    from splatco_amd import densify, knn_grid, scene_init
    assert densify.buckets is knn_grid.buckets and scene_init.buckets is knn_grid.buckets
    assert scene_init.bounds is knn_grid.bounds
    for gone in ("_knn_grid", "_knn3_grid", "_knn3_buckets", "_bounds"):
        assert not hasattr(densify, gone) and not hasattr(scene_init, gone), gone
    imported = [a.name for node in ast.walk(ast.parse(open(knn_grid.__file__).read()))
                if isinstance(node, (ast.Import, ast.ImportFrom)) for a in node.names + [ast.alias(name=getattr(node, "module", None) or "")]]
    assert imported and not [m for m in imported if "densify" in m or "scene_init" in m], imported
