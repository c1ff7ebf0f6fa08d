"""CPU side of the depth / opacity maps: the public surface exists with defaults that keep every existing call as it was, and
the library exports the entry points (no compute calls; the GPU tests are in test_gpu_aux_maps.py)."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_surface_defaults_keep_existing_calls():
    from splatco_amd import rasterizer as R
    from splatco_amd.renderer import render
    fwd = inspect.signature(R.GaussianRasterizer.forward).parameters
    assert fwd["return_aux"].default is False and list(fwd)[-1] == "return_aux"
    assert inspect.signature(R.rasterize_gaussians).parameters["return_aux"].default is False
    assert inspect.signature(R.rasterize_forward).parameters["aux"].default is False
    assert inspect.signature(render).parameters["aux"].default is False
    assert len(R.GaussianRasterizationSettings._fields) == 12
    import diff_gaussian_rasterization as D
    assert D.GaussianRasterizer is R.GaussianRasterizer


REMOVED = ("scr_forward_plan_mode", "scr_forward_run_aux", "scr_forward_plan_run_aux", "scr_forward_plan_run_mode",
           "scr_backward_aux", "scr_backward_camera", "scr_backward_scratch_bytes_aux", "scr_backward_scratch_bytes_camera")


def test_library_exports_the_aux_entry_points():
    """ABI 34: the maps are arguments of scr_forward_run / scr_forward_plan_run / scr_backward, not entry points of their own."""
    from splatco_amd import _C
    hdr = open(os.path.join(ROOT, "include", "splatco_raster.h")).read()
    for name in ("scr_forward_run", "scr_forward_plan_run", "scr_backward", "scr_backward_scratch_bytes"):
        assert hasattr(_C.lib, name) and name in _C.SYMBOLS and re.search(rf"\b{name}\(", hdr), name
    for name in REMOVED:
        assert not hasattr(_C.lib, name) and name not in _C.SYMBOLS and name not in hdr, name
    assert _C.ABI_VERSION >= 34
    # the records and, behind them, one float per instance, each part 256-byte aligned
    for n in (0, 1, 63, 64, 1000, 4_390_000):
        plain, aux = _C.lib.scr_backward_scratch_bytes(n, 0, 0, 0), _C.lib.scr_backward_scratch_bytes(n, 0, 1, 0)
        assert plain % 256 == 0 and aux % 256 == 0 and plain >= 36 * n and aux - plain >= 4 * n and aux - plain < 4 * n + 512
    # each family's one prototype is the superset its last variant had
    sig = {s[0]: s for s in _C.SIGNATURES}
    assert len(sig["scr_forward_plan"]) - 2 == 15 and len(sig["scr_forward_run"]) - 2 == 12
    assert len(sig["scr_forward_plan_run"]) - 2 == 21 and len(sig["scr_backward"]) - 2 == 30
