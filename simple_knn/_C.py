"""`simple_knn._C` of the reference's environment: distCUDA2(points[N,3]) -> [N] float32, the mean squared distance of
every point to its 3 nearest other points.  Semantics and their standing: splatco_amd/scene_init.py."""
from splatco_amd.scene_init import dist2 as distCUDA2  # noqa: F401
