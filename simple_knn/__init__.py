"""Drop-in package name: `from simple_knn._C import distCUDA2` (scene/gaussian_model.py:22) resolves here when this
repository is on sys.path.  The implementation lives in splatco_amd/scene_init.py (HIP kernels for MI355X behind a C-ABI)."""
