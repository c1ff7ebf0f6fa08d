"""ctypes binding of the C-ABI in include/splatco_raster.h and of the family headers include/splatco_bilagrid.h,
include/splatco_normals.h, include/splatco_tsdf.h, include/splatco_tsdf_sparse.h, include/splatco_mesh.h and
include/splatco_surfeval.h (libsplatco_raster.so, gfx950).

This is the binding a maintainer of the reference would write in place of the pybind module
`diff_gaussian_rasterization._C`.  There is NO fallback: if the HIP library
is missing or was built against another ABI version, importing this module raises.
"""
import ctypes as C
import os

# PyTorch-ROCm carries its own libamdhip64: load it BEFORE this library, so that both use ONE HIP runtime (the library's
# device pointers and streams are torch's).  Loaded the other way round -- e.g. build() and smoke() in one process --
# this library binds to /opt/rocm's copy and its first HIP call fails with "no ROCm-capable device is detected".
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# developer override for A/B experiments with variant builds of the same library
LIB_PATH = os.environ.get("SPLATCO_RASTER_LIB", os.path.join(_HERE, "csrc", "libsplatco_raster.so"))

PLAN_NONFINITE_COLOUR, PLAN_LARGE_RECTS, PLAN_ANTIALIASED = 1, 2, 4      # SCR_PLAN_*
MODE_ANTIALIASED = 1                                # SCR_MODE_* (scr_forward_plan / scr_forward_plan_run)
PROF_COUNT = 20
ABI_VERSION = 37
FLIP_MAX_RADIUS = 16                                # SCR_FLIP_MAX_RADIUS

(DBG_TILES_TOUCHED, DBG_POINT_OFFSETS, DBG_RANGES, DBG_POINT_LIST, DBG_N_CONTRIB, DBG_FINAL_T, DBG_SPLAT_RECORDS, DBG_QMASK,
 DBG_GM_INDEX) = range(9)

vp, cp, u8, i32, i64, f32, f64, sz = C.c_void_p, C.c_char_p, C.c_uint8, C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t
P = C.POINTER


class Settings(C.Structure):
    """struct scr_settings (include/splatco_raster.h): the 12 fields of
    GaussianRasterizationSettings, same order (gaussian_renderer/__init__.py:145-158)."""
    _fields_ = [
        ("image_height", i32), ("image_width", i32),
        ("tanfovx", f32), ("tanfovy", f32),
        ("bg", vp), ("scale_modifier", f32),
        ("viewmatrix", vp), ("projmatrix", vp),
        ("sh_degree", i32), ("campos", vp),
        ("prefiltered", i32), ("debug", i32),
    ]


class AdamTensor(C.Structure):
    """scr_adam_tensor (include/splatco_raster.h)."""
    _fields_ = [("param", vp), ("grad", vp), ("exp_avg", vp), ("exp_avg_sq", vp),
                ("numel", i64), ("step_size", f64), ("bias_correction2_sqrt", f64)]


class TvPlane(C.Structure):
    """scr_tv_plane (include/splatco_raster.h)."""
    _fields_ = [("plane", vp), ("grad", vp), ("channels", i32), ("rows", i32), ("cols", i32), ("coef", f32)]


# (name, restype, *argtypes) of every function in include/splatco_raster.h, in header order.  `int` is i32 here;
# tests/test_abi_and_multiview.py checks every entry, struct and constant above against the header.
SIGNATURES = [
    ("scr_abi_version", i32),
    ("scr_last_error", cp),
    ("scr_geom_bytes", sz, i64, i32, i32),
    ("scr_binning_bytes", sz, i64, i64),
    ("scr_image_bytes", sz, i32, i32),
    ("scr_backward_scratch_bytes", sz, i64, i64, i32, i32),
    ("scr_visible_filter", i32, i64, vp, vp, vp, vp, P(Settings), vp, vp),
    ("scr_mark_visible", i32, i64, vp, vp, vp, vp),
    ("scr_forward_plan", i32, i64, i64, i32, *[vp] * 7, P(Settings), vp, vp, P(i64), vp),
    ("scr_forward_run", i32, i64, i64, i64, i64, P(Settings), *[vp] * 7),
    ("scr_forward_plan_run", i32, i64, i64, i32, *[vp] * 7, P(Settings), vp, vp, P(i64), vp, sz, *[vp] * 5),
    ("scr_backward", i32, i64, i32, i64, i64, *[vp] * 5, P(Settings), *[vp] * 20),
    ("scr_debug_force_deep_lists", i32, i32),
    ("scr_debug_get", i32, i32, i64, i64, i32, i32, *[vp] * 5),
    ("scr_tpa_scratch_bytes", sz, i32, i32, i32),
    ("scr_tpa_stats", i32, i32, i32, i32, *[vp] * 8),
    ("scr_tpa_forward", i32, i32, i32, i32, *[vp] * 12),
    ("scr_tpa_backward", i32, i32, i32, i32, *[vp] * 18),
    ("scr_tpa_backward_stats", i32, i32, i32, i32, *[vp] * 7),
    ("scr_expand_scratch_bytes", sz, i64),
    ("scr_expand_plan", i32, i64, vp, vp, P(i64), vp),
    ("scr_mask_index_plan", i32, i64, vp, vp, P(i64), vp),
    ("scr_mask_index_run", i32, i64, *[vp] * 5),
    ("scr_expand_run", i32, i64, i32, vp, vp, vp, vp, i32, *[vp] * 11),
    ("scr_expand_backward", i32, i64, i32, vp, vp, i32, *[vp] * 14, i64, vp),
    ("scr_triplane_backward_multi_scratch_bytes", sz, i64, i32, vp, vp, vp, vp),
    ("scr_triplane_backward_multi", i32, i64, vp, i32, i32, *[vp] * 6, i32, vp, vp, vp, vp, i32, vp, i32, vp),
    ("scr_plane_row_pairs", i32, i32, i32, i32, vp, vp, vp),
    ("scr_triplane_forward", i32, i64, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, i32, i32, vp),
    ("scr_plane_sample_scratch_bytes", sz, i64, i32, i32, i32),
    ("scr_triplane_backward_scratch_bytes", sz, i64, i32, i32, i32, i32),
    ("scr_triplane_backward", i32, i64, vp, i32, i32, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp),
    ("scr_plane_sample_backward", i32, i64, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp),
    ("scr_l1_ssim_scratch_bytes", sz, i32, i32, i32, i32),
    ("scr_l1_ssim_forward", i32, i32, i32, i32, vp, vp, vp, i32, vp, vp),
    ("scr_l1_ssim_backward", i32, i32, i32, i32, *[vp] * 7),
    ("scr_flip_scratch_bytes", sz, i32, i32, i32),
    ("scr_flip_forward", i32, i32, i32, i32, vp, vp, f64, i32, *[vp] * 5),
    ("scr_flip_filters", i32, f64, vp, vp, vp),
    ("scr_scaling_reg_scratch_bytes", sz, i64),
    ("scr_scaling_reg_forward", i32, i64, vp, vp, vp, vp),
    ("scr_scaling_reg_backward", i32, i64, vp, vp, vp, vp),
    ("scr_pair_l1_scratch_bytes", sz, i64),
    ("scr_pair_l1_forward", i32, i64, *[vp] * 7),
    ("scr_pair_l1_backward", i32, i64, *[vp] * 8),
    ("scr_depth_loss_scratch_bytes", sz, i32, i32),
    ("scr_depth_loss_forward", i32, i32, i32, vp, vp, vp, vp, i32, i32, i32, f32, vp, vp, vp),
    ("scr_depth_loss_backward", i32, i32, i32, vp, vp, vp, vp, i32, i32, f32, vp, vp, vp, vp, vp),
    ("scr_anchor_gather_stat_rows", i32, i64),
    ("scr_anchor_gather_stat_buffer_rows", i64, i64),
    ("scr_anchor_gather", i32, i64, *[vp] * 10, i32, vp, vp),
    ("scr_anchor_gather_backward", i32, i64, i64, *[vp] * 7, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, i32, vp),
    ("scr_norm_linear_scratch_bytes", sz, i64),
    ("scr_box_coords", i32, i64, *[vp] * 5),
    ("scr_norm_fold", i32, i32, i32, *[vp] * 10),
    ("scr_norm_fold_backward", i32, i32, i32, *[vp] * 13),
    ("scr_norm_running_stats", i32, i32, i32, *[vp] * 9, i64, vp),
    ("scr_norm_linear_forward", i32, i64, i32, vp, i32, vp, vp, f32, *[vp] * 6, i32, vp),
    ("scr_norm_linear_dx", i32, i64, i32, vp, i32, vp, i32, vp, vp, i32, vp),
    ("scr_norm_linear_backward", i32, i64, i32, vp, i32, vp, i32, vp, vp, vp, vp, i32, *[vp] * 5),
    ("scr_mlp_heads_hidden_bytes", sz, i64),
    ("scr_mlp_heads_partial_bytes", sz, i64),
    ("scr_mlp_heads_forward", i32, i64, vp, i32, *[vp] * 17),
    ("scr_mlp_heads_backward", i32, i64, vp, i32, *[vp] * 28),
    ("scr_statis_compute", i32, i64, i32, vp, vp, vp, vp, i32, vp, vp, vp),
    ("scr_statis_apply", i32, i64, i32, *[vp] * 8),
    ("scr_adam_step", i32, i32, P(AdamTensor), f64, f64, f64, vp),
    ("scr_adam_step_rows", i32, i32, P(AdamTensor), vp, i64, f64, f64, f64, vp),
    ("scr_tv_add_grad", i32, i32, P(TvPlane), vp),
    ("scr_knn_cell_keys", i32, i64, P(f32), vp, vp, vp),
    ("scr_knn", i32, i64, i32, P(f32), *[vp] * 5),
    ("scr_knn3_dist2", i32, i64, P(f32), *[vp] * 5),
    ("scr_knn_curvature", i32, i64, i32, vp, vp, vp, vp),
    ("scr_points_bounds_scratch_bytes", sz, i64),
    ("scr_points_bounds", i32, i64, vp, vp, vp, vp),
    ("scr_voxel_unique_scratch_bytes", sz, i64),
    ("scr_voxel_keys", i32, i64, vp, f32, P(i32), i32, vp, vp),
    ("scr_voxel_unique_plan", i32, i64, vp, vp, P(i64), vp),
    ("scr_voxel_unique_run", i32, i64, vp, vp, f32, P(i32), vp, vp),
    ("scr_filter3d_distance", i32, i64, vp, i32, vp, vp, vp),
    ("scr_filter3d_apply", i32, i64, i32, i64, *[vp] * 7),
    ("scr_filter3d_apply_backward", i32, i64, i32, i64, *[vp] * 9),
    ("scr_copy_probe", i32, vp, vp, sz, vp),
    ("scr_profile_enable", i32, i32),
    ("scr_profile_stride", i32, i32),
    ("scr_profile_read", i32, P(f64), P(i64)),
    ("scr_profile_kernel_name", cp, i32),
    ("scr_markers_enable", i32, i32),
    ("scr_marker_push", i32, cp),
    ("scr_marker_pop", i32),
]
SYMBOLS = [s[0] for s in SIGNATURES]

# A family with a header of its own (include/splatco_bilagrid.h), in the same library: same layout as SIGNATURES, its own
# version.  Launched through family_call(); tests/test_bilagrid_host.py checks every entry against that header.
BILAGRID_ABI_VERSION = 1
BILAGRID_SIGNATURES = [
    ("scr_bilagrid_abi_version", i32),
    ("scr_bilagrid_scratch_bytes", sz, i32, i32, i32, i32, i32),
    ("scr_bilagrid_slice", i32, vp, i32, i32, i32, vp, i32, i32, vp, vp),
    ("scr_bilagrid_slice_backward", i32, vp, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp, sz, vp),
    ("scr_bilagrid_tv_add_grad", i32, vp, vp, i64, i32, i32, i32, f32, vp),
]

# The depth-map normals and the normal-prior loss (include/splatco_normals.h); tests/test_normals_host.py checks every entry.
NORMALS_ABI_VERSION = 1
NORMALS_SIGNATURES = [
    ("scr_normals_abi_version", i32),
    ("scr_normals_map", i32, i32, i32, vp, vp, f64, f64, f64, f64, vp, f32, vp, vp),
    ("scr_normals_map_backward", i32, i32, i32, vp, vp, f64, f64, f64, f64, vp, f32, vp, vp, vp, vp),
    ("scr_normals_loss_scratch_bytes", sz, i32, i32),
    ("scr_normals_loss_forward", i32, i32, i32, vp, vp, vp, vp, i32, f64, f64, f64, f64, f32, vp, vp, vp),
    ("scr_normals_loss_backward", i32, i32, i32, vp, vp, vp, vp, i32, f64, f64, f64, f64, f32, vp, vp, vp, vp),
]


class TsdfView(C.Structure):
    """struct scr_tsdf_view (include/splatco_tsdf.h): one view of scr_tsdf_integrate."""
    _fields_ = [("depth", vp), ("alpha", vp), ("image", vp), ("mask", vp), ("H", i32), ("W", i32), ("mask_kind", i32),
                ("min_alpha", f32), ("fx", f64), ("fy", f64), ("cx", f64), ("cy", f64), ("w2c", f64 * 12), ("near", f64)]


# TSDF fusion and mesh extraction (include/splatco_tsdf.h); tests/test_tsdf_host.py checks every entry and the struct.
TSDF_ABI_VERSION = 1
TSDF_MAX_VIEWS = 16                                 # SCR_TSDF_MAX_VIEWS
TSDF_SIGNATURES = [
    ("scr_tsdf_abi_version", i32),
    ("scr_tsdf_integrate", i32, i32, i32, i32, vp, f32, f64, f32, vp, vp, vp, i32, P(TsdfView), vp),
    ("scr_tsdf_extract_scratch_bytes", sz, i32, i32, i32),
    ("scr_tsdf_extract_vertices_plan", i32, i32, i32, i32, vp, vp, f32, vp, P(i64), vp),
    ("scr_tsdf_extract_vertices_run", i32, i32, i32, i32, vp, f32, vp, vp, vp, f32, vp, i64, vp, vp, vp, vp),
    ("scr_tsdf_extract_faces_plan", i32, i32, i32, i32, vp, vp, f32, vp, P(i64), vp),
    ("scr_tsdf_extract_faces_run", i32, i32, i32, i32, vp, vp, f32, vp, i64, vp, i64, vp, vp),
]

class TsdfsView(C.Structure):
    """struct scr_tsdfs_view (include/splatco_tsdf_sparse.h): the view and the rows of the camera-to-world matrix."""
    _fields_ = [("view", TsdfView), ("c2w", f64 * 12)]


# The block-sparse TSDF volume (include/splatco_tsdf_sparse.h); tests/test_tsdf_sparse_host.py checks every entry and the struct.
TSDFS_ABI_VERSION = 1
TSDFS_BLOCK = 8                                     # SCR_TSDFS_BLOCK
TSDFS_SIGNATURES = [
    ("scr_tsdfs_abi_version", i32),
    ("scr_tsdfs_alloc_scratch_bytes", sz, i32, i32, i32),
    ("scr_tsdfs_alloc_plan", i32, i32, i32, i32, vp, f32, f64, P(TsdfsView), vp, vp, P(i64), vp),
    ("scr_tsdfs_alloc_run", i32, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp),
    ("scr_tsdfs_init_blocks", i32, i64, i64, vp, vp, vp, vp),
    ("scr_tsdfs_integrate", i32, i32, i32, i32, vp, f32, f64, f32, i64, vp, vp, vp, vp, vp, P(TsdfsView), vp),
    ("scr_tsdfs_neighbors", i32, i32, i32, i32, i64, vp, vp, vp),
    ("scr_tsdfs_extract_scratch_bytes", sz, i64),
    ("scr_tsdfs_extract_vertices_plan", i32, i32, i32, i32, i64, i64, i64, vp, vp, vp, vp, vp, f32, vp, P(i64), vp),
    ("scr_tsdfs_extract_vertices_run", i32, i32, i32, i32, vp, f32, i64, i64, i64, vp, vp, vp, vp, vp, vp, f32, vp, i64, vp, vp, vp, vp),
    ("scr_tsdfs_extract_faces_plan", i32, i32, i32, i32, i64, i64, i64, vp, vp, vp, vp, vp, f32, vp, P(i64), vp),
    ("scr_tsdfs_extract_faces_run", i32, i32, i32, i32, i64, i64, i64, vp, vp, vp, vp, vp, f32, vp, i64, vp, i64, vp, vp),
]

# Mesh clean-up: components, size filter, vertex normals (include/splatco_mesh.h); tests/test_mesh_host.py checks every entry.
MESH_ABI_VERSION = 1
MESH_SIGNATURES = [
    ("scr_mesh_abi_version", i32),
    ("scr_mesh_scratch_bytes", sz, i64, i64),
    ("scr_mesh_components", i32, i64, i64, vp, vp, vp, vp, vp, vp),
    ("scr_mesh_roots_plan", i32, i64, vp, vp, vp, P(i64), vp),
    ("scr_mesh_roots_run", i32, i64, vp, vp, vp, i64, vp, vp, vp),
    ("scr_mesh_vertices_plan", i32, i64, vp, vp, i32, vp, P(i64), vp),
    ("scr_mesh_vertices_run", i32, i64, vp, vp, i32, vp, i64, vp, vp, vp, vp, vp, vp),
    ("scr_mesh_faces_plan", i32, i64, vp, vp, vp, i32, vp, P(i64), vp),
    ("scr_mesh_faces_run", i32, i64, vp, vp, vp, i32, vp, i64, vp, vp, vp),
    ("scr_mesh_vertex_normals", i32, i64, i64, vp, vp, vp, vp, vp),
]

# Mesh evaluation: surface sampling, cross-set nearest neighbour, score (include/splatco_surfeval.h);
# tests/test_surfeval_host.py checks every entry.
SURFEVAL_ABI_VERSION = 1
SURFEVAL_MAX_THRESHOLDS = 8                         # SCR_SURFEVAL_MAX_THRESHOLDS
SURFEVAL_SIGNATURES = [
    ("scr_surfeval_abi_version", i32),
    ("scr_surfeval_score_scratch_bytes", sz, i64),
    ("scr_surfeval_face_counts", i32, i64, vp, vp, f64, C.c_uint32, vp, vp),
    ("scr_surfeval_sample", i32, i64, i64, vp, vp, vp, C.c_uint32, vp, vp, vp),
    ("scr_surfeval_nearest", i32, i64, i64, P(f32), vp, vp, vp, vp, vp, f32, vp, vp, vp),
    ("scr_surfeval_score", i32, i64, vp, i32, P(f32), vp, vp, vp),
]
_FAMILY_HEADERS = {"include/splatco_bilagrid.h": BILAGRID_SIGNATURES, "include/splatco_normals.h": NORMALS_SIGNATURES,
                   "include/splatco_tsdf.h": TSDF_SIGNATURES, "include/splatco_tsdf_sparse.h": TSDFS_SIGNATURES,
                   "include/splatco_mesh.h": MESH_SIGNATURES, "include/splatco_surfeval.h": SURFEVAL_SIGNATURES}
_FAMILY_NAMES = frozenset(s[0] for sigs in _FAMILY_HEADERS.values() for s in sigs)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP rasterizer library is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C splatco_amd/csrc`). "
            "There is deliberately no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, restype, *argtypes in (SIGNATURES + BILAGRID_SIGNATURES + NORMALS_SIGNATURES + TSDF_SIGNATURES + TSDFS_SIGNATURES
                                     + MESH_SIGNATURES + SURFEVAL_SIGNATURES):
        if not hasattr(lib, name):
            raise ImportError(f"{LIB_PATH} does not export {name}")
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes
    if lib.scr_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI version {lib.scr_abi_version()}, expected {ABI_VERSION}")
    if lib.scr_bilagrid_abi_version() != BILAGRID_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has bilateral-grid ABI version {lib.scr_bilagrid_abi_version()}, expected {BILAGRID_ABI_VERSION}")
    if lib.scr_normals_abi_version() != NORMALS_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has normals ABI version {lib.scr_normals_abi_version()}, expected {NORMALS_ABI_VERSION}")
    if lib.scr_tsdf_abi_version() != TSDF_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has TSDF ABI version {lib.scr_tsdf_abi_version()}, expected {TSDF_ABI_VERSION}")
    if lib.scr_tsdfs_abi_version() != TSDFS_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has sparse-TSDF ABI version {lib.scr_tsdfs_abi_version()}, expected {TSDFS_ABI_VERSION}")
    if lib.scr_mesh_abi_version() != MESH_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has mesh ABI version {lib.scr_mesh_abi_version()}, expected {MESH_ABI_VERSION}")
    if lib.scr_surfeval_abi_version() != SURFEVAL_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has mesh-evaluation ABI version {lib.scr_surfeval_abi_version()}, expected {SURFEVAL_ABI_VERSION}")
    return lib


lib = _load()


def profile_enable(which, every=1):
    """True / -1: time every kernel class; False / 0: off; a kernel name: only that class.  every: bracket only every
    `every`-th launch of a timed class (the event pair costs ~6 us of stream time around the launch it times)."""
    check(lib.scr_profile_stride(max(int(every), 1)))
    if isinstance(which, str):
        names = [lib.scr_profile_kernel_name(i).decode() for i in range(PROF_COUNT)]
        mask = 1 << names.index(which)
    else:
        mask = -1 if which is True or which == -1 else int(which)
    lib.scr_profile_enable(mask)


MARKERS = False


def markers_enable(on=True):
    """Opt-in roctx stage markers (include/splatco_raster.h, scr_markers_enable): every C-ABI entry point, every kernel class
    and the host stages below open a range that `rocprofv3 --marker-trace` records.  Also switched on by SPLATCO_MARKERS=1
    in the environment when the library is loaded."""
    global MARKERS
    check(lib.scr_markers_enable(1 if on else 0))
    MARKERS = bool(on)


class stage:
    """with stage("rasterize"): ...   A host-side roctx range around a stage of the training iteration (the reference brackets
    the whole iteration with one event pair, train.py:136-137,163,245).  Off (the default): two attribute reads.  On: the
    range is closed behind a device synchronisation, so that the kernels it launched lie INSIDE it on the profiler's
    time line -- marker mode serialises host and device at stage boundaries on purpose; never use it for timing."""
    __slots__ = ("name", "on")

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.on = MARKERS
        if self.on:
            lib.scr_marker_push(self.name.encode())
        return self

    def __exit__(self, *exc):
        if self.on:
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            lib.scr_marker_pop()
        return False


def profile_read():
    """{kernel name: (total ms, launches)} since the last read (HIP events on the launch stream)."""
    ms = (C.c_double * PROF_COUNT)()
    n = (C.c_int64 * PROF_COUNT)()
    check(lib.scr_profile_read(ms, n))
    return {lib.scr_profile_kernel_name(i).decode(): (ms[i], n[i]) for i in range(PROF_COUNT)}


def check(rc):
    if rc != 0:
        raise RuntimeError("splatco_raster: " + lib.scr_last_error().decode())


_check = check          # call()'s `check` parameter shadows the function


def stream(device=None):
    """The caller's current stream ON THE TENSORS' DEVICE (the process may have another device current).  Without a
    device: the current device's, for calls made inside a `torch.cuda.device(...)` block."""
    return torch.cuda.current_stream(device).cuda_stream


def call(name, *args, device=None, check=True):
    """Launches the streamed entry point `name` (an scr_* function whose last header parameter is `void* stream`) with
    `args` followed by the caller's current stream.  A tensor argument becomes its device address, None stays None (NULL),
    everything else (numbers, ctypes arrays and structs, addresses already computed, `ptr(t)`) passes through.

    Kernels launch on the CURRENT device and on the stream they are handed, so both are made the operands' here: the
    device is `device` if given (calls whose operands arrive only in struct tables or pointer arrays must give it),
    otherwise the first tensor argument's; it is current during the call, and the stream is the caller's current stream
    on it.  Every tensor argument must live on that device: ValueError otherwise, before anything is launched.  A non-zero
    status raises through check(); with check=False it is returned instead.  The function is looked up at call time."""
    return _launch(name, args, device, check)


def family_call(name, *args, device=None, check=True):
    """call() for the streamed entry points of the family headers (BILAGRID_SIGNATURES, include/splatco_bilagrid.h;
    NORMALS_SIGNATURES, include/splatco_normals.h; TSDF_SIGNATURES, include/splatco_tsdf.h; TSDFS_SIGNATURES,
    include/splatco_tsdf_sparse.h; MESH_SIGNATURES, include/splatco_mesh.h; SURFEVAL_SIGNATURES, include/splatco_surfeval.h): any other name is refused with ValueError before anything is looked up or launched; everything
    else is call()'s own code."""
    if name not in _FAMILY_NAMES:
        raise ValueError(f"family_call: {name} is not declared in {' or '.join(_FAMILY_HEADERS)}")
    return _launch(name, args, device, check)


def _launch(name, args, device, check):
    fn = getattr(lib, name)
    if device is not None:
        device = torch.device(device)
    argv = list(args)
    for i, a in enumerate(argv):
        if isinstance(a, torch.Tensor):
            if device is None:
                device = a.device
            elif a.device != device:
                raise ValueError(f"{name}: argument {i} is on {a.device}, the launch is on {device}")
            argv[i] = a.data_ptr()
    if device is None:
        raise ValueError(f"{name}: no tensor argument and no device= to launch on")
    if device.index is not None and device.index == torch.cuda.current_device():
        rc = fn(*argv, stream(device))          # already current (every single-GPU run): no guard to enter and leave
    else:
        with torch.cuda.device(device):
            rc = fn(*argv, stream(device))
    if check:
        _check(rc)
    return rc


def ptr(t):
    """A tensor argument: its device address, NULL for None or an empty tensor."""
    return None if t is None or t.numel() == 0 else t.data_ptr()


def host_array(values, ctype=i32):
    """A host array argument (the header's `*_host` parameters): int32 unless another ctype is given."""
    values = list(values)
    return (ctype * len(values))(*values)


def ptr_array(tensors):
    """A host array of the tensors' device addresses (the header's `void* const*` / `float* const*` parameters)."""
    return host_array([t.data_ptr() for t in tensors], vp)


def scratch_size(nbytes):
    """Size class of a large scratch request: above 32 MiB the next multiple of 1/8 of the power of two below it (eight
    classes per octave, at most 12.5 % more than asked).  The buffers behind these requests scale with the number of
    visible anchors / Gaussians / tile instances, which drift from step to step while a scene trains: asked for by the
    byte, a slowly GROWING buffer misses the caching allocator's pool on every step and costs a device allocation each
    time (cfg3: one 1.9 GB hipMalloc per step, 0.4 ms, and 2 GB more reserved per step -- profiles/HISTORY.md, round 5)."""
    n = max(int(nbytes), 1)
    if n < (32 << 20):
        return n
    step = 1 << (n.bit_length() - 4)
    return (n + step - 1) // step * step


def scratch(nbytes, device):
    """Uninitialised device bytes for a kernel's scratch / saved state, in scratch_size() classes."""
    return torch.empty(scratch_size(nbytes), dtype=torch.uint8, device=device)


if os.environ.get("SPLATCO_MARKERS", "") not in ("", "0"):
    markers_enable(True)
