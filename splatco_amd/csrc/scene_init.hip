// splatco_amd/csrc/scene_init.hip -- a scene from a point cloud on the device (gfx950): the kernels behind
// splatco_amd/scene_init.py (GaussianModel.create_from_pcd / voxelize_sample, scene/gaussian_model.py:447-451,472-508,
// and simple_knn's distCUDA2, whose source is not in the reference tree -- the arithmetic below is this project's
// specification of it, see scene_init.py).
//
//   points_bounds   per-axis min / max and a non-finite flag of the cloud (12 B read per point).
//   voxel_keys      q = rint(p / v) per component (binary32 division, round half to even); packed: one 63-bit key
//                   (qx - lo_x) << 42 | (qy - lo_y) << 21 | (qz - lo_z), whose integer order is the lexicographic order
//                   of (qx, qy, qz) -- what np.unique(axis=0) returns; unpacked (an axis needs more than 21 bits): the
//                   three integers, for the caller's lexicographic row sort.  12 B read, 8 B written per point.
//   voxel_unique    on the SORTED keys: head flags (key[i] != key[i-1]) compacted with the count / scan / write scheme
//                   of compact.h, decode to float32(q) * v.  8 B read per key in each pass, 12 B written per survivor.
//   knn_cell_keys   every point's cell of the uniform grid of knn_grid.h, for this file's search and for densify.hip's.
//   knn3_dist2      mean of the squared distances to the 3 nearest OTHER points, fused: the grid search of knn_grid.h
//                   keeping three distances in registers.  Writes 4 B per point; no index array, no gather.
//
// Arithmetic order is normative (-ffp-contract=off): e = p_j - p_i, d = (ex*ex + ey*ey) + ez*ez, ((b0 + b1) + b2) / 3.
// The three smallest VALUES are unique whatever the tie-breaking, so the result is independent of the search order and
// bit-identical to a brute force.  No atomics.
#include "knn_grid.h"

#include <math.h>

namespace scr {

constexpr int SI_THREADS = 256;                       // block size of the bounds, keys and kNN kernels

// ------------------------------------------------------------------ bounding box
// min / max of every axis and a non-finite flag, in two passes of plain reductions (no atomics): torch.aminmax(dim=0) of a
// [10 M, 3] tensor took 5 ms of the 6.6 ms of a whole voxelize call (profiles/r07_scene_init.txt).  fminf / fmaxf drop a
// NaN, so the flag is what reports it.
constexpr int SI_BOUNDS_PER_WG = SI_THREADS * 16;     // points per workgroup of the first pass

struct Bounds7 { float v[7]; };       // min x, y, z, max x, y, z, flag (> 0: a coordinate is NaN or infinite)

__device__ __forceinline__ void bounds_merge(Bounds7& a, const Bounds7& b) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.v[c] = fminf(a.v[c], b.v[c]); a.v[3 + c] = fmaxf(a.v[3 + c], b.v[3 + c]); }
    a.v[6] = fmaxf(a.v[6], b.v[6]);
}

// the workgroup's merged value, valid in thread 0
__device__ __forceinline__ Bounds7 bounds_reduce_wg(Bounds7 a) {
    __shared__ float part[SI_THREADS / WAVE][7];
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
        Bounds7 o;
#pragma unroll
        for (int c = 0; c < 7; ++c) o.v[c] = __shfl_xor(a.v[c], d, WAVE);
        bounds_merge(a, o);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 7; ++c) part[threadIdx.x >> 6][c] = a.v[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SI_THREADS / WAVE; ++w) {
            Bounds7 o;
#pragma unroll
            for (int c = 0; c < 7; ++c) o.v[c] = part[w][c];
            bounds_merge(a, o);
        }
    }
    return a;
}

__device__ __forceinline__ Bounds7 bounds_identity() {
    Bounds7 a;
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.v[c] = INFINITY; a.v[3 + c] = -INFINITY; }
    a.v[6] = 0.0f;
    return a;
}

__global__ void __launch_bounds__(SI_THREADS)
points_bounds_kernel(int64_t N, const float* __restrict__ pts, float* __restrict__ partial) {
    Bounds7 a = bounds_identity();
    const int64_t base = (int64_t)blockIdx.x * SI_BOUNDS_PER_WG + threadIdx.x;
#pragma unroll 4
    for (int j = 0; j < SI_BOUNDS_PER_WG / SI_THREADS; ++j) {
        const int64_t i = base + (int64_t)j * SI_THREADS;
        if (i < N) {
            Bounds7 o;
            o.v[0] = o.v[3] = pts[3 * i]; o.v[1] = o.v[4] = pts[3 * i + 1]; o.v[2] = o.v[5] = pts[3 * i + 2];
            o.v[6] = (fabsf(o.v[0]) <= 3.4028235e38f && fabsf(o.v[1]) <= 3.4028235e38f && fabsf(o.v[2]) <= 3.4028235e38f) ? 0.0f : 1.0f;
            bounds_merge(a, o);
        }
    }
    a = bounds_reduce_wg(a);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 7; ++c) partial[(size_t)blockIdx.x * 8 + c] = a.v[c];
    }
}

__global__ void __launch_bounds__(SI_THREADS)
points_bounds_final_kernel(int64_t nwg, const float* __restrict__ partial, float* __restrict__ out) {
    Bounds7 a = bounds_identity();
    for (int64_t w = threadIdx.x; w < nwg; w += SI_THREADS) {
        Bounds7 o;
#pragma unroll
        for (int c = 0; c < 7; ++c) o.v[c] = partial[(size_t)w * 8 + c];
        bounds_merge(a, o);
    }
    a = bounds_reduce_wg(a);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 7; ++c) out[c] = a.v[c];
    }
}

static size_t points_bounds_nwg(int64_t N) { return (size_t)((N + SI_BOUNDS_PER_WG - 1) / SI_BOUNDS_PER_WG); }

// ------------------------------------------------------------------ voxel keys
__global__ void __launch_bounds__(SI_THREADS)
voxel_keys_kernel(int64_t N, const float* __restrict__ pts, float v, int lox, int loy, int loz, int packed,
                  int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * SI_THREADS + threadIdx.x;
    if (i >= N) return;
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    // |q| < 2^31 and, packed, 0 <= q - lo < 2^21: the caller checked both on the cloud's bounding box (rint(x / v) is
    // monotone in x)
    const int64_t qx = (int64_t)rintf(x / v), qy = (int64_t)rintf(y / v), qz = (int64_t)rintf(z / v);
    if (packed) {
        out[i] = ((qx - lox) << 42) | ((qy - loy) << 21) | (qz - loz);
    } else {
        out[3 * i] = qx; out[3 * i + 1] = qy; out[3 * i + 2] = qz;
    }
}

// a sorted key is kept where a run of equal keys begins
struct KeepHead {
    struct Operand { int64_t k, prev; };
    const int64_t* __restrict__ keys;
    __device__ Operand load(int64_t c) const { return {keys[c], keys[max(c - 1, (int64_t)0)]}; }
    __device__ bool keep(const Operand& o, int64_t i) const { return i == 0 || o.k != o.prev; }
};

__global__ void __launch_bounds__(COMPACT_THREADS)
voxel_unique_write_kernel(int64_t n, KeepHead head, const uint32_t* __restrict__ wg_offset, float v, int lox, int loy, int loz,
                          float* __restrict__ out) {
    const CompactRank<KeepHead> c = compact_rank(n, head, wg_offset);
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) {
        if (c.keep[r]) {
            const int64_t k = c.v[r].k;
            const size_t o = 3 * (size_t)c.pos[r];
            out[o] = (float)((int)(k >> 42) + lox) * v;
            out[o + 1] = (float)((int)((k >> 21) & 0x1fffff) + loy) * v;
            out[o + 2] = (float)((int)(k & 0x1fffff) + loz) * v;
        }
    }
}

// ------------------------------------------------------------------ fused 3-NN mean squared distance
__global__ void __launch_bounds__(SI_THREADS)
knn_cell_keys_kernel(int64_t N, KnnGrid gr, const float* __restrict__ pts, int64_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * SI_THREADS + threadIdx.x;
    if (i >= N) return;
    const int cx = knn_cell(pts[3 * i], gr.x0, gr.inv_h, gr.nx), cy = knn_cell(pts[3 * i + 1], gr.y0, gr.inv_h, gr.ny),
              cz = knn_cell(pts[3 * i + 2], gr.z0, gr.inv_h, gr.nz);
    keys[i] = ((int64_t)cz * gr.ny + cy) * gr.nx + cx;
}

// the three smallest distances so far, ascending; values only
struct Best3 {
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
    __device__ __forceinline__ void offer(float d, int) {       // branch-free insertion into the ascending triple
        float t = d;
        const float n0 = fminf(b0, t); t = fmaxf(b0, t);
        const float n1 = fminf(b1, t); t = fmaxf(b1, t);
        b2 = fminf(b2, t); b1 = n1; b0 = n0;
    }
    __device__ __forceinline__ float worst() const { return b2; }
};

// sorted_pts: the points in cell order; sorted_id[s]: original index of sorted point s; cell_start[ncells + 1].
// out[original index] = ((b0 + b1) + b2) / 3 of the three smallest squared distances to OTHER points (by position:
// an exact duplicate is another point, at distance 0).
__global__ void __launch_bounds__(SI_THREADS)
knn3_dist2_kernel(int64_t N, KnnGrid gr, const float* __restrict__ sorted_pts, const int64_t* __restrict__ sorted_id,
                 const int32_t* __restrict__ cell_start, float* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * SI_THREADS + threadIdx.x;      // position in cell order: neighbours in memory
    if (s >= N) return;
    Best3 best;
    knn_grid_search(s, gr, sorted_pts, cell_start, best);
    out[sorted_id[s]] = ((best.b0 + best.b1) + best.b2) / 3.0f;
}

static int check_voxel_args(const char* who, int64_t N, float voxel_size, const int32_t* lo_host) {
    if (N <= 0 || N >= (1ll << 31)) return fail("%s: need 0 < N < 2^31", who);
    if (!(voxel_size > 0.0f) || !(voxel_size <= 3.0e38f)) return fail("%s: voxel_size must be positive and finite", who);
    if (!lo_host) return fail("%s: lo_host is NULL", who);
    return 0;
}

}  // namespace scr

using namespace scr;

extern "C" {

size_t scr_voxel_unique_scratch_bytes(int64_t N) { return compact_scratch_bytes(N > 0 ? N : 1); }

size_t scr_points_bounds_scratch_bytes(int64_t N) { return align_up(points_bounds_nwg(N > 0 ? N : 1) * 8 * sizeof(float)); }

int scr_points_bounds(int64_t N, const float* points, void* scratch, float* out7, void* stream) {
    SCR_MARK_FN;
    if (N <= 0 || N >= (1ll << 31)) return fail("scr_points_bounds: need 0 < N < 2^31");
    if (!points || !scratch || !out7) return fail("scr_points_bounds: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const size_t nwg = points_bounds_nwg(N);
    points_bounds_kernel<<<(unsigned)nwg, SI_THREADS, 0, st>>>(N, points, (float*)scratch);
    points_bounds_final_kernel<<<1, SI_THREADS, 0, st>>>((int64_t)nwg, (float*)scratch, out7);
    CHECK_LAUNCH("points_bounds_kernel", 0, st);
    return 0;
}

int scr_voxel_keys(int64_t N, const float* points, float voxel_size, const int32_t* lo_host, int32_t packed, int64_t* out,
                   void* stream) {
    SCR_MARK_FN;
    if (check_voxel_args("scr_voxel_keys", N, voxel_size, lo_host)) return 1;
    if (!points || !out) return fail("scr_voxel_keys: NULL argument");
    voxel_keys_kernel<<<(unsigned)((N + SI_THREADS - 1) / SI_THREADS), SI_THREADS, 0, (hipStream_t)stream>>>(
        N, points, voxel_size, lo_host[0], lo_host[1], lo_host[2], packed != 0, out);
    CHECK_LAUNCH("voxel_keys_kernel", 0, (hipStream_t)stream);
    return 0;
}

int scr_voxel_unique_plan(int64_t N, const int64_t* sorted_keys, void* scratch, int64_t* num_unique_host, void* stream) {
    SCR_MARK_FN;
    if (!num_unique_host) return fail("num_unique_host is NULL");
    *num_unique_host = 0;
    if (N <= 0 || N >= (1ll << 31)) return fail("scr_voxel_unique_plan: need 0 < N < 2^31");
    if (!sorted_keys || !scratch) return fail("scr_voxel_unique_plan: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    return compact_plan("compact_count_kernel<KeepHead>", N, scratch, num_unique_host, st,
                        [&](const CompactScratch& s, unsigned long long* mb, unsigned long long seq) {
                            launch_compact_count(N, KeepHead{sorted_keys}, s, mb, seq, st);
                        });
}

int scr_voxel_unique_run(int64_t N, const int64_t* sorted_keys, const void* scratch, float voxel_size,
                         const int32_t* lo_host, float* out_xyz, void* stream) {
    SCR_MARK_FN;
    if (check_voxel_args("scr_voxel_unique_run", N, voxel_size, lo_host)) return 1;
    if (!sorted_keys || !scratch || !out_xyz) return fail("scr_voxel_unique_run: NULL argument");
    voxel_unique_write_kernel<<<(uint32_t)compact_nwg(N), COMPACT_THREADS, 0, (hipStream_t)stream>>>(
        N, KeepHead{sorted_keys}, (const uint32_t*)scratch, voxel_size, lo_host[0], lo_host[1], lo_host[2], out_xyz);
    CHECK_LAUNCH("voxel_unique_write_kernel", 0, (hipStream_t)stream);
    return 0;
}

int scr_knn_cell_keys(int64_t N, const float* grid_host, const float* points, int64_t* keys, void* stream) {
    SCR_MARK_FN;
    if (check_knn_grid("scr_knn_cell_keys", N, grid_host)) return 1;
    if (!points || !keys) return fail("scr_knn_cell_keys: NULL argument");
    knn_cell_keys_kernel<<<(unsigned)((N + SI_THREADS - 1) / SI_THREADS), SI_THREADS, 0, (hipStream_t)stream>>>(
        N, knn_grid(grid_host), points, keys);
    CHECK_LAUNCH("knn_cell_keys_kernel", 0, (hipStream_t)stream);
    return 0;
}

int scr_knn3_dist2(int64_t N, const float* grid_host, const float* sorted_pts, const int64_t* sorted_id,
                   const int32_t* cell_start, float* out, void* stream) {
    SCR_MARK_FN;
    if (check_knn_grid("scr_knn3_dist2", N, grid_host)) return 1;
    if (N < 4) return fail("scr_knn3_dist2: fewer than 4 points");
    if (!sorted_pts || !sorted_id || !cell_start || !out) return fail("scr_knn3_dist2: NULL argument");
    knn3_dist2_kernel<<<(unsigned)((N + SI_THREADS - 1) / SI_THREADS), SI_THREADS, 0, (hipStream_t)stream>>>(
        N, knn_grid(grid_host), sorted_pts, sorted_id, cell_start, out);
    CHECK_LAUNCH("knn3_dist2_kernel", 0, (hipStream_t)stream);
    return 0;
}

}  // extern "C"
