// splatco_amd/csrc/knn_grid.h -- exact nearest-neighbour search over a uniform grid of cells, written once (gfx950): the
// grid descriptor, the cell function and the search behind the curvature kNN (densify.hip: knn_kernel<K>) and the fused
// 3-NN distances (scene_init.hip: knn3_dist2_kernel).  The host half -- cell size, slack, bucketing -- is
// splatco_amd/knn_grid.py.
//
// The points come sorted by cell (knn_cell_keys_kernel + the caller's sort; cell_start[ncells + 1]).  One thread per
// query, in cell order, walks the cube of cells around its own -- the cells of one (y, z) row are ONE contiguous range of
// the sorted points -- and grows the cube shell by shell until the worst distance it keeps lies inside what it has
// searched.  What "keeps" means is the caller's policy:
//   struct Best { __device__ void offer(float d, int p);        // d: squared distance of sorted point p, INFINITY for
//                                                               //    the query itself
//                 __device__ float worst() const; };            // the search may stop once worst() <= reach^2
// Arithmetic order is normative (-ffp-contract=off): e = p_j - p_i, d = (ex*ex + ey*ey) + ez*ez.
#pragma once
#include "capi.h"        // fail(): both users define entry points

#include <math.h>

namespace scr {

struct KnnGrid {
    float x0, y0, z0, inv_h, h, slack;
    int nx, ny, nz;
};

// from the C-ABI's grid_host[8] = x0, y0, z0, h, nx, ny, nz, slack
inline __host__ KnnGrid knn_grid(const float* g8) {
    KnnGrid g;
    g.x0 = g8[0]; g.y0 = g8[1]; g.z0 = g8[2]; g.h = g8[3]; g.inv_h = 1.0f / g8[3];
    g.nx = (int)g8[4]; g.ny = (int)g8[5]; g.nz = (int)g8[6]; g.slack = g8[7];
    return g;
}

// the one grid descriptor check of scr_knn_cell_keys, scr_knn and scr_knn3_dist2: the kernels index points and cells with int
inline __host__ int check_knn_grid(const char* who, int64_t N, const float* g) {
    if (N <= 0 || N >= (1ll << 31)) return fail("%s: need 0 < N < 2^31", who);
    if (!g) return fail("%s: grid_host is NULL", who);
    if (!(g[3] > 0.0f) || g[4] < 1 || g[5] < 1 || g[6] < 1 || !(g[7] >= 0.0f)) return fail("%s: bad grid", who);
    if ((double)g[4] * g[5] * g[6] >= 2147483647.0) return fail("%s: more than 2^31 - 2 cells", who);
    return 0;
}

// the ONE cell function: the bucketing kernel and the search both call it, so a point's bucket is the cell the search
// believes it is in
__device__ __forceinline__ int knn_cell(float v, float lo, float inv_h, int n) {
    const int c = (int)floorf((v - lo) * inv_h);
    return c < 0 ? 0 : (c >= n ? n - 1 : c);
}

// Offers every point the query at sorted position s may need to `best`.  The row scan has ONE call site, a loop over
// the row's one or two ranges: with a call site per range the K-wide insertion of knn_kernel<K> is inlined three times,
// which costs it a wave of occupancy (156 against 100 VGPRs at K = 16), and the 3-NN kernel keeps its times with this
// form (profiles/r14_knn_grid.txt).
template <class Best>
__device__ __forceinline__ void knn_grid_search(int64_t s, const KnnGrid& gr, const float* __restrict__ sorted_pts,
                                                const int32_t* __restrict__ cell_start, Best& best) {
    const float qx = sorted_pts[3 * s], qy = sorted_pts[3 * s + 1], qz = sorted_pts[3 * s + 2];
    const int cx = knn_cell(qx, gr.x0, gr.inv_h, gr.nx), cy = knn_cell(qy, gr.y0, gr.inv_h, gr.ny),
              cz = knn_cell(qz, gr.z0, gr.inv_h, gr.nz);
    // distance from the query to the faces of its own cell, in cells: the cube of radius r reaches at least (r + that) * h
    const float fx = (qx - gr.x0) * gr.inv_h - (float)cx, fy = (qy - gr.y0) * gr.inv_h - (float)cy,
                fz = (qz - gr.z0) * gr.inv_h - (float)cz;
    const float margin = gr.h * fminf(fminf(fminf(fx, 1.0f - fx), fminf(fy, 1.0f - fy)), fminf(fz, 1.0f - fz));
    const int rmax = max(gr.nx, max(gr.ny, gr.nz));
    for (int r = 1; r <= rmax; ++r) {                       // r = 1 takes the whole 3x3x3 cube, r > 1 the cube's surface
        for (int dz = -r; dz <= r; ++dz) {
            const int z = cz + dz;
            if (z < 0 || z >= gr.nz) continue;
            for (int dy = -r; dy <= r; ++dy) {
                const int y = cy + dy;
                if (y < 0 || y >= gr.ny) continue;
                const int64_t row = ((int64_t)z * gr.ny + y) * gr.nx;
                // a row of the surface's top, bottom, front or back (and every row at r = 1): cells cx - r .. cx + r,
                // one range; any other row: the two end cells, each a range if it is inside the grid
                const bool whole = r == 1 || dz == -r || dz == r || dy == -r || dy == r;
                for (int side = 0; side < (whole ? 1 : 2); ++side) {
                    const int xa = whole ? max(cx - r, 0) : (side ? cx + r : cx - r);
                    const int xb = whole ? min(cx + r, gr.nx - 1) : xa;
                    if (xa < 0 || xb >= gr.nx) continue;
                    const int p1 = cell_start[row + xb + 1];
                    for (int p = cell_start[row + xa]; p < p1; ++p) {
                        const float ex = sorted_pts[3 * (int64_t)p] - qx, ey = sorted_pts[3 * (int64_t)p + 1] - qy,
                                    ez = sorted_pts[3 * (int64_t)p + 2] - qz;
                        best.offer(p == s ? INFINITY : (ex * ex + ey * ey) + ez * ez, p);
                    }
                }
            }
        }
        // every point closer than `reach` has been seen; slack: the rounding of the cell function (knn_grid.py)
        const float reach = (float)r * gr.h + margin - gr.slack;
        if (reach > 0.0f && best.worst() <= reach * reach) break;
    }
}

}  // namespace scr
