// splatco_amd/csrc/knn_grid.h -- exact nearest-neighbour search over a uniform grid of cells, written once (gfx950): the
// grid descriptor, the cell function and the search behind the curvature kNN (densify.hip: knn_kernel<K>) and the fused
// 3-NN distances (scene_init.hip: knn3_dist2_kernel), and below it the search from ANOTHER set into the bucketed one
// (surfeval.hip: surfeval_nearest_kernel).  The host half -- cell size, slack, bucketing -- is splatco_amd/knn_grid.py.
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

// ------------------------------------------------------------------ a query that is NOT a point of the bucketed set
// (surfeval.hip: surfeval_nearest_kernel; the definition, the bound and its rounding argument are include/splatco_surfeval.h's).
// Nothing knn_grid_search relies on holds: the query may lie far outside the box, its cell is a clamped one, and nothing may
// turn up for many shells.  So every loop range is clipped to the rows and cells that exist -- an iteration always has a cell
// behind it: a query visits at most every cell once plus one step per shell, and a line-shaped grid of 8 N + 64 cells costs
// that many steps, not their square -- and the stop test counts only the sides of the cube on which grid is left.

// one row's cells xa .. xb (inside the grid): ONE contiguous range of the sorted points
template <class Best>
__device__ __forceinline__ void knn_cross_row(int64_t row, int xa, int xb, float qx, float qy, float qz,
                                              const float* __restrict__ sorted_pts, const int32_t* __restrict__ cell_start, Best& best) {
    const int p1 = cell_start[row + xb + 1];
    for (int p = cell_start[row + xa]; p < p1; ++p) {
        const float ex = sorted_pts[3 * (int64_t)p] - qx, ey = sorted_pts[3 * (int64_t)p + 1] - qy,
                    ez = sorted_pts[3 * (int64_t)p + 2] - qz;
        best.offer((ex * ex + ey * ey) + ez * ez, p);
    }
}

// the lower bound of one side of the cube, in cells squared: (r + margin - tol)^2 + the other axes' distances from the box
__device__ __forceinline__ float knn_cross_side(float low, bool exists, float along, float tol, float others) {
    const float s = fmaxf(along - tol, 0.0f);
    return exists ? fminf(low, s * s + others) : low;
}

// Best: offer(d, p) as above and worst(); best.worst() starts at the cap (INFINITY: none).  Returns with every point offered
// that can have d <= worst(), ties included.
template <class Best>
__device__ __forceinline__ void knn_grid_search_cross(float qx, float qy, float qz, const KnnGrid& gr,
                                                      const float* __restrict__ sorted_pts,
                                                      const int32_t* __restrict__ cell_start, Best& best) {
    const float tx = (qx - gr.x0) * gr.inv_h, ty = (qy - gr.y0) * gr.inv_h, tz = (qz - gr.z0) * gr.inv_h;
    // knn_cell's cell, clamped BEFORE the conversion: t may be far outside what an int holds
    const int cx = (int)fminf(fmaxf(floorf(tx), 0.0f), (float)(gr.nx - 1)), cy = (int)fminf(fmaxf(floorf(ty), 0.0f), (float)(gr.ny - 1)),
              cz = (int)fminf(fmaxf(floorf(tz), 0.0f), (float)(gr.nz - 1));
    const float fx = tx - (float)cx, fy = ty - (float)cy, fz = tz - (float)cz;
    const int nmax = max(gr.nx, max(gr.ny, gr.nz));
    const float tol = gr.slack * gr.inv_h + 0x1p-19f * (fmaxf(fmaxf(fabsf(tx), fabsf(ty)), fabsf(tz)) + (float)nmax);
    const float scale = gr.h * gr.h * (1.0f - 0x1p-16f);
    // distance from the grid's box per axis, in cells (0 inside)
    const float gx = fmaxf(fmaxf(-tx, tx - (float)gr.nx) - tol, 0.0f), gy = fmaxf(fmaxf(-ty, ty - (float)gr.ny) - tol, 0.0f),
                gz = fmaxf(fmaxf(-tz, tz - (float)gr.nz) - tol, 0.0f);
    const float ox = gy * gy + gz * gz, oy = gx * gx + gz * gz, oz = gx * gx + gy * gy;
    if (((gx * gx + gy * gy) + gz * gz) * scale > best.worst()) return;          // further than the cap from everything
    for (int r = 0;; ++r) {
        const int y0 = max(cy - r, 0), y1 = min(cy + r, gr.ny - 1), x0 = max(cx - r, 0), x1 = min(cx + r, gr.nx - 1);
        // the cube's two z faces: whole rows
        for (int side = 0; side < (r ? 2 : 1); ++side) {
            const int z = side ? cz + r : cz - r;
            if (z < 0 || z >= gr.nz) continue;
            for (int y = y0; y <= y1; ++y)
                knn_cross_row(((int64_t)z * gr.ny + y) * gr.nx, x0, x1, qx, qy, qz, sorted_pts, cell_start, best);
        }
        if (r) {
            const int zi0 = max(cz - r + 1, 0), zi1 = min(cz + r - 1, gr.nz - 1);
            // the two y faces between them: whole rows
            for (int side = 0; side < 2; ++side) {
                const int y = side ? cy + r : cy - r;
                if (y < 0 || y >= gr.ny) continue;
                for (int z = zi0; z <= zi1; ++z)
                    knn_cross_row(((int64_t)z * gr.ny + y) * gr.nx, x0, x1, qx, qy, qz, sorted_pts, cell_start, best);
            }
            // the two x faces between those: single cells
            const int yi0 = max(cy - r + 1, 0), yi1 = min(cy + r - 1, gr.ny - 1);
            for (int side = 0; side < 2; ++side) {
                const int x = side ? cx + r : cx - r;
                if (x < 0 || x >= gr.nx) continue;
                for (int z = zi0; z <= zi1; ++z)
                    for (int y = yi0; y <= yi1; ++y)
                        knn_cross_row(((int64_t)z * gr.ny + y) * gr.nx, x, x, qx, qy, qz, sorted_pts, cell_start, best);
            }
        }
        // what is unseen lies beyond the cube on a side on which grid is left
        const float fr = (float)r;
        float low = INFINITY;
        low = knn_cross_side(low, cx - r - 1 >= 0, fr + fx, tol, ox);
        low = knn_cross_side(low, cx + r + 1 < gr.nx, fr + (1.0f - fx), tol, ox);
        low = knn_cross_side(low, cy - r - 1 >= 0, fr + fy, tol, oy);
        low = knn_cross_side(low, cy + r + 1 < gr.ny, fr + (1.0f - fy), tol, oy);
        low = knn_cross_side(low, cz - r - 1 >= 0, fr + fz, tol, oz);
        low = knn_cross_side(low, cz + r + 1 < gr.nz, fr + (1.0f - fz), tol, oz);
        // no side left: the cube covers the grid (integers only: this is what ends the loop, after fewer than max n shells)
        if (cx - r - 1 < 0 && cx + r + 1 >= gr.nx && cy - r - 1 < 0 && cy + r + 1 >= gr.ny && cz - r - 1 < 0 && cz + r + 1 >= gr.nz) break;
        const float reach2 = low * scale;
        if (reach2 > 0.0f && reach2 < INFINITY && best.worst() <= reach2) break;
    }
}

}  // namespace scr
