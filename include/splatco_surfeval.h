/* splatco_surfeval.h -- C-ABI of the mesh evaluation (gfx950): a deterministic area-weighted surface sampler, the exact
 * nearest neighbour from one point set into another, and the fused reduction behind accuracy / completeness / Chamfer (DTU)
 * and precision / recall / F-score (Tanks and Temples).  A family of its own next to splatco_raster.h, splatco_bilagrid.h,
 * splatco_normals.h, splatco_tsdf.h and splatco_mesh.h.
 *
 * The functions live in the same libsplatco_raster.so and report through the same scr_last_error() (splatco_raster.h), but
 * they are versioned on their own: SCR_SURFEVAL_ABI_VERSION changes when one of THESE prototypes or definitions changes, and
 * no other version does.  Every streamed function takes the stream last; every pointer is a device address except the stream
 * and the ones named *_host.  A refused call returns 1, launches nothing and leaves "name: ..." in scr_last_error().  No
 * function allocates or synchronises.  The library is built with -ffp-contract=off: the written order is the order.
 *
 * Sampling.  vertices [nv, 3] float32, faces [nf, 3] int32, contiguous, 1 <= nf, 3 nf < 2^31; EVERY face index must lie in
 * [0, nv): the kernels index with them and cannot refuse them; the caller checks (splatco_amd/surface_eval.py).  For face f
 * with corners p0, p1, p2, float32 widened to binary64:
 *   e1 = p1 - p0, e2 = p2 - p0
 *   cx = e1y e2z - e1z e2y, cy = e1z e2x - e1x e2z, cz = e1x e2y - e1y e2x
 *   A  = 0.5 * sqrt((cx cx + cy cy) + cz cz)
 * Random numbers: u32(seed, f, c) = mix(mix(mix(seed) ^ f) ^ c) in uint32, with
 *   mix(x): x ^= x >> 16; x *= 0x21f0aaad; x ^= x >> 15; x *= 0x735a2d97; x ^= x >> 15
 * and U(seed, f, c) = (double)u32(seed, f, c) * 2^-32, which is exact.
 *   n_f = floor(A * density + U(seed, f, 0)): stochastic rounding, the expected count is A * density; n_f = 0 where A is not
 *   finite; n_f = 2^31 where the sum is 2^31 or more (the caller refuses any total of 2^31 or more).
 * scr_surfeval_face_counts writes counts[f] = n_f (int64 [nf]).  The caller forms ends = the INCLUSIVE prefix sum of counts
 * (int64 [nf], integers only) and ns = ends[nf - 1] < 2^31.  Samples are laid out face by face in ascending f, then ascending
 * j: sample s belongs to the first face f with ends[f] > s (binary search, no atomics) and j = s - ends[f - 1] (s for f = 0).
 *   r1 = U(seed, f, 1 + 2 j), r2 = U(seed, f, 2 + 2 j); where r1 + r2 > 1.0 both are replaced by 1.0 - r
 *   point = (p0 + r1 e1) + r2 e2 per coordinate in binary64, rounded to float32 once
 * scr_surfeval_sample writes points [ns, 3] float32 and face_index [ns] int32.  Every output bit is fixed by the definition.
 *
 * Nearest neighbour.  query [nq, 3] and target [nt, 3] float32 with finite coordinates, 1 <= nq, nt < 2^31.
 *   d(i, j) = (ex ex + ey ey) + ez ez in float32 with e = target_j - query_i (knn_grid.h's order)
 *   cap2 = +inf when max_dist < 0 (none), otherwise max_dist * max_dist in float32
 *   dist2[i] = min(cap2, min_j d(i, j))
 *   index[i] = the smallest j with d(i, j) == dist2[i], or -1 where there is none
 * The minimum does not depend on the order of the search and ties are settled by comparing (d, j), never by arrival order, so
 * every output bit is fixed by the definition.
 * The target comes bucketed as scr_knn / scr_knn3_dist2 take it (splatco_raster.h; splatco_amd/knn_grid.py): grid_host[8] =
 * x0, y0, z0, h, nx, ny, nz, slack, sorted_target in cell order, target_id[s] the original index of sorted point s,
 * cell_start[ncells + 1].  The queries come in the order of their CLAMPED cell key in the target's grid (scr_knn_cell_keys
 * under grid_host, then a sort): sorted_query, and query_id[s] the original index at which the result is written.  Neighbours
 * in a wave then walk nearly the same cells.
 * The search (knn_grid.h: knn_grid_search_cross) visits the cells at Chebyshev distance r = 0, 1, 2, ... from the query's
 * clamped cell c, every loop range clipped to the rows and cells that exist: no iteration without a cell behind it.  After
 * shell r an unseen point lies beyond r cells on at least one axis, on a side on which grid exists, and inside the grid's box
 * on every axis.  With t_a = (q_a - x0_a) / h, f_a = t_a - c_a, g_b = max(-t_b, t_b - n_b, 0) the query's distance from the box
 * on axis b in cells,
 *   lower^2 = h^2 min over axes a and EXISTING sides of ((r + f_a)^2 [side below: c_a - r - 1 >= 0]
 *                                                   or (r + 1 - f_a)^2 [side above: c_a + r + 1 <= n_a - 1]) + sum_{b != a} g_b^2
 * bounds the squared distance of everything unseen.  A side below exists only where c_a >= 1, so f_a >= 0; a side above only
 * where c_a <= n_a - 2, so 1 - f_a > 0: for a clamped query the margin is never negative, it GROWS with the distance from the
 * box.  Rounding: t is (q - x0) * (1 / h) in float32, three roundings of relative size 2^-24 each, so t errs by at most
 * 3 * 2^-24 |t|, which for a clamped query is no longer bounded by the grid's size as knn_grid.py's slack assumes; f, 1 - f
 * and r + f add three more of size 2^-24 (|t| + 2 max n); a target's own cell errs by 3 * 2^-24 max n.  All of it is below
 * tol = slack / h + 2^-19 (max_a |t_a| + max n) cells, which is subtracted from every term before it is squared (terms below 0
 * count as 0); the result is scaled by 1 - 2^-16 for the rounding of the squares, of h^2 and of the d compared (6 * 2^-24).
 * The search stops when the best (d, j) has d <= lower^2 and lower^2 > 0, or when no side exists (the cube covers the grid).
 * With max_dist the best starts at cap2, so this is "reach >= max_dist"; a query whose box distance h^2 sum_b g_b^2 (same
 * tolerances) exceeds cap2 returns (cap2, -1) without a search.
 * Bound on the work of one query: with max_dist at most the cells within max_dist + h (1 + tol) of it; without, at most every
 * cell of the grid once plus one step per shell, and there are at most max n shells.
 *
 * Score.  dist2 [n] float32, 1 <= n < 2^31; d = sqrt((double)dist2).  out [10] binary64:
 *   out[0] = sum of d in wg.h's fixed order (a lane adds its items in index order, item = base + lane, + 256, ...; 4096 items
 *            per workgroup; the records of the workgroups are folded by fold_sum): the same bits run after run
 *   out[1] = max of d (0 <= d, NaN-free inputs)
 *   out[2 + k] = the number of d <= (double)thresholds_host[k], k < num_thresholds <= 8, exact integers; 0 for k >= num_thresholds
 * scratch: scr_surfeval_score_scratch_bytes(n) bytes, taken uninitialised.
 */
#ifndef SPLATCO_SURFEVAL_H
#define SPLATCO_SURFEVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCR_SURFEVAL_ABI_VERSION 1
#define SCR_SURFEVAL_MAX_THRESHOLDS 8

int scr_surfeval_abi_version(void);
size_t scr_surfeval_score_scratch_bytes(int64_t n);
int scr_surfeval_face_counts(int64_t nf, const float* vertices, const int32_t* faces, double density, uint32_t seed,
                             int64_t* counts, void* stream);
int scr_surfeval_sample(int64_t nf, int64_t ns, const float* vertices, const int32_t* faces, const int64_t* ends, uint32_t seed,
                        float* points, int32_t* face_index, void* stream);
int scr_surfeval_nearest(int64_t nq, int64_t nt, const float* grid_host, const float* sorted_query, const int64_t* query_id,
                         const float* sorted_target, const int64_t* target_id, const int32_t* cell_start, float max_dist,
                         float* dist2, int32_t* index, void* stream);
int scr_surfeval_score(int64_t n, const float* dist2, int32_t num_thresholds, const float* thresholds_host, void* scratch,
                       double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPLATCO_SURFEVAL_H */
