/* splatco_tsdf.h -- C-ABI of the TSDF fusion of rendered depth maps and of the mesh extraction (gfx950), a family of its own
 * next to splatco_raster.h, splatco_bilagrid.h and splatco_normals.h.
 *
 * The functions live in the same libsplatco_raster.so and report through the same scr_last_error() (splatco_raster.h), but
 * they are versioned on their own: SCR_TSDF_ABI_VERSION changes when one of THESE prototypes or definitions changes, and
 * SCR_ABI_VERSION does not.  Every streamed function takes the stream last; every pointer is a device address except the
 * stream and the ones named *_host.  A refused call returns 1, launches nothing and leaves "name: ..." in scr_last_error().
 *
 * Volume.  Nodes p(i, j, k) = lo + h (i, j, k), 0 <= i < nx, 0 <= j < ny, 0 <= k < nz, every dimension >= 2, nx ny nz < 2^31;
 * linear node index n = (k ny + j) nx + i; tsdf [nz, ny, nx] and weight [nz, ny, nx] float32, optionally colour [3, nz, ny, nx]
 * float32, all contiguous.  A fresh volume holds tsdf = 1, weight = 0, colour = 0.  lo and h are float32 values; trunc, near and
 * the camera are binary64, min_alpha, max_weight and min_weight float32.  ALL arithmetic between the float32 inputs and the
 * float32 outputs is binary64, in the written order, uncontracted.
 *
 * Integrating one view (struct scr_tsdf_view: depth D and alpha A [H, W] float32 of the rasterizer's image pass, optionally an
 * image [3, H, W] float32 and a mask [H, W]; pinhole fx, fy, cx, cy in pixels; w2c the first three ROWS of the world-to-camera
 * matrix, row-major, = world_view_transform^T).  Per node:
 *   1. pc = R p + t, each row ((r0 p.x + r1 p.y) + r2 p.z) + t;  zc = pc.z;  skip the node if zc <= near
 *   2. u = fx pc.x / zc + cx, v = fy pc.y / zc + cy;  px = floor(u), py = floor(v) (pixel px covers [px, px + 1));  skip if
 *      the pixel is outside the image
 *   3. ok: D, A finite, A >= min_alpha, D > 0, and the mask (if given) positive; skip otherwise.  z = D / A, ONE binary32
 *      division (splatco_normals.h).  mask_kind 0: none; 1: float32, > 0; 2: uint8, nonzero
 *   4. sdf = z - zc;  skip if sdf < -trunc;  d = min(1, sdf / trunc)
 *   5. with Wt the stored weight and w = 1:  tsdf <- (tsdf Wt + d w) / (Wt + w);  colour_c <- (colour_c Wt + image_c w) / (Wt + w)
 *      where an image was given and its three values at the pixel are finite (the colour is left alone otherwise);
 *      weight <- min(Wt + w, max_weight);  each rounded to float32 once per view
 * Views are applied in array order.  scr_tsdf_integrate takes 1 .. SCR_TSDF_MAX_VIEWS views and makes ONE pass over the volume
 * for all of them: a thread keeps its nodes in registers across the views.  A batch gives the bits of the same views applied
 * one call each; longer lists are split by the caller, in order.  No atomics: the same bits run after run.
 * Checked before anything is launched: the dimensions, h and trunc finite and > 0, max_weight finite and > 0, lo finite, 1 <=
 * nviews <= SCR_TSDF_MAX_VIEWS, and per view H, W >= 1, H W < 2^31, fx, fy finite and > 0, cx, cy, w2c finite, near finite and
 * >= 0, min_alpha finite and >= 0, mask_kind in {0, 1, 2}, then the pointers (image only with a colour volume).
 *
 * Extraction: marching tetrahedra at level 0.  A cube (i, j, k), i < nx - 1 etc., is valid when all 8 of its nodes have
 * weight > min_weight.  It is cut into the six Kuhn tetrahedra around its main diagonal: tetrahedron q = 0..5 belongs to the
 * axis permutation pi in lexicographic order (xyz, xzy, yxz, yzx, zxy, zyx), its nodes are v0 = corner, v1 = v0 + e_pi1,
 * v2 = v1 + e_pi2, v3 = corner + (1, 1, 1).  A node is inside when tsdf < 0 (exactly 0 is outside).  Lattice edges are
 * (n, dir), dir = 0..6 for the offsets (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1), edge id 7 n + dir.  An edge
 * carries a vertex when its two nodes differ in insideness and it belongs to at least one valid cube.  Vertices are listed in
 * ascending edge id; with a the node of lower linear index (the edge's own n) and b the other, s the tsdf values,
 * t = s_a / (s_a - s_b), position p_a + (p_b - p_a) t, colour c_a + (c_b - c_a) t.  Triangles of a tetrahedron with local
 * nodes 0..3: one inside node a, outside b < c < d: (e(a,b), e(a,c), e(a,d)); one outside node a, inside b < c < d: likewise;
 * inside a < b, outside c < d: the quad e(a,c), e(a,d), e(b,d), e(b,c) split along e(a,c) - e(b,d) into (e(a,c), e(a,d), e(b,d))
 * and (e(a,c), e(b,d), e(b,c)).  Winding: counter-clockwise seen from the outside (tsdf >= 0) side; the last two vertices of
 * a triangle are swapped when bit m of 0x4D24 (m = the 4-bit inside mask, bit x = local node x inside) differs from the parity
 * of pi (0 for xyz, yzx, zxy).  Faces are listed by ascending cube index ((k (ny - 1) + j) (nx - 1) + i), then q, then
 * triangle; indices are int32 positions in the vertex list.  The mesh is indexed and welded: no vertex twice, none unused.
 *
 * Two order-preserving compactions (count, scan, write), each a *_plan that reads ONE count back to the host and a *_run that
 * writes: the 7 nx ny nz edge ids (needs 7 nx ny nz < 2^31), then the 12 triangle slots of every cube (12 (nx - 1)(ny - 1)
 * (nz - 1) < 2^31).  scratch: scr_tsdf_extract_scratch_bytes() bytes, taken uninitialised, the same block for a plan and its
 * run; it may be reused for the second compaction after the first run.  edge_ids [nv] int32 is the sorted list of kept edge
 * ids the faces are looked up in (binary search; there is no dense edge-to-vertex map).  A run with nv or nf == 0 is a no-op.
 */
#ifndef SPLATCO_TSDF_H
#define SPLATCO_TSDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCR_TSDF_ABI_VERSION 1
#define SCR_TSDF_MAX_VIEWS 16

typedef struct scr_tsdf_view {
    const float* depth;
    const float* alpha;
    const float* image;
    const void* mask;
    int32_t H, W;
    int32_t mask_kind;
    float min_alpha;
    double fx, fy, cx, cy;
    double w2c[12];
    double near;
} scr_tsdf_view;

int scr_tsdf_abi_version(void);
int scr_tsdf_integrate(int32_t nx, int32_t ny, int32_t nz, const float* lo_host, float h, double trunc, float max_weight,
                       float* tsdf, float* weight, float* color, int32_t nviews, const scr_tsdf_view* views_host, void* stream);
size_t scr_tsdf_extract_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);
int scr_tsdf_extract_vertices_plan(int32_t nx, int32_t ny, int32_t nz, const float* tsdf, const float* weight, float min_weight,
                                   void* scratch, int64_t* count_host, void* stream);
int scr_tsdf_extract_vertices_run(int32_t nx, int32_t ny, int32_t nz, const float* lo_host, float h, const float* tsdf,
                                  const float* weight, const float* color, float min_weight, const void* scratch, int64_t nv,
                                  int32_t* edge_ids, float* vertices, float* colors, void* stream);
int scr_tsdf_extract_faces_plan(int32_t nx, int32_t ny, int32_t nz, const float* tsdf, const float* weight, float min_weight,
                                void* scratch, int64_t* count_host, void* stream);
int scr_tsdf_extract_faces_run(int32_t nx, int32_t ny, int32_t nz, const float* tsdf, const float* weight, float min_weight,
                               const void* scratch, int64_t nv, const int32_t* edge_ids, int64_t nf, int32_t* faces, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPLATCO_TSDF_H */
