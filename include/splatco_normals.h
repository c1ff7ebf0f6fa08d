/* splatco_normals.h -- C-ABI of the depth-map normals and the normal-prior loss (gfx950), a family of its own next to
 * splatco_raster.h and splatco_bilagrid.h.
 *
 * The functions live in the same libsplatco_raster.so and report through the same scr_last_error() (splatco_raster.h), but
 * they are versioned on their own: SCR_NORMALS_ABI_VERSION changes when one of THESE prototypes or definitions changes, and
 * SCR_ABI_VERSION does not.  Every streamed function takes the stream last and only enqueues work on it; every pointer but
 * the stream and rot_host is a device address; every map is float32 and contiguous.
 *
 * The maps are those of the rasterizer's image pass, depth D = sum w z and alpha A = sum w, both [H, W], seen by a COLMAP
 * camera (+x right, +y down, +z forward) with the pinhole intrinsics fx, fy, cx, cy in pixels.  Per pixel e = (px, py):
 *   ok(e)     D, A finite, A >= min_alpha, D > 0
 *   z         D / A, ONE binary32 division;   ray = ((px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy, 1);   P = z ray
 *   tx, ty    P(px + 1, py) - P(px - 1, py),  P(px, py + 1) - P(px, py - 1);   c = ty x tx  (fronto-parallel: (0, 0, -1))
 *   valid(e)  the four neighbours lie inside the image, ok holds at e and at all four, and c . c > 1e-24
 *   n         c / |c| at valid pixels, exactly (0, 0, 0) at every other pixel (a hole): the whole one-pixel border, and
 *             every pixel of an image with H < 3 or W < 3
 * A hole gives no loss term and gets no gradient through its own normal, whatever it holds (NaN and Inf included); as a
 * neighbour, an ok pixel still receives the gradient of the valid pixels around it.
 *
 * rot_host: NULL (normals in the camera frame) or nine HOST floats, the row-major camera-to-world rotation R; the map is
 * then R n, and R is a constant of the backward pass.
 *
 * Sizes and scalars are checked first, before any pointer and before anything is launched: H, W >= 0, H W < 2^31, neither
 * side above 2^31 - 257 (such an image has one row or column and no normal; tile indices stay int32), fx, fy finite and > 0, cx, cy finite, min_alpha finite and >= 0, mask_kind in {0, 1, 2}.  A refused call returns 1 and leaves
 * "name: ..." in scr_last_error().  H W == 0 is a no-op that returns 0 whatever the pointers.
 *
 * scr_normals_map: normals[3, H, W]; every element is written.
 * scr_normals_map_backward: d_depth[H, W], d_alpha[H, W] from dL_dnormals[3, H, W] (in the frame of rot_host); either may be
 *   NULL (not computed), every element of the ones given is written, 0.0 at pixels that are not ok.  With h = dL/dn at a
 *   valid pixel: g = (h - (h . n) n) / |c|, dL/dtx = g x ty, dL/dty = tx x g; P(E) gets +dL/dtx, P(W) -dL/dtx, P(S) +dL/dty,
 *   P(N) -dL/dty; dz = ray . dL/dP, dD = dz / A, dA = -dz D / A^2.  A gather in the fixed order W, E, N, S: no atomics, the
 *   same bits run after run.  Nothing is saved by the forward pass.
 * scr_normals_loss_forward: prior[3, H, W] in the camera frame, any length (normalised here); a pixel whose prior is not
 *   finite or has squared length <= 1e-24 is a hole.  mask_kind 0: none (mask ignored); 1: float32 weights m >= 0; 2: uint8,
 *   nonzero = 1; m <= 0 is a hole.  out2 = (L, n_valid),  L = (1 / (H W)) sum_valid m (1 - n . prior / |prior|), each term
 *   rounded to float32, the sum binary64 in the fixed order of the library's workgroup sums, rounded once.  scratch: at
 *   least scr_normals_loss_scratch_bytes(H, W) bytes, taken uninitialised.
 * scr_normals_loss_backward: the same backward with h = -g_up[0] m prior / |prior| / (H W); g_up is ONE float in device
 *   memory (the upstream gradient of L).  The normal map is recomputed, not read.
 */
#ifndef SPLATCO_NORMALS_H
#define SPLATCO_NORMALS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCR_NORMALS_ABI_VERSION 1

int scr_normals_abi_version(void);
int scr_normals_map(int32_t H, int32_t W, const float* depth, const float* alpha, double fx, double fy, double cx, double cy,
                    const float* rot_host, float min_alpha, float* normals, void* stream);
int scr_normals_map_backward(int32_t H, int32_t W, const float* depth, const float* alpha, double fx, double fy, double cx, double cy,
                             const float* rot_host, float min_alpha, const float* dL_dnormals, float* d_depth, float* d_alpha,
                             void* stream);
size_t scr_normals_loss_scratch_bytes(int32_t H, int32_t W);
int scr_normals_loss_forward(int32_t H, int32_t W, const float* depth, const float* alpha, const float* prior, const void* mask,
                             int32_t mask_kind, double fx, double fy, double cx, double cy, float min_alpha, void* scratch,
                             float* out2, void* stream);
int scr_normals_loss_backward(int32_t H, int32_t W, const float* depth, const float* alpha, const float* prior, const void* mask,
                              int32_t mask_kind, double fx, double fy, double cx, double cy, float min_alpha, const float* g_up,
                              float* d_depth, float* d_alpha, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPLATCO_NORMALS_H */
