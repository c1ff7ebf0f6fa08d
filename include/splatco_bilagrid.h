/* splatco_bilagrid.h -- C-ABI of the per-view bilateral grids (gfx950), a family of its own next to splatco_raster.h.
 *
 * The functions live in the same libsplatco_raster.so and report through the same scr_last_error() (splatco_raster.h), but
 * they are versioned on their own: SCR_BILAGRID_ABI_VERSION changes when one of THESE prototypes or definitions changes, and
 * SCR_ABI_VERSION does not.  Every streamed function takes the stream last and only enqueues work on it; every pointer but
 * the stream is a device address; everything is float32 and contiguous.
 *
 * A grid is G[12, L, Gh, Gw]: channel 4 i + j holds A[i][j] of a 3x4 affine colour transform.  For pixel (px, py) of an
 * image rgb[3, H, W]:
 *   u = (px + 0.5) / W (Gw - 1),  v = (py + 0.5) / H (Gh - 1),  z = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1) (L - 1)
 *   A(px, py) = the trilinear interpolation of G at (z, v, u);   out = A[:, :3] rgb + A[:, 3]
 * Gradients: to G the trilinear weights times the outer product of dL/dout and [r, g, b, 1]; to rgb A[:, :3]^T dL/dout plus
 * the term through z, ((dA/dz [rgb; 1]) . dL/dout) (L - 1) (0.299, 0.587, 0.114), which is exactly zero where the unclamped
 * luminance is <= 0 or >= 1.  Finite inputs are a precondition.
 *
 * Sizes are checked first, before any pointer and before anything is launched: 2 <= L <= 16, 2 <= Gh, Gw <= 64, H, W >= 0,
 * H W < 2^31.  A refused call returns 1 and leaves "name: ..." in scr_last_error().  H W == 0 (and N == 0) is a no-op that
 * returns 0 whatever the pointers.
 *
 * scr_bilagrid_slice: out[3, H, W].
 * scr_bilagrid_slice_backward: dL_drgb[3, H, W] and dL_dgrid[12, L, Gh, Gw], either may be NULL (not computed).  Every element
 *   of the ones given is written; vertices no pixel reaches get zeros.  dL_dgrid needs scratch of at least
 *   scr_bilagrid_scratch_bytes(L, Gh, Gw, H, W) bytes, taken uninitialised.  No atomics: every sum has the order of the
 *   library's workgroup sums, so a result is the same bits run after run.
 * scr_bilagrid_tv_add_grad: grids[N, 12, L, Gh, Gw]; adds coef times the derivative of
 *   sum over d in {L, Gh, Gw} of S_d / c_d  into grads (same shape, a distinct buffer), S_d = the sum of the squared
 *   differences of neighbours along d over all N grids, c_d = the number of such pairs in ONE grid (12 channels included):
 *   element x gets  2 coef / c_d ((x - x_prev) + (x - x_next))  per direction, one-sided at the ends.  N 12 L Gh Gw < 2^31.
 */
#ifndef SPLATCO_BILAGRID_H
#define SPLATCO_BILAGRID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCR_BILAGRID_ABI_VERSION 1

int scr_bilagrid_abi_version(void);
size_t scr_bilagrid_scratch_bytes(int32_t L, int32_t Gh, int32_t Gw, int32_t H, int32_t W);
int scr_bilagrid_slice(const float* grid, int32_t L, int32_t Gh, int32_t Gw, const float* rgb, int32_t H, int32_t W, float* out,
                       void* stream);
int scr_bilagrid_slice_backward(const float* grid, int32_t L, int32_t Gh, int32_t Gw, const float* rgb, const float* dL_dout,
                                int32_t H, int32_t W, float* dL_drgb, float* dL_dgrid, void* scratch, size_t scratch_bytes,
                                void* stream);
int scr_bilagrid_tv_add_grad(const float* grids, float* grads, int64_t N, int32_t L, int32_t Gh, int32_t Gw, float coef,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPLATCO_BILAGRID_H */
