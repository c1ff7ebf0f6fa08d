// splatco_amd/csrc/bilagrid.hip -- per-view bilateral grids: fused slice, its two gradients and the grids' total-variation
// term (gfx950).
//
// A bilateral grid is a small learnable lattice G[12, L, Gh, Gw] of 3x4 affine colour transforms (channel 4 i + j = A[i][j]),
// indexed by pixel position and luminance, applied to the RENDERED image before the loss ("Bilateral Guided Radiance Field
// Processing"; gsplat's use_bilateral_grid).  The definition (include/splatco_bilagrid.h restates it), float32 except the
// pixel coordinates u and v, no contraction (-ffp-contract=off) except the fmaf written out in the grid backward:
//   u = (px + 0.5) ((Gw - 1) / W) in binary64, v alike;  lum = (0.299 r + 0.587 g) + 0.114 b;  z = min(max(lum, 0), 1) (L - 1)
//   cell c0 = min((int)u, G - 2), fraction f = u - c0 (u, v: rounded to float32 here), for each of the three axes
//   (grid_sample with align_corners = True and border padding)
//   B_l = (((1-fy)(1-fx) G[l, y0, x0] + (1-fy) fx G[l, y0, x0+1]) + fy (1-fx) G[l, y0+1, x0]) + fy fx G[l, y0+1, x0+1]
//   A = (1 - fz) B_l0 + fz B_(l0+1);   out_i = ((A_i0 r + A_i1 g) + A_i2 b) + A_i3
//   dL/drgb_j = sum_i A_ij g_i + [0 < lum < 1] (sum_i g_i ((B_(l0+1) - B_l0)_i . [r, g, b, 1])) (L - 1) k_j
//   dL/dG[4i+j, l, gy, gx] = sum over pixels of  wz_l (wy wx g_i [r, g, b, 1]_j),  wz_l = max(0, 1 - |z - l|)
// In framework ops that is a 5-D grid_sample forward and backward per view on a full-resolution image, and the backward
// scatters with float atomics.  Here:
//   slice / backward to rgb   one kernel, one pass over the pixels.  A workgroup owns a tile of BG_TW x BG_TH pixels; the few
//                             (Gh, Gw) vertices the tile touches (2 x 2 or 3 x 2 at 1080p) are staged in LDS as [12 L][ny][nx]
//                             columns, and every pixel reads its 96 values from there.  Where the tile covers more vertices than
//                             BG_LDS_FLOATS hold (an image smaller than the grid) the pixels read the grid itself.  A wave is 64
//                             consecutive pixels of a row: the planar images are read and written coalesced.
//   backward to the grid      gather form, no atomics.  Vertex (gy, gx) receives from the pixel rectangle |u - gx| < 1,
//                             |v - gy| < 1.  `parts` workgroups per vertex (a function of the shapes alone) split the rectangle's
//                             rows; each walks its pixels in index order, a lane holding BG_LC x 12 sums (levels unrolled, no
//                             dynamic indexing; L > BG_LC takes a second pass over the rectangle), and writes one record per
//                             level (wg_sum).  A fold workgroup per (vertex, level) adds the records (fold_sum).  Every sum has
//                             the order of wg.h, every record and every element of dL/dG is written: no memset.
//   total variation           one gather pass over the N 12 L Gh Gw elements.
#include "capi.h"
#include "wg.h"
#include "../../include/splatco_bilagrid.h"

namespace scr {

constexpr int BG_THREADS = 256;
constexpr int BG_TW = 64, BG_TH = 16;       // pixel tile of a slice workgroup: a wave takes rows w, w + 4, w + 8, w + 12
constexpr int BG_LDS_FLOATS = 12288;        // staged vertex columns (48 KB: three workgroups per CU)
constexpr int BG_LC = 8;                    // levels a grid-backward lane accumulates per pass (96 sums)
constexpr int BG_PART_ROWS = 32;            // rectangle rows per grid-backward workgroup, until ...
constexpr int BG_MAX_PARTS = 64;            // ... a vertex would need more workgroups than this (= BG_FOLD: one record per lane)
constexpr int BG_FOLD = 64;                 // threads of the fold workgroup
constexpr int BG_CH = 12;

struct BgDims {
    int L, Gh, Gw, H, W;
    double sx, sy;                          // (Gw - 1) / W, (Gh - 1) / H
};
static inline __host__ BgDims bg_dims(int L, int Gh, int Gw, int H, int W) {
    return BgDims{L, Gh, Gw, H, W, (double)(Gw - 1) / (double)W, (double)(Gh - 1) / (double)H};
}

// pixel p of n along an axis of G vertices: its cell and the fraction inside it
// (u in binary64, rounded once when the fraction is taken: with 64 vertices a float32 u would carry an absolute error of
// 64 roundings into the fraction)
__device__ __forceinline__ void bg_axis(int p, double scale, int G, int& c0, float& f) {
    const double u = ((double)p + 0.5) * scale;
    c0 = min((int)u, G - 2);
    f = (float)(u - (double)c0);
}

// the guide: level cell, fraction, z itself, and whether the unclamped luminance lies strictly inside (0, 1)
__device__ __forceinline__ void bg_guide(float r, float g, float b, int L, int& l0, float& fz, float& z, bool& inside) {
    const float lum = (0.299f * r + 0.587f * g) + 0.114f * b;
    inside = lum > 0.0f && lum < 1.0f;
    z = fminf(fmaxf(lum, 0.0f), 1.0f) * (float)(L - 1);
    l0 = min((int)z, L - 2);
    fz = z - (float)l0;
}

// [lo, hi): a superset of the pixels p of n with |u(p) - g| < 1 (one pixel of slack on either side: the kernel decides every
// pixel's weight with bg_axis itself, the rectangle only has to contain them)
__host__ __device__ inline void bg_rect(int g, int n, int G, int& lo, int& hi) {
    const double a = (double)(g - 1) * (double)n / (double)(G - 1) - 0.5;
    const double b = (double)(g + 1) * (double)n / (double)(G - 1) - 0.5;
    const long long l = (long long)floor(a) - 1, h = (long long)ceil(b) + 2;
    lo = (int)(l < 0 ? 0 : (l > n ? n : l));
    hi = (int)(h > n ? n : (h < lo ? lo : h));
}

// rows per part and parts per vertex of the grid backward: BG_PART_ROWS rows each, at most BG_MAX_PARTS parts
struct BgSplit { int parts, part_rows; };
static inline __host__ BgSplit bg_split(int Gh, int H) {
    int tallest = 1;
    for (int gy = 0; gy < Gh; ++gy) {
        int lo, hi;
        bg_rect(gy, H, Gh, lo, hi);
        tallest = max(tallest, hi - lo);
    }
    BgSplit s;
    s.parts = min(BG_MAX_PARTS, (tallest + BG_PART_ROWS - 1) / BG_PART_ROWS);
    s.part_rows = (tallest + s.parts - 1) / s.parts;
    return s;
}
static inline __host__ size_t bg_scratch_bytes(int L, int Gh, int Gw, int H) {
    return align_up((size_t)Gh * Gw * L * bg_split(Gh, H).parts * BG_CH * sizeof(float));
}

// One pixel of the slice.  src holds the columns as [12 L][..][..] with row stride sy, level stride sl and channel stride
// L sl; `at` is the index of (channel 0, level l0, y0, x0).  MODE 0: dst = out.  MODE 1: dst = dL/drgb, gout = dL/dout.
template <int MODE>
__device__ __forceinline__ void bg_pixel(const float* __restrict__ src, int sy, int sl, int at, int L, float fy, float fx, float fz,
                                         bool inside, float r, float g, float b, const float* __restrict__ gout,
                                         float* __restrict__ dst, size_t e, size_t plane) {
    const int sc = L * sl;
    const float w00 = (1.0f - fy) * (1.0f - fx), w01 = (1.0f - fy) * fx, w10 = fy * (1.0f - fx), w11 = fy * fx;
    float B0[BG_CH], B1[BG_CH];
#pragma unroll
    for (int c = 0; c < BG_CH; ++c) {
        const float* q = src + at + c * sc;
        B0[c] = ((w00 * q[0] + w01 * q[1]) + w10 * q[sy]) + w11 * q[sy + 1];
        B1[c] = ((w00 * q[sl] + w01 * q[sl + 1]) + w10 * q[sl + sy]) + w11 * q[sl + sy + 1];
    }
    float A[BG_CH];
#pragma unroll
    for (int c = 0; c < BG_CH; ++c) A[c] = (1.0f - fz) * B0[c] + fz * B1[c];
    if (MODE == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) dst[e + i * plane] = ((A[4 * i] * r + A[4 * i + 1] * g) + A[4 * i + 2] * b) + A[4 * i + 3];
    } else {
        const float g0 = gout[e], g1 = gout[e + plane], g2 = gout[e + 2 * plane];
        float through = 0.0f;
        if (inside) {
            const float gi[3] = {g0, g1, g2};
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float d0 = B1[4 * i] - B0[4 * i], d1 = B1[4 * i + 1] - B0[4 * i + 1], d2 = B1[4 * i + 2] - B0[4 * i + 2],
                            d3 = B1[4 * i + 3] - B0[4 * i + 3];
                s += gi[i] * (((d0 * r + d1 * g) + d2 * b) + d3);
            }
            through = s * (float)(L - 1);
        }
        dst[e] = ((A[0] * g0 + A[4] * g1) + A[8] * g2) + through * 0.299f;
        dst[e + plane] = ((A[1] * g0 + A[5] * g1) + A[9] * g2) + through * 0.587f;
        dst[e + 2 * plane] = ((A[2] * g0 + A[6] * g1) + A[10] * g2) + through * 0.114f;
    }
}

template <int MODE>
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_slice_kernel(const BgDims d, const float* __restrict__ grid, const float* __restrict__ rgb,
                      const float* __restrict__ gout, float* __restrict__ dst) {
    __shared__ float cols[BG_LDS_FLOATS];
    const int tiles_x = (d.W + BG_TW - 1) / BG_TW;
    const int px_a = (int)(blockIdx.x % (unsigned)tiles_x) * BG_TW, py_a = (int)(blockIdx.x / (unsigned)tiles_x) * BG_TH;
    const int px_b = min(d.W, px_a + BG_TW) - 1, py_b = min(d.H, py_a + BG_TH) - 1;
    // the tile's cells along each axis (u rises with the pixel, so every pixel's cell lies between the ends')
    int xa, xb, ya, yb;
    float unused;
    bg_axis(px_a, d.sx, d.Gw, xa, unused);
    bg_axis(px_b, d.sx, d.Gw, xb, unused);
    bg_axis(py_a, d.sy, d.Gh, ya, unused);
    bg_axis(py_b, d.sy, d.Gh, yb, unused);
    const int nvx = xb - xa + 2, nvy = yb - ya + 2;
    const int n_staged = BG_CH * d.L * nvy * nvx;
    const bool staged = n_staged <= BG_LDS_FLOATS;          // the same in every thread of the workgroup
    if (staged) {
        for (int t = threadIdx.x; t < n_staged; t += BG_THREADS) {
            const int x = t % nvx, y = (t / nvx) % nvy, cl = t / (nvx * nvy);
            cols[t] = grid[((size_t)cl * d.Gh + (ya + y)) * d.Gw + (xa + x)];
        }
        __syncthreads();
    }
    const int px = px_a + (threadIdx.x & (BG_TW - 1));
    if (px > px_b) return;
    const size_t plane = (size_t)d.H * d.W;
    int x0;
    float fx;
    bg_axis(px, d.sx, d.Gw, x0, fx);
    for (int py = py_a + (threadIdx.x / BG_TW); py <= py_b; py += BG_THREADS / BG_TW) {
        int y0, l0;
        float fy, fz, z;
        bool inside;
        bg_axis(py, d.sy, d.Gh, y0, fy);
        const size_t e = (size_t)py * d.W + px;
        const float r = rgb[e], g = rgb[e + plane], b = rgb[e + 2 * plane];
        bg_guide(r, g, b, d.L, l0, fz, z, inside);
        if (staged)
            bg_pixel<MODE>(cols, nvx, nvy * nvx, (l0 * nvy + (y0 - ya)) * nvx + (x0 - xa), d.L, fy, fx, fz, inside, r, g, b, gout, dst,
                           e, plane);
        else
            bg_pixel<MODE>(grid, d.Gw, d.Gh * d.Gw, (l0 * d.Gh + y0) * d.Gw + x0, d.L, fy, fx, fz, inside, r, g, b, gout, dst, e,
                           plane);
    }
}

// rec[vertex][level][part][12]: part `part` of vertex v's rectangle, levels chunk BG_LC .. chunk BG_LC + BG_LC - 1
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_grid_backward_kernel(const BgDims d, int parts, int part_rows, int chunks, const float* __restrict__ rgb,
                              const float* __restrict__ gout, float* __restrict__ rec) {
    __shared__ float red[BG_LC * (BG_THREADS / WAVE) * BG_CH];
    unsigned blk = blockIdx.x;
    const int part = (int)(blk % (unsigned)parts);
    blk /= (unsigned)parts;
    const int chunk = (int)(blk % (unsigned)chunks), v = (int)(blk / (unsigned)chunks);
    const int gy = v / d.Gw, gx = v % d.Gw;
    int x_lo, x_hi, y_lo, y_hi;
    bg_rect(gx, d.W, d.Gw, x_lo, x_hi);
    bg_rect(gy, d.H, d.Gh, y_lo, y_hi);
    const int y_a = (int)min((long long)y_hi, (long long)y_lo + (long long)part * part_rows);
    const int y_b = (int)min((long long)y_hi, (long long)y_a + part_rows);
    const unsigned rw = (unsigned)(x_hi - x_lo), n = rw * (unsigned)(y_b - y_a);      // n <= H W < 2^31
    const size_t plane = (size_t)d.H * d.W;
    const int lbase = chunk * BG_LC;
    float acc[BG_LC][BG_CH];
#pragma unroll
    for (int l = 0; l < BG_LC; ++l)
#pragma unroll
        for (int c = 0; c < BG_CH; ++c) acc[l][c] = 0.0f;
    for (unsigned i = threadIdx.x; i < n; i += BG_THREADS) {
        const int py = y_a + (int)(i / rw), px = x_lo + (int)(i % rw);
        int x0, y0, l0;
        float fx, fy, fz, z;
        bool inside;
        bg_axis(px, d.sx, d.Gw, x0, fx);
        bg_axis(py, d.sy, d.Gh, y0, fy);
        const float wx = x0 == gx ? 1.0f - fx : (x0 + 1 == gx ? fx : 0.0f);
        const float wy = y0 == gy ? 1.0f - fy : (y0 + 1 == gy ? fy : 0.0f);
        const float w = wy * wx;
        const size_t e = (size_t)py * d.W + px;
        const float r = rgb[e], g = rgb[e + plane], b = rgb[e + 2 * plane];
        const float gi[3] = {w * gout[e], w * gout[e + plane], w * gout[e + 2 * plane]};
        bg_guide(r, g, b, d.L, l0, fz, z, inside);
        float t[BG_CH];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            t[4 * k] = gi[k] * r;
            t[4 * k + 1] = gi[k] * g;
            t[4 * k + 2] = gi[k] * b;
            t[4 * k + 3] = gi[k];
        }
#pragma unroll
        for (int l = 0; l < BG_LC; ++l) {
            const float wz = fmaxf(0.0f, 1.0f - fabsf(z - (float)(lbase + l)));
#pragma unroll
            for (int c = 0; c < BG_CH; ++c) acc[l][c] = __builtin_fmaf(wz, t[c], acc[l][c]);
        }
    }
#pragma unroll
    for (int l = 0; l < BG_LC; ++l) {
        if (lbase + l < d.L)                                   // the same in every thread: the barrier inside is safe
            wg_sum<BG_THREADS / WAVE>(acc[l], red + l * (BG_THREADS / WAVE) * BG_CH,
                                      rec + (((size_t)v * d.L + (lbase + l)) * parts + part) * BG_CH);
    }
}

// one workgroup per (vertex, level): dL/dG[:, level, vertex] = the records of the vertex's parts, added in ascending order
__global__ void __launch_bounds__(BG_FOLD)
bilagrid_grid_fold_kernel(int L, int vertices, int parts, const float* __restrict__ rec, float* __restrict__ dgrid) {
    __shared__ float red[(BG_FOLD / WAVE) * BG_CH];
    float a[BG_CH];
    const int v = (int)(blockIdx.x / (unsigned)L), l = (int)(blockIdx.x % (unsigned)L);
    fold_sum<BG_FOLD>(parts, rec + (size_t)blockIdx.x * parts * BG_CH, red, a);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < BG_CH; ++c) dgrid[((size_t)c * L + l) * vertices + v] = a[c];
    }
}

// element e of [N 12][L][Gh][Gw]: grad += kL ((x - x_l-1) + (x - x_l+1)) + kH (...) + kW (...), one-sided at the ends
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_tv_kernel(unsigned n, int L, int Gh, int Gw, float kL, float kH, float kW, const float* __restrict__ p,
                   float* __restrict__ grad) {
    const unsigned e = blockIdx.x * (unsigned)BG_THREADS + threadIdx.x;
    if (e >= n) return;
    const int x = (int)(e % (unsigned)Gw), y = (int)((e / (unsigned)Gw) % (unsigned)Gh), l = (int)((e / (unsigned)(Gw * Gh)) % (unsigned)L);
    const int sy = Gw, sl = Gw * Gh;
    const float c = p[e];
    const float dl = (l > 0 ? c - p[e - sl] : 0.0f) + (l + 1 < L ? c - p[e + sl] : 0.0f);
    const float dy = (y > 0 ? c - p[e - sy] : 0.0f) + (y + 1 < Gh ? c - p[e + sy] : 0.0f);
    const float dx = (x > 0 ? c - p[e - 1] : 0.0f) + (x + 1 < Gw ? c - p[e + 1] : 0.0f);
    grad[e] = grad[e] + ((kL * dl + kH * dy) + kW * dx);
}

// sizes first; returns 1 after fail()
static int bg_sizes(const char* fn, int32_t L, int32_t Gh, int32_t Gw) {
    if (L < 2 || L > 16) return fail("%s: L = %d is outside 2 .. 16", fn, L);
    if (Gh < 2 || Gh > 64 || Gw < 2 || Gw > 64) return fail("%s: Gh = %d, Gw = %d are outside 2 .. 64", fn, Gh, Gw);
    return 0;
}
static int bg_image(const char* fn, int32_t H, int32_t W) {
    if (H < 0 || W < 0) return fail("%s: bad image size H = %d, W = %d", fn, H, W);
    if ((int64_t)H * W >= (1ll << 31)) return fail("%s: H W = %lld is not below 2^31", fn, (long long)H * W);
    return 0;
}

}  // namespace scr

using namespace scr;

extern "C" {

int scr_bilagrid_abi_version(void) { return SCR_BILAGRID_ABI_VERSION; }

size_t scr_bilagrid_scratch_bytes(int32_t L, int32_t Gh, int32_t Gw, int32_t H, int32_t W) {
    if (L < 2 || L > 16 || Gh < 2 || Gh > 64 || Gw < 2 || Gw > 64 || H < 1 || W < 1) return 256;
    return bg_scratch_bytes(L, Gh, Gw, H);
}

int scr_bilagrid_slice(const float* grid, int32_t L, int32_t Gh, int32_t Gw, const float* rgb, int32_t H, int32_t W, float* out,
                       void* stream) {
    SCR_MARK_FN;
    if (bg_sizes(__func__, L, Gh, Gw) || bg_image(__func__, H, W)) return 1;
    if ((int64_t)H * W == 0) return 0;
    if (!grid || !rgb || !out) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    const BgDims d = bg_dims(L, Gh, Gw, H, W);
    const unsigned tiles = (unsigned)((W + BG_TW - 1) / BG_TW) * (unsigned)((H + BG_TH - 1) / BG_TH);
    bilagrid_slice_kernel<0><<<tiles, BG_THREADS, 0, st>>>(d, grid, rgb, nullptr, out);
    CHECK_LAUNCH("bilagrid_slice_kernel", 0, st);
    return 0;
}

int scr_bilagrid_slice_backward(const float* grid, int32_t L, int32_t Gh, int32_t Gw, const float* rgb, const float* dL_dout,
                                int32_t H, int32_t W, float* dL_drgb, float* dL_dgrid, void* scratch, size_t scratch_bytes,
                                void* stream) {
    SCR_MARK_FN;
    if (bg_sizes(__func__, L, Gh, Gw) || bg_image(__func__, H, W)) return 1;
    if ((int64_t)H * W == 0) return 0;
    if (!grid || !rgb || !dL_dout) return fail("%s: NULL argument", __func__);
    if (dL_dgrid && (!scratch || scratch_bytes < bg_scratch_bytes(L, Gh, Gw, H)))
        return fail("%s: dL_dgrid needs %zu bytes of scratch, got %zu", __func__, bg_scratch_bytes(L, Gh, Gw, H), scratch ? scratch_bytes : (size_t)0);
    hipStream_t st = (hipStream_t)stream;
    const BgDims d = bg_dims(L, Gh, Gw, H, W);
    if (dL_drgb) {
        const unsigned tiles = (unsigned)((W + BG_TW - 1) / BG_TW) * (unsigned)((H + BG_TH - 1) / BG_TH);
        bilagrid_slice_kernel<1><<<tiles, BG_THREADS, 0, st>>>(d, grid, rgb, dL_dout, dL_drgb);
        CHECK_LAUNCH("bilagrid_slice_kernel", 0, st);
    }
    if (dL_dgrid) {
        const BgSplit s = bg_split(Gh, H);
        const int chunks = (L + BG_LC - 1) / BG_LC;
        bilagrid_grid_backward_kernel<<<(unsigned)(Gh * Gw * chunks * s.parts), BG_THREADS, 0, st>>>(d, s.parts, s.part_rows, chunks, rgb,
                                                                                                   dL_dout, (float*)scratch);
        bilagrid_grid_fold_kernel<<<(unsigned)(Gh * Gw * L), BG_FOLD, 0, st>>>(L, Gh * Gw, s.parts, (const float*)scratch, dL_dgrid);
        CHECK_LAUNCH("bilagrid_grid_backward_kernel", 0, st);
    }
    return 0;
}

int scr_bilagrid_tv_add_grad(const float* grids, float* grads, int64_t N, int32_t L, int32_t Gh, int32_t Gw, float coef,
                             void* stream) {
    SCR_MARK_FN;
    if (bg_sizes(__func__, L, Gh, Gw)) return 1;
    if (N < 0) return fail("%s: N = %lld", __func__, (long long)N);
    if (N == 0) return 0;
    const int64_t per = (int64_t)BG_CH * L * Gh * Gw;
    if (N > ((1ll << 31) - 1) / per) return fail("%s: N 12 L Gh Gw = %lld x %lld is not below 2^31", __func__, (long long)N, (long long)per);
    if (!grids || !grads) return fail("%s: NULL argument", __func__);
    if ((const float*)grads == grids) return fail("%s: grids and grads must be distinct buffers", __func__);
    const unsigned n = (unsigned)(N * per);
    const double two = 2.0 * (double)coef;
    const float kL = (float)(two / ((double)BG_CH * (L - 1) * Gh * Gw)), kH = (float)(two / ((double)BG_CH * L * (Gh - 1) * Gw)),
                kW = (float)(two / ((double)BG_CH * L * Gh * (Gw - 1)));
    hipStream_t st = (hipStream_t)stream;
    bilagrid_tv_kernel<<<(n + BG_THREADS - 1) / BG_THREADS, BG_THREADS, 0, st>>>(n, L, Gh, Gw, kL, kH, kW, grids, grads);
    CHECK_LAUNCH("bilagrid_tv_kernel", 0, st);
    return 0;
}

}  // extern "C"
