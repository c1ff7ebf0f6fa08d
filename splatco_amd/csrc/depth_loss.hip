// splatco_amd/csrc/depth_loss.hip -- aligned inverse-depth loss on the rasterizer's depth / opacity maps (gfx950).
//
// Depth supervision as upstream 3DGS's depth_l1_weight (invdepthmap, depth_mask), on the maps of the image pass
// (D = sum w z, A = sum w).  Per pixel e of the H W pixels, all maps float32:
//   valid(e)   m > 0, g, D, A finite, A >= min_alpha, D > 0            (everything else is a hole: no term, zero gradient)
//   p          A / D ("inverse", mode 0) or D / A ("expected", mode 1): ONE binary32 division
//   (s, t)     argmin sum_valid m (s p + t - g)^2 from the binary64 moments S0 = sum m, Sp = sum m p, Spp = sum m p^2,
//              Sg = sum m g, Spg = sum m p g;  (1, 0) without alignment, with fewer than two valid pixels, or when
//              S0 Spp - Sp^2 <= 1e-12 S0 Spp;  constants of the backward pass
//   L          (1 / (H W)) sum_valid m |s p + t - g|, residual and sum in binary64, rounded once
//   q          g_up m s sign(s p + t - g) / (H W), sign(0) = 0;  inverse: dA = q / D, dD = -q A / D^2;  expected: dD = q / A,
//              dA = -q D / A^2
// In framework ops that is about twenty element-wise kernels and five reductions per view, with a float32 sum() whose order
// is not fixed.  Here: a moment pass (only with alignment) and a residual pass, each one streaming read of the maps with one
// record per workgroup, each followed by a one-workgroup fold, and one element-wise backward pass.  Every sum has the fixed
// order of wg.h (wg_sum per workgroup, fold_sum over the records), so a result is the same bits run after run.  No atomics,
// no memset: every scratch word that is read was written by an earlier launch of the same call.
#include "capi.h"
#include "wg.h"

namespace scr {

constexpr int DL_THREADS = 256;
constexpr int DL_ROUNDS = 16;                          // pixels per lane
constexpr int DL_PER_WG = DL_THREADS * DL_ROUNDS;      // 4096 contiguous pixels per workgroup
constexpr int DL_FOLD = 1024;                          // threads of the fold workgroup
constexpr int DL_MOM = 6;                              // doubles per moment record: S0, Sp, Spp, Sg, Spg, n_valid
constexpr int DL_RES = 2;                              // doubles per residual record: sum m |r|, n_valid

// scratch: [0, 256) header (double s, t) | moment records [nb][6] | residual records [nb][2]
struct DlScratch {
    double* st;
    double* mom;
    double* res;
    size_t bytes;
};
static inline __host__ int64_t dl_blocks(int64_t n) { return (n + DL_PER_WG - 1) / DL_PER_WG; }
static inline __host__ DlScratch dl_layout(void* scratch, int64_t n) {
    const size_t nb = (size_t)dl_blocks(n);
    char* p = (char*)scratch;
    DlScratch s;
    s.st = (double*)p;
    s.mom = (double*)(p + 256);
    s.res = (double*)(p + 256 + align_up(nb * DL_MOM * sizeof(double)));
    s.bytes = 256 + align_up(nb * DL_MOM * sizeof(double)) + align_up(nb * DL_RES * sizeof(double));
    return s;
}

// The pixel's weight and prediction; false for a hole (nothing of a hole is used afterwards, so a NaN in it goes nowhere).
__device__ __forceinline__ bool dl_pixel(int64_t e, const float* __restrict__ depth, const float* __restrict__ alpha,
                                         const float* __restrict__ target, const void* __restrict__ mask, int mask_kind,
                                         int mode, float min_alpha, float& m, float& p, float& g, float& D, float& A) {
    m = mask_kind == 0 ? 1.0f : mask_kind == 1 ? ((const float*)mask)[e] : (((const uint8_t*)mask)[e] ? 1.0f : 0.0f);
    g = target[e];
    D = depth[e];
    A = alpha[e];
    const bool ok = m > 0.0f && __builtin_isfinite(g) && __builtin_isfinite(D) && __builtin_isfinite(A) && A >= min_alpha && D > 0.0f;
    p = ok ? (mode == 0 ? A / D : D / A) : 0.0f;
    return ok;
}

// pass A: mom[block] = the moments of the block's DL_PER_WG pixels
__global__ void __launch_bounds__(DL_THREADS)
depth_loss_moments_kernel(int64_t n, const float* __restrict__ depth, const float* __restrict__ alpha,
                          const float* __restrict__ target, const void* __restrict__ mask, int mask_kind, int mode,
                          float min_alpha, double* __restrict__ mom) {
    __shared__ double red[4 * DL_MOM];
    double v[DL_MOM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t e0 = (int64_t)blockIdx.x * DL_PER_WG;
    const int64_t e1 = min(n, e0 + DL_PER_WG);
    for (int64_t e = e0 + threadIdx.x; e < e1; e += DL_THREADS) {
        float m, p, g, D, A;
        if (dl_pixel(e, depth, alpha, target, mask, mask_kind, mode, min_alpha, m, p, g, D, A)) {
            const double md = (double)m, pd = (double)p, gd = (double)g;
            v[0] += md;
            v[1] += md * pd;
            v[2] += md * (pd * pd);
            v[3] += md * gd;
            v[4] += md * (pd * gd);
            v[5] += 1.0;
        }
    }
    wg_sum<DL_THREADS / WAVE>(v, red, mom + (size_t)blockIdx.x * DL_MOM);
}

// fold of pass A: st = (s, t) of the weighted least-squares line, (1, 0) where the fit is degenerate
__global__ void __launch_bounds__(DL_FOLD)
depth_loss_solve_kernel(int nb, const double* __restrict__ mom, double* __restrict__ st) {
    __shared__ double red[(DL_FOLD / WAVE) * DL_MOM];
    double a[DL_MOM];
    fold_sum<DL_FOLD>(nb, mom, red, a);
    if (threadIdx.x == 0) {
        const double S0 = a[0], Sp = a[1], Spp = a[2], Sg = a[3], Spg = a[4];
        const double det = S0 * Spp - Sp * Sp;
        double s = 1.0, t = 0.0;
        if (a[5] >= 2.0 && det > 1e-12 * (S0 * Spp)) {
            s = (S0 * Spg - Sp * Sg) / det;
            t = (Sg - s * Sp) / S0;
        }
        st[0] = s;
        st[1] = t;
    }
}

// pass B: res[block] = (sum m |s p + t - g|, n_valid) of the block's pixels
__global__ void __launch_bounds__(DL_THREADS)
depth_loss_residual_kernel(int64_t n, const float* __restrict__ depth, const float* __restrict__ alpha,
                           const float* __restrict__ target, const void* __restrict__ mask, int mask_kind, int mode,
                           float min_alpha, const double* __restrict__ st /*NULL: s, t = 1, 0*/, double* __restrict__ res) {
    __shared__ double red[4 * DL_RES];
    const double s = st ? st[0] : 1.0, t = st ? st[1] : 0.0;
    double v[DL_RES] = {0.0, 0.0};
    const int64_t e0 = (int64_t)blockIdx.x * DL_PER_WG;
    const int64_t e1 = min(n, e0 + DL_PER_WG);
    for (int64_t e = e0 + threadIdx.x; e < e1; e += DL_THREADS) {
        float m, p, g, D, A;
        if (dl_pixel(e, depth, alpha, target, mask, mask_kind, mode, min_alpha, m, p, g, D, A)) {
            v[0] += (double)m * fabs((s * (double)p + t) - (double)g);
            v[1] += 1.0;
        }
    }
    wg_sum<DL_THREADS / WAVE>(v, red, res + (size_t)blockIdx.x * DL_RES);
}

// fold of pass B: out4 = (L, s, t, n_valid); without alignment it also leaves (1, 0) in the header for the backward pass
__global__ void __launch_bounds__(DL_FOLD)
depth_loss_finish_kernel(int nb, const double* __restrict__ res, double inv_n, int align, double* __restrict__ st,
                         float* __restrict__ out4) {
    __shared__ double red[(DL_FOLD / WAVE) * DL_RES];
    double a[DL_RES];
    fold_sum<DL_FOLD>(nb, res, red, a);
    if (threadIdx.x == 0) {
        double s = 1.0, t = 0.0;
        if (align) { s = st[0]; t = st[1]; }
        else { st[0] = s; st[1] = t; }
        out4[0] = (float)(a[0] * inv_n);
        out4[1] = (float)s;
        out4[2] = (float)t;
        out4[3] = (float)a[1];
    }
}

// backward: every pixel of both maps is written (0.0 at holes); either map may be NULL
__global__ void __launch_bounds__(DL_THREADS)
depth_loss_backward_kernel(int64_t n, const float* __restrict__ depth, const float* __restrict__ alpha,
                           const float* __restrict__ target, const void* __restrict__ mask, int mask_kind, int mode,
                           float min_alpha, const double* __restrict__ st, const float* __restrict__ g_up, double inv_n,
                           float* __restrict__ d_depth, float* __restrict__ d_alpha) {
    const double s = st[0], t = st[1];
    const double w = ((double)g_up[0] * s) * inv_n;
    const int64_t e0 = (int64_t)blockIdx.x * DL_PER_WG;
    const int64_t e1 = min(n, e0 + DL_PER_WG);
    for (int64_t e = e0 + threadIdx.x; e < e1; e += DL_THREADS) {
        float m, p, g, D, A;
        float dD = 0.0f, dA = 0.0f;
        if (dl_pixel(e, depth, alpha, target, mask, mask_kind, mode, min_alpha, m, p, g, D, A)) {
            const double r = (s * (double)p + t) - (double)g;
            if (r != 0.0) {
                const double q = r > 0.0 ? w * (double)m : -(w * (double)m);
                const double num = mode == 0 ? (double)A : (double)D, den = mode == 0 ? (double)D : (double)A;
                const float d_den = (float)(-(q * num) / (den * den)), d_num = (float)(q / den);   // p = num / den
                dD = mode == 0 ? d_den : d_num;
                dA = mode == 0 ? d_num : d_den;
            }
        }
        if (d_depth) d_depth[e] = dD;
        if (d_alpha) d_alpha[e] = dA;
    }
}

static int depth_loss_args(int32_t H, int32_t W, const void* mask, int32_t mask_kind, int32_t mode, float min_alpha) {
    if (H < 1 || W < 1) return fail("depth_loss: bad image size H = %d, W = %d", H, W);
    if ((int64_t)H * W > 2147483647LL) return fail("depth_loss: H W = %lld exceeds 2^31 - 1", (long long)H * W);
    if (mask_kind < 0 || mask_kind > 2) return fail("depth_loss: mask_kind %d (0 none, 1 float32, 2 uint8)", mask_kind);
    if (mask_kind != 0 && !mask) return fail("depth_loss: mask is NULL with mask_kind %d", mask_kind);
    if (mode != 0 && mode != 1) return fail("depth_loss: mode %d (0 inverse, 1 expected)", mode);
    if (!(min_alpha >= 0.0f) || !(min_alpha <= 3.402823466e38f)) return fail("depth_loss: min_alpha %g must be finite and >= 0", (double)min_alpha);
    return 0;
}

}  // namespace scr

using namespace scr;

extern "C" {

size_t scr_depth_loss_scratch_bytes(int32_t H, int32_t W) { return dl_layout(nullptr, (int64_t)(H > 0 ? H : 1) * (W > 0 ? W : 1)).bytes; }

int scr_depth_loss_forward(int32_t H, int32_t W, const float* depth, const float* alpha, const float* target, const void* mask,
                           int32_t mask_kind, int32_t mode, int32_t align, float min_alpha, void* scratch, float* out4,
                           void* stream) {
    SCR_MARK_FN;
    if (depth_loss_args(H, W, mask, mask_kind, mode, min_alpha)) return 1;
    if (!depth || !alpha || !target || !scratch || !out4) return fail("depth_loss: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W;
    const int nb = (int)dl_blocks(n);
    const DlScratch sc = dl_layout(scratch, n);
    { ProfScope ps_(SCR_PROF_L1_SSIM, st);
      if (align) {
          depth_loss_moments_kernel<<<nb, DL_THREADS, 0, st>>>(n, depth, alpha, target, mask, mask_kind, mode, min_alpha, sc.mom);
          depth_loss_solve_kernel<<<1, DL_FOLD, 0, st>>>(nb, sc.mom, sc.st);
      }
      depth_loss_residual_kernel<<<nb, DL_THREADS, 0, st>>>(n, depth, alpha, target, mask, mask_kind, mode, min_alpha,
                                                           align ? sc.st : nullptr, sc.res);
      depth_loss_finish_kernel<<<1, DL_FOLD, 0, st>>>(nb, sc.res, 1.0 / (double)n, align != 0, sc.st, out4); }
    CHECK_LAUNCH("depth_loss_residual_kernel", 0, st);
    return 0;
}

int scr_depth_loss_backward(int32_t H, int32_t W, const float* depth, const float* alpha, const float* target, const void* mask,
                            int32_t mask_kind, int32_t mode, float min_alpha, const void* scratch, const float* g, float* d_depth,
                            float* d_alpha, void* stream) {
    SCR_MARK_FN;
    if (depth_loss_args(H, W, mask, mask_kind, mode, min_alpha)) return 1;
    if (!depth || !alpha || !target || !scratch || !g) return fail("depth_loss: NULL argument");
    if (!d_depth && !d_alpha) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W;
    { ProfScope ps_(SCR_PROF_L1_SSIM_BACKWARD, st);
      depth_loss_backward_kernel<<<(int)dl_blocks(n), DL_THREADS, 0, st>>>(n, depth, alpha, target, mask, mask_kind, mode, min_alpha,
                                                                           (const double*)scratch, g, 1.0 / (double)n, d_depth, d_alpha); }
    CHECK_LAUNCH("depth_loss_backward_kernel", 0, st);
    return 0;
}

}  // extern "C"
