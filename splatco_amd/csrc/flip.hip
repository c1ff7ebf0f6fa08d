// splatco_amd/csrc/flip.hip -- LDR-FLIP image difference (Andersson et al., HPG 2020) of [N,3,H,W] sRGB pairs (gfx950).
//
// The evaluation scripts score every test view with FLIP (metrics.py:38-108, utils/flip.py LDRFLIPLoss at its defaults:
// qc 0.7, qf 0.5, pc 0.4, pt 0.95, eps 1e-15).  There that is seven 2-D conv2d (21x21 CSF, 19x19 feature taps at the
// default 67 pixels per degree) plus some forty elementwise launches and a host read per image.  Every filter of it is
// exactly separable, so one fused pass does the lot: each 16x16 output tile stages its halo of one image as
// (Y, Cx, Cz, (Y+16)/116) in LDS, runs seven horizontal 1-D passes (CSF: A, RG, BY1, BY2; features: edge, point and
// Gaussian profiles), then eight vertical ones in registers, keeps the Hunt-adjusted L*a*b* and the two feature norms
// of the reference image in registers, repeats for the test image, and evaluates the per-pixel error.  Tile sums of
// FLIP and of the squared RGB error go to per-tile partials, added in a fixed order per image by a second launch
// (deterministic; an image's bits do not depend on the batch it was scored in).
//
// Every filter reads its input with replicate padding (coordinates clamped to the image), which the separable form
// keeps exactly: the vertical pass reads the horizontal results of clamped rows.
#include <math.h>

#include "capi.h"
#include "wg.h"

namespace scr {

constexpr int FL_T = 16;                      // output tile edge
constexpr int FL_RMAX = SCR_FLIP_MAX_RADIUS;  // largest filter radius (CSF and features)
constexpr int FL_S = FL_T + 2 * FL_RMAX;      // staged region edge
constexpr int FL_NW = 2 * FL_RMAX + 1;        // taps of the widest 1-D filter

// the 1-D weights, tap k at offset k - r (binary32 roundings of the host's binary64 values, flip_filters below)
struct FlipFilters {
    int rc, rf;                                   // CSF radius, feature radius
    float a[FL_NW], rg[FL_NW], by1[FL_NW], by2[FL_NW];  // CSF profiles, each summing to 1
    float by_c1, by_c2;                           // BY = by_c1 by1 (x) by1 + by_c2 by2 (x) by2
    float edge[FL_NW], point[FL_NW], gauss[FL_NW];  // feature profiles: edge / point along the detector's axis, Gaussian across
    float cmax;                                   // HyAB^qc of (green, blue) after the Hunt adjustment
    int quantize;                                 // 8-bit round trip after the clamp
};

constexpr int FL_PLANES = 4;   // staged: Y, Cx, Cz, (Y + 16) / 116
constexpr int FL_HZ = 7;       // horizontal results: A, RG, BY1, BY2 (CSF); edge, point, Gaussian (features)
constexpr size_t FL_LDS = sizeof(float) * ((size_t)FL_PLANES * FL_S * FL_S + (size_t)FL_HZ * FL_S * FL_T);
static_assert(FL_LDS <= 64 * 1024, "flip_kernel's LDS must stay under 64 KiB");

// sRGB -> YCxCz constants (D65): linear RGB -> XYZ is sRGB's primaries matrix, then XYZ is divided by the white point
constexpr float FL_M00 = (float)(10135552.0 / 24577794.0), FL_M01 = (float)(8788810.0 / 24577794.0),
                FL_M02 = (float)(4435075.0 / 24577794.0);
constexpr float FL_M10 = (float)(2613072.0 / 12288897.0), FL_M11 = (float)(8788810.0 / 12288897.0),
                FL_M12 = (float)(887015.0 / 12288897.0);
constexpr float FL_M20 = (float)(1425312.0 / 73733382.0), FL_M21 = (float)(8788810.0 / 73733382.0),
                FL_M22 = (float)(70074185.0 / 73733382.0);
// the inverse matrix, as the reference rounds it
constexpr float FL_I00 = 3.241003275f, FL_I01 = -1.537398934f, FL_I02 = -0.498615861f;
constexpr float FL_I10 = -0.969224334f, FL_I11 = 1.875930071f, FL_I12 = 0.041554224f;
constexpr float FL_I20 = 0.055639423f, FL_I21 = -0.204011202f, FL_I22 = 1.057148933f;
constexpr float FL_WX = 0.950428545f, FL_WZ = 1.088900371f;        // D65 white (Y = 1)
constexpr float FL_IWX = 1.052156925f, FL_IWZ = 0.918357670f;      // its reciprocal, as the reference rounds it
constexpr float FL_QC = 0.7f, FL_PC = 0.4f, FL_PT = 0.95f, FL_EPS = 1e-15f;

// clamp to [0,1], optionally the 8-bit PNG round trip (save_image: floor(255 x + 0.5); to_tensor: / 255)
__device__ __forceinline__ float fl_prep(float v, int quantize) {
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    if (quantize) v = floorf(255.0f * v + 0.5f) / 255.0f;
    return v;
}
__device__ __forceinline__ float fl_srgb2lin(float v) {
    return v > 0.04045f ? powf((fmaxf(v, 0.04045f) + 0.055f) / 1.055f, 2.4f) : v / 12.92f;
}
__device__ __forceinline__ float fl_lab_f(float t) {
    const float d = 6.0f / 29.0f, d3 = d * d * d, k = 1.0f / (3.0f * d * d);
    return t > d3 ? cbrtf(fmaxf(t, d3)) : k * t + 4.0f / 29.0f;
}

// filtered YCxCz of one pixel -> Hunt-adjusted L*a*b* (the colour pipeline up to HyAB)
__device__ __forceinline__ void fl_filtered_to_lab(float yf, float cxf, float czf, float lab[3]) {
    const float y = (yf + 16.0f) / 116.0f, cx = cxf / 500.0f, cz = czf / 200.0f;
    const float X = (y + cx) * FL_WX, Y = y, Z = (y - cz) * FL_WZ;
    const float r = fminf(fmaxf(FL_I00 * X + FL_I01 * Y + FL_I02 * Z, 0.0f), 1.0f);
    const float g = fminf(fmaxf(FL_I10 * X + FL_I11 * Y + FL_I12 * Z, 0.0f), 1.0f);
    const float b = fminf(fmaxf(FL_I20 * X + FL_I21 * Y + FL_I22 * Z, 0.0f), 1.0f);
    const float fx = fl_lab_f((FL_M00 * r + FL_M01 * g + FL_M02 * b) * FL_IWX);
    const float fy = fl_lab_f(FL_M10 * r + FL_M11 * g + FL_M12 * b);
    const float fz = fl_lab_f((FL_M20 * r + FL_M21 * g + FL_M22 * b) * FL_IWZ);
    const float L = 116.0f * fy - 16.0f;
    lab[0] = L;
    lab[1] = (0.01f * L) * (500.0f * (fx - fy));
    lab[2] = (0.01f * L) * (200.0f * (fy - fz));
}

// One image of the pair through the tile: stage, filter, and leave this thread's pixel's Hunt-adjusted L*a*b* and its
// edge / point magnitudes.  Ends with a barrier, so the caller may restage.
__device__ __forceinline__ void fl_tile_image(const float* __restrict__ img, int H, int W, int ox, int oy, int R,
                                              const FlipFilters& F, float (*st)[FL_S][FL_S], float (*hz)[FL_S][FL_T],
                                              float lab[3], float& e_norm, float& p_norm) {
    const int S = FL_T + 2 * R;
    const size_t plane = (size_t)H * W;
    for (int i = threadIdx.x; i < S * S; i += 256) {
        const int ly = i / S, lx = i - ly * S;
        const int y = min(max(oy + ly - R, 0), H - 1), x = min(max(ox + lx - R, 0), W - 1);
        const size_t o = (size_t)y * W + x;
        const float r = fl_srgb2lin(fl_prep(img[o], F.quantize));
        const float g = fl_srgb2lin(fl_prep(img[plane + o], F.quantize));
        const float b = fl_srgb2lin(fl_prep(img[2 * plane + o], F.quantize));
        const float X = (FL_M00 * r + FL_M01 * g + FL_M02 * b) * FL_IWX;
        const float Y = FL_M10 * r + FL_M11 * g + FL_M12 * b;
        const float Z = (FL_M20 * r + FL_M21 * g + FL_M22 * b) * FL_IWZ;
        const float yy = 116.0f * Y - 16.0f;
        st[0][ly][lx] = yy;
        st[1][ly][lx] = 500.0f * (X - Y);
        st[2][ly][lx] = 200.0f * (Y - Z);
        st[3][ly][lx] = (yy + 16.0f) / 116.0f;
    }
    __syncthreads();
    const int dc = R - F.rc, df = R - F.rf;      // a filter of radius r starts at column / row R - r of the region
    for (int i = threadIdx.x; i < S * FL_T; i += 256) {
        const int ly = i / FL_T, lx = i - ly * FL_T;
        float a = 0, rg = 0, b1 = 0, b2 = 0, ed = 0, pt = 0, ga = 0;
        for (int k = 0; k <= 2 * F.rc; ++k) {
            const int c = lx + dc + k;
            a += F.a[k] * st[0][ly][c];
            rg += F.rg[k] * st[1][ly][c];
            const float z = st[2][ly][c];
            b1 += F.by1[k] * z;
            b2 += F.by2[k] * z;
        }
        for (int k = 0; k <= 2 * F.rf; ++k) {
            const float v = st[3][ly][lx + df + k];
            ed += F.edge[k] * v;
            pt += F.point[k] * v;
            ga += F.gauss[k] * v;
        }
        hz[0][ly][lx] = a; hz[1][ly][lx] = rg; hz[2][ly][lx] = b1; hz[3][ly][lx] = b2;
        hz[4][ly][lx] = ed; hz[5][ly][lx] = pt; hz[6][ly][lx] = ga;
    }
    __syncthreads();
    const int lx = threadIdx.x & (FL_T - 1), ly = threadIdx.x / FL_T;
    float a = 0, rg = 0, b1 = 0, b2 = 0;
    for (int k = 0; k <= 2 * F.rc; ++k) {
        const int r = ly + dc + k;   // the CSF kernels are isotropic: the vertical profile is the horizontal one
        a += F.a[k] * hz[0][r][lx];
        rg += F.rg[k] * hz[1][r][lx];
        b1 += F.by1[k] * hz[2][r][lx];
        b2 += F.by2[k] * hz[3][r][lx];
    }
    float ex = 0, px = 0, ey = 0, py = 0;
    for (int k = 0; k <= 2 * F.rf; ++k) {
        const int r = ly + df + k;
        const float g = F.gauss[k];
        ex += g * hz[4][r][lx];              // edge along x: edge profile across columns, Gaussian down rows
        px += g * hz[5][r][lx];
        const float v = hz[6][r][lx];        // along y: Gaussian across columns, edge / point profile down rows
        ey += F.edge[k] * v;
        py += F.point[k] * v;
    }
    fl_filtered_to_lab(a, rg, F.by_c1 * b1 + F.by_c2 * b2, lab);
    e_norm = sqrtf(ex * ex + ey * ey);
    p_norm = sqrtf(px * px + py * py);
    __syncthreads();
}

// grid (ceil(W/16), ceil(H/16), N), 256 threads.  partial[tile] = (sum FLIP, sum squared RGB error) of the tile.
__global__ void __launch_bounds__(256)
flip_kernel(int H, int W, const float* __restrict__ test, const float* __restrict__ ref, FlipFilters F,
            float* __restrict__ map, float2* __restrict__ partial) {
    __shared__ float st[FL_PLANES][FL_S][FL_S];
    __shared__ float hz[FL_HZ][FL_S][FL_T];
    __shared__ float wsum[4 * 2];
    const int n = blockIdx.z;
    const size_t plane = (size_t)H * W;
    const float* t_img = test + (size_t)n * 3 * plane;
    const float* r_img = ref + (size_t)n * 3 * plane;
    const int ox = blockIdx.x * FL_T, oy = blockIdx.y * FL_T;
    const int R = max(F.rc, F.rf);
    float lab_r[3], lab_t[3], e_r, p_r, e_t, p_t;
    fl_tile_image(r_img, H, W, ox, oy, R, F, st, hz, lab_r, e_r, p_r);
    fl_tile_image(t_img, H, W, ox, oy, R, F, st, hz, lab_t, e_t, p_t);

    const int px = ox + (threadIdx.x & (FL_T - 1)), py = oy + threadIdx.x / FL_T;
    float fsum = 0.0f, sse = 0.0f;
    if (px < W && py < H) {
        // colour: HyAB of the Hunt-adjusted L*a*b*, ^qc, redistributed onto [0,1] by cmax
        const float dL = lab_r[0] - lab_t[0], da = lab_r[1] - lab_t[1], db = lab_r[2] - lab_t[2];
        const float hyab = sqrtf(fmaxf(dL * dL, FL_EPS)) + sqrtf(da * da + db * db);
        const float pw = powf(hyab, FL_QC);
        const float pcc = FL_PC * F.cmax;
        const float dEc = pw < pcc ? (FL_PT / pcc) * pw : FL_PT + ((pw - pcc) / (F.cmax - pcc)) * (1.0f - FL_PT);
        // features: the larger change of edge or point magnitude, (dE / sqrt 2)^qf with qf = 1/2
        const float dEf0 = fmaxf(fmaxf(fabsf(e_r - e_t), fabsf(p_t - p_r)), FL_EPS);
        const float dEf = sqrtf(0.70710678118654752f * dEf0);
        const float f = powf(dEc, 1.0f - dEf);
        fsum = f;
        const size_t o = (size_t)py * W + px;
        if (map) map[(size_t)n * plane + o] = f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float d = fl_prep(t_img[c * plane + o], F.quantize) - fl_prep(r_img[c * plane + o], F.quantize);
            sse += d * d;
        }
    }
    float v[2] = {fsum, sse};   // tile sums in the order of wg.h; threads 0 and 1 write the partial's x and y
    wg_sum<4>(v, wsum, (float*)(partial + ((size_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x));
}

// grid N, 256 threads: image n's tile partials in a fixed order -> mean FLIP over H W, mean squared error over 3 H W
__global__ void __launch_bounds__(256)
flip_reduce_kernel(int tiles, const float2* __restrict__ partial, double inv_hw, float* __restrict__ mean_out,
                   float* __restrict__ mse_out) {
    __shared__ double sa[256], sb[256];
    const float2* p = partial + (size_t)blockIdx.x * tiles;
    double a = 0, b = 0;
    for (int i = threadIdx.x; i < tiles; i += 256) { a += p[i].x; b += p[i].y; }
    sa[threadIdx.x] = a; sb[threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { sa[threadIdx.x] += sa[threadIdx.x + s]; sb[threadIdx.x] += sb[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mean_out[blockIdx.x] = (float)(sa[0] * inv_hw);
        if (mse_out) mse_out[blockIdx.x] = (float)(sb[0] * (inv_hw / 3.0));
    }
}

// ---- host: the filters of utils/flip.py restated in binary64 (generate_spatial_filter, feature_detection)
constexpr double FL_PI = 3.14159265358979323846;

// radii for `ppd`: 0 on success, -1 when ppd is not a finite value >= 1 or a radius exceeds FL_RMAX
static int flip_radii(double ppd, int* rc, int* rf) {
    if (!(ppd >= 1.0) || !std::isfinite(ppd)) return -1;
    // CSF: 3 standard deviations of the widest Gaussian (b = 0.04 of the BY CSF); features: 3 sd of the detector
    const double c = ceil(3.0 * sqrt(0.04 / (2.0 * FL_PI * FL_PI)) * ppd);
    const double f = ceil(3.0 * (0.5 * 0.082 * ppd));
    if (c > FL_RMAX || f > FL_RMAX) return -1;
    *rc = (int)c;
    *rf = (int)f;
    return 0;
}

// binary64 1-D weights [7][FL_NW] (a, rg, by1, by2, edge, point, gauss; tap k at offset k - r, zero beyond 2r),
// scalars [3] = (by_c1, by_c2, cmax)
static int flip_filters(double ppd, double* w, int* radii, double* scalars) {
    int rc, rf;
    if (flip_radii(ppd, &rc, &rf)) return -1;
    for (int i = 0; i < 7 * FL_NW; ++i) w[i] = 0.0;
    double* a = w; double* rg = w + FL_NW; double* by1 = w + 2 * FL_NW; double* by2 = w + 3 * FL_NW;
    double* ed = w + 4 * FL_NW; double* pt = w + 5 * FL_NW; double* ga = w + 6 * FL_NW;
    // CSF: a1 sqrt(pi / b1) exp(-pi^2 d^2 / b1) + a2 sqrt(pi / b2) exp(-pi^2 d^2 / b2), d in degrees; the 2-D kernel
    // normalised to sum 1.  A (b1 0.0047) and RG (b1 0.0053) have a2 = 0: one Gaussian, the outer product of the
    // normalised 1-D profile with itself.  BY (a1 34.1, b1 0.04, a2 13.5, b2 0.025): two such terms.
    const double dx = 1.0 / ppd;
    auto gauss1d = [&](double b, double* out) {
        double s = 0.0;
        for (int k = 0; k <= 2 * rc; ++k) {
            const double d = (k - rc) * dx;
            out[k] = exp(-FL_PI * FL_PI * d * d / b);
            s += out[k];
        }
        for (int k = 0; k <= 2 * rc; ++k) out[k] /= s;
        return s;
    };
    gauss1d(0.0047, a);
    gauss1d(0.0053, rg);
    const double s1 = gauss1d(0.04, by1), s2 = gauss1d(0.025, by2);
    const double c1 = 34.1 * sqrt(FL_PI / 0.04) * s1 * s1, c2 = 13.5 * sqrt(FL_PI / 0.025) * s2 * s2;
    scalars[0] = c1 / (c1 + c2);
    scalars[1] = c2 / (c1 + c2);
    // features: the 2-D detector is f(x) g(y), g(y) = exp(-y^2 / 2 sd^2), f = -x g(x) (edge) or (x^2 / sd^2 - 1) g(x)
    // (point), its positive weights scaled to sum 1 and its negative ones to -1: the sign follows f alone, so that is
    // f scaled by its own positive / negative sums, times g / sum g.
    const double sd = 0.5 * 0.082 * ppd;
    double gs = 0.0;
    for (int k = 0; k <= 2 * rf; ++k) {
        const double x = k - rf, g = exp(-(x * x) / (2.0 * sd * sd));
        ga[k] = g;
        gs += g;
        ed[k] = -x * g;
        pt[k] = (x * x / (sd * sd) - 1.0) * g;
    }
    for (double* f : {ed, pt}) {
        double pos = 0.0, neg = 0.0;
        for (int k = 0; k <= 2 * rf; ++k) (f[k] > 0 ? pos : neg) += f[k];
        for (int k = 0; k <= 2 * rf; ++k) f[k] = f[k] > 0 ? f[k] / pos : (f[k] < 0 ? f[k] / -neg : 0.0);
    }
    for (int k = 0; k <= 2 * rf; ++k) ga[k] /= gs;
    // cmax = HyAB(green, blue)^qc in Hunt-adjusted L*a*b*, green = (0,1,0) and blue = (0,0,1) in linear RGB
    auto hunt_lab = [](double r, double g, double b, double* lab) {
        const double X = (10135552.0 / 24577794.0 * r + 8788810.0 / 24577794.0 * g + 4435075.0 / 24577794.0 * b) * 1.052156925;
        const double Y = 2613072.0 / 12288897.0 * r + 8788810.0 / 12288897.0 * g + 887015.0 / 12288897.0 * b;
        const double Z = (1425312.0 / 73733382.0 * r + 8788810.0 / 73733382.0 * g + 70074185.0 / 73733382.0 * b) * 0.918357670;
        const double d = 6.0 / 29.0, d3 = d * d * d;
        auto f = [&](double t) { return t > d3 ? cbrt(t) : t / (3.0 * d * d) + 4.0 / 29.0; };
        const double L = 116.0 * f(Y) - 16.0;
        lab[0] = L;
        lab[1] = 0.01 * L * 500.0 * (f(X) - f(Y));
        lab[2] = 0.01 * L * 200.0 * (f(Y) - f(Z));
    };
    double gl[3], bl[3];
    hunt_lab(0.0, 1.0, 0.0, gl);
    hunt_lab(0.0, 0.0, 1.0, bl);
    const double dL = gl[0] - bl[0], da = gl[1] - bl[1], db = gl[2] - bl[2];
    scalars[2] = pow(sqrt(std::max(dL * dL, 1e-15)) + sqrt(da * da + db * db), 0.7);
    radii[0] = rc;
    radii[1] = rf;
    return 0;
}

}  // namespace scr

using namespace scr;

extern "C" {

size_t scr_flip_scratch_bytes(int32_t N, int32_t H, int32_t W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    const size_t tiles = (size_t)((W + FL_T - 1) / FL_T) * ((H + FL_T - 1) / FL_T);
    return align_up(tiles * N * sizeof(float2));
}

int scr_flip_forward(int32_t N, int32_t H, int32_t W, const float* test, const float* ref, double pixels_per_degree,
                     int32_t quantize, void* scratch, float* mean_out, float* mse_out, float* map_out, void* stream) {
    SCR_MARK_FN;
    if (N <= 0 || H <= 0 || W <= 0) return fail("bad image size");
    if (N > 65535 || (H + 15) / 16 > 65535) return fail("N = %d / H = %d exceed the launch grid", N, H);
    if (!test || !ref || !scratch || !mean_out) return fail("NULL argument");
    double w[7 * FL_NW], sc[3];
    int radii[2];
    if (flip_filters(pixels_per_degree, w, radii, sc))
        return fail("pixels_per_degree %g: must be >= 1 with filter radii <= %d", pixels_per_degree, SCR_FLIP_MAX_RADIUS);
    hipStream_t st = (hipStream_t)stream;
    FlipFilters F;
    F.rc = radii[0];
    F.rf = radii[1];
    for (int k = 0; k < FL_NW; ++k) {
        F.a[k] = (float)w[k]; F.rg[k] = (float)w[FL_NW + k]; F.by1[k] = (float)w[2 * FL_NW + k];
        F.by2[k] = (float)w[3 * FL_NW + k]; F.edge[k] = (float)w[4 * FL_NW + k]; F.point[k] = (float)w[5 * FL_NW + k];
        F.gauss[k] = (float)w[6 * FL_NW + k];
    }
    F.by_c1 = (float)sc[0];
    F.by_c2 = (float)sc[1];
    F.cmax = (float)sc[2];
    F.quantize = quantize ? 1 : 0;
    const dim3 grid((W + FL_T - 1) / FL_T, (H + FL_T - 1) / FL_T, N);
    float2* partial = (float2*)scratch;
    { ProfScope ps_(SCR_PROF_FLIP, st);
      flip_kernel<<<grid, 256, 0, st>>>(H, W, test, ref, F, map_out, partial);
      flip_reduce_kernel<<<N, 256, 0, st>>>((int)(grid.x * grid.y), partial, 1.0 / ((double)H * W), mean_out, mse_out); }
    CHECK_LAUNCH("flip_kernel", 0, st);
    return 0;
}

int scr_flip_filters(double pixels_per_degree, double* weights, int32_t* radii, double* scalars) {
    if (!weights || !radii || !scalars) return fail("NULL argument");
    if (flip_filters(pixels_per_degree, weights, radii, scalars))
        return fail("pixels_per_degree %g: must be >= 1 with filter radii <= %d", pixels_per_degree, SCR_FLIP_MAX_RADIUS);
    return 0;
}

}  // extern "C"
