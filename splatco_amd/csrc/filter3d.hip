// splatco_amd/csrc/filter3d.hip -- Mip-Splatting's 3D smoothing filter: per-anchor sampling distance, fused apply (gfx950).
//
// The world-space half of Mip-Splatting (the screen-space half is the rasterizer's antialiased mode): every primitive gets a
// lower size limit from the highest sampling rate at which a training camera observed it.  All float32, no contraction
// (-ffp-contract=off), every comparison exactly as written here and in include/splatco_raster.h:
//   camera row   16 floats: rows 0..2 of the 3x4 [R | t] (r00 r01 r02 t0 | r10 ... | r20 ...), tx, ty, focal, 0
//   p            px = ((r00 x + r01 y) + r02 z) + t0, py and pz alike
//   observed     x, y, z finite and pz > 0.2f and |px| <= tx pz and |py| <= ty pz
//   m            min over the observing cameras of pz / focal, +inf without one.  A minimum has no order: the same bits for
//                every order of the cameras
//   apply        Gaussian j of candidate c = row * k + slot (j = out_index[c] >= 0), f = row_filter[row]:
//                t_i = sqrt(s_i^2 + f^2), r_i = s_i / t_i, s'_i = t_i, o' = o ((r_0 r_1) r_2).  f == 0: the inputs' bits
//   backward     ds_i = g_s'_i r_i + ((g_o' o) prod_{j != i} r_j) (f / t_i)^2 / t_i, do = g_o' ((r_0 r_1) r_2); a NULL upstream
//                gradient is zero; f == 0: the upstream gradients' bits.  No division by s_i.
// In framework ops the distance pass is a dozen element-wise kernels over [N] per camera, and the apply step about twenty
// over [P,3] with an index_select of the filter per Gaussian.  Here: one pass over the points with the cameras read as
// wave-uniform data, and one pass over the V k candidates per direction.  Compaction keeps order, so j rises with c and a
// wave's rows of scaling / opacity are contiguous.  Every output row is written exactly once: no atomics, no memset, no scratch.
#include "capi.h"

namespace scr {

constexpr int F3_THREADS = 256;
constexpr int F3_CAM = 16;             // floats per packed camera

// One point per lane; the camera index is the same in every lane, so a camera row is wave-uniform data (scalar loads, one
// 64-byte row per camera and wave, no LDS, no barrier).  Any C >= 1: the loop has no chunks.
__global__ void __launch_bounds__(F3_THREADS)
filter3d_distance_kernel(int64_t N, const float* __restrict__ points, int C, const float* __restrict__ cams,
                         float* __restrict__ m_out) {
    const int64_t i = (int64_t)blockIdx.x * F3_THREADS + threadIdx.x;
    if (i >= N) return;
    const float x = points[3 * i + 0], y = points[3 * i + 1], z = points[3 * i + 2];
    float m = __builtin_inff();
    if (!nonfinite3(x, y, z)) {
        // the next camera's row is asked for before this one's arithmetic, and the three tests are evaluated without a
        // branch: a short-circuit would put a dependent scalar load behind each of them
        float4 a = ((const float4*)cams)[0], b = ((const float4*)cams)[1], d = ((const float4*)cams)[2], e = ((const float4*)cams)[3];
        for (int c = 0; c < C; ++c) {
            const float4* __restrict__ nx = (const float4*)(cams + (size_t)(c + 1 < C ? c + 1 : c) * F3_CAM);
            const float4 na = nx[0], nb = nx[1], nd = nx[2], ne = nx[3];
            const float px = ((a.x * x + a.y * y) + a.z * z) + a.w;
            const float py = ((b.x * x + b.y * y) + b.z * z) + b.w;
            const float pz = ((d.x * x + d.y * y) + d.z * z) + d.w;
            const float r = pz / e.z;
            const int take = (int)(pz > 0.2f) & (int)(fabsf(px) <= e.x * pz) & (int)(fabsf(py) <= e.y * pz) & (int)(r < m);
            m = take ? r : m;
            a = na; b = nb; d = nd; e = ne;
        }
    }
    m_out[i] = m;
}

struct F3Row {
    float s[3], o, f;
    int64_t j;
};
// candidate c -> its Gaussian's inputs; false where the candidate was not kept (or names a row outside [0, P))
__device__ __forceinline__ bool f3_load(int64_t c, int k, int64_t P, const int32_t* __restrict__ out_index,
                                        const float* __restrict__ row_filter, const float* __restrict__ scaling,
                                        const float* __restrict__ opacity, F3Row& r) {
    const int32_t j = out_index[c];
    if (j < 0 || (int64_t)j >= P) return false;
    r.j = j;
    r.f = row_filter[(uint32_t)c / (uint32_t)k];
    r.s[0] = scaling[3 * r.j + 0];
    r.s[1] = scaling[3 * r.j + 1];
    r.s[2] = scaling[3 * r.j + 2];
    r.o = opacity[r.j];
    return true;
}

__global__ void __launch_bounds__(F3_THREADS)
filter3d_apply_kernel(int64_t n, int k, int64_t P, const int32_t* __restrict__ out_index, const float* __restrict__ row_filter,
                      const float* __restrict__ scaling, const float* __restrict__ opacity, float* __restrict__ scaling_out,
                      float* __restrict__ opacity_out) {
    const int64_t c = (int64_t)blockIdx.x * F3_THREADS + threadIdx.x;
    F3Row r;
    if (c >= n || !f3_load(c, k, P, out_index, row_filter, scaling, opacity, r)) return;
    float t[3] = {r.s[0], r.s[1], r.s[2]}, o = r.o;
    if (r.f != 0.0f) {
        const float f2 = r.f * r.f;
        float q[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            t[i] = sqrtf(r.s[i] * r.s[i] + f2);
            q[i] = r.s[i] / t[i];
        }
        o = r.o * ((q[0] * q[1]) * q[2]);
    }
    scaling_out[3 * r.j + 0] = t[0];
    scaling_out[3 * r.j + 1] = t[1];
    scaling_out[3 * r.j + 2] = t[2];
    opacity_out[r.j] = o;
}

__global__ void __launch_bounds__(F3_THREADS)
filter3d_apply_backward_kernel(int64_t n, int k, int64_t P, const int32_t* __restrict__ out_index,
                               const float* __restrict__ row_filter, const float* __restrict__ scaling,
                               const float* __restrict__ opacity, const float* __restrict__ g_scaling /*may be NULL*/,
                               const float* __restrict__ g_opacity /*may be NULL*/, float* __restrict__ d_scaling,
                               float* __restrict__ d_opacity) {
    const int64_t c = (int64_t)blockIdx.x * F3_THREADS + threadIdx.x;
    F3Row r;
    if (c >= n || !f3_load(c, k, P, out_index, row_filter, scaling, opacity, r)) return;
    float ds[3] = {0.0f, 0.0f, 0.0f}, d_o = 0.0f;
    if (g_scaling) {
        ds[0] = g_scaling[3 * r.j + 0];
        ds[1] = g_scaling[3 * r.j + 1];
        ds[2] = g_scaling[3 * r.j + 2];
    }
    if (g_opacity) d_o = g_opacity[r.j];
    if (r.f != 0.0f) {
        const float f2 = r.f * r.f;
        float t[3], q[3], u[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            t[i] = sqrtf(r.s[i] * r.s[i] + f2);
            q[i] = r.s[i] / t[i];
            const float w = r.f / t[i];
            u[i] = (w * w) / t[i];                  // f^2 / t^3 without forming either power
        }
        const float go = d_o * r.o;
        ds[0] = ds[0] * q[0] + (go * (q[1] * q[2])) * u[0];
        ds[1] = ds[1] * q[1] + (go * (q[0] * q[2])) * u[1];
        ds[2] = ds[2] * q[2] + (go * (q[0] * q[1])) * u[2];
        d_o = d_o * ((q[0] * q[1]) * q[2]);
    }
    d_scaling[3 * r.j + 0] = ds[0];
    d_scaling[3 * r.j + 1] = ds[1];
    d_scaling[3 * r.j + 2] = ds[2];
    d_opacity[r.j] = d_o;
}

// the sizes of both apply entry points; V k < 2^31 (out_index is int32 and the kernels divide a 32-bit candidate index)
static int filter3d_apply_args(const char* name, int64_t V, int32_t k, int64_t P) {
    if (V < 0 || k < 1) return fail("%s: bad sizes V = %lld, k = %d", name, (long long)V, k);
    if (V > 2147483647LL / k) return fail("%s: V k = %lld x %d exceeds 2^31 - 1", name, (long long)V, k);
    if (P < 0 || P > V * k) return fail("%s: P = %lld outside [0, V k = %lld]", name, (long long)P, (long long)(V * k));
    return 0;
}

}  // namespace scr

using namespace scr;

extern "C" {

int scr_filter3d_distance(int64_t N, const float* points, int32_t C, const float* cameras, float* m, void* stream) {
    SCR_MARK_FN;
    if (N < 0 || N > 2147483647LL * F3_THREADS) return fail("scr_filter3d_distance: bad point count N = %lld", (long long)N);
    if (C < 1) return fail("scr_filter3d_distance: C = %d cameras (at least one)", C);
    if (N == 0) return 0;
    if (!points || !cameras || !m) return fail("scr_filter3d_distance: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    filter3d_distance_kernel<<<(unsigned)((N + F3_THREADS - 1) / F3_THREADS), F3_THREADS, 0, st>>>(N, points, C, cameras, m);
    CHECK_LAUNCH("filter3d_distance_kernel", 0, st);
    return 0;
}

int scr_filter3d_apply(int64_t V, int32_t k, int64_t P, const int32_t* out_index, const float* row_filter, const float* scaling,
                       const float* opacity, float* scaling_out, float* opacity_out, void* stream) {
    SCR_MARK_FN;
    if (filter3d_apply_args("scr_filter3d_apply", V, k, P)) return 1;
    if (P == 0) return 0;
    if (!out_index || !row_filter || !scaling || !opacity || !scaling_out || !opacity_out)
        return fail("scr_filter3d_apply: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = V * k;
    filter3d_apply_kernel<<<(unsigned)((n + F3_THREADS - 1) / F3_THREADS), F3_THREADS, 0, st>>>(
        n, k, P, out_index, row_filter, scaling, opacity, scaling_out, opacity_out);
    CHECK_LAUNCH("filter3d_apply_kernel", 0, st);
    return 0;
}

int scr_filter3d_apply_backward(int64_t V, int32_t k, int64_t P, const int32_t* out_index, const float* row_filter,
                                const float* scaling, const float* opacity, const float* g_scaling, const float* g_opacity,
                                float* d_scaling, float* d_opacity, void* stream) {
    SCR_MARK_FN;
    if (filter3d_apply_args("scr_filter3d_apply_backward", V, k, P)) return 1;
    if (P == 0) return 0;
    if (!out_index || !row_filter || !scaling || !opacity || !d_scaling || !d_opacity)
        return fail("scr_filter3d_apply_backward: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = V * k;
    filter3d_apply_backward_kernel<<<(unsigned)((n + F3_THREADS - 1) / F3_THREADS), F3_THREADS, 0, st>>>(
        n, k, P, out_index, row_filter, scaling, opacity, g_scaling, g_opacity, d_scaling, d_opacity);
    CHECK_LAUNCH("filter3d_apply_backward_kernel", 0, st);
    return 0;
}

}  // extern "C"
