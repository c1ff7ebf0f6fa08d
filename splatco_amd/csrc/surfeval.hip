// splatco_amd/csrc/surfeval.hip -- mesh evaluation on the device (gfx950): the area-weighted surface sampler, the exact nearest
// neighbour from one point set into another and the score reduction behind accuracy / completeness / Chamfer and precision /
// recall / F-score.
//
// The definitions are include/splatco_surfeval.h's (tests/surfeval_ref.py restates them in numpy).  The sampler and the score are
// binary64 in the written order between float32 inputs and outputs; the Makefile's -ffp-contract=off keeps them uncontracted.
//
// Sampler: one thread per face for the counts; the caller's integer prefix sum; one thread per SAMPLE, which finds its face by
//   binary search in the inclusive prefix (as tsdf.hip finds an edge's vertex) -- a face with 100 000 samples is 100 000
//   threads that end in the same slot, not one thread with a long loop.  No atomics.
// Nearest: one thread per query in the order of the queries' clamped cells in the target's grid, knn_grid.h's
//   knn_grid_search_cross; the best is the pair (d, original index), compared as a pair.
// Score: 4096 items per workgroup, a record of 10 binary64 per workgroup (sum, max, eight counts), folded by one workgroup
//   (wg.h: the one summation order).  Counts are summed as binary64 integers below 2^31 each: exact.
#include "capi.h"
#include "knn_grid.h"
#include "wg.h"
#include "../../include/splatco_surfeval.h"

namespace scr {

constexpr int SE_THREADS = 256;
constexpr int SE_SCORE_ITEMS = 16;                                   // per thread
constexpr int SE_SCORE_PER_WG = SE_THREADS * SE_SCORE_ITEMS;         // 4096
constexpr int SE_REC = 2 + SCR_SURFEVAL_MAX_THRESHOLDS;              // sum, max, counts

// ------------------------------------------------------------------ sampler
__host__ __device__ __forceinline__ uint32_t se_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x21f0aaadu; x ^= x >> 15; x *= 0x735a2d97u; x ^= x >> 15;
    return x;
}
__device__ __forceinline__ double se_uniform(uint32_t seed_mixed, uint32_t f, uint32_t c) {
    return (double)se_mix(se_mix(seed_mixed ^ f) ^ c) * 0x1p-32;
}

struct SeFace { double p0[3], e1[3], e2[3]; };

__device__ __forceinline__ SeFace se_face(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t f) {
    const float* a = vertices + 3 * (size_t)faces[3 * f];
    const float* b = vertices + 3 * (size_t)faces[3 * f + 1];
    const float* c = vertices + 3 * (size_t)faces[3 * f + 2];
    SeFace t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t.p0[k] = (double)a[k];
        t.e1[k] = (double)b[k] - t.p0[k];
        t.e2[k] = (double)c[k] - t.p0[k];
    }
    return t;
}

__global__ void __launch_bounds__(SE_THREADS)
surfeval_face_counts_kernel(int64_t nf, const float* __restrict__ vertices, const int32_t* __restrict__ faces, double density,
                            uint32_t seed_mixed, int64_t* __restrict__ counts) {
    const int64_t f = (int64_t)blockIdx.x * SE_THREADS + threadIdx.x;
    if (f >= nf) return;
    const SeFace t = se_face(vertices, faces, f);
    const double cx = t.e1[1] * t.e2[2] - t.e1[2] * t.e2[1];
    const double cy = t.e1[2] * t.e2[0] - t.e1[0] * t.e2[2];
    const double cz = t.e1[0] * t.e2[1] - t.e1[1] * t.e2[0];
    const double area = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    const double want = area * density + se_uniform(seed_mixed, (uint32_t)f, 0u);
    int64_t n = 0;
    if (area - area == 0.0) n = want >= 0x1p31 ? (1ll << 31) : (int64_t)floor(want);      // A finite; want is not NaN then
    counts[f] = n;
}

__global__ void __launch_bounds__(SE_THREADS)
surfeval_sample_kernel(int64_t nf, int64_t ns, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                       const int64_t* __restrict__ ends, uint32_t seed_mixed, float* __restrict__ points,
                       int32_t* __restrict__ face_index) {
    const int64_t s = (int64_t)blockIdx.x * SE_THREADS + threadIdx.x;
    if (s >= ns) return;
    int64_t lo = 0, hi = nf - 1;                            // the first face with ends[f] > s; ends[nf - 1] = ns > s
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ends[mid] > s) hi = mid; else lo = mid + 1;
    }
    const int64_t f = lo;
    const uint32_t j = (uint32_t)(s - (f ? ends[f - 1] : 0));
    const SeFace t = se_face(vertices, faces, f);
    double r1 = se_uniform(seed_mixed, (uint32_t)f, 1u + 2u * j), r2 = se_uniform(seed_mixed, (uint32_t)f, 2u + 2u * j);
    if (r1 + r2 > 1.0) { r1 = 1.0 - r1; r2 = 1.0 - r2; }
#pragma unroll
    for (int k = 0; k < 3; ++k) points[3 * s + k] = (float)((t.p0[k] + r1 * t.e1[k]) + r2 * t.e2[k]);
    face_index[s] = (int32_t)f;
}

// ------------------------------------------------------------------ nearest neighbour
// the smallest (d, original index) at or below the cap; id = INT32_MAX: none (every index is below it)
struct BestCross {
    const int64_t* __restrict__ target_id;
    float d;
    int32_t id;
    __device__ __forceinline__ void offer(float v, int p) {
        if (v <= d) {                                       // rare after the first cells: the gather of the index is too
            const int32_t j = (int32_t)target_id[p];
            if (v < d || j < id) { d = v; id = j; }
        }
    }
    __device__ __forceinline__ float worst() const { return d; }
};

__global__ void __launch_bounds__(SE_THREADS)
surfeval_nearest_kernel(int64_t nq, KnnGrid gr, float cap2, const float* __restrict__ sorted_query, const int64_t* __restrict__ query_id,
                        const float* __restrict__ sorted_target, const int64_t* __restrict__ target_id,
                        const int32_t* __restrict__ cell_start, float* __restrict__ dist2, int32_t* __restrict__ index) {
    const int64_t s = (int64_t)blockIdx.x * SE_THREADS + threadIdx.x;      // position in cell order: neighbours in memory
    if (s >= nq) return;
    BestCross best{target_id, cap2, INT32_MAX};
    knn_grid_search_cross(sorted_query[3 * s], sorted_query[3 * s + 1], sorted_query[3 * s + 2], gr, sorted_target, cell_start, best);
    const int64_t i = query_id[s];
    dist2[i] = best.d;
    index[i] = best.id == INT32_MAX ? -1 : best.id;
}

// ------------------------------------------------------------------ score
struct SeThresholds { double t[SCR_SURFEVAL_MAX_THRESHOLDS]; };       // +-0 <= d always; unused slots hold -1: never counted

__device__ __forceinline__ double se_wave_max(double v) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) v = fmax(v, __shfl_xor(v, d, WAVE));
    return v;
}

// rec[wg] = (sum, max, counts[8]) of the workgroup's 4096 items; thread t takes items base + t, base + t + 256, ...
__global__ void __launch_bounds__(SE_THREADS)
surfeval_score_kernel(int64_t n, const float* __restrict__ dist2, SeThresholds thr, double* __restrict__ rec) {
    __shared__ double lds[(SE_THREADS / WAVE) * SE_REC];
    const int64_t base = (int64_t)blockIdx.x * SE_SCORE_PER_WG;
    double v[SE_REC];
#pragma unroll
    for (int k = 0; k < SE_REC; ++k) v[k] = 0.0;
    double m = 0.0;
#pragma unroll 4
    for (int it = 0; it < SE_SCORE_ITEMS; ++it) {
        const int64_t i = base + it * SE_THREADS + threadIdx.x;
        if (i >= n) break;
        const double d = sqrt((double)dist2[i]);
        v[0] += d;
        m = fmax(m, d);
#pragma unroll
        for (int k = 0; k < SCR_SURFEVAL_MAX_THRESHOLDS; ++k) v[2 + k] += d <= thr.t[k] ? 1.0 : 0.0;
    }
    m = se_wave_max(m);
    wg_wave_parts<SE_THREADS / WAVE>(v, lds);               // v[1] = 0 in every lane: slot 1 of each wave's row is free
    if (threadIdx.x < SE_REC && threadIdx.x != 1) {
        double t = lds[threadIdx.x];
#pragma unroll
        for (int w = 1; w < SE_THREADS / WAVE; ++w) t += lds[w * SE_REC + threadIdx.x];
        rec[(size_t)blockIdx.x * SE_REC + threadIdx.x] = t;
    }
    __syncthreads();                                        // the sums are read: the rows may take the maxima
    if ((threadIdx.x & (WAVE - 1)) == 0) lds[(threadIdx.x / WAVE) * SE_REC + 1] = m;
    __syncthreads();
    if (threadIdx.x == 1) {
        double t = lds[1];
#pragma unroll
        for (int w = 1; w < SE_THREADS / WAVE; ++w) t = fmax(t, lds[w * SE_REC + 1]);
        rec[(size_t)blockIdx.x * SE_REC + 1] = t;
    }
}

__global__ void __launch_bounds__(SE_THREADS)
surfeval_score_fold_kernel(int nwg, const double* __restrict__ rec, double* __restrict__ out) {
    __shared__ double lds[(SE_THREADS / WAVE) * SE_REC];
    __shared__ double lds_max[SE_THREADS / WAVE];
    double m = 0.0;
    for (int b = threadIdx.x; b < nwg; b += SE_THREADS) m = fmax(m, rec[(size_t)b * SE_REC + 1]);
    m = se_wave_max(m);
    if ((threadIdx.x & (WAVE - 1)) == 0) lds_max[threadIdx.x / WAVE] = m;
    double acc[SE_REC];
    fold_sum<SE_THREADS>(nwg, rec, lds, acc);               // holds a barrier: lds_max is visible after it
    if (threadIdx.x == 0) {
        m = lds_max[0];
#pragma unroll
        for (int w = 1; w < SE_THREADS / WAVE; ++w) m = fmax(m, lds_max[w]);
#pragma unroll
        for (int k = 0; k < SE_REC; ++k) out[k] = k == 1 ? m : acc[k];
    }
}

static unsigned se_grid(int64_t n) { return (unsigned)((n + SE_THREADS - 1) / SE_THREADS); }
static int64_t se_score_nwg(int64_t n) { return (n + SE_SCORE_PER_WG - 1) / SE_SCORE_PER_WG; }

}  // namespace scr

using namespace scr;

extern "C" {

int scr_surfeval_abi_version(void) { return SCR_SURFEVAL_ABI_VERSION; }

size_t scr_surfeval_score_scratch_bytes(int64_t n) {
    if (n < 1 || n >= (1ll << 31)) return 256;
    return align_up((size_t)se_score_nwg(n) * SE_REC * sizeof(double));
}

int scr_surfeval_face_counts(int64_t nf, const float* vertices, const int32_t* faces, double density, uint32_t seed,
                             int64_t* counts, void* stream) {
    SCR_MARK_FN;
    if (nf < 1 || 3 * nf >= (1ll << 31)) return fail("%s: nf = %lld: 3 nf is not in 3 .. 2^31 - 1", __func__, (long long)nf);
    if (!(density > 0.0) || !(density <= 1.79e308)) return fail("%s: density must be positive and finite", __func__);
    if (!vertices || !faces || !counts) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    surfeval_face_counts_kernel<<<se_grid(nf), SE_THREADS, 0, st>>>(nf, vertices, faces, density, se_mix(seed), counts);
    CHECK_LAUNCH("surfeval_face_counts_kernel", 0, st);
    return 0;
}

int scr_surfeval_sample(int64_t nf, int64_t ns, const float* vertices, const int32_t* faces, const int64_t* ends, uint32_t seed,
                        float* points, int32_t* face_index, void* stream) {
    SCR_MARK_FN;
    if (nf < 1 || 3 * nf >= (1ll << 31)) return fail("%s: nf = %lld: 3 nf is not in 3 .. 2^31 - 1", __func__, (long long)nf);
    if (ns < 0 || ns >= (1ll << 31)) return fail("%s: ns = %lld is not in 0 .. 2^31 - 1", __func__, (long long)ns);
    if (ns == 0) return 0;
    if (!vertices || !faces || !ends || !points || !face_index) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    surfeval_sample_kernel<<<se_grid(ns), SE_THREADS, 0, st>>>(nf, ns, vertices, faces, ends, se_mix(seed), points, face_index);
    CHECK_LAUNCH("surfeval_sample_kernel", 0, st);
    return 0;
}

int scr_surfeval_nearest(int64_t nq, int64_t nt, const float* grid_host, const float* sorted_query, const int64_t* query_id,
                         const float* sorted_target, const int64_t* target_id, const int32_t* cell_start, float max_dist,
                         float* dist2, int32_t* index, void* stream) {
    SCR_MARK_FN;
    if (nq < 1 || nq >= (1ll << 31)) return fail("%s: nq = %lld is not in 1 .. 2^31 - 1", __func__, (long long)nq);
    if (check_knn_grid(__func__, nt, grid_host)) return 1;
    if (max_dist != max_dist) return fail("%s: max_dist is NaN", __func__);
    if (!sorted_query || !query_id || !sorted_target || !target_id || !cell_start || !dist2 || !index)
        return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    const float cap2 = max_dist < 0.0f ? INFINITY : max_dist * max_dist;
    surfeval_nearest_kernel<<<se_grid(nq), SE_THREADS, 0, st>>>(nq, knn_grid(grid_host), cap2, sorted_query, query_id, sorted_target,
                                                              target_id, cell_start, dist2, index);
    CHECK_LAUNCH("surfeval_nearest_kernel", 0, st);
    return 0;
}

int scr_surfeval_score(int64_t n, const float* dist2, int32_t num_thresholds, const float* thresholds_host, void* scratch,
                       double* out, void* stream) {
    SCR_MARK_FN;
    if (n < 1 || n >= (1ll << 31)) return fail("%s: n = %lld is not in 1 .. 2^31 - 1", __func__, (long long)n);
    if (num_thresholds < 0 || num_thresholds > SCR_SURFEVAL_MAX_THRESHOLDS)
        return fail("%s: num_thresholds = %d is not in 0 .. %d", __func__, num_thresholds, SCR_SURFEVAL_MAX_THRESHOLDS);
    if (num_thresholds > 0 && !thresholds_host) return fail("%s: thresholds_host is NULL", __func__);
    SeThresholds thr;
    for (int k = 0; k < SCR_SURFEVAL_MAX_THRESHOLDS; ++k) {
        thr.t[k] = -1.0;
        if (k < num_thresholds) {
            if (!(thresholds_host[k] >= 0.0f)) return fail("%s: threshold %d is negative or NaN", __func__, k);
            thr.t[k] = (double)thresholds_host[k];
        }
    }
    if (!dist2 || !scratch || !out) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nwg = se_score_nwg(n);
    surfeval_score_kernel<<<(unsigned)nwg, SE_THREADS, 0, st>>>(n, dist2, thr, (double*)scratch);
    CHECK_LAUNCH("surfeval_score_kernel", 0, st);
    surfeval_score_fold_kernel<<<1, SE_THREADS, 0, st>>>((int)nwg, (const double*)scratch, out);
    CHECK_LAUNCH("surfeval_score_fold_kernel", 0, st);
    return 0;
}

}  // extern "C"
