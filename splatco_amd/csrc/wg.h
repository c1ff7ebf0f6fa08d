// splatco_amd/csrc/wg.h -- workgroup sums, record folds and the block scan, written once (gfx950).
//
// The library promises the same bits run after run, so every floating-point sum has ONE order, stated here and nowhere else:
//   a lane      adds its items in index order;
//   a wave      sums its 64 lanes by the xor butterfly over 32, 16, ..., 1 (wave_sum);
//   a workgroup adds its waves in ascending order, ((w0 + w1) + w2) + ... (wg_sum);
//   records     (one per workgroup of an earlier launch) are added in ascending order by one workgroup: thread t takes
//               records t, t + THREADS, ..., then the butterfly, then the waves in ascending order from 0 (fold_sum).
// A site whose waves combine in another order stages them with wg_wave_parts and states its own one-line combine.
// The caller owns the LDS: no helper hides a __shared__ array.  Every thread of the workgroup must call a helper that
// holds a barrier (all but wave_sum).
#pragma once
#include "common.h"

namespace scr {

// every lane returns the sum of the wave's 64 values (float or double)
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

// lds[w * K + k] = wave w's sum of component k; one barrier, after the stores.  v is left holding this wave's sums.
template <int WAVES, int K, class T>
__device__ __forceinline__ void wg_wave_parts(T (&v)[K], T* lds /*[WAVES][K]*/) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) lds[(threadIdx.x / WAVE) * K + k] = v[k];
    }
    __syncthreads();
}
template <int WAVES, class T>
__device__ __forceinline__ void wg_wave_parts(T v, T* lds /*[WAVES]*/) {
    T a[1] = {v};
    wg_wave_parts<WAVES>(a, lds);
}

// out[k] = the workgroup's sum of component k, written by thread k
template <int WAVES, int K, class T>
__device__ __forceinline__ void wg_sum(T (&v)[K], T* lds /*[WAVES][K]*/, T* __restrict__ out /*[K]*/) {
    wg_wave_parts<WAVES>(v, lds);
    if (threadIdx.x < K) {
        T t = lds[threadIdx.x];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) t += lds[w * K + threadIdx.x];
        out[threadIdx.x] = t;
    }
}

// One workgroup of THREADS: acc[k] = column k of rec[n][K].  The result is valid in thread 0.
template <int THREADS, int K, class T>
__device__ __forceinline__ void fold_sum(int n, const T* __restrict__ rec /*[n][K]*/, T* lds /*[THREADS / WAVE][K]*/, T (&acc)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = T(0);
    for (int b = threadIdx.x; b < n; b += THREADS) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += rec[(size_t)b * K + k];
    }
    wg_wave_parts<THREADS / WAVE>(acc, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            T t = T(0);
            for (int w = 0; w < THREADS / WAVE; ++w) t += lds[w * K + k];
            acc[k] = t;
        }
    }
}

// ------------------------------------------------------------------ block-wide exclusive scan
template <int THREADS>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds_waves /*[THREADS/64+1]*/,
                                                         uint32_t& block_total) {
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        uint32_t n = __shfl_up(inc, d, WAVE);
        if (lane >= d) inc += n;
    }
    if (lane == WAVE - 1) lds_waves[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < THREADS / WAVE; ++k) {
        uint32_t s = lds_waves[k];
        if (k < w) base += s;
        tot += s;
    }
    block_total = tot;
    __syncthreads();
    return base + inc - v;
}

}  // namespace scr
