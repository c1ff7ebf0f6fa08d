// splatco_amd/csrc/compact.h -- order-preserving stream compaction on the device, written once (gfx950): the
// count / scan / write scheme behind the expansion (expand.hip: opacity > 0), the mask -> index list (expand.hip) and the
// distinct voxel keys (scene_init.hip: head flags on sorted keys).  The block scan it rests on is wg.h's.
//
//   count   compact_count_kernel<Keep>: kept items per workgroup of 1024 items (256 threads x 4 rounds of 256 items)
//   scan    compact_scan_kernel (one workgroup): exclusive prefix of the workgroup counts in place, the total to the
//           scratch and to the host's pinned mailbox (compact_plan() of capi.h reads it there to size the outputs)
//   write   the user's own kernel, same launch shape; compact_rank() gives every item its `keep` and its output position
//           = workgroup offset + kept items of earlier rounds + of earlier waves of this round + of lower lanes
//
// A use supplies its predicate as a functor of two phases, so that the loads of a thread's four items are issued together and
// no ballot waits behind a branch around a load (`i < n && load` cost four memory round trips one after the other):
//   struct Keep { using Operand = ...;
//                 __device__ Operand load(int64_t c) const;              // c = min(i, n - 1): always in bounds
//                 __device__ bool keep(const Operand& v, int64_t i) const; };      // asked for i < n only
#pragma once
#include "wg.h"        // block_exclusive_scan

namespace scr {

// ------------------------------------------------------------------ geometry and scratch
constexpr int COMPACT_THREADS = 256;
constexpr int COMPACT_ITEMS = 4;                                    // items per thread, one per round
constexpr int COMPACT_PER_WG = COMPACT_THREADS * COMPACT_ITEMS;     // items per workgroup

inline __host__ size_t compact_nwg(int64_t n) { return (size_t)((n + COMPACT_PER_WG - 1) / COMPACT_PER_WG); }
inline __host__ size_t compact_scratch_bytes(int64_t n) { return align_up((compact_nwg(n) + 1) * 4) + 256; }

// the caller-owned scratch block: what the count pass leaves for the write pass
struct CompactScratch {
    uint32_t* wg;                 // [nwg + 1] kept items per workgroup; after the scan their exclusive prefix
    unsigned long long* total;    // kept items in all
};
inline __host__ CompactScratch compact_scratch(void* base, int64_t n) {
    return {(uint32_t*)base, (unsigned long long*)((char*)base + align_up((compact_nwg(n) + 1) * 4))};
}

// item of this thread in round r
__device__ __forceinline__ int64_t compact_item(int r) {
    return (int64_t)blockIdx.x * COMPACT_PER_WG + r * COMPACT_THREADS + threadIdx.x;
}

// ------------------------------------------------------------------ count
// kept items of this workgroup, valid in thread 0
template <class Keep>
__device__ __forceinline__ uint32_t compact_count(int64_t n, const Keep& k) {
    __shared__ uint32_t wsum[COMPACT_THREADS / WAVE];
    typename Keep::Operand v[COMPACT_ITEMS];
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) v[r] = k.load(min(compact_item(r), n - 1));
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) {
        const int64_t i = compact_item(r);
        c += (uint32_t)__builtin_popcountll(lanes(i < n && k.keep(v[r], i)));
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;  // every lane of a wave holds the wave's count
    __syncthreads();
    return threadIdx.x == 0 ? wsum[0] + wsum[1] + wsum[2] + wsum[3] : 0u;
}

template <class Keep>
__global__ void __launch_bounds__(COMPACT_THREADS) compact_count_kernel(int64_t n, Keep k, uint32_t* __restrict__ wg_count) {
    const uint32_t c = compact_count(n, k);
    if (threadIdx.x == 0) wg_count[blockIdx.x] = c;
}

// ------------------------------------------------------------------ rank
// per item of this thread: the operand the predicate loaded, its verdict (false for i >= n) and, where kept, the item's
// position in the compacted output
template <class Keep>
struct CompactRank {
    typename Keep::Operand v[COMPACT_ITEMS];
    bool keep[COMPACT_ITEMS];
    uint32_t pos[COMPACT_ITEMS];
};

template <class Keep>
__device__ __forceinline__ CompactRank<Keep> compact_rank(int64_t n, const Keep& k, const uint32_t* __restrict__ wg_offset) {
    __shared__ uint32_t wcnt[COMPACT_ITEMS][COMPACT_THREADS / WAVE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    CompactRank<Keep> o;
    uint32_t below[COMPACT_ITEMS];
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) o.v[r] = k.load(min(compact_item(r), n - 1));
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) {
        const int64_t i = compact_item(r);
        o.keep[r] = i < n && k.keep(o.v[r], i);
        const unsigned long long bal = lanes(o.keep[r]);
        below[r] = lanes_below(bal);
        if (lane == 0) wcnt[r][w] = (uint32_t)__builtin_popcountll(bal);
    }
    __syncthreads();
    uint32_t run = wg_offset[blockIdx.x];
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) {
        uint32_t base = run;
#pragma unroll
        for (int q = 0; q < COMPACT_THREADS / WAVE; ++q) {
            const uint32_t c = wcnt[r][q];
            if (q < w) base += c;
            run += c;
        }
        o.pos[r] = base + below[r];
    }
    return o;
}

// ------------------------------------------------------------------ scan + launch
// one workgroup: exclusive scan of the workgroup counts in place, the total to *total and to the mailbox (expand.hip)
__global__ void __launch_bounds__(1024) compact_scan_kernel(uint32_t nwg, uint32_t* __restrict__ wg_count,
                                                            unsigned long long* __restrict__ total,
                                                            volatile unsigned long long* mailbox, unsigned long long seq);

// the count pass of a compaction of n > 0 items: per-workgroup counts, then their scan
template <class Keep>
void launch_compact_count(int64_t n, Keep keep, const CompactScratch& s, unsigned long long* mailbox,
                          unsigned long long seq, hipStream_t st) {
    const uint32_t nwg = (uint32_t)compact_nwg(n);
    compact_count_kernel<Keep><<<nwg, COMPACT_THREADS, 0, st>>>(n, keep, s.wg);
    compact_scan_kernel<<<1, 1024, 0, st>>>(nwg, s.wg, s.total, mailbox, seq);
}

}  // namespace scr
