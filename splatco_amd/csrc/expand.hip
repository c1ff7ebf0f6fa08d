// splatco_amd/csrc/expand.hip -- fused neural-Gaussian expansion + opacity-mask compaction (gfx950).
//
// Replaces the torch op chain of gaussian_renderer/__init__.py:68-111 (mask = neural_opacity > 0;
// repeat / cat / boolean-index / split; sigmoid, normalize, FMA): ~12 full-size temporaries become
// one streaming pass.  Candidate c = anchor v * k + offset slot; kept candidates keep their order
// (stable compaction), exactly like `concatenated_all[mask]`.
//
//   opacity = neural_opacity[c]                         color_out = color[c]
//   scaling = grid_scaling[v,3:6] * sigmoid(scale_rot[c,0:3])
//   rot     = scale_rot[c,3:7] / max(||.||, 1e-12)      (torch.nn.functional.normalize)
//   xyz     = anchor[v] + offsets[c] * grid_scaling[v,0:3]
//
// HBM-bound: 56 B read per candidate (+36 B per anchor), 56 B written per kept Gaussian.
// Compaction = the count / scan / write scheme of compact.h (count pass reads 4 B per candidate); this file
// supplies the predicates, the write kernels and the scheme's one scan kernel.  Backward is one thread per candidate;
// the per-anchor sums over its k candidates go through LDS in slot order -> no atomics, deterministic.
#include "capi.h"

namespace scr {

// pass 2 of every compaction (one workgroup; declared in compact.h): exclusive scan of the workgroup counts, total to *total
__global__ void __launch_bounds__(1024) compact_scan_kernel(uint32_t nwg, uint32_t* __restrict__ wg_count,
                                                            unsigned long long* __restrict__ total,
                                                            volatile unsigned long long* mailbox, unsigned long long seq) {
    __shared__ uint32_t lds[1024 / WAVE + 1];
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < nwg; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nwg ? wg_count[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<1024>(v, lds, tot);
        if (i < nwg) wg_count[i] = (uint32_t)carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        *total = carry;
        if (mailbox) {  // pinned host words the caller polls (capi.hip): value, then the stamp
            mailbox[0] = carry;
            __threadfence_system();
            mailbox[1] = seq;
        }
    }
}

// the expansion keeps a candidate whose opacity is positive
struct KeepOpacity {
    using Operand = float;
    const float* __restrict__ neural_opacity;
    __device__ float load(int64_t c) const { return neural_opacity[c]; }
    __device__ bool keep(float no, int64_t) const { return no > 0.0f; }
};

// ---- mask -> index list (the visible-anchor index of gaussian_renderer/__init__.py:23-29, `t[visible_mask]`): the same
// count / scan / write scheme on a byte mask; replaces torch.nonzero (a 60 GB/s int64 reduction + a select)
struct KeepMask {
    using Operand = uint8_t;
    const uint8_t* __restrict__ mask;
    __device__ uint8_t load(int64_t c) const { return mask[c]; }
    __device__ bool keep(uint8_t m, int64_t) const { return m != 0; }
};

__global__ void __launch_bounds__(COMPACT_THREADS)
mask_index_kernel(int64_t n, KeepMask mask, const uint32_t* __restrict__ wg_offset, int64_t* __restrict__ index,
                  int64_t* __restrict__ inverse) {
    const CompactRank<KeepMask> c = compact_rank(n, mask, wg_offset);
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) {
        const int64_t i = compact_item(r);
        if (c.keep[r]) index[c.pos[r]] = i;
        if (inverse && i < n) inverse[i] = c.keep[r] ? (int64_t)c.pos[r] : -1ll;
    }
}

// pass 3: expand + compact
__global__ void __launch_bounds__(COMPACT_THREADS)
expand_run_kernel(int64_t n, int k, const float* __restrict__ neural_opacity, const float* __restrict__ color,
                  const float* __restrict__ scale_rot, const float* __restrict__ offsets, int ldo,
                  const float* __restrict__ grid_scaling, const float* __restrict__ anchor,
                  const uint32_t* __restrict__ wg_offset, int32_t* __restrict__ out_index,
                  uint8_t* __restrict__ mask_out, float* __restrict__ xyz, float* __restrict__ color_out,
                  float* __restrict__ opacity, float* __restrict__ scaling, float* __restrict__ rot) {
    const CompactRank<KeepOpacity> cr = compact_rank(n, KeepOpacity{neural_opacity}, wg_offset);
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) {
        const int64_t i = compact_item(r);
        if (i >= n) continue;
        if (mask_out) mask_out[i] = cr.keep[r];
        if (!cr.keep[r]) {
            out_index[i] = -1;
            continue;
        }
        const size_t p = cr.pos[r];
        out_index[i] = (int32_t)p;
        const int64_t v = i / k;
        const float* sr = scale_rot + 7 * i;
        const float* gs = grid_scaling + 6 * v;
        opacity[p] = cr.v[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            color_out[3 * p + c] = color[3 * i + c];
            scaling[3 * p + c] = gs[3 + c] * (1.0f / (1.0f + __expf(-sr[c])));
            xyz[3 * p + c] = anchor[3 * v + c] + offsets[v * ldo + 3 * (i - v * k) + c] * gs[c];     // offsets rows: ldo floats apart (3 k when packed)
        }
        const float q0 = sr[3], q1 = sr[4], q2 = sr[5], q3 = sr[6];
        const float inv = 1.0f / fmaxf(sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3), 1e-12f);
        rot[4 * p + 0] = q0 * inv;
        rot[4 * p + 1] = q1 * inv;
        rot[4 * p + 2] = q2 * inv;
        rot[4 * p + 3] = q3 * inv;
    }
}

// backward: one thread per CANDIDATE (coalesced per-candidate reads / writes); the per-anchor sums
// (d grid_scaling, d anchor) of the k candidates of an anchor are added in slot order through LDS
// -> no atomics, deterministic.  A workgroup owns `apw` consecutive anchors (32, fewer when k is
// so large that 32 k partial records would not fit 48 KB of LDS).

__global__ void __launch_bounds__(1024)
expand_backward_kernel(int64_t V, int k, int apw, const float* __restrict__ scale_rot,
                       const float* __restrict__ offsets, int ldo, const float* __restrict__ grid_scaling,
                       const int32_t* __restrict__ out_index,
                       const float* __restrict__ g_xyz, const float* __restrict__ g_color,
                       const float* __restrict__ g_opacity, const float* __restrict__ g_scaling,
                       const float* __restrict__ g_rot, float* __restrict__ d_neural_opacity,
                       float* __restrict__ d_color, float* __restrict__ d_scale_rot, float* __restrict__ d_offsets,
                       float* __restrict__ d_grid_scaling, float* __restrict__ d_anchor,
                       const float* __restrict__ g_reg, float inv_P) {
    extern __shared__ __attribute__((aligned(16))) float part[];  // [apw * k][9]
    const int64_t v0 = (int64_t)blockIdx.x * apw;
    const int nloc = (int)min((int64_t)apw, V - v0) * k;  // candidates of this workgroup
    for (int c = threadIdx.x; c < nloc; c += blockDim.x) {
        const int64_t i = v0 * k + c, v = i / k;
        const int32_t p = out_index[i];
        const float* gs = grid_scaling + 6 * v;
        float dsr[7] = {0, 0, 0, 0, 0, 0, 0}, dof[3] = {0, 0, 0}, dcol[3] = {0, 0, 0}, dop = 0.0f;
        float acc9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // (d grid_scaling[0..5], d anchor[0..2]) of this candidate
        if (p >= 0) {
            const float* sr = scale_rot + 7 * i;
            dop = g_opacity[p];
            float sg[3], gsc[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                sg[ch] = 1.0f / (1.0f + __expf(-sr[ch]));
                gsc[ch] = g_scaling[3 * (size_t)p + ch];
            }
            if (g_reg) {   // + dL/dreg * d mean(prod(scaling)) / d scaling: the regulariser's gradient never exists as a tensor
                const float a = gs[3] * sg[0], b = gs[4] * sg[1], c = gs[5] * sg[2];     // the forward's scaling, recomputed
                const float w = g_reg[0] * inv_P;
                gsc[0] = gsc[0] + w * (b * c);
                gsc[1] = gsc[1] + w * (a * c);
                gsc[2] = gsc[2] + w * (a * b);
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                dcol[ch] = g_color[3 * (size_t)p + ch];
                const float gx = g_xyz[3 * (size_t)p + ch];
                acc9[6 + ch] = gx;
                dof[ch] = gx * gs[ch];
                acc9[ch] = gx * offsets[v * ldo + 3 * (i - v * k) + ch];
                acc9[3 + ch] = gsc[ch] * sg[ch];
                dsr[ch] = gsc[ch] * gs[3 + ch] * sg[ch] * (1.0f - sg[ch]);
            }
            const float q0 = sr[3], q1 = sr[4], q2 = sr[5], q3 = sr[6];
            const float nrm = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
            const float g0 = g_rot[4 * (size_t)p], g1 = g_rot[4 * (size_t)p + 1], g2 = g_rot[4 * (size_t)p + 2],
                        g3 = g_rot[4 * (size_t)p + 3];
            if (nrm > 1e-12f) {  // y = x/|x| : dx = (g - y (y.g)) / |x|
                const float inv = 1.0f / nrm;
                const float y0 = q0 * inv, y1 = q1 * inv, y2 = q2 * inv, y3 = q3 * inv;
                const float dot = y0 * g0 + y1 * g1 + y2 * g2 + y3 * g3;
                dsr[3] = (g0 - y0 * dot) * inv;
                dsr[4] = (g1 - y1 * dot) * inv;
                dsr[5] = (g2 - y2 * dot) * inv;
                dsr[6] = (g3 - y3 * dot) * inv;
            } else {  // clamped denominator: y = x / 1e-12
                dsr[3] = g0 * 1e12f; dsr[4] = g1 * 1e12f; dsr[5] = g2 * 1e12f; dsr[6] = g3 * 1e12f;
            }
        }
        d_neural_opacity[i] = dop;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            d_color[3 * i + ch] = dcol[ch];
            d_offsets[3 * i + ch] = dof[ch];
        }
#pragma unroll
        for (int ch = 0; ch < 7; ++ch) d_scale_rot[7 * i + ch] = dsr[ch];
#pragma unroll
        for (int ch = 0; ch < 9; ++ch) part[c * 9 + ch] = acc9[ch];
    }
    __syncthreads();
    // anchor sums: thread (anchor a, component ch) adds the k candidates in slot order
    const int na = nloc / k;
    for (int j = threadIdx.x; j < na * 9; j += blockDim.x) {
        const int a_ = j / 9, ch = j % 9;
        float sum = 0.0f;
        for (int sidx = 0; sidx < k; ++sidx) sum += part[(a_ * k + sidx) * 9 + ch];
        if (ch < 6) d_grid_scaling[6 * (v0 + a_) + ch] = sum;
        else d_anchor[3 * (v0 + a_) + ch - 6] = sum;
    }
}

}  // namespace scr

using namespace scr;

extern "C" {

size_t scr_expand_scratch_bytes(int64_t n) { return compact_scratch_bytes(n); }

int scr_expand_plan(int64_t n, const float* neural_opacity, void* scratch, int64_t* num_selected_host,
                    void* stream) {
    SCR_MARK_FN;
    if (!num_selected_host) return fail("num_selected_host is NULL");
    *num_selected_host = 0;
    if (n < 0) return fail("n < 0");
    if (n == 0) return 0;
    if (!neural_opacity || !scratch) return fail("NULL argument");
    if (n >= (1ll << 31)) return fail("more than 2^31 candidates");
    hipStream_t st = (hipStream_t)stream;
    return compact_plan("compact_count_kernel<KeepOpacity>", n, scratch, num_selected_host, st,
                        [&](const CompactScratch& s, unsigned long long* mb, unsigned long long seq) {
                            ProfScope ps_(SCR_PROF_EXPAND, st);
                            launch_compact_count(n, KeepOpacity{neural_opacity}, s, mb, seq, st);
                        });
}

// mask -> index list with the expansion's count / scan / write scheme (scratch: scr_expand_scratch_bytes(n))
int scr_mask_index_plan(int64_t n, const uint8_t* mask, void* scratch, int64_t* num_set_host, void* stream) {
    SCR_MARK_FN;
    if (!num_set_host) return fail("num_set_host is NULL");
    *num_set_host = 0;
    if (n < 0) return fail("n < 0");
    if (n == 0) return 0;
    if (!mask || !scratch) return fail("NULL argument");
    if (n >= (1ll << 31)) return fail("more than 2^31 mask entries");
    hipStream_t st = (hipStream_t)stream;
    return compact_plan("compact_count_kernel<KeepMask>", n, scratch, num_set_host, st,
                        [&](const CompactScratch& s, unsigned long long* mb, unsigned long long seq) {
                            ProfScope ps_(SCR_PROF_EXPAND, st);
                            launch_compact_count(n, KeepMask{mask}, s, mb, seq, st);
                        });
}

int scr_mask_index_run(int64_t n, const uint8_t* mask, const void* scratch, int64_t* index, int64_t* inverse, void* stream) {
    SCR_MARK_FN;
    if (n <= 0) return n < 0 ? fail("n < 0") : 0;
    if (!mask || !scratch || (!index && !inverse)) return fail("NULL argument");
    hipStream_t st = (hipStream_t)stream;
    { ProfScope ps_(SCR_PROF_EXPAND, st);
      mask_index_kernel<<<(uint32_t)compact_nwg(n), COMPACT_THREADS, 0, st>>>(n, KeepMask{mask}, (const uint32_t*)scratch, index, inverse); }
    CHECK_LAUNCH("mask_index_kernel", 0, st);
    return 0;
}

int scr_expand_run(int64_t V, int32_t k, const float* neural_opacity, const float* color,
                   const float* scale_rot, const float* offsets, int32_t offsets_ld, const float* grid_scaling,
                   const float* anchor, const void* scratch, int32_t* out_index, uint8_t* mask_out,
                   float* xyz, float* color_out, float* opacity, float* scaling, float* rot, void* stream) {
    SCR_MARK_FN;
    if (V < 0 || k <= 0) return fail("bad V / k");
    if (offsets_ld < 3 * k) return fail("offsets_ld %d: the offset rows of an anchor are 3 k = %d floats long", offsets_ld, 3 * k);
    if (V == 0) return 0;
    if (!neural_opacity || !color || !scale_rot || !offsets || !grid_scaling || !anchor || !scratch || !out_index)
        return fail("NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = V * k;
    { ProfScope ps_(SCR_PROF_EXPAND, st);
      expand_run_kernel<<<(uint32_t)compact_nwg(n), COMPACT_THREADS, 0, st>>>(n, k, neural_opacity, color, scale_rot, offsets, offsets_ld,
                                                                              grid_scaling, anchor, (const uint32_t*)scratch, out_index,
                                                                              mask_out, xyz, color_out, opacity, scaling, rot); }
    CHECK_LAUNCH("expand_run_kernel", 0, st);
    return 0;
}

int scr_expand_backward(int64_t V, int32_t k, const float* scale_rot, const float* offsets, int32_t offsets_ld,
                        const float* grid_scaling, const int32_t* out_index, const float* g_xyz,
                        const float* g_color, const float* g_opacity, const float* g_scaling,
                        const float* g_rot, float* d_neural_opacity, float* d_color, float* d_scale_rot,
                        float* d_offsets, float* d_grid_scaling, float* d_anchor, const float* g_reg, int64_t P,
                        void* stream) {
    SCR_MARK_FN;
    if (V < 0 || k <= 0) return fail("bad V / k");
    if (g_reg && P <= 0) return fail("scr_expand_backward: g_reg needs P = the number of selected candidates");
    if (offsets_ld < 3 * k) return fail("offsets_ld %d: the offset rows of an anchor are 3 k = %d floats long", offsets_ld, 3 * k);
    if (V == 0) return 0;
    if (!scale_rot || !offsets || !grid_scaling || !out_index || !d_neural_opacity || !d_color || !d_scale_rot ||
        !d_offsets || !d_grid_scaling || !d_anchor)
        return fail("NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int apw = max(1, min(32, (48 * 1024) / (k * 9 * (int)sizeof(float))));
    const int threads = min(1024, ((apw * k + 63) / 64) * 64);
    { ProfScope ps_(SCR_PROF_EXPAND_BACKWARD, st);
      expand_backward_kernel<<<(unsigned)((V + apw - 1) / apw), threads, (size_t)apw * k * 9 * sizeof(float), st>>>(
          V, k, apw, scale_rot, offsets, offsets_ld, grid_scaling, out_index, g_xyz, g_color, g_opacity, g_scaling, g_rot,
          d_neural_opacity, d_color, d_scale_rot, d_offsets, d_grid_scaling, d_anchor, g_reg,
          P > 0 ? (float)(1.0 / (double)P) : 0.0f); }
    CHECK_LAUNCH("expand_backward_kernel", 0, st);
    return 0;
}

}  // extern "C"
