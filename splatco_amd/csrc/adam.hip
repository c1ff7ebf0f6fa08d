// splatco_amd/csrc/adam.hip -- the optimizer step of the sharded training step as one streaming pass (gfx950).
//
// Reference: train.py:310-312 (`gaussians.optimizer.step()`), the optimizer is torch.optim.Adam(l, lr=0.0, eps=1e-15)
// over one group per per-anchor parameter plus the MLP / plane groups (scene/gaussian_model.py:520-575); no weight decay,
// no amsgrad.  At 20 M anchors the four per-anchor parameters are 5.7 GB: the step reads parameter, gradient and both
// moments and writes three of them back -- 40 GB, a tenth of the cfg4 step -- so it is priced against the copy probe,
// not against anything arithmetic.  Shape: one float4 of each of the four streams per lane and nothing else in flight
// (tools/exp/copy_probe.hip: the flat shape reaches 6.3 TB/s, eight loads per lane 3.6); up to ADAM_MAX tensors share a
// launch (the MLP / plane group is dozens of small tensors), a workgroup finds its tensor in a prefix table that lives
// in the kernel arguments.
//
// Arithmetic = torch's (fused_adam_utils.cuh; the single-tensor path gives the same numbers):
//   m  = m + (1 - beta1) (g - m)                      v = beta2 v + ((1 - beta2) g) g          (1 - beta in double, then fp32)
//   p -= (lr / bias1) * m / (sqrt(v) / sqrt(bias2) + eps)          bias_i = 1 - beta_i^step  (the two scalars formed in double by
//   the caller, as torch's Python does, and rounded to fp32 once)
#include "capi.h"

namespace scr {

constexpr int ADAM_MAX = 24;      // tensors per launch (the table travels in the kernel arguments: 1.4 KB)

typedef float adam_f4 __attribute__((ext_vector_type(4)));

struct AdamArgs {
    int n;
    float beta1, beta2, omb1, omb2, eps;    // omb = 1 - beta, rounded ONCE from double (1 - 0.999f is 4.7e-5 off)
    uint32_t first_block[ADAM_MAX + 1];     // tensor t owns workgroups first_block[t] .. first_block[t + 1] - 1
    float* p[ADAM_MAX];
    const float* g[ADAM_MAX];
    float* m[ADAM_MAX];
    float* v[ADAM_MAX];
    int64_t numel[ADAM_MAX];
    float step_size[ADAM_MAX];              // lr / bias1 (the caller's double quotient, rounded once)
    float bias2_sqrt[ADAM_MAX];             // torch divides by it (no reciprocal)
    uint8_t aligned[ADAM_MAX];              // all four pointers on 16 bytes
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float omb1, float b2, float omb2, float eps,
                                         float step_size, float bias2_sqrt) {
    m = m + omb1 * (g - m);
    v = b2 * v + (omb2 * g) * g;
    const float denom = sqrtf(v) / bias2_sqrt + eps;
    p = p - step_size * (m / denom);
}

__global__ void __launch_bounds__(256) adam_kernel(const AdamArgs a) {
    int t = 0;
    while (t + 1 < a.n && blockIdx.x >= a.first_block[t + 1]) ++t;      // uniform: scalar registers
    const int64_t n = a.numel[t];
    const int64_t e0 = ((int64_t)(blockIdx.x - a.first_block[t]) * 256 + threadIdx.x) * 4;
    if (e0 >= n) return;
    float* __restrict__ p = a.p[t];
    const float* __restrict__ g = a.g[t];
    float* __restrict__ m = a.m[t];
    float* __restrict__ v = a.v[t];
    const float o1 = a.omb1, b2 = a.beta2, o2 = a.omb2, eps = a.eps, ss = a.step_size[t], bs = a.bias2_sqrt[t];
    if (a.aligned[t] && e0 + 3 < n) {
        adam_f4 P = *(const adam_f4*)(p + e0), M = *(const adam_f4*)(m + e0), V = *(const adam_f4*)(v + e0);
        const adam_f4 G = __builtin_nontemporal_load((const adam_f4*)(g + e0));      // the gradient is dead after this pass
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = P[j], mj = M[j], vj = V[j];
            adam_one(pj, G[j], mj, vj, o1, b2, o2, eps, ss, bs);
            P[j] = pj;
            M[j] = mj;
            V[j] = vj;
        }
        *(adam_f4*)(p + e0) = P;
        *(adam_f4*)(m + e0) = M;
        *(adam_f4*)(v + e0) = V;
    } else {
        for (int64_t e = e0; e < min(e0 + 4, n); ++e) {
            float P = p[e], M = m[e], V = v[e];
            adam_one(P, g[e], M, V, o1, b2, o2, eps, ss, bs);
            p[e] = P;
            m[e] = M;
            v[e] = V;
        }
    }
}

// ---- row-sparse step: the same update on the rows a byte mask marks visible, every other row left alone (bit for bit).
// Tensors are row-major [n_rows, width]; a lane owns the same float4 as in adam_kernel, finds the rows of its four
// elements by a 32-bit division by the tensor's width (a multiply-high and two shifts with per-tensor constants:
// Granlund & Montgomery 1994, figure 4.1 -- exact for every 32-bit dividend), reads their mask bytes and only then touches
// the four streams: a lane without a visible element returns before any load, so a wave of such lanes issues none.  A
// float4 that straddles rows of different visibility is loaded whole, updated per element, and the select writes the old
// bits back to the invisible elements (their gradient may be NaN: it reaches nothing that is stored).
struct AdamRowsArgs {
    AdamArgs a;
    const uint8_t* mask;                    // [n_rows], nonzero = visible
    uint32_t width[ADAM_MAX];               // numel / n_rows
    uint32_t magic[ADAM_MAX];               // floor(2^32 (2^L - width) / width) + 1, L = ceil(log2 width)
    uint8_t sh1[ADAM_MAX], sh2[ADAM_MAX];   // min(L, 1), max(L - 1, 0)
};

__device__ __forceinline__ uint32_t adam_div(uint32_t n, uint32_t magic, uint32_t sh1, uint32_t sh2) {
    const uint32_t t = __umulhi(magic, n);
    return (t + ((n - t) >> sh1)) >> sh2;
}

__global__ void __launch_bounds__(256) adam_rows_kernel(const AdamRowsArgs ra) {
    const AdamArgs& a = ra.a;
    int t = 0;
    while (t + 1 < a.n && blockIdx.x >= a.first_block[t + 1]) ++t;      // uniform: scalar registers
    const uint32_t n = (uint32_t)a.numel[t];                            // the launcher refuses numel >= 2^32
    const uint64_t e64 = ((uint64_t)(blockIdx.x - a.first_block[t]) * 256 + threadIdx.x) * 4;
    if (e64 >= n) return;
    const uint32_t e0 = (uint32_t)e64;
    const uint32_t w = ra.width[t], mg = ra.magic[t], s1 = ra.sh1[t], s2 = ra.sh2[t];
    const uint8_t* __restrict__ mask = ra.mask;
    float* __restrict__ p = a.p[t];
    const float* __restrict__ g = a.g[t];
    float* __restrict__ m = a.m[t];
    float* __restrict__ v = a.v[t];
    const float o1 = a.omb1, b2 = a.beta2, o2 = a.omb2, eps = a.eps, ss = a.step_size[t], bs = a.bias2_sqrt[t];
    if (a.aligned[t] && n - e0 >= 4) {
        bool vis[4];
        const uint32_t r0 = adam_div(e0, mg, s1, s2);
        if (w >= 4) {                       // uniform.  At most two rows under one float4: the first element's and the last's
            const uint32_t left = w - (e0 - r0 * w);      // elements of row r0 from e0 on (>= 1)
            const bool v0 = mask[r0] != 0, v1 = mask[r0 + (left < 4 ? 1u : 0u)] != 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) vis[j] = (uint32_t)j < left ? v0 : v1;
        } else {
            vis[0] = mask[r0] != 0;
#pragma unroll
            for (int j = 1; j < 4; ++j) vis[j] = mask[adam_div(e0 + j, mg, s1, s2)] != 0;
        }
        if (!(vis[0] | vis[1] | vis[2] | vis[3])) return;
        adam_f4 P = *(const adam_f4*)(p + e0), M = *(const adam_f4*)(m + e0), V = *(const adam_f4*)(v + e0);
        const adam_f4 G = __builtin_nontemporal_load((const adam_f4*)(g + e0));      // the gradient is dead after this pass
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = P[j], mj = M[j], vj = V[j];
            adam_one(pj, G[j], mj, vj, o1, b2, o2, eps, ss, bs);
            P[j] = vis[j] ? pj : P[j];
            M[j] = vis[j] ? mj : M[j];
            V[j] = vis[j] ? vj : V[j];
        }
        *(adam_f4*)(p + e0) = P;
        *(adam_f4*)(m + e0) = M;
        *(adam_f4*)(v + e0) = V;
    } else {
        const uint32_t e1 = n - e0 < 4 ? n : e0 + 4;
        for (uint32_t e = e0; e < e1; ++e) {
            if (!mask[adam_div(e, mg, s1, s2)]) continue;
            float P = p[e], M = m[e], V = v[e];
            adam_one(P, g[e], M, V, o1, b2, o2, eps, ss, bs);
            p[e] = P;
            m[e] = M;
            v[e] = V;
        }
    }
}

// the launch table of tensors ts[0 .. a.n - 1] (a.n set by the caller); false: more than 2^31 workgroups in one launch
static bool adam_table(AdamArgs& a, const scr_adam_tensor* ts, double beta1, double beta2, double eps) {
    a.beta1 = (float)beta1;
    a.beta2 = (float)beta2;
    a.omb1 = (float)(1.0 - beta1);
    a.omb2 = (float)(1.0 - beta2);
    a.eps = (float)eps;
    uint64_t blocks = 0;
    for (int t = 0; t < a.n; ++t) {
        const scr_adam_tensor& x = ts[t];
        a.first_block[t] = (uint32_t)blocks;
        blocks += (uint64_t)((x.numel + 1023) / 1024);     // 256 lanes x one float4
        if (blocks > 0x7fffffffull) return false;
        a.p[t] = x.param;
        a.g[t] = x.grad;
        a.m[t] = x.exp_avg;
        a.v[t] = x.exp_avg_sq;
        a.numel[t] = x.numel;
        a.step_size[t] = (float)x.step_size;
        a.bias2_sqrt[t] = (float)x.bias_correction2_sqrt;
        a.aligned[t] = ((((uintptr_t)x.param | (uintptr_t)x.grad | (uintptr_t)x.exp_avg | (uintptr_t)x.exp_avg_sq) & 15u) == 0);
    }
    a.first_block[a.n] = (uint32_t)blocks;
    return true;
}

}  // namespace scr

using namespace scr;

extern "C" {

int scr_adam_step(int32_t n_tensors, const scr_adam_tensor* tensors, double beta1, double beta2, double eps, void* stream) {
    SCR_MARK_FN;
    if (n_tensors < 0) return fail("scr_adam_step: n_tensors < 0");
    if (n_tensors == 0) return 0;
    if (!tensors) return fail("scr_adam_step: tensors is NULL");
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0)) return fail("scr_adam_step: bad beta / eps");
    for (int t = 0; t < n_tensors; ++t) {
        const scr_adam_tensor& x = tensors[t];
        if (x.numel < 0 || (x.numel > 0 && (!x.param || !x.grad || !x.exp_avg || !x.exp_avg_sq))) return fail("scr_adam_step: NULL tensor");
        if (!(x.step_size >= 0.0) || !(x.step_size < 1e30) || !(x.bias_correction2_sqrt > 0.0))
            return fail("scr_adam_step: step_size must be finite and >= 0, bias_correction2_sqrt > 0 (step >= 1)");
    }
    hipStream_t st = (hipStream_t)stream;
    for (int t0 = 0; t0 < n_tensors; t0 += ADAM_MAX) {
        AdamArgs a;
        a.n = min(ADAM_MAX, n_tensors - t0);
        if (!adam_table(a, tensors + t0, beta1, beta2, eps)) return fail("scr_adam_step: more than 2^31 workgroups in one launch");
        if (a.first_block[a.n]) adam_kernel<<<a.first_block[a.n], 256, 0, st>>>(a);
    }
    CHECK_LAUNCH("adam_kernel", 0, st);
    return 0;
}

// the same update on the rows of [n_rows, numel / n_rows] tensors that row_mask marks (nonzero), nothing else touched
int scr_adam_step_rows(int32_t n_tensors, const scr_adam_tensor* tensors, const uint8_t* row_mask, int64_t n_rows,
                       double beta1, double beta2, double eps, void* stream) {
    SCR_MARK_FN;
    if (n_tensors < 0) return fail("scr_adam_step_rows: n_tensors < 0");
    if (n_rows < 0) return fail("scr_adam_step_rows: n_rows < 0");
    if (n_tensors > 0 && !tensors) return fail("scr_adam_step_rows: tensors is NULL");
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0)) return fail("scr_adam_step_rows: bad beta / eps");
    if (n_rows > 0 && !row_mask) return fail("scr_adam_step_rows: row_mask is NULL");
    int64_t total = 0;
    for (int t = 0; t < n_tensors; ++t) {
        const scr_adam_tensor& x = tensors[t];
        if (x.numel < 0 || (x.numel > 0 && (!x.param || !x.grad || !x.exp_avg || !x.exp_avg_sq))) return fail("scr_adam_step_rows: NULL tensor");
        if (!(x.step_size >= 0.0) || !(x.step_size < 1e30) || !(x.bias_correction2_sqrt > 0.0))
            return fail("scr_adam_step_rows: step_size must be finite and >= 0, bias_correction2_sqrt > 0 (step >= 1)");
        if (n_rows == 0 ? x.numel != 0 : x.numel % n_rows != 0) return fail("scr_adam_step_rows: numel is not a multiple of n_rows");
        if (x.numel > 0xffffffffll) return fail("scr_adam_step_rows: numel of 2^32 or more (32-bit element index)");
        total += x.numel;
    }
    if (total == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    for (int t0 = 0; t0 < n_tensors; t0 += ADAM_MAX) {
        AdamRowsArgs ra;
        AdamArgs& a = ra.a;
        ra.mask = row_mask;
        a.n = min(ADAM_MAX, n_tensors - t0);
        if (!adam_table(a, tensors + t0, beta1, beta2, eps)) return fail("scr_adam_step_rows: more than 2^31 workgroups in one launch");
        for (int t = 0; t < a.n; ++t) {
            const uint32_t w = a.numel[t] > 0 ? (uint32_t)(a.numel[t] / n_rows) : 1u;      // an empty tensor launches nothing
            uint32_t L = 0;
            while (L < 32 && (1ull << L) < w) ++L;
            ra.width[t] = w;
            ra.magic[t] = (uint32_t)((((1ull << L) - w) << 32) / w + 1);
            ra.sh1[t] = (uint8_t)(L < 1 ? L : 1);
            ra.sh2[t] = (uint8_t)(L > 1 ? L - 1 : 0);
        }
        if (a.first_block[a.n]) adam_rows_kernel<<<a.first_block[a.n], 256, 0, st>>>(ra);
    }
    CHECK_LAUNCH("adam_rows_kernel", 0, st);
    return 0;
}

}  // extern "C"
