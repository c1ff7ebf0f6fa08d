// splatco_amd/csrc/common.h -- shared declarations of the gfx950 rasterizer kernels.
// Written for CDNA4 (wave64, 256 CUs / 8 XCDs) only; there is no other target.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/splatco_raster.h"

namespace scr {

// min(a + b, 2^32 - 1)
__host__ __device__ __forceinline__ uint32_t sat_add_u32(uint32_t a, uint32_t b) {
    const uint32_t s = a + b;
    return s < a ? 0xFFFFFFFFu : s;
}


constexpr int TILE = SCR_TILE;          // 16x16 pixels
constexpr int TILE_PIX = TILE * TILE;   // 256
constexpr int WAVE = 64;                // CDNA wavefront
constexpr int NUM_XCD = 8;
constexpr int PRE_BLOCK = 256;          // Gaussians per preprocess-backward workgroup
constexpr int BIN_THREADS = 1024;       // threads of a preprocess / scatter workgroup
constexpr int BIN_ROUNDS = 4;           // Gaussians per thread
constexpr int BIN_GPW = BIN_THREADS * BIN_ROUNDS;  // Gaussians per preprocess / scatter workgroup
constexpr int LDS_HIST_MAX_TILES = 40000;  // per-tile LDS histogram (4 B / tile) in the CU's 160 KB of LDS (4K images: 32400 tiles)
constexpr int ID_BITS = 28;             // sort key = depth:32 | id:28 | quadrant mask:4  ->  P < 2^28
constexpr int WG_SORT_MAX = 8192;       // keys an on-chip workgroup sort takes (binning.hip tile_sort_wg_kernel): one wave per 1024
constexpr int REC_F = 12;               // floats per splat record (48 B, three float4)
constexpr int GRAD_F = 9;               // floats per per-instance gradient record (GradRec)

inline __host__ __device__ size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

struct Grid {
    int W, H, gx, gy, tiles;
    __host__ __device__ Grid(int H_, int W_)
        : W(W_), H(H_), gx((W_ + TILE - 1) / TILE), gy((H_ + TILE - 1) / TILE), tiles(gx * gy) {}
};

// ---- geom buffer: per-Gaussian state (written by the plan phase) + per-tile counters ----
struct GeomView {
    float4* rec;            // [P][3] float4 : (mx,my,A,B) (C,o,r,g) (b,depth,rect_lo,rect_hi)
    uint32_t* tiles_touched;  // [P]
    uint32_t* point_offsets;  // [P] inclusive scan of tiles_touched (written by the scatter kernel)
    uint8_t* clamped;         // [P] bit c set when SH colour channel c was clamped at 0
    uint2* gm_base;           // [P] (b, rw): Gaussian-major index of the instance in tile (tx, ty) = b + ty*rw + tx
                              //     (b = first index - y0*rw - x0 mod 2^32, rw = rect width; written by the scatter kernel)
    uint32_t* live_bits;      // [P] bit k: the k-th tile of the Gaussian's rect walk (row-major) can be reached by one of its
                              //     quadrants (quadrant mask != 0), k < 32; written by the scatter kernel.  An instance whose bit
                              //     is clear gets no gradient record (blend backward) and none is read (preprocess backward)
    uint8_t* has_rec;         // [P] deep lists only: set by the blend backward for every Gaussian that got at least one gradient
                              //     record, so that preprocess_backward skips the record loop of the others (at 20 M anchors most
                              //     Gaussians sit behind every pixel's last contributor in all of their tiles)
    uint32_t* block_sums;     // [ceil(P/BIN_GPW)] -> exclusive prefix after scan
    uint32_t* tile_count;     // [tiles] instances per tile (preprocess -> plan scan); afterwards the blend launches' tile order
    uint32_t* ranges;         // [tiles][2] (start, end)
    uint32_t* cursor;         // [tiles]
    int64_t P;                  // Gaussians (for the per-Gaussian arrays' sizes)
    unsigned long long* total;  // [16] number of instances, largest per-tile instance count, [2] 1 = tile_count holds the blend tile
                                //      order, [3] plan flags (SCR_PLAN_*, raised by preprocess_kernel), [4..12] first entry of
                                //      every XCD's list in the tile order
    size_t bytes;
};

inline __host__ GeomView geom_view(void* base, int64_t P, int H, int W) {
    Grid g(H, W);
    char* p = (char*)base;
    size_t off = 0;
    GeomView v;
    auto take = [&](size_t n) { char* q = p ? p + off : nullptr; off += align_up(n); return q; };
    size_t nblk = (size_t)((P + BIN_GPW - 1) / BIN_GPW);
    v.rec = (float4*)take((size_t)P * REC_F * 4);
    v.tiles_touched = (uint32_t*)take((size_t)P * 4);
    v.point_offsets = (uint32_t*)take((size_t)P * 4);
    v.clamped = (uint8_t*)take((size_t)P);
    v.gm_base = (uint2*)take((size_t)P * 8);
    v.live_bits = (uint32_t*)take((size_t)P * 4);
    v.has_rec = (uint8_t*)take((size_t)P);
    v.block_sums = (uint32_t*)take((nblk + 1) * 4);
    v.tile_count = (uint32_t*)take((size_t)g.tiles * 4);
    v.ranges = (uint32_t*)take((size_t)g.tiles * 8);
    v.cursor = (uint32_t*)take((size_t)g.tiles * 4);
    v.total = (unsigned long long*)take(128);
    v.bytes = off;
    v.P = P;
    return v;
}

// Deep tile lists (MatrixCity scale: tens of thousands of entries per tile, a few hundred of them in front of the pixels'
// last contributors): the tile sort does not materialise gm_index -- one 8-byte gm_base gather per instance, most of them
// for entries the backward pass never visits -- and the blend backward derives the index of the entries it does visit
// from gm_base itself.  With every entry live (the benchmark density) the sort's coalesced gm_index is the cheaper way
// round (measured both ways: tile sort 5.1 -> 4.0 ms at 20 M anchors; blend backward +4 % at cfg1 / cfg2).
// Both passes derive the choice from the same two numbers.
extern int g_force_deep_lists;      // capi.hip; scr_debug_force_deep_lists: -1 = by the rule below, 0 / 1 = forced (parity tests)
inline __host__ bool deep_lists(int64_t I, int tiles) {
    return g_force_deep_lists >= 0 ? g_force_deep_lists != 0 : I > (int64_t)8192 * tiles;
}

// per-Gaussian record flags (has_rec): from which mean list length on the blend backward marks the Gaussians it wrote a
// record for and preprocess_backward treats the others like invisible ones.  Measured (round 3): with 2048 entries per
// tile on average and more the flags pay (preprocess_backward 0.88 -> 0.79 ms at cfg2, 0.97 -> 0.86 at cfg3, 4.6 -> 2.2 at
// cfg4; the byte stores are lost in the blend backward); at the benchmark density (540 per tile, nearly every Gaussian has
// a record) they cost the blend backward 1 - 2 %.  Forced together with the deep-list variants by the test hook.
constexpr int FLAGS_MIN_MEAN = 2048;
inline __host__ bool record_flags(int64_t I, int tiles) {
    return g_force_deep_lists >= 0 ? g_force_deep_lists != 0 : I > (int64_t)FLAGS_MIN_MEAN * tiles;
}

// ---- binning buffer: per (Gaussian, tile) instance lists ----
struct BinView {
    unsigned long long* keys;  // [I] grouped by tile, unsorted: depth bits << 32 | gaussian id << 4 | quadrant mask
    uint32_t* point_list;      // [I] Gaussian ids, per tile sorted by (depth, id)
    uint32_t* gm_index;        // [I] sorted position -> Gaussian-major instance index (where its gradient record goes)
    uint8_t* qmask;            // [I] sorted position -> 4-bit mask of the tile's 8x8 quadrants the splat can touch
    unsigned long long* keys2; // [I] second buffer of the merge passes (only when a tile exceeds one sort chunk)
    size_t bytes;
};

inline __host__ BinView bin_view(void* base, int64_t I, int64_t max_tile_instances) {
    char* p = (char*)base;
    size_t off = 0;
    BinView v;
    auto take = [&](size_t n) { char* q = p ? p + off : nullptr; off += align_up(n); return q; };
    size_t n = (size_t)(I > 0 ? I : 1);
    v.keys = (unsigned long long*)take(n * 8);
    v.point_list = (uint32_t*)take(n * 4);
    v.gm_index = (uint32_t*)take(n * 4);
    v.qmask = (uint8_t*)take(n);
    const bool merge = max_tile_instances > WG_SORT_MAX;  // tiles above one workgroup sort chunk (binning.hip) take global merge passes
    v.keys2 = merge ? (unsigned long long*)take(n * 8) : nullptr;
    v.bytes = off;
    return v;
}

// ---- backward scratch: one gradient record per (Gaussian, tile) instance at its Gaussian-major index: nine floats
// (Y = opacity G dL/dalpha: sum Y dx, sum Y dy, sum Y dx^2, sum Y dx dy | sum Y dy^2, sum Y, c0, c1 | c2), 36 bytes, back to back.  The two
// four-float parts are moved with dword-aligned 16-byte accesses (gfx950 global memory needs dword alignment only);
// separate arrays per part were measured and rejected: the lone 4-byte stores cost a whole 32-byte sector each.
struct __attribute__((packed, aligned(4))) GradQuad { float x, y, z, w; };
struct __attribute__((packed, aligned(4))) GradRec { GradQuad a, b; float c; };
static_assert(sizeof(GradRec) == 36, "36-byte gradient records");
// With gradients of the depth / opacity maps (the *_aux entry points) a second stream lies behind the records: one float per
// instance at the same Gaussian-major index, sum_pixels (alpha T) dL/ddepth.  It is written, zeroed and skipped exactly where
// the record of the same index is, so every verdict of the record readers (live_bits, cut keys, has_rec) holds for it.
inline __host__ size_t grad_rec_bytes(int64_t I) { return align_up((size_t)(I > 0 ? I : 1) * sizeof(GradRec)); }
inline __host__ size_t grad_z_bytes(int64_t I) { return align_up((size_t)(I > 0 ? I : 1) * sizeof(float)); }

// ---- image buffer ----
struct ImgView {
    float* final_T;       // [H*W]
    uint32_t* n_contrib;  // [H*W]
    unsigned long long* cut_key;  // [tiles] written by the blend backward: sort key (depth bits << 32 | id) of the tile's first
                                  //         list entry that got no gradient record (~0: all have one)
    size_t bytes;
};

inline __host__ ImgView img_view(void* base, int H, int W) {
    char* p = (char*)base;
    size_t off = 0;
    ImgView v;
    auto take = [&](size_t n) { char* q = p ? p + off : nullptr; off += align_up(n); return q; };
    v.final_T = (float*)take((size_t)H * W * 4);
    v.n_contrib = (uint32_t*)take((size_t)H * W * 4);
    v.cut_key = (unsigned long long*)take((size_t)Grid(H, W).tiles * 8 + 8);   // [tiles] is the stamp word, see blend.hip
    v.bytes = off;
    return v;
}

// Kernel-side copy of the settings (scalars by value, matrices by device pointer).
struct KSettings {
    int H, W;
    float tanfovx, tanfovy, fx, fy;
    const float* bg;
    float scale_modifier;
    const float* view;
    const float* proj;
    int sh_degree;
    const float* campos;
};

inline __host__ KSettings ksettings(const scr_settings* s) {
    KSettings k;
    k.H = s->image_height;
    k.W = s->image_width;
    k.tanfovx = s->tanfovx;
    k.tanfovy = s->tanfovy;
    k.fx = (float)s->image_width / (2.0f * s->tanfovx);   // normative: binary32, this order
    k.fy = (float)s->image_height / (2.0f * s->tanfovy);
    k.bg = s->bg;
    k.scale_modifier = s->scale_modifier;
    k.view = s->viewmatrix;
    k.proj = s->projmatrix;
    k.sh_degree = s->sh_degree;
    k.campos = s->campos;
    return k;
}

// Per-lane select through an SGPR-pair lane mask.  hipcc usually emits the VOP2 form
// `v_cndmask_b32_e32 ..., vcc`, which gfx950 issues at ~23 cycles per wave instruction against
// ~4.5 for the VOP3 form with the mask in an SGPR pair (tools/exp/valu_probe2.hip), so the hot
// loops spell the VOP3 form out.  mask bit set -> t, clear -> f.
__device__ __forceinline__ float sel(unsigned long long mask, float t, float f) {
    float r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(mask));
    return r;
}
__device__ __forceinline__ uint32_t sel(unsigned long long mask, uint32_t t, uint32_t f) {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(mask));
    return r;
}
// IEEE minNum without the canonicalising v_max the compiler puts in front of fminf's v_min
__device__ __forceinline__ float vmin(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ unsigned long long lanes(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ uint32_t lanes_below(unsigned long long ballot) {  // popcount of lower lanes
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}
// any of three values NaN or +-Inf (v_cmp_class_f32: signalling NaN, quiet NaN, -Inf, +Inf)
__device__ __forceinline__ bool nonfinite3(float a, float b, float c) {
    constexpr int NAN_OR_INF = 0x1 | 0x2 | 0x4 | 0x200;
    return __builtin_amdgcn_classf(a, NAN_OR_INF) || __builtin_amdgcn_classf(b, NAN_OR_INF) || __builtin_amdgcn_classf(c, NAN_OR_INF);
}

// XCD-aware block -> tile map: consecutive tiles (which share splats) run on one XCD so their
// record gathers hit that XCD's L2.  Blocks are observed to be dealt round-robin to the 8 XCDs;
// the map is a speed choice only.  Returns -1 for the padding blocks.
__device__ inline int xcd_tile(int block, int tiles) {
    int chunk = (tiles + NUM_XCD - 1) / NUM_XCD;
    int t = (block % NUM_XCD) * chunk + block / NUM_XCD;
    return t < tiles ? t : -1;
}
inline __host__ int xcd_grid(int tiles) { return ((tiles + NUM_XCD - 1) / NUM_XCD) * NUM_XCD; }
// XCD of a tile when the scene is not uniform (tile_order_kernel): 4x4-tile blocks dealt round-robin, so that every XCD
// gets the same mix of dense and sparse image regions (the contiguous bands of xcd_tile leave the XCDs of the image
// centre with most of the work, and blocks are dealt to the XCDs in turn: the launch runs at the pace of the slowest)
__host__ __device__ inline int xcd_of_tile(int t, int gx) {
    const int tx = t % gx, ty = t / gx;
    return ((tx >> 2) + (ty >> 2) * ((gx + 3) >> 2)) % NUM_XCD;
}

// Conservative sub-tile culling.  A 16x16 tile is blended by four waves, one per 8x8-pixel
// quadrant (bit q = (y half << 1) | x half).  Bit q is CLEARED only when no pixel of the quadrant
// can pass the blend kernels' `alpha >= 1/255` test: the minimum of the quadratic form
// q(d) = -power(d) over the quadrant's (continuous) pixel box is bounded below, and the splat is
// dropped when o * exp(-qmin) is below 1/255 by a safety margin that dwarfs the rounding
// difference between this bound and the per-pixel evaluation.  Dropping such a splat cannot
// change any result (it would be skipped by every pixel anyway), so lists, n_contrib and images
// stay bit-identical to the un-culled semantics.  NaNs compare false -> kept.
struct SplatForm {
    float mx, my, a, b, c, thr;
    float vy, vx;  // minimiser slopes along an edge: dy* = vy * dx on a vertical edge, dx* = vx * dy on a horizontal one
    bool ok;       // finite and positive definite; anything else is simply kept everywhere
};
__device__ inline SplatForm splat_form(float4 r0, float4 r1) {
    SplatForm f;
    f.mx = r0.x; f.my = r0.y;
    f.a = -r0.z; f.b = -r0.w; f.c = -r1.x;  // q = a dx^2 + b dx dy + c dy^2, a,c > 0
    f.thr = __logf(255.0f * r1.y) + 0.01f;  // q above this -> alpha < 1/255 (with margin)
    f.ok = (f.a > 0.0f && f.c > 0.0f && 4.0f * f.a * f.c - f.b * f.b > 0.0f) && (f.mx - f.mx == 0.0f) &&
           (f.my - f.my == 0.0f) && (f.thr - f.thr == 0.0f);
    // one division per direction and Gaussian instead of one per edge: q is stationary at the minimiser, so
    // the last-bit difference to (-b * fix) / (2 k) moves the edge minimum by a second-order amount, far
    // inside the margins below
    f.vy = -f.b / (2.0f * f.c);
    f.vx = -f.b / (2.0f * f.a);
    return f;
}
// The four quadrants of a tile at once.  The exact minimum of q over each box, found with two edge minima per quadrant
// instead of four: q is convex with its minimiser at d = 0, so over a box that does not contain 0 the minimum lies on a
// face that is VISIBLE from 0 (from a point of any other face a step towards 0 stays inside the box and lowers q) --
// at most the vertical edge dx = cx and the horizontal edge dy = cy, where (cx, cy) = 0 clamped into the box
// (v_med3_f32).  A coordinate of 0 that already lies inside the box's range gives cx = 0: the "edge" dx = 0 is then just
// another line through the box (a valid upper bound of the minimum, equal to it when 0 is inside the box: q = 0), so no
// case distinction is left.  Everything that depends on one axis only is shared by the two quadrants of a row / column.
// The splat is kept when either candidate stays within the threshold plus the rounding margin of its own terms.
// S = edge of the four boxes in pixels: 8 = the quadrants of a tile (origin = the tile's), 4 = the 4x4-pixel sub-blocks of a
// quadrant (origin = the quadrant's; blend.hip packs four of them into a wave).  Bit (hy << 1) | hx.
template <int S>
__device__ inline uint32_t box_mask4(float4 r0, float4 r1, int box_x0, int box_y0) {
    const SplatForm f = splat_form(r0, r1);
    if (!f.ok) return 0xfu;
    const float x0 = (float)box_x0, y0 = (float)box_y0;
    float dxl[2], dxh[2], dyl[2], dyh[2];     // d = mean - pixel over the half's columns / rows (low, high end)
    float cx[2], cy[2], qx[2], qy[2], bcx[2], bcy[2], sy[2], sx[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        dxh[h] = f.mx - (x0 + (float)(S * h));
        dxl[h] = f.mx - (x0 + (float)(S * h + S - 1));
        dyh[h] = f.my - (y0 + (float)(S * h));
        dyl[h] = f.my - (y0 + (float)(S * h + S - 1));
        cx[h] = __builtin_amdgcn_fmed3f(0.0f, dxl[h], dxh[h]);
        cy[h] = __builtin_amdgcn_fmed3f(0.0f, dyl[h], dyh[h]);
        qx[h] = f.a * cx[h] * cx[h];          // the fixed coordinate's own term
        qy[h] = f.c * cy[h] * cy[h];
        bcx[h] = f.b * cx[h];
        bcy[h] = f.b * cy[h];
        sy[h] = f.vy * cx[h];                 // unclamped minimiser along the edge
        sx[h] = f.vx * cy[h];
    }
    uint32_t mask = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int hx = q & 1, hy = q >> 1;
        const float v = __builtin_amdgcn_fmed3f(sy[hx], dyl[hy], dyh[hy]);
        const float t1 = bcx[hx] * v, t2 = f.c * v * v;
        const float qv = qx[hx] + t1 + t2, magv = qx[hx] + fabsf(t1) + t2;
        const float u = __builtin_amdgcn_fmed3f(sx[hy], dxl[hx], dxh[hx]);
        const float s1 = bcy[hy] * u, s2 = f.a * u * u;
        const float qh = qy[hy] + s1 + s2, magh = qy[hy] + fabsf(s1) + s2;
        const bool far = qv > __builtin_fmaf(1.0e-5f, magv, f.thr) && qh > __builtin_fmaf(1.0e-5f, magh, f.thr);
        if (!far) mask |= 1u << q;
    }
    return mask;
}
__device__ inline uint32_t quadrant_mask(float4 r0, float4 r1, int tile_x0, int tile_y0) { return box_mask4<8>(r0, r1, tile_x0, tile_y0); }


// Several buffers cleared by ONE kernel launch (preprocess.hip).  hipMemsetAsync costs a 5 us fill kernel AND 8 - 11 us of
// idle stream time in front of it per call (profiles/r03x_step_gaps.txt): one per forward pass at cfg1, eighteen per
// tri-plane backward.  Pointers 4-byte aligned, sizes in bytes (multiples of 4).
struct ZeroList {
    static constexpr int MAX = 20;
    void* p[MAX];
    unsigned long long n[MAX];
    int count = 0;
    bool full() const { return count >= MAX; }
    // queue one buffer; a full list is launched first (on `st`) and restarted, so that no buffer is ever dropped
    void add(void* ptr, size_t bytes, hipStream_t st);
};
void launch_zero(const ZeroList& z, hipStream_t st);      // launches nothing for an empty list
void launch_zero_far_records(int64_t P, const GeomView& gv, GradRec* grad_rec, float* grad_z, hipStream_t st);
inline void ZeroList::add(void* ptr, size_t bytes, hipStream_t st) {
    if (!ptr || !bytes) return;
    if (full()) { launch_zero(*this, st); count = 0; }
    p[count] = ptr;
    n[count] = bytes;
    ++count;
}

// More than the default 64 KB of dynamic LDS for `kernel` on the current device (gfx950 has 160 KB per CU).  The attribute is
// per function and device: the largest grant of each pair is remembered, and the runtime is asked only for more.  A refused
// attribute shows up as the error of the launch that follows.  (capi.hip)
void allow_dynamic_lds(const void* kernel, size_t bytes);

// launchers of the rasterizer pipeline (preprocess.hip, binning.hip, blend.hip), orchestrated by capi.hip.  Every other
// operator family keeps its launches next to its entry points, in its own .hip file.
void launch_filter(int64_t P, const float* means3D, const float* scales, const float* rotations,
                   const float* cov3D, const KSettings& ks, int32_t* radii, hipStream_t st);
void launch_mark_visible(int64_t P, const float* means3D, const float* view, uint8_t* out, hipStream_t st);
void launch_preprocess(int64_t P, int M, const float* means3D, const float* scales, const float* rotations,
                       const float* cov3D, const float* opacities, const float* shs, const float* colors,
                       const KSettings& ks, const GeomView& gv, int32_t* radii, bool antialiased, hipStream_t st);
void launch_plan_scans(int64_t P, const KSettings& ks, const GeomView& gv, unsigned long long* mailbox,
                       unsigned long long seq, hipStream_t st);
void launch_scatter(int64_t P, const KSettings& ks, const GeomView& gv, const BinView& bv, unsigned long long cap_instances,
                    hipStream_t st);
void launch_tile_sort(const KSettings& ks, const GeomView& gv, const BinView& bv, int64_t max_tile_instances,
                      bool with_gm_index, hipStream_t st);
void launch_blend_forward(const KSettings& ks, const GeomView& gv, const BinView& bv, const ImgView& iv,
                          float* out_color, float* out_depth, float* out_alpha, bool longest_first, bool safe,
                          hipStream_t st);
void launch_blend_backward(const KSettings& ks, const GeomView& gv, const BinView& bv, const ImgView& iv,
                           const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha, GradRec* grad_rec,
                           float* grad_z, unsigned long long stamp, bool deep, bool flags, bool safe, hipStream_t st);
void launch_preprocess_backward(int64_t P, int M, const float* means3D, const float* scales,
                                const float* rotations, const float* cov3D, const float* shs,
                                const KSettings& ks, const int32_t* radii, const GeomView& gv,
                                const BinView& bv, const GradRec* grad_rec, const float* grad_z,
                                const unsigned long long* cut_key, unsigned long long stamp, bool deep, float* dL_dmeans3D,
                                float* dL_dmeans2D, float* dL_dcolors, float* dL_dsh, float* dL_dopacity,
                                float* dL_dscales, float* dL_drotations, float* dL_dcov3D, float* cam_partials,
                                bool antialiased, hipStream_t st);
// camera gradients (preprocess.hip): one 32-float row per preprocess-backward workgroup, summed by one more small kernel
size_t camera_partials_bytes(int64_t P);
void launch_camera_grad_finish(int64_t P, const float* cam_partials, float* dL_dview, float* dL_dproj, float* dL_dcampos,
                               hipStream_t st);

constexpr int NL_DP = 80;               // padded width of the BatchNorm-Linear's coefficient rows AND of a row of column statistics

}  // namespace scr
