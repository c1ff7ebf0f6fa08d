// splatco_amd/csrc/tsdf_sparse.hip -- the block-sparse TSDF volume: allocation of 8 x 8 x 8-node blocks where a depth map puts
// a surface, integration over the allocated blocks, marching tetrahedra across block boundaries (gfx950).
//
// The definition is include/splatco_tsdf_sparse.h's (tests/tsdf_sparse_ref.py restates the allocation rule in numpy float64).
// The per-node update and the lattice tables are tsdf_node.h's, shared with the dense family (tsdf.hip).
//
// Allocation.  One thread per pixel forms the world box of its frustum slab and stores 1 into every mark of its block range
// that is still 0: same-value stores, so the marks do not depend on timing.  compact.h then takes the marks that are 1, which
// yields the new keys in ascending order; the write kernel raises their marks to 2 and a merge kernel (one thread per old or
// new key, its position = own index + lower bound in the other list) writes the joined keys and slots.
//
// Integration.  One workgroup of 128 threads per allocated block; thread t owns the four x-adjacent nodes 4 t .. 4 t + 3 of the
// block's row, so every access of tsdf, weight and the three colour rows is one 16-byte load or store (a row is 2 KiB and
// 16-byte aligned).  Before anything is loaded the workgroup bounds zc, and where the block is wholly in front, u and v, of
// all its nodes: every operation of steps 1 and 2 is monotone in each lattice coordinate, so the bounds are taken at the
// block's extreme coordinates with the nodes' own operations and hold for the computed values, not only the exact ones.
//
// Extraction.  The two compactions of tsdf.hip over 3584 Nb edge ids and 6144 Nb triangle slots; a node at local coordinates
// -1 .. 8 of a block is reached through the [Nb, 27] table of neighbour ranks.  compact.h counts below 2^31 items, so a pass
// covers the blocks of rank first .. first + count - 1 (its functor adds the pass's first item to the item index); ids stay
// global, and the face pass searches the joined id list of all vertex passes.
#include "capi.h"
#include "tsdf_node.h"
#include "../../include/splatco_tsdf_sparse.h"

namespace scr {

constexpr int TSS_B = SCR_TSDFS_BLOCK;
constexpr int TSS_NODES = TSS_B * TSS_B * TSS_B;        // 512
constexpr int TSS_EDGES = 7 * TSS_NODES;                // 3584 edge ids per block
constexpr int TSS_SLOTS = 12 * TSS_NODES;               // 6144 triangle slots per block
constexpr int TSS_THREADS = TSS_NODES / 4;              // 128: four nodes per thread
static_assert(TSS_B == 8, "the local index arithmetic below is written for 8-node blocks");

struct TssVol {
    int nx, ny, nz, nbx, nby, nbz;
    double lox, loy, loz, h, trunc, max_weight;
};

// ------------------------------------------------------------------ allocation
__global__ void __launch_bounds__(256) tsdfs_mark_kernel(TssVol g, scr_tsdfs_view sv, uint8_t* marks) {
    const scr_tsdf_view& V = sv.view;
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (int64_t)V.H * V.W) return;
    const int py = (int)(pix / V.W), px = (int)(pix - (int64_t)py * V.W);
    const float D = V.depth[pix], A = V.alpha[pix];
    bool ok = ts_finite(D) && ts_finite(A) && A >= V.min_alpha && D > 0.0f;
    if (V.mask_kind == 1) ok = ok && ((const float*)V.mask)[pix] > 0.0f;
    if (V.mask_kind == 2) ok = ok && ((const uint8_t*)V.mask)[pix] != 0;
    if (!ok) return;
    const double z = (double)(D / A);
    const double z0 = fmax(z - g.trunc, V.near), z1 = z + g.trunc;
    if (!(z0 <= z1)) return;
    const double* C = sv.c2w;
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const double zc = (c & 4) ? z1 : z0;
        const double xc = ((double)(px + (c & 1)) - V.cx) / V.fx * zc, yc = ((double)(py + ((c >> 1) & 1)) - V.cy) / V.fy * zc;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double w = ((C[4 * a] * xc + C[4 * a + 1] * yc) + C[4 * a + 2] * zc) + C[4 * a + 3];
            mn[a] = fmin(mn[a], w);
            mx[a] = fmax(mx[a], w);
        }
    }
    const double pad = g.h * 0.125, side = 8.0 * g.h;
    const double lo[3] = {g.lox, g.loy, g.loz};
    const int nb[3] = {g.nbx, g.nby, g.nbz};
    int b0[3], b1[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double f0 = floor(((mn[a] - pad) - lo[a]) / side), f1 = floor(((mx[a] + pad) - lo[a]) / side);
        if (!(f1 >= 0.0) || !(f0 <= (double)(nb[a] - 1)) || !(f0 <= f1)) return;         // empty, or not a number
        b0[a] = f0 > 0.0 ? (int)f0 : 0;
        b1[a] = f1 < (double)(nb[a] - 1) ? (int)f1 : nb[a] - 1;
    }
    for (int bk = b0[2]; bk <= b1[2]; ++bk)
        for (int bj = b0[1]; bj <= b1[1]; ++bj)
            for (int bi = b0[0]; bi <= b1[0]; ++bi) {
                uint8_t* m = marks + (((int64_t)bk * g.nby + bj) * g.nbx + bi);
                if (*m == 0) *m = 1;                    // every writer stores the same value over the same value
            }
}

// a virtual block is kept where a view touched it and it is not allocated yet
struct KeepMark {
    struct Operand { uint8_t m; };
    const uint8_t* marks;
    __device__ Operand load(int64_t c) const { return {marks[c]}; }
    __device__ bool keep(const Operand& v, int64_t) const { return v.m == 1; }
};

__global__ void __launch_bounds__(COMPACT_THREADS)
tsdfs_key_write_kernel(int64_t items, KeepMark km, const uint32_t* __restrict__ wg_offset, int64_t nnew, uint8_t* marks, int32_t* __restrict__ new_keys) {
    const CompactRank<KeepMark> c = compact_rank(items, km, wg_offset);
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) {
        if (!c.keep[r] || (int64_t)c.pos[r] >= nnew) continue;
        const int64_t key = compact_item(r);
        new_keys[c.pos[r]] = (int32_t)key;
        marks[key] = 2;
    }
}

__device__ __forceinline__ int64_t tss_lower_bound(const int32_t* __restrict__ a, int64_t n, int32_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// two ascending lists of distinct keys into one: an element's position is its own index plus its lower bound in the other list
__global__ void __launch_bounds__(256)
tsdfs_merge_kernel(int64_t nb_old, const int32_t* __restrict__ keys_old, const int32_t* __restrict__ slots_old, int64_t nnew,
                   const int32_t* __restrict__ new_keys, int32_t* __restrict__ keys, int32_t* __restrict__ slots) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nb_old + nnew) return;
    if (t < nb_old) {
        const int32_t key = keys_old[t];
        const int64_t pos = t + tss_lower_bound(new_keys, nnew, key);
        keys[pos] = key;
        slots[pos] = slots_old[t];
    } else {
        const int64_t j = t - nb_old;
        const int32_t key = new_keys[j];
        const int64_t pos = j + tss_lower_bound(keys_old, nb_old, key);
        keys[pos] = key;
        slots[pos] = (int32_t)(nb_old + j);
    }
}

__global__ void __launch_bounds__(TSS_THREADS)
tsdfs_init_kernel(int64_t first, float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color) {
    const size_t row = (size_t)first + blockIdx.x, at = row * TSS_NODES + 4 * threadIdx.x;
    *(float4*)(tsdf + at) = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    *(float4*)(weight + at) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (color) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) *(float4*)(color + (row * 3 + ch) * TSS_NODES + 4 * threadIdx.x) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// ------------------------------------------------------------------ integration
// a bound of row m of w2c over the box [x0, x1] x [y0, y1] x [z0, z1] of node positions, made of the nodes' own operations:
// fl(m x) is monotone in x, fl(a + b) in a and in b, so the extreme of the COMPUTED row is the row computed at a corner
__device__ __forceinline__ double tss_row_bound(const double* m, bool upper, double x0, double x1, double y0, double y1, double z0, double z1) {
    const double x = (m[0] >= 0.0) == upper ? x1 : x0, y = (m[1] >= 0.0) == upper ? y1 : y0, z = (m[2] >= 0.0) == upper ? z1 : z0;
    return ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
}

template <bool COLOR>
__global__ void __launch_bounds__(TSS_THREADS)
tsdfs_integrate_kernel(TssVol g, scr_tsdf_view V, const int32_t* __restrict__ keys, const int32_t* __restrict__ slots,
                       float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color) {
    const int key = keys[blockIdx.x];
    const int bi = key % g.nbx, rest = key / g.nbx, bj = rest % g.nby, bk = rest / g.nby;
    const int i0 = bi * TSS_B, j0 = bj * TSS_B, k0 = bk * TSS_B;
    {   // the whole block behind `near`, or outside the image on one side: no node of it would pass steps 1 and 2
        const double x0 = g.lox + g.h * (double)i0, x1 = g.lox + g.h * (double)min(i0 + TSS_B - 1, g.nx - 1);
        const double y0 = g.loy + g.h * (double)j0, y1 = g.loy + g.h * (double)min(j0 + TSS_B - 1, g.ny - 1);
        const double z0 = g.loz + g.h * (double)k0, z1 = g.loz + g.h * (double)min(k0 + TSS_B - 1, g.nz - 1);
        const double zhi = tss_row_bound(V.w2c + 8, true, x0, x1, y0, y1, z0, z1);
        if (zhi <= V.near) return;
        const double zlo = tss_row_bound(V.w2c + 8, false, x0, x1, y0, y1, z0, z1);
        if (zlo > V.near) {                             // every zc is in [zlo, zhi], positive: t / zc is monotone in t and in zc
            const double tlo = V.fx * tss_row_bound(V.w2c, false, x0, x1, y0, y1, z0, z1), thi = V.fx * tss_row_bound(V.w2c, true, x0, x1, y0, y1, z0, z1);
            if (fmax(thi / zlo, thi / zhi) + V.cx < 0.0) return;
            if (fmin(tlo / zlo, tlo / zhi) + V.cx >= (double)V.W) return;
            const double slo = V.fy * tss_row_bound(V.w2c + 4, false, x0, x1, y0, y1, z0, z1), shi = V.fy * tss_row_bound(V.w2c + 4, true, x0, x1, y0, y1, z0, z1);
            if (fmax(shi / zlo, shi / zhi) + V.cy < 0.0) return;
            if (fmin(slo / zlo, slo / zhi) + V.cy >= (double)V.H) return;
        }
    }
    const int l0 = 4 * threadIdx.x, li = l0 & 7, lj = (l0 >> 3) & 7, lk = l0 >> 6;
    const int ci = i0 + li, cj = j0 + lj, ck = k0 + lk;
    if (ci >= g.nx || cj >= g.ny || ck >= g.nz) return;                 // the thread's four nodes lie outside dims
    const size_t row = (size_t)slots[blockIdx.x];
    float4* ps = (float4*)(tsdf + row * TSS_NODES + l0);
    float4* pw = (float4*)(weight + row * TSS_NODES + l0);
    float4* pc = COLOR ? (float4*)(color + row * 3 * TSS_NODES + l0) : nullptr;
    const size_t HW = (size_t)V.H * V.W;
    float s[4], w[4], c0[4], c1[4], c2[4];
    { const float4 t = *ps; s[0] = t.x; s[1] = t.y; s[2] = t.z; s[3] = t.w; }
    { const float4 t = *pw; w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w; }
    if (COLOR) {
        { const float4 t = pc[0]; c0[0] = t.x; c0[1] = t.y; c0[2] = t.z; c0[3] = t.w; }
        { const float4 t = pc[TSS_NODES / 4]; c1[0] = t.x; c1[1] = t.y; c1[2] = t.z; c1[3] = t.w; }
        { const float4 t = pc[2 * TSS_NODES / 4]; c2[0] = t.x; c2[1] = t.y; c2[2] = t.z; c2[3] = t.w; }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (ci + r < g.nx) ts_node_update<COLOR>(g, V, V.w2c, HW, ci + r, cj, ck, s[r], w[r], c0[r], c1[r], c2[r]);     // tsdf_node.h
    *ps = make_float4(s[0], s[1], s[2], s[3]);
    *pw = make_float4(w[0], w[1], w[2], w[3]);
    if (COLOR) {
        pc[0] = make_float4(c0[0], c0[1], c0[2], c0[3]);
        pc[TSS_NODES / 4] = make_float4(c1[0], c1[1], c1[2], c1[3]);
        pc[2 * TSS_NODES / 4] = make_float4(c2[0], c2[1], c2[2], c2[3]);
    }
}

// ------------------------------------------------------------------ extraction
__global__ void __launch_bounds__(256)
tsdfs_neighbor_kernel(int nbx, int nby, int nbz, int64_t nb, const int32_t* __restrict__ keys, int32_t* __restrict__ table) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= 27 * nb) return;
    const int64_t r = t / 27;
    const int n = (int)(t - 27 * r);
    const int key = keys[r];
    const int bi = key % nbx + n % 3 - 1, rest = key / nbx, bj = rest % nby + (n / 3) % 3 - 1, bk = rest / nby + n / 9 - 1;
    int32_t rank = -1;
    if (bi >= 0 && bj >= 0 && bk >= 0 && bi < nbx && bj < nby && bk < nbz) {
        const int32_t want = (int32_t)(((int64_t)bk * nby + bj) * nbx + bi);
        const int64_t at = tss_lower_bound(keys, nb, want);
        if (at < nb && keys[at] == want) rank = (int32_t)at;
    }
    table[t] = rank;
}

struct TssGrid {
    int nx, ny, nz, nbx, nby;
    const int32_t* __restrict__ keys;
    const int32_t* __restrict__ slots;
    const int32_t* __restrict__ table;
    const float* __restrict__ tsdf;
    const float* __restrict__ weight;
    float min_weight;
    // the first node of the block of rank r
    __device__ __forceinline__ void origin(int64_t r, int& i0, int& j0, int& k0) const {
        const int key = keys[r], rest = key / nbx;
        i0 = (key % nbx) * TSS_B; j0 = (rest % nby) * TSS_B; k0 = (rest / nby) * TSS_B;
    }
    // the node at local coordinates -1 .. 8 of block r: the rank of the block that stores it (-1: not allocated) and its l
    __device__ __forceinline__ int32_t owner(int64_t r, int li, int lj, int lk, int& l) const {
        l = ((lk & 7) * 8 + (lj & 7)) * 8 + (li & 7);
        return table[27 * r + (((lk >> 3) + 1) * 3 + ((lj >> 3) + 1)) * 3 + ((li >> 3) + 1)];
    }
    __device__ __forceinline__ size_t at(int32_t rank, int l) const { return (size_t)slots[rank] * TSS_NODES + l; }
    // the cube with its corner at local (ci, cj, ck), -1 .. 7, of block r (first node i0, j0, k0) is valid
    __device__ bool cube_valid(int64_t r, int i0, int j0, int k0, int ci, int cj, int ck) const {
        if (i0 + ci < 0 || j0 + cj < 0 || k0 + ck < 0 || i0 + ci + 1 >= nx || j0 + cj + 1 >= ny || k0 + ck + 1 >= nz) return false;
        for (int code = 0; code < 8; ++code) {
            int l;
            const int32_t rank = owner(r, ci + (code & 1), cj + ((code >> 1) & 1), ck + ((code >> 2) & 1), l);
            if (rank < 0 || !(weight[at(rank, l)] > min_weight)) return false;
        }
        return true;
    }
};

struct TssEdge { int64_t r; int l, li, lj, lk, dir, code; };
__device__ __forceinline__ TssEdge tss_edge(int64_t e) {
    TssEdge o;
    o.r = e / TSS_EDGES;
    const int rem = (int)(e - o.r * TSS_EDGES);
    o.l = rem / 7;
    o.dir = rem - 7 * o.l;
    o.code = ts_dir_code(o.dir);
    o.li = o.l & 7; o.lj = (o.l >> 3) & 7; o.lk = o.l >> 6;
    return o;
}

// an edge id is kept where the edge carries a vertex
struct KeepEdgeS {
    struct Operand { float sa, sb; };
    TssGrid g;
    int64_t base;                                       // the first edge id of this pass: items count from it
    // the edge's far node: the rank of its block and its l, or -1 where it is outside dims or not allocated
    __device__ __forceinline__ int32_t far_node(const TssEdge& ed, int& l) const {
        int i0, j0, k0;
        g.origin(ed.r, i0, j0, k0);
        const int bi = ed.li + (ed.code & 1), bj = ed.lj + ((ed.code >> 1) & 1), bk = ed.lk + ((ed.code >> 2) & 1);
        const int32_t rank = g.owner(ed.r, bi, bj, bk, l);
        return (i0 + bi < g.nx && j0 + bj < g.ny && k0 + bk < g.nz) ? rank : -1;
    }
    __device__ Operand load(int64_t c) const {
        const TssEdge ed = tss_edge(c + base);
        const float sa = g.tsdf[g.at((int32_t)ed.r, ed.l)];
        int l;
        const int32_t rank = far_node(ed, l);
        return {sa, rank >= 0 ? g.tsdf[g.at(rank, l)] : sa};                       // no far node: no sign change
    }
    __device__ bool keep(const Operand& v, int64_t i) const {
        if ((v.sa < 0.0f) == (v.sb < 0.0f)) return false;
        const TssEdge ed = tss_edge(i + base);
        int i0, j0, k0;
        g.origin(ed.r, i0, j0, k0);
        // the cubes around the edge: the corner may step back along every axis the edge does not run along
        for (int back = 0; back < 8; ++back) {
            if (back & ed.code) continue;
            if (g.cube_valid(ed.r, i0, j0, k0, ed.li - (back & 1), ed.lj - ((back >> 1) & 1), ed.lk - ((back >> 2) & 1))) return true;
        }
        return false;
    }
};

struct TssGeo { double lox, loy, loz, h; };

__global__ void __launch_bounds__(COMPACT_THREADS)
tsdfs_vertex_write_kernel(int64_t items, KeepEdgeS ke, const uint32_t* __restrict__ wg_offset, TssGeo geo, const float* __restrict__ color,
                          int64_t nv, int64_t* __restrict__ ids, float* __restrict__ verts, float* __restrict__ cols) {
    const CompactRank<KeepEdgeS> c = compact_rank(items, ke, wg_offset);
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) {
        if (!c.keep[r] || (int64_t)c.pos[r] >= nv) continue;
        const int64_t e = compact_item(r) + ke.base;
        const TssEdge ed = tss_edge(e);
        int i0, j0, k0, lb;
        ke.g.origin(ed.r, i0, j0, k0);
        const int32_t rb = ke.far_node(ed, lb);         // >= 0: the edge's nodes differ
        const double sa = (double)c.v[r].sa, sb = (double)c.v[r].sb;
        const double t = sa / (sa - sb);
        const size_t o = 3 * (size_t)c.pos[r];
        ids[c.pos[r]] = e;
        const int ia = i0 + ed.li, ja = j0 + ed.lj, ka = k0 + ed.lk;
        const double ax = geo.lox + geo.h * (double)ia, ay = geo.loy + geo.h * (double)ja, az = geo.loz + geo.h * (double)ka;
        const double bx = geo.lox + geo.h * (double)(ia + (ed.code & 1)), by = geo.loy + geo.h * (double)(ja + ((ed.code >> 1) & 1)),
                     bz = geo.loz + geo.h * (double)(ka + ((ed.code >> 2) & 1));
        verts[o] = (float)(ax + (bx - ax) * t);
        verts[o + 1] = (float)(ay + (by - ay) * t);
        verts[o + 2] = (float)(az + (bz - az) * t);
        if (color) {
            const size_t pa = (size_t)ke.g.slots[ed.r] * 3 * TSS_NODES + ed.l, pb = (size_t)ke.g.slots[rb >= 0 ? rb : (int32_t)ed.r] * 3 * TSS_NODES + lb;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double ca = (double)color[pa + (size_t)ch * TSS_NODES], cb = (double)color[pb + (size_t)ch * TSS_NODES];
                cols[o + ch] = (float)(ca + (cb - ca) * t);
            }
        }
    }
}

struct TssSlot { int64_t r; int li, lj, lk, q, tri; };
__device__ __forceinline__ TssSlot tss_slot(int64_t it) {
    TssSlot o;
    o.r = it / TSS_SLOTS;
    const int rem = (int)(it - o.r * TSS_SLOTS), l = rem / 12, s = rem - 12 * l;
    o.q = s >> 1;
    o.tri = s & 1;
    o.li = l & 7; o.lj = (l >> 3) & 7; o.lk = l >> 6;
    return o;
}

// a triangle slot (cube, tetrahedron, 0 / 1) is kept where the tetrahedron is cut and its cube is valid
struct KeepSlotS {
    struct Operand { uint32_t mask; };                  // bit x: local node x of the tetrahedron is inside
    TssGrid g;
    int64_t base;                                       // the first slot of this pass, a multiple of 6144
    __device__ Operand load(int64_t it) const {
        const TssSlot sl = tss_slot(it + base);
        uint32_t m = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int code = ts_tet_code(sl.q, x);
            int l;
            const int32_t rank = g.owner(sl.r, sl.li + (code & 1), sl.lj + ((code >> 1) & 1), sl.lk + ((code >> 2) & 1), l);
            m |= (rank >= 0 && g.tsdf[g.at(rank, l)] < 0.0f ? 1u : 0u) << x;         // a missing node: the cube is not valid
        }
        return {m};
    }
    __device__ bool keep(const Operand& v, int64_t it) const {
        const int cnt = __builtin_popcount(v.mask);
        if (cnt == 0 || cnt == 4 || ((it & 1) && cnt != 2)) return false;      // 12 | it - slot: the slot's parity is it's
        const TssSlot sl = tss_slot(it + base);
        int i0, j0, k0;
        g.origin(sl.r, i0, j0, k0);
        return g.cube_valid(sl.r, i0, j0, k0, sl.li, sl.lj, sl.lk);
    }
};

// position of edge id `key` in the sorted list (it is there: the two compactions read the same volume)
__device__ __forceinline__ int32_t tss_find(const int64_t* __restrict__ ids, int64_t nv, int64_t key) {
    int64_t lo = 0, hi = nv;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ids[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (int32_t)min(lo, nv - 1);
}

__global__ void __launch_bounds__(COMPACT_THREADS)
tsdfs_face_write_kernel(int64_t items, KeepSlotS ks, const uint32_t* __restrict__ wg_offset, int64_t nv, const int64_t* __restrict__ ids,
                        int64_t nf, int32_t* __restrict__ faces) {
    const CompactRank<KeepSlotS> c = compact_rank(items, ks, wg_offset);
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) {
        if (!c.keep[r] || (int64_t)c.pos[r] >= nf) continue;
        const TssSlot sl = tss_slot(compact_item(r) + ks.base);
        int ex[3], ey[3];                               // the triangle's edges as pairs of local nodes
        ts_triangle_edges(c.v[r].mask, sl.q, sl.tri, ex, ey);
        const size_t o = 3 * (size_t)c.pos[r];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int cx = ts_tet_code(sl.q, min(ex[e], ey[e])), cy = ts_tet_code(sl.q, max(ex[e], ey[e]));
            int l;
            const int32_t rank = ks.g.owner(sl.r, sl.li + (cx & 1), sl.lj + ((cx >> 1) & 1), sl.lk + ((cx >> 2) & 1), l);
            const int64_t eid = (int64_t)TSS_EDGES * (rank >= 0 ? rank : 0) + 7 * l + ts_code_dir(cx ^ cy);      // the cube is valid: rank >= 0
            faces[o + e] = tss_find(ids, nv, eid);
        }
    }
}

// ------------------------------------------------------------------ host checks
static bool tss_fin(double x) { return x == x && x - x == 0.0; }
static bool tss_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int tss_dims(const char* who, int nx, int ny, int nz, TssVol* g) {
    if (nx < 2 || ny < 2 || nz < 2) return fail("%s: dims (%d, %d, %d): every dimension must be >= 2", who, nx, ny, nz);
    if (nx >= (1 << 20) || ny >= (1 << 20) || nz >= (1 << 20)) return fail("%s: dims (%d, %d, %d): every dimension must be below 2^20", who, nx, ny, nz);
    const int64_t nbx = (nx + TSS_B - 1) / TSS_B, nby = (ny + TSS_B - 1) / TSS_B, nbz = (nz + TSS_B - 1) / TSS_B;
    if (nbx * nby * nbz >= (1ll << 31)) return fail("%s: dims (%d, %d, %d): the block count %lld is not below 2^31", who, nx, ny, nz, (long long)(nbx * nby * nbz));
    if (g) {
        g->nx = nx; g->ny = ny; g->nz = nz;
        g->nbx = (int)nbx; g->nby = (int)nby; g->nbz = (int)nbz;
    }
    return 0;
}
static int64_t tss_virtual_blocks(const TssVol& g) { return (int64_t)g.nbx * g.nby * g.nbz; }

static int tss_geometry(const char* who, const float* lo_host, float h, double trunc, TssVol* g) {
    if (!(h > 0.0f) || !tss_fin(h)) return fail("%s: voxel size h = %g must be finite and > 0", who, (double)h);
    if (!(trunc > 0.0) || !tss_fin(trunc)) return fail("%s: trunc = %g must be finite and > 0", who, trunc);
    if (!lo_host) return fail("%s: lo_host is NULL", who);
    if (!tss_fin(lo_host[0]) || !tss_fin(lo_host[1]) || !tss_fin(lo_host[2])) return fail("%s: lo is not finite", who);
    g->lox = lo_host[0]; g->loy = lo_host[1]; g->loz = lo_host[2];
    g->h = h; g->trunc = trunc; g->max_weight = 0.0;
    return 0;
}

// the scalars of a view, then (pointers = true) its pointers
static int tss_view(const char* who, const scr_tsdfs_view* sv, bool pointers, bool has_color) {
    const scr_tsdf_view& v = sv->view;
    if (!pointers) {
        if (v.H < 1 || v.W < 1) return fail("%s: H = %d, W = %d must be >= 1", who, v.H, v.W);
        if ((int64_t)v.H * v.W >= (1ll << 31)) return fail("%s: H W is not below 2^31", who);
        if (!(v.fx > 0.0) || !(v.fy > 0.0) || !tss_fin(v.fx) || !tss_fin(v.fy)) return fail("%s: fx, fy must be finite and > 0", who);
        if (!tss_fin(v.cx) || !tss_fin(v.cy)) return fail("%s: cx, cy must be finite", who);
        for (int m = 0; m < 12; ++m)
            if (!tss_fin(v.w2c[m])) return fail("%s: w2c is not finite", who);
        for (int m = 0; m < 12; ++m)
            if (!tss_fin(sv->c2w[m])) return fail("%s: c2w is not finite", who);
        if (!(v.near >= 0.0) || !tss_fin(v.near)) return fail("%s: near = %g must be finite and >= 0", who, v.near);
        if (!(v.min_alpha >= 0.0f) || !tss_fin(v.min_alpha)) return fail("%s: min_alpha must be finite and >= 0", who);
        if (v.mask_kind < 0 || v.mask_kind > 2) return fail("%s: mask_kind %d is not 0, 1 or 2", who, v.mask_kind);
        return 0;
    }
    if (!v.depth || !v.alpha) return fail("%s: NULL map", who);
    if (v.mask_kind != 0 && !v.mask) return fail("%s: mask is NULL with mask_kind %d", who, v.mask_kind);
    if (v.image && !has_color) return fail("%s: an image, but the volume has no colour", who);
    return 0;
}

static int tss_count(const char* who, const TssVol& g, int64_t nb) {
    if (nb < 0 || nb > tss_virtual_blocks(g)) return fail("%s: nb = %lld is not in 0 .. %lld", who, (long long)nb, (long long)tss_virtual_blocks(g));
    return 0;
}
static int tss_extract_count(const char* who, const TssVol& g, int64_t nb, int64_t first, int64_t count) {
    if (tss_count(who, g, nb)) return 1;
    if (first < 0 || count < 0 || first + count > nb) return fail("%s: blocks %lld + %lld are not within 0 .. nb = %lld", who, (long long)first, (long long)count, (long long)nb);
    if ((int64_t)TSS_SLOTS * count >= (1ll << 31)) return fail("%s: 6144 count = %lld triangle slots are not below 2^31", who, (long long)(TSS_SLOTS * count));
    return 0;
}

}  // namespace scr

using namespace scr;

extern "C" {

int scr_tsdfs_abi_version(void) { return SCR_TSDFS_ABI_VERSION; }

size_t scr_tsdfs_alloc_scratch_bytes(int32_t nx, int32_t ny, int32_t nz) {
    TssVol g;
    if (nx < 2 || ny < 2 || nz < 2 || nx >= (1 << 20) || ny >= (1 << 20) || nz >= (1 << 20)) return 256;
    g.nbx = (nx + TSS_B - 1) / TSS_B; g.nby = (ny + TSS_B - 1) / TSS_B; g.nbz = (nz + TSS_B - 1) / TSS_B;
    if (tss_virtual_blocks(g) >= (1ll << 31)) return 256;
    return compact_scratch_bytes(tss_virtual_blocks(g));
}

int scr_tsdfs_alloc_plan(int32_t nx, int32_t ny, int32_t nz, const float* lo_host, float h, double trunc,
                         const scr_tsdfs_view* view_host, uint8_t* marks, void* scratch, int64_t* count_host, void* stream) {
    SCR_MARK_FN;
    if (!count_host) return fail("%s: count_host is NULL", __func__);
    *count_host = 0;
    TssVol g;
    if (tss_dims(__func__, nx, ny, nz, &g) || tss_geometry(__func__, lo_host, h, trunc, &g)) return 1;
    if (!view_host) return fail("%s: view_host is NULL", __func__);
    if (tss_view(__func__, view_host, false, true)) return 1;
    if (!marks || !scratch) return fail("%s: NULL argument", __func__);
    if (tss_view(__func__, view_host, true, true)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t pixels = (int64_t)view_host->view.H * view_host->view.W;
    tsdfs_mark_kernel<<<(uint32_t)((pixels + 255) / 256), 256, 0, st>>>(g, *view_host, marks);
    CHECK_LAUNCH("tsdfs_mark_kernel", 0, st);
    const int64_t items = tss_virtual_blocks(g);
    const KeepMark km{marks};
    return compact_plan("compact_count_kernel<KeepMark>", items, scratch, count_host, st,
                        [&](const CompactScratch& s, unsigned long long* mb, unsigned long long seq) {
                            launch_compact_count(items, km, s, mb, seq, st);
                        });
}

int scr_tsdfs_alloc_run(int32_t nx, int32_t ny, int32_t nz, uint8_t* marks, const void* scratch, int64_t nb_old,
                        const int32_t* keys_old, const int32_t* slots_old, int64_t nnew, int32_t* new_keys, int32_t* keys,
                        int32_t* slots, void* stream) {
    SCR_MARK_FN;
    TssVol g;
    if (tss_dims(__func__, nx, ny, nz, &g) || tss_count(__func__, g, nb_old)) return 1;
    if (nnew < 0 || nb_old + nnew > tss_virtual_blocks(g)) return fail("%s: nnew = %lld with nb_old = %lld is not in 0 .. the block count", __func__, (long long)nnew, (long long)nb_old);
    if (nnew == 0) return 0;
    if (!marks || !scratch || !new_keys || !keys || !slots) return fail("%s: NULL argument", __func__);
    if (nb_old > 0 && (!keys_old || !slots_old)) return fail("%s: NULL old lists with nb_old = %lld", __func__, (long long)nb_old);
    hipStream_t st = (hipStream_t)stream;
    const int64_t items = tss_virtual_blocks(g);
    const KeepMark km{marks};
    tsdfs_key_write_kernel<<<(uint32_t)compact_nwg(items), COMPACT_THREADS, 0, st>>>(items, km, (const uint32_t*)scratch, nnew, marks, new_keys);
    CHECK_LAUNCH("tsdfs_key_write_kernel", 0, st);
    tsdfs_merge_kernel<<<(uint32_t)((nb_old + nnew + 255) / 256), 256, 0, st>>>(nb_old, keys_old, slots_old, nnew, new_keys, keys, slots);
    CHECK_LAUNCH("tsdfs_merge_kernel", 0, st);
    return 0;
}

int scr_tsdfs_init_blocks(int64_t first, int64_t count, float* tsdf, float* weight, float* color, void* stream) {
    SCR_MARK_FN;
    if (first < 0 || count < 0 || first + count >= (1ll << 31)) return fail("%s: rows %lld + %lld are not in 0 .. 2^31 - 1", __func__, (long long)first, (long long)count);
    if (count == 0) return 0;
    if (!tsdf || !weight) return fail("%s: NULL volume", __func__);
    if (!tss_al16(tsdf) || !tss_al16(weight) || !tss_al16(color)) return fail("%s: the block storage is not 16-byte aligned", __func__);
    hipStream_t st = (hipStream_t)stream;
    tsdfs_init_kernel<<<(uint32_t)count, TSS_THREADS, 0, st>>>(first, tsdf, weight, color);
    CHECK_LAUNCH("tsdfs_init_kernel", 0, st);
    return 0;
}

int scr_tsdfs_integrate(int32_t nx, int32_t ny, int32_t nz, const float* lo_host, float h, double trunc, float max_weight, int64_t nb,
                        const int32_t* keys, const int32_t* slots, float* tsdf, float* weight, float* color,
                        const scr_tsdfs_view* view_host, void* stream) {
    SCR_MARK_FN;
    TssVol g;
    if (tss_dims(__func__, nx, ny, nz, &g) || tss_geometry(__func__, lo_host, h, trunc, &g)) return 1;
    if (!(max_weight > 0.0f) || !tss_fin(max_weight)) return fail("%s: max_weight = %g must be finite and > 0", __func__, (double)max_weight);
    g.max_weight = max_weight;
    if (tss_count(__func__, g, nb)) return 1;
    if (!view_host) return fail("%s: view_host is NULL", __func__);
    if (tss_view(__func__, view_host, false, color != nullptr)) return 1;
    if (nb == 0) return 0;
    if (!keys || !slots || !tsdf || !weight) return fail("%s: NULL volume", __func__);
    if (!tss_al16(tsdf) || !tss_al16(weight) || !tss_al16(color)) return fail("%s: the block storage is not 16-byte aligned", __func__);
    if (tss_view(__func__, view_host, true, color != nullptr)) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (color) tsdfs_integrate_kernel<true><<<(uint32_t)nb, TSS_THREADS, 0, st>>>(g, view_host->view, keys, slots, tsdf, weight, color);
    else tsdfs_integrate_kernel<false><<<(uint32_t)nb, TSS_THREADS, 0, st>>>(g, view_host->view, keys, slots, tsdf, weight, nullptr);
    CHECK_LAUNCH("tsdfs_integrate_kernel", 0, st);
    return 0;
}

int scr_tsdfs_neighbors(int32_t nx, int32_t ny, int32_t nz, int64_t nb, const int32_t* keys, int32_t* table, void* stream) {
    SCR_MARK_FN;
    TssVol g;
    if (tss_dims(__func__, nx, ny, nz, &g) || tss_count(__func__, g, nb)) return 1;
    if (nb == 0) return 0;
    if (!keys || !table) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    tsdfs_neighbor_kernel<<<(uint32_t)((27 * nb + 255) / 256), 256, 0, st>>>(g.nbx, g.nby, g.nbz, nb, keys, table);
    CHECK_LAUNCH("tsdfs_neighbor_kernel", 0, st);
    return 0;
}

size_t scr_tsdfs_extract_scratch_bytes(int64_t count) {
    if (count < 1 || (int64_t)TSS_SLOTS * count >= (1ll << 31)) return 256;
    return compact_scratch_bytes((int64_t)TSS_SLOTS * count);
}

int scr_tsdfs_extract_vertices_plan(int32_t nx, int32_t ny, int32_t nz, int64_t nb, int64_t first, int64_t count, const int32_t* keys,
                                    const int32_t* slots, const int32_t* table, const float* tsdf, const float* weight,
                                    float min_weight, void* scratch, int64_t* count_host, void* stream) {
    SCR_MARK_FN;
    if (!count_host) return fail("%s: count_host is NULL", __func__);
    *count_host = 0;
    TssVol g;
    if (tss_dims(__func__, nx, ny, nz, &g) || tss_extract_count(__func__, g, nb, first, count)) return 1;
    if (min_weight != min_weight) return fail("%s: min_weight is NaN", __func__);
    if (count == 0) return 0;
    if (!keys || !slots || !table || !tsdf || !weight || !scratch) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    const int64_t items = (int64_t)TSS_EDGES * count;
    const KeepEdgeS ke{TssGrid{nx, ny, nz, g.nbx, g.nby, keys, slots, table, tsdf, weight, min_weight}, (int64_t)TSS_EDGES * first};
    return compact_plan("compact_count_kernel<KeepEdgeS>", items, scratch, count_host, st,
                        [&](const CompactScratch& s, unsigned long long* mb, unsigned long long seq) {
                            launch_compact_count(items, ke, s, mb, seq, st);
                        });
}

int scr_tsdfs_extract_vertices_run(int32_t nx, int32_t ny, int32_t nz, const float* lo_host, float h, int64_t nb, int64_t first,
                                   int64_t count, const int32_t* keys, const int32_t* slots, const int32_t* table, const float* tsdf,
                                   const float* weight, const float* color, float min_weight, const void* scratch, int64_t nv,
                                   int64_t* edge_ids, float* vertices, float* colors, void* stream) {
    SCR_MARK_FN;
    TssVol g;
    if (tss_dims(__func__, nx, ny, nz, &g) || tss_geometry(__func__, lo_host, h, 1.0, &g) || tss_extract_count(__func__, g, nb, first, count)) return 1;
    if (min_weight != min_weight) return fail("%s: min_weight is NaN", __func__);
    if (nv < 0 || nv >= (1ll << 31)) return fail("%s: nv = %lld is not in 0 .. 2^31 - 1", __func__, (long long)nv);
    if (nv == 0) return 0;
    if (count == 0) return fail("%s: %lld vertices but no blocks", __func__, (long long)nv);
    if (!keys || !slots || !table || !tsdf || !weight || !scratch || !edge_ids || !vertices) return fail("%s: NULL argument", __func__);
    if ((color != nullptr) != (colors != nullptr)) return fail("%s: color and colors: give both or neither", __func__);
    hipStream_t st = (hipStream_t)stream;
    const int64_t items = (int64_t)TSS_EDGES * count;
    const KeepEdgeS ke{TssGrid{nx, ny, nz, g.nbx, g.nby, keys, slots, table, tsdf, weight, min_weight}, (int64_t)TSS_EDGES * first};
    tsdfs_vertex_write_kernel<<<(uint32_t)compact_nwg(items), COMPACT_THREADS, 0, st>>>(
        items, ke, (const uint32_t*)scratch, TssGeo{g.lox, g.loy, g.loz, g.h}, color, nv, edge_ids, vertices, colors);
    CHECK_LAUNCH("tsdfs_vertex_write_kernel", 0, st);
    return 0;
}

int scr_tsdfs_extract_faces_plan(int32_t nx, int32_t ny, int32_t nz, int64_t nb, int64_t first, int64_t count, const int32_t* keys,
                                 const int32_t* slots, const int32_t* table, const float* tsdf, const float* weight, float min_weight,
                                 void* scratch, int64_t* count_host, void* stream) {
    SCR_MARK_FN;
    if (!count_host) return fail("%s: count_host is NULL", __func__);
    *count_host = 0;
    TssVol g;
    if (tss_dims(__func__, nx, ny, nz, &g) || tss_extract_count(__func__, g, nb, first, count)) return 1;
    if (min_weight != min_weight) return fail("%s: min_weight is NaN", __func__);
    if (count == 0) return 0;
    if (!keys || !slots || !table || !tsdf || !weight || !scratch) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    const int64_t items = (int64_t)TSS_SLOTS * count;
    const KeepSlotS ks{TssGrid{nx, ny, nz, g.nbx, g.nby, keys, slots, table, tsdf, weight, min_weight}, (int64_t)TSS_SLOTS * first};
    return compact_plan("compact_count_kernel<KeepSlotS>", items, scratch, count_host, st,
                        [&](const CompactScratch& s, unsigned long long* mb, unsigned long long seq) {
                            launch_compact_count(items, ks, s, mb, seq, st);
                        });
}

int scr_tsdfs_extract_faces_run(int32_t nx, int32_t ny, int32_t nz, int64_t nb, int64_t first, int64_t count, const int32_t* keys,
                                const int32_t* slots, const int32_t* table, const float* tsdf, const float* weight, float min_weight,
                                const void* scratch, int64_t nv, const int64_t* edge_ids, int64_t nf, int32_t* faces, void* stream) {
    SCR_MARK_FN;
    TssVol g;
    if (tss_dims(__func__, nx, ny, nz, &g) || tss_extract_count(__func__, g, nb, first, count)) return 1;
    if (min_weight != min_weight) return fail("%s: min_weight is NaN", __func__);
    if (nv < 0 || nv >= (1ll << 31)) return fail("%s: nv = %lld is not in 0 .. 2^31 - 1", __func__, (long long)nv);
    if (nf < 0 || nf >= (1ll << 31)) return fail("%s: nf = %lld is not in 0 .. 2^31 - 1", __func__, (long long)nf);
    if (nf == 0) return 0;
    if (nv == 0 || count == 0) return fail("%s: %lld faces but no vertices", __func__, (long long)nf);
    if (!keys || !slots || !table || !tsdf || !weight || !scratch || !edge_ids || !faces) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    const int64_t items = (int64_t)TSS_SLOTS * count;
    const KeepSlotS ks{TssGrid{nx, ny, nz, g.nbx, g.nby, keys, slots, table, tsdf, weight, min_weight}, (int64_t)TSS_SLOTS * first};
    tsdfs_face_write_kernel<<<(uint32_t)compact_nwg(items), COMPACT_THREADS, 0, st>>>(items, ks, (const uint32_t*)scratch, nv, edge_ids, nf, faces);
    CHECK_LAUNCH("tsdfs_face_write_kernel", 0, st);
    return 0;
}

}  // extern "C"
