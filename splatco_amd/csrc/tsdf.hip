// splatco_amd/csrc/tsdf.hip -- TSDF fusion of rendered depth maps into a dense volume, and marching tetrahedra on it (gfx950).
//
// The definition is include/splatco_tsdf.h's (tests/tsdf_ref.py restates it in numpy float64).  Everything between the float32
// inputs and the float32 outputs is binary64 in the written order; the Makefile's -ffp-contract=off keeps it uncontracted.
// The update of one node by one view (ts_node_update) and the lattice tables live in tsdf_node.h, which the block-sparse
// family (tsdf_sparse.hip) shares: a node of a sparse block gets this kernel's own code.
//
// Integration.  One pass over the volume per batch of up to SCR_TSDF_MAX_VIEWS views.  The volume is walked as the LINEAR array
// of its nx ny nz nodes: thread t owns the nodes 4 t .. 4 t + 3, x-adjacent except where a row ends inside the run, and carries
// (i, j, k) along with a carry at nx and ny, so nx is arbitrary and every access of tsdf, weight and the three colour planes
// is one 16-byte load or store (taken when the node count is a multiple of 4 and the tensors are 16-byte aligned; guarded
// dword accesses otherwise, and in either case nothing beyond node N - 1 is touched).  The five values of a node stay in
// registers across the views of the batch, re-widened from their float32 rounding for every view, so a batch gives the bits
// of one call per view while the volume is read and written once.  The camera records of the batch are a kernel argument (184
// bytes per view, 2944 for 16) read through the scalar cache; depth, alpha, mask and image are gathered through the vector
// cache (neighbouring nodes hit neighbouring pixels).  A node that a view does not reach leaves the loop body before the
// gather; no atomics, one owner per node.
//
// Extraction.  Two order-preserving compactions on compact.h (count, scan, write; one host read each through compact_plan):
//   1. items = the 7 N lattice edge ids, keep = the edge's nodes differ in insideness and one of the cubes around it is valid;
//      the write kernel stores the kept id, the vertex and its colour at the item's rank, so the id list comes out sorted;
//   2. items = 12 triangle slots per cube (6 tetrahedra x 2), keep = slot used; the write kernel finds each of the three
//      vertices by binary search of its edge id in the sorted list.  There is no dense edge -> vertex map.
// The predicates read the two (edge) or four (tetrahedron) tsdf values in load(); the eight weights of a cube are read in
// keep(), and only for the few items that passed the sign test.
#include "capi.h"
#include "tsdf_node.h"

namespace scr {

constexpr int TS_THREADS = 256;
constexpr int TS_RUN = 4;                               // nodes per thread: one 16-byte access per tensor plane

struct TsVol {
    int nx, ny, nz, vec;                                // vec: 16-byte accesses are possible
    int64_t N;
    double lox, loy, loz, h, trunc, max_weight;
};
struct TsBatch {
    int n;
    scr_tsdf_view v[SCR_TSDF_MAX_VIEWS];
};
static_assert(sizeof(TsBatch) + sizeof(TsVol) + 3 * sizeof(void*) <= 4096, "the batch must fit the kernel argument segment");

__device__ __forceinline__ void ts_load4(const float* __restrict__ p, int64_t n0, int cnt, int vec, float (&v)[TS_RUN]) {
    if (vec) {
        const float4 t = *(const float4*)(p + n0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int r = 0; r < TS_RUN; ++r) v[r] = r < cnt ? p[n0 + r] : 0.0f;
    }
}
__device__ __forceinline__ void ts_store4(float* __restrict__ p, int64_t n0, int cnt, int vec, const float (&v)[TS_RUN]) {
    if (vec) {
        *(float4*)(p + n0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int r = 0; r < TS_RUN; ++r)
            if (r < cnt) p[n0 + r] = v[r];
    }
}

template <bool COLOR>
__global__ void __launch_bounds__(TS_THREADS)
tsdf_integrate_kernel(TsVol g, TsBatch b, float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color) {
    const int64_t n0 = ((int64_t)blockIdx.x * TS_THREADS + threadIdx.x) * TS_RUN;
    if (n0 >= g.N) return;
    const int cnt = (int)min((int64_t)TS_RUN, g.N - n0);           // vec implies N % 4 == 0: cnt == 4
    float s[TS_RUN], w[TS_RUN], c0[TS_RUN], c1[TS_RUN], c2[TS_RUN];
    ts_load4(tsdf, n0, cnt, g.vec, s);
    ts_load4(weight, n0, cnt, g.vec, w);
    if (COLOR) {
        ts_load4(color, n0, cnt, g.vec, c0);
        ts_load4(color + g.N, n0, cnt, g.vec, c1);
        ts_load4(color + 2 * g.N, n0, cnt, g.vec, c2);
    }
    const int i0 = (int)(n0 % g.nx);
    const int64_t row = n0 / g.nx;
    const int j0 = (int)(row % g.ny), k0 = (int)(row / g.ny);

    for (int view = 0; view < b.n; ++view) {
        const scr_tsdf_view& V = b.v[view];
        const double* M = V.w2c;
        const size_t HW = (size_t)V.H * V.W;
        int i = i0, j = j0, k = k0;
#pragma unroll
        for (int r = 0; r < TS_RUN; ++r) {
            const int ci = i, cj = j, ck = k;
            if (++i == g.nx) {
                i = 0;
                if (++j == g.ny) { j = 0; ++k; }
            }
            if (r >= cnt) continue;
            ts_node_update<COLOR>(g, V, M, HW, ci, cj, ck, s[r], w[r], c0[r], c1[r], c2[r]);     // tsdf_node.h
        }
    }
    ts_store4(tsdf, n0, cnt, g.vec, s);
    ts_store4(weight, n0, cnt, g.vec, w);
    if (COLOR) {
        ts_store4(color, n0, cnt, g.vec, c0);
        ts_store4(color + g.N, n0, cnt, g.vec, c1);
        ts_store4(color + 2 * g.N, n0, cnt, g.vec, c2);
    }
}

// ------------------------------------------------------------------ extraction (the lattice tables are tsdf_node.h's)
struct TsGrid {
    int nx, ny, nz;
    const float* __restrict__ tsdf;
    const float* __restrict__ weight;
    float min_weight;
    __device__ __forceinline__ int64_t lin(int i, int j, int k) const { return ((int64_t)k * ny + j) * nx + i; }
    __device__ __forceinline__ int64_t code_step(int code) const {
        return (int64_t)(code & 1) + (int64_t)((code >> 1) & 1) * nx + (int64_t)((code >> 2) & 1) * nx * ny;
    }
    // the cube with corner (i, j, k) exists and all 8 of its nodes have weight > min_weight
    __device__ bool cube_valid(int i, int j, int k) const {
        if (i < 0 || j < 0 || k < 0 || i >= nx - 1 || j >= ny - 1 || k >= nz - 1) return false;
        const float* p = weight + lin(i, j, k);
        bool ok = true;
#pragma unroll
        for (int code = 0; code < 8; ++code) ok = ok && p[code_step(code)] > min_weight;
        return ok;
    }
};

struct TsEdge { int i, j, k, dir, code; int64_t n; };
__device__ __forceinline__ TsEdge ts_edge(const TsGrid& g, int64_t e) {
    TsEdge o;
    o.n = e / 7;
    o.dir = (int)(e - 7 * o.n);
    o.code = ts_dir_code(o.dir);
    o.i = (int)(o.n % g.nx);
    const int64_t row = o.n / g.nx;
    o.j = (int)(row % g.ny);
    o.k = (int)(row / g.ny);
    return o;
}

// an edge id is kept where the edge carries a vertex
struct KeepEdge {
    struct Operand { float sa, sb; };
    TsGrid g;
    __device__ Operand load(int64_t e) const {
        const TsEdge ed = ts_edge(g, e);
        const bool in = ed.i + (ed.code & 1) < g.nx && ed.j + ((ed.code >> 1) & 1) < g.ny && ed.k + ((ed.code >> 2) & 1) < g.nz;
        return {g.tsdf[ed.n], g.tsdf[in ? ed.n + g.code_step(ed.code) : ed.n]};      // off the lattice: no sign change
    }
    __device__ bool keep(const Operand& v, int64_t e) const {
        if ((v.sa < 0.0f) == (v.sb < 0.0f)) return false;
        const TsEdge ed = ts_edge(g, e);
        // the cubes around the edge: the corner may step back along every axis the edge does not run along
        for (int back = 0; back < 8; ++back) {
            if (back & ed.code) continue;
            if (g.cube_valid(ed.i - (back & 1), ed.j - ((back >> 1) & 1), ed.k - ((back >> 2) & 1))) return true;
        }
        return false;
    }
};

struct TsGeo { double lox, loy, loz, h; };

__global__ void __launch_bounds__(COMPACT_THREADS)
tsdf_vertex_write_kernel(int64_t items, KeepEdge ke, const uint32_t* __restrict__ wg_offset, TsGeo geo, const float* __restrict__ color,
                         int64_t N, int64_t nv, int32_t* __restrict__ ids, float* __restrict__ verts, float* __restrict__ cols) {
    const CompactRank<KeepEdge> c = compact_rank(items, ke, wg_offset);
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) {
        if (!c.keep[r] || (int64_t)c.pos[r] >= nv) continue;
        const int64_t e = compact_item(r);
        const TsEdge ed = ts_edge(ke.g, e);
        const int64_t nb = ed.n + ke.g.code_step(ed.code);
        const double sa = (double)c.v[r].sa, sb = (double)c.v[r].sb;
        const double t = sa / (sa - sb);
        const size_t o = 3 * (size_t)c.pos[r];
        ids[c.pos[r]] = (int32_t)e;
        const double ax = geo.lox + geo.h * (double)ed.i, ay = geo.loy + geo.h * (double)ed.j, az = geo.loz + geo.h * (double)ed.k;
        const double bx = geo.lox + geo.h * (double)(ed.i + (ed.code & 1)), by = geo.loy + geo.h * (double)(ed.j + ((ed.code >> 1) & 1)),
                     bz = geo.loz + geo.h * (double)(ed.k + ((ed.code >> 2) & 1));
        verts[o] = (float)(ax + (bx - ax) * t);
        verts[o + 1] = (float)(ay + (by - ay) * t);
        verts[o + 2] = (float)(az + (bz - az) * t);
        if (color) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double ca = (double)color[(size_t)ch * N + ed.n], cb = (double)color[(size_t)ch * N + nb];
                cols[o + ch] = (float)(ca + (cb - ca) * t);
            }
        }
    }
}

struct TsSlot { int i, j, k, q, tri; int64_t n; };
__device__ __forceinline__ TsSlot ts_slot(const TsGrid& g, int64_t it) {
    TsSlot o;
    const int64_t cube = it / 12;
    const int s = (int)(it - 12 * cube);
    o.q = s >> 1;
    o.tri = s & 1;
    o.i = (int)(cube % (g.nx - 1));
    const int64_t row = cube / (g.nx - 1);
    o.j = (int)(row % (g.ny - 1));
    o.k = (int)(row / (g.ny - 1));
    o.n = g.lin(o.i, o.j, o.k);
    return o;
}

// a triangle slot (cube, tetrahedron, 0 / 1) is kept where the tetrahedron is cut and its cube is valid
struct KeepSlot {
    struct Operand { uint32_t mask; };                  // bit x: local node x of the tetrahedron is inside
    TsGrid g;
    __device__ Operand load(int64_t it) const {
        const TsSlot sl = ts_slot(g, it);
        uint32_t m = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) m |= (g.tsdf[sl.n + g.code_step(ts_tet_code(sl.q, x))] < 0.0f ? 1u : 0u) << x;
        return {m};
    }
    __device__ bool keep(const Operand& v, int64_t it) const {
        const int cnt = __builtin_popcount(v.mask);
        if (cnt == 0 || cnt == 4 || ((it & 1) && cnt != 2)) return false;      // 12 | it - slot: the slot's parity is it's
        const TsSlot sl = ts_slot(g, it);
        return g.cube_valid(sl.i, sl.j, sl.k);
    }
};

// position of edge id `key` in the sorted list (it is there: the two compactions read the same volume)
__device__ __forceinline__ int32_t ts_find(const int32_t* __restrict__ ids, int64_t nv, int32_t key) {
    int64_t lo = 0, hi = nv;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ids[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (int32_t)min(lo, nv - 1);
}

__global__ void __launch_bounds__(COMPACT_THREADS)
tsdf_face_write_kernel(int64_t items, KeepSlot ks, const uint32_t* __restrict__ wg_offset, int64_t nv, const int32_t* __restrict__ ids,
                       int64_t nf, int32_t* __restrict__ faces) {
    const CompactRank<KeepSlot> c = compact_rank(items, ks, wg_offset);
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) {
        if (!c.keep[r] || (int64_t)c.pos[r] >= nf) continue;
        const TsSlot sl = ts_slot(ks.g, compact_item(r));
        int ex[3], ey[3];                               // the triangle's edges as pairs of local nodes
        ts_triangle_edges(c.v[r].mask, sl.q, sl.tri, ex, ey);
        const size_t o = 3 * (size_t)c.pos[r];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int cx = ts_tet_code(sl.q, min(ex[e], ey[e])), cy = ts_tet_code(sl.q, max(ex[e], ey[e]));
            const int64_t eid = 7 * (sl.n + ks.g.code_step(cx)) + ts_code_dir(cx ^ cy);
            faces[o + e] = ts_find(ids, nv, (int32_t)eid);
        }
    }
}

// ------------------------------------------------------------------ host checks
static int ts_dims(const char* who, int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return fail("%s: dims (%d, %d, %d): every dimension must be >= 2", who, nx, ny, nz);
    if ((int64_t)nx * ny >= (1ll << 31) || (int64_t)nx * ny * nz >= (1ll << 31))
        return fail("%s: dims (%d, %d, %d): the node count is not below 2^31", who, nx, ny, nz);
    return 0;
}
static int ts_extract_dims(const char* who, int nx, int ny, int nz) {
    if (ts_dims(who, nx, ny, nz)) return 1;
    if (7 * ((int64_t)nx * ny * nz) >= (1ll << 31)) return fail("%s: 7 nx ny nz edge ids are not below 2^31", who);
    return 0;
}
static int64_t ts_edge_items(int nx, int ny, int nz) { return 7 * ((int64_t)nx * ny * nz); }
static int64_t ts_slot_items(int nx, int ny, int nz) { return 12 * ((int64_t)(nx - 1) * (ny - 1) * (nz - 1)); }
static bool ts_fin(double x) { return x == x && x - x == 0.0; }
static bool ts_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace scr

using namespace scr;

extern "C" {

int scr_tsdf_abi_version(void) { return SCR_TSDF_ABI_VERSION; }

int scr_tsdf_integrate(int32_t nx, int32_t ny, int32_t nz, const float* lo_host, float h, double trunc, float max_weight,
                       float* tsdf, float* weight, float* color, int32_t nviews, const scr_tsdf_view* views_host, void* stream) {
    SCR_MARK_FN;
    if (ts_dims(__func__, nx, ny, nz)) return 1;
    if (!(h > 0.0f) || !ts_fin(h)) return fail("%s: voxel size h = %g must be finite and > 0", __func__, (double)h);
    if (!(trunc > 0.0) || !ts_fin(trunc)) return fail("%s: trunc = %g must be finite and > 0", __func__, trunc);
    if (!(max_weight > 0.0f) || !ts_fin(max_weight)) return fail("%s: max_weight = %g must be finite and > 0", __func__, (double)max_weight);
    if (!lo_host) return fail("%s: lo_host is NULL", __func__);
    if (!ts_fin(lo_host[0]) || !ts_fin(lo_host[1]) || !ts_fin(lo_host[2])) return fail("%s: lo is not finite", __func__);
    if (nviews < 1 || nviews > SCR_TSDF_MAX_VIEWS) return fail("%s: nviews = %d is not in 1 .. %d", __func__, nviews, SCR_TSDF_MAX_VIEWS);
    if (!views_host) return fail("%s: views_host is NULL", __func__);
    TsBatch b;
    b.n = nviews;
    for (int i = 0; i < SCR_TSDF_MAX_VIEWS; ++i) b.v[i] = views_host[i < nviews ? i : 0];
    for (int i = 0; i < nviews; ++i) {
        const scr_tsdf_view& v = b.v[i];
        if (v.H < 1 || v.W < 1) return fail("%s: view %d: H = %d, W = %d must be >= 1", __func__, i, v.H, v.W);
        if ((int64_t)v.H * v.W >= (1ll << 31)) return fail("%s: view %d: H W is not below 2^31", __func__, i);
        if (!(v.fx > 0.0) || !(v.fy > 0.0) || !ts_fin(v.fx) || !ts_fin(v.fy)) return fail("%s: view %d: fx, fy must be finite and > 0", __func__, i);
        if (!ts_fin(v.cx) || !ts_fin(v.cy)) return fail("%s: view %d: cx, cy must be finite", __func__, i);
        for (int m = 0; m < 12; ++m)
            if (!ts_fin(v.w2c[m])) return fail("%s: view %d: w2c is not finite", __func__, i);
        if (!(v.near >= 0.0) || !ts_fin(v.near)) return fail("%s: view %d: near = %g must be finite and >= 0", __func__, i, v.near);
        if (!(v.min_alpha >= 0.0f) || !ts_fin(v.min_alpha)) return fail("%s: view %d: min_alpha must be finite and >= 0", __func__, i);
        if (v.mask_kind < 0 || v.mask_kind > 2) return fail("%s: view %d: mask_kind %d is not 0, 1 or 2", __func__, i, v.mask_kind);
    }
    if (!tsdf || !weight) return fail("%s: NULL volume", __func__);
    for (int i = 0; i < nviews; ++i) {
        const scr_tsdf_view& v = b.v[i];
        if (!v.depth || !v.alpha) return fail("%s: view %d: NULL map", __func__, i);
        if (v.mask_kind != 0 && !v.mask) return fail("%s: view %d: mask is NULL with mask_kind %d", __func__, i, v.mask_kind);
        if (v.image && !color) return fail("%s: view %d: an image, but the volume has no colour", __func__, i);
    }
    TsVol g;
    g.nx = nx; g.ny = ny; g.nz = nz;
    g.N = (int64_t)nx * ny * nz;
    g.vec = (g.N % TS_RUN == 0 && ts_al16(tsdf) && ts_al16(weight) && ts_al16(color)) ? 1 : 0;
    g.lox = lo_host[0]; g.loy = lo_host[1]; g.loz = lo_host[2];
    g.h = h; g.trunc = trunc; g.max_weight = max_weight;
    hipStream_t st = (hipStream_t)stream;
    const unsigned nwg = (unsigned)((g.N + (int64_t)TS_THREADS * TS_RUN - 1) / ((int64_t)TS_THREADS * TS_RUN));
    if (color) tsdf_integrate_kernel<true><<<nwg, TS_THREADS, 0, st>>>(g, b, tsdf, weight, color);
    else tsdf_integrate_kernel<false><<<nwg, TS_THREADS, 0, st>>>(g, b, tsdf, weight, nullptr);
    CHECK_LAUNCH("tsdf_integrate_kernel", 0, st);
    return 0;
}

size_t scr_tsdf_extract_scratch_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2 || 7 * ((double)nx * ny * nz) >= 2147483648.0) return 256;
    const int64_t e = ts_edge_items(nx, ny, nz), s = ts_slot_items(nx, ny, nz);
    return compact_scratch_bytes(e > s ? e : s);
}

int scr_tsdf_extract_vertices_plan(int32_t nx, int32_t ny, int32_t nz, const float* tsdf, const float* weight, float min_weight,
                                   void* scratch, int64_t* count_host, void* stream) {
    SCR_MARK_FN;
    if (!count_host) return fail("%s: count_host is NULL", __func__);
    *count_host = 0;
    if (ts_extract_dims(__func__, nx, ny, nz)) return 1;
    if (min_weight != min_weight) return fail("%s: min_weight is NaN", __func__);
    if (!tsdf || !weight || !scratch) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    const int64_t items = ts_edge_items(nx, ny, nz);
    const KeepEdge ke{TsGrid{nx, ny, nz, tsdf, weight, min_weight}};
    return compact_plan("compact_count_kernel<KeepEdge>", items, scratch, count_host, st,
                        [&](const CompactScratch& s, unsigned long long* mb, unsigned long long seq) {
                            launch_compact_count(items, ke, s, mb, seq, st);
                        });
}

int scr_tsdf_extract_vertices_run(int32_t nx, int32_t ny, int32_t nz, const float* lo_host, float h, const float* tsdf,
                                  const float* weight, const float* color, float min_weight, const void* scratch, int64_t nv,
                                  int32_t* edge_ids, float* vertices, float* colors, void* stream) {
    SCR_MARK_FN;
    if (ts_extract_dims(__func__, nx, ny, nz)) return 1;
    if (!(h > 0.0f) || !ts_fin(h)) return fail("%s: voxel size h = %g must be finite and > 0", __func__, (double)h);
    if (!lo_host) return fail("%s: lo_host is NULL", __func__);
    if (!ts_fin(lo_host[0]) || !ts_fin(lo_host[1]) || !ts_fin(lo_host[2])) return fail("%s: lo is not finite", __func__);
    if (min_weight != min_weight) return fail("%s: min_weight is NaN", __func__);
    if (nv < 0 || nv >= (1ll << 31)) return fail("%s: nv = %lld is not in 0 .. 2^31 - 1", __func__, (long long)nv);
    if (nv == 0) return 0;
    if (!tsdf || !weight || !scratch || !edge_ids || !vertices) return fail("%s: NULL argument", __func__);
    if ((color != nullptr) != (colors != nullptr)) return fail("%s: color and colors: give both or neither", __func__);
    hipStream_t st = (hipStream_t)stream;
    const int64_t items = ts_edge_items(nx, ny, nz);
    const KeepEdge ke{TsGrid{nx, ny, nz, tsdf, weight, min_weight}};
    tsdf_vertex_write_kernel<<<(uint32_t)compact_nwg(items), COMPACT_THREADS, 0, st>>>(
        items, ke, (const uint32_t*)scratch, TsGeo{lo_host[0], lo_host[1], lo_host[2], h}, color, (int64_t)nx * ny * nz, nv, edge_ids,
        vertices, colors);
    CHECK_LAUNCH("tsdf_vertex_write_kernel", 0, st);
    return 0;
}

int scr_tsdf_extract_faces_plan(int32_t nx, int32_t ny, int32_t nz, const float* tsdf, const float* weight, float min_weight,
                                void* scratch, int64_t* count_host, void* stream) {
    SCR_MARK_FN;
    if (!count_host) return fail("%s: count_host is NULL", __func__);
    *count_host = 0;
    if (ts_extract_dims(__func__, nx, ny, nz)) return 1;
    if (min_weight != min_weight) return fail("%s: min_weight is NaN", __func__);
    if (!tsdf || !weight || !scratch) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    const int64_t items = ts_slot_items(nx, ny, nz);
    const KeepSlot ks{TsGrid{nx, ny, nz, tsdf, weight, min_weight}};
    return compact_plan("compact_count_kernel<KeepSlot>", items, scratch, count_host, st,
                        [&](const CompactScratch& s, unsigned long long* mb, unsigned long long seq) {
                            launch_compact_count(items, ks, s, mb, seq, st);
                        });
}

int scr_tsdf_extract_faces_run(int32_t nx, int32_t ny, int32_t nz, const float* tsdf, const float* weight, float min_weight,
                               const void* scratch, int64_t nv, const int32_t* edge_ids, int64_t nf, int32_t* faces, void* stream) {
    SCR_MARK_FN;
    if (ts_extract_dims(__func__, nx, ny, nz)) return 1;
    if (min_weight != min_weight) return fail("%s: min_weight is NaN", __func__);
    if (nv < 0 || nv >= (1ll << 31)) return fail("%s: nv = %lld is not in 0 .. 2^31 - 1", __func__, (long long)nv);
    if (nf < 0 || nf >= (1ll << 31)) return fail("%s: nf = %lld is not in 0 .. 2^31 - 1", __func__, (long long)nf);
    if (nf == 0) return 0;
    if (nv == 0) return fail("%s: %lld faces but no vertices", __func__, (long long)nf);
    if (!tsdf || !weight || !scratch || !edge_ids || !faces) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    const int64_t items = ts_slot_items(nx, ny, nz);
    const KeepSlot ks{TsGrid{nx, ny, nz, tsdf, weight, min_weight}};
    tsdf_face_write_kernel<<<(uint32_t)compact_nwg(items), COMPACT_THREADS, 0, st>>>(items, ks, (const uint32_t*)scratch, nv, edge_ids, nf,
                                                                                    faces);
    CHECK_LAUNCH("tsdf_face_write_kernel", 0, st);
    return 0;
}

}  // extern "C"
