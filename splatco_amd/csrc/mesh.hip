// splatco_amd/csrc/mesh.hip -- clean-up of an indexed triangle mesh on the device (gfx950): connected components, the size
// filter of 2DGS's post_process_mesh, and vertex normals.
//
// The definition is include/splatco_mesh.h's (tests/mesh_ref.py restates it in numpy).  The normals are binary64 in the written
// order between the float32 inputs and the float32 outputs; the Makefile's -ffp-contract=off keeps them uncontracted.
//
// Components: a lock-free union-find over parent[nv], single pass (init, hook, flatten), then the face counts.
//   Invariant: parent[x] <= x at all times, and parent[x] is a vertex of x's component.  Only two kinds of write exist, both
//   atomic: the compare-and-swap parent[r]: r -> s with s < r that links a ROOT under a smaller vertex, and the atomic min
//   parent[x] <- g of the path halving, with g an earlier value of parent[parent[x]] and x already seen as a non-root.  Hence
//   parent chains strictly decrease (no cycle, at most nv steps), a non-root never becomes a root again, and the smallest
//   vertex of a component never gets a parent but itself: when every union is done, each component is one tree whose root is
//   its smallest index.
//   Cross-XCD visibility: the L2 is per XCD, so inside the hook kernel parent is read with relaxed agent-scope atomic loads
//   (they bypass the L1) and written with atomics only.  A load may still return an OLDER value of parent[x].  Every value
//   parent[x] ever held is x itself or a vertex below x in x's component, so a walk through stale values still ends at a
//   vertex r of the right component that SOME load saw as a root.  Whether r is a root now is decided by the compare-and-swap
//   alone, which acts on the one true copy: it succeeds only where parent[r] == r holds at that instant, and otherwise hands
//   back the current parent, from which the union starts again.  Linking a true root under a vertex that has stopped being
//   a root meanwhile is harmless: it is smaller and its component is the one to join.
//   Every loop is bounded: a union has a budget of 4 nv + 1024 walk steps (each retry makes at least two), a flatten walk
//   nv + 1; a thread that runs out raises *status and leaves.  The host sees the status in bit 31 of the roots count.
//
// Filter: three compact.h compactions (roots over the vertices, kept vertices, kept faces); the vertex write kernel leaves
// remap[v], the face write kernel re-indexes through it.
//
// Normals: the caller sorts the keys v nf + f; one thread per vertex finds its first key by binary search (as tsdf.hip finds
// edge ids) and walks its run in ascending face index, recomputing each face's cross product.  No atomics.
#include "capi.h"
#include "../../include/splatco_mesh.h"

namespace scr {

constexpr int MS_THREADS = 256;
constexpr long long MS_STATUS_BIT = 1ll << 31;

__device__ __forceinline__ int32_t ms_load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(MS_THREADS)
mesh_init_kernel(int64_t nv, int32_t* __restrict__ parent, int32_t* __restrict__ vertex_faces, int32_t* __restrict__ status) {
    const int64_t v = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (v == 0) *status = 0;
    if (v >= nv) return;
    parent[v] = (int32_t)v;
    vertex_faces[v] = 0;
}

// a vertex of x's component that a load saw as a root, halving the path on the way; -1 when the budget ran out
__device__ __forceinline__ int32_t ms_find(int32_t* parent, int32_t x, int64_t& budget) {
    while (budget-- > 0) {
        const int32_t p = ms_load(parent + x);
        if (p == x) return x;
        const int32_t g = ms_load(parent + p);
        if (g == p) return p;
        atomicMin(parent + x, g);
        x = g;
    }
    return -1;
}

__device__ __forceinline__ bool ms_union(int32_t* parent, int32_t a, int32_t b, int64_t& budget) {
    if (a == b) return true;
    // two vertices with one parent are in one component: most faces of a labelled region end here, without a read of the
    // root's word, which every other walk ends at.  A parent stands for its child in what follows
    a = ms_load(parent + a);
    b = ms_load(parent + b);
    if (a == b) return true;
    for (;;) {                                          // every round spends budget in ms_find: bounded
        int32_t ra = ms_find(parent, a, budget);
        int32_t rb = ra < 0 ? -1 : ms_find(parent, b, budget);
        if (rb < 0) return false;
        if (ra == rb) return true;
        if (ra < rb) { const int32_t t = ra; ra = rb; rb = t; }
        const int32_t old = atomicCAS(parent + ra, ra, rb);
        if (old == ra) return true;
        a = old;                                        // ra was linked by someone else: go on from what it points to now
        b = rb;
    }
}

__global__ void __launch_bounds__(MS_THREADS)
mesh_hook_kernel(int64_t nf, int64_t nv, const int32_t* __restrict__ faces, int32_t* parent, int32_t* status) {
    const int64_t f = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (f >= nf) return;
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    int64_t budget = 4 * nv + 1024;
    if (!ms_union(parent, i0, i1, budget)) { atomicOr(status, 1); return; }
    budget = 4 * nv + 1024;
    if (!ms_union(parent, i1, i2, budget)) atomicOr(status, 1);
}

__global__ void __launch_bounds__(MS_THREADS)
mesh_flatten_kernel(int64_t nv, const int32_t* __restrict__ parent, int32_t* __restrict__ labels, int32_t* status) {
    const int64_t v = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (v >= nv) return;
    int32_t x = (int32_t)v;
    int64_t steps = nv + 1;
    for (; steps > 0; --steps) {
        const int32_t p = parent[x];
        if (p == x) break;
        x = p;
    }
    if (steps == 0) atomicOr(status, 2);
    labels[v] = x;
}

// One add per wave and label, not per face: the faces of a large component all count at ONE word, and adds to one address are
// served one after the other.  The lanes of a wave that share the first pending lane's label are counted by a ballot and added
// once; at most 64 rounds, one for most waves of a mesh with few large components.  (With one add per face and without the
// same-parent exit of ms_union the components of a 6.25 M-face mesh took 61 ms, with both 5.7 ms, profiles/r20_mesh.txt; the
// two were not measured apart.)
__global__ void __launch_bounds__(MS_THREADS)
mesh_face_count_kernel(int64_t nf, const int32_t* __restrict__ faces, const int32_t* __restrict__ labels, int32_t* vertex_faces) {
    const int64_t f = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    bool todo = f < nf;
    const int32_t label = todo ? labels[faces[3 * f]] : -1;
    for (int round = 0; round < WAVE; ++round) {
        const unsigned long long pending = lanes(todo);
        if (pending == 0) break;
        const int leader = __builtin_ctzll(pending);
        const int32_t which = __builtin_amdgcn_readlane(label, leader);
        const bool mine = todo && label == which;
        const unsigned long long same = lanes(mine);
        if (lane == leader) atomicAdd(vertex_faces + which, (int32_t)__builtin_popcountll(same));
        todo = todo && !mine;
    }
}

// ------------------------------------------------------------------ compactions
struct KeepRoot {
    using Operand = int32_t;
    const int32_t* __restrict__ labels;
    __device__ Operand load(int64_t c) const { return labels[c]; }
    __device__ bool keep(const Operand& v, int64_t i) const { return (int64_t)v == i; }
};
// a vertex is kept where its component has at least `threshold` faces
struct KeepVertex {
    using Operand = int32_t;
    const int32_t* __restrict__ labels;
    const int32_t* __restrict__ vertex_faces;
    int32_t threshold;
    __device__ Operand load(int64_t c) const { return vertex_faces[labels[c]]; }
    __device__ bool keep(const Operand& v, int64_t) const { return v >= threshold; }
};
// a face is kept where its first vertex is
struct KeepFace {
    using Operand = int32_t;
    const int32_t* __restrict__ faces;
    KeepVertex kv;
    __device__ Operand load(int64_t c) const { return kv.load(faces[3 * c]); }
    __device__ bool keep(const Operand& v, int64_t i) const { return kv.keep(v, i); }
};

// the status word rides to the host in bit 31 of the roots count: the last workgroup's count takes it before the scan, whose
// exclusive prefixes (what the write pass reads) do not contain the last count.  nv < 2^31 leaves the bit free.
__global__ void mesh_status_fold_kernel(const int32_t* __restrict__ status, uint32_t* __restrict__ last_count) {
    if (*status != 0) *last_count |= 0x80000000u;
}

__global__ void __launch_bounds__(COMPACT_THREADS)
mesh_roots_write_kernel(int64_t items, KeepRoot k, const uint32_t* __restrict__ wg_offset, const int32_t* __restrict__ vertex_faces,
                        int64_t nc, int32_t* __restrict__ roots, int32_t* __restrict__ face_counts) {
    const CompactRank<KeepRoot> c = compact_rank(items, k, wg_offset);
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) {
        if (!c.keep[r] || (int64_t)c.pos[r] >= nc) continue;
        const int64_t v = compact_item(r);
        roots[c.pos[r]] = (int32_t)v;
        face_counts[c.pos[r]] = vertex_faces[v];
    }
}

__global__ void __launch_bounds__(COMPACT_THREADS)
mesh_vertices_write_kernel(int64_t items, KeepVertex k, const uint32_t* __restrict__ wg_offset, int64_t nkept,
                           const float* __restrict__ vertices, const float* __restrict__ colors, float* __restrict__ out_vertices,
                           float* __restrict__ out_colors, int32_t* __restrict__ remap) {
    const CompactRank<KeepVertex> c = compact_rank(items, k, wg_offset);
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) {
        if (!c.keep[r] || (int64_t)c.pos[r] >= nkept) continue;
        const size_t i = 3 * (size_t)compact_item(r), o = 3 * (size_t)c.pos[r];
        remap[compact_item(r)] = (int32_t)c.pos[r];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out_vertices[o + ch] = vertices[i + ch];
        if (colors) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out_colors[o + ch] = colors[i + ch];
        }
    }
}

__global__ void __launch_bounds__(COMPACT_THREADS)
mesh_faces_write_kernel(int64_t items, KeepFace k, const uint32_t* __restrict__ wg_offset, int64_t nkept,
                        const int32_t* __restrict__ remap, int32_t* __restrict__ out_faces) {
    const CompactRank<KeepFace> c = compact_rank(items, k, wg_offset);
#pragma unroll
    for (int r = 0; r < COMPACT_ITEMS; ++r) {
        if (!c.keep[r] || (int64_t)c.pos[r] >= nkept) continue;
        const size_t i = 3 * (size_t)compact_item(r), o = 3 * (size_t)c.pos[r];
#pragma unroll
        for (int e = 0; e < 3; ++e) out_faces[o + e] = remap[k.faces[i + e]];
    }
}

// ------------------------------------------------------------------ normals
__device__ __forceinline__ bool ms_finite(double x) { return x - x == 0.0; }                  // false for NaN and +-Inf

__global__ void __launch_bounds__(MS_THREADS)
mesh_normals_kernel(int64_t nv, int64_t nf, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                    const int64_t* __restrict__ keys, float* __restrict__ normals) {
    const int64_t v = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (v >= nv) return;
    const int64_t nk = 3 * nf, k0 = v * nf, k1 = k0 + nf;
    int64_t lo = 0, hi = nk;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < k0) lo = mid + 1; else hi = mid;
    }
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int64_t j = lo; j < nk; ++j) {
        const int64_t key = keys[j];
        if (key >= k1) break;
        const size_t f = (size_t)(key - k0);                                                  // in [0, nf)
        const float* p0 = vertices + 3 * (size_t)faces[3 * f];
        const float* p1 = vertices + 3 * (size_t)faces[3 * f + 1];
        const float* p2 = vertices + 3 * (size_t)faces[3 * f + 2];
        const double ax = (double)p0[0], ay = (double)p0[1], az = (double)p0[2];
        const double ux = (double)p1[0] - ax, uy = (double)p1[1] - ay, uz = (double)p1[2] - az;
        const double wx = (double)p2[0] - ax, wy = (double)p2[1] - ay, wz = (double)p2[2] - az;
        sx += uy * wz - uz * wy;
        sy += uz * wx - ux * wz;
        sz += ux * wy - uy * wx;
    }
    const double n = sqrt((sx * sx + sy * sy) + sz * sz);
    const bool ok = ms_finite(sx) && ms_finite(sy) && ms_finite(sz) && ms_finite(n) && n > 0.0;
    normals[3 * v] = ok ? (float)(sx / n) : 0.0f;
    normals[3 * v + 1] = ok ? (float)(sy / n) : 0.0f;
    normals[3 * v + 2] = ok ? (float)(sz / n) : 0.0f;
}

// ------------------------------------------------------------------ host checks
static int ms_sizes(const char* who, int64_t nv, int64_t nf) {
    if (nv < 0 || nv >= (1ll << 31)) return fail("%s: nv = %lld is not in 0 .. 2^31 - 1", who, (long long)nv);
    if (nf < 0 || 3 * nf >= (1ll << 31)) return fail("%s: nf = %lld: 3 nf is not in 0 .. 2^31 - 1", who, (long long)nf);
    return 0;
}
static int ms_threshold(const char* who, int32_t t) {
    return t >= 1 ? 0 : fail("%s: threshold = %d must be >= 1", who, t);
}
static unsigned ms_grid(int64_t n) { return (unsigned)((n + MS_THREADS - 1) / MS_THREADS); }

}  // namespace scr

using namespace scr;

extern "C" {

int scr_mesh_abi_version(void) { return SCR_MESH_ABI_VERSION; }

size_t scr_mesh_scratch_bytes(int64_t nv, int64_t nf) {
    if (nv < 0 || nf < 0 || nv >= (1ll << 31) || nf >= (1ll << 31)) return 256;
    const int64_t n = nv > nf ? nv : nf;
    return compact_scratch_bytes(n > 0 ? n : 1);
}

int scr_mesh_components(int64_t nv, int64_t nf, const int32_t* faces, int32_t* parent, int32_t* labels, int32_t* vertex_faces,
                        int32_t* status, void* stream) {
    SCR_MARK_FN;
    if (ms_sizes(__func__, nv, nf)) return 1;
    if (nv == 0 && nf > 0) return fail("%s: %lld faces but no vertices", __func__, (long long)nf);
    if (!status) return fail("%s: status is NULL", __func__);
    if (nv > 0 && (!parent || !labels || !vertex_faces)) return fail("%s: NULL argument", __func__);
    if (nf > 0 && !faces) return fail("%s: faces is NULL", __func__);
    hipStream_t st = (hipStream_t)stream;
    mesh_init_kernel<<<ms_grid(nv > 0 ? nv : 1), MS_THREADS, 0, st>>>(nv, parent, vertex_faces, status);
    CHECK_LAUNCH("mesh_init_kernel", 0, st);
    if (nv == 0) return 0;
    if (nf > 0) {
        mesh_hook_kernel<<<ms_grid(nf), MS_THREADS, 0, st>>>(nf, nv, faces, parent, status);
        CHECK_LAUNCH("mesh_hook_kernel", 0, st);
    }
    mesh_flatten_kernel<<<ms_grid(nv), MS_THREADS, 0, st>>>(nv, parent, labels, status);
    CHECK_LAUNCH("mesh_flatten_kernel", 0, st);
    if (nf > 0) {
        mesh_face_count_kernel<<<ms_grid(nf), MS_THREADS, 0, st>>>(nf, faces, labels, vertex_faces);
        CHECK_LAUNCH("mesh_face_count_kernel", 0, st);
    }
    return 0;
}

int scr_mesh_roots_plan(int64_t nv, const int32_t* labels, const int32_t* status, void* scratch, int64_t* count_host, void* stream) {
    SCR_MARK_FN;
    if (!count_host) return fail("%s: count_host is NULL", __func__);
    *count_host = 0;
    if (nv < 1 || nv >= (1ll << 31)) return fail("%s: nv = %lld is not in 1 .. 2^31 - 1", __func__, (long long)nv);
    if (!labels || !status || !scratch) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    const KeepRoot k{labels};
    const uint32_t nwg = (uint32_t)compact_nwg(nv);
    if (compact_plan("compact_count_kernel<KeepRoot>", nv, scratch, count_host, st,
                     [&](const CompactScratch& s, unsigned long long* mb, unsigned long long seq) {
                         compact_count_kernel<KeepRoot><<<nwg, COMPACT_THREADS, 0, st>>>(nv, k, s.wg);
                         mesh_status_fold_kernel<<<1, 1, 0, st>>>(status, s.wg + (nwg - 1));
                         compact_scan_kernel<<<1, 1024, 0, st>>>(nwg, s.wg, s.total, mb, seq);
                     }))
        return 1;
    if (*count_host & MS_STATUS_BIT) {
        *count_host = 0;
        return fail("%s: a component walk exceeded its iteration bound (the mesh was not labelled)", __func__);
    }
    return 0;
}

int scr_mesh_roots_run(int64_t nv, const int32_t* labels, const int32_t* vertex_faces, const void* scratch, int64_t nc,
                       int32_t* roots, int32_t* face_counts, void* stream) {
    SCR_MARK_FN;
    if (nv < 1 || nv >= (1ll << 31)) return fail("%s: nv = %lld is not in 1 .. 2^31 - 1", __func__, (long long)nv);
    if (nc < 0 || nc > nv) return fail("%s: nc = %lld is not in 0 .. nv", __func__, (long long)nc);
    if (nc == 0) return 0;
    if (!labels || !vertex_faces || !scratch || !roots || !face_counts) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    mesh_roots_write_kernel<<<(uint32_t)compact_nwg(nv), COMPACT_THREADS, 0, st>>>(nv, KeepRoot{labels}, (const uint32_t*)scratch,
                                                                                  vertex_faces, nc, roots, face_counts);
    CHECK_LAUNCH("mesh_roots_write_kernel", 0, st);
    return 0;
}

int scr_mesh_vertices_plan(int64_t nv, const int32_t* labels, const int32_t* vertex_faces, int32_t threshold, void* scratch,
                           int64_t* count_host, void* stream) {
    SCR_MARK_FN;
    if (!count_host) return fail("%s: count_host is NULL", __func__);
    *count_host = 0;
    if (nv < 1 || nv >= (1ll << 31)) return fail("%s: nv = %lld is not in 1 .. 2^31 - 1", __func__, (long long)nv);
    if (ms_threshold(__func__, threshold)) return 1;
    if (!labels || !vertex_faces || !scratch) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    const KeepVertex k{labels, vertex_faces, threshold};
    return compact_plan("compact_count_kernel<KeepVertex>", nv, scratch, count_host, st,
                        [&](const CompactScratch& s, unsigned long long* mb, unsigned long long seq) {
                            launch_compact_count(nv, k, s, mb, seq, st);
                        });
}

int scr_mesh_vertices_run(int64_t nv, const int32_t* labels, const int32_t* vertex_faces, int32_t threshold, const void* scratch,
                          int64_t nkept, const float* vertices, const float* colors, float* out_vertices, float* out_colors,
                          int32_t* remap, void* stream) {
    SCR_MARK_FN;
    if (nv < 1 || nv >= (1ll << 31)) return fail("%s: nv = %lld is not in 1 .. 2^31 - 1", __func__, (long long)nv);
    if (ms_threshold(__func__, threshold)) return 1;
    if (nkept < 0 || nkept > nv) return fail("%s: nkept = %lld is not in 0 .. nv", __func__, (long long)nkept);
    if (nkept == 0) return 0;
    if (!labels || !vertex_faces || !scratch || !vertices || !out_vertices || !remap) return fail("%s: NULL argument", __func__);
    if ((colors != nullptr) != (out_colors != nullptr)) return fail("%s: colors and out_colors: give both or neither", __func__);
    hipStream_t st = (hipStream_t)stream;
    mesh_vertices_write_kernel<<<(uint32_t)compact_nwg(nv), COMPACT_THREADS, 0, st>>>(
        nv, KeepVertex{labels, vertex_faces, threshold}, (const uint32_t*)scratch, nkept, vertices, colors, out_vertices, out_colors, remap);
    CHECK_LAUNCH("mesh_vertices_write_kernel", 0, st);
    return 0;
}

int scr_mesh_faces_plan(int64_t nf, const int32_t* faces, const int32_t* labels, const int32_t* vertex_faces, int32_t threshold,
                        void* scratch, int64_t* count_host, void* stream) {
    SCR_MARK_FN;
    if (!count_host) return fail("%s: count_host is NULL", __func__);
    *count_host = 0;
    if (nf < 1 || 3 * nf >= (1ll << 31)) return fail("%s: nf = %lld: 3 nf is not in 3 .. 2^31 - 1", __func__, (long long)nf);
    if (ms_threshold(__func__, threshold)) return 1;
    if (!faces || !labels || !vertex_faces || !scratch) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    const KeepFace k{faces, KeepVertex{labels, vertex_faces, threshold}};
    return compact_plan("compact_count_kernel<KeepFace>", nf, scratch, count_host, st,
                        [&](const CompactScratch& s, unsigned long long* mb, unsigned long long seq) {
                            launch_compact_count(nf, k, s, mb, seq, st);
                        });
}

int scr_mesh_faces_run(int64_t nf, const int32_t* faces, const int32_t* labels, const int32_t* vertex_faces, int32_t threshold,
                       const void* scratch, int64_t nkept, const int32_t* remap, int32_t* out_faces, void* stream) {
    SCR_MARK_FN;
    if (nf < 1 || 3 * nf >= (1ll << 31)) return fail("%s: nf = %lld: 3 nf is not in 3 .. 2^31 - 1", __func__, (long long)nf);
    if (ms_threshold(__func__, threshold)) return 1;
    if (nkept < 0 || nkept > nf) return fail("%s: nkept = %lld is not in 0 .. nf", __func__, (long long)nkept);
    if (nkept == 0) return 0;
    if (!faces || !labels || !vertex_faces || !scratch || !remap || !out_faces) return fail("%s: NULL argument", __func__);
    hipStream_t st = (hipStream_t)stream;
    mesh_faces_write_kernel<<<(uint32_t)compact_nwg(nf), COMPACT_THREADS, 0, st>>>(
        nf, KeepFace{faces, KeepVertex{labels, vertex_faces, threshold}}, (const uint32_t*)scratch, nkept, remap, out_faces);
    CHECK_LAUNCH("mesh_faces_write_kernel", 0, st);
    return 0;
}

int scr_mesh_vertex_normals(int64_t nv, int64_t nf, const float* vertices, const int32_t* faces, const int64_t* keys,
                            float* normals, void* stream) {
    SCR_MARK_FN;
    if (ms_sizes(__func__, nv, nf)) return 1;
    if (nv == 0) return 0;
    if (!vertices || !normals) return fail("%s: NULL argument", __func__);
    if (nf > 0 && (!faces || !keys)) return fail("%s: faces or keys is NULL", __func__);
    hipStream_t st = (hipStream_t)stream;
    mesh_normals_kernel<<<ms_grid(nv), MS_THREADS, 0, st>>>(nv, nf, vertices, faces, keys, normals);
    CHECK_LAUNCH("mesh_normals_kernel", 0, st);
    return 0;
}

}  // extern "C"
