// splatco_amd/csrc/capi.hip -- the C-ABI of include/splatco_raster.h: what every entry point shares, and the rasterizer.
// The entry points of an operator family (expansion, tri-planes, attention, losses, heads, optimizer, ...) live in the
// family's own .hip file, next to its kernels; capi.h is what those files include.  Here: scr_last_error and fail(), the
// profiling / marker scopes, the mailbox, scr_copy_probe, and the rasterizer pipeline (scr_geom_bytes ... scr_backward,
// scr_debug_*, scr_visible_filter, scr_mark_visible), whose launchers span preprocess.hip, binning.hip and blend.hip.
// Every data buffer is caller-owned (several forward graphs are alive at once in the mv loop of
// train.py:171-240).  Process-lifetime state of the library, all of it below: a thread-local error string, one pinned
// 64-byte mailbox per calling host thread + a process-wide stamp counter for the plan read-backs, a per-device flag for
// the dynamic-LDS attribute, and the opt-in profiling event pool (g_prof_*; single-threaded, see the header).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "capi.h"
#include <dlfcn.h>
#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <utility>
#include <vector>
#include <cstring>

using namespace scr;

static thread_local char g_err[512] = "";

// ---- opt-in kernel timing (scr_profile_*): hipEvent pairs on the launch stream
namespace {
struct ProfRec { int idx; hipEvent_t a, b; };
unsigned g_prof_mask = 0;  // bit i set: kernel class i is timed
unsigned g_prof_stride = 1;             // every g_prof_stride-th launch of a timed class is bracketed (scr_profile_stride)
unsigned g_prof_seen[32] = {};          // launches of class i since the mask was set
std::vector<ProfRec> g_prof_recs;
std::vector<hipEvent_t> g_prof_pool;
hipEvent_t prof_event() {
    hipEvent_t e;
    if (!g_prof_pool.empty()) { e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
    (void)hipEventCreate(&e);
    return e;
}
// ---- opt-in stage markers (scr_markers_enable): roctx ranges on the calling thread, the library loaded on first use
bool g_mark_on = false;
int (*g_roctx_push)(const char*) = nullptr;
int (*g_roctx_pop)() = nullptr;
const char* const kProfNames[SCR_PROF_COUNT] = {
    "filter_kernel", "preprocess_kernel", "plan_scan_kernel", "scatter_kernel", "tile_sort_kernel",
    "blend_forward_kernel", "blend_backward_kernel", "preprocess_backward_kernel", "expand_kernel",
    "expand_backward_kernel", "plane_sample_backward_kernels", "l1_ssim_forward_kernel",
    "l1_ssim_backward_kernel", "triplane_forward_kernel", "mlp_heads_kernel", "mlp_heads_backward_kernel",
    "norm_linear_kernels", "norm_linear_backward_kernels", "plane_attention_kernels", "flip_kernel"};
}  // namespace

namespace scr {
int g_force_deep_lists = -1;

void allow_dynamic_lds(const void* kernel, size_t bytes) {
    if (bytes <= 65536) return;
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> granted;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    size_t& have = granted[{dev, kernel}];
    if (bytes <= have) return;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess) have = bytes;
    (void)hipGetLastError();
}

int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

MarkScope::MarkScope(const char* name) : on(g_mark_on) { if (on) (void)g_roctx_push(name); }
MarkScope::~MarkScope() { if (on) (void)g_roctx_pop(); }

ProfScope::ProfScope(int idx_, hipStream_t s) : on((g_prof_mask >> idx_) & 1u), st(s), idx(idx_), mark(kProfNames[idx_]) {
    if (on && g_prof_stride > 1) on = (g_prof_seen[idx]++ % g_prof_stride) == 0;
    if (on) { a = prof_event(); b = prof_event(); (void)hipEventRecord(a, st); }
}
ProfScope::~ProfScope() { if (on) { (void)hipEventRecord(b, st); g_prof_recs.push_back({idx, a, b}); } }

Mailbox& mailbox() {
    thread_local Mailbox mb;
    thread_local bool tried = false;
    if (!tried) {
        tried = true;
        void* h = nullptr;
        if (hipHostMalloc(&h, 64, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess && h) {
            void* d = nullptr;
            if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess && d) {
                memset(h, 0, 64);
                mb.host = (volatile unsigned long long*)h;
                mb.dev = (unsigned long long*)d;
            } else {
                (void)hipHostFree(h);
            }
        }
        (void)hipGetLastError();
    }
    return mb;
}

bool mailbox_wait(Mailbox& mb, unsigned long long seq, bool two, hipStream_t st) {
    if (!mb.host) return false;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        // stamp first, with acquire ordering: the value words read afterwards are at least as new as the stamp
        if (__atomic_load_n(&mb.host[1], __ATOMIC_ACQUIRE) == seq && (!two || __atomic_load_n(&mb.host[3], __ATOMIC_ACQUIRE) == seq))
            return true;
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
        if ((spins & 1023u) == 1023u) {
            if (hipStreamQuery(st) != hipErrorNotReady)
                return __atomic_load_n(&mb.host[1], __ATOMIC_ACQUIRE) == seq &&
                       (!two || __atomic_load_n(&mb.host[3], __ATOMIC_ACQUIRE) == seq);
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) return false;
        }
    }
}
}  // namespace scr

// streaming copy, 16 B per lane, four loads in flight per thread, non-temporal: the shape that reaches the highest HBM
// bandwidth on MI355X among those of tools/exp/copy_probe.hip (6.3 TB/s read + write; a grid-stride loop with few
// workgroups stays at 4.7).  bench.py quotes its rate as the achievable peak next to the 8 TB/s datasheet figure.
typedef float copy_f4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) copy_probe_kernel(const copy_f4* __restrict__ src, copy_f4* __restrict__ dst, size_t n) {
    const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x;
    copy_f4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) if (base + u * 256 < n) v[u] = __builtin_nontemporal_load(&src[base + u * 256]);
#pragma unroll
    for (int u = 0; u < 4; ++u) if (base + u * 256 < n) __builtin_nontemporal_store(v[u], &dst[base + u * 256]);
}

static int check_settings(const scr_settings* s) {
    if (!s) return fail("settings is NULL");
    if (s->image_height <= 0 || s->image_width <= 0) return fail("image size must be positive");
    if (s->image_width > 16 * 65535 || s->image_height > 16 * 65535) return fail("image too large for 16-bit tile coordinates");
    if (!s->bg || !s->viewmatrix || !s->projmatrix || !s->campos) return fail("bg / viewmatrix / projmatrix / campos must be device pointers");
    if (s->sh_degree < 0 || s->sh_degree > 3) return fail("sh_degree must be 0..3");
    return 0;
}

static int check_plan_flags(int64_t plan_flags) {
    if (plan_flags & ~(int64_t)(SCR_PLAN_NONFINITE_COLOUR | SCR_PLAN_LARGE_RECTS | SCR_PLAN_ANTIALIASED)) return fail("plan_flags %lld: not a value scr_forward_plan returned", (long long)plan_flags);
    return 0;
}

// out_depth / out_alpha of the forward: both NULL (no maps) or both given
static int check_maps(const float* out_depth, const float* out_alpha) {
    if ((out_depth != nullptr) != (out_alpha != nullptr)) return fail("out_depth / out_alpha: give both maps or neither");
    return 0;
}

extern "C" {

int scr_abi_version(void) { return SCR_ABI_VERSION; }
const char* scr_last_error(void) { return g_err; }

size_t scr_geom_bytes(int64_t P, int32_t H, int32_t W) { return geom_view(nullptr, P, H, W).bytes; }
size_t scr_binning_bytes(int64_t I, int64_t max_tile) { return bin_view(nullptr, I, max_tile).bytes; }
size_t scr_image_bytes(int32_t H, int32_t W) { return img_view(nullptr, H, W).bytes; }
size_t scr_backward_scratch_bytes(int64_t I, int64_t P, int32_t maps, int32_t camera) {
    return grad_rec_bytes(I) + (maps || camera ? grad_z_bytes(I) : 0) + (camera ? camera_partials_bytes(P) : 0);
}

int scr_visible_filter(int64_t P, const float* means3D, const float* scales, const float* rotations,
                       const float* cov3D_precomp, const scr_settings* settings, int32_t* radii_out,
                       void* stream) {
    SCR_MARK_FN;
    if (check_settings(settings)) return 1;
    if (P < 0) return fail("P < 0");
    if (P == 0) return 0;
    if (!means3D || !radii_out) return fail("means3D / radii_out is NULL");
    if (!cov3D_precomp && !(scales && rotations)) return fail("provide (scales, rotations) or cov3D_precomp");
    hipStream_t st = (hipStream_t)stream;
    { ProfScope ps_(SCR_PROF_FILTER, st);
      launch_filter(P, means3D, scales, rotations, cov3D_precomp, ksettings(settings), radii_out, st); }
    CHECK_LAUNCH("filter_kernel", settings->debug, st);
    return 0;
}

int scr_mark_visible(int64_t P, const float* means3D, const float* viewmatrix, uint8_t* present_out,
                     void* stream) {
    SCR_MARK_FN;
    if (P < 0) return fail("P < 0");
    if (P == 0) return 0;
    if (!means3D || !viewmatrix || !present_out) return fail("NULL argument");
    hipStream_t st = (hipStream_t)stream;
    launch_mark_visible(P, means3D, viewmatrix, present_out, st);
    CHECK_LAUNCH("mark_visible_kernel", 0, st);
    return 0;
}

// phase 1, first half: argument checks, tile counts, projection, scans; the two counts are on their way to the mailbox
static int plan_enqueue(int64_t P, int32_t M, const float* means3D, const float* scales, const float* rotations,
                        const float* cov3D_precomp, const float* opacities, const float* shs, const float* colors_precomp,
                        const scr_settings* settings, void* geom_buf, int32_t* radii_out, int64_t* plan_host, hipStream_t st,
                        unsigned long long& seq_out, int64_t mode) {
    if (mode & ~(int64_t)SCR_MODE_ANTIALIASED) return fail("mode %lld: unknown bit (SCR_MODE_ANTIALIASED = %d is the only one)", (long long)mode, (int)SCR_MODE_ANTIALIASED);
    if (check_settings(settings)) return 1;
    if (P < 0) return fail("P < 0");
    if (!plan_host) return fail("plan_host is NULL");
    plan_host[0] = plan_host[1] = plan_host[3] = 0;
    if (!geom_buf) return fail("geom_buf is NULL");
    if ((shs != nullptr) == (colors_precomp != nullptr))
        return fail("pass either shs or colors_precomp (one of them, not both, not neither)");
    if (((scales != nullptr) || (rotations != nullptr)) == (cov3D_precomp != nullptr) || ((scales != nullptr) != (rotations != nullptr)))
        if (!(cov3D_precomp && !scales && !rotations) && !(scales && rotations && !cov3D_precomp))
            return fail("pass either scales + rotations or cov3D_precomp (one form of the covariance)");
    if (P > 0 && (!means3D || !opacities || !radii_out)) return fail("means3D / opacities / radii_out is NULL");
    if (P >= (1ll << ID_BITS)) return fail("P = %lld exceeds the 2^%d Gaussians a sort key can index", (long long)P, ID_BITS);
    if (shs && (M < (settings->sh_degree + 1) * (settings->sh_degree + 1)))
        return fail("shs has %d coefficients, sh_degree %d needs %d", M, settings->sh_degree,
                    (settings->sh_degree + 1) * (settings->sh_degree + 1));
    KSettings ks = ksettings(settings);
    GeomView gv = geom_view(geom_buf, P, ks.H, ks.W);
    Grid g(ks.H, ks.W);
    { ZeroList z; z.add(gv.tile_count, (size_t)g.tiles * 4, st); z.add(gv.total + 3, 8, st); launch_zero(z, st); }
    { ProfScope ps_(SCR_PROF_PREPROCESS, st);
      launch_preprocess(P, M, means3D, scales, rotations, cov3D_precomp, opacities, shs, colors_precomp, ks, gv,
                        radii_out, (mode & SCR_MODE_ANTIALIASED) != 0, st); }
    CHECK_LAUNCH("preprocess_kernel", settings->debug, st);
    // The two counts come back through a small pinned, device-visible mailbox (one per host thread, created on
    // first use): the scan kernel posts them with a sequence stamp and this thread spins on the stamp.  A blocking
    // hipStreamSynchronize + 16-byte copy costs a copy launch and, worse, a wake-up of the sleeping thread, which
    // on a busy host is anywhere between 10 and 200 us of idle GPU in the middle of every forward pass.
    Mailbox& mb = mailbox();
    seq_out = ++mb.seq;
    { ProfScope ps_(SCR_PROF_PLAN_SCAN, st); launch_plan_scans(P, ks, gv, mb.dev, seq_out, st); }
    CHECK_LAUNCH("plan_scan_kernel", settings->debug, st);
    return 0;
}

// phase 1, second half: wait for the two counts
static int plan_wait(const scr_settings* settings, void* geom_buf, int64_t P, unsigned long long seq, int64_t* plan_host,
                     hipStream_t st) {
    KSettings ks = ksettings(settings);
    GeomView gv = geom_view(geom_buf, P, ks.H, ks.W);
    Mailbox& mb = mailbox();
    unsigned long long total[4] = {0, 0, 0, 0};      // instances, largest tile, -, plan flags
    const bool posted = mailbox_wait(mb, seq, true, st);
    if (posted) {
        total[0] = mb.host[0];
        total[1] = mb.host[2] & 0xffffffffull;
        total[3] = mb.host[2] >> 32;
    }
    if (!posted) {  // no mailbox, or its writes are not visible on this system: the classic read-back
        HIP_TRY(hipMemcpyAsync(total, gv.total, 32, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    // per-workgroup sums saturate at 2^32 - 1 (preprocess_kernel) and the scan adds them in 64 bits: any total at or above
    // 2^32 - 1 means "does not fit" (the prefix values are meaningless then; nothing has been written through them yet)
    if (total[0] >= 0xFFFFFFFFull)
        return fail("num_rendered >= 2^32 - 1 (counted %llu): the (Gaussian, tile) instances do not fit 32-bit indices", total[0]);
    plan_host[0] = (int64_t)total[0];
    plan_host[1] = (int64_t)total[1];
    plan_host[3] = (int64_t)total[3];
    return 0;
}

int scr_forward_plan(int64_t mode, int64_t P, int32_t M, const float* means3D, const float* scales,
                     const float* rotations, const float* cov3D_precomp, const float* opacities,
                     const float* shs, const float* colors_precomp, const scr_settings* settings,
                     void* geom_buf, int32_t* radii_out, int64_t* plan_host, void* stream) {
    SCR_MARK_FN;
    unsigned long long seq = 0;
    const int rc = plan_enqueue(P, M, means3D, scales, rotations, cov3D_precomp, opacities, shs, colors_precomp, settings, geom_buf,
                                radii_out, plan_host, (hipStream_t)stream, seq, mode);
    return rc ? rc : plan_wait(settings, geom_buf, P, seq, plan_host, (hipStream_t)stream);
}

// phase 2 behind scr_forward_run and scr_forward_plan_run (scatter_done: the latter's early scatter filled the keys)
static int forward_run(int64_t P, int64_t I, int64_t max_tile, int64_t plan_flags, const scr_settings* settings, void* geom_buf,
                       void* binning_buf, void* image_buf, float* out_color, float* out_depth, float* out_alpha,
                       void* stream, bool scatter_done) {
    if (check_settings(settings)) return 1;
    if (check_plan_flags(plan_flags)) return 1;
    if (!geom_buf || !binning_buf || !image_buf || !out_color) return fail("NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    KSettings ks = ksettings(settings);
    GeomView gv = geom_view(geom_buf, P, ks.H, ks.W);
    BinView bv = bin_view(binning_buf, I, max_tile);
    ImgView iv = img_view(image_buf, ks.H, ks.W);
    if (I > 0) {
        if (!scatter_done) {
            { ProfScope ps_(SCR_PROF_SCATTER, st); launch_scatter(P, ks, gv, bv, ~0ull, st); }
            CHECK_LAUNCH("scatter_kernel", settings->debug, st);
        }
        { ProfScope ps_(SCR_PROF_TILE_SORT, st); launch_tile_sort(ks, gv, bv, max_tile, !deep_lists(I, Grid(ks.H, ks.W).tiles), st); }
        CHECK_LAUNCH("tile_sort_kernel", settings->debug, st);
    }
    { ProfScope ps_(SCR_PROF_BLEND_FORWARD, st); launch_blend_forward(ks, gv, bv, iv, out_color, out_depth, out_alpha, 2 * max_tile * (int64_t)Grid(ks.H, ks.W).tiles > 3 * I,
                                                                      (plan_flags & SCR_PLAN_NONFINITE_COLOUR) != 0, st); }
    CHECK_LAUNCH("blend_forward_kernel", settings->debug, st);
    return 0;
}

int scr_forward_run(int64_t P, int64_t I, int64_t max_tile, int64_t plan_flags, const scr_settings* settings, void* geom_buf,
                    void* binning_buf, void* image_buf, float* out_color, float* out_depth, float* out_alpha, void* stream) {
    SCR_MARK_FN;
    if (check_maps(out_depth, out_alpha)) return 1;
    return forward_run(P, I, max_tile, plan_flags, settings, geom_buf, binning_buf, image_buf, out_color, out_depth, out_alpha,
                       stream, false);
}

int scr_forward_plan_run(int64_t mode, int64_t P, int32_t M, const float* means3D, const float* scales, const float* rotations,
                         const float* cov3D_precomp, const float* opacities, const float* shs, const float* colors_precomp,
                         const scr_settings* settings, void* geom_buf, int32_t* radii_out, int64_t* plan_host,
                         void* binning_buf, size_t binning_capacity_bytes, void* image_buf, float* out_color,
                         float* out_depth, float* out_alpha, void* stream) {
    SCR_MARK_FN;
    if (check_maps(out_depth, out_alpha)) return 1;
    if (!plan_host) return fail("plan_host is NULL");
    plan_host[2] = 0;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long seq = 0;
    int rc = plan_enqueue(P, M, means3D, scales, rotations, cov3D_precomp, opacities, shs, colors_precomp, settings, geom_buf,
                          radii_out, plan_host, st, seq, mode);
    if (rc) return rc;
    // The scatter kernel goes out BEFORE this thread has seen the instance count: it needs nothing the host knows (the
    // keys are the first array of the binning buffer whatever the count), only room -- and checks on the device that the
    // count fits (17 bytes per instance is the least a binning buffer of that many instances takes, so the keys fit).
    // While it runs, the count arrives, the sort and the blend are queued behind it: the 12 - 20 us the GPU used to idle
    // in the middle of every forward pass (profiles/r03x_step_gaps.txt) are gone.
    const unsigned long long cap = binning_buf ? (unsigned long long)(binning_capacity_bytes / 17) : 0ull;
    const bool early = binning_buf && P > 0 && cap > 0 && image_buf && out_color;
    if (early) {
        KSettings ks = ksettings(settings);
        GeomView gv = geom_view(geom_buf, P, ks.H, ks.W);
        BinView bv = bin_view(binning_buf, 0, 0);
        { ProfScope ps_(SCR_PROF_SCATTER, st); launch_scatter(P, ks, gv, bv, cap, st); }
        CHECK_LAUNCH("scatter_kernel", settings->debug, st);
    }
    rc = plan_wait(settings, geom_buf, P, seq, plan_host, st);
    if (rc) return rc;
    const bool fits = binning_buf && scr_binning_bytes(plan_host[0], plan_host[1]) <= binning_capacity_bytes;
    const bool scattered = early && (unsigned long long)plan_host[0] <= cap;
    if (!fits) {
        if (scattered && plan_host[0] > 0) {      // the early scatter ran and used up the cursors: give scr_forward_run fresh ones
            KSettings ks = ksettings(settings);
            GeomView gv = geom_view(geom_buf, P, ks.H, ks.W);
            ZeroList z;
            z.add(gv.cursor, (size_t)Grid(ks.H, ks.W).tiles * 4, st);
            launch_zero(z, st);
        }
        return 0;                                  // caller allocates, then scr_forward_run
    }
    rc = forward_run(P, plan_host[0], plan_host[1], plan_host[3], settings, geom_buf, binning_buf, image_buf, out_color, out_depth,
                     out_alpha, stream, scattered);
    if (rc) return rc;
    plan_host[2] = 1;
    return 0;
}

// dL_ddepth / dL_dalpha both NULL: the colour-only kernels; the three camera outputs all NULL: the kernels without the
// camera sums
int scr_backward(int64_t P, int32_t M, int64_t I, int64_t plan_flags, const float* means3D, const float* scales,
                 const float* rotations, const float* cov3D_precomp, const float* shs,
                 const scr_settings* settings, const int32_t* radii, void* geom_buf,
                 const void* binning_buf, void* image_buf, const float* dL_dcolor, const float* dL_ddepth,
                 const float* dL_dalpha, void* scratch,
                 float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dcolors, float* dL_dsh,
                 float* dL_dopacity, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                 float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos, void* stream) {
    SCR_MARK_FN;
    if (check_settings(settings)) return 1;
    if (P < 0) return fail("P < 0");
    const bool camera = dL_dviewmatrix || dL_dprojmatrix || dL_dcampos;
    if (P == 0) {      // no Gaussian, no kernel: the camera's gradients are zeros, not what the caller's memory held
        if (dL_dviewmatrix) HIP_TRY(hipMemsetAsync(dL_dviewmatrix, 0, 16 * sizeof(float), (hipStream_t)stream));
        if (dL_dprojmatrix) HIP_TRY(hipMemsetAsync(dL_dprojmatrix, 0, 16 * sizeof(float), (hipStream_t)stream));
        if (dL_dcampos) HIP_TRY(hipMemsetAsync(dL_dcampos, 0, 3 * sizeof(float), (hipStream_t)stream));
        return 0;
    }
    if (check_plan_flags(plan_flags)) return 1;
    if (!geom_buf || !binning_buf || !image_buf || !dL_dcolor || !scratch) return fail("NULL buffer");
    if (!means3D || !radii || !dL_dmeans3D || !dL_dmeans2D || !dL_dopacity) return fail("NULL argument");
    if (shs ? !dL_dsh : !dL_dcolors) return fail("colour gradient output missing");
    if (cov3D_precomp ? !dL_dcov3D : !(dL_dscales && dL_drotations && scales && rotations))
        return fail("covariance gradient output missing");
    hipStream_t st = (hipStream_t)stream;
    KSettings ks = ksettings(settings);
    GeomView gv = geom_view(geom_buf, P, ks.H, ks.W);
    BinView bv = bin_view((void*)binning_buf, I, 0);  // the lists read here come first in the layout
    ImgView iv = img_view(image_buf, ks.H, ks.W);
    // a value no earlier call of this process used (and that uninitialised memory is unlikely to hold): see blend.hip
    static std::atomic<unsigned long long> stamp_counter{0x5ca1ab1e00000000ull};
    const unsigned long long stamp = ++stamp_counter;
    // the depth sums lie behind the records (scr_backward_scratch_bytes with maps)
    float* const grad_z = (I > 0 && (dL_ddepth || dL_dalpha)) ? (float*)((char*)scratch + grad_rec_bytes(I)) : nullptr;
    // the camera sums' rows lie behind both (scr_backward_scratch_bytes with camera reserves the depth sums whether used or not)
    float* const cam_partials = camera ? (float*)((char*)scratch + grad_rec_bytes(I) + grad_z_bytes(I)) : nullptr;
    if (settings->debug) {      // the flags the caller carried from scr_forward_plan against the ones the forward left in geom_buf
        unsigned long long dev_flags = 0;
        HIP_TRY(hipMemcpyAsync(&dev_flags, gv.total + 3, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((long long)dev_flags != (long long)plan_flags)
            return fail("plan_flags %lld passed to scr_backward, but the forward pass of this geom_buf raised %llu", (long long)plan_flags, dev_flags);
    }
    if (I > 0) {
        // records 32.. of large rects are cleared whatever plan_flags says: the kernel reads the forward's verdict from
        // geom_buf and leaves at once when there are none (2 us), so a stale argument cannot make preprocess_backward sum
        // uninitialised scratch
        launch_zero_far_records(P, gv, (GradRec*)scratch, grad_z, st);
        CHECK_LAUNCH("zero_far_records_kernel", settings->debug, st);
        { ProfScope ps_(SCR_PROF_BLEND_BACKWARD, st);
          launch_blend_backward(ks, gv, bv, iv, dL_dcolor, dL_ddepth, dL_dalpha, (GradRec*)scratch, grad_z, stamp, deep_lists(I, Grid(ks.H, ks.W).tiles),
                                record_flags(I, Grid(ks.H, ks.W).tiles), (plan_flags & SCR_PLAN_NONFINITE_COLOUR) != 0, st); }
        CHECK_LAUNCH("blend_backward_kernel", settings->debug, st);
    }
    { ProfScope ps_(SCR_PROF_PREPROCESS_BACKWARD, st);
      launch_preprocess_backward(P, M, means3D, scales, rotations, cov3D_precomp, shs, ks, radii, gv, bv,
                                 (const GradRec*)scratch, grad_z, iv.cut_key, stamp, record_flags(I, Grid(ks.H, ks.W).tiles), dL_dmeans3D, dL_dmeans2D, shs ? nullptr : dL_dcolors,
                                 shs ? dL_dsh : nullptr, dL_dopacity, cov3D_precomp ? nullptr : dL_dscales,
                                 cov3D_precomp ? nullptr : dL_drotations, cov3D_precomp ? dL_dcov3D : nullptr, cam_partials,
                                 (plan_flags & SCR_PLAN_ANTIALIASED) != 0, st); }
    CHECK_LAUNCH("preprocess_backward_kernel", settings->debug, st);
    if (camera) {      // I == 0 included: every row is zero then, and so is every output
        launch_camera_grad_finish(P, cam_partials, dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, st);
        CHECK_LAUNCH("camera_grad_finish_kernel", settings->debug, st);
    }
    return 0;
}

int scr_debug_force_deep_lists(int mode) {
    if (mode < -1 || mode > 1) return fail("scr_debug_force_deep_lists: -1 (automatic), 0 or 1");
    scr::g_force_deep_lists = mode;
    return 0;
}

int scr_debug_get(int which, int64_t P, int64_t I, int32_t H, int32_t W, const void* geom_buf,
                  const void* binning_buf, const void* image_buf, void* out, void* stream) {
    SCR_MARK_FN;
    hipStream_t st = (hipStream_t)stream;
    Grid g(H, W);
    const void* src = nullptr;
    size_t bytes = 0;
    if (which <= SCR_DBG_RANGES || which == SCR_DBG_SPLAT_RECORDS) {
        if (!geom_buf) return fail("geom_buf is NULL");
        GeomView gv = geom_view((void*)geom_buf, P, H, W);
        if (which == SCR_DBG_TILES_TOUCHED) { src = gv.tiles_touched; bytes = (size_t)P * 4; }
        else if (which == SCR_DBG_POINT_OFFSETS) { src = gv.point_offsets; bytes = (size_t)P * 4; }
        else if (which == SCR_DBG_RANGES) { src = gv.ranges; bytes = (size_t)g.tiles * 8; }
        else { src = gv.rec; bytes = (size_t)P * REC_F * 4; }
    } else if (which == SCR_DBG_POINT_LIST) {
        if (!binning_buf) return fail("binning_buf is NULL");
        src = bin_view((void*)binning_buf, I, 0).point_list;
        bytes = (size_t)I * 4;
    } else if (which == SCR_DBG_QMASK || which == SCR_DBG_GM_INDEX) {
        if (!binning_buf) return fail("binning_buf is NULL");
        BinView bv = bin_view((void*)binning_buf, I, 0);
        if (which == SCR_DBG_GM_INDEX && deep_lists(I, g.tiles))
            return fail("gm_index is not materialised for deep tile lists (I > 8192 per tile on average)");
        src = which == SCR_DBG_QMASK ? (const void*)bv.qmask : (const void*)bv.gm_index;
        bytes = which == SCR_DBG_QMASK ? (size_t)I : (size_t)I * 4;
    } else if (which == SCR_DBG_N_CONTRIB || which == SCR_DBG_FINAL_T) {
        if (!image_buf) return fail("image_buf is NULL");
        ImgView iv = img_view((void*)image_buf, H, W);
        src = which == SCR_DBG_N_CONTRIB ? (const void*)iv.n_contrib : (const void*)iv.final_T;
        bytes = (size_t)H * W * 4;
    } else {
        return fail("unknown debug selector %d", which);
    }
    if (bytes) HIP_TRY(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
}

int scr_copy_probe(const void* src, void* dst, size_t bytes, void* stream) {
    SCR_MARK_FN;
    if (!src || !dst || bytes < 16) return fail("NULL argument");
    const size_t n = bytes / 16;
    copy_probe_kernel<<<(unsigned)((n + 1023) / 1024), 256, 0, (hipStream_t)stream>>>((const copy_f4*)src, (copy_f4*)dst, n);
    CHECK_LAUNCH("copy_probe_kernel", 0, (hipStream_t)stream);
    return 0;
}

int scr_profile_enable(int mask) {
    g_prof_mask = mask < 0 ? 0xffffffffu : (unsigned)mask;
    memset(g_prof_seen, 0, sizeof(g_prof_seen));
    return 0;
}

int scr_profile_stride(int every) {
    if (every < 1) return fail("scr_profile_stride: every >= 1");
    g_prof_stride = (unsigned)every;
    memset(g_prof_seen, 0, sizeof(g_prof_seen));
    return 0;
}

int scr_profile_read(double* total_ms, int64_t* launches) {
    if (!total_ms || !launches) return fail("NULL argument");
    for (auto& r : g_prof_recs) {
        HIP_TRY(hipEventSynchronize(r.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        total_ms[r.idx] += ms;
        launches[r.idx] += 1;
        g_prof_pool.push_back(r.a);
        g_prof_pool.push_back(r.b);
    }
    g_prof_recs.clear();
    return 0;
}

const char* scr_profile_kernel_name(int idx) { return idx >= 0 && idx < SCR_PROF_COUNT ? kProfNames[idx] : ""; }

int scr_markers_enable(int on) {
    if (!on) { g_mark_on = false; return 0; }
    if (!g_roctx_push) {
        void* h = nullptr;
        for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (h && dlsym(h, "roctxRangePushA") && dlsym(h, "roctxRangePop")) break;
            h = nullptr;
        }
        if (!h) return fail("scr_markers_enable: no roctx library (librocprofiler-sdk-roctx.so / libroctx64.so) can be loaded");
        g_roctx_push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        g_roctx_pop = (int (*)())dlsym(h, "roctxRangePop");
    }
    g_mark_on = true;
    return 0;
}
int scr_marker_push(const char* name) {
    if (g_mark_on && name) (void)g_roctx_push(name);
    return 0;
}
int scr_marker_pop(void) {
    if (g_mark_on) (void)g_roctx_pop();
    return 0;
}

}  // extern "C"
