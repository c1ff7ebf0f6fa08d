// splatco_amd/csrc/capi.h -- what a file that defines C-ABI entry points (extern "C" scr_*) needs: the error return, the
// launch checks, the marker / timing scopes and, for the compaction plans, the mailbox.  Host only.  The state behind all of
// it (error string, event pool, roctx handles, the pinned mailboxes) is private to capi.hip.
#pragma once
#include "common.h"
#include "compact.h"

namespace scr {

// formats the calling thread's scr_last_error() text; returns 1
int fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail("%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// after a kernel launch: always catch launch errors; in debug mode also run it to completion
#define CHECK_LAUNCH(name, debug, st)                                                      \
    do {                                                                                   \
        hipError_t e_ = hipGetLastError();                                                 \
        if (e_ != hipSuccess) return fail("launch of %s failed: %s", name, hipGetErrorString(e_)); \
        if (debug) {                                                                       \
            e_ = hipStreamSynchronize(st);                                                 \
            if (e_ != hipSuccess) return fail("%s faulted: %s", name, hipGetErrorString(e_)); \
        }                                                                                  \
    } while (0)

// opt-in stage markers (scr_markers_enable): a roctx range on the calling thread
struct MarkScope {
    bool on;
    explicit MarkScope(const char* name);
    ~MarkScope();
};
#define SCR_MARK_FN MarkScope mark_fn_(__func__)

// opt-in kernel timing (scr_profile_*): a hipEvent pair on the launch stream around the launches of class `idx` (SCR_PROF_*)
struct ProfScope {
    bool on; hipStream_t st; int idx; hipEvent_t a, b; MarkScope mark;
    ProfScope(int idx, hipStream_t s);
    ~ProfScope();
};

// pinned host memory the GPU writes and the host polls (scr_forward_plan); per host thread, lives for the process
struct Mailbox {
    volatile unsigned long long* host = nullptr;
    unsigned long long* dev = nullptr;
    unsigned long long seq = 0;
};
Mailbox& mailbox();
// spin until the kernel(s) of this call have posted stamp `seq` (slot 1, and slot 3 when `two`); false when the
// stream finished without a visible post (caller falls back to a copy + stream synchronisation)
bool mailbox_wait(Mailbox& mb, unsigned long long seq, bool two, hipStream_t st);

// the plan half of a compaction (compact.h) of n items: `launch(scratch view, mailbox, stamp)` enqueues the count pass of
// kernel `name`, and the number of kept items comes back to *count_host
template <class Launch>
static int compact_plan(const char* name, int64_t n, void* scratch, int64_t* count_host, hipStream_t st, Launch launch) {
    if (!count_host || !scratch || n <= 0 || n >= (1ll << 31)) return fail("%s: bad plan arguments", name);
    const CompactScratch s = compact_scratch(scratch, n);
    Mailbox& mb = mailbox();
    const unsigned long long seq = ++mb.seq;
    launch(s, mb.dev, seq);
    CHECK_LAUNCH(name, 0, st);
    unsigned long long t = 0;
    if (mailbox_wait(mb, seq, false, st)) {
        t = mb.host[0];
    } else {
        HIP_TRY(hipMemcpyAsync(&t, s.total, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    *count_host = (int64_t)t;
    return 0;
}

}  // namespace scr
