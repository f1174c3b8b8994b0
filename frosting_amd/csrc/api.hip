// C ABI of libfrosting_rasterizer.so (include/frosting_rasterizer.h), the rasterizer: host-side
// orchestration of the forward / backward kernel sequence on the caller's HIP
// stream.  Mirrors the reference's Rasterizer::forward / backward control flow
// (rasterizer_impl.cu:198-336, :340-434) -- one blocking 48-byte read-back for
// num_rendered, everything else asynchronous.  The other entry points are in api_ops.hip.
#include "host_common.h"

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <initializer_list>
#include <mutex>
#include <optional>
#include <thread>

// ---- the error record ---------------------------------------------------------
static thread_local char g_err[512] = "";

int frg::fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

using frg::cpu_relax;
using frg::fail;

// ---- options ------------------------------------------------------------------
// the stages of frg_stage_times (option "profile_stage" names one)
enum { ST_PREPROCESS = 0, ST_SCAN, ST_SCATTER, ST_SORT, ST_BLEND_FWD, ST_BLEND_BWD, ST_PREPROCESS_BWD, ST_SH_COLOR, ST_COUNT };

// the options the launchers read (declared in kernels.h)
namespace frg {
std::atomic<int> g_rows_grid{0};
std::atomic<int> g_sort_heavy_on_caller{1};
std::atomic<int> g_fwd_prefetch{1};
std::atomic<int> g_fwd_order{1};
std::atomic<int> g_bwd_waves{0};
std::atomic<int> g_combine_blocks{0};   // 3, 6, 12 or 24 are the useful values; same results
}  // namespace frg

namespace {

std::atomic<int> g_exact_blend{-1};
std::atomic<int> g_profile{0};
std::atomic<int> g_profile_stage{-1};  // -1: every stage; k: only stage k gets events (each record costs ~3 us of stream time)
// Options below shape the FORWARD only.  What a backward needs to know about the forward that filled its
// buffers travels with those buffers: the carve of every field the backward reads depends on (P, W, H, R)
// alone, and the binning mode is stamped into the image chunk's counters (Counters::tight_binning).
std::atomic<int> g_global_bins{0};    // test hook: force the large-image (global-atomic) binning path
std::atomic<int> g_ablate{0};         // TIMING EXPERIMENTS ONLY: kernels skip parts of their work (results are wrong)
std::atomic<int> g_async_sh{0};       // SH colours on a side stream beside the binning stages (0: inside preprocess)
std::atomic<int> g_bwd_batch{3};      // tuning: instances per reduction step of the backward blend (2 | 3)
std::atomic<int> g_bwd_seg_log{0};    // 0: the backward blend's segment length by the frame's instance count (frg_common.h) | 8 .. 10: pinned
std::atomic<int> g_tight_binning{0};  // drop (Gaussian, tile) instances that cannot reach alpha >= 1/255 in the tile
// TIMING EXPERIMENTS ONLY (results are those of the previous frame's lists / slots): bit 0 launches the forward blend
// beside the sort, bit 1 the per-Gaussian backward beside the backward blend -- an upper bound on what overlapping
// a VALU-bound with an LDS- or HBM-bound stage can give before any dependency-respecting pipeline is built
std::atomic<int> g_probe{0};
// TEST HOOK (FROSTING_EXPERIMENTS=1): pretend every forward posted "no heavy waves", so that the backward skips the 16-wave
// launch of the per-Gaussian backward whatever the geometry holds -- the plain kernel's safety net must then do that work
std::atomic<int> g_assume_no_heavy{0};
std::atomic<int> g_use_mailbox{1};
std::atomic<int> g_sh_no_dir{0};           // option "sh_dir_in_backward"
std::atomic<int> g_fwd_unroll8{1};         // option "fwd_unroll8": 0 never | 1 frames of a few long lists (the host's rule) | 2 always
std::atomic<int> g_fused_small{1};         // option "fused_small": frames of at most 2^20 instances sort their short lists inside the forward blend
std::atomic<int> g_sparse_sh{1};            // option "sparse_sh": the SH pass over the visible Gaussians only, where a view sees a part of the model
std::atomic<int> g_bwd_heavy_first{1};
std::atomic<int> g_clear_image_state{0};   // 1: the memset in front of every forward, needed or not

// Every option of frg_set_option / frg_get_option: its name, where its value lives, what is stored for a requested value.
// Experiment knobs ("ablate" and "probe" make kernels skip work or ignore dependencies: WRONG results) can be set only in a
// process started with FROSTING_EXPERIMENTS=1, so that a stray call cannot switch them on, and do not answer frg_get_option.
struct Option {
    const char* name;
    std::atomic<int>* value;
    int (*stored)(int requested);
    bool experiment;
};
int as_flag(int v) { return v ? 1 : 0; }
int not_negative(int v) { return v < 0 ? 0 : v; }
const Option kOptions[] = {
    {"exact_blend", &g_exact_blend, as_flag, false},     // (unset until first asked for: FROSTING_EXACT_BLEND, exact_blend())
    {"profile", &g_profile, as_flag, false},
    {"profile_stage", &g_profile_stage, [](int v) { return v < 0 || v >= ST_COUNT ? -1 : v; }, false},
    {"global_bins", &g_global_bins, as_flag, false},
    {"tight_binning", &g_tight_binning, as_flag, false},
    {"bwd_batch", &g_bwd_batch, [](int v) { return v == 2 ? 2 : 3; }, false},
    {"bwd_seg_log", &g_bwd_seg_log, [](int v) { return v >= FRG_BWD_SEG_LOG_MIN && v <= FRG_BWD_SEG_LOG_MAX ? v : 0; }, false},
    {"counter_mailbox", &g_use_mailbox, as_flag, false},
    {"sparse_sh", &g_sparse_sh, as_flag, false},
    {"fwd_prefetch", &frg::g_fwd_prefetch, as_flag, false},
    {"bwd_heavy_first", &g_bwd_heavy_first, as_flag, false},
    {"bwd_waves", &frg::g_bwd_waves, not_negative, false},
    {"fwd_order", &frg::g_fwd_order, as_flag, false},
    {"sh_dir_in_backward", &g_sh_no_dir, as_flag, false},
    {"clear_image_state", &g_clear_image_state, as_flag, false},
    {"sort_heavy_on_caller", &frg::g_sort_heavy_on_caller, as_flag, false},
    {"async_sh", &g_async_sh, [](int v) { return v < 0 || v > 3 ? 1 : v; }, false},
    {"fused_small", &g_fused_small, as_flag, false},
    {"fwd_unroll8", &g_fwd_unroll8, [](int v) { return v < 0 || v > 2 ? 1 : v; }, false},
    {"combine_blocks", &frg::g_combine_blocks, not_negative, false},
    {"ablate", &g_ablate, [](int v) { return v; }, true},
    {"probe", &g_probe, [](int v) { return v; }, true},
    {"assume_no_heavy", &g_assume_no_heavy, as_flag, true},
    {"rows_grid", &frg::g_rows_grid, [](int v) { return v <= 0 ? 0 : v < 8 ? 8 : v; }, true},
};
const Option* find_option(const char* name)
{
    for (const Option& o : kOptions) if (name && strcmp(name, o.name) == 0) return &o;
    return nullptr;
}

int exact_blend()
{
    int v = g_exact_blend.load();
    if (v < 0) {
        const char* e = getenv("FROSTING_EXACT_BLEND");
        v = (e && e[0] == '1') ? 1 : 0;
        g_exact_blend.store(v);
    }
    return v;
}

// ---- stage timers -------------------------------------------------------------
// Optional per-stage GPU timing (frg_set_option("profile", 1)): hipEvents are
// recorded on the caller's stream between the kernels of one forward / backward;
// frg_stage_times() synchronises and returns the elapsed milliseconds.
// Event pairs are kept for the last ST_SLOTS launches of every stage and only read (and
// synchronised on) by frg_stage_times(), so timing a run of steps does not serialise them.
constexpr int ST_SLOTS = 64;
struct StageTimers {
    hipEvent_t ev[ST_COUNT][ST_SLOTS][2];
    unsigned launches[ST_COUNT];
    bool init = false;
    bool ensure()
    {
        if (init) return true;
        for (int i = 0; i < ST_COUNT; i++) {
            for (int k = 0; k < ST_SLOTS; k++) {
                if (hipEventCreate(&ev[i][k][0]) != hipSuccess || hipEventCreate(&ev[i][k][1]) != hipSuccess) return false;
            }
            launches[i] = 0;
        }
        init = true;
        return true;
    }
};
// One timer set per DEVICE, shared by every host thread (torch runs autograd backward on its engine
// thread: thread-local timers would never show the backward stages to the thread that asks for them).
constexpr int kMaxDevices = 16;
std::mutex g_timers_mu;
StageTimers g_timers[kMaxDevices];

struct StageScope {
    int id; hipStream_t s; bool on; int slot; int dev;
    StageScope(int id_, hipStream_t s_) : id(id_), s(s_), on(g_profile.load() != 0), slot(0), dev(-1)
    {
        const int only = g_profile_stage.load();
        if (only >= 0 && only != id) on = false;
        if (!on) return;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) { on = false; return; }
        std::lock_guard<std::mutex> lk(g_timers_mu);
        StageTimers& t = g_timers[dev];
        if (!t.ensure()) { on = false; return; }
        slot = (int)(t.launches[id] % ST_SLOTS);
        (void)hipEventRecord(t.ev[id][slot][0], s);
    }
    ~StageScope()
    {
        if (!on) return;
        std::lock_guard<std::mutex> lk(g_timers_mu);
        StageTimers& t = g_timers[dev];
        (void)hipEventRecord(t.ev[id][slot][1], s);
        t.launches[id]++;
    }
};

// ---- what the host keeps between calls, per thread and per process ------------
// One pinned landing pad per host thread for the counters read-back.
frg::Counters* pinned_counters()
{
    thread_local frg::Counters* p = nullptr;
    if (!p) {
        if (hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(frg::Counters), hipHostMallocDefault) != hipSuccess) p = nullptr;
    }
    return p;
}

// Deferred-counters forward: the counters of each outstanding forward land in a pinned slot
// behind an event; frg_forward_finish() waits on that event only (not on the whole stream).
// Per host thread: a deferred forward is finished by the thread that started it.
struct PendingCounters {
    frg::Counters* host = nullptr;     // pinned
    hipEvent_t ev = nullptr;           // counters have landed in `host`
    hipEvent_t scanned = nullptr;      // scan finished on the caller's stream
    hipStream_t copy_stream = nullptr; // carries the 48-byte read-back off the caller's stream
    const void* key = nullptr;      // image buffer of the forward; cleared by frg_forward_finish
    const void* last_key = nullptr; // ... kept: the next forward on the same buffer orders itself after the read-back
    int device = -1;
};
constexpr int kPendingSlots = 8;
struct PendingRing {
    PendingCounters slot[kPendingSlots];
    int next = 0;
    uint32_t last_class_count[FRG_SORT_CLASSES] = {0, 0, 0, 0, 0};
    bool have_hint = false;
    PendingCounters* acquire(const void* key, bool* reused)
    {
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess) return nullptr;
        PendingCounters* p = nullptr;
        for (auto& c : slot) if (c.last_key == key && c.ev && c.device == dev) p = &c;   // the same image buffer again
        *reused = p != nullptr;
        if (!p) { p = &slot[next]; next = (next + 1) % kPendingSlots; }
        if (!p->host && hipHostMalloc(reinterpret_cast<void**>(&p->host), sizeof(frg::Counters), hipHostMallocDefault) != hipSuccess) return nullptr;
        if (p->ev && p->device != dev) {
            (void)hipEventDestroy(p->ev); (void)hipEventDestroy(p->scanned); (void)hipStreamDestroy(p->copy_stream);
            p->ev = nullptr; p->scanned = nullptr; p->copy_stream = nullptr;
        }
        if (!p->ev && hipEventCreateWithFlags(&p->ev, hipEventDisableTiming) != hipSuccess) return nullptr;
        if (!p->scanned && hipEventCreateWithFlags(&p->scanned, hipEventDisableTiming) != hipSuccess) return nullptr;
        if (!p->copy_stream && hipStreamCreateWithFlags(&p->copy_stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
        p->device = dev;
        p->key = key;
        p->last_key = key;
        return p;
    }
    PendingCounters* find(const void* key)
    {
        for (auto& c : slot) if (c.key == key && c.ev) return &c;
        return nullptr;
    }
};
thread_local PendingRing g_pending;

// The host thread's mailbox (frg::Mailbox, frg_common.h): pinned, mapped, written by the scan workgroups.
struct HostMail {
    frg::Mailbox* host = nullptr;
    uint32_t seq = 0;
    bool long_lists = false;     // the previous forward of this thread had tile lists beyond the LDS sort
    int last_P = 0; uint32_t last_seq = 0;      // the forward whose scatter post may still be in the mailbox
    // the previous forward of this thread, on a model of the same size, saw less than three quarters of it
    bool sparse_view(int P) const
    {
        if (!host || P != last_P || (uint32_t)(__atomic_load_n(&host->heavy_post, __ATOMIC_ACQUIRE) >> 32) != last_seq) return false;
        return (uint64_t)host->visible * 4u < (uint64_t)P * 3u;
    }
    bool failed = false;         // a post never arrived although the stream had drained: stay with the copy + synchronise
    frg::Mailbox* get()
    {
        if (!host && !failed) {
            if (hipHostMalloc(reinterpret_cast<void**>(&host), sizeof(frg::Mailbox), hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) {
                host = nullptr; failed = true;
                (void)hipGetLastError();
            } else memset(host, 0, sizeof(frg::Mailbox));
        }
        return host;
    }
};
thread_local HostMail g_mail;

// What the host remembers about the forward that last filled a geometry buffer (process-wide: autograd runs the backward
// on another thread than the forward): which mailbox post is its scatter's, how many instances it rendered, whether it was
// told that no backward follows.  Scheduling hints and early refusals only -- keyed by ADDRESS, a note can be stale (a buffer
// copied to an address an earlier forward used), so nothing that decides a gradient bit hangs on one: the blend arithmetic
// and "nothing kept" are stamped into the image chunk by the forward's blend kernel (Counters::fwd_flags) and read there
// (settle_forward_stamp); so is "the SH directions were rotated" (a note's `rotated` only decides whether the stamp is read).  A ring of kFwdNotes entries (the entry of the same address is overwritten, else the next ring
// slot); a forgotten forward's note reads "unknown" everywhere (rendered -1, forward_only settled by the stamp, both forms
// of the per-Gaussian backward launched as if nothing had been posted).  The pinned mailboxes are never freed.
struct FwdNote {
    const void* geom = nullptr; const frg::Mailbox* mail = nullptr; uint32_t seq = 0; int exact = -1; int rendered = -1; bool fwd_only = false;
    bool rotated = false;     // frg_forward_args::sh_rotations was given (the stamp: FRG_FWD_ROTATED)
    // -> the number of heavy waves the forward's scatter posted, or -1 when unknown (no post, not arrived yet, the mailbox
    // already belongs to a later forward)
    int heavy_waves_posted() const
    {
        if (!mail || !g_use_mailbox.load(std::memory_order_relaxed)) return -1;
        // The forward returned when the scan stage was through; the scatter posts as its first act.  A backward called
        // straight away may be a few microseconds early: it waits that long (the GPU has the rest of the forward ahead of
        // it, the host nothing better to do), but not for a scatter stuck behind other work.
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spin = 0;; spin++) {
            const unsigned long long post = __atomic_load_n(&mail->heavy_post, __ATOMIC_ACQUIRE);    // (sequence << 32) | count, one word
            const uint32_t cur = (uint32_t)(post >> 32);
            if (cur == seq) return (int)((uint32_t)post > 0x7fffffffu ? 0x7fffffffu : (uint32_t)post);
            if ((int32_t)(cur - seq) > 0) return -1;      // the mailbox already carries a later forward's post
            if ((spin & 63u) == 63u && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(40)) return -1;
            cpu_relax();
        }
    }
};
class FwdNotes {
    static constexpr int kFwdNotes = 1024;
    std::mutex mu;
    FwdNote ring[kFwdNotes];
    unsigned next = 0;
    FwdNote* locate(const void* geom)
    {
        for (auto& n : ring) if (n.geom == geom) return &n;
        return nullptr;
    }
public:
    // a forward starts on `geom`: whatever an earlier forward posted about this buffer is void now
    void begin(const void* geom, int exact, bool fwd_only, bool rotated)
    {
        std::lock_guard<std::mutex> lk(mu);
        FwdNote* n = locate(geom);
        *(n ? n : &ring[next++ % kFwdNotes]) = FwdNote{geom, nullptr, 0, exact, -1, fwd_only, rotated};
    }
    // the forward on `geom` learnt something (its instance count, its scatter's mailbox post); a forgotten forward learns nothing
    template <class Fn>
    void update(const void* geom, Fn fn)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (FwdNote* n = locate(geom)) fn(*n);
    }
    // -> a copy of the note of the forward that last filled `geom`; nothing when that forward is not remembered
    std::optional<FwdNote> find(const void* geom)
    {
        std::lock_guard<std::mutex> lk(mu);
        const FwdNote* n = locate(geom);
        return n ? std::optional<FwdNote>(*n) : std::nullopt;
    }
};
FwdNotes g_fwd_notes;

// Two-call backward (frg_backward_args::phase): phase 2 reads the nine per-Gaussian sums phase 1 left in the workspace.
// What phase 1 was called with is remembered per workspace pointer (process-wide, a ring of kPhaseNotes); a phase 2 that
// does not match (an arena that grew or was reused between the calls, another frame's buffers) is refused instead of
// producing garbage gradients.  A note decides that refusal and nothing else.
class PhaseNotes {
    struct Note { const void* workspace = nullptr; const void* geom = nullptr; const void* image = nullptr; int P = 0, R = 0; bool rotated = false; };
    static constexpr int kPhaseNotes = 16;
    std::mutex mu;
    Note ring[kPhaseNotes];
    unsigned next = 0;
public:
    // phase 1 ran on `workspace`
    void record(const void* workspace, const void* geom, const void* image, int P, int R, bool rotated)
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto& n : ring) if (n.workspace == workspace) { n = Note{workspace, geom, image, P, R, rotated}; return; }
        ring[next++ % kPhaseNotes] = Note{workspace, geom, image, P, R, rotated};
    }
    // -> phase 1 ran on `workspace` with these arguments; the sums are consumed once
    bool consume(const void* workspace, const void* geom, const void* image, int P, int R)
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto& n : ring)
            if (n.workspace == workspace) {
                const bool ok = n.geom == geom && n.image == image && n.P == P && n.R == R;
                n = Note{};
                return ok;
            }
        return false;
    }
    // -> the phase 1 that last ran on `workspace` (and was not consumed yet) was called with sh_rotations
    bool rotated(const void* workspace)
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto& n : ring) if (n.workspace == workspace) return n.rotated;
        return false;
    }
};
PhaseNotes g_phase_notes;

// Side streams (frg::SideStream, kernels.h), one per host thread each:
// the deferred SH colour kernel's (fork: the geometry is there | join: the colours are).  Lowest priority: the colour
// kernel floods every CU with streaming waves; the small latency-bound kernels of the binning stages on the caller's
// stream must win the arbitration
thread_local frg::SideStream g_sh_side{frg::SideStream::LOWEST};
// the timing experiments' ("probe")
thread_local frg::SideStream g_probe_side{frg::SideStream::DEFAULT};
// the per-Gaussian backward's 16-wave launch's.  HIGHEST priority: the 16-wave workgroups need a whole CU's LDS each; both
// launches become ready when the blend backward ends, and unless the dispatcher places these first they wait until the
// plain kernel has drained (rocprofv3, round 3: 274 us "duration" for a launch whose workgroups found an empty list)
thread_local frg::SideStream g_bwd_side{frg::SideStream::HIGHEST};

// ---- helpers of both directions -----------------------------------------------
// Spin until the kernel's post arrives.  false: the stream failed, or it drained without the post becoming visible.
bool mailbox_wait(const uint32_t* flag, uint32_t seq, hipStream_t stream)
{
    for (unsigned spin = 1;; spin++) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return true;
        if ((spin & 0x7ffu) == 0) {
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess) return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq;
            if (q != hipErrorNotReady) return false;
        }
        // a long wait (a 3 M-Gaussian preprocess is ~0.25 ms ahead of the first post): after the first ~10 us give the core
        // to whoever else wants it (data loaders, the other ranks' host threads on a busy node) between looks
        if (spin > 4096 && (spin & 63u) == 0) std::this_thread::yield();
        cpu_relax();
    }
}

// debug mode: synchronise after every stage so a faulting kernel is attributed
// (the reference's CHECK_CUDA, auxiliary.h:166-173)
#define FRG_STAGE(call, name)                                                                               \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        if (e_ == hipSuccess && debug) e_ = hipStreamSynchronize(stream);                                   \
        if (e_ != hipSuccess) return fail(FRG_EHIP, "stage '%s' failed: %s", name, hipGetErrorString(e_)); \
    } while (0)

// Modes of one forward: each is the per-call value of frg_forward_args when given, else the process-wide option.
struct FwdModes {
    int exact, tight, async_sh;
    int fwd_only = 0;     // frg_forward_args::forward_only (per call only: there is no process-wide form)
    static int pick(int field, int max_value, int fallback) { return field >= 1 && field <= max_value + 1 ? field - 1 : fallback; }
};
FwdModes default_modes() { return FwdModes{exact_blend(), g_tight_binning.load(), g_async_sh.load(), 0}; }

frg::ViewParams make_view(int D, int M, int width, int height, float tan_fovx, float tan_fovy, float scale_modifier, int tight)
{
    frg::ViewParams vp;
    vp.tan_fovx = tan_fovx; vp.tan_fovy = tan_fovy;
    vp.focal_y = height / (2.0f * tan_fovy);  // rasterizer_impl.cu:222-223
    vp.focal_x = width / (2.0f * tan_fovx);
    vp.scale_modifier = scale_modifier;
    vp.W = width; vp.H = height;
    vp.gx = (width + FRG_TILE - 1) / FRG_TILE; vp.gy = (height + FRG_TILE - 1) / FRG_TILE;
    vp.D = D; vp.M = M;
    vp.tight = tight;
    vp.sparse_sh = 0;
    vp.sh_no_dir = 0;
    return vp;
}

// frg_forward_args / frg_backward_args grew field by field: a caller built against an earlier header states a smaller
// struct_size.  One of the accepted generation sizes: *full <- the caller's bytes, the fields it does not know zeroed --
// every field added after the first generation reads 0 / NULL as "absent / the process default / one call".
template <class Args>
bool widen(const Args* a, std::initializer_list<size_t> generations, Args* full)
{
    if (!a || std::find(generations.begin(), generations.end(), a->struct_size) == generations.end()) return false;
    *full = Args{};
    memcpy(full, a, a->struct_size);
    return true;
}

// the raw-parameter fields, named alike in frg_forward_args and frg_backward_args
template <class Args>
frg::RawInputs raw_inputs_of(const Args& a)
{
    frg::RawInputs rw;
    rw.raw_opacity = a.raw_opacities; rw.raw_scale = a.raw_scales; rw.raw_rot = a.raw_rotations;
    rw.shell_logits = a.shell_logits; rw.shell_verts = a.shell_cell_verts; rw.shell_cells = a.shell_cells;
    rw.bary_mode = a.shell_bary_mode;
    return rw;
}

// ---- forward ------------------------------------------------------------------
// The argument checks of a forward, in the order their messages are promised.  An empty model (P == 0) needs nothing
// beyond sizes and out_color: the checks behind that line are not made for it.
int validate_forward(const frg_forward_args& a)
{
    if (a.instance_capacity < 0) return fail(FRG_EINVAL, "instance_capacity < 0");
    if (a.forward_only < 0 || a.forward_only > 1) return fail(FRG_EINVAL, "frg_forward_args: forward_only must be 0 or 1");
    if (a.forward_only && a.instance_capacity > 0)
        return fail(FRG_EINVAL, "frg_forward_args: forward_only with deferred counters (instance_capacity > 0) is not offered");
    if (a.exact_blend < 0 || a.exact_blend > 2 || a.tight_binning < 0 || a.tight_binning > 2 || a.async_sh < 0 ||
        a.async_sh > 4 || a.shell_bary_mode < 0 || a.shell_bary_mode > 1)
        return fail(FRG_EINVAL, "frg_forward_args: mode out of range (exact_blend %d, tight_binning %d, async_sh %d, shell_bary_mode %d)",
                    a.exact_blend, a.tight_binning, a.async_sh, a.shell_bary_mode);
    if (a.P < 0 || a.width <= 0 || a.height <= 0) return fail(FRG_EINVAL, "bad sizes P=%d W=%d H=%d", a.P, a.width, a.height);
    if (!a.out_color) return fail(FRG_EINVAL, "out_color is null");
    if (a.P == 0) return FRG_OK;
    if (!a.viewmatrix || !a.projmatrix || !a.cam_pos || !a.background) return fail(FRG_EINVAL, "null required pointer");
    if ((a.means3D == nullptr) == (a.shell_logits == nullptr))
        return fail(FRG_EINVAL, "provide exactly one of means3D / shell_logits");
    if (a.shell_logits && (!a.shell_cell_verts || !a.shell_cells))
        return fail(FRG_EINVAL, "shell_logits needs shell_cell_verts and shell_cells");
    if ((a.opacities == nullptr) == (a.raw_opacities == nullptr))
        return fail(FRG_EINVAL, "provide exactly one of opacities / raw_opacities");
    if (a.sh_rotations && (!a.shs || a.colors_precomp))
        return fail(FRG_EINVAL, "sh_rotations rotate the directions of the SH colour: they come with shs, not with colors_precomp");
    if ((a.shs == nullptr) == (a.colors_precomp == nullptr))
        return fail(FRG_EINVAL, "provide exactly one of shs / colors_precomp");
    if ((a.raw_scales == nullptr) != (a.raw_rotations == nullptr))
        return fail(FRG_EINVAL, "raw_scales and raw_rotations come together");
    const bool have_sr = (a.scales && a.rotations) || a.raw_scales;
    if ((a.scales || a.rotations) && a.raw_scales) return fail(FRG_EINVAL, "provide (scales, rotations) or their raw forms, not both");
    if (((a.scales == nullptr) != (a.rotations == nullptr)) || have_sr == (a.cov3D_precomp != nullptr))
        return fail(FRG_EINVAL, "provide exactly one of (scales, rotations) / cov3D_precomp");
    if (a.shs && (a.D < 0 || a.D > 3 || a.M < (a.D + 1) * (a.D + 1)))
        return fail(FRG_EINVAL, "SH degree %d needs %d coefficients, got M=%d", a.D, (a.D + 1) * (a.D + 1), a.M);
    if (!a.geometry_alloc || !a.binning_alloc || !a.image_alloc) return fail(FRG_EINVAL, "null allocation callback");
    return FRG_OK;
}

struct FwdCtx;
// SH colours: nothing before the blend needs them, and the stages in between (scan, scatter, sort) leave the
// HBM nearly idle -- the colour kernel (the largest single stream of the forward, 192 B per visible Gaussian)
// runs beside them on this thread's side stream (g_sh_side); the blend joins it.  An error return between the fork
// and the join must not leave the side kernel running on the caller's inputs: the destructor waits for it.
class ShFork {
    int mode = 0;      // 0 inside preprocess | side stream forked after: 1 preprocess, 2 scan, 3 scatter
    bool forked = false, joined = false;
public:
    ShFork() = default;
    ShFork(const ShFork&) = delete;
    ~ShFork() { if (forked && !joined) (void)hipStreamSynchronize(g_sh_side.stream); }
    void arm(int sh_mode) { mode = sh_mode != 0 && g_sh_side.ensure() ? sh_mode : 0; }
    bool deferred() const { return mode != 0; }
    // stage `at` has been enqueued: launches the colour kernel if this is the stage it was to follow (at the latest after the scatter)
    int fork(int at, const FwdCtx& x);
    // the caller's stream waits for the colours
    int join(hipStream_t stream)
    {
        if (!deferred()) return FRG_OK;
        FRG_HIP(hipStreamWaitEvent(stream, g_sh_side.join, 0));
        joined = true;
        return FRG_OK;
    }
};

// What the steps of one forward share.
struct FwdCtx {
    const frg_forward_args& a;
    FwdModes md;
    int debug;            // (deferred counters: no synchronisation, the stage-by-stage one included)
    int seg_forced;       // option "bwd_seg_log", read once: the size asked of the callback and the carve must agree
    hipStream_t stream;
    frg::ViewParams vp;
    int T, index_bits;    // tiles | bits needed for a Gaussian index
    char *geom_chunk, *img_chunk;
    frg::GeomState g;
    frg::ImageState img;
    int* radii;
    frg::FwdInputs in;
    ShFork sh;
    // the binning chunk of R instances whose longest tile list has `longest` entries, from the caller's callback
    int alloc_binning(int R, int longest, frg::BinningState* b) const
    {
        char* bin_chunk = a.binning_alloc(a.user, frg::BinningState::carve(nullptr, R, longest, seg_forced).bytes);
        if (!bin_chunk) return fail(FRG_EALLOC, "binning allocation callback returned null");
        *b = frg::BinningState::carve(bin_chunk, R, longest, seg_forced);
        return FRG_OK;
    }
    hipError_t blend(const frg::BinningState& b, bool fwd_only, bool fused_sort, bool long_lists) const
    {
        return (md.exact ? frg::launch_blend_fwd_exact : frg::launch_blend_fwd_fast)(vp, g, img, b, a.background, a.out_color, stream, fwd_only,
                                                                                     fused_sort, long_lists);
    }
};

int ShFork::fork(int at, const FwdCtx& x)
{
    if (!deferred() || forked || (at < mode && at < 3)) return FRG_OK;
    forked = true;
    FRG_HIP(g_sh_side.fork_from(x.stream));
    {
        StageScope sc_(ST_SH_COLOR, g_sh_side.stream);
        FRG_HIP(frg::launch_sh_color(x.a.P, x.vp, x.in, x.radii, x.g, g_sh_side.stream));
    }
    FRG_HIP(hipEventRecord(g_sh_side.join, g_sh_side.stream));
    if (x.debug) FRG_HIP(hipStreamSynchronize(g_sh_side.stream));
    return FRG_OK;
}

// LDS-bins paths: nothing of the image chunk needs clearing in front of the forward -- colsum_kernel zeroes the
// scatter cursors and the blend's depth marks on its way, every counter is written unconditionally; only the flag
// of the prefiltered assertion is set-only.  Global bins (more tiles than the LDS holds): the per-tile counts are
// accumulated with atomics, the whole region is cleared.
int clear_image_state(const FwdCtx& x)
{
    const frg::ImageState& img = x.img;
    if (!img.lds_bins || g_clear_image_state.load(std::memory_order_relaxed)) FRG_HIP(hipMemsetAsync(x.img_chunk + img.zero_begin, 0, img.zero_bytes, x.stream));
    else if (x.a.prefiltered || x.a.instance_capacity > 0) FRG_HIP(hipMemsetAsync(&img.counters->filtered, 0, sizeof(uint32_t), x.stream));   // (deferred: frg_forward_finish is told `prefiltered` again)
    return FRG_OK;
}

int stage_preprocess(FwdCtx& x)
{
    const int debug = x.debug;
    hipStream_t stream = x.stream;
    { StageScope sc_(ST_PREPROCESS, stream); FRG_STAGE(frg::launch_preprocess_fwd(x.a.P, x.vp, x.in, x.radii, x.g, x.img, x.a.prefiltered, x.sh.deferred(), stream), "preprocess"); }
    return x.sh.fork(1, x);
}

// mail (optional): where the scan workgroups post the counters for the polling host thread
int stage_scan(FwdCtx& x, frg::Mailbox* mail, uint32_t mail_seq)
{
    const int debug = x.debug;
    hipStream_t stream = x.stream;
    { StageScope sc_(ST_SCAN, stream); FRG_STAGE(frg::launch_scan(x.a.P, x.vp, x.g, x.img, (uint32_t)x.a.instance_capacity, stream, mail, mail_seq), "scan"); }
    return x.sh.fork(2, x);
}

// instance_capacity > 0: no host synchronisation at all -- the binning buffer is sized for `capacity` instances up
// front, launches that depend on the counters use device-side values, and the counters travel to a pinned slot that
// frg_forward_finish() inspects later.  Everything is enqueued without knowing R on the host; the 48-byte read-back
// rides a side stream so that no later kernel queues behind it.
int forward_deferred(FwdCtx& x)
{
    const int capacity = x.a.instance_capacity, debug = x.debug, T = x.T;
    hipStream_t stream = x.stream;
    const frg::ImageState& img = x.img;
    bool reused = false;
    PendingCounters* pend = g_pending.acquire(x.img_chunk, &reused);
    if (!pend) return fail(FRG_EHIP, "pinned counter slot / event creation failed");
    // the previous deferred forward on this image buffer reads its counters back on a side stream:
    // that copy must have happened before the counters are cleared again
    if (reused) FRG_HIP(hipStreamWaitEvent(stream, pend->ev, 0));
    FRG_TRY(clear_image_state(x));
    FRG_TRY(stage_preprocess(x));
    FRG_TRY(stage_scan(x, nullptr, 0));
    FRG_HIP(hipEventRecord(pend->scanned, stream));
    FRG_HIP(hipStreamWaitEvent(pend->copy_stream, pend->scanned, 0));
    FRG_HIP(hipMemcpyAsync(pend->host, img.counters, sizeof(frg::Counters), hipMemcpyDeviceToHost, pend->copy_stream));
    FRG_HIP(hipEventRecord(pend->ev, pend->copy_stream));
    frg::BinningState b;
    FRG_TRY(x.alloc_binning(capacity, FRG_SORT_LDS_CAP + 1, &b));
    FRG_STAGE(frg::launch_sort_plan(T, nullptr, img.counters->class_count, img.class_tiles, img.ranges, b.big_plan, (uint32_t)capacity, stream), "sort plan");
    { StageScope sc_(ST_SCATTER, stream); FRG_STAGE(frg::launch_scatter(x.a.P, x.vp, x.radii, x.g, img, b, stream, g_ablate.load()), "scatter"); }
    FRG_TRY(x.sh.fork(3, x));
    { StageScope sc_(ST_SORT, stream); FRG_STAGE(frg::launch_tile_sort(T, nullptr, g_pending.have_hint ? g_pending.last_class_count : nullptr, img.counters->class_count, img.class_tiles, img.ranges, b.pairs, b.pairs_tmp, b.big_hist, b.big_plan, (uint32_t)capacity, 0, x.index_bits, b.point_list, stream), "sort"); }
    FRG_TRY(x.sh.join(stream));
    StageScope sc_(ST_BLEND_FWD, stream);
    FRG_STAGE(x.blend(b, false, false, false), "blend");
    return capacity;
}

// The mailbox's first post said how many instances the frame has: the binning buffer is sized for every sort path -- the
// longest tile list is not known yet -- and the scatter is enqueued while the reorder still runs.
int scatter_early(FwdCtx& x, int R, frg::Mailbox* mail, uint32_t mail_seq, frg::BinningState* b)
{
    const int debug = x.debug;
    hipStream_t stream = x.stream;
    const frg::ImageState& img = x.img;
    FRG_TRY(x.alloc_binning(R, FRG_SORT_LDS_CAP + 1, b));
    if (g_mail.long_lists)
        FRG_STAGE(frg::launch_sort_plan(x.T, nullptr, img.counters->class_count, img.class_tiles, img.ranges, b->big_plan, (uint32_t)R, stream, 1), "sort plan");
    { StageScope sc_(ST_SCATTER, stream); FRG_STAGE(frg::launch_scatter(x.a.P, x.vp, x.radii, x.g, img, *b, stream, g_ablate.load(), mail, mail_seq), "scatter"); }
    FRG_TRY(x.sh.fork(3, x));
    g_fwd_notes.update(x.geom_chunk, [&](FwdNote& n) { n.mail = mail; n.seq = mail_seq; });
    g_mail.last_P = x.a.P; g_mail.last_seq = mail_seq;
    return FRG_OK;
}

// The one place that yields the host's copy of a blocking forward's counters: the mailbox's second post (the tile scan's;
// `first_post` tells whether its first one arrived), else the pinned copy + stream synchronisation.  A mailbox whose post
// did not arrive is marked failed: this thread stays with the copy from then on.
int read_counters(const FwdCtx& x, const frg::Mailbox* mail, uint32_t mail_seq, bool first_post, frg::Counters* c)
{
    if (mail) {
        if (first_post && mailbox_wait(&mail->seq_c, mail_seq, x.stream)) { *c = mail->c; return FRG_OK; }
        g_mail.failed = true, g_mail.host = nullptr;    // (the pinned block is left to the process)
    }
    frg::Counters* host = pinned_counters();
    if (!host) return fail(FRG_EHIP, "hipHostMalloc failed");
    FRG_HIP(hipMemcpyAsync(host, x.img.counters, sizeof(frg::Counters), hipMemcpyDeviceToHost, x.stream));
    FRG_HIP(hipStreamSynchronize(x.stream));
    *c = *host;
    return FRG_OK;
}

// small frames (at most 2^20 instances: C2 has 350 000 in 2 500 lists of 140): the lists of up to 512 entries are sorted by the
// forward blend's own workgroups (blend_impl.h FUSED) -- one launch and the point_list round trip less in a step that is a
// chain of short launches; the longest-first tile order (class lists) is what the fused form walks
bool fused_small_sort(int R, int option, int fwd_order, int probe)
{
    return option != 0 && R > 0 && R <= (1 << 20) && fwd_order != 0 && !(probe & 1);
}

// A frame that does not fill the GPU (fewer than 1280 instances per tile of the image on average) and whose longest list
// is several times its mean list -- the limb of a shell seen from outside (C4: 792 per tile, 6 267 against a mean of
// 1 366 over the active tiles) -- walks eight entries per trip: its launch is stall-bound inside the waves of its long
// tiles (0.240 -> 0.222 ms).  A full frame is bound by instruction issue and keeps four, uniform (C3: 0.203 -> 0.243 with
// eight) or clustered (the skew scene, 2 670 per tile: 0.186 -> 0.218).  Same bits either way.  (option: "fwd_unroll8")
bool eight_entries_per_trip(const frg::Counters& c, int R, int T, int option)
{
    if (R <= 0 || option == 0) return false;
    uint32_t active = 0;
    for (int k = 0; k < FRG_SORT_CLASSES; k++) active += c.class_count[k];
    return option == 2 || ((double)(int)c.max_tile_count >= 3.5 * (double)R / (double)(active ? active : 1u) && (double)R < 1280.0 * (double)T);
}

// instance_capacity == 0: the reference's flow, one blocking read of the counters between scan and scatter.  The scan
// workgroups post the counters into this thread's pinned mailbox (frg_common.h) and the host polls it, instead of a copy
// kernel + stream synchronisation behind the scan.  First post: the instance count (by the chunk scan, ~40 us before the
// scan stage ends at C3) -- the scatter goes out on it.  Second post: the tile scan's counters (the sort's grids).
int forward_blocking(FwdCtx& x)
{
    const frg_forward_args& a = x.a;
    const int P = a.P, debug = x.debug, T = x.T;
    hipStream_t stream = x.stream;
    const frg::ImageState& img = x.img;
    FRG_TRY(clear_image_state(x));
    FRG_TRY(stage_preprocess(x));
    frg::Mailbox* mail = (!debug && g_use_mailbox.load(std::memory_order_relaxed)) ? g_mail.get() : nullptr;
    uint32_t mail_seq = 0;
    if (mail) { if (++g_mail.seq == 0) g_mail.seq = 1; mail_seq = g_mail.seq; }
    FRG_TRY(stage_scan(x, mail, mail_seq));

    // the single host synchronisation of the op (rasterizer_impl.cu:280-281)
    frg::BinningState b;
    bool early = false;
    const bool first_post = mail && mailbox_wait(&mail->seq_r, mail_seq, stream);
    if (first_post) {
        const uint32_t r = mail->num_rendered;
        if (r > 0x7fffffffu) return fail(FRG_EINVAL, "num_rendered overflows int32");
        if (r > 0) { FRG_TRY(scatter_early(x, (int)r, mail, mail_seq, &b)); early = true; }
    }
    frg::Counters c;
    FRG_TRY(read_counters(x, mail, mail_seq, first_post, &c));
    if (a.prefiltered && c.filtered)
        return fail(FRG_EFILTER, "Point is filtered although prefiltered is set. This shouldn't happen!");
    if (c.num_rendered > 0x7fffffffu) return fail(FRG_EINVAL, "num_rendered overflows int32");
    const int R = (int)c.num_rendered, max_tile = (int)c.max_tile_count;
    g_fwd_notes.update(x.geom_chunk, [&](FwdNote& n) { n.rendered = R; });      // (a deferred forward does not know)

    if (!early) FRG_TRY(x.alloc_binning(R, max_tile, &b));
    const bool forked_plan = early && g_mail.long_lists;
    if (mail) g_mail.long_lists = c.class_count[4] > 0;
    const bool fused_small = fused_small_sort(R, g_fused_small.load(), frg::g_fwd_order.load(), g_probe.load());
    const bool probe_fwd = (g_probe.load() & 1) && R > 0 && !x.md.exact && g_probe_side.ensure();
    if (R > 0) {
        FRG_STAGE(frg::launch_sort_plan(T, c.class_count, img.counters->class_count, img.class_tiles, img.ranges, b.big_plan, (uint32_t)R, stream, forked_plan ? 2 : 0), "sort plan");
        if (!early) {
            { StageScope sc_(ST_SCATTER, stream); FRG_STAGE(frg::launch_scatter(P, x.vp, x.radii, x.g, img, b, stream, g_ablate.load()), "scatter"); }
            FRG_TRY(x.sh.fork(3, x));
        }
        if (probe_fwd) {
            FRG_HIP(g_probe_side.fork_from(stream));
            FRG_HIP(frg::launch_blend_fwd_fast(x.vp, x.g, img, b, a.background, a.out_color, g_probe_side.stream));
            FRG_HIP(hipEventRecord(g_probe_side.join, g_probe_side.stream));
        }
        { StageScope sc_(ST_SORT, stream); FRG_STAGE(frg::launch_tile_sort(T, c.class_count, nullptr, img.counters->class_count, img.class_tiles, img.ranges, b.pairs, b.pairs_tmp, b.big_hist, b.big_plan, (uint32_t)R, max_tile, x.index_bits, b.point_list, stream, fused_small), "sort"); }
        if (probe_fwd) { FRG_HIP(hipStreamWaitEvent(stream, g_probe_side.join, 0)); return R; }
    } else {
        // point_offsets must still be defined for backward
        FRG_STAGE(frg::launch_scatter(P, x.vp, x.radii, x.g, img, b, stream), "scatter");
        FRG_TRY(x.sh.fork(3, x));
    }
    FRG_TRY(x.sh.join(stream));
    StageScope sc_(ST_BLEND_FWD, stream);
    FRG_STAGE(x.blend(b, x.md.fwd_only != 0, fused_small, eight_entries_per_trip(c, R, T, g_fwd_unroll8.load())), "blend");
    return R;
}

// Validates, asks the caller for the geometry and image chunks, then runs one of the two flows.  -> num_rendered
// (deferred: the capacity) or a negative error code.
int forward_impl(const frg_forward_args& a)
{
    FRG_TRY(validate_forward(a));
    hipStream_t stream = (hipStream_t)a.hip_stream;
    if (a.P == 0) {  // rasterize_points.cu:68,81: zero image, background not applied
        FRG_HIP(hipMemsetAsync(a.out_color, 0, (size_t)3 * a.width * a.height * sizeof(float), stream));
        return 0;
    }
    FwdCtx x{a};
    x.md = default_modes();
    x.md.exact = FwdModes::pick(a.exact_blend, 1, x.md.exact);
    x.md.tight = FwdModes::pick(a.tight_binning, 1, x.md.tight);
    x.md.async_sh = FwdModes::pick(a.async_sh, 3, x.md.async_sh);
    x.md.fwd_only = a.forward_only;
    x.debug = a.instance_capacity > 0 ? 0 : a.debug;
    x.seg_forced = g_bwd_seg_log.load();
    x.stream = stream;
    x.vp = make_view(a.D, a.M, a.width, a.height, a.tan_fovx, a.tan_fovy, a.scale_modifier, x.md.tight);
    // Will this view see only a part of the model?  With an occlusion mask: yes.  Otherwise: what the previous forward of
    // this thread saw (posted by its scatter) -- the SH pass then streams the rows of the visible Gaussians only.
    x.vp.sparse_sh = g_sparse_sh.load(std::memory_order_relaxed) && (a.keep_mask != nullptr || g_mail.sparse_view(a.P));
    x.vp.sh_no_dir = (g_sh_no_dir.load(std::memory_order_relaxed) || x.md.fwd_only) ? 1 : 0;
    x.T = x.vp.gx * x.vp.gy;
    x.index_bits = 1;
    while (x.index_bits < 32 && (1u << x.index_bits) < (uint32_t)a.P) x.index_bits++;

    x.geom_chunk = a.geometry_alloc(a.user, frg_geometry_bytes(a.P));
    x.img_chunk = a.image_alloc(a.user, frg_image_bytes(a.width, a.height));
    if (!x.geom_chunk || !x.img_chunk) return fail(FRG_EALLOC, "allocation callback returned null");
    g_fwd_notes.begin(x.geom_chunk, x.md.exact, x.md.fwd_only != 0, a.sh_rotations != nullptr);
    x.g = frg::GeomState::carve(x.geom_chunk, a.P);
    x.img = frg::ImageState::carve(x.img_chunk, a.width, a.height, g_global_bins.load() != 0);
    x.radii = a.radii ? a.radii : x.g.internal_radii;   // rasterizer_impl.cu:228-231
    x.in = frg::FwdInputs{a.means3D, a.scales, a.rotations, a.opacities, a.shs, a.cov3D_precomp, a.colors_precomp, a.viewmatrix, a.projmatrix, a.cam_pos};
    x.in.keep_mask = a.keep_mask;
    x.in.raw = raw_inputs_of(a);
    x.in.sh_rotations = a.sh_rotations;
    x.sh.arm((a.shs != nullptr && !a.shell_logits) ? x.md.async_sh : 0);
    return a.instance_capacity > 0 ? forward_deferred(x) : forward_blocking(x);
}

// the positional parameters of frg_forward / frg_forward_deferred are the struct's fields up to radii, in its order, and
// hip_stream; debug and the later fields stay 0 / NULL: absent
frg_forward_args positional_forward_args(frg_alloc_fn geometry_alloc, frg_alloc_fn binning_alloc, frg_alloc_fn image_alloc, void* user,
                                         int P, int D, int M, const float* background, int width, int height,
                                         const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                                         const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                         const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                                         float tan_fovx, float tan_fovy, int prefiltered, float* out_color, int* radii, void* hip_stream)
{
    return frg_forward_args{sizeof(frg_forward_args), geometry_alloc, binning_alloc, image_alloc, user, P, D, M, background,
                            width, height, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations,
                            cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, out_color,
                            radii, /* debug */ 0, hip_stream};
}

// ---- backward -----------------------------------------------------------------
// The argument checks of a backward up to its workspace, in the order their messages are promised (those of the phase
// and the range follow the forward's stamp, in backward_impl).  An empty model (P == 0) needs nothing beyond sizes.
int validate_backward(const frg_backward_args& a)
{
    if (a.exact_blend < 0 || a.exact_blend > 2 || a.shell_bary_mode < 0 || a.shell_bary_mode > 1)
        return fail(FRG_EINVAL, "frg_backward_args: mode out of range (exact_blend %d, shell_bary_mode %d)", a.exact_blend, a.shell_bary_mode);
    if (a.P < 0 || a.R < 0 || a.width <= 0 || a.height <= 0) return fail(FRG_EINVAL, "bad sizes");
    if (a.P == 0) return FRG_OK;
    if (!a.geom_buffer || !a.binning_buffer || !a.image_buffer || !a.dL_dpix || !a.background || !a.viewmatrix || !a.projmatrix || !a.campos)
        return fail(FRG_EINVAL, "null required pointer");
    if ((a.means3D == nullptr) == (a.shell_logits == nullptr)) return fail(FRG_EINVAL, "provide exactly one of means3D / shell_logits");
    if (a.shell_logits && (!a.shell_cell_verts || !a.shell_cells || !a.dL_dshell_logits))
        return fail(FRG_EINVAL, "shell_logits needs shell_cell_verts, shell_cells and dL_dshell_logits");
    if (!a.dL_dmean2D || !a.dL_dopacity || !a.dL_dmean3D) return fail(FRG_EINVAL, "null gradient output");
    if (a.sh_rotations && (!a.shs || a.colors_precomp))
        return fail(FRG_EINVAL, "sh_rotations rotate the directions of the SH colour: they come with shs, not with colors_precomp");
    // (dL_dsh == NULL asks for the factor of the SH gradient, which frg_sh_grad_from_views multiplies with the basis at the UNROTATED direction)
    if (a.sh_rotations && !a.dL_dsh)
        return fail(FRG_EINVAL, "sh_rotations with dL_dsh == NULL: rotated SH directions are a single-view render feature, the factored exchange does not carry them");
    // intermediates of the chain may be left out when the caller has no use for them: dL_dcolor when the SH rows are
    // written (it is then only the factor of dL_dsh), dL_dcov3D when the covariance comes from scales / rotations
    if (!a.dL_dcolor && !(a.shs && a.dL_dsh)) return fail(FRG_EINVAL, "dL_dcolor may only be NULL when shs and dL_dsh are given");
    if (!a.dL_dcov3D && a.cov3D_precomp) return fail(FRG_EINVAL, "dL_dcov3D may only be NULL without cov3D_precomp");
    if ((a.raw_scales == nullptr) != (a.raw_rotations == nullptr)) return fail(FRG_EINVAL, "raw_scales and raw_rotations come together");
    if (((a.scales && (!a.dL_dscale || !a.dL_drot || !a.rotations))) || (a.raw_scales && (!a.dL_dscale || !a.dL_drot)))
        return fail(FRG_EINVAL, "null gradient output for a provided input");
    // R sizes the slots and the backward blend's item list: fewer than the forward rendered would overrun them.  (More is
    // fine -- a deferred forward's capacity: where the forward's checkpoints lie in the binning chunk is taken from what the
    // forward stamped, Counters::carved_R, not from R.)
    if (a.workspace_bytes < frg_backward_workspace_bytes(a.P, a.R) || !a.workspace)
        return fail(FRG_EALLOC, "workspace too small: need %zu bytes", frg_backward_workspace_bytes(a.P, a.R));
    return FRG_OK;
}

// The arithmetic of this backward's blend pass (the backward recomputes its forward's alpha, T and contributor tests: the
// same arithmetic keeps them consistent) and whether that forward kept anything for a backward were stamped into the
// image chunk by the forward's blend kernel (Counters::fwd_flags): they travel with the buffers.  The host's notes are
// keyed by ADDRESS -- a buffer copied to an address some earlier forward used would inherit that forward's note -- so
// they decide nothing a stamp can contradict:
//   * arithmetic: what the caller states (frg_backward_args::exact_blend; the Python layer carries it in its autograd
//     ctx), else BOTH instantiations are launched and each leaves at once unless the stamp names it (*exact = -1);
//   * forward_only: a note that says "an ordinary forward" lets the call through (a forward_only stamp then still leaves
//     the kernels without work); anything else -- no note, or a note that says forward_only -- is settled by reading the
//     stamp back, one blocking copy of the forward's counters, which also tells the arithmetic.
//   * R: a note that says the forward rendered MORE instances than this call's R (slots and item lists would overrun) is
//     checked against the stamped count the same way before the call is refused.
//   * sh_rotations: a note that says "rotated" where the call has no matrices, or the reverse, is checked against the stamp
//     (FRG_FWD_ROTATED) the same way; behind a note that agrees -- possibly a stale one -- preprocess_bwd_kernel compares the
//     stamp with its ROT instantiation and writes zero rows on a mismatch instead of gradients of the wrong directions.
// -> *exact: 1 | 0 as stated or stamped, -1 "as stamped, on the device"
int settle_forward_stamp(const frg_backward_args& a, const std::optional<FwdNote>& note, int* exact)
{
    *exact = a.exact_blend == 0 ? -1 : FwdModes::pick(a.exact_blend, 1, 0);
    // rotated SH directions (frg_forward_args::sh_rotations): the backward's matrices must be there exactly when the forward's
    // were.  A note that disagrees with the call is a reason to read the stamp, and only the stamp refuses; a note that agrees
    // lets the call through, and the per-Gaussian backward compares the stamp's bit with its own instantiation on the device
    const bool rotated = a.sh_rotations != nullptr;
    const char* const rot_missing = "the forward that filled these buffers was given sh_rotations: the backward needs the same matrices (frg_backward_args::sh_rotations is NULL)";
    const char* const rot_extra = "sh_rotations given, but the forward that filled these buffers had none";
    const bool ask_the_stamp = !note || note->fwd_only || (note->rendered >= 0 && a.R < note->rendered) || note->rotated != rotated;
    if (!ask_the_stamp || a.phase == 2) return FRG_OK;
    hipStream_t stream = (hipStream_t)a.hip_stream;
    frg::Counters* host = pinned_counters();
    if (!host) return fail(FRG_EHIP, "hipHostMalloc failed");
    const frg::ImageState img0 = frg::ImageState::carve(a.image_buffer, a.width, a.height, false);
    FRG_HIP(hipMemcpyAsync(host, img0.counters, sizeof(frg::Counters), hipMemcpyDeviceToHost, stream));
    FRG_HIP(hipStreamSynchronize(stream));
    const uint32_t flags = host->fwd_flags;
    if (!(flags & FRG_FWD_STAMPED))
        return fail(FRG_EINVAL, "the image buffer carries no forward's stamp: these are not the buffers of a completed frg_forward");
    if (flags & FRG_FWD_ONLY)
        return fail(FRG_EINVAL, "the forward that filled these buffers was called with forward_only = 1: it kept nothing for a backward");
    if ((uint32_t)a.R < host->num_rendered)
        return fail(FRG_EINVAL, "R = %d, but the forward that filled this geometry buffer rendered %u instances", a.R, host->num_rendered);
    if (((flags & FRG_FWD_ROTATED) != 0u) != rotated) return fail(FRG_EINVAL, "%s", rotated ? rot_extra : rot_missing);
    if (*exact < 0) *exact = (flags & FRG_FWD_EXACT) ? 1 : 0;
    return FRG_OK;
}

// Where the two forms of the per-Gaussian backward go.  The 16-wave form for the Gaussians that own thousands of slots
// runs beside the plain kernel (usually its workgroups find an empty list and leave); the forward's scatter posted how
// many waves of Gaussians need it (Mailbox::heavy): none, usually -- the launch is then skipped.
//   Known to exist: the few 16-wave workgroups go on the CALLER's stream and start at once on an empty GPU, the
// plain kernel follows on the side stream a cross-queue hop later and fills the rest -- behind the plain kernel's
// 47 k waves the 1024-thread workgroups waited for a whole free CU and ran mostly after it (clustered scene:
// 0.41 -> 0.33 ms).  Unknown (no post): the 16-wave form on the high-priority side stream (g_bwd_side).
struct PbwStreams {
    hipStream_t heavy, plain;
    bool side;           // one of the two is g_bwd_side's: fork before, join behind
    bool skip_heavy;
};
PbwStreams pick_pbw_streams(hipStream_t stream, int debug, const std::optional<FwdNote>& note)
{
    const int heavy = g_assume_no_heavy.load(std::memory_order_relaxed) ? 0 : debug || !note ? -1 : note->heavy_waves_posted();
    const bool skip_heavy = heavy == 0;
    const bool side = !skip_heavy && !debug && g_bwd_side.ensure();
    const bool heavy_first = side && heavy > 0 && g_bwd_heavy_first.load(std::memory_order_relaxed);
    hipStream_t other = side ? g_bwd_side.stream : stream;
    return PbwStreams{heavy_first ? stream : other, heavy_first ? other : stream, side, skip_heavy};
}

int backward_impl(const frg_backward_args& a)
{
    FRG_TRY(validate_backward(a));
    if (a.P == 0) return FRG_OK;
    const int P = a.P, R = a.R, debug = a.debug, phase = a.phase;
    hipStream_t stream = (hipStream_t)a.hip_stream;
    const std::optional<FwdNote> note = g_fwd_notes.find(a.geom_buffer);
    int exact;
    FRG_TRY(settle_forward_stamp(a, note, &exact));

    // Nothing here depends on the process-wide binning options: every field of the three chunks that the
    // backward reads is carved from (P, W, H, R) alone (the option-dependent matrices of the binning stage
    // come last in the image chunk), and the kernels take the forward's binning mode from the counters it
    // stamped.  "exact_blend" only selects the arithmetic of this backward's own blend pass.
    const frg::ViewParams vp = make_view(a.D, a.M, a.width, a.height, a.tan_fovx, a.tan_fovy, a.scale_modifier, 0);
    const frg::GeomState g = frg::GeomState::carve(a.geom_buffer, P);
    const frg::ImageState img = frg::ImageState::carve(a.image_buffer, a.width, a.height, false);
    const frg::BinningState b = frg::BinningState::carve(a.binning_buffer, R, 0);
    const frg::BwdWorkspace ws = frg::BwdWorkspace::carve(a.workspace, P, R);
    unsigned long long* const live_masks = phase == 1 ? ws.live_masks : nullptr;
    if (phase < 0 || phase > 2) return fail(FRG_EINVAL, "frg_backward_args: phase %d (0 whole | 1 blend + slot sums | 2 the rest)", phase);
    const int* const radii = a.radii ? a.radii : g.internal_radii;   // rasterizer_impl.cu:375-377

    frg::FwdInputs in{a.means3D, a.scales, a.rotations, nullptr, a.shs, a.cov3D_precomp, a.colors_precomp, a.viewmatrix, a.projmatrix, a.campos};
    in.raw = raw_inputs_of(a);
    in.sh_rotations = a.sh_rotations;
    frg::BwdOutputs out{a.dL_dmean2D, a.dL_dconic, a.dL_dopacity, a.dL_dcolor, a.dL_dmean3D, a.dL_dcov3D, a.dL_dsh, a.dL_dscale, a.dL_drot};
    out.dL_dshell_logits = a.dL_dshell_logits;
    out.dL_dshell_verts = a.dL_dshell_cell_verts;
    out.row_live = a.row_live;
    const int pbw_flags = phase == 1 ? FRG_PBW_SUMS_ONLY : phase == 2 ? FRG_PBW_FROM_SUMS : 0;
    // the per-Gaussian backward: each call site states its flags, its form (heavy_only), its stream and, in phase 1, what it leaves
    auto preprocess_bwd = [&](int flags, bool heavy_only, hipStream_t s, unsigned long long* masks = nullptr, float* dirs = nullptr,
                              int range_first = 0, int range_count = 0) {
        return frg::launch_preprocess_bwd(P, vp, in, radii, g, img, ws.slots, out, g_ablate.load(), flags, heavy_only, s, ws.sums, masks, dirs,
                                          range_first, range_count);
    };
    if (phase == 2) {     // the sums are in the workspace: one launch, no slot reduction, hence no 16-wave form either
        if (!g_phase_notes.consume(a.workspace, a.geom_buffer, a.image_buffer, P, R))
            return fail(FRG_EINVAL, "backward phase 2 without a matching phase 1 on this workspace (same P, R, geometry and image buffers)");
        StageScope sc_(ST_PREPROCESS_BWD, stream);
        FRG_STAGE(preprocess_bwd(pbw_flags | FRG_PBW_NO_HEAVY_LAUNCH, false, stream), "preprocess_bwd (phase 2)");
        return FRG_OK;
    }
    if (phase == 1) g_phase_notes.record(a.workspace, a.geom_buffer, a.image_buffer, P, R, a.sh_rotations != nullptr);
    const bool ranged = a.range_count > 0;
    if (ranged) {
        if (phase != 1) return fail(FRG_EINVAL, "frg_backward_args: a range is offered with phase 1 only (phase %d)", phase);
        if (a.range_first < 0 || a.range_first % 256 != 0 || (long long)a.range_first + a.range_count > P)
            return fail(FRG_EINVAL, "frg_backward_args: range [%d, +%d) of %d Gaussians (range_first: a multiple of 256)", a.range_first, a.range_count, P);
    }
    const bool probe_bwd = (g_probe.load() & 2) && g_probe_side.ensure();
    if (probe_bwd) {   // timing experiment: the per-Gaussian backward beside the blend (it reads the previous frame's slots)
        FRG_HIP(g_probe_side.fork_from(stream));
        FRG_HIP(preprocess_bwd(pbw_flags, false, g_probe_side.stream));
        FRG_HIP(preprocess_bwd(pbw_flags, true, g_probe_side.stream));
        FRG_HIP(hipEventRecord(g_probe_side.join, g_probe_side.stream));
    }
    if (!ranged || a.range_first == 0) {
        StageScope sc_(ST_BLEND_BWD, stream);
        if (exact != 0)
            FRG_STAGE(frg::launch_blend_bwd_exact(vp, g, img, b, a.background, a.dL_dpix, ws.slots, (uint32_t)R, g_bwd_batch.load(), stream, exact < 0), "blend_bwd");
        if (exact <= 0)
            FRG_STAGE(frg::launch_blend_bwd_fast(vp, g, img, b, a.background, a.dL_dpix, ws.slots, (uint32_t)R, g_bwd_batch.load(), stream, exact < 0), "blend_bwd");
    }
    if (probe_bwd) { FRG_HIP(hipStreamWaitEvent(stream, g_probe_side.join, 0)); return FRG_OK; }
    StageScope sc_(ST_PREPROCESS_BWD, stream);
    if (ranged) {      // phase 1 in pieces: the plain kernel over this range, whatever its waves own (no 16-wave side launch)
        FRG_STAGE(preprocess_bwd(pbw_flags | FRG_PBW_NO_HEAVY_LAUNCH, false, stream, live_masks, ws.dir_terms, a.range_first, a.range_count), "preprocess_bwd (phase 1, range)");
        return FRG_OK;
    }
    const PbwStreams to = pick_pbw_streams(stream, debug, note);
    if (to.side) FRG_HIP(g_bwd_side.fork_from(stream));
    if (!to.skip_heavy)
        FRG_STAGE(preprocess_bwd(pbw_flags, true, to.heavy, live_masks, ws.dir_terms), "preprocess_bwd (long runs)");
    FRG_STAGE(preprocess_bwd(pbw_flags | (to.skip_heavy ? FRG_PBW_NO_HEAVY_LAUNCH : 0), false, to.plain, live_masks, ws.dir_terms), "preprocess_bwd");
    if (to.side) { FRG_HIP(hipEventRecord(g_bwd_side.join, g_bwd_side.stream)); FRG_HIP(hipStreamWaitEvent(stream, g_bwd_side.join, 0)); }
    return FRG_OK;
}

}  // namespace

// The exchange entry points (api_ops.hip) run the per-Gaussian chain without the matrices and refuse a rotated forward early.
// frg_pack_sum_rows asks what the phase 1 that filled its workspace was CALLED with (that call's matrices were checked against
// the stamp); frg_sh_color_grad has only the geometry buffer, hence only the forward's note: an early refusal for the caller
// that renders with rotations and trains view-parallel on the same buffers, no guarantee for copies of them.
bool frg::forward_was_rotated(const void* geom_buffer)
{
    const std::optional<FwdNote> note = g_fwd_notes.find(geom_buffer);
    return note && note->rotated;
}
bool frg::phase1_was_rotated(const void* workspace) { return g_phase_notes.rotated(workspace); }

extern "C" {

int frg_version(void) { return 2; }
const char* frg_last_error(void) { return g_err; }

int frg_set_option(const char* name, int value)
{
    const Option* o = find_option(name);
    if (!o) return fail(FRG_EINVAL, "unknown option '%s'", name ? name : "(null)");
    if (o->experiment) {
        static const bool experiments = [] { const char* e = getenv("FROSTING_EXPERIMENTS"); return e && e[0] == '1'; }();
        if (!experiments)
            return fail(FRG_EINVAL, "option '%s' is a timing experiment (results are wrong by design): start the process with "
                                    "FROSTING_EXPERIMENTS=1 to use it", name);
    }
    if (o->value == &g_exact_blend) (void)exact_blend();      // the previous value is the resolved one
    return o->value->exchange(o->stored(value));
}

int frg_get_option(const char* name)
{
    const Option* o = find_option(name);
    if (!o || o->experiment) return fail(FRG_EINVAL, "unknown option '%s'", name ? name : "(null)");
    return o->value == &g_exact_blend ? exact_blend() : o->value->load();
}

int frg_stage_times(float* ms, int n)
{
    if (!ms || n < ST_COUNT) return fail(FRG_EINVAL, "need room for %d stages", (int)ST_COUNT);
    for (int i = 0; i < n; i++) ms[i] = -1.0f;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return ST_COUNT;
    std::lock_guard<std::mutex> lk(g_timers_mu);
    StageTimers& tm = g_timers[dev];
    if (!tm.init) return ST_COUNT;
    for (int i = 0; i < ST_COUNT; i++) {
        const unsigned cnt = tm.launches[i] < (unsigned)ST_SLOTS ? tm.launches[i] : (unsigned)ST_SLOTS;
        double sum = 0.0;
        unsigned good = 0;
        for (unsigned k = 0; k < cnt; k++) {
            if (hipEventSynchronize(tm.ev[i][k][1]) != hipSuccess) continue;
            float t = -1.0f;
            if (hipEventElapsedTime(&t, tm.ev[i][k][0], tm.ev[i][k][1]) == hipSuccess) { sum += t; good++; }
        }
        if (good) ms[i] = (float)(sum / good);
        tm.launches[i] = 0;
    }
    return ST_COUNT;
}

size_t frg_geometry_bytes(int P) { return frg::GeomState::carve(nullptr, P).bytes; }
size_t frg_image_bytes(int width, int height) { return frg::ImageState::carve(nullptr, width, height, g_global_bins.load() != 0).bytes; }
size_t frg_binning_bytes(int R, int max_tile_count) { return frg::BinningState::carve(nullptr, R, max_tile_count, g_bwd_seg_log.load()).bytes; }
size_t frg_backward_workspace_bytes(int P, int R) { return frg::BwdWorkspace::carve(nullptr, P, R).bytes; }

int frg_geometry_layout_n(int P, long long* out, int n)
{
    frg::GeomState s = frg::GeomState::carve(nullptr, P);
    const long long v[6] = {(long long)(size_t)s.xydr, (long long)(size_t)s.conic_opacity, (long long)(size_t)s.rgb_clamped,
                            (long long)(size_t)s.tiles_touched, (long long)(size_t)s.point_offsets,
                            (long long)(16 * FRG_REC)};   // [5]: byte stride between consecutive Gaussians' float4 of out[0..2]
    for (int i = 0; i < n && i < 6; i++) out[i] = v[i];
    return 6;
}
void frg_geometry_layout(int P, long long* out) { (void)frg_geometry_layout_n(P, out, 5); }   // the five values of version 1 callers
void frg_image_layout(int width, int height, long long* out)
{
    frg::ImageState s = frg::ImageState::carve(nullptr, width, height, g_global_bins.load() != 0);
    out[0] = (long long)(size_t)s.final_T; out[1] = (long long)(size_t)s.n_contrib; out[2] = (long long)(size_t)s.ranges;
    out[3] = (long long)(size_t)s.tile_count;
}
void frg_binning_layout(int R, int max_tile_count, long long* out)
{
    frg::BinningState s = frg::BinningState::carve(nullptr, R, max_tile_count);
    out[0] = (long long)(size_t)s.point_list; out[1] = (long long)(size_t)s.pairs;
}

int frg_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     unsigned char* present, void* hip_stream)
{
    (void)projmatrix;  // the reference's frustum test only uses the view matrix (auxiliary.h:154)
    if (P < 0) return fail(FRG_EINVAL, "P < 0");
    if (P == 0) return FRG_OK;
    if (!means3D || !viewmatrix || !present) return fail(FRG_EINVAL, "null pointer");
    FRG_HIP(frg::launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)hip_stream));
    return FRG_OK;
}

int frg_forward(frg_alloc_fn geometry_alloc, frg_alloc_fn binning_alloc, frg_alloc_fn image_alloc, void* user,
                int P, int D, int M, const float* background, int width, int height,
                const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                float tan_fovx, float tan_fovy, int prefiltered,
                float* out_color, int* radii, int debug, void* hip_stream)
{
    frg_forward_args a = positional_forward_args(geometry_alloc, binning_alloc, image_alloc, user, P, D, M, background, width, height, means3D, shs,
                                                 colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp, viewmatrix,
                                                 projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, out_color, radii, hip_stream);
    a.debug = debug;
    return forward_impl(a);
}

int frg_forward_deferred(frg_alloc_fn geometry_alloc, frg_alloc_fn binning_alloc, frg_alloc_fn image_alloc, void* user,
                         int P, int D, int M, const float* background, int width, int height,
                         const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                         const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                         const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                         float tan_fovx, float tan_fovy, int prefiltered,
                         float* out_color, int* radii, int instance_capacity, void* hip_stream)
{
    if (instance_capacity <= 0) return fail(FRG_EINVAL, "instance_capacity must be positive");
    frg_forward_args a = positional_forward_args(geometry_alloc, binning_alloc, image_alloc, user, P, D, M, background, width, height, means3D, shs,
                                                 colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp, viewmatrix,
                                                 projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered, out_color, radii, hip_stream);
    a.instance_capacity = instance_capacity;
    return forward_impl(a);
}

int frg_forward_ex(const frg_forward_args* a)
{
    // five generations of the struct: up to keep_mask (version 1 callers), with the raw-parameter fields, with the
    // per-call modes, with forward_only, with sh_rotations
    const size_t v1 = offsetof(frg_forward_args, raw_opacities), v2 = offsetof(frg_forward_args, exact_blend),
                 v3 = offsetof(frg_forward_args, forward_only), v4 = offsetof(frg_forward_args, sh_rotations);
    frg_forward_args full;
    if (!widen(a, {sizeof(frg_forward_args), v4, v3, v2, v1}, &full))
        return fail(FRG_EINVAL, "frg_forward_args: struct_size %zu, this library expects %zu (or %zu, %zu, %zu, %zu)", a ? a->struct_size : (size_t)0,
                    sizeof(frg_forward_args), v4, v3, v2, v1);
    return forward_impl(full);
}

int frg_forward_finish(const char* image_buffer, int prefiltered, int* num_rendered)
{
    PendingCounters* p = g_pending.find(image_buffer);
    if (!p) return fail(FRG_EINVAL, "no deferred forward is pending for this image buffer on this thread");
    FRG_HIP(hipEventSynchronize(p->ev));
    const frg::Counters c = *p->host;
    p->key = nullptr;
    if (num_rendered) *num_rendered = (int)(c.num_rendered > 0x7fffffffu ? 0x7fffffffu : c.num_rendered);
    if (c.num_rendered > 0x7fffffffu) return fail(FRG_EINVAL, "num_rendered overflows int32");
    if (c.overflow)
        return fail(FRG_ECAPACITY, "%u instances exceed the instance capacity of the deferred forward: nothing was "
                                   "rasterized, repeat the view with a larger capacity", c.num_rendered);
    for (int k = 0; k < FRG_SORT_CLASSES; k++) g_pending.last_class_count[k] = c.class_count[k];
    g_pending.have_hint = true;
    if (prefiltered && c.filtered)
        return fail(FRG_EFILTER, "Point is filtered although prefiltered is set. This shouldn't happen!");
    return FRG_OK;
}

int frg_backward(int P, int D, int M, int R, const float* background, int width, int height,
                 const float* means3D, const float* shs, const float* colors_precomp,
                 const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                 const float* viewmatrix, const float* projmatrix, const float* campos,
                 float tan_fovx, float tan_fovy, const int* radii,
                 char* geom_buffer, char* binning_buffer, char* image_buffer, const float* dL_dpix,
                 float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                 float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                 char* workspace, size_t workspace_bytes, int debug, void* hip_stream)
{
    // (the parameters are the struct's fields up to hip_stream, in its order; the later fields stay 0 / NULL: absent)
    return backward_impl(frg_backward_args{sizeof(frg_backward_args), P, D, M, R, background, width, height, means3D, shs, colors_precomp,
                                           scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx,
                                           tan_fovy, radii, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_dmean2D, dL_dconic,
                                           dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, workspace,
                                           workspace_bytes, debug, hip_stream});
}

int frg_backward_ex(const frg_backward_args* a)
{
    // six generations of the struct: up to shell_*, + exact_blend / shell_bary_mode, + phase, + row_live, + range_first / range_count,
    // + sh_rotations
    const size_t b1 = offsetof(frg_backward_args, exact_blend), b2 = offsetof(frg_backward_args, phase), b3 = offsetof(frg_backward_args, row_live),
                 b4 = offsetof(frg_backward_args, range_first), b5 = offsetof(frg_backward_args, sh_rotations);
    frg_backward_args full;
    if (!widen(a, {sizeof(frg_backward_args), b5, b4, b3, b2, b1}, &full))
        return fail(FRG_EINVAL, "frg_backward_args: struct_size %zu, this library expects %zu (or %zu, %zu, %zu, %zu, %zu)", a ? a->struct_size : (size_t)0,
                    sizeof(frg_backward_args), b5, b4, b3, b2, b1);
    return backward_impl(full);
}

}  // extern "C"
