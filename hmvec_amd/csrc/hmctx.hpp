// Internal header of libhmgrid: the context, the error plumbing and the host helpers shared by its translation units -
// runtime.hip (contexts, memory, events, lanes, captured steps), comm.hip (RCCL) and the units that hold kernels and
// their launch entry points (the Makefile lists them).  Not part of the C ABI (include/hmgrid.h).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <rocfft/rocfft.h>

#include <cstdio>
#include <map>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/hmgrid.h"
#include "ldsfft.hpp"
#include "sici.hpp"

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
// (the message of the last failed call of this thread: hmg_last_error; both live in runtime.hip)
extern thread_local std::string g_last_error;
int fail(const char* what, const char* detail, const char* file, int line);
// (a failed runtime call also leaves a sticky "last error" behind: clear it, or the next
// hipGetLastError() check after a perfectly good kernel launch would report it again)
#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            (void)hipGetLastError();                                                    \
            return fail(#expr, hipGetErrorString(e_), __FILE__, __LINE__);              \
        }                                                                               \
    } while (0)
#define FFT_TRY(expr)                                                                   \
    do {                                                                                \
        rocfft_status s_ = (expr);                                                      \
        if (s_ != rocfft_status_success) {                                              \
            char m_[32];                                                                \
            snprintf(m_, sizeof(m_), "rocfft status %d", (int)s_);                      \
            return fail(#expr, m_, __FILE__, __LINE__);                                 \
        }                                                                               \
    } while (0)
#define NCCL_TRY(expr)                                                                  \
    do {                                                                                \
        ncclResult_t r_ = (expr);                                                       \
        if (r_ != ncclSuccess) return fail(#expr, ncclGetErrorString(r_), __FILE__, __LINE__); \
    } while (0)
#define REQUIRE(cond, msg)                                                              \
    do {                                                                                \
        if (!(cond)) return fail("invalid argument", msg, __FILE__, __LINE__);          \
    } while (0)

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
struct FftPlan {
    rocfft_plan plan = nullptr;
    rocfft_execution_info info = nullptr;
    void* work = nullptr;
    size_t work_bytes = 0;
};

namespace hmg { struct UnpackTw; }
struct FusedPlan {
    hmg::FftPlanDev plan;
    hmg::cplx* twM = nullptr;
    hmg::UnpackTw* twN = nullptr;
    int maxb = 0, maxp = 0;
};

struct PrunedPlan {                       // tables of the long-grid routes, per (nxs, LP); LP = 0: the mode-ordered pair
    hmg::cplx* twB = nullptr;             // LP == 0: exp(-2 pi i t / M), t < M = nxs/2 (narrow-band route)
    hmg::UnpackTw* twN = nullptr;         // LP == 0: unpack constants for j <= M/2 by mode (chirp and narrow-band routes)
    hmg::cplx* twR = nullptr;             // LP > 0: the residues' twiddles on the samples, by residue (ldsfft.hpp)
    hmg::UnpackTw* twNr = nullptr;        // LP > 0: unpack constants by residue
};
struct ChirpPlan {                        // tables of the chirp route (ldsfft.hpp: ChirpTables), per (nxs, LP, p0)
    hmg::cplx *chP = nullptr, *chJ = nullptr, *Bw = nullptr;
    int Jw = 0;
};
struct SupportKey {                       // what a measured bound on a launch's rows was measured for
    const void *cmax, *xs, *rss, *ks;
    int rows, nxs, nk;
    long long epoch;                      // the caller's tag of the arrays' CONTENTS (hmg_profile_support_epoch), 0 = none
    bool operator<(const SupportKey& o) const {
        return std::tie(cmax, xs, rss, ks, rows, nxs, nk, epoch) < std::tie(o.cmax, o.xs, o.rss, o.ks, o.rows, o.nxs, o.nk, o.epoch);
    }
};

struct PrefixEntry {                      // a tensor some transform wrote with its left fill deferred (hmg_prefix_deferral)
    int* nconst = nullptr;                // the hint arrays that describe the unwritten tiles
    double* cconst = nullptr;
    int rows = 0, nk = 0;
    bool pending = false;                 // the tiles are unwritten right now
    // the other kind of entry - series deferral of the analytic NFW tensor: the unwritten tiles are those below nser[row],
    // their values nfw_series_short of the row's series coefficients (acoef), c, r_s, z and the wavenumbers
    int* nser = nullptr;
    const double *acoef = nullptr, *cs = nullptr, *rss = nullptr, *zs = nullptr, *ks = nullptr;
    int nm = 0;
    bool described() const { return nconst || nser; }
};
struct SeriesCounts { int* d = nullptr; int rows = 0; };      // the context's nser array of one NFW tensor

struct hmg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;             // stream of the current lane
    hipStream_t lanes[HMG_LANES] = {};        // lane 0 is the main stream
    int lane = 0;
    hipEvent_t ev[HMG_EVENT_SLOTS] = {};
    int bracket[HMG_KERNEL_COUNT][2];  // one-shot event brackets per kernel id, -1 = off
    // grow-only scratch arenas (device)
    void* scratch[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t scratch_bytes[7] = {0, 0, 0, 0, 0, 0, 0};
    std::map<std::pair<int, int>, FftPlan> plans;  // (nxs, batch) -> plan
    std::map<int, struct FusedPlan> fused;          // nxs -> workgroup-FFT tables
    size_t fft_chunk_bytes = 0;                    // 0 = default
    int use_fused_fft = 1;                         // HMG_FUSED_FFT=0 forces the rocFFT path
    int use_pruned_fft = 1;                        // HMG_PRUNED_FFT=0: long grids go to rocFFT as before round 4
    int fused_max_m = 6144;                        // HMG_FUSED_MAX_M: longest packed row the one-row-in-LDS kernel takes
    int fused_prefer_m = 2500;                     // HMG_FUSED_PREFER_M: above this the long-grid route is tried first
    int pruned_lp_min = 0;                         // HMG_PRUNED_LP_MIN: smallest sub-transform length to consider
    int use_chirp = 1;                             // HMG_CHIRP=0: every row of a long grid takes the decomposition
    int use_band_fft = 1;                          // HMG_BAND_FFT=0: supports that do not prune go to rocFFT
    int use_tensor_group = 1;                     // HMG_NO_TENSOR_GROUP=1: hmg_group_tensors as its two launches (testing, A/B)
    int fused_generic = 0;                         // HMG_FUSED_GENERIC=1 (testing): the run-time plan for every one-row length
    int force_gatherv = 0;                         // HMG_FORCE_GATHERV=1 (testing): no all-gather shortcut for equal slab lengths
    std::map<std::tuple<int, int, int>, ChirpPlan> chirp;   // (nxs, LP, p0) -> tables
    std::map<std::pair<int, int>, PrunedPlan> pruned;   // (nxs, LP) -> tables of the long-grid routes
    std::map<int, hmg::cplx*> pass_tw;             // L -> per-pass twiddle table of the length-L plan (ldsfft.hpp)
    std::map<SupportKey, std::pair<int, int>> support;   // last measured bounds of a launch's rows: (support in packed samples, needed modes)
    // word a kernel raises when it cannot do what it was launched for: ONE word in page-locked host memory that the
    // device writes directly (a system-scope store), so that a host that has waited for the kernel - through whichever
    // stream, lane or event - reads it without a copy and without a question of which stream the copy belongs to
    int* h_fault = nullptr;
    int* d_fault = nullptr;                        // the device's address of the same word
    long long support_epoch = 0;                   // hmg_profile_support_epoch: tag of the contents of cmax / rss / ks arrays
    int sig_nz = 0, sig_nm = 0, sig_nq = 0;        // shape of the partial sums the last sigma^2 contraction left in scratch[4]
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_size = 1;
    double* d_barrier = nullptr;
    hmg::SiciTable* d_sici = nullptr;  // Si/Ci coefficients, read through the scalar cache
    void* pinned[2] = {nullptr, nullptr};   // host bounce buffers for pageable <-> device copies
    // small host -> device copies: a ring of pinned slots, so that an upload is a memcpy + an asynchronous DMA
    // and the host does not wait for the stream (a model's constructor makes ~20 of these)
    static constexpr int UP_SLOTS = 32;
    static constexpr size_t UP_SLOT_BYTES = (size_t)256 << 10;
    char* up_ring = nullptr;
    hipEvent_t up_ev[UP_SLOTS] = {};
    int up_next = 0;
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    int num_cu = 256;
    // device blocks handed back by hmg_free, kept for reuse by size: dropping an array never
    // synchronises the device and a steady stream of same-shaped temporaries never reaches hipMalloc
    std::multimap<size_t, void*> free_blocks;
    std::map<void*, size_t> block_bytes;           // every live or cached block from hmg_malloc
    size_t cached_bytes = 0;
    bool lanes_dirty = false;                      // work was enqueued on a lane other than 0 since the last sync
    // captured steps (hmg_graph_*)
    bool capturing = false;
    std::vector<void*> freed_in_capture;           // hmg_free calls that arrived during a capture ...
    std::map<int, std::vector<void*>> graph_blocks; // ... stay with the graph that may use them until it is destroyed
    std::map<int, hipGraphExec_t> graphs;
    std::map<int, int> graph_kernels;              // kernel nodes per captured graph
    int next_graph_id = 1;
    // deferred left fills: the state per tensor pointer; what the launches of the capture in progress do to it (a
    // capture executes nothing, so the state itself stays); what each captured step does to it at every replay
    int prefix_deferral = 0;
    std::map<void*, PrefixEntry> prefix;
    std::map<void*, PrefixEntry> prefix_capture;
    std::map<int, std::map<void*, PrefixEntry>> graph_prefix;
    std::map<void*, SeriesCounts> series_counts;   // per NFW tensor pointer; grown outside captures only
    std::vector<void*> series_retired;             // outgrown count arrays: a captured step may still write them
    hmg_ctx() { for (auto& b : bracket) b[0] = b[1] = -1; }
};
constexpr size_t FREE_CACHE_LIMIT = (size_t)4 << 30;   // bytes kept in the free list before real frees

// ---- host helpers defined in runtime.hip
int event_at(hmg_ctx* c, int slot, hipEvent_t* out);      // events are created on first use
int check_fault(hmg_ctx* c);                              // report and clear the context's device fault word
int sync_all(hmg_ctx* c);                                 // all lanes + fault check; refuses inside a capture
int ensure_scratch(hmg_ctx* c, int slot, size_t bytes);   // grow-only scratch arenas; refuses inside a capture
int bracket_open(hmg_ctx* c, int kid, int* stop_slot);    // one-shot event brackets around a kernel (hmg_bracket_next)
int bracket_close(hmg_ctx* c, int stop_slot);
// ---- deferred left fills (the kernel and its entry points: hmgrid.hip)
// A transform wrote the tensor at `out`: with hint arrays (e.nconst) and its prefix deferred (e.pending) or whole, or
// without hint arrays - nothing describes its rows any more.  Entries stay after a fill: a captured step records the
// fill of every tensor the context knows (hmg_prefix_fill).
static inline void prefix_note(hmg_ctx* c, void* out, const PrefixEntry& e) {
    auto& m = c->capturing ? c->prefix_capture : c->prefix;
    if (e.described() || c->capturing) m[out] = e;
    else m.erase(out);
}
// a captured step ran: its launches' effects on the state
static inline void prefix_replayed(hmg_ctx* c, const std::map<void*, PrefixEntry>& fx) {
    for (auto& kv : fx) {
        if (kv.second.described()) c->prefix[kv.first] = kv.second;
        else c->prefix.erase(kv.first);
    }
}
// the block [p, p + bytes) leaves its owner: no entry may outlive it
static inline void prefix_drop_block(hmg_ctx* c, void* p, size_t bytes) {
    auto lo = c->prefix.lower_bound(p), hi = c->prefix.lower_bound((char*)p + bytes);
    c->prefix.erase(lo, hi);
}
// Series deferral (hmgrid.hip).  Every native reader of a tensor other than the batched mass integrals calls
// series_ensure_whole on it first: if p lies in an NFW tensor whose short-series tiles are unwritten they are filled (in
// a capture: recorded, with the semantics of hmg_prefix_fill).  Every native writer calls series_forget: nothing
// describes the tensor any more.
int series_ensure_whole(hmg_ctx* c, const void* p);
void series_forget(hmg_ctx* c, const void* p);
static inline dim3 grid1d(size_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }
// Run-time flags as template arguments: with_flags(f, a, b, ...) calls f(std::bool_constant<a>{}, std::bool_constant<b>{},
// ...), so that a generic lambda picks the instantiation a set of nullable output pointers asks for.
template <class F>
static inline void with_flags(F f) { f(); }
template <class F, class... Rest>
static inline void with_flags(F f, bool first, Rest... rest) {
    if (first) with_flags([&](auto... bs) { f(std::true_type{}, bs...); }, rest...);
    else with_flags([&](auto... bs) { f(std::false_type{}, bs...); }, rest...);
}
// every tensor of the tracers a call reads, whole (an NFW tensor with deferred series tiles is filled first)
static inline int tracers_ensure_whole(hmg_ctx* c, const hmg_tracer* t, int count) {      // (a contiguous array)
    for (int i = 0; i < count; ++i)
        if (series_ensure_whole(c, t[i].d_prof) || series_ensure_whole(c, t[i].d_cprof)) return 1;
    return 0;
}
static inline int tracers_ensure_whole(hmg_ctx* c, const hmg_tracer* const* t, int count) {
    for (int i = 0; i < count; ++i)
        if (tracers_ensure_whole(c, t[i], 1)) return 1;
    return 0;
}
// The temporaries of one call that cannot be part of a captured step - the words of its table check, what its prepasses
// leave for its main kernel, outputs the caller did not ask for - are ONE ordinary block of the context's allocator, live
// while f(block) enqueues the call (no scratch arena grows here: a captured step may have an arena's address baked in).
// It goes back to the free list before the call returns; whatever reuses it is enqueued behind the kernels of f.
template <class F>
static inline int with_block(hmg_ctx* c, size_t bytes, F f) {
    void* blk = nullptr;
    if (hmg_malloc(c, bytes, &blk)) return 1;
    const int rc = f(blk);
    return hmg_free(c, blk) || rc;
}
// A device-side check and its answer: zero `words` ints at d_bad, run `launch` (it enqueues the kernel that raises them),
// copy them to `bad` and wait for the stream.
template <class F>
static inline int check_words(hmg_ctx* c, int* d_bad, int* bad, int words, F launch) {
    HIP_TRY(hipMemsetAsync(d_bad, 0, words * sizeof(int), c->stream));
    launch();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(bad, d_bad, words * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}
