// pgt_api.cpp — the C-ABI of libpgtwin (include/pgtwin.h): context, argument checks, the
// host-buffer entry points (copy in -> GPU -> copy out) and the device-resident entry points.
// There is deliberately no CPU code path here: without a HIP device every reduce fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "pgt_internal.h"

// Host I/O of the host-buffer entry points (pgt_fst_reduce & co., what INTEGRATION.md binds), kept per context:
//  * a PINNED STAGING RING for the column uploads: `workers` host threads copy 16-MiB pieces of the caller's pageable columns
//    into their own two pinned slots and queue the DMA of each piece themselves (hipMemcpyAsync on one copy stream), so the
//    host-side memcpy of piece k+1 overlaps the DMA of piece k and nothing of the caller's memory has to be page-locked.
//    A plain hipMemcpy from pageable memory lets the runtime pin the caller's pages first: 0.45 ms/MiB the first time a
//    range is seen (tools/probes/upload_probe.cpp on the gpurun box: 182 ms for 400 MiB, 7.5 ms for the same buffer again)
//    — and a command-line tool sees every range for the first time;
//  * a CACHED WORKSPACE (window table, rows, tree, genome-wide total): grown when a call needs more, freed by pgt_close —
//    tools that reduce in passes call these entry points once per pass with the same sizes.
struct HostIo {
    static constexpr int kMaxWorkers = 16, kSlots = 2 * kMaxWorkers;
    static constexpr size_t kChunk = (size_t)8 << 20;  // threshold for taking the ring at all: 4 of these
    // geometry: profiles/r06/host_api_ring_geometry_sweep.txt (2 GB of fst columns, steady state): 16-MiB pieces 38.8 ms = 51.5 GB/s
    // with 2 … 12 workers alike, 8 MiB 40.5, 4 MiB 44.5, 2 MiB 52; a plain hipMemcpy of the SAME buffer again 36.5 (the runtime
    // caches its pin of the caller's pages; a first call pays 85 ms more)
    // What the ring costs to set up (tools/probes/first_use_probe.cpp): hipHostMalloc 15 ms per 64 MiB; a stream of its own 18 ms
    // (it would only buy what nobody needs: the kernels that follow wait for the columns anyway) — so: the NULL stream, and the
    // smallest geometry that still runs at the link's rate.
    int workers = 2;                   // PGT_UPLOAD_WORKERS (1 … 16)
    size_t chunk = (size_t)16 << 20;   // PGT_UPLOAD_CHUNK_MIB (1 … 64); two slots of this size per worker: 64 MiB pinned
    bool ring_ready = false;
    char *pin[kSlots] = {};
    hipEvent_t slot_done[kSlots] = {};
    hipStream_t copy_stream = nullptr;  // the NULL stream (see above)
    enum { kWin = 0, kRows, kTree, kTot, kKinds };
    void *ws[kKinds] = {};
    size_t ws_bytes[kKinds] = {};
};

struct pgt_ctx {
    int device = 0;
    std::string error;
    bool profiling = false;
    bool have_timing = false;
    bool timing_query_only = false;  // the last profiled call has no build phase (pgt_dstat_jackknife_dev): ev[0] was not recorded
    pgt::Hints hints;  // pgt_set_max_window / pgt_set_window_step (0 = unknown)
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // build start, build end, query end
    HostIo io;
};

namespace {

using namespace pgt;

int ctx_fail(pgt_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->error = msg;
    set_global_error(msg);
    return code;
}

int hip_check(pgt_ctx *ctx, hipError_t e, const char *what) {
    if (e == hipSuccess) return PGT_OK;
    return ctx_fail(ctx, PGT_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ABI 4: every row output carries its capacity; refuse before anything is launched
int room_check(pgt_ctx *ctx, const char *who, uint64_t rows, size_t row_bytes, size_t out_bytes) {
    if (rows != 0 && (rows > SIZE_MAX / row_bytes || rows * row_bytes > out_bytes))
        return ctx_fail(ctx, PGT_EARG, std::string(who) + ": the rows do not fit the output buffer (" + std::to_string(rows) + " rows of " +
                                           std::to_string(row_bytes) + " bytes, capacity " + std::to_string(out_bytes) + " bytes)");
    return PGT_OK;
}

// RAII device buffer for the host-buffer entry points (the columns: as large as the input, not cached)
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(pgt_ctx *ctx, size_t bytes, const char *what) {
        return hip_check(ctx, hipMalloc(&p, bytes ? bytes : 16), what);
    }
};

// PGT_TRACE_API=1: one stderr line per phase of a host-buffer entry point (where a call's milliseconds go)
struct ApiTrace {
    const char *who;
    bool on;
    std::chrono::steady_clock::time_point t;
    explicit ApiTrace(const char *w) : who(w), on(std::getenv("PGT_TRACE_API") != nullptr), t(std::chrono::steady_clock::now()) {}
    void lap(const char *what, size_t bytes = 0) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(now - t).count();
        if (bytes) std::fprintf(stderr, "[pgt-api] %s: %-18s %9.3f ms  %8.1f MB  %6.1f GB/s\n", who, what, ms, bytes / 1e6, bytes / ms / 1e6);
        else std::fprintf(stderr, "[pgt-api] %s: %-18s %9.3f ms\n", who, what, ms);
        t = now;
    }
};

// the cached workspace: -> a device pointer good for `bytes` until the next call that asks for more of the same kind
int workspace(pgt_ctx *ctx, int kind, size_t bytes, void **out) {
    HostIo &io = ctx->io;
    if (bytes == 0) bytes = 16;
    if (io.ws_bytes[kind] < bytes) {
        if (io.ws[kind]) (void)hipFree(io.ws[kind]);
        io.ws[kind] = nullptr;
        io.ws_bytes[kind] = 0;
        const size_t want = (bytes + (bytes >> 3) + 4095) & ~(size_t)4095;  // 12 % of slack: passes of slightly different sizes
        if (int rc = hip_check(ctx, hipMalloc(&io.ws[kind], want), "workspace: hipMalloc")) return rc;
        io.ws_bytes[kind] = want;
    }
    *out = io.ws[kind];
    return PGT_OK;
}

int ring_prepare(pgt_ctx *ctx) {
    HostIo &io = ctx->io;
    if (io.ring_ready) return PGT_OK;
    if (!io.pin[0]) {  // the geometry is fixed by the first attempt
        if (const char *e = std::getenv("PGT_UPLOAD_WORKERS")) io.workers = std::min(std::max(std::atoi(e), 1), (int)HostIo::kMaxWorkers);
        if (const char *e = std::getenv("PGT_UPLOAD_CHUNK_MIB")) io.chunk = (size_t)std::min(std::max(std::atoi(e), 1), 64) << 20;
    }
    for (int s = 0; s < 2 * io.workers; ++s) {  // (a slot that exists already: an earlier attempt failed further on)
        if (!io.pin[s])
            if (int rc = hip_check(ctx, hipHostMalloc(reinterpret_cast<void **>(&io.pin[s]), io.chunk, hipHostMallocDefault), "upload ring: hipHostMalloc")) {
                io.pin[s] = nullptr;
                return rc;
            }
        if (!io.slot_done[s])
            if (int rc = hip_check(ctx, hipEventCreateWithFlags(&io.slot_done[s], hipEventDisableTiming), "upload ring: hipEventCreate")) {
                io.slot_done[s] = nullptr;
                return rc;
            }
    }
    io.ring_ready = true;
    return PGT_OK;
}

void host_io_release(pgt_ctx *ctx) {
    HostIo &io = ctx->io;
    for (int s = 0; s < HostIo::kSlots; ++s) {
        if (io.pin[s]) (void)hipHostFree(io.pin[s]);
        if (io.slot_done[s]) (void)hipEventDestroy(io.slot_done[s]);
        io.pin[s] = nullptr;
        io.slot_done[s] = nullptr;
    }
    io.ring_ready = false;
    for (int k = 0; k < HostIo::kKinds; ++k) {
        if (io.ws[k]) (void)hipFree(io.ws[k]);
        io.ws[k] = nullptr;
        io.ws_bytes[k] = 0;
    }
}

// Host columns -> freshly allocated device columns, all of one call together.
struct UploadJob {
    DevBuf *dst;
    const void *src;
    size_t bytes;
    const char *what;
};

int upload_columns(pgt_ctx *ctx, UploadJob *jobs, int n_jobs, ApiTrace &trace) {
    size_t total = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (int rc = jobs[j].dst->alloc(ctx, jobs[j].bytes, jobs[j].what)) return rc;
        total += jobs[j].bytes;
    }
    trace.lap("alloc columns");
    const char *mode = std::getenv("PGT_UPLOAD");  // "plain": hipMemcpy from the caller's pageable memory, column after column
    if (total < 4 * HostIo::kChunk || (mode && std::strcmp(mode, "plain") == 0)) {
        for (int j = 0; j < n_jobs; ++j)
            if (jobs[j].bytes)
                if (int rc = hip_check(ctx, hipMemcpy(jobs[j].dst->p, jobs[j].src, jobs[j].bytes, hipMemcpyHostToDevice), jobs[j].what)) return rc;
        trace.lap("upload (hipMemcpy)", total);
        return PGT_OK;
    }
    if (int rc = ring_prepare(ctx)) return rc;
    trace.lap("staging ring");
    struct Piece {
        char *dst;
        const char *src;
        size_t bytes;
    };
    HostIo &io = ctx->io;
    std::vector<Piece> pieces;
    for (int j = 0; j < n_jobs; ++j)
        for (size_t off = 0; off < jobs[j].bytes; off += io.chunk)
            pieces.push_back({static_cast<char *>(jobs[j].dst->p) + off, static_cast<const char *>(jobs[j].src) + off,
                              std::min(io.chunk, jobs[j].bytes - off)});
    std::atomic<size_t> next{0};
    std::atomic<int> failed{0};  // a hipError_t, first one wins
    const int device = ctx->device;
    auto worker = [&](int w) {
        if (hipSetDevice(device) != hipSuccess) { int z = 0; failed.compare_exchange_strong(z, (int)hipErrorInvalidDevice); return; }
        bool used[2] = {false, false};
        for (int turn = 0;; turn ^= 1) {
            const size_t i = next.fetch_add(1);
            if (i >= pieces.size() || failed.load()) break;
            const int s = 2 * w + turn;
            hipError_t e = used[turn] ? hipEventSynchronize(io.slot_done[s]) : hipSuccess;  // the DMA that last read this slot
            if (e == hipSuccess) {
                std::memcpy(io.pin[s], pieces[i].src, pieces[i].bytes);
                e = hipMemcpyAsync(pieces[i].dst, io.pin[s], pieces[i].bytes, hipMemcpyHostToDevice, io.copy_stream);
            }
            if (e == hipSuccess) e = hipEventRecord(io.slot_done[s], io.copy_stream);
            used[turn] = true;
            if (e != hipSuccess) { int z = 0; failed.compare_exchange_strong(z, (int)e); break; }
        }
    };
    std::vector<std::thread> th;
    const int n_workers = (int)std::min<size_t>((size_t)io.workers, pieces.size());
    for (int w = 1; w < n_workers; ++w) {
        try {
            th.emplace_back(worker, w);
        } catch (...) {  // no thread to be had: the workers that exist (at least this one) take all pieces
            break;
        }
    }
    worker(0);
    for (auto &t : th) t.join();
    const hipError_t sync = hipStreamSynchronize(io.copy_stream);
    if (failed.load()) return hip_check(ctx, (hipError_t)failed.load(), "upload columns");
    if (int rc = hip_check(ctx, sync, "upload columns: synchronize")) return rc;
    trace.lap("upload (ring)", total);
    return PGT_OK;
}

// The three hints of a host table (pgt_table_hints): longest window; typical (median) length and typical step = median
// distance between consecutive window starts, both over a sample from the middle of the table (chromosome boundaries and
// the Q1 carry make a few distances irregular).  The typical length decides whether the group query fits, not the longest
// window: base-pair windows (dxyWindow) vary in their number of sites, and a strategy chosen for the longest would run the
// fallback of most.
void derive_hints(const pgt_win *win, uint64_t n_win, uint64_t *max_window, uint64_t *typical_window, uint64_t *window_step) {
    uint64_t m = 1;
    for (uint64_t i = 0; i < n_win; ++i)
        if (win[i].hi >= win[i].lo && win[i].hi - win[i].lo > m) m = win[i].hi - win[i].lo;
    std::vector<uint64_t> d, len;
    const uint64_t from = n_win > 4097 ? n_win / 2 - 2048 : 0, to = n_win > 4097 ? from + 4096 : (n_win ? n_win - 1 : 0);
    for (uint64_t i = from; i < to; ++i) {
        if (win[i + 1].lo >= win[i].lo) d.push_back(win[i + 1].lo - win[i].lo);
        if (win[i].hi >= win[i].lo) len.push_back(win[i].hi - win[i].lo);
    }
    uint64_t typical = 0, step = 0;
    if (!len.empty()) {
        std::nth_element(len.begin(), len.begin() + len.size() / 2, len.end());
        typical = len[len.size() / 2];
    }
    if (!d.empty()) {
        std::nth_element(d.begin(), d.begin() + d.size() / 2, d.end());
        step = d[d.size() / 2];
    }
    *max_window = m;
    *typical_window = typical;
    *window_step = step;
}

// RAII: the host-buffer entry points know the table, so they set the hints that are unset themselves
struct HintScope {
    pgt_ctx *ctx;
    pgt::Hints saved;
    HintScope(pgt_ctx *c, const pgt_win *win, uint64_t n_win) : ctx(c), saved(c->hints) {
        uint64_t m = 1, typical = 0, step = 0;
        derive_hints(win, n_win, &m, &typical, &step);
        // an explicit hint (the caller knows the whole table: a shard of it arrives here) stays, and stands for the typical
        // length too — unless THIS table contradicts it (a window longer than the hint: a stale pgt_set_max_window of an
        // earlier, unrelated table; the query would walk hundreds of nodes of too low a level), then the table speaks
        if (saved.max_window == 0 || m > saved.max_window) {
            c->hints.max_window = m;
            c->hints.typical_window = typical;
            if (saved.max_window != 0) c->hints.window_step = step;  // a stale longest window means a stale step as well
        }
        if (saved.window_step == 0) c->hints.window_step = step;
    }
    ~HintScope() { ctx->hints = saved; }
};

int check_windows_host(pgt_ctx *ctx, const pgt_win *win, uint64_t n_win, uint64_t n, bool need_coords_or_sites) {
    for (uint64_t i = 0; i < n_win; ++i) {
        if (win[i].lo > win[i].hi || win[i].hi > n)
            return ctx_fail(ctx, PGT_EARG, "window range outside [0, n_sites]");
        if (need_coords_or_sites && win[i].lo == win[i].hi && !(win[i].flags & PGT_WIN_COORDS))
            return ctx_fail(ctx, PGT_EARG, "empty window without explicit coordinates");
    }
    return PGT_OK;
}

// what a launcher ends in (LaunchEnv): the caller's stream, the context's events when it profiles, its message and hints
LaunchEnv events_for(pgt_ctx *ctx, void *stream) {
    if (!ctx->profiling) return LaunchEnv{stream, nullptr, nullptr, nullptr, &ctx->error, ctx->hints};
    ctx->have_timing = true;
    ctx->timing_query_only = false;
    return LaunchEnv{stream, ctx->ev[0], ctx->ev[1], ctx->ev[2], &ctx->error, ctx->hints};
}

// Every entry point runs on ctx's device and leaves the CALLER's current device as it found it (a
// torch caller whose current device differs must not have it switched under its feet).
struct DeviceScope {
    int saved = -1;
    bool switched = false;
    int enter(pgt_ctx *ctx) {
        if (!ctx) return ctx_fail(nullptr, PGT_EARG, "NULL context");
        if (hipGetDevice(&saved) != hipSuccess) saved = -1;
        if (saved == ctx->device) return PGT_OK;
        if (int rc = hip_check(ctx, hipSetDevice(ctx->device), "hipSetDevice")) return rc;
        switched = true;
        return PGT_OK;
    }
    ~DeviceScope() {
        if (switched && saved >= 0) (void)hipSetDevice(saved);
    }
};
#define PGT_USE_DEVICE(ctx)  \
    DeviceScope device_scope; \
    if (int rc_ = device_scope.enter(ctx)) return rc_

// What is particular to one statistic of the (freq, nInd) front ends (pgt_{dxy,fst,pi}_pops_reduce and _dev); the rest of
// their argument checks is one text for all of them: pops_check_range, pops_check_dev, pops_reduce_dev, pops_reduce_host.
struct PopsStat {
    const char *who;                                          // the prefix of every message
    uint32_t min_pops;                                        // min_pops <= n_pops <= max_pops
    bool minind_from_1;                                       // minind < 1 is refused (dxy takes it as it comes)
    uint64_t (*tables)(uint32_t n_pops);                      // row tables, and totals, of one call
    const char *tables_word;                                  // ... and the word for them in the overflow message
    size_t row_bytes;
    size_t (*tree_bytes)(uint32_t n_pops, uint64_t n_sites);
    uint32_t max_pops = (uint32_t)kPopsMaxPops;               // (the trios of pgt_dstat_pops_reduce stop at 7)
    // a workspace that holds more than the tree and depends on the window count (pgt_pbs_pops_reduce): its size instead of
    // tree_bytes, and its name in the messages
    size_t (*work_bytes)(uint32_t n_pops, uint64_t n_sites, uint64_t n_win) = nullptr;
    const char *work_word = "tree";
};
uint64_t pops_pairs(uint32_t n_pops) { return (uint64_t)n_pops * (n_pops - 1) / 2; }
uint64_t pops_each(uint32_t n_pops) { return n_pops; }
uint64_t pops_trios(uint32_t n_pops) { return (uint64_t)(n_pops - 1) * (n_pops - 2) * (n_pops - 3) / 6; }  // C(n_pops - 1, 3): the last population is the outgroup

bool pops_in_range(const PopsStat &st, uint32_t n_pops) { return n_pops >= st.min_pops && n_pops <= st.max_pops; }
// a *_pops_tree_bytes: `sums` sums per table over the FST layout; 0 outside the statistic's populations
size_t pops_tree_bytes(const PopsStat &st, int sums, uint32_t n_pops, uint64_t n_sites) {
    if (!pops_in_range(st, n_pops)) return 0;
    return pops_tree_view(tree_layout(PGT_STAT_FST, n_sites), (int)st.tables(n_pops), sums, nullptr, 0).bytes;
}

// the bytes behind the `tree` (or `work`) argument of a call
size_t pops_work_bytes(const PopsStat &st, uint32_t n_pops, uint64_t n_sites, uint64_t n_win) {
    return st.work_bytes ? st.work_bytes(n_pops, n_sites, n_win) : st.tree_bytes(n_pops, n_sites);
}

// first in both forms, and before the device form's early PGT_OK
int pops_check_range(pgt_ctx *ctx, const PopsStat &st, uint32_t n_pops, int minind) {
    if (!pops_in_range(st, n_pops))
        return ctx_fail(ctx, PGT_EARG, std::string(st.who) + ": n_pops must be " + std::to_string(st.min_pops) + " ... " + std::to_string(st.max_pops));
    if (st.minind_from_1 && minind < 1) return ctx_fail(ctx, PGT_EARG, std::string(st.who) + ": minind must be at least 1");
    return PGT_OK;
}

// Every check of a *_pops_reduce_dev entry point.  *launch = false with PGT_OK: a shard without sites, windows and total.
int pops_check_dev(pgt_ctx *ctx, const PopsStat &st, const uint32_t *pos, const double *const *freq, const int32_t *const *nind,
                   uint32_t n_pops, uint64_t n, int minind, const pgt_win *win, uint64_t n_win, const void *out, size_t out_bytes,
                   const void *tot, const void *tree, size_t tree_bytes, bool *launch) {
    *launch = false;
    if (int rc = pops_check_range(ctx, st, n_pops, minind)) return rc;
    if (n == 0 && n_win == 0 && !tot) return PGT_OK;
    const std::string who = std::string(st.who) + ": ";
    if (!freq) return ctx_fail(ctx, PGT_EARG, who + "freq is NULL");
    if (!nind) return ctx_fail(ctx, PGT_EARG, who + "nind is NULL");
    if (!tree) return ctx_fail(ctx, PGT_EARG, who + st.work_word + " is NULL");
    if (n_win && !win) return ctx_fail(ctx, PGT_EARG, who + "win is NULL");
    if (n_win && !out) return ctx_fail(ctx, PGT_EARG, who + "out is NULL");
    if (n_win && n && !pos) return ctx_fail(ctx, PGT_EARG, who + "pos is NULL");  // windows without PGT_WIN_COORDS read pos[lo], pos[hi-1]
    for (uint32_t k = 0; k < n_pops; ++k) {
        const std::string at = "[" + std::to_string(k) + "]";
        if (!freq[k]) return ctx_fail(ctx, PGT_EARG, who + "freq" + at + " is NULL");
        if (!nind[k]) return ctx_fail(ctx, PGT_EARG, who + "nind" + at + " is NULL");
        if (!aligned16(freq[k])) return ctx_fail(ctx, PGT_EARG, who + "freq" + at + " is not 16-byte aligned");
        if (!aligned16(nind[k])) return ctx_fail(ctx, PGT_EARG, who + "nind" + at + " is not 16-byte aligned");
    }
    if (n >= (1ull << 32)) return ctx_fail(ctx, PGT_EARG, who + "n: at most 2^32-1 sites per call");
    if (!aligned16(tree)) return ctx_fail(ctx, PGT_EARG, who + st.work_word + " is not 16-byte aligned");
    if (tree_bytes < pops_work_bytes(st, n_pops, n, n_win))
        return ctx_fail(ctx, PGT_EARG, who + st.work_word + "_bytes too small (" + std::to_string(tree_bytes) + " bytes, " +
                                           std::to_string(pops_work_bytes(st, n_pops, n, n_win)) + " needed)");
    const uint64_t tables = st.tables(n_pops);
    if (n_win > UINT64_MAX / tables) return ctx_fail(ctx, PGT_EARG, who + st.tables_word + " * n_win overflows");
    if (int rc = room_check(ctx, (who + "out_bytes").c_str(), tables * n_win, st.row_bytes, out_bytes)) return rc;
    *launch = true;
    return PGT_OK;
}

// The body of every *_pops_reduce_dev entry point: the checks, then the statistic's launch (a launch_*_pops, or a callable
// with its arguments).
template <class Row, class Tot, class Launch>
int pops_reduce_dev(pgt_ctx *ctx, const PopsStat &st, Launch launch_stat, const uint32_t *pos, const double *const *freq,
                    const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind, const pgt_win *win, uint64_t n_win, Row *out,
                    size_t out_bytes, Tot *tot, void *tree, size_t tree_bytes, void *stream) {
    PGT_USE_DEVICE(ctx);
    bool launch;
    if (int rc = pops_check_dev(ctx, st, pos, freq, nind, n_pops, n, minind, win, n_win, out, out_bytes, tot, tree, tree_bytes, &launch)) return rc;
    if (!launch) return PGT_OK;
    return launch_stat(pos, freq, nind, n_pops, n, minind, win, n_win, out, tot, tree, events_for(ctx, stream));
}

}  // namespace

extern "C" {

int pgt_abi_version(void) { return PGT_ABI_VERSION; }

pgt_ctx *pgt_open(int device) {
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev == 0) {
        set_global_error(std::string("pgt_open: no HIP device available (") +
                         (e != hipSuccess ? hipGetErrorString(e) : "device count is 0") +
                         "); libpgtwin has no CPU fallback");
        return nullptr;
    }
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= n_dev) {
        set_global_error("pgt_open: device ordinal out of range");
        return nullptr;
    }
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) {
        set_global_error(std::string("pgt_open: hipGetDeviceProperties: ") + hipGetErrorString(e));
        return nullptr;
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_global_error(std::string("pgt_open: device is ") + prop.gcnArchName +
                         ", but libpgtwin carries gfx950 (MI355X) code objects only");
        return nullptr;
    }
    int caller_device = -1;
    if (hipGetDevice(&caller_device) != hipSuccess) caller_device = -1;
    if ((e = hipSetDevice(device)) != hipSuccess) {
        set_global_error(std::string("pgt_open: hipSetDevice: ") + hipGetErrorString(e));
        return nullptr;
    }
    struct Restore {  // the caller's current device is left as it was found
        int dev, ctx_dev;
        ~Restore() { if (dev >= 0 && dev != ctx_dev) (void)hipSetDevice(dev); }
    } restore{caller_device, device};
    std::string init_err;
    if (init_kernels(&init_err) != PGT_OK || init_af_kernels(&init_err) != PGT_OK || init_dxy_pops_kernels(&init_err) != PGT_OK ||
        init_fst_pops_kernels(&init_err) != PGT_OK || init_dstat_pops_kernels(&init_err) != PGT_OK ||
        init_fd_pops_kernels(&init_err) != PGT_OK || init_f3_pops_kernels(&init_err) != PGT_OK || init_pbs_pops_kernels(&init_err) != PGT_OK ||
        init_f4_pops_kernels(&init_err) != PGT_OK || init_f4ratio_pops_kernels(&init_err) != PGT_OK) {
        set_global_error("pgt_open: " + init_err);
        return nullptr;
    }
    pgt_ctx *ctx = new pgt_ctx;
    ctx->device = device;
    if (const char *e = std::getenv("PGT_FST_BUILD_BLOCKS")) ctx->hints.fst_build_blocks = (uint32_t)std::max(std::atoi(e), 0);  // a testing knob, see Hints
    for (auto &ev : ctx->ev)
        if ((e = hipEventCreate(&ev)) != hipSuccess) {
            set_global_error(std::string("pgt_open: hipEventCreate: ") + hipGetErrorString(e));
            pgt_close(ctx);
            return nullptr;
        }
    return ctx;
}

void pgt_close(pgt_ctx *ctx) {
    if (!ctx) return;
    int saved = -1;
    const bool sw = hipGetDevice(&saved) == hipSuccess && saved != ctx->device && hipSetDevice(ctx->device) == hipSuccess;
    host_io_release(ctx);
    for (auto &ev : ctx->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (sw) (void)hipSetDevice(saved);
    delete ctx;
}

int pgt_prepare_host_io(pgt_ctx *ctx, uint64_t expected_column_bytes) {
    PGT_USE_DEVICE(ctx);
    // the ring only when uploads will take it (0 = unknown: yes); 15 ms of hipHostMalloc a small input need not wait for
    const bool ring = expected_column_bytes == 0 || expected_column_bytes >= 4 * HostIo::kChunk;
    if (ring)
        if (int rc = ring_prepare(ctx)) return rc;
    // The FIRST copy of a process in each direction and flavour pays for the runtime's own set-up (its DMA queues and staging
    // buffers: 20-30 ms for the first GPU operation of any kind, 8-9 ms more for the first host-to-device DMA, ~5 ms for the first
    // small pageable copy; tools/probes/first_use_probe.cpp, host_api_probe.py) — pay it here, beside the caller's parse, with
    // 64 KiB instead of inside the first reduce.
    HostIo &io = ctx->io;
    void *scratch = nullptr;
    if (int rc = workspace(ctx, HostIo::kWin, 65536, &scratch)) return rc;
    std::vector<char> pageable(65536, 0);
    void *pinned = ring ? static_cast<void *>(io.pin[0]) : nullptr;
    if (!pinned)
        if (int rc = hip_check(ctx, hipHostMalloc(&pinned, 65536, hipHostMallocDefault), "host io warm-up: hipHostMalloc")) return rc;
    int rc = hip_check(ctx, hipMemcpyAsync(scratch, pinned, 65536, hipMemcpyHostToDevice, io.copy_stream), "host io warm-up");
    if (!rc) rc = hip_check(ctx, hipStreamSynchronize(io.copy_stream), "host io warm-up");
    if (!ring) (void)hipHostFree(pinned);
    if (rc) return rc;
    if (int rc2 = hip_check(ctx, hipMemcpy(scratch, pageable.data(), pageable.size(), hipMemcpyHostToDevice), "host io warm-up")) return rc2;
    return hip_check(ctx, hipMemcpy(pageable.data(), scratch, pageable.size(), hipMemcpyDeviceToHost), "host io warm-up");
}

const char *pgt_last_error(const pgt_ctx *ctx) {
    if (ctx) return ctx->error.c_str();
    return global_error().c_str();
}

size_t pgt_tree_bytes(int stat, uint64_t n_sites) {
    if (stat < PGT_STAT_FST || stat > PGT_STAT_EXT) return 0;
    return tree_layout(stat, n_sites).bytes;
}

int pgt_set_profiling(pgt_ctx *ctx, int enabled) {
    if (!ctx) return ctx_fail(nullptr, PGT_EARG, "NULL context");
    ctx->profiling = enabled != 0;
    ctx->have_timing = false;
    return PGT_OK;
}

int pgt_set_max_window(pgt_ctx *ctx, uint64_t max_window_sites) {
    if (!ctx) return ctx_fail(nullptr, PGT_EARG, "NULL context");
    ctx->hints.max_window = max_window_sites;
    ctx->hints.typical_window = 0;  // the explicit value stands for the typical length too
    return PGT_OK;
}

int pgt_set_typical_window(pgt_ctx *ctx, uint64_t typical_sites) {
    if (!ctx) return ctx_fail(nullptr, PGT_EARG, "NULL context");
    ctx->hints.typical_window = typical_sites;
    return PGT_OK;
}

int pgt_table_hints(const pgt_win *win, uint64_t n_win, uint64_t *max_window, uint64_t *typical_window, uint64_t *window_step) {
    if ((n_win && !win) || !max_window || !typical_window || !window_step)
        return ctx_fail(nullptr, PGT_EARG, "pgt_table_hints: NULL argument");
    derive_hints(win, n_win, max_window, typical_window, window_step);
    if (*window_step == 0) *window_step = UINT64_MAX;  // "one wave per window", said explicitly: 0 would let a slice estimate its own
    return PGT_OK;
}

int pgt_set_window_step(pgt_ctx *ctx, uint64_t step_sites) {
    if (!ctx) return ctx_fail(nullptr, PGT_EARG, "NULL context");
    ctx->hints.window_step = step_sites;
    return PGT_OK;
}

int pgt_last_kernel_ms(pgt_ctx *ctx, float *build_ms, float *query_ms) {
    if (!ctx || !build_ms || !query_ms) return ctx_fail(ctx, PGT_EARG, "pgt_last_kernel_ms: NULL argument");
    if (!ctx->have_timing) return ctx_fail(ctx, PGT_EARG, "pgt_last_kernel_ms: no profiled call yet");
    if (int rc = hip_check(ctx, hipEventSynchronize(ctx->ev[2]), "hipEventSynchronize")) return rc;
    *build_ms = 0.0f;
    if (!ctx->timing_query_only)
        if (int rc = hip_check(ctx, hipEventElapsedTime(build_ms, ctx->ev[0], ctx->ev[1]), "hipEventElapsedTime")) return rc;
    return hip_check(ctx, hipEventElapsedTime(query_ms, ctx->ev[1], ctx->ev[2]), "hipEventElapsedTime");
}

/* ---------------- device-resident entry points ---------------- */

int pgt_fst_reduce_pairs_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *a, const double *const *b,
                             uint32_t n_pairs, uint64_t n, const pgt_win *win, uint64_t n_win, pgt_fst_row *out,
                             size_t out_bytes, void *tree, size_t tree_bytes, void *stream) {
    PGT_USE_DEVICE(ctx);
    if (n == 0 && n_win == 0) return PGT_OK;  // a shard without windows (more ranks than windows)
    if (!a || !b || n_pairs == 0 || !tree || (n_win && (!win || !out || !pos)))
        return ctx_fail(ctx, PGT_EARG, "pgt_fst_reduce: NULL argument");
    for (uint32_t p = 0; p < n_pairs; ++p)
        if (!a[p] || !b[p] || !aligned16(a[p]) || !aligned16(b[p]))
            return ctx_fail(ctx, PGT_EARG, "pgt_fst_reduce: f64 columns must be non-NULL and 16-byte aligned");
    if (!aligned16(tree) || tree_bytes < (size_t)n_pairs * pgt_tree_bytes(PGT_STAT_FST, n))
        return ctx_fail(ctx, PGT_EARG, "pgt_fst_reduce: tree workspace too small or misaligned");
    if (n_win > UINT64_MAX / n_pairs) return ctx_fail(ctx, PGT_EARG, "pgt_fst_reduce: n_pairs * n_win overflows");
    if (int rc = room_check(ctx, "pgt_fst_reduce", (uint64_t)n_pairs * n_win, sizeof(pgt_fst_row), out_bytes)) return rc;
    return launch_fst(pos, a, b, n_pairs, n, win, n_win, out, tree, events_for(ctx, stream));
}

int pgt_fst_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *a, const double *b, uint64_t n,
                       const pgt_win *win, uint64_t n_win, pgt_fst_row *out, size_t out_bytes, void *tree,
                       size_t tree_bytes, void *stream) {
    const double *pa[1] = {a}, *pb[1] = {b};
    return pgt_fst_reduce_pairs_dev(ctx, pos, pa, pb, 1, n, win, n_win, out, out_bytes, tree, tree_bytes, stream);
}

int pgt_het_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const int8_t *g, uint64_t n, const pgt_win *win,
                       uint64_t n_win, pgt_het_row *out, size_t out_bytes, void *tree, size_t tree_bytes, void *stream) {
    PGT_USE_DEVICE(ctx);
    if (n == 0 && n_win == 0) return PGT_OK;
    if (!g || !tree || (n_win && (!win || !out || !pos))) return ctx_fail(ctx, PGT_EARG, "pgt_het_reduce: NULL argument");
    if (!aligned16(g)) return ctx_fail(ctx, PGT_EARG, "pgt_het_reduce: genotype column must be 16-byte aligned");
    if (n >= (1ull << 32)) return ctx_fail(ctx, PGT_EARG, "pgt_het_reduce: at most 2^32-1 sites per call");
    if (!aligned16(tree) || tree_bytes < pgt_tree_bytes(PGT_STAT_HET, n))
        return ctx_fail(ctx, PGT_EARG, "pgt_het_reduce: tree workspace too small or misaligned");
    if (int rc = room_check(ctx, "pgt_het_reduce", n_win, sizeof(pgt_het_row), out_bytes)) return rc;
    return launch_het(pos, g, n, win, n_win, out, tree, events_for(ctx, stream));
}

int pgt_dxy_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *p1, const double *p2, const int32_t *n1,
                       const int32_t *n2, uint64_t n, int minind, const pgt_win *win, uint64_t n_win,
                       pgt_dxy_row *out, size_t out_bytes, pgt_dxy_total *tot, void *tree, size_t tree_bytes, void *stream) {
    PGT_USE_DEVICE(ctx);
    if (n == 0 && n_win == 0 && !tot) return PGT_OK;
    if (!p1 || !p2 || !n1 || !n2 || !tree || (n_win && (!win || !out)))
        return ctx_fail(ctx, PGT_EARG, "pgt_dxy_reduce: NULL argument");
    if (!aligned16(p1) || !aligned16(p2) || !aligned16(n1) || !aligned16(n2))
        return ctx_fail(ctx, PGT_EARG, "pgt_dxy_reduce: the f64 and i32 columns must be 16-byte aligned");
    if (n >= (1ull << 32)) return ctx_fail(ctx, PGT_EARG, "pgt_dxy_reduce: at most 2^32-1 sites per call");
    if (!aligned16(tree) || tree_bytes < pgt_tree_bytes(PGT_STAT_DXY, n))
        return ctx_fail(ctx, PGT_EARG, "pgt_dxy_reduce: tree workspace too small or misaligned");
    if (int rc = room_check(ctx, "pgt_dxy_reduce", n_win, sizeof(pgt_dxy_row), out_bytes)) return rc;
    return launch_dxy(pos, p1, p2, n1, n2, n, minind, win, n_win, out, tot, tree, events_for(ctx, stream));
}

int pgt_dxy_het_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *p1, const double *p2, const int32_t *n1,
                           const int32_t *n2, const int8_t *g1, const int8_t *g2, uint64_t n, int minind,
                           const pgt_win *win, uint64_t n_win, pgt_dxy_row *dxy_out, size_t dxy_out_bytes, pgt_dxy_total *tot,
                           pgt_het_row *het_out1, pgt_het_row *het_out2, size_t het_out_bytes, void *tree, size_t tree_bytes,
                           void *stream) {
    PGT_USE_DEVICE(ctx);
    if (n == 0 && n_win == 0 && !tot) return PGT_OK;
    if (!p1 || !p2 || !n1 || !n2 || !g1 || !g2 || !tree || (n_win && (!win || !dxy_out || !het_out1 || !het_out2 || !pos)))
        return ctx_fail(ctx, PGT_EARG, "pgt_dxy_het_reduce: NULL argument");
    if (!aligned16(p1) || !aligned16(p2) || !aligned16(g1) || !aligned16(g2) ||
        !aligned16(n1) || !aligned16(n2))
        return ctx_fail(ctx, PGT_EARG, "pgt_dxy_het_reduce: the f64, i32 and i8 columns must be 16-byte aligned");
    if (n >= (1ull << 32)) return ctx_fail(ctx, PGT_EARG, "pgt_dxy_het_reduce: at most 2^32-1 sites per call");
    if (!aligned16(tree) || tree_bytes < pgt_tree_bytes(PGT_STAT_DXY, n) + 2 * pgt_tree_bytes(PGT_STAT_HET, n))
        return ctx_fail(ctx, PGT_EARG, "pgt_dxy_het_reduce: tree workspace too small or misaligned");
    if (int rc = room_check(ctx, "pgt_dxy_het_reduce (dxy rows)", n_win, sizeof(pgt_dxy_row), dxy_out_bytes)) return rc;
    if (int rc = room_check(ctx, "pgt_dxy_het_reduce (het rows)", n_win, sizeof(pgt_het_row), het_out_bytes)) return rc;
    return launch_dxy_het(pos, p1, p2, n1, n2, g1, g2, n, minind, win, n_win, dxy_out, tot, het_out1, het_out2, tree,
                          events_for(ctx, stream));
}

size_t pgt_af_tree_bytes(uint32_t n_pops, uint64_t n_sites) {
    if (n_pops < 2 || n_pops > (uint32_t)kAfMaxPops) return 0;
    return af_tree_bytes(tree_layout(PGT_STAT_FST, n_sites), (int)(n_pops + n_pops * (n_pops - 1) / 2));
}

int pgt_fst_af_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const double *nsamp,
                          uint32_t n_pops, uint64_t n, const pgt_win *win, uint64_t n_win, pgt_fst_row *out, size_t out_bytes,
                          void *tree, size_t tree_bytes, void *stream) {
    PGT_USE_DEVICE(ctx);
    if (n == 0 && n_win == 0) return PGT_OK;
    if (!freq || !nsamp || !tree || (n_win && (!win || !out || !pos)))
        return ctx_fail(ctx, PGT_EARG, "pgt_fst_af_reduce: NULL argument");
    if (n_pops < 2 || n_pops > (uint32_t)kAfMaxPops) return ctx_fail(ctx, PGT_EARG, "pgt_fst_af_reduce: 2 <= n_pops <= 8");
    for (uint32_t k = 0; k < n_pops; ++k) {
        if (!freq[k] || !aligned16(freq[k]))
            return ctx_fail(ctx, PGT_EARG, "pgt_fst_af_reduce: frequency columns must be non-NULL and 16-byte aligned");
        if (!(nsamp[k] > 0.0)) return ctx_fail(ctx, PGT_EARG, "pgt_fst_af_reduce: sample sizes must be positive");
    }
    if (!aligned16(tree) || tree_bytes < pgt_af_tree_bytes(n_pops, n))
        return ctx_fail(ctx, PGT_EARG, "pgt_fst_af_reduce: tree workspace too small or misaligned");
    if (n_win > UINT64_MAX / 28) return ctx_fail(ctx, PGT_EARG, "pgt_fst_af_reduce: n_pairs * n_win overflows");
    if (int rc = room_check(ctx, "pgt_fst_af_reduce", (uint64_t)(n_pops * (n_pops - 1) / 2) * n_win, sizeof(pgt_fst_row), out_bytes)) return rc;
    return launch_fst_af(pos, freq, nsamp, n_pops, n, win, n_win, out, tree, events_for(ctx, stream));
}

// Each statistic's populations (min_pops, max_pops) are stated once, in its PopsStat: its *_pops_tree_bytes reads them there.
static const PopsStat kDxyPops = {"pgt_dxy_pops_reduce", 2, false, pops_pairs, "n_pairs", sizeof(pgt_dxy_row), pgt_dxy_pops_tree_bytes};
size_t pgt_dxy_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites) { return pops_tree_bytes(kDxyPops, 1, n_pops, n_sites); }

int pgt_dxy_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind,
                            uint32_t n_pops, uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_dxy_row *out,
                            size_t out_bytes, pgt_dxy_total *tot, void *tree, size_t tree_bytes, void *stream) {
    return pops_reduce_dev(ctx, kDxyPops, launch_dxy_pops, pos, freq, nind, n_pops, n, minind, win, n_win, out, out_bytes, tot, tree, tree_bytes, stream);
}

// minind >= 1: npool >= 2 and n1, n2 > 0 at every counted site
static const PopsStat kFstPops = {"pgt_fst_pops_reduce", 2, true, pops_pairs, "n_pairs", sizeof(pgt_fst_row), pgt_fst_pops_tree_bytes};
size_t pgt_fst_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites) { return pops_tree_bytes(kFstPops, 2, n_pops, n_sites); }

int pgt_fst_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind,
                            uint32_t n_pops, uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_fst_row *out,
                            size_t out_bytes, pgt_fst_total *tot, void *tree, size_t tree_bytes, void *stream) {
    return pops_reduce_dev(ctx, kFstPops, [](auto &&...a) { return launch_fst_pops(a..., FstPopsEstimator::WeirCockerham); },
                           pos, freq, nind, n_pops, n, minind, win, n_win, out, out_bytes, tot, tree, tree_bytes, stream);
}

// Hudson's estimator on the same columns, tree layout and row types: one more PopsStat, the other per-site function
size_t pgt_fst_hudson_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites) { return pgt_fst_pops_tree_bytes(n_pops, n_sites); }
// minind >= 1: 2 nind - 1 >= 1 at every counted site
static const PopsStat kFstHudsonPops = {"pgt_fst_hudson_pops_reduce", 2, true, pops_pairs, "n_pairs", sizeof(pgt_fst_row), pgt_fst_hudson_pops_tree_bytes};

int pgt_fst_hudson_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind,
                                   uint32_t n_pops, uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_fst_row *out,
                                   size_t out_bytes, pgt_fst_total *tot, void *tree, size_t tree_bytes, void *stream) {
    return pops_reduce_dev(ctx, kFstHudsonPops, [](auto &&...a) { return launch_fst_pops(a..., FstPopsEstimator::Hudson); },
                           pos, freq, nind, n_pops, n, minind, win, n_win, out, out_bytes, tot, tree, tree_bytes, stream);
}

// one table per population; minind >= 1: 2 nind - 1 >= 1 at every counted site
static const PopsStat kPiPops = {"pgt_pi_pops_reduce", 1, true, pops_each, "n_pops", sizeof(pgt_dxy_row), pgt_pi_pops_tree_bytes};
size_t pgt_pi_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites) {
    if (!pops_in_range(kPiPops, n_pops)) return 0;
    return (size_t)n_pops * tree_layout(PGT_STAT_DXY, n_sites).bytes;  // one tree of the two-population dxy layout per population
}

int pgt_pi_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind,
                           uint32_t n_pops, uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_dxy_row *out,
                           size_t out_bytes, pgt_dxy_total *tot, void *tree, size_t tree_bytes, void *stream) {
    return pops_reduce_dev(ctx, kPiPops, launch_pi_pops, pos, freq, nind, n_pops, n, minind, win, n_win, out, out_bytes, tot, tree, tree_bytes, stream);
}

// ABBA-BABA patterns of all ingroup trios against the last population: one more PopsStat, with an upper bound of its own
static const PopsStat kDstatPops = {"pgt_dstat_pops_reduce", 4, true, pops_trios, "n_trios", sizeof(pgt_dstat_row), pgt_dstat_pops_tree_bytes, 7};
size_t pgt_dstat_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites) { return pops_tree_bytes(kDstatPops, 3, n_pops, n_sites); }

int pgt_dstat_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind,
                              uint32_t n_pops, uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_dstat_row *out,
                              size_t out_bytes, pgt_dstat_total *tot, void *tree, size_t tree_bytes, void *stream) {
    return pops_reduce_dev(ctx, kDstatPops, launch_dstat_pops, pos, freq, nind, n_pops, n, minind, win, n_win, out, out_bytes, tot, tree, tree_bytes, stream);
}

// f_d / f_dM of the same trios: one more PopsStat; three sums per trio as D has, so the tree is the D call's size
size_t pgt_fd_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites) { return pgt_dstat_pops_tree_bytes(n_pops, n_sites); }
static const PopsStat kFdPops = {"pgt_fd_pops_reduce", 4, true, pops_trios, "n_trios", sizeof(pgt_fd_row), pgt_fd_pops_tree_bytes, 7};

int pgt_fd_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind,
                           uint32_t n_pops, uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_fd_row *out,
                           size_t out_bytes, pgt_fd_total *tot, void *tree, size_t tree_bytes, void *stream) {
    return pops_reduce_dev(ctx, kFdPops, launch_fd_pops, pos, freq, nind, n_pops, n, minind, win, n_win, out, out_bytes, tot, tree, tree_bytes, stream);
}

// f3 of ALL trios of the populations, each population of a trio as the target: one more PopsStat; three sums per trio as D has,
// so the tree is the D call's at one population more (C(n, 3) = C((n + 1) - 1, 3))
static uint64_t pops_all_trios(uint32_t n_pops) { return (uint64_t)n_pops * (n_pops - 1) * (n_pops - 2) / 6; }
// minind >= 1: 2 nind - 1 >= 1 at every counted site
static const PopsStat kF3Pops = {"pgt_f3_pops_reduce", 3, true, pops_all_trios, "n_trios", sizeof(pgt_f3_row), pgt_f3_pops_tree_bytes, 6};
size_t pgt_f3_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites) { return pops_tree_bytes(kF3Pops, 3, n_pops, n_sites); }

int pgt_f3_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind,
                           uint32_t n_pops, uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_f3_row *out,
                           size_t out_bytes, pgt_f3_total *tot, void *tree, size_t tree_bytes, void *stream) {
    return pops_reduce_dev(ctx, kF3Pops, launch_f3_pops, pos, freq, nind, n_pops, n, minind, win, n_win, out, out_bytes, tot, tree, tree_bytes, stream);
}

// The population branch statistic of the same trios, every population of a trio as the focal one: two passes of the walk and a
// finishing kernel behind one entry point per FST estimator; the workspace holds a pass's tree (f3's) and the passes' scratch
// rows and totals, so its size knows the window count.  minind >= 1: the estimators' divisors at every counted site
size_t pgt_pbs_pops_work_bytes(uint32_t n_pops, uint64_t n_sites, uint64_t n_win) {
    if (n_pops < 3 || n_pops > 6) return 0;
    return pbs_work(n_pops, n_sites, n_win).bytes;
}
static_assert(sizeof(pgt_pbs_row) == 88 && offsetof(pgt_pbs_row, num_ij) == 40 && sizeof(pgt_pbs_total) == 88 && offsetof(pgt_pbs_total, neff) == 72 &&
              sizeof(PbsPassRow) == 40 && sizeof(PbsPassTotal) == 40, "the documented layouts");
static const PopsStat kPbsPops = {"pgt_pbs_pops_reduce", 3, true, pops_all_trios, "n_trios", sizeof(pgt_pbs_row), nullptr, 6, pgt_pbs_pops_work_bytes, "work"};

int pgt_pbs_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind,
                            uint32_t n_pops, uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_pbs_row *out,
                            size_t out_bytes, pgt_pbs_total *tot, void *work, size_t work_bytes, void *stream) {
    return pops_reduce_dev(ctx, kPbsPops, [](auto &&...a) { return launch_pbs_pops(a..., FstPopsEstimator::WeirCockerham); },
                           pos, freq, nind, n_pops, n, minind, win, n_win, out, out_bytes, tot, work, work_bytes, stream);
}

int pgt_pbs_hudson_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind,
                                   uint32_t n_pops, uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_pbs_row *out,
                                   size_t out_bytes, pgt_pbs_total *tot, void *work, size_t work_bytes, void *stream) {
    return pops_reduce_dev(ctx, kPbsPops, [](auto &&...a) { return launch_pbs_pops(a..., FstPopsEstimator::Hudson); },
                           pos, freq, nind, n_pops, n, minind, win, n_win, out, out_bytes, tot, work, work_bytes, stream);
}

// f4 of ALL quartets of the populations, each quartet in its three pairings: one more PopsStat; three sums per quartet
static uint64_t pops_all_quartets(uint32_t n_pops) { return (uint64_t)n_pops * (n_pops - 1) * (n_pops - 2) * (n_pops - 3) / 24; }
// minind >= 1: what pgt_dstat_pops_reduce_dev accepts (the counts decide the predicate alone)
static const PopsStat kF4Pops = {"pgt_f4_pops_reduce", 4, true, pops_all_quartets, "n_quartets", sizeof(pgt_f4_row), pgt_f4_pops_tree_bytes, 6};
size_t pgt_f4_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites) { return pops_tree_bytes(kF4Pops, 3, n_pops, n_sites); }
static_assert(sizeof(pgt_f4_row) == 48 && offsetof(pgt_f4_row, reserved_) == 16 && offsetof(pgt_f4_row, f4_ij_kl) == offsetof(pgt_f3_row, f3_i) &&
              offsetof(pgt_f4_row, f4_ik_jl) == offsetof(pgt_f3_row, f3_j) && offsetof(pgt_f4_row, f4_il_jk) == offsetof(pgt_f3_row, f3_k) &&
              sizeof(pgt_f4_total) == 40 && offsetof(pgt_f4_total, neff) == 24 && sizeof(pgt_f4_jack) == 48, "the documented layouts");

int pgt_f4_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind,
                           uint32_t n_pops, uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_f4_row *out,
                           size_t out_bytes, pgt_f4_total *tot, void *tree, size_t tree_bytes, void *stream) {
    return pops_reduce_dev(ctx, kF4Pops, launch_f4_pops, pos, freq, nind, n_pops, n, minind, win, n_win, out, out_bytes, tot, tree, tree_bytes, stream);
}

// The f4-ratio sums of ALL triples of the middle populations between the first population and the last: one more PopsStat;
// three sums per triple.  minind >= 1: what pgt_f4_pops_reduce_dev accepts (the counts decide the predicate alone)
static uint64_t pops_middle_triples(uint32_t n_pops) { return (uint64_t)(n_pops - 2) * (n_pops - 3) * (n_pops - 4) / 6; }
static const PopsStat kF4RatioPops = {"pgt_f4ratio_pops_reduce", 5, true, pops_middle_triples, "n_triples", sizeof(pgt_f4ratio_row), pgt_f4ratio_pops_tree_bytes, 7};
size_t pgt_f4ratio_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites) { return pops_tree_bytes(kF4RatioPops, 3, n_pops, n_sites); }
static_assert(sizeof(pgt_f4ratio_row) == 48 && offsetof(pgt_f4ratio_row, reserved_) == 16 && offsetof(pgt_f4ratio_row, g_ij) == offsetof(pgt_f4_row, f4_ij_kl) &&
              offsetof(pgt_f4ratio_row, g_ik) == offsetof(pgt_f4_row, f4_ik_jl) && offsetof(pgt_f4ratio_row, g_jk) == offsetof(pgt_f4_row, f4_il_jk) &&
              sizeof(pgt_f4ratio_total) == 40 && offsetof(pgt_f4ratio_total, neff) == 24 && sizeof(pgt_f4ratio_jack) == 48, "the documented layouts");

int pgt_f4ratio_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind,
                                uint32_t n_pops, uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_f4ratio_row *out,
                                size_t out_bytes, pgt_f4ratio_total *tot, void *tree, size_t tree_bytes, void *stream) {
    return pops_reduce_dev(ctx, kF4RatioPops, launch_f4ratio_pops, pos, freq, nind, n_pops, n, minind, win, n_win, out, out_bytes, tot, tree, tree_bytes, stream);
}

// Block jackknife of the rows above: its own checks (no columns, no window table), the message prefix of both forms.
// One text for the estimators (D: pgt_dstat_jackknife; the mean of f3: pgt_f3_jackknife; the mean of f4: pgt_f4_jackknife): rows
// and results of all are 48 bytes, so plan, workspace and every check are the same, under the entry's own prefix, name of the
// tables and largest number of them.  The ratio of the f4-ratio (pgt_f4ratio_jackknife) goes through them too, with six items
// per table where the others have three: its results and its workspace are larger by that.
size_t pgt_dstat_jackknife_work_bytes(uint32_t n_trios, uint64_t n_win) {
    if (n_trios < 1 || n_trios > kJackMaxTrios) return 0;
    return jack_work(n_trios, n_win).bytes;
}
size_t pgt_f3_jackknife_work_bytes(uint32_t n_trios, uint64_t n_win) { return pgt_dstat_jackknife_work_bytes(n_trios, n_win); }
size_t pgt_f4_jackknife_work_bytes(uint32_t n_quartets, uint64_t n_win) {
    return n_quartets <= kJackMaxQuartets ? pgt_dstat_jackknife_work_bytes(n_quartets, n_win) : 0;
}

size_t pgt_f4ratio_jackknife_work_bytes(uint32_t n_triples, uint64_t n_win) {
    if (n_triples < 1 || n_triples > kJackMaxTriples) return 0;
    return jack_work(n_triples, n_win, kJackRatioItems).bytes;
}

// PBS and PBSn1 (pgt_pbs_jackknife) go through them as well, over rows of 88 bytes with six sums: the row size, the rows'
// alignment (8 bytes) and the sums of the workspace are the estimator's.
size_t pgt_pbs_jackknife_work_bytes(uint32_t n_trios, uint64_t n_win) {
    if (n_trios < 1 || n_trios > kJackMaxTrios) return 0;
    return jack_work(n_trios, n_win, kJackPbsItems, kJackPbsSums).bytes;
}

enum JackEstimator { kJackD, kJackF3Mean, kJackF4Mean, kJackF4Ratio, kJackPbs };
static const char *jack_who(JackEstimator est) {
    if (est == kJackPbs) return "pgt_pbs_jackknife: ";
    return est == kJackD ? "pgt_dstat_jackknife: " : (est == kJackF3Mean ? "pgt_f3_jackknife: " : (est == kJackF4Mean ? "pgt_f4_jackknife: " : "pgt_f4ratio_jackknife: "));
}
static const char *jack_tables_word(JackEstimator est) { return est == kJackF4Mean ? "n_quartets" : (est == kJackF4Ratio ? "n_triples" : "n_trios"); }
static uint32_t jack_max_tables(JackEstimator est) { return est == kJackF4Mean ? kJackMaxQuartets : (est == kJackF4Ratio ? kJackMaxTriples : kJackMaxTrios); }
static int jack_items(JackEstimator est) { return est == kJackF4Ratio ? kJackRatioItems : (est == kJackPbs ? kJackPbsItems : kJackTopologies); }
static int jack_sums(JackEstimator est) { return est == kJackPbs ? kJackPbsSums : kJackSums; }
static size_t jack_row_bytes(JackEstimator est) { return est == kJackPbs ? sizeof(pgt_pbs_row) : sizeof(pgt_dstat_row); }
static_assert(kJackMaxQuartets <= kJackMaxTrios, "jack_work is sized for up to kJackMaxTrios tables");

static int jack_check_range(pgt_ctx *ctx, JackEstimator est, uint32_t n_trios, uint64_t n_win) {
    const std::string who = jack_who(est), word = jack_tables_word(est);
    if (n_trios < 1 || n_trios > jack_max_tables(est))
        return ctx_fail(ctx, PGT_EARG, who + word + " must be 1 ... " + std::to_string(jack_max_tables(est)));
    if (n_win > (UINT64_MAX / jack_row_bytes(est)) / n_trios) return ctx_fail(ctx, PGT_EARG, who + word + " * n_win overflows");
    return PGT_OK;
}
static_assert(sizeof(pgt_f3_row) == sizeof(pgt_dstat_row) && sizeof(pgt_f3_jack) == sizeof(pgt_dstat_jack), "one set of jackknife checks");
static_assert(sizeof(pgt_f4_row) == sizeof(pgt_dstat_row) && sizeof(pgt_f4_jack) == sizeof(pgt_dstat_jack), "one set of jackknife checks");
static_assert(sizeof(pgt_f4ratio_row) == sizeof(pgt_dstat_row) && sizeof(pgt_f4ratio_jack) == sizeof(pgt_dstat_jack), "one set of jackknife checks");
static_assert(sizeof(pgt_pbs_row) == 88 && sizeof(pgt_pbs_jack) == sizeof(pgt_dstat_jack) && offsetof(pgt_pbs_jack, stat_jack) == 8 && offsetof(pgt_pbs_jack, n_blocks) == 40,
              "one set of jackknife checks: the results of all estimators are one layout");

static int jackknife_dev(pgt_ctx *ctx, JackEstimator est, const void *rows, uint64_t n_win, uint32_t n_trios, void *out,
                         size_t out_bytes, void *work, size_t work_bytes, void *stream) {
    const std::string who = jack_who(est);
    if (int rc = jack_check_range(ctx, est, n_trios, n_win)) return rc;
    if (n_win && !rows) return ctx_fail(ctx, PGT_EARG, who + "rows is NULL");
    if (!out) return ctx_fail(ctx, PGT_EARG, who + "out is NULL");
    if (!work) return ctx_fail(ctx, PGT_EARG, who + "work is NULL");
    if (est == kJackPbs) {  // an 88-byte row at an odd index is not 16-byte aligned: its loads are 8 bytes wide
        if (reinterpret_cast<uintptr_t>(rows) & 7u) return ctx_fail(ctx, PGT_EARG, who + "rows is not 8-byte aligned");
    } else if (!aligned16(rows)) {
        return ctx_fail(ctx, PGT_EARG, who + "rows is not 16-byte aligned");
    }
    if (reinterpret_cast<uintptr_t>(out) & 7u) return ctx_fail(ctx, PGT_EARG, who + "out is not 8-byte aligned");
    if (!aligned16(work)) return ctx_fail(ctx, PGT_EARG, who + "work is not 16-byte aligned");
    if (int rc = room_check(ctx, (who + "out_bytes").c_str(), (uint64_t)n_trios * jack_items(est), sizeof(pgt_dstat_jack), out_bytes)) return rc;
    const size_t need = jack_work(n_trios, n_win, jack_items(est), jack_sums(est)).bytes;
    if (work_bytes < need)
        return ctx_fail(ctx, PGT_EARG, who + "work_bytes too small (" + std::to_string(work_bytes) + " bytes, " + std::to_string(need) + " needed)");
    void *q0 = nullptr, *q1 = nullptr;
    if (ctx->profiling) {  // the whole call is the "query"; there is no build
        q0 = ctx->ev[1];
        q1 = ctx->ev[2];
        ctx->have_timing = true;
        ctx->timing_query_only = true;
    }
    if (est == kJackPbs)
        return launch_pbs_jackknife(static_cast<const pgt_pbs_row *>(rows), n_win, n_trios, static_cast<pgt_pbs_jack *>(out), work, stream, q0, q1, &ctx->error);
    if (est == kJackF4Ratio)
        return launch_f4ratio_jackknife(static_cast<const pgt_f4ratio_row *>(rows), n_win, n_trios, static_cast<pgt_f4ratio_jack *>(out), work, stream, q0, q1, &ctx->error);
    if (est == kJackF4Mean)
        return launch_f4_jackknife(static_cast<const pgt_f4_row *>(rows), n_win, n_trios, static_cast<pgt_f4_jack *>(out), work, stream, q0, q1, &ctx->error);
    if (est == kJackF3Mean)
        return launch_f3_jackknife(static_cast<const pgt_f3_row *>(rows), n_win, n_trios, static_cast<pgt_f3_jack *>(out), work, stream, q0, q1, &ctx->error);
    return launch_dstat_jackknife(static_cast<const pgt_dstat_row *>(rows), n_win, n_trios, static_cast<pgt_dstat_jack *>(out), work, stream, q0, q1, &ctx->error);
}

int pgt_dstat_jackknife_dev(pgt_ctx *ctx, const pgt_dstat_row *rows, uint64_t n_win, uint32_t n_trios, pgt_dstat_jack *out,
                            size_t out_bytes, void *work, size_t work_bytes, void *stream) {
    PGT_USE_DEVICE(ctx);
    return jackknife_dev(ctx, kJackD, rows, n_win, n_trios, out, out_bytes, work, work_bytes, stream);
}

// out: 3 n_trios items, u = 3 t + c with c the target i / j / k of trio t
int pgt_f3_jackknife_dev(pgt_ctx *ctx, const pgt_f3_row *rows, uint64_t n_win, uint32_t n_trios, pgt_f3_jack *out,
                         size_t out_bytes, void *work, size_t work_bytes, void *stream) {
    PGT_USE_DEVICE(ctx);
    return jackknife_dev(ctx, kJackF3Mean, rows, n_win, n_trios, out, out_bytes, work, work_bytes, stream);
}

// out: 3 n_quartets items, u = 3 q + c with c the pairing (ij;kl) / (ik;jl) / (il;jk) of quartet q
int pgt_f4_jackknife_dev(pgt_ctx *ctx, const pgt_f4_row *rows, uint64_t n_win, uint32_t n_quartets, pgt_f4_jack *out,
                         size_t out_bytes, void *work, size_t work_bytes, void *stream) {
    PGT_USE_DEVICE(ctx);
    return jackknife_dev(ctx, kJackF4Mean, rows, n_win, n_quartets, out, out_bytes, work, work_bytes, stream);
}

// out: 6 n_triples items, u = 6 t + c with c the (B, X, C) of middle triple t
int pgt_f4ratio_jackknife_dev(pgt_ctx *ctx, const pgt_f4ratio_row *rows, uint64_t n_win, uint32_t n_triples, pgt_f4ratio_jack *out,
                              size_t out_bytes, void *work, size_t work_bytes, void *stream) {
    PGT_USE_DEVICE(ctx);
    return jackknife_dev(ctx, kJackF4Ratio, rows, n_win, n_triples, out, out_bytes, work, work_bytes, stream);
}

// out: 6 n_trios items, u = 6 t + c: PBS (c < 3) and PBSn1 (c >= 3) with population c % 3 of trio t as the focal one
int pgt_pbs_jackknife_dev(pgt_ctx *ctx, const pgt_pbs_row *rows, uint64_t n_win, uint32_t n_trios, pgt_pbs_jack *out,
                          size_t out_bytes, void *work, size_t work_bytes, void *stream) {
    PGT_USE_DEVICE(ctx);
    return jackknife_dev(ctx, kJackPbs, rows, n_win, n_trios, out, out_bytes, work, work_bytes, stream);
}

size_t pgt_align_workspace_bytes(uint32_t n_files, uint64_t n_rows_file0) {
    if (n_files < 2 || n_files > (uint32_t)kAlignMaxFiles) return 0;
    return align_layout(n_files, n_rows_file0).bytes;
}

int pgt_sites_align(pgt_ctx *ctx, const uint32_t *const *pos, const uint64_t *n_rows, uint32_t n_files, const pgt_seg *seg,
                    size_t n_seg, uint32_t *const *idx, uint64_t cap, uint64_t *seg_count, uint64_t *n_common, void *work,
                    size_t work_bytes, void *stream) {
    PGT_USE_DEVICE(ctx);
    if (n_files < 2 || n_files > (uint32_t)kAlignMaxFiles) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: n_files must be 2 ... 8");
    if (!pos) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: pos is NULL");
    if (!n_rows) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: n_rows is NULL");
    if (!idx) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: idx is NULL");
    if (!n_common) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: n_common is NULL");
    if (n_seg && !seg) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: seg is NULL");
    if (n_seg && !seg_count) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: seg_count is NULL");
    if (!work) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: work is NULL");
    if (n_seg % n_files != 0) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: n_seg is not a multiple of n_files");
    const size_t n_chr = n_seg / n_files;
    if (n_chr > kAlignMaxChr) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: at most " + std::to_string(kAlignMaxChr) + " matched chromosomes per call");
    for (uint32_t k = 0; k < n_files; ++k) {
        const std::string at = "[" + std::to_string(k) + "]";
        if (n_rows[k] >= 0xFFFFFFFFull) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: n_rows" + at + ": at most 2^32-2 rows per file");
        if (n_rows[k] && !pos[k]) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: pos" + at + " is NULL");
        if (n_rows[k] && (reinterpret_cast<uintptr_t>(pos[k]) & 3u)) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: pos" + at + " is not 4-byte aligned");
        if (cap && !idx[k]) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: idx" + at + " is NULL");
        uint64_t end = 0;  // a file's segments follow one another
        for (size_t m = 0; m < n_chr; ++m) {
            const pgt_seg &sg = seg[m * n_files + k];
            if (sg.off > n_rows[k] || sg.len > n_rows[k] - sg.off)
                return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: seg[" + std::to_string(m * n_files + k) + "] runs beyond n_rows" + at);
            if (sg.off < end) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: seg[" + std::to_string(m * n_files + k) + "] starts before the end of the file's previous segment");
            end = sg.off + sg.len;
        }
    }
    if (!aligned16(work)) return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: work is not 16-byte aligned");
    if (work_bytes < pgt_align_workspace_bytes(n_files, n_rows[0]))
        return ctx_fail(ctx, PGT_EARG, "pgt_sites_align: work_bytes too small (" + std::to_string(work_bytes) + " bytes, " +
                                           std::to_string(pgt_align_workspace_bytes(n_files, n_rows[0])) + " needed)");
    if (int rc = launch_sites_align(pos, n_rows, n_files, seg, n_chr, idx, cap, seg_count, n_common, work, stream, &ctx->error)) return rc;
    if (*n_common > cap) return ctx_fail(ctx, PGT_ECAP, "pgt_sites_align: output capacity too small");
    return PGT_OK;
}

int pgt_gather_dev(pgt_ctx *ctx, void *dst, const void *src, const uint32_t *idx, uint64_t n, uint32_t elem_bytes, void *stream) {
    PGT_USE_DEVICE(ctx);
    if (elem_bytes != 4 && elem_bytes != 8) return ctx_fail(ctx, PGT_EARG, "pgt_gather: elem_bytes must be 4 or 8");
    if (n == 0) return PGT_OK;
    if (!dst) return ctx_fail(ctx, PGT_EARG, "pgt_gather: dst is NULL");
    if (!src) return ctx_fail(ctx, PGT_EARG, "pgt_gather: src is NULL");
    if (!idx) return ctx_fail(ctx, PGT_EARG, "pgt_gather: idx is NULL");
    if (n >= (1ull << 32)) return ctx_fail(ctx, PGT_EARG, "pgt_gather: n: at most 2^32-1 elements per call");
    if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & (elem_bytes - 1)) return ctx_fail(ctx, PGT_EARG, "pgt_gather: dst / src are not aligned to elem_bytes");
    if (reinterpret_cast<uintptr_t>(idx) & 3u) return ctx_fail(ctx, PGT_EARG, "pgt_gather: idx is not 4-byte aligned");
    return launch_gather(dst, src, idx, n, elem_bytes, stream, &ctx->error);
}

int pgt_extreme_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *score, uint64_t n, int mode, double cutoff,
                           const pgt_win *win, uint64_t n_win, pgt_ext_row *out, size_t out_bytes, void *tree,
                           size_t tree_bytes, void *stream) {
    PGT_USE_DEVICE(ctx);
    if (n == 0 && n_win == 0) return PGT_OK;
    if (!score || !tree || (n_win && (!win || !out || !pos))) return ctx_fail(ctx, PGT_EARG, "pgt_extreme_reduce: NULL argument");
    if (mode < PGT_EXT_IHS || mode > PGT_EXT_XP_MIN) return ctx_fail(ctx, PGT_EARG, "pgt_extreme_reduce: unknown mode");
    if (!aligned16(score)) return ctx_fail(ctx, PGT_EARG, "pgt_extreme_reduce: score column must be 16-byte aligned");
    if (n >= 0xFFFFFFFFull) return ctx_fail(ctx, PGT_EARG, "pgt_extreme_reduce: at most 2^32-2 sites per call");
    if (!aligned16(tree) || tree_bytes < pgt_tree_bytes(PGT_STAT_EXT, n))
        return ctx_fail(ctx, PGT_EARG, "pgt_extreme_reduce: tree workspace too small or misaligned");
    if (int rc = room_check(ctx, "pgt_extreme_reduce", n_win, sizeof(pgt_ext_row), out_bytes)) return rc;
    return launch_ext(pos, score, n, mode, cutoff, win, n_win, out, tree, events_for(ctx, stream));
}

/* ---------------- device-side text ingest ---------------- */

int pgt_ingest_text(pgt_ctx *ctx, const char *text, size_t len, const uint8_t *tokens, int n_tokens, pgt_ingest **out) {
    PGT_USE_DEVICE(ctx);
    return ingest_text(ctx->device, text, len, tokens, n_tokens, 0, out, &ctx->error);
}

int pgt_ingest_text_behind(pgt_ctx *ctx, const char *text, size_t len, const uint8_t *tokens, int n_tokens, uint64_t rows_in_front,
                           pgt_ingest **out) {
    PGT_USE_DEVICE(ctx);
    return ingest_text(ctx->device, text, len, tokens, n_tokens, rows_in_front, out, &ctx->error);
}

/* ---------------- multi-GPU row exchange ---------------- */

static_assert(sizeof(hipIpcMemHandle_t) == PGT_IPC_HANDLE_BYTES, "pgt_ipc_handle must hold a hipIpcMemHandle_t");

int pgt_peer_access(pgt_ctx *ctx, int peer_device) {
    PGT_USE_DEVICE(ctx);
    if (peer_device == ctx->device) return PGT_OK;
    int can = 0;
    if (int rc = hip_check(ctx, hipDeviceCanAccessPeer(&can, ctx->device, peer_device), "hipDeviceCanAccessPeer")) return rc;
    if (!can) return ctx_fail(ctx, PGT_EDEVICE, "pgt_peer_access: no peer access between the two devices");
    const hipError_t e = hipDeviceEnablePeerAccess(peer_device, 0);
    if (e == hipErrorPeerAccessAlreadyEnabled) {
        (void)hipGetLastError();
        return PGT_OK;
    }
    return hip_check(ctx, e, "hipDeviceEnablePeerAccess");
}

int pgt_rowbuf_create(pgt_ctx *ctx, size_t bytes, void **dev_ptr, pgt_ipc_handle *handle) {
    PGT_USE_DEVICE(ctx);
    if (!dev_ptr || !handle) return ctx_fail(ctx, PGT_EARG, "pgt_rowbuf_create: NULL argument");
    void *p = nullptr;
    if (int rc = hip_check(ctx, hipMalloc(&p, bytes ? bytes : 256), "pgt_rowbuf_create: hipMalloc")) return rc;
    hipIpcMemHandle_t h;
    if (int rc = hip_check(ctx, hipIpcGetMemHandle(&h, p), "pgt_rowbuf_create: hipIpcGetMemHandle")) {
        (void)hipFree(p);
        return rc;
    }
    std::memcpy(handle->opaque, &h, sizeof h);
    *dev_ptr = p;
    return PGT_OK;
}

int pgt_rowbuf_open(pgt_ctx *ctx, const pgt_ipc_handle *handle, void **dev_ptr) {
    PGT_USE_DEVICE(ctx);
    if (!dev_ptr || !handle) return ctx_fail(ctx, PGT_EARG, "pgt_rowbuf_open: NULL argument");
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle->opaque, sizeof h);
    void *p = nullptr;
    if (int rc = hip_check(ctx, hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess), "pgt_rowbuf_open: hipIpcOpenMemHandle"))
        return rc;
    *dev_ptr = p;
    return PGT_OK;
}

int pgt_rowbuf_close(pgt_ctx *ctx, void *dev_ptr, int owner) {
    PGT_USE_DEVICE(ctx);
    if (!dev_ptr) return PGT_OK;
    return owner ? hip_check(ctx, hipFree(dev_ptr), "pgt_rowbuf_close: hipFree")
                 : hip_check(ctx, hipIpcCloseMemHandle(dev_ptr), "pgt_rowbuf_close: hipIpcCloseMemHandle");
}

int pgt_rowbuf_read(pgt_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes, void *stream) {
    PGT_USE_DEVICE(ctx);
    if (bytes == 0) return PGT_OK;
    if (!host_dst || !dev_src) return ctx_fail(ctx, PGT_EARG, "pgt_rowbuf_read: NULL argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = hip_check(ctx, hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, s), "pgt_rowbuf_read: copy")) return rc;
    return hip_check(ctx, hipStreamSynchronize(s), "pgt_rowbuf_read: synchronize");
}

int pgt_rowbuf_fill(pgt_ctx *ctx, void *dev_ptr, size_t bytes, uint64_t seed, void *stream) {
    PGT_USE_DEVICE(ctx);
    if (bytes == 0) return PGT_OK;
    if (!dev_ptr || (bytes & 7u) || (reinterpret_cast<uintptr_t>(dev_ptr) & 7u))
        return ctx_fail(ctx, PGT_EARG, "pgt_rowbuf_fill: NULL or misaligned argument");
    return launch_fill_pattern(static_cast<uint64_t *>(dev_ptr), bytes / 8, seed, stream, &ctx->error);
}

/* ---------------- plain device buffers ---------------- */

int pgt_dev_alloc(pgt_ctx *ctx, size_t bytes, void **dev_ptr) {
    PGT_USE_DEVICE(ctx);
    if (!dev_ptr) return ctx_fail(ctx, PGT_EARG, "pgt_dev_alloc: NULL argument");
    return hip_check(ctx, hipMalloc(dev_ptr, bytes ? bytes : 16), "pgt_dev_alloc: hipMalloc");
}

int pgt_dev_memory(pgt_ctx *ctx, size_t *free_bytes, size_t *total_bytes) {
    PGT_USE_DEVICE(ctx);
    size_t f = 0, t = 0;
    if (int rc = hip_check(ctx, hipMemGetInfo(&f, &t), "pgt_dev_memory: hipMemGetInfo")) return rc;
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return PGT_OK;
}

int pgt_dev_free(pgt_ctx *ctx, void *dev_ptr) {
    PGT_USE_DEVICE(ctx);
    if (!dev_ptr) return PGT_OK;
    return hip_check(ctx, hipFree(dev_ptr), "pgt_dev_free: hipFree");
}

int pgt_dev_upload(pgt_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes) {
    PGT_USE_DEVICE(ctx);
    if (bytes == 0) return PGT_OK;
    if (!dev_dst || !host_src) return ctx_fail(ctx, PGT_EARG, "pgt_dev_upload: NULL argument");
    return hip_check(ctx, hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice), "pgt_dev_upload: hipMemcpy");
}

int pgt_dev_copy(pgt_ctx *dst_ctx, void *dst, pgt_ctx *src_ctx, const void *src, size_t bytes) {
    PGT_USE_DEVICE(dst_ctx);
    if (!src_ctx) return ctx_fail(dst_ctx, PGT_EARG, "pgt_dev_copy: NULL source context");
    if (bytes == 0) return PGT_OK;
    if (!dst || !src) return ctx_fail(dst_ctx, PGT_EARG, "pgt_dev_copy: NULL argument");
    if (src_ctx->device == dst_ctx->device)
        return hip_check(dst_ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice), "pgt_dev_copy: hipMemcpy");
    return hip_check(dst_ctx, hipMemcpyPeer(dst, dst_ctx->device, src, src_ctx->device, bytes), "pgt_dev_copy: hipMemcpyPeer");
}

/* ---------------- host-buffer entry points ---------------- */

extern "C++" {
namespace {

// What every *_cols entry point does around its device call: window table up (cached workspace), rows and tree from the
// cached workspace, kernels, rows down.  `run` gets (device windows, device rows, tree, tree bytes, device total or NULL).
// `tables` row tables of n_win rows each (pair-major) and as many totals where `tot` is given; tb = the tree's bytes.
template <class Row, class Tot, class Run>
int reduce_tables_with_workspace(pgt_ctx *ctx, const char *who, size_t tb, uint64_t tables, uint64_t n, const pgt_win *win, uint64_t n_win,
                                 Row *out, size_t out_bytes, Tot *tot, Run run) {
    ApiTrace trace(who);
    if (n_win > UINT64_MAX / tables) return ctx_fail(ctx, PGT_EARG, std::string(who) + ": the number of rows overflows");
    const uint64_t n_rows = tables * n_win;
    if (int rc = room_check(ctx, who, n_rows, sizeof(Row), out_bytes)) return rc;
    if (int rc = check_windows_host(ctx, win, n_win, n, true)) return rc;
    const HintScope hint(ctx, win, n_win);
    void *dwin = nullptr, *dout = nullptr, *dtree = nullptr, *dtot = nullptr;
    if (int rc = workspace(ctx, HostIo::kWin, n_win * sizeof(pgt_win), &dwin)) return rc;
    if (int rc = workspace(ctx, HostIo::kRows, n_rows * sizeof(Row), &dout)) return rc;
    if (int rc = workspace(ctx, HostIo::kTree, tb, &dtree)) return rc;
    if (tot)
        if (int rc = workspace(ctx, HostIo::kTot, tables * sizeof(Tot), &dtot)) return rc;
    trace.lap("workspace");
    if (n_win)
        if (int rc = hip_check(ctx, hipMemcpy(dwin, win, n_win * sizeof(pgt_win), hipMemcpyHostToDevice), "upload windows")) return rc;
    trace.lap("upload windows", n_win * sizeof(pgt_win));
    if (int rc = run(static_cast<const pgt_win *>(dwin), static_cast<Row *>(dout), dtree, tb, static_cast<Tot *>(dtot))) return rc;
    if (int rc = hip_check(ctx, hipStreamSynchronize(nullptr), "kernels")) return rc;
    trace.lap("kernels");
    if (n_win)
        if (int rc = hip_check(ctx, hipMemcpy(out, dout, n_rows * sizeof(Row), hipMemcpyDeviceToHost), "download rows")) return rc;
    if (tot)
        if (int rc = hip_check(ctx, hipMemcpy(tot, dtot, tables * sizeof(Tot), hipMemcpyDeviceToHost), "download total")) return rc;
    trace.lap("download rows", n_rows * sizeof(Row));
    return PGT_OK;
}

// The host-buffer form of a (freq, nInd) front end: checks, pos and n_pops x (freq, nind) up, the statistic's _dev entry point
// `dev` between reduce_tables_with_workspace's copies.  Rows and totals are written by every call (the query stores every row
// of every table, the build every tree level the query reads): nothing of the cached workspace survives.
template <class Row, class Tot>
int pops_reduce_host(pgt_ctx *ctx, const PopsStat &st,
                     int (*dev)(pgt_ctx *, const uint32_t *, const double *const *, const int32_t *const *, uint32_t, uint64_t, int,
                                const pgt_win *, uint64_t, Row *, size_t, Tot *, void *, size_t, void *),
                     const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                     const pgt_win *win, uint64_t n_win, Row *out, Tot *tot) {
    if (int rc = pops_check_range(ctx, st, n_pops, minind)) return rc;
    const std::string who = st.who;
    if (!freq || !nind || (n && !pos) || (n_win && (!win || !out))) return ctx_fail(ctx, PGT_EARG, who + ": NULL argument");
    for (uint32_t k = 0; k < n_pops; ++k)
        if (n && (!freq[k] || !nind[k])) return ctx_fail(ctx, PGT_EARG, who + ": NULL column");
    ApiTrace trace(st.who);
    const uint64_t tables = st.tables(n_pops);
    if (n_win > UINT64_MAX / tables / sizeof(Row)) return ctx_fail(ctx, PGT_EARG, who + ": " + st.tables_word + " * n_win overflows");
    DevBuf dpos, df[kPopsMaxPops], dn[kPopsMaxPops];
    UploadJob jobs[1 + 2 * kPopsMaxPops];
    int n_jobs = 0;
    jobs[n_jobs++] = {&dpos, pos, n * sizeof(uint32_t), "upload pos"};
    for (uint32_t k = 0; k < n_pops; ++k) {
        jobs[n_jobs++] = {&df[k], freq[k], n * sizeof(double), "upload freq"};
        jobs[n_jobs++] = {&dn[k], nind[k], n * sizeof(int32_t), "upload nind"};
    }
    if (int rc = upload_columns(ctx, jobs, n_jobs, trace)) return rc;
    const double *pf[kPopsMaxPops];
    const int32_t *pn[kPopsMaxPops];
    for (uint32_t k = 0; k < n_pops; ++k) { pf[k] = static_cast<double *>(df[k].p); pn[k] = static_cast<int32_t *>(dn[k].p); }
    const size_t row_bytes = (size_t)(tables * n_win) * sizeof(Row);
    return reduce_tables_with_workspace<Row>(ctx, st.who, pops_work_bytes(st, n_pops, n, n_win), tables, n, win, n_win, out, row_bytes, tot,
        [&](const pgt_win *dw, Row *dr, void *tree, size_t tb, Tot *dtot) {
            return dev(ctx, static_cast<uint32_t *>(dpos.p), pf, pn, n_pops, n, minind, dw, n_win, dr, row_bytes, dtot, tree, tb, nullptr);
        });
}

template <class Row, class Run>
int reduce_with_workspace(pgt_ctx *ctx, const char *who, int stat, uint64_t n, const pgt_win *win, uint64_t n_win, Row *out, size_t out_bytes,
                          pgt_dxy_total *tot, Run run) {
    return reduce_tables_with_workspace<Row>(ctx, who, pgt_tree_bytes(stat, n), 1, n, win, n_win, out, out_bytes, tot, run);
}

}  // namespace
}  // extern "C++"

int pgt_extreme_reduce_cols(pgt_ctx *ctx, const uint32_t *d_pos, const double *d_score, uint64_t n, int mode, double cutoff,
                            const pgt_win *win, uint64_t n_win, pgt_ext_row *out, size_t out_bytes) {
    PGT_USE_DEVICE(ctx);
    if ((n && (!d_pos || !d_score)) || (n_win && (!win || !out))) return ctx_fail(ctx, PGT_EARG, "pgt_extreme_reduce_cols: NULL argument");
    return reduce_with_workspace<pgt_ext_row>(ctx, "pgt_extreme_reduce_cols", PGT_STAT_EXT, n, win, n_win, out, out_bytes, nullptr,
        [&](const pgt_win *dw, pgt_ext_row *dr, void *tree, size_t tb, pgt_dxy_total *) {
            return pgt_extreme_reduce_dev(ctx, d_pos, d_score, n, mode, cutoff, dw, n_win, dr, n_win * sizeof(pgt_ext_row), tree, tb, nullptr);
        });
}

int pgt_extreme_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *score, uint64_t n, int mode, double cutoff,
                       const pgt_win *win, uint64_t n_win, pgt_ext_row *out) {
    PGT_USE_DEVICE(ctx);
    if ((n && (!pos || !score)) || (n_win && (!win || !out))) return ctx_fail(ctx, PGT_EARG, "pgt_extreme_reduce: NULL argument");
    ApiTrace trace("pgt_extreme_reduce");
    DevBuf dpos, ds;
    UploadJob jobs[] = {{&dpos, pos, n * sizeof(uint32_t), "upload pos"}, {&ds, score, n * sizeof(double), "upload scores"}};
    if (int rc = upload_columns(ctx, jobs, 2, trace)) return rc;
    return pgt_extreme_reduce_cols(ctx, static_cast<uint32_t *>(dpos.p), static_cast<double *>(ds.p), n, mode, cutoff, win, n_win, out,
                                   (size_t)n_win * sizeof(pgt_ext_row));
}


/* device columns (e.g. from pgt_ingest_text), window table and rows in HOST memory */
int pgt_fst_reduce_cols(pgt_ctx *ctx, const uint32_t *d_pos, const double *d_a, const double *d_b, uint64_t n,
                        const pgt_win *win, uint64_t n_win, pgt_fst_row *out, size_t out_bytes) {
    PGT_USE_DEVICE(ctx);
    if ((n && (!d_pos || !d_a || !d_b)) || (n_win && (!win || !out))) return ctx_fail(ctx, PGT_EARG, "pgt_fst_reduce: NULL argument");
    return reduce_with_workspace<pgt_fst_row>(ctx, "pgt_fst_reduce_cols", PGT_STAT_FST, n, win, n_win, out, out_bytes, nullptr,
        [&](const pgt_win *dw, pgt_fst_row *dr, void *tree, size_t tb, pgt_dxy_total *) {
            return pgt_fst_reduce_dev(ctx, d_pos, d_a, d_b, n, dw, n_win, dr, n_win * sizeof(pgt_fst_row), tree, tb, nullptr);
        });
}

int pgt_fst_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *a, const double *b, uint64_t n,
                   const pgt_win *win, uint64_t n_win, pgt_fst_row *out) {
    PGT_USE_DEVICE(ctx);
    if ((n && (!pos || !a || !b)) || (n_win && (!win || !out))) return ctx_fail(ctx, PGT_EARG, "pgt_fst_reduce: NULL argument");
    ApiTrace trace("pgt_fst_reduce");
    DevBuf dpos, da, db;
    UploadJob jobs[] = {{&dpos, pos, n * sizeof(uint32_t), "upload pos"}, {&da, a, n * sizeof(double), "upload a"},
                        {&db, b, n * sizeof(double), "upload b"}};
    if (int rc = upload_columns(ctx, jobs, 3, trace)) return rc;
    return pgt_fst_reduce_cols(ctx, static_cast<uint32_t *>(dpos.p), static_cast<double *>(da.p), static_cast<double *>(db.p), n,
                               win, n_win, out, n_win * sizeof(pgt_fst_row));
}

int pgt_het_reduce_cols(pgt_ctx *ctx, const uint32_t *d_pos, const int8_t *d_g, uint64_t n, const pgt_win *win,
                        uint64_t n_win, pgt_het_row *out, size_t out_bytes) {
    PGT_USE_DEVICE(ctx);
    if ((n && (!d_pos || !d_g)) || (n_win && (!win || !out))) return ctx_fail(ctx, PGT_EARG, "pgt_het_reduce: NULL argument");
    return reduce_with_workspace<pgt_het_row>(ctx, "pgt_het_reduce_cols", PGT_STAT_HET, n, win, n_win, out, out_bytes, nullptr,
        [&](const pgt_win *dw, pgt_het_row *dr, void *tree, size_t tb, pgt_dxy_total *) {
            return pgt_het_reduce_dev(ctx, d_pos, d_g, n, dw, n_win, dr, n_win * sizeof(pgt_het_row), tree, tb, nullptr);
        });
}

int pgt_het_reduce(pgt_ctx *ctx, const uint32_t *pos, const int8_t *g, uint64_t n, const pgt_win *win,
                   uint64_t n_win, pgt_het_row *out) {
    PGT_USE_DEVICE(ctx);
    if ((n && (!pos || !g)) || (n_win && (!win || !out))) return ctx_fail(ctx, PGT_EARG, "pgt_het_reduce: NULL argument");
    ApiTrace trace("pgt_het_reduce");
    DevBuf dpos, dg;
    UploadJob jobs[] = {{&dpos, pos, n * sizeof(uint32_t), "upload pos"}, {&dg, g, n * sizeof(int8_t), "upload genotypes"}};
    if (int rc = upload_columns(ctx, jobs, 2, trace)) return rc;
    return pgt_het_reduce_cols(ctx, static_cast<uint32_t *>(dpos.p), static_cast<int8_t *>(dg.p), n, win, n_win, out,
                               n_win * sizeof(pgt_het_row));
}

int pgt_dxy_reduce_cols(pgt_ctx *ctx, const uint32_t *d_pos, const double *d_p1, const double *d_p2, const int32_t *d_n1,
                        const int32_t *d_n2, uint64_t n, int minind, const pgt_win *win, uint64_t n_win,
                        pgt_dxy_row *out, size_t out_bytes, pgt_dxy_total *tot) {
    PGT_USE_DEVICE(ctx);
    if ((n && (!d_pos || !d_p1 || !d_p2 || !d_n1 || !d_n2)) || (n_win && (!win || !out)))
        return ctx_fail(ctx, PGT_EARG, "pgt_dxy_reduce: NULL argument");
    return reduce_with_workspace<pgt_dxy_row>(ctx, "pgt_dxy_reduce_cols", PGT_STAT_DXY, n, win, n_win, out, out_bytes, tot,
        [&](const pgt_win *dw, pgt_dxy_row *dr, void *tree, size_t tb, pgt_dxy_total *dtot) {
            return pgt_dxy_reduce_dev(ctx, d_pos, d_p1, d_p2, d_n1, d_n2, n, minind, dw, n_win, dr, n_win * sizeof(pgt_dxy_row), dtot, tree, tb,
                                      nullptr);
        });
}

int pgt_dxy_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *p1, const double *p2, const int32_t *n1,
                   const int32_t *n2, uint64_t n, int minind, const pgt_win *win, uint64_t n_win,
                   pgt_dxy_row *out, pgt_dxy_total *tot) {
    PGT_USE_DEVICE(ctx);
    if ((n && (!pos || !p1 || !p2 || !n1 || !n2)) || (n_win && (!win || !out)))
        return ctx_fail(ctx, PGT_EARG, "pgt_dxy_reduce: NULL argument");
    ApiTrace trace("pgt_dxy_reduce");
    DevBuf dpos, d1, d2, dn1, dn2;
    UploadJob jobs[] = {{&dpos, pos, n * sizeof(uint32_t), "upload pos"}, {&d1, p1, n * sizeof(double), "upload p1"},
                        {&d2, p2, n * sizeof(double), "upload p2"}, {&dn1, n1, n * sizeof(int32_t), "upload n1"},
                        {&dn2, n2, n * sizeof(int32_t), "upload n2"}};
    if (int rc = upload_columns(ctx, jobs, 5, trace)) return rc;
    return pgt_dxy_reduce_cols(ctx, static_cast<uint32_t *>(dpos.p), static_cast<double *>(d1.p), static_cast<double *>(d2.p),
                               static_cast<int32_t *>(dn1.p), static_cast<int32_t *>(dn2.p), n, minind, win, n_win, out,
                               n_win * sizeof(pgt_dxy_row), tot);
}

/* all pairs of n_pops populations: columns, table and rows in HOST memory (pops_reduce_host) */
int pgt_dxy_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                        uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_dxy_row *out, pgt_dxy_total *tot) {
    PGT_USE_DEVICE(ctx);
    return pops_reduce_host(ctx, kDxyPops, pgt_dxy_pops_reduce_dev, pos, freq, nind, n_pops, n, minind, win, n_win, out, tot);
}

/* FST of all pairs from per-population (freq, nInd) columns: the host-buffer form, as pgt_dxy_pops_reduce */
int pgt_fst_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                        uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_fst_row *out, pgt_fst_total *tot) {
    PGT_USE_DEVICE(ctx);
    return pops_reduce_host(ctx, kFstPops, pgt_fst_pops_reduce_dev, pos, freq, nind, n_pops, n, minind, win, n_win, out, tot);
}

/* Hudson's FST of all pairs: the host-buffer form, as pgt_fst_pops_reduce */
int pgt_fst_hudson_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                               uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_fst_row *out, pgt_fst_total *tot) {
    PGT_USE_DEVICE(ctx);
    return pops_reduce_host(ctx, kFstHudsonPops, pgt_fst_hudson_pops_reduce_dev, pos, freq, nind, n_pops, n, minind, win, n_win, out, tot);
}

/* pi per population from (freq, nInd) columns: the host-buffer form, as pgt_dxy_pops_reduce with one table per population */
int pgt_pi_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                       uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_dxy_row *out, pgt_dxy_total *tot) {
    PGT_USE_DEVICE(ctx);
    return pops_reduce_host(ctx, kPiPops, pgt_pi_pops_reduce_dev, pos, freq, nind, n_pops, n, minind, win, n_win, out, tot);
}

/* ABBA-BABA patterns of all ingroup trios: the host-buffer form, as pgt_fst_pops_reduce with one table per trio */
int pgt_dstat_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                          uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_dstat_row *out, pgt_dstat_total *tot) {
    PGT_USE_DEVICE(ctx);
    return pops_reduce_host(ctx, kDstatPops, pgt_dstat_pops_reduce_dev, pos, freq, nind, n_pops, n, minind, win, n_win, out, tot);
}

/* f_d / f_dM of all ingroup trios: the host-buffer form, as pgt_dstat_pops_reduce */
int pgt_fd_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                       uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_fd_row *out, pgt_fd_total *tot) {
    PGT_USE_DEVICE(ctx);
    return pops_reduce_host(ctx, kFdPops, pgt_fd_pops_reduce_dev, pos, freq, nind, n_pops, n, minind, win, n_win, out, tot);
}

/* f3 of all trios: the host-buffer form, as pgt_dstat_pops_reduce */
int pgt_f3_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                       uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_f3_row *out, pgt_f3_total *tot) {
    PGT_USE_DEVICE(ctx);
    return pops_reduce_host(ctx, kF3Pops, pgt_f3_pops_reduce_dev, pos, freq, nind, n_pops, n, minind, win, n_win, out, tot);
}

/* f4 of all quartets: the host-buffer form, as pgt_f3_pops_reduce */
int pgt_f4_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                       uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_f4_row *out, pgt_f4_total *tot) {
    PGT_USE_DEVICE(ctx);
    return pops_reduce_host(ctx, kF4Pops, pgt_f4_pops_reduce_dev, pos, freq, nind, n_pops, n, minind, win, n_win, out, tot);
}

/* the f4-ratio sums of all middle triples: the host-buffer form, as pgt_f4_pops_reduce */
int pgt_f4ratio_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                            uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_f4ratio_row *out, pgt_f4ratio_total *tot) {
    PGT_USE_DEVICE(ctx);
    return pops_reduce_host(ctx, kF4RatioPops, pgt_f4ratio_pops_reduce_dev, pos, freq, nind, n_pops, n, minind, win, n_win, out, tot);
}

/* PBS of all trios: the host-buffer form, as pgt_f3_pops_reduce, one per FST estimator */
int pgt_pbs_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                        uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_pbs_row *out, pgt_pbs_total *tot) {
    PGT_USE_DEVICE(ctx);
    return pops_reduce_host(ctx, kPbsPops, pgt_pbs_pops_reduce_dev, pos, freq, nind, n_pops, n, minind, win, n_win, out, tot);
}

int pgt_pbs_hudson_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                               uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_pbs_row *out, pgt_pbs_total *tot) {
    PGT_USE_DEVICE(ctx);
    return pops_reduce_host(ctx, kPbsPops, pgt_pbs_hudson_pops_reduce_dev, pos, freq, nind, n_pops, n, minind, win, n_win, out, tot);
}

/* block jackknife of a host table of rows: rows up, the device form on the cached workspace, 3 (f4-ratio: 6) n_trios results down */
static int jackknife_host(pgt_ctx *ctx, JackEstimator est, const void *rows, uint64_t n_win, uint32_t n_trios, void *out) {
    const std::string who = jack_who(est);
    if (int rc = jack_check_range(ctx, est, n_trios, n_win)) return rc;
    if ((n_win && !rows) || !out) return ctx_fail(ctx, PGT_EARG, who + "NULL argument");
    const size_t row_bytes = (size_t)n_trios * n_win * jack_row_bytes(est), out_bytes = (size_t)n_trios * jack_items(est) * sizeof(pgt_dstat_jack);
    const size_t work_bytes = jack_work(n_trios, n_win, jack_items(est), jack_sums(est)).bytes;
    void *drows = nullptr, *dwork = nullptr, *dout = nullptr;
    if (int rc = workspace(ctx, HostIo::kRows, row_bytes, &drows)) return rc;
    if (int rc = workspace(ctx, HostIo::kTree, work_bytes, &dwork)) return rc;
    if (int rc = workspace(ctx, HostIo::kTot, out_bytes, &dout)) return rc;
    if (row_bytes)
        if (int rc = hip_check(ctx, hipMemcpy(drows, rows, row_bytes, hipMemcpyHostToDevice), "upload rows")) return rc;
    if (int rc = jackknife_dev(ctx, est, drows, n_win, n_trios, dout, out_bytes, dwork, work_bytes, nullptr)) return rc;
    if (int rc = hip_check(ctx, hipStreamSynchronize(nullptr), "kernels")) return rc;
    return hip_check(ctx, hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost), "download jackknife");
}

int pgt_dstat_jackknife(pgt_ctx *ctx, const pgt_dstat_row *rows, uint64_t n_win, uint32_t n_trios, pgt_dstat_jack *out) {
    PGT_USE_DEVICE(ctx);
    return jackknife_host(ctx, kJackD, rows, n_win, n_trios, out);
}

int pgt_f3_jackknife(pgt_ctx *ctx, const pgt_f3_row *rows, uint64_t n_win, uint32_t n_trios, pgt_f3_jack *out) {
    PGT_USE_DEVICE(ctx);
    return jackknife_host(ctx, kJackF3Mean, rows, n_win, n_trios, out);
}

int pgt_f4_jackknife(pgt_ctx *ctx, const pgt_f4_row *rows, uint64_t n_win, uint32_t n_quartets, pgt_f4_jack *out) {
    PGT_USE_DEVICE(ctx);
    return jackknife_host(ctx, kJackF4Mean, rows, n_win, n_quartets, out);
}

int pgt_f4ratio_jackknife(pgt_ctx *ctx, const pgt_f4ratio_row *rows, uint64_t n_win, uint32_t n_triples, pgt_f4ratio_jack *out) {
    PGT_USE_DEVICE(ctx);
    return jackknife_host(ctx, kJackF4Ratio, rows, n_win, n_triples, out);
}

int pgt_pbs_jackknife(pgt_ctx *ctx, const pgt_pbs_row *rows, uint64_t n_win, uint32_t n_trios, pgt_pbs_jack *out) {
    PGT_USE_DEVICE(ctx);
    return jackknife_host(ctx, kJackPbs, rows, n_win, n_trios, out);
}

/* ---------------- window tables built on the device ---------------- */

struct pgt_wintab {
    int device = 0;
    uint64_t n_win = 0;
    uint32_t W = 0, S = 0;
    std::vector<uint64_t> first;  // n_runs + 1
    pgt_win *d_win = nullptr;
};

int pgt_wintab_sites(pgt_ctx *ctx, const uint64_t *run_len, size_t n_runs, uint32_t W, uint32_t S, pgt_wintab **out) {
    PGT_USE_DEVICE(ctx);
    if (!out) return ctx_fail(ctx, PGT_EARG, "pgt_wintab_sites: NULL argument");
    std::vector<RunPlan> plan;
    uint64_t count = 0;
    if (int rc = plan_site_windows(run_len, n_runs, W, S, plan, &count)) return ctx_fail(ctx, rc, global_error());
    std::unique_ptr<pgt_wintab> tab(new pgt_wintab);
    tab->device = ctx->device;
    tab->n_win = count;
    tab->W = W;
    tab->S = S;
    tab->first.resize(n_runs + 1);
    for (size_t r = 0; r < n_runs; ++r) tab->first[r] = plan[r].out0;
    tab->first[n_runs] = count;
    if (count) {
        DevBuf dplan;
        if (int rc = dplan.alloc(ctx, plan.size() * sizeof(RunPlan), "alloc window plan")) return rc;
        if (int rc = hip_check(ctx, hipMemcpy(dplan.p, plan.data(), plan.size() * sizeof(RunPlan), hipMemcpyHostToDevice), "upload window plan")) return rc;
        void *p = nullptr;
        if (int rc = hip_check(ctx, hipMalloc(&p, count * sizeof(pgt_win)), "alloc window table")) return rc;
        tab->d_win = static_cast<pgt_win *>(p);
        int rc = launch_windows_from_plan(static_cast<const RunPlan *>(dplan.p), n_runs, count, W, S, tab->d_win, nullptr, &ctx->error);
        if (!rc) rc = hip_check(ctx, hipStreamSynchronize(nullptr), "window table kernel");  // dplan is freed on return
        if (rc) {
            (void)hipFree(tab->d_win);
            return rc;
        }
    }
    *out = tab.release();
    return PGT_OK;
}

uint64_t pgt_wintab_size(const pgt_wintab *tab) { return tab ? tab->n_win : 0; }
const uint64_t *pgt_wintab_first(const pgt_wintab *tab) { return tab ? tab->first.data() : nullptr; }
const pgt_win *pgt_wintab_device(const pgt_wintab *tab) { return tab ? tab->d_win : nullptr; }
void pgt_wintab_free(pgt_wintab *tab) {
    if (!tab) return;
    int saved = -1;
    const bool sw = hipGetDevice(&saved) == hipSuccess && saved != tab->device && hipSetDevice(tab->device) == hipSuccess;
    if (tab->d_win) (void)hipFree(tab->d_win);
    if (sw) (void)hipSetDevice(saved);
    delete tab;
}

namespace {
// the hints a table built from (W, S) implies, for the duration of one reduce
struct TabHints {
    pgt_ctx *ctx;
    pgt::Hints saved;
    TabHints(pgt_ctx *c, const pgt_wintab *t) : ctx(c), saved(c->hints) {
        c->hints.max_window = t->W;
        c->hints.typical_window = 0;  // W stands for the typical length
        c->hints.window_step = t->S;
    }
    ~TabHints() { ctx->hints = saved; }
};
int tab_check(pgt_ctx *ctx, const pgt_wintab *tab, const void *out, const char *who) {
    if (!tab || (tab->n_win && !out)) return ctx_fail(ctx, PGT_EARG, std::string(who) + ": NULL argument");
    if (tab->device != ctx->device) return ctx_fail(ctx, PGT_EARG, std::string(who) + ": the window table lives on another device");
    return PGT_OK;
}
}  // namespace

extern "C++" {
namespace {
// the *_tab entry points: table already on the device; rows and tree from the cached workspace
template <class Row, class Run>
int reduce_tab(pgt_ctx *ctx, const char *who, int stat, uint64_t n, const pgt_wintab *tab, Row *out, pgt_dxy_total *tot, ApiTrace &trace, Run run) {
    const TabHints hint(ctx, tab);
    void *dout = nullptr, *dtree = nullptr, *dtot = nullptr;
    const size_t tb = pgt_tree_bytes(stat, n);
    if (int rc = workspace(ctx, HostIo::kRows, tab->n_win * sizeof(Row), &dout)) return rc;
    if (int rc = workspace(ctx, HostIo::kTree, tb, &dtree)) return rc;
    if (tot)
        if (int rc = workspace(ctx, HostIo::kTot, sizeof(pgt_dxy_total), &dtot)) return rc;
    trace.lap("workspace");
    if (int rc = run(static_cast<Row *>(dout), dtree, tb, static_cast<pgt_dxy_total *>(dtot))) return rc;
    if (int rc = hip_check(ctx, hipStreamSynchronize(nullptr), who)) return rc;
    trace.lap("kernels");
    if (tab->n_win)
        if (int rc = hip_check(ctx, hipMemcpy(out, dout, tab->n_win * sizeof(Row), hipMemcpyDeviceToHost), "download rows")) return rc;
    if (tot)
        if (int rc = hip_check(ctx, hipMemcpy(tot, dtot, sizeof(pgt_dxy_total), hipMemcpyDeviceToHost), "download total")) return rc;
    trace.lap("download rows", tab->n_win * sizeof(Row));
    return PGT_OK;
}
}  // namespace
}  // extern "C++"

int pgt_fst_reduce_tab(pgt_ctx *ctx, const uint32_t *pos, const double *a, const double *b, uint64_t n, int cols_on_device,
                       const pgt_wintab *tab, pgt_fst_row *out, size_t out_bytes) {
    PGT_USE_DEVICE(ctx);
    if (int rc = tab_check(ctx, tab, out, "pgt_fst_reduce_tab")) return rc;
    if (int rc = room_check(ctx, "pgt_fst_reduce_tab", tab->n_win, sizeof(pgt_fst_row), out_bytes)) return rc;
    if (n && (!pos || !a || !b)) return ctx_fail(ctx, PGT_EARG, "pgt_fst_reduce_tab: NULL argument");
    if (tab->n_win == 0) return PGT_OK;
    ApiTrace trace("pgt_fst_reduce_tab");
    DevBuf dpos, da, db;
    if (!cols_on_device) {
        UploadJob jobs[] = {{&dpos, pos, n * sizeof(uint32_t), "upload pos"}, {&da, a, n * sizeof(double), "upload a"},
                            {&db, b, n * sizeof(double), "upload b"}};
        if (int rc = upload_columns(ctx, jobs, 3, trace)) return rc;
        pos = static_cast<uint32_t *>(dpos.p); a = static_cast<double *>(da.p); b = static_cast<double *>(db.p);
    }
    return reduce_tab<pgt_fst_row>(ctx, "fst kernels", PGT_STAT_FST, n, tab, out, nullptr, trace,
        [&](pgt_fst_row *dr, void *tree, size_t tb, pgt_dxy_total *) {
            return pgt_fst_reduce_dev(ctx, pos, a, b, n, tab->d_win, tab->n_win, dr, tab->n_win * sizeof(pgt_fst_row), tree, tb, nullptr);
        });
}

int pgt_het_reduce_tab(pgt_ctx *ctx, const uint32_t *pos, const int8_t *g, uint64_t n, int cols_on_device, const pgt_wintab *tab,
                       pgt_het_row *out, size_t out_bytes) {
    PGT_USE_DEVICE(ctx);
    if (int rc = tab_check(ctx, tab, out, "pgt_het_reduce_tab")) return rc;
    if (int rc = room_check(ctx, "pgt_het_reduce_tab", tab->n_win, sizeof(pgt_het_row), out_bytes)) return rc;
    if (n && (!pos || !g)) return ctx_fail(ctx, PGT_EARG, "pgt_het_reduce_tab: NULL argument");
    if (tab->n_win == 0) return PGT_OK;
    ApiTrace trace("pgt_het_reduce_tab");
    DevBuf dpos, dg;
    if (!cols_on_device) {
        UploadJob jobs[] = {{&dpos, pos, n * sizeof(uint32_t), "upload pos"}, {&dg, g, n * sizeof(int8_t), "upload genotypes"}};
        if (int rc = upload_columns(ctx, jobs, 2, trace)) return rc;
        pos = static_cast<uint32_t *>(dpos.p); g = static_cast<int8_t *>(dg.p);
    }
    return reduce_tab<pgt_het_row>(ctx, "het kernels", PGT_STAT_HET, n, tab, out, nullptr, trace,
        [&](pgt_het_row *dr, void *tree, size_t tb, pgt_dxy_total *) {
            return pgt_het_reduce_dev(ctx, pos, g, n, tab->d_win, tab->n_win, dr, tab->n_win * sizeof(pgt_het_row), tree, tb, nullptr);
        });
}

int pgt_dxy_reduce_tab(pgt_ctx *ctx, const uint32_t *pos, const double *p1, const double *p2, const int32_t *n1, const int32_t *n2,
                       uint64_t n, int minind, int cols_on_device, const pgt_wintab *tab, pgt_dxy_row *out, size_t out_bytes,
                       pgt_dxy_total *tot) {
    PGT_USE_DEVICE(ctx);
    if (int rc = tab_check(ctx, tab, out, "pgt_dxy_reduce_tab")) return rc;
    if (int rc = room_check(ctx, "pgt_dxy_reduce_tab", tab->n_win, sizeof(pgt_dxy_row), out_bytes)) return rc;
    if (n && (!pos || !p1 || !p2 || !n1 || !n2)) return ctx_fail(ctx, PGT_EARG, "pgt_dxy_reduce_tab: NULL argument");
    ApiTrace trace("pgt_dxy_reduce_tab");
    DevBuf dpos, d1, d2, dn1, dn2;
    if (!cols_on_device) {
        UploadJob jobs[] = {{&dpos, pos, n * sizeof(uint32_t), "upload pos"}, {&d1, p1, n * sizeof(double), "upload p1"},
                            {&d2, p2, n * sizeof(double), "upload p2"}, {&dn1, n1, n * sizeof(int32_t), "upload n1"},
                            {&dn2, n2, n * sizeof(int32_t), "upload n2"}};
        if (int rc = upload_columns(ctx, jobs, 5, trace)) return rc;
        pos = static_cast<uint32_t *>(dpos.p); p1 = static_cast<double *>(d1.p); p2 = static_cast<double *>(d2.p);
        n1 = static_cast<int32_t *>(dn1.p); n2 = static_cast<int32_t *>(dn2.p);
    }
    return reduce_tab<pgt_dxy_row>(ctx, "dxy kernels", PGT_STAT_DXY, n, tab, out, tot, trace,
        [&](pgt_dxy_row *dr, void *tree, size_t tb, pgt_dxy_total *dtot) {
            return pgt_dxy_reduce_dev(ctx, pos, p1, p2, n1, n2, n, minind, tab->d_win, tab->n_win, dr, tab->n_win * sizeof(pgt_dxy_row), dtot, tree,
                                      tb, nullptr);
        });
}

/* copy of a device column of an ingest object to the host (dxyWindow's site synchronisation and bp-window
 * table work on host positions) */
int pgt_ingest_download(pgt_ctx *ctx, const pgt_ingest *ing, int token, void *host_dst, size_t bytes) {
    PGT_USE_DEVICE(ctx);
    void *src = pgt_ingest_column(ing, token);
    if (bytes == 0) return PGT_OK;
    if (!src || !host_dst) return ctx_fail(ctx, PGT_EARG, "pgt_ingest_download: no such column");
    if (bytes > ingest_column_bytes(ing, token)) return ctx_fail(ctx, PGT_EARG, "pgt_ingest_download: more bytes than the column holds");
    return hip_check(ctx, hipMemcpy(host_dst, src, bytes, hipMemcpyDeviceToHost), "pgt_ingest_download");
}

}  // extern "C"
