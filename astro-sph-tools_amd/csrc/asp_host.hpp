// asp_host.hpp -- host runtime shared by every unit: errors, environment knobs, the
// per-device workspace cache (HBM buffers reused across calls), HIP-event stage timing.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/asp.h"

namespace asp {

inline thread_local std::string t_err;

inline int fail(int code, const std::string& msg) {
    t_err = msg;
    return code;
}

#define ASP_HIP(expr)                                                                    \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return fail(ASP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define ASP_TRY(expr)                  \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != ASP_OK) return rc_; \
    } while (0)

// Environment knobs (tuning, A/B switches, test hooks): every read goes through these two.
// env_int: the variable's integer value clamped to [lo, hi], or def when it is not set.
// Knobs are read on every call (tests change them mid-process) unless the caller keeps
// the value in a function static.
inline long long env_int(const char* name, long long def, long long lo = INT_MIN,
                         long long hi = INT_MAX) {
    const char* e = getenv(name);
    return e ? std::max(lo, std::min(hi, atoll(e))) : def;
}
inline bool env_set(const char* name) { return getenv(name) != nullptr; }

// Runtime (kernel id, map count, deterministic) -> compile-time constants: calls
// f(Int<KID>, Int<NOUT>, Int<ACC>) with ACC = 0 (fp64 sums) / 1 (fixed point), the values of
// kAccF64 / kAccFix.  f is a generic lambda; only the combinations named here instantiate.
// Used by the 2-D map's launchers (asp_map_bin.hip, asp_map_deposit.hip).
template <int V>
using Int = std::integral_constant<int, V>;
template <class F>
inline int dispatch_kid(int kid, F&& f) {
    return kid == 0 ? f(Int<0>{}) : kid == 1 ? f(Int<1>{}) : kid == 2 ? f(Int<2>{})
         : kid == 3 ? f(Int<3>{}) : f(Int<4>{});
}
template <class F>
inline int dispatch(int kid, int nout, bool det, F&& f) {
    return dispatch_kid(kid, [&](auto K) {
        if (nout == 1) return det ? f(K, Int<1>{}, Int<1>{}) : f(K, Int<1>{}, Int<0>{});
        return det ? f(K, Int<2>{}, Int<1>{}) : f(K, Int<2>{}, Int<0>{});
    });
}

struct Buf {
    void* p = nullptr;
    size_t cap = 0;
};

constexpr int kStages = 24;
constexpr int kNStats = 16;  // asp_last_stats
constexpr int kMarks = 8;  // launches of one stage timed per call
enum Stage {
    kSMemset = 0, kSCount, kSColscan, kSTilescan, kSScatter, kSScale, kSDeposit, kSMerge,
    kSWide, kSRatio,
    // 3-D cube (asp_project3d)
    kS3Count = 10, kS3Colscan, kS3Tilescan, kS3Scatter, kS3Deposit, kS3Merge,
    kSGather = 16,  // 2-D gathered deposit of the large-record stream
    kSKnnPrep = 17, kSKnnSearch = 18,  // k-NN: keys / sort / tables; the search kernel
    // asp_nearest: centre check / cell sort; the search (with the query sort, when on)
    kSNearestPrep = 19, kSNearestSearch = 20,
    // asp_sample2d: point keys / sort / cell offsets; the particle -> point deposit
    kSSamplePrep = 21, kSSampleDeposit = 22,
    // asp_spectra2d: the (pair, velocity bin) deposit and its finalising pass (its prep: 21)
    kSSpectraDeposit = 23
};

// What the slots of the workspace's buffer arrays hold (Workspace::knn, nearest, match,
// sample, profiles, aux, pairs).
// asp_knn_smoothing_lengths
enum KnnBuf {
    kKnnPos, kKnnH,            // staged positions and smoothing lengths (host callers)
    kKnnPartials,              // bounding-box reduction partials
    kKnnKeys, kKnnIndex,       // sort keys and indices, in / out
    kKnnSorted,                // positions in key order (SoA)
    kKnnSortTmp,               // radix sort scratch
    kKnnCells,                 // the level-L cell table
    kKnnSubCells, kKnnSubTable,  // its sub-tables
    kKnnBlockMin,              // the suffix-minimum block minima of the table's scan
    kKnnCounters,              // the ASP_KNN_COUNT distance counters
    kKnnBufCount
};
// asp_nearest
enum NearestBuf {
    kNearCentres, kNearMembers,  // staged centres and member words
    kNearCheck,                  // check counters
    kNearCellCount,              // cell counts, then cursors
    kNearCellStart,
    kNearEntries,
    kNearScanTmp,                // scan scratch
    kNearCounter,                // the ASP_NEAREST_COUNT counter
    kNearQueries, kNearOutputs,  // staged queries and outputs
    kNearSortKeys, kNearSortIndex, kNearSortTmp,  // the query sort
    kNearestBufCount
};
// asp_match_ids / asp_take_rows
enum MatchBuf {
    kMatchIds, kMatchFilters, kMatchOutputs,  // staged IDs, filters, outputs
    kMatchPartCount,                          // partition counts, then cursors
    kMatchPartStart,
    kMatchKeys, kMatchPositions,              // record keys and positions
    kMatchCounters,           // asp_match_ids' counters; asp_take_rows' bad-index flag
    kMatchScanTmp,            // scan scratch
    kMatchRows, kMatchRowsOut, kMatchRowIndex,  // asp_take_rows: staged rows, output, index
    kMatchBufCount
};
// asp_sample2d / asp_sample3d and their _f64 forms (sample_driver, asp_sample.hpp)
enum SampleBuf {
    kSmpPart0, kSmpPart1, kSmpPart2, kSmpPart3, kSmpPart4,  // staged particle arrays (host callers)
    kSmpPx, kSmpPy,            // staged point coordinates (the third: kSmpPz)
    kSmpOut0, kSmpOut1,        // staged outputs
    kSmpDesc,                  // the point grid's descriptor (bounding box, scales, counters)
    kSmpKeys, kSmpIndex,       // cell keys and point indices, in / out
    kSmpSortTmp,               // radix sort scratch
    kSmpCellCount, kSmpCellStart,  // points per cell and their exclusive scan
    kSmpScanTmp,               // scan scratch
    kSmpSorted,                // point coordinates in cell order (x, then y, then z in 3-D)
    kSmpAcc,                   // per-point accumulators (fp64 or int64), in cell order
    kSmpPz,                    // staged third point coordinate (3-D)
    kSmpVc, kSmpB,             // asp_spectra2d: staged velocity coordinates and Doppler parameters
    kSampleBufCount
};
// asp_halo_profiles
enum ProfilesBuf {
    kProfPos, kProfProps,          // staged particle batch (host callers)
    kProfCentres, kProfRadius,     // staged centres and radii
    kProfEdges,                    // staged bin edges
    kProfCount, kProfSum,          // staged outputs
    kProfCheck,                    // centre / radius check word
    kProfKeys, kProfIndex,         // cell keys and particle indices, in / out
    kProfSortTmp,                  // radix sort scratch
    kProfCellStart,                // first particle of every cell
    kProfSorted,                   // wrapped coordinates, then the properties, in cell order (SoA)
    kProfCand, kProfItems,         // candidates per halo; items per halo, then their exclusive scan
    kProfScanTmp,                  // scan scratch
    kProfCounters,                 // pairs tested (ASP_PROFILE_COUNT)
    kProfilesBufCount
};
// Per-call scratch that several entry points reuse, each with its own meaning for slots
// 0 .. 4 (a local enum at the top of the user); the last holds a call's few 64-bit
// counter words (asp_stage_particles' image counts, the ASP_COUNT_EVALS sums).
enum AuxBuf { kAuxCounters = 5, kAuxBufCount };
// the kernel_func plug-in session: per-pixel pair counts, per-tile pair totals
enum PairsBuf { kPairsPixCount, kPairsTileTotals, kPairsBufCount };

// Every device buffer of a workspace, and nothing else: free_buffers walks the struct as
// an array of Buf, so a buffer added here is released with the rest.
struct WorkspaceBufs {
    Buf knn[kKnnBufCount];
    Buf nearest[kNearestBufCount];
    Buf match[kMatchBufCount];
    Buf sample[kSampleBufCount];
    Buf profiles[kProfilesBufCount];
    Buf aux[kAuxBufCount];
    Buf in[5], out[2], hist, cmx, tile_total, tile_start, tile_k, items, merges, counters, recs,
        wide, slabs, morton, iorder;
    Buf morton3;     // brick order of the 3-D cube
    Buf in64[4];     // asp_project2d_f64: the caller's fp64 arrays, resident for exact decisions
    Buf ext;         // asp_project2d_props: per record, the coefficients of properties 2..5
    Buf inx[4];      // asp_project2d_props_f64: fp32 working copies of properties 2..5
    Buf pairs[kPairsBufCount];  // the kernel_func plug-in session
    Buf inw[2];      // asp_project2d_sph(_f64) from host arrays: the masses and densities
    Buf wts[6];      // asp_project2d_sph(_f64): fp32 working copies of m / rho * property
};
static_assert(std::is_standard_layout<WorkspaceBufs>::value, "viewed as an array of Buf");
static_assert(sizeof(WorkspaceBufs) % sizeof(Buf) == 0, "Buf members only");

inline void free_buffers(WorkspaceBufs& bufs) {
    Buf* b = reinterpret_cast<Buf*>(&bufs);
    for (size_t k = 0; k < sizeof(WorkspaceBufs) / sizeof(Buf); ++k) {
        if (b[k].p) (void)hipFree(b[k].p);
        b[k] = Buf{};
    }
}

// The 2-D map's layout tag ("Layout reuse"): after a counted pass of
// project2d_device the prefix rows (hist), tile totals and starts, work items, dispatch
// order, merge list and device counters in the workspace are a function of the particle
// positions, h and the grid alone, so the next pass over the same particle set may skip
// its count and scans.  The tag says that those buffers are intact (valid) and what they
// were made for (key: compared word for word, zero-filled first); the pass that reuses
// them proves on the device that they are exact for ITS particles (k_scatter, verify), so
// the key decides only whether the attempt is worth making.
struct LayoutKey {
    long long n, nblk, stride;             // particles, count workgroups, Src64::stride
    double x_min, y_min, psx, psy_pix, psy_cull;  // the window grid (Grid)
    int nx, ny, cs, gnx, ox, ntiles, nty, nonsquare, mixed;
    int grp, item_target, item_identity;   // scatter group, deposit items and their order
    int wide_tiles, gather_min, gather_area;
    const void* src[5];                    // Src64's fp64 arrays (null: an fp32 caller)
    const void* pos[3];                    // the pass's u, v, h
    const void* buf[7];                    // hist, tile_total, tile_start, items, iorder,
    size_t cap[7];                         // merges, counters: where they are, and their
                                           // sizes (a re-allocation always grows them)
};
constexpr int kLayoutCounters = 7;  // n_recs, n_items, n_merges, n_slabs, n_wide, n_large, chunk
struct Layout {
    bool valid = false;
    LayoutKey key;
    long long ctr[kLayoutCounters] = {0};  // the counted pass's host counters
    // Arming (a wasted attempt must be rare): a counted pass arms reuse, a failed attempt
    // disarms it, and while disarmed a counted pass re-arms it only when its counters
    // (the last, the records per item, follows from the others) equal the previous
    // counted pass's -- a caller that rewrites its positions in place pays one wasted scatter.
    bool armed = true;
    bool have_last = false;
    long long last[kLayoutCounters] = {0};
};

struct Workspace : WorkspaceBufs {
    std::mutex mu;
    Layout layout;
    // HIP-event profiling (asp_profile): per-stage start/stop events of the last call,
    // folded into the running sums at the next call or at asp_profile_read.
    bool prof = false;
    unsigned prof_mask = 0u;  // stages timed (bit k = stage k)
    // Two event sets, used by alternate calls: a call folds the set of the call two back,
    // which has completed by then (the previous call's counter read-back waited for it),
    // so profiling never makes the host wait for the GPU to drain between calls.
    hipEvent_t ev[2][kStages][kMarks][2] = {};
    int ev_live[2][kStages] = {};  // marks recorded per set (a stage may launch once per
                                   // particle chunk)
    int pset = 0;                  // the set the current call records into
    double stage_ms[kStages] = {};
    long long stage_n[kStages] = {};
    int* h_counters = nullptr;  // pinned
    int morton_ntx = -1, morton_nty = -1;
    int morton3_key[3] = {-1, -1, -1};
    long long stats[kNStats] = {0};
    // Side stream of the chunked host staging (asp_stage_particles).
    hipStream_t side = nullptr;
    hipEvent_t chunk_ev[kMarks] = {};
    hipEvent_t done_ev = nullptr;
    hipEvent_t scan_ev = nullptr;  // 2-D pipeline: binning scans done (st)
    hipEvent_t cnt_ev = nullptr;   // ... and their counters copied to the host (side)
    // End of the last call's GPU work on the workspace: the next call's stream waits for
    // it, so calls on different streams never overwrite buffers still being read.
    hipEvent_t last_ev = nullptr;
    // Host -> device copies of pageable caller arrays go through two pinned bounce
    // buffers (h2d_staged): the CPU copy of one piece overlaps the DMA of the previous.
    void* pin[2] = {nullptr, nullptr};
    hipEvent_t pin_ev[2] = {};
    bool pin_busy[2] = {false, false};
    int pin_next = 0;
};

inline int ensure_side(Workspace& ws) {
    if (ws.side) return ASP_OK;
    ASP_HIP(hipStreamCreateWithFlags(&ws.side, hipStreamNonBlocking));
    for (int c = 0; c < kMarks; ++c)
        ASP_HIP(hipEventCreateWithFlags(&ws.chunk_ev[c], hipEventDisableTiming));
    ASP_HIP(hipEventCreateWithFlags(&ws.done_ev, hipEventDisableTiming));
    ASP_HIP(hipEventCreateWithFlags(&ws.scan_ev, hipEventDisableTiming));
    ASP_HIP(hipEventCreateWithFlags(&ws.cnt_ev, hipEventDisableTiming));
    return ASP_OK;
}

// Everything a private workspace (a plug-in session's) owns: device buffers, the pinned
// counters and bounce buffers, the side stream and its events.  The shared per-device
// workspaces (g_ws) live for the process; asp_release frees only their buffers.
void release_pinned(Workspace& ws);
inline void ws_teardown(Workspace& ws) {
    free_buffers(ws);
    if (ws.h_counters) (void)hipHostFree(ws.h_counters);
    ws.h_counters = nullptr;
    release_pinned(ws);
    for (hipEvent_t& e : ws.chunk_ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    for (hipEvent_t* e : {&ws.done_ev, &ws.scan_ev, &ws.cnt_ev, &ws.last_ev}) {
        if (*e) (void)hipEventDestroy(*e);
        *e = nullptr;
    }
    if (ws.side) (void)hipStreamDestroy(ws.side);
    ws.side = nullptr;
    for (auto& q : ws.ev)
        for (auto& k : q)
            for (auto& j : k)
                for (hipEvent_t& e : j) {
                    if (e) (void)hipEventDestroy(e);
                    e = nullptr;
                }
}

constexpr int kMaxDevices = 64;  // devices the per-device tables below have room for
inline Workspace g_ws[kMaxDevices];

// 2-D maps from DIFFERENT streams get different workspaces (slots), so consecutive
// independent maps enqueued on two streams overlap on the device (the binning of map
// i + 1 beside the deposit of map i).  Slot 0 is g_ws (shared with every
// other entry point); a map call on a stream that already owns a slot reuses it, a new
// stream takes the least recently used slot.  Within a slot calls stay ordered (ws_begin
// waits for the slot's previous call); across slots the caller's streams order the work,
// as for any two HIP streams.  ASP_MAP_SLOTS=1: one slot (every call ordered).
#ifndef ASP_MAP_SLOTS_MAX  // (an A/B build switch: 3 slots measured in round 5)
#define ASP_MAP_SLOTS_MAX 2
#endif
constexpr int kMapSlots = ASP_MAP_SLOTS_MAX;
inline Workspace g_ws_alt[kMaxDevices][kMapSlots - 1];
struct SlotTable {
    std::mutex mu;
    hipStream_t stream[kMapSlots] = {};
    bool used[kMapSlots] = {};
    int last = kMapSlots - 1;
};
inline SlotTable g_slots[kMaxDevices];
inline Workspace& slot_ws(int device, int s) { return s == 0 ? g_ws[device] : g_ws_alt[device][s - 1]; }
inline int map_slot(int device, hipStream_t st) {
    static const int nslots = (int)env_int("ASP_MAP_SLOTS", kMapSlots, 1, kMapSlots);
    SlotTable& T = g_slots[device];
    std::lock_guard<std::mutex> lock(T.mu);
    int s = -1;
    for (int k = 0; k < nslots && s < 0; ++k)
        if (T.used[k] && T.stream[k] == st) s = k;
    for (int k = 0; k < nslots && s < 0; ++k)
        if (!T.used[k]) s = k;
    if (s < 0) s = (T.last + 1) % nslots;  // the least recently used of two
    T.used[s] = true;
    T.stream[s] = st;
    T.last = s;
    return s;
}

// Scatter gate (ASP_SCATTER_GATE=1, read per call): with maps on two streams (two slots),
// a map's count and scans may run beside the previous map's deposit, but its scatter
// waits for that deposit -- the scatter and the deposit both stream GBs through the memory
// system and slowed each other when fully overlapped.  The event of
// the most recent map's deposit end, per device, with the stream that recorded it.
struct DepositGate {
    std::mutex mu;
    hipEvent_t ev = nullptr;
    hipStream_t st = nullptr;
};
inline DepositGate g_gate[kMaxDevices];
inline bool scatter_gate_on() { return env_int("ASP_SCATTER_GATE", 0) != 0; }
inline int gate_wait(int device, hipStream_t st) {  // before a map's scatter
    DepositGate& G = g_gate[device];
    std::lock_guard<std::mutex> lock(G.mu);
    if (G.ev && G.st != st) ASP_HIP(hipStreamWaitEvent(st, G.ev, 0));
    return ASP_OK;
}
inline int gate_record(int device, hipStream_t st) {  // after a map's deposit
    DepositGate& G = g_gate[device];
    std::lock_guard<std::mutex> lock(G.mu);
    if (!G.ev) ASP_HIP(hipEventCreateWithFlags(&G.ev, hipEventDisableTiming));
    ASP_HIP(hipEventRecord(G.ev, st));
    G.st = st;
    return ASP_OK;
}

inline int set_device(int device) {
    int ndev = 0;
    ASP_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= std::min(ndev, kMaxDevices))
        return fail(ASP_ERR_INVALID, "bad device");
    ASP_HIP(hipSetDevice(device));
    return ASP_OK;
}

// Cross-call ordering of the shared workspace (the caller holds ws.mu): a call's stream
// first waits for the end of the previous call's work, and records the new end.
inline int ws_begin(Workspace& ws, hipStream_t st) {
    if (ws.last_ev) ASP_HIP(hipStreamWaitEvent(st, ws.last_ev, 0));
    return ASP_OK;
}
inline int ws_end(Workspace& ws, hipStream_t st) {
    if (!ws.last_ev) ASP_HIP(hipEventCreateWithFlags(&ws.last_ev, hipEventDisableTiming));
    ASP_HIP(hipEventRecord(ws.last_ev, st));
    return ASP_OK;
}
// Created right after ws_begin: every exit of the call -- error returns included, which
// may already have enqueued work on st -- records the end event, so the next call on
// another stream waits for that work.  finish() is the success path's (checked) record.
struct WsEnd {
    Workspace& ws;
    hipStream_t st;
    bool done = false;
    WsEnd(Workspace& w, hipStream_t s) : ws(w), st(s) {}
    int finish() {
        done = true;
        return ws_end(ws, st);
    }
    ~WsEnd() {
        if (!done) (void)ws_end(ws, st);
    }
};

// asp_stage.hip: reader arrays on the device -> the projector's fp32 working copies
// (axis selection of _projector.py:38-46, round to nearest), enqueued on st.
// Pageable host -> device copy through the workspace's pinned bounce buffers, ordered on
// st (asp_stage.hip).  Returns once every piece's DMA is enqueued; the host source may be
// reused then (its bytes are in the bounce buffers or already on the device).
int h2d_staged(Workspace& ws, void* dst, const void* src, size_t bytes, hipStream_t st);
void release_pinned(Workspace& ws);
int stage_device(const double* pos, const double* h, const double* a0, const double* a1,
                 long long n, int axis, float* u, float* v, float* hf, float* a0f, float* a1f,
                 hipStream_t st);

inline int prof_fold_set(Workspace& ws, int set) {
    for (int k = 0; k < kStages; ++k) {
        for (int j = 0; j < ws.ev_live[set][k]; ++j) {
            ASP_HIP(hipEventSynchronize(ws.ev[set][k][j][1]));
            float ms = 0.0f;
            ASP_HIP(hipEventElapsedTime(&ms, ws.ev[set][k][j][0], ws.ev[set][k][j][1]));
            ws.stage_ms[k] += ms;
            ws.stage_n[k] += 1;
        }
        ws.ev_live[set][k] = 0;
    }
    return ASP_OK;
}

// At the start of a call: switch sets, folding what the call two back recorded there.
inline int prof_next(Workspace& ws) {
    ws.pset ^= 1;
    return prof_fold_set(ws, ws.pset);
}

// Everything recorded so far (asp_profile_read).
inline int prof_fold(Workspace& ws) {
    int rc = prof_fold_set(ws, ws.pset ^ 1);
    return rc != ASP_OK ? rc : prof_fold_set(ws, ws.pset);
}

struct StageMark {
    Workspace& ws;
    int k;
    hipStream_t st;
    bool on;
    StageMark(Workspace& w, int stage, hipStream_t s)
        : ws(w), k(stage), st(s),
          on(w.prof && ((w.prof_mask >> stage) & 1u) && w.ev_live[w.pset][stage] < kMarks) {
        if (on) (void)hipEventRecord(ws.ev[ws.pset][k][ws.ev_live[ws.pset][k]][0], st);
    }
    void done() {
        if (on) {
            (void)hipEventRecord(ws.ev[ws.pset][k][ws.ev_live[ws.pset][k]][1], st);
            ws.ev_live[ws.pset][k] += 1;
        }
    }
};

inline int ensure(Buf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return ASP_OK;
    if (b.p) {
        (void)hipFree(b.p);
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes + bytes / 4;  // grow with slack: fewer re-allocations across calls
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        want = bytes;
        e = hipMalloc(&b.p, want);
    }
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(ASP_ERR_NOMEM, "hipMalloc(" + std::to_string(bytes) + ") failed: " +
                                       hipGetErrorString(e));
    }
    b.cap = want;
    if (env_set("ASP_PRINT_ALLOC")) fprintf(stderr, "asp alloc %zu B at %p\n", want, b.p);
    return ASP_OK;
}

// The prologue and epilogue of every entry point that works in a shared workspace: the
// device, the workspace under its lock -- the slot of the call's stream (map_slot: the 2-D
// map and the cube) or the device's first -- ordered behind the workspace's previous call;
// body(ws, st) is the call.  Every exit of the body records the end event (WsEnd).
template <class F>
inline int with_workspace(int device, hipStream_t st, bool per_stream_slot, F&& body) {
    ASP_TRY(set_device(device));
    Workspace& ws = per_stream_slot ? slot_ws(device, map_slot(device, st)) : g_ws[device];
    std::lock_guard<std::mutex> lock(ws.mu);
    ASP_TRY(ws_begin(ws, st));
    WsEnd end(ws, st);
    ASP_TRY(body(ws, st));
    return end.finish();
}

// Host-array callers: arrays staged into workspace slots, results copied back.
// How a host array reaches the device.  The two run at different speeds, so an entry
// point keeps the one it was measured with.
enum class Copy {
    kPlain,   // hipMemcpyAsync from the caller's (pageable) array
    kPinned   // h2d_staged: through the workspace's pinned bounce buffers
};
// Slot b holds `bytes` bytes at byte offset off; p points there.  (Arrays that share a slot:
// the first one staged gives the whole size -- ensure() never shrinks, so the later ones
// leave the slot in place.)
template <class T>
inline int device_scratch(Buf& b, T*& p, size_t bytes, size_t off = 0) {
    ASP_TRY(ensure(b, off + bytes));
    p = (T*)((char*)b.p + off);
    return ASP_OK;
}
// ... and the host array p copied there on st; p is redirected to the copy.
template <class T>
inline int to_device(Workspace& ws, Buf& b, const T*& p, size_t bytes, hipStream_t st, Copy kind,
                     size_t off = 0) {
    const T* d = nullptr;
    ASP_TRY(device_scratch(b, d, bytes, off));
    if (bytes > 0 && kind == Copy::kPinned) ASP_TRY(h2d_staged(ws, (void*)d, p, bytes, st));
    if (bytes > 0 && kind == Copy::kPlain)
        ASP_HIP(hipMemcpyAsync((void*)d, p, bytes, hipMemcpyHostToDevice, st));
    p = d;
    return ASP_OK;
}
inline int to_host(void* dst, const void* src, size_t bytes, hipStream_t st) {
    ASP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    return ASP_OK;
}

// A one-word diagnostic counter behind an environment switch (ASP_NEAREST_COUNT,
// ASP_PROFILE_COUNT).  begin(): p is the zeroed word in slot b when the variable is set,
// null otherwise, and kernels add to a non-null p (an atomic per lane, so off in timed
// runs); end(): the total goes to asp_last_stats[9].
struct DiagCounter {
    unsigned long long* p = nullptr;
    int begin(const char* env, Buf& b, hipStream_t st) {
        if (!env_set(env)) return ASP_OK;
        ASP_TRY(ensure(b, sizeof(*p)));
        p = (unsigned long long*)b.p;
        ASP_HIP(hipMemsetAsync(p, 0, sizeof(*p), st));
        return ASP_OK;
    }
    int end(Workspace& ws, hipStream_t st) {
        if (!p) return ASP_OK;
        unsigned long long h = 0;
        ASP_HIP(hipMemcpyAsync(&h, p, sizeof(h), hipMemcpyDeviceToHost, st));
        ASP_HIP(hipStreamSynchronize(st));
        ws.stats[9] = (long long)h;
        return ASP_OK;
    }
};

// Dynamic LDS above the 64 KiB default: the kernel's attribute is raised once per (kernel,
// device) to at least `bytes`, under a lock -- calls may run on several threads (one per
// map slot or stream) and several devices in one process.
inline int allow_dyn_lds(const void* kern, size_t bytes) {
    if (bytes <= 65536) return ASP_OK;
    int dev = 0;
    ASP_HIP(hipGetDevice(&dev));
    struct Set {
        const void* kern;
        int dev;
        size_t bytes;
    };
    static std::mutex mu;
    static std::vector<Set> done;
    std::lock_guard<std::mutex> lk(mu);
    for (Set& d : done)
        if (d.kern == kern && d.dev == dev) {
            if (d.bytes >= bytes) return ASP_OK;
            ASP_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
            d.bytes = bytes;
            return ASP_OK;
        }
    ASP_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done.push_back({kern, dev, bytes});
    return ASP_OK;
}

// Record-buffer placement trials.  The scatter's time depends on where the record buffer
// lands in physical memory: the same call runs 1.88 or 2.38 ms at 10^8 depending on the
// allocation (tools/alloc_probe.py: both modes within one process as the
// buffer is re-allocated), while count, scans and deposit do not move.  When the buffer
// is freshly allocated for a large call, the call's own scatter (`scatter()`: it must also reset any counter it advances) is run into up to
// ASP_PLACEMENT_TRIALS candidate buffers (default 16; each allocated while the best so far
// is still held, so it lands elsewhere), timed with events, and the fastest is kept -- it
// then holds this call's records (the scatter's output does not depend on the buffer).
// Used by the 2-D and the 3-D scatter (ws.recs).
// A one-time cost on the first large call (~3 ms per trial at 10^8); 0 or 1 disables it.
template <class F>
inline int place_records(Workspace& ws, size_t bytes, hipStream_t st, F&& scatter, bool& placed,
                         int* ntrials = nullptr) {
    placed = false;
    if (ntrials) *ntrials = 0;
    const int trials = (int)env_int("ASP_PLACEMENT_TRIALS", 16, 0);
    const size_t min_mb = (size_t)env_int("ASP_PLACEMENT_MIN_MB", 256);  // tests lower it
    if (trials < 2 || bytes < (min_mb << 20)) return ASP_OK;
    hipEvent_t t0, t1;
    ASP_HIP(hipEventCreate(&t0));
    ASP_HIP(hipEventCreate(&t1));
    auto timed = [&](float& ms) -> int {
        ASP_HIP(hipEventRecord(t0, st));
        ASP_TRY(scatter());
        ASP_HIP(hipEventRecord(t1, st));
        ASP_HIP(hipEventSynchronize(t1));
        ASP_HIP(hipEventElapsedTime(&ms, t0, t1));
        return ASP_OK;
    };
    float best_ms = 0.0f;
    int rc = timed(best_ms);  // the buffer ensure() just allocated
    int runs = 1;
    float worst_ms = best_ms;
    // Stop once the best placement is 18 % under the slowest seen: the fast mode (1.8 ms at
    // 10^8) is ~20-25 % under the slow one (2.3-2.4 ms).  Round 2 stopped at 15 % under the
    // FIRST trial, which accepted the intermediate mode (2.1 ms) whenever the first was
    // slow (round 3); a first trial in the fast mode now searches all trials
    // (a few ms each, once per process) without finding better.
    for (int t = 1; t < trials && rc == ASP_OK && best_ms > 0.82f * worst_ms; ++t) {
        Buf best = ws.recs, cand;  // cand is allocated while best is held: other pages
        if (ensure(cand, bytes) != ASP_OK) {
            (void)hipGetLastError();
            break;  // no room for a candidate: keep the best
        }
        ws.recs = cand;
        float ms = 0.0f;
        rc = timed(ms);
        ++runs;
        worst_ms = std::max(worst_ms, ms);
        if (rc == ASP_OK && ms < 0.97f * best_ms) {
            (void)hipFree(best.p);  // the candidate wins and holds this call's records
            best_ms = ms;
        } else {
            (void)hipFree(cand.p);  // the best still holds this call's records from its run
            ws.recs = best;
        }
        if (env_set("ASP_PRINT_ALLOC"))
            fprintf(stderr, "asp placement trial %d: %.3f ms (best %.3f)\n", t, ms, best_ms);
    }
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    if (ntrials) *ntrials = runs;
    placed = rc == ASP_OK;
    return rc;
}

// ----------------------------------------------------------------------------------
// Pieces of the count -> scans -> counter read-back -> scatter sequence that the 2-D map
// (project2d_device) and the cube (cube_pass) share; each pipeline calls them in order.
// ----------------------------------------------------------------------------------
constexpr int kRetSplit = 1;  // internal: >= 2^31 records in one pass; the caller splits
// The capacity a scatter launched AFTER the read-back is given: no pass that gets that far
// has more records (record_limit), so it never declines.
constexpr long long kNoRecordCap = 0x7fffffffLL;

// The device counters, zeroed on st, and their pinned host mirror.
inline int counters_begin(Workspace& ws, int ncounters, hipStream_t st) {
    ASP_TRY(ensure(ws.counters, (size_t)ncounters * sizeof(int)));
    if (!ws.h_counters)
        ASP_HIP(hipHostMalloc((void**)&ws.h_counters, kMarks * ncounters * sizeof(int)));
    ASP_HIP(hipMemsetAsync(ws.counters.p, 0, (size_t)ncounters * sizeof(int), st));
    return ASP_OK;
}

// Records are 32 B (two float4); record cursors are 32-bit (ASP_MAX_RECORDS: tests).
inline size_t record_bytes(long long n_recs) { return (size_t)n_recs * 32; }
inline long long record_limit() { return env_int("ASP_MAX_RECORDS", 0x7fffffffLL, 1, LLONG_MAX); }
// Records the buffer left by an earlier call holds: what a speculative scatter, enqueued
// before the host has the counters, checks them against.  < 2^31 - 1: the tilescan's
// clamped record count always exceeds it when it overflows.
inline long long record_capacity(const Workspace& ws) {
    return (long long)std::min<size_t>(ws.recs.cap / 32, 0x7ffffffe);
}
inline bool speculate_on() { return !env_set("ASP_NO_SPECULATE"); }

// With the counters on the host: kRetSplit when the pass makes too many records (nothing
// is kept), else pre = the speculative scatter did the work.  One that did not (it
// returned at once, or its records are discarded) is waited for, so that the buffers it
// was given can be re-allocated.
inline int settle_speculation(bool spec, long long n_recs, bool fits, hipStream_t st, bool& pre) {
    const bool split = n_recs >= record_limit();
    pre = spec && fits && !split;
    if (spec && !pre) ASP_HIP(hipStreamSynchronize(st));
    return split ? kRetSplit : ASP_OK;
}

// The record buffer grown to n_recs records; fresh: it was re-allocated, so its placement
// is worth trials (place_records).
inline int ensure_records(Workspace& ws, long long n_recs, bool& fresh) {
    const void* before = ws.recs.p;
    ASP_TRY(ensure(ws.recs, record_bytes(n_recs)));
    fresh = ws.recs.p != before;
    return ASP_OK;
}

// Particles per pipeline pass: particle indices and record cursors are 32-bit, so larger
// calls run as batches accumulating into the same output (ASP_MAX_BATCH lowers it for
// tests).  pass(a, b, i) runs particles [a, b) as the i-th pass that completes; a batch
// whose pass returns kRetSplit is halved and tried again.  The caller accumulates for
// i > 0 and forms a ratio only after the last pass (b - a < n: there are several).
template <class F>
inline int for_batches(long long n, F&& pass) {
    const long long B = env_int("ASP_MAX_BATCH", 1LL << 30, 1, LLONG_MAX);
    std::vector<std::pair<long long, long long>> todo;  // batches, last first
    for (long long a = ((n - 1) / B) * B; a >= 0; a -= B) todo.push_back({a, std::min(n, a + B)});
    for (int i = 0; !todo.empty();) {
        const auto [a, b] = todo.back();
        todo.pop_back();
        const int rc = pass(a, b, i);
        if (rc == kRetSplit) {
            if (b - a < 2) return fail(ASP_ERR_UNSUPPORTED, "one particle makes >= 2^31 records");
            todo.push_back({a + (b - a) / 2, b});
            todo.push_back({a, a + (b - a) / 2});
            continue;
        }
        ASP_TRY(rc);
        ++i;
    }
    return ASP_OK;
}

// asp_last_stats reads slot 0's words: a call clears its workspace's, fills in what it
// measures and, when it ran in another slot, publishes them -- under slot 0's lock, since a
// slot-0 call on another thread writes the same words (no cycle: slot-0 calls never take
// another slot's lock).
inline void stats_clear(Workspace& ws) { std::fill(ws.stats, ws.stats + kNStats, 0LL); }
inline void stats_publish(Workspace& ws, int device) {
    if (&ws == &g_ws[device]) return;
    std::lock_guard<std::mutex> lk(g_ws[device].mu);
    std::copy(ws.stats, ws.stats + kNStats, g_ws[device].stats);
}

#define ASP_LAUNCHED()                                                                    \
    do {                                                                                  \
        hipError_t e_ = hipGetLastError();                                                \
        if (e_ != hipSuccess)                                                             \
            return fail(ASP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e_)); \
    } while (0)


}  // namespace asp
