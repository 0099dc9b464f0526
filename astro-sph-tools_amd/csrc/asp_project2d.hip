// asp_project2d.hip -- MI355X (gfx950) SPH particle -> pixel-grid projection.
//
// Replaces the reference's create_image / process_chunk / calculate_pixel_value /
// quartic_spline_kernel path (the reference's src/astro_sph_tools/tools/projections/
// _projector.py:13-120, _pixel_calculations.pyx:9-36, _kernels.pyx:9-20) with a
// scatter formulation built for CDNA4:
//
//   K1 count     one streaming pass over (u, v, h): per-workgroup LDS histogram of
//                (particle, GPU tile) insertions -> hist[block][tile], two streams per
//                tile: records whose box clipped to the tile is small / mid-size, and
//                LARGE ones (>= gather_min pixels on both axes, or >= gather_area pixels)
//   K2a colscan  per tile, exclusive prefix over blocks (in place) + tile totals
//   K2b tilescan one workgroup: tile start offsets in Morton order of the tiles, the
//                deposit work list (runs of <= CH records of one tile; empty tiles get
//                a zero item) and the merge list of tiles split over several items
//   K3 scatter   second streaming pass: each insertion written as a 32-byte PREPARED
//                record into its tile's run of its stream (LDS cursors)
//   K3b scale    (deterministic mode) per tile: power-of-two fixed-point scale
//   K4 deposit   one workgroup per work item of the small/mid stream: records -> LDS tile
//                accumulators; boxes of <= 4 x 4 pixels lane-per-record, mid-size boxes
//                swept by a whole wave (LDS atomics); the tile is written once, or (split
//                tiles) stored as a partial slab
//   K4g gather   the large stream: one single-wave workgroup per (work item, 16 x 32
//                region of the tile); the wave streams the item's records into per-lane
//                entries, walks those meeting its region with v_readlane (fields in
//                SGPRs), each lane summing one pixel of each 8 x 8 block in registers
//                (packed fp32, no per-pair atomics); tile or slab written from registers
//   K5 merge     split tiles: sum of their slabs in slab order, write
//   K6 wide      particles overlapping > wide_tiles tiles, per tile region, gathered
//   K7 ratio     out0 / out1 (mass-weighted maps) when not fused into K4/K5
//   K8 pairs     the kernel_func plug-in: every included (pixel, particle, r^2) pair
//
// No MFMA: this is gather/scatter work; the bounds are HBM bytes and VALU/LDS-atomic
// issue.
//
// Where the stages live (asp_map.hpp declares what the units share on the host,
// asp_map_device.hpp the device code more than one of them uses):
//   asp_map_bin.hip      K1, K3, K3b and their launchers
//   asp_binning.hpp      K2a, K2b (shared with the cube; launched from this file)
//   asp_map_deposit.hip  K4, K4g, K5, K6, K7, the evals diagnostic and their launchers
//   asp_pairs.hip        K8 and the plug-in session (asp_pairs_begin / _emit / _end)
//   asp_probes.hip       asp_kernel_eval, asp_chunk_ranges, asp_pixel_neighbours
//   this file            grids and windows, the pass driver (project2d_device,
//                        project2d_full), the map entry points and the library's general
//                        C-ABI (version, errors, ratio, profiling, stats, release)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/asp.h"
#include "asp_binning.hpp"
#include "asp_device.hpp"
#include "asp_host.hpp"
#include "asp_map.hpp"
#include "asp_map_device.hpp"

namespace asp {

// Records whose box clipped to a tile is at least this wide on both axes go to the large
// stream (K4g); the threshold is a Grid field so it can be tuned per call
// (ASP_GATHER_MIN).
constexpr int kGatherMinDefault = 5;
// ... or at least this many pixels: the thin slivers of large discs clipped at tile edges,
// which K4 sweeps a whole wave per record (ASP_GATHER_AREA): cfg 2 at
// physical h 11.42-11.49 -> 11.10 ms (12-20 alike), the pixel-scale map unchanged at 20
// (16 sends its 4 x 4 boxes to K4g: 3.25 -> 3.32 ms)
constexpr int kGatherAreaDefault = 20;

static uint32_t spread_bits(uint32_t x) {
    x &= 0xffff;
    x = (x | (x << 8)) & 0x00ff00ff;
    x = (x | (x << 4)) & 0x0f0f0f0f;
    x = (x | (x << 2)) & 0x33333333;
    x = (x | (x << 1)) & 0x55555555;
    return x;
}

static int ensure_morton(Workspace& ws, int ntx, int nty, hipStream_t st) {
    if (ws.morton_ntx == ntx && ws.morton_nty == nty) return ASP_OK;
    std::vector<std::pair<uint32_t, int>> key((size_t)ntx * nty);
    for (int tx = 0; tx < ntx; ++tx)
        for (int ty = 0; ty < nty; ++ty)
            key[(size_t)tx * nty + ty] = {spread_bits(tx) << 1 | spread_bits(ty), tx * nty + ty};
    std::sort(key.begin(), key.end());
    std::vector<int> order(key.size());
    for (size_t i = 0; i < key.size(); ++i) order[i] = key[i].second;
    ASP_TRY(ensure(ws.morton, order.size() * sizeof(int)));
    ASP_HIP(hipMemcpyAsync(ws.morton.p, order.data(), order.size() * sizeof(int),
                           hipMemcpyHostToDevice, st));
    ASP_HIP(hipStreamSynchronize(st));
    ws.morton_ntx = ntx;
    ws.morton_nty = nty;
    return ASP_OK;
}

bool make_grid(double x_min, double x_max, double y_min, double y_max, int nx, int ny, int cs,
               Grid& g) {
    if (!(nx > 0 && ny > 0 && cs > 0)) return false;
    if (!(x_max > x_min) || !(y_max > y_min)) return false;
    if (!std::isfinite(x_min) || !std::isfinite(x_max) || !std::isfinite(y_min) ||
        !std::isfinite(y_max))
        return false;
    g.x_min = x_min;
    g.y_min = y_min;
    g.psx = (x_max - x_min) / nx;
    g.psy_pix = (y_max - y_min) / nx;
    g.psy_cull = (y_max - y_min) / ny;
    if (!(g.psx > 0.0) || !(g.psy_pix > 0.0) || !(g.psy_cull > 0.0)) return false;
    g.xminf = (float)x_min;
    g.yminf = (float)y_min;
    g.ipsx = (float)(1.0 / g.psx);
    g.ipsy = (float)(1.0 / g.psy_pix);
    if (!std::isfinite(g.ipsx) || !std::isfinite(g.ipsy)) return false;
    // |corner| over the grid (absolute frame); 2x the tile span (the records' frames)
    const double mgl = 2.0 * kTile * std::max(g.psx, g.psy_pix);
    double mg = std::max({std::fabs(x_min), std::fabs(x_min + nx * g.psx), std::fabs(y_min),
                          std::fabs(y_min + ny * g.psy_pix), mgl});
    g.mg = (float)(mg * (1.0 + 1e-6));
    g.mgl = (float)(mgl * (1.0 + 1e-6));
    g.nx = nx;
    g.gnx = nx;
    g.ox = 0;
    g.ny = ny;
    g.cs = cs;
    g.ncx = (nx + cs - 1) / cs;
    g.ncy = (ny + cs - 1) / cs;
    g.ntx = (nx + kTile - 1) / kTile;
    g.nty = (ny + kTile - 1) / kTile;
    g.ntiles = g.ntx * g.nty;
    g.nonsquare = nx != ny;
    g.mixed = 0;
    g.wide_tiles = kWideTilesDefault;
    g.gather_min = kGatherMinDefault;
    g.gather_area = kGatherAreaDefault;
    return true;
}

constexpr int kMaxBinBlocks = 1024;  // count workgroups (hist rows)
constexpr int kMaxTiles = 4096;  // K1/K3 LDS: cursors + per-tile max (12 B/tile at 2 maps)
static_assert(kMaxTiles <= kScanThreads * 4, "k_tilescan holds <= 4 tiles per thread");

// Images of more than kMaxTiles GPU tiles are projected as WINDOWS of whole tile rows
// (image rows [ox, ox + nx) x all columns; kMaxTiles / nty tile rows each): every window
// is one pass of the pipeline over all particles with the footprints clipped to it, and
// its map is a contiguous part of the (nx, ny) C-order output.  Pixel corners, pitches
// and the chunk cull stay those of the whole image (Grid::gnx, Grid::ox), so every
// decision is the one-window decision.
int window_rows(const Grid& full) {  // tile rows per window
    return std::max(1, std::min(full.ntx, kMaxTiles / full.nty));
}
// Image rows [r0, r1) as a window (any r0: its tile grid starts at row r0).
Grid window_grid_rows(const Grid& full, int r0, int r1) {
    Grid g = full;
    g.ox = r0;
    g.nx = r1 - r0;
    g.ntx = (g.nx + kTile - 1) / kTile;
    g.ntiles = g.ntx * g.nty;
    return g;
}
Grid window_grid(const Grid& full, int tx0, int tx1) {  // whole tile rows
    return window_grid_rows(full, tx0 * kTile, std::min(tx1 * kTile, full.gnx));
}

// items / merges in the work-list buffers
// Deposit items in tilescan order (ASP_ITEM_ORDER=0, an A/B switch) instead of largest first.
// The split tile scan pays when maps run one after another on one stream (the side
// kernel runs beside this map's scatter, a free CU slot away).  With maps on two streams
// (two workspace slots in use) the device is already full of the other map's work: the
// side kernel, and the host's wait for the counters behind it, start late and the
// two-stream overlap loses more than the split saves (1.25e7 share: 0.592 vs 0.540 ms), so
// the one-launch scan is used there.  ASP_SPLIT_SCAN=0 / 1 forces either (read per call).
static bool split_scan_on() {
    if (env_set("ASP_SPLIT_SCAN")) return env_int("ASP_SPLIT_SCAN", 0) != 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return false;
    SlotTable& T = g_slots[dev];
    std::lock_guard<std::mutex> lock(T.mu);
    for (int k = 1; k < kMapSlots; ++k)
        if (T.used[k]) return false;
    return true;
}

static int item_order_identity() {  // (read once per process)
    static const int identity = env_int("ASP_ITEM_ORDER", 1) == 0 ? 1 : 0;
    return identity;
}
// deposit work items per map (ASP_ITEMS overrides kTargetItems2d; tuning only, read once)
static inline int item_target() {
    static const int t = (int)env_int("ASP_ITEMS", kTargetItems2d, 64);
    return t;
}
static inline size_t item_cap(const Grid& g) { return (size_t)2 * g.ntiles + item_target() + kTargetItems1 + 16; }
static inline size_t merge_cap(const Grid& g) { return (size_t)g.ntiles + 16; }

static int ratio_stage(Workspace& ws, float* o0, const float* o1, long long npix, hipStream_t st,
                       const int* guard = nullptr) {
    StageMark m(ws, kSRatio, st);
    ASP_TRY(launch_ratio(o0, o1, npix, st, guard));
    m.done();
    return ASP_OK;
}

// K3..K7 for one kernel / map count, on the caller's stream.  guard: the counter words
// behind a verifying scatter (every kernel returns at once when it rejected the layout).
static int run_tail(const Grid& g, const Src64& s, Workspace& ws, const Plan& pl, int kid, int nout,
                    bool det, const float* u, const float* v, const float* h, const float* a0,
                    const float* a1, float* o0, float* o1, int flags, hipStream_t st,
                    bool pre_scattered, const XArgs* xa, const int* guard = nullptr) {
    const bool ratio = (flags & ASP_F_RATIO) != 0;
    const bool fuse_ratio = ratio && pl.n_wide == 0;
    const int dflags = ((flags & ASP_F_ACCUMULATE) ? kFlagAccumulate : 0) |
                       (fuse_ratio ? kFlagRatio : 0);
    if (!pre_scattered)
        ASP_TRY(launch_scatter(g, s, ws, pl, kid, nout, det, u, v, h, a0, a1, kNoRecordCap,
                               0x7fffffff, st, false, xa));
    if (det) ASP_TRY(launch_tilescale(g, ws, pl, nout, st, guard));
    ASP_TRY(launch_deposit(g, s, ws, pl, kid, nout, det, u, v, h, a0, a1, o0, o1, dflags, st,
                           guard));
    if (ratio && !fuse_ratio) ASP_TRY(ratio_stage(ws, o0, o1, (long long)g.nx * g.ny, st, guard));
    return ASP_OK;
}

// ASP_REUSE_LAYOUT=0 (read per call: A/Bs, tests): every pass counts.
static bool reuse_layout_on() { return env_int("ASP_REUSE_LAYOUT", 1) != 0; }

static LayoutKey layout_key(const Workspace& ws, const Grid& g, const Src64& s, const Plan& pl,
                            const float* u, const float* v, const float* h) {
    LayoutKey k;
    memset(&k, 0, sizeof(k));  // (padding included: keys are compared word for word)
    k.n = pl.n;
    k.nblk = pl.nblk;
    k.stride = s.u64 ? s.stride : 0;
    k.x_min = g.x_min;
    k.y_min = g.y_min;
    k.psx = g.psx;
    k.psy_pix = g.psy_pix;
    k.psy_cull = g.psy_cull;
    k.nx = g.nx;
    k.ny = g.ny;
    k.cs = g.cs;
    k.gnx = g.gnx;
    k.ox = g.ox;
    k.ntiles = g.ntiles;
    k.nty = g.nty;
    k.nonsquare = g.nonsquare;
    k.mixed = g.mixed;
    k.grp = pl.grp;
    k.item_target = item_target();
    k.item_identity = item_order_identity();
    k.wide_tiles = g.wide_tiles;
    k.gather_min = g.gather_min;
    k.gather_area = g.gather_area;
    const void* src[5] = {s.u64, s.v64, s.cu64, s.cv64, s.h64};
    for (int j = 0; j < 5; ++j) k.src[j] = s.u64 ? src[j] : nullptr;
    k.pos[0] = u;
    k.pos[1] = v;
    k.pos[2] = h;
    const Buf* buf[7] = {&ws.hist, &ws.tile_total, &ws.tile_start, &ws.items, &ws.iorder,
                         &ws.merges, &ws.counters};
    for (int j = 0; j < 7; ++j) {
        k.buf[j] = buf[j]->p;
        k.cap[j] = buf[j]->cap;
    }
    return k;
}

// Tunables read once per call (experiments; the defaults are the measured choices).
static void grid_tunables(Grid& g) {
    g.wide_tiles = (int)env_int("ASP_WIDE_TILES", g.wide_tiles, 1);
    g.gather_min = (int)env_int("ASP_GATHER_MIN", g.gather_min, 2);
    g.gather_area = (int)env_int("ASP_GATHER_AREA", g.gather_area, 4);
}

// What asp_last_stats reports of a pass (asp.h): the layout's counters, how the records
// were scattered (path, ntrials) and whether the layout was reused.
static void pass_stats(Workspace& ws, const Grid& g, const Plan& pl, long long chunk, int path,
                       int ntrials, int reuse) {
    ws.stats[0] = pl.n_recs;
    ws.stats[1] = pl.n_items;
    ws.stats[2] = pl.n_wide;
    ws.stats[3] = kTile;
    ws.stats[4] = g.ntiles;
    ws.stats[5] = chunk;
    ws.stats[6] = pl.n_merges;
    ws.stats[7] = pl.n_slabs;
    ws.stats[8] = pl.n_large;
    ws.stats[13] = path;
    ws.stats[14] = ntrials;
    ws.stats[15] = reuse;
}

// A pass on the layout the previous pass left (ws.layout, whose key matches this pass):
// no count, no scans, no counter read-back.  The scatter runs in its verifying mode and the
// whole tail is enqueued behind it, every kernel guarded by the scatter's verdict; the host
// waits only for the copy of the verdict words, made on the side stream while the deposit
// runs.  outcome 1: the layout was exact for this pass's particles, the maps are written,
// and the pass is the counted pass's, kernel for kernel.  2: it was not; nothing was
// written (the outputs are untouched, also under ASP_F_ACCUMULATE), st is idle, and the
// caller counts.  0: not tried (the record or wide buffers are gone or too small).
static int reuse_pass(Workspace& ws, const Grid& g, const Src64& s, Plan pl, int kid, int nout,
                      bool det, const float* du, const float* dv, const float* dh,
                      const float* da0, const float* da1, float* d0, float* d1, int flags,
                      hipStream_t st, int& outcome) {
    outcome = 0;
    const Layout& L = ws.layout;
    pl.n_recs = L.ctr[0];
    pl.n_items = (int)L.ctr[1];
    pl.n_merges = (int)L.ctr[2];
    pl.n_slabs = (int)L.ctr[3];
    pl.n_wide = (int)L.ctr[4];
    pl.n_large = L.ctr[5];
    const long long rec_cap = record_capacity(ws);
    const int wide_cap = (int)std::min<size_t>(ws.wide.cap / sizeof(int), 0x7fffffff);
    if (!ws.recs.p || !ws.wide.p || !ws.h_counters || pl.n_recs > rec_cap || pl.n_wide > wide_cap)
        return ASP_OK;
    ASP_TRY(ensure(ws.slabs, (size_t)pl.n_slabs * nout * kTilePix * sizeof(long long)));
    ASP_TRY(ensure_side(ws));
    // The device counters the kernels read (records, wide count) are the counted pass's,
    // still in place; the words a scatter writes start from zero.
    int* dc = (int*)ws.counters.p;
    ASP_HIP(hipMemsetAsync(dc + cWideCursor, 0, kScatterWords * sizeof(int), st));
    int gate_dev = -1;
    if (scatter_gate_on() && hipGetDevice(&gate_dev) == hipSuccess) ASP_TRY(gate_wait(gate_dev, st));
    ASP_TRY(launch_scatter(g, s, ws, pl, kid, nout, det, du, dv, dh, da0, da1, rec_cap, wide_cap,
                           st, false, nullptr, true));
    int* hv = ws.h_counters + cNum;  // (the pinned mirror holds kMarks * cNum words)
    ASP_HIP(hipEventRecord(ws.scan_ev, st));
    ASP_HIP(hipStreamWaitEvent(ws.side, ws.scan_ev, 0));
    ASP_HIP(hipMemcpyAsync(hv, dc + cWideCursor, kScatterWords * sizeof(int),
                           hipMemcpyDeviceToHost, ws.side));
    ASP_HIP(hipEventRecord(ws.cnt_ev, ws.side));
    ASP_TRY(run_tail(g, s, ws, pl, kid, nout, det, du, dv, dh, da0, da1, d0, d1, flags, st, true,
                     nullptr, dc));
    if (gate_dev >= 0) ASP_TRY(gate_record(gate_dev, st));
    ASP_HIP(hipEventSynchronize(ws.cnt_ev));
    outcome = hv[cLayoutBad - cWideCursor] == 0 && hv[0] == pl.n_wide ? 1 : 2;
    if (outcome == 2) {  // the guarded tail returns at once; the buffers may be re-allocated after it
        ASP_HIP(hipStreamSynchronize(st));
        return ASP_OK;
    }
    stats_clear(ws);
    pass_stats(ws, g, pl, L.ctr[6], 1, 0, 1);
    return ASP_OK;
}

// The projection on DEVICE arrays (fp32 working copies u, v, h, a0, a1; s: the caller's
// fp64 arrays for exact re-decisions, or none) into DEVICE outputs, on stream st.  The
// caller holds the workspace lock and has ordered st behind the previous call.
// bin_only (the kernel_func plug-in session): stop after the scatter -- the records stay in
// ws for k_pairs -- and return the number of wide particles there.
// Returns kRetSplit (nothing written) when the pass would make >= 2^31 records.
// xa / nxp / xo (asp_project2d_props): nxp (1..4) further properties xa->a[0 ..] binned
// with the first two (their coefficients beside each record) and deposited in further
// passes into xo[0 ..] (two-map fp64 calls only).
int project2d_device(Workspace& ws, const Grid& gin, const Src64& s, const float* du,
                     const float* dv, const float* dh, const float* da0, const float* da1,
                     long long n, int kid, int flags, float* d0, float* d1, hipStream_t st,
                     int* bin_only, const XArgs* xa, int nxp, float* const* xo,
                     bool caller_arrays) {
    Grid g = gin;
    const int nout = d1 ? 2 : 1;
    const long long npix = (long long)g.nx * g.ny;
    // Every pass writes the layout buffers: the tag is set again only by a counted pass
    // that completes (or kept by a pass that reused the layout).
    const bool had_layout = ws.layout.valid;
    ws.layout.valid = false;
    if (ws.prof) ASP_TRY(prof_next(ws));
    Plan pl{};
    pl.n = n;
    if (n == 0) {  // all-zero map(s) (the ratio map of 0 / 0 is 0 as well)
        if (bin_only) {
            *bin_only = 0;
            return ASP_OK;
        }
        if (!(flags & ASP_F_ACCUMULATE)) {
            StageMark m(ws, kSMemset, st);
            ASP_HIP(hipMemsetAsync(d0, 0, npix * sizeof(float), st));
            if (d1) ASP_HIP(hipMemsetAsync(d1, 0, npix * sizeof(float), st));
            for (int j = 0; j < nxp; ++j) ASP_HIP(hipMemsetAsync(xo[j], 0, npix * sizeof(float), st));
            m.done();
        }
        stats_clear(ws);
        return ASP_OK;
    }
    ASP_TRY(ensure_morton(ws, g.ntx, g.nty, st));
    const long long max_blk = env_int("ASP_BIN_BLOCKS", kMaxBinBlocks, 1);
    pl.nblk = std::min<long long>(max_blk, std::max<long long>(1, (n + 8191) / 8192));
    pl.grp = (int)env_int("ASP_SCATTER_GROUP", kScatterGroup, 1);
    pl.nblk_s = (pl.nblk + pl.grp - 1) / pl.grp;
    const bool det = (flags & ASP_F_DETERMINISTIC) != 0;
    ASP_TRY(ensure(ws.hist, (size_t)pl.nblk * 2 * g.ntiles * sizeof(int)));
    if (det) ASP_TRY(ensure(ws.cmx, (size_t)pl.nblk_s * g.ntiles * nout * sizeof(unsigned)));
    ASP_TRY(ensure(ws.tile_total, (size_t)2 * g.ntiles * sizeof(int)));
    ASP_TRY(ensure(ws.tile_start, (size_t)2 * g.ntiles * sizeof(long long)));
    ASP_TRY(ensure(ws.tile_k, (size_t)g.ntiles * sizeof(int2)));
    ASP_TRY(ensure(ws.items, item_cap(g) * sizeof(Item)));
    ASP_TRY(ensure(ws.iorder, item_cap(g) * sizeof(int)));  // deposit order (k_tilescan)
    ASP_TRY(ensure(ws.merges, merge_cap(g) * sizeof(Merge)));
    // Layout reuse: caller_arrays -- u, v, h and s are the caller's own device
    // arrays (or derived from them on every call), not staging copies of host arrays, so
    // equal addresses mean the same particle set unless the caller rewrote it in place.
    int reuse = 0;  // stats[15]: 1 the layout was reused, 2 tried and rejected
    const bool may_reuse = caller_arrays && !xa && !bin_only && reuse_layout_on() &&
                           speculate_on() && !env_set("ASP_COUNT_EVALS");
    if (may_reuse && had_layout && ws.layout.armed) {
        const LayoutKey key = layout_key(ws, g, s, pl, du, dv, dh);
        if (memcmp(&key, &ws.layout.key, sizeof(key)) == 0) {
            ASP_TRY(reuse_pass(ws, g, s, pl, kid, nout, det, du, dv, dh, da0, da1, d0, d1, flags,
                               st, reuse));
            if (reuse == 1) {
                ws.layout.valid = true;
                return ASP_OK;
            }
            // a rejected attempt disarms at once: the counted pass below may leave early
            // (kRetSplit, an error) before it tags the layout
            if (reuse == 2) ws.layout.armed = false;
        }
    }
    ASP_TRY(counters_begin(ws, cNum, st));
    int* dc = (int*)ws.counters.p;
    ASP_TRY(launch_count(g, s, ws, pl, du, dv, dh, st));
    {
        StageMark m(ws, kSColscan, st);
        hipLaunchKernelGGL(k_colscan, dim3((2 * g.ntiles + 63) / 64, 1), dim3(kColscanBlock), 0,
                           st, (int*)ws.hist.p, (int)pl.nblk, 2 * g.ntiles,
                           (int*)ws.tile_total.p, (int)pl.nblk);
        ASP_LAUNCHED();
        m.done();
    }
    // The tile scan in two parts (round 6, ASP_SPLIT_SCAN=0: one launch): the tile starts
    // the scatter needs, on st; the work items, merge list and dispatch order the deposit
    // needs, on the side stream beside the scatter (a one-workgroup kernel off the critical
    // path).
    const bool split = split_scan_on();
    {
        StageMark m(ws, kSTilescan, st);
        if (split)
            hipLaunchKernelGGL((k_tilescan<4, 1>), dim3(1), dim3(kScanThreads), 0, st,
                               (const int*)ws.tile_total.p, (const int*)ws.morton.p, g.ntiles, 2,
                               (long long*)ws.tile_start.p, (Item*)ws.items.p, (Merge*)ws.merges.p,
                               dc, (int*)ws.iorder.p, item_order_identity(), item_target());
        else
            hipLaunchKernelGGL((k_tilescan<4>), dim3(1), dim3(kScanThreads), 0, st,
                               (const int*)ws.tile_total.p, (const int*)ws.morton.p, g.ntiles, 2,
                               (long long*)ws.tile_start.p, (Item*)ws.items.p, (Merge*)ws.merges.p,
                               dc, (int*)ws.iorder.p, item_order_identity(), item_target());
        ASP_LAUNCHED();
        m.done();
    }
    // One small read-back sizes the record / slab buffers.  With buffers
    // left by an earlier call, the scatter is enqueued BEFORE the host waits for it
    // (speculatively: it checks the counters against those capacities itself), so the
    // GPU does not idle across the host round trip.  The copy runs on the side stream, so
    // the scatter behind it on st need not wait for the copy's own latency (the cube's copy
    // is on its own stream: it has no side kernel to follow).
    ASP_TRY(ensure_side(ws));
    ASP_HIP(hipEventRecord(ws.scan_ev, st));
    int gate_dev = -1;  // ASP_SCATTER_GATE: this map's scatter after the last map's deposit
    if (scatter_gate_on() && hipGetDevice(&gate_dev) == hipSuccess) ASP_TRY(gate_wait(gate_dev, st));
    ASP_HIP(hipStreamWaitEvent(ws.side, ws.scan_ev, 0));
    if (split) {
        hipLaunchKernelGGL((k_tilescan<4, 2>), dim3(1), dim3(kScanThreads), 0, ws.side,
                           (const int*)ws.tile_total.p, (const int*)ws.morton.p, g.ntiles, 2,
                           (long long*)ws.tile_start.p, (Item*)ws.items.p, (Merge*)ws.merges.p,
                           dc, (int*)ws.iorder.p, item_order_identity(), item_target());
        ASP_LAUNCHED();
    }
    ASP_HIP(hipMemcpyAsync(ws.h_counters, dc, (size_t)cNum * sizeof(int), hipMemcpyDeviceToHost,
                           ws.side));
    ASP_HIP(hipEventRecord(ws.cnt_ev, ws.side));
    const long long rec_cap = record_capacity(ws);
    const int wide_cap = (int)std::min<size_t>(ws.wide.cap / sizeof(int), 0x7fffffff);
    // every scatter of this pass: the kernel for (kid, nout, det), given capacities, PROBE
    auto scatter = [&](long long rcap, int wcap, bool probe) {
        return launch_scatter(g, s, ws, pl, kid, nout, det, du, dv, dh, da0, da1, rcap, wcap, st,
                              probe);
    };
    // (not with extra properties: their coefficient array is sized from the counters)
    const bool spec = ws.recs.p && ws.wide.p && !xa && speculate_on();
    if (spec) ASP_TRY(scatter(rec_cap, wide_cap, false));
    ASP_HIP(hipEventSynchronize(ws.cnt_ev));
    if (split) ASP_HIP(hipStreamWaitEvent(st, ws.cnt_ev, 0));  // the deposit reads part 2's output
    const int* hc = ws.h_counters;
    pl.n_recs = hc[cRecs];
    pl.n_items = hc[cItems];
    pl.n_merges = hc[cMerges];
    pl.n_slabs = hc[cSlabs];
    pl.n_wide = hc[cWideCount];
    pl.n_large = hc[cLarge];
    bool pre = false;  // the speculative scatter did the work
    ASP_TRY(settle_speculation(spec, pl.n_recs, pl.n_recs <= rec_cap && pl.n_wide <= wide_cap, st,
                               pre));
    bool fresh = false;
    ASP_TRY(ensure_records(ws, pl.n_recs, fresh));
    ASP_TRY(ensure(ws.wide, (size_t)pl.n_wide * sizeof(int)));
    ASP_TRY(ensure(ws.slabs, (size_t)pl.n_slabs * nout * kTilePix * sizeof(long long)));
    XArgs xw{};
    if (xa) {  // the extra properties' coefficient array, one float4 per record
        ASP_TRY(ensure(ws.ext, (size_t)std::max(pl.n_recs, 1LL) * sizeof(float4)));
        xw = *xa;
        xw.ext = (float4*)ws.ext.p;
    }
    bool placed = false;  // the records are already scattered (by the placement trials)
    int ntrials = 0;      // scatter runs of the placement trials
    // (plain maps only: not the plug-in session's binning, nor a scatter that also writes
    // the extra properties' ws.ext)
    if (!bin_only && !xa && !pre && fresh) {
        auto trial = [&]() -> int {
            // the wide-list cursor is the one counter the scatter advances
            ASP_HIP(hipMemsetAsync(dc + cWideCursor, 0, sizeof(int), st));
            return scatter(kNoRecordCap, 0x7fffffff, true);
        };
        ASP_TRY(place_records(ws, record_bytes(pl.n_recs), st, trial, placed, &ntrials));
    }
    if (bin_only) {  // the plugin session: the records, for k_pairs
        // (the session bins with (indicator, 1 map, fp64): kid, nout and det are those)
        if (!pre) ASP_TRY(scatter(kNoRecordCap, 0x7fffffff, false));
        *bin_only = pl.n_wide;
        return ASP_OK;
    }
    const XArgs* xp = xa ? &xw : nullptr;
    ASP_TRY(run_tail(g, s, ws, pl, kid, nout, det, du, dv, dh, da0, da1, d0, d1, flags, st,
                     pre || placed, xp));
    for (int j = 0; xa && j < nxp; j += 2) {  // properties 2.. from the records, two per pass
        const bool two = j + 1 < nxp;
        const int dflags = (flags & ASP_F_ACCUMULATE) ? kFlagAccumulate : 0;
        // (fp64 sums only: check_props)
        ASP_TRY(launch_deposit_props(g, s, ws, pl, kid, two ? 2 : 1, du, dv, dh, xw.a[j],
                                     xw.a[two ? j + 1 : j], xo[j], two ? xo[j + 1] : nullptr,
                                     dflags, st, j / 2 + 1));
    }
    if (gate_dev >= 0) ASP_TRY(gate_record(gate_dev, st));
    stats_clear(ws);  // (the evals diagnostic below is of THIS pass only)
    if (env_set("ASP_COUNT_EVALS")) {  // diagnostic: the deposit kernels' lane-slots
        Buf& evals = ws.aux[kAuxCounters];
        ASP_TRY(ensure(evals, 3 * sizeof(unsigned long long)));
        ASP_HIP(hipMemsetAsync(evals.p, 0, 3 * sizeof(unsigned long long), st));
        ASP_TRY(launch_evals(g, s, ws, pl, kid, du, dv, dh, (unsigned long long*)evals.p, st));
        unsigned long long e[3];
        ASP_HIP(hipMemcpyAsync(e, evals.p, sizeof(e), hipMemcpyDeviceToHost, st));
        ASP_HIP(hipStreamSynchronize(st));
        ws.stats[9] = (long long)(e[0] + e[1] + e[2]);
        ws.stats[10] = (long long)e[0];
        ws.stats[11] = (long long)e[1];
        ws.stats[12] = (long long)e[2];
    }
    // how this pass's records were scattered: 1 the speculative launch (enqueued before the
    // counter read-back) was kept, 2 placement trials (stats[14] scatter runs), 3 the
    // speculative launch found the buffers too small and the scatter was relaunched after
    // growing them, 0 no earlier buffers (one plain launch)
    pass_stats(ws, g, pl, hc[cChunk], pre ? 1 : placed ? 2 : spec ? 3 : 0, ntrials, reuse);
    if (!xa) {  // the layout buffers are whole and this pass's: tag them
        Layout& L = ws.layout;
        const long long c[kLayoutCounters] = {pl.n_recs, pl.n_items, pl.n_merges, pl.n_slabs,
                                              pl.n_wide, pl.n_large, hc[cChunk]};
        if (reuse == 2) L.armed = false;
        else if (!L.armed) L.armed = L.have_last && std::equal(c, c + 6, L.last);
        std::copy(c, c + kLayoutCounters, L.ctr);
        std::copy(c, c + kLayoutCounters, L.last);
        L.have_last = true;
        L.key = layout_key(ws, g, s, pl, du, dv, dh);
        L.valid = caller_arrays;
    }
    return ASP_OK;
}

static Src64 src_from(const Src64& s, long long b) {  // particles b.. of s
    Src64 r = s;
    if (s.u64) {
        r.u64 += b * s.stride;
        r.v64 += b * s.stride;
        r.cu64 += b * s.stride;
        r.cv64 += b * s.stride;
        r.h64 += b;
    }
    r.u32 += b;
    r.v32 += b;
    r.h32 += b;
    return r;
}

// The whole call: every window of the image (window_grid) and, inside it, the particle
// batches of for_batches.  Batches after the first accumulate; the ratio of a batched map
// is formed at the end.
// rows [row_lo, row_hi) of the image only (asp_project2d_rows; default the whole image),
// d0 / d1 pointing at row row_lo: windows of <= window_rows tile rows from row_lo on.
// caller_arrays: the particle arrays are the caller's device arrays (project2d_device).
int project2d_full(Workspace& ws, const Grid& full, const Src64& s, const float* du,
                   const float* dv, const float* dh, const float* da0, const float* da1,
                   long long n, int kid, int flags, float* d0, float* d1, hipStream_t st,
                   int device, bool caller_arrays, int row_lo = 0, int row_hi = -1,
                   const XArgs* xa = nullptr, int nxp = 0, float* const* xo = nullptr) {
    const int wr = window_rows(full);
    long long agg[kNStats] = {0};
    if (row_hi < 0) row_hi = full.gnx;
    for (int r0 = row_lo; r0 < row_hi; r0 += wr * kTile) {
        const Grid g = window_grid_rows(full, r0, std::min(r0 + wr * kTile, row_hi));
        const long long off = (long long)(g.ox - row_lo) * full.ny;
        float* w0 = d0 + off;
        float* w1 = d1 ? d1 + off : nullptr;
        float* wx[4] = {nullptr, nullptr, nullptr, nullptr};  // the extra properties' maps
        for (int j = 0; j < nxp; ++j) wx[j] = xo[j] + off;
        int passes = 0;
        ASP_TRY(for_batches(n, [&](long long a, long long b, int i) -> int {
            int f = flags;
            if (b - a < n) f &= ~ASP_F_RATIO;  // ratio after the last batch
            if (i > 0) f |= ASP_F_ACCUMULATE;
            XArgs xb{};
            if (xa) {
                xb = *xa;
                for (int j = 0; j < 4; ++j) xb.a[j] += a;
            }
            ASP_TRY(project2d_device(ws, g, src_from(s, a), du + a, dv + a, dh + a, da0 + a,
                                     da1 ? da1 + a : nullptr, b - a, kid, f, w0, w1, st, nullptr,
                                     xa ? &xb : nullptr, nxp, wx, caller_arrays));
            passes = i + 1;
            for (int k : {0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 14}) agg[k] += ws.stats[k];
            agg[13] = std::max(agg[13], ws.stats[13]);
            agg[15] = std::max(agg[15], ws.stats[15]);
            return ASP_OK;
        }));
        if (passes > 1 && (flags & ASP_F_RATIO))
            ASP_TRY(ratio_stage(ws, w0, w1, (long long)g.nx * g.ny, st));
    }
    for (int k : {0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}) ws.stats[k] = agg[k];
    ws.stats[4] = (long long)((row_hi - row_lo + kTile - 1) / kTile) * full.nty;
    stats_publish(ws, device);
    return ASP_OK;
}

// The properties to deposit (T: the caller's precision): the first two, nxp further ones
// (asp_project2d_props) and the SPH weights m (, rho) of asp_project2d_sph.
template <class T>
struct Props {
    const T *a0 = nullptr, *a1 = nullptr;
    const T* const* xprops = nullptr;
    int nxp = 0;
    const T *wm = nullptr, *wr = nullptr;
};

static int check_args(const void* a1, const float* out0, const float* out1, long long n, int kid,
                      int flags) {
    if (n < 0) return fail(ASP_ERR_INVALID, "n < 0");
    if (kid < 0 || kid > ASP_KERNEL_WENDLAND_C2_COLUMN)
        return fail(ASP_ERR_INVALID, "unknown kernel_id");
    if (!out0) return fail(ASP_ERR_INVALID, "out0 is NULL");
    if ((a1 == nullptr) != (out1 == nullptr))
        return fail(ASP_ERR_INVALID, "a1 and out1 must both be given or both be NULL");
    if ((flags & ASP_F_RATIO) && !out1) return fail(ASP_ERR_INVALID, "ASP_F_RATIO needs out1");
    if ((flags & ASP_F_RATIO) && (flags & ASP_F_ACCUMULATE))
        return fail(ASP_ERR_INVALID, "ASP_F_RATIO cannot be combined with ASP_F_ACCUMULATE");
    // The int64 fixed point quantises each map on its own per-tile scale: pixels covered
    // only by kernel tails keep a few units of weight, so their quotient has no precision
    // (DESIGN.md §4, round 4).  Ratio maps are fp64-accumulated only.
    if ((flags & ASP_F_RATIO) && (flags & ASP_F_DETERMINISTIC))
        return fail(ASP_ERR_INVALID, "ASP_F_RATIO cannot be combined with ASP_F_DETERMINISTIC "
                                     "(fixed-point components carry no relative precision in "
                                     "kernel-tail pixels; form ratios from fp64 maps)");
    return ASP_OK;
}

int setup_grid(const MapArgs& m, Grid& g) {
    if (!make_grid(m.x_min, m.x_max, m.y_min, m.y_max, m.nx, m.ny, m.cs, g))
        return fail(ASP_ERR_INVALID,
                    "invalid grid: need nx, ny, chunk_size >= 1, finite x_max > x_min, "
                    "y_max > y_min");
    grid_tunables(g);
    if (g.nty > kMaxTiles)
        return fail(ASP_ERR_UNSUPPORTED, "image too wide (ny > 4096 * 64 pixels)");
    return ASP_OK;
}

// Host outputs: device maps in the workspace (pre-loaded for ASP_F_ACCUMULATE).
static int host_outputs(Workspace& ws, float* out0, float* out1, long long npix, int flags,
                        hipStream_t st, float*& d0, float*& d1) {
    const size_t bytes = (size_t)npix * sizeof(float);
    ASP_TRY(device_scratch(ws.out[0], d0, bytes));
    if (out1) ASP_TRY(device_scratch(ws.out[1], d1, bytes));
    if (flags & ASP_F_ACCUMULATE) {
        ASP_HIP(hipMemcpyAsync(d0, out0, bytes, hipMemcpyHostToDevice, st));
        if (d1) ASP_HIP(hipMemcpyAsync(d1, out1, bytes, hipMemcpyHostToDevice, st));
    }
    return ASP_OK;
}

static int host_results(float* out0, float* out1, const float* d0, const float* d1,
                        long long npix, hipStream_t st) {
    ASP_TRY(to_host(out0, d0, npix * sizeof(float), st));
    if (out1) ASP_TRY(to_host(out1, d1, npix * sizeof(float), st));
    ASP_HIP(hipStreamSynchronize(st));
    return ASP_OK;
}

// xprops / nxp / xouts: asp_project2d_props' properties 2.. (device pointers).
static int check_props(int nxp, const void* const* xprops, float* const* xouts, int flags) {
    if (nxp == 0) return ASP_OK;
    if (nxp < 0 || nxp > 4) return fail(ASP_ERR_INVALID, "nprops must be 1 .. 6");
    if (!xprops || !xouts) return fail(ASP_ERR_INVALID, "NULL props / outs");
    for (int j = 0; j < nxp; ++j)
        if (!xprops[j] || !xouts[j]) return fail(ASP_ERR_INVALID, "NULL property or output");
    if (!(flags & ASP_F_DEVICE_PTRS))
        return fail(ASP_ERR_UNSUPPORTED, "more than two properties: device pointers only "
                                         "(ASP_F_DEVICE_PTRS)");
    if (flags & (ASP_F_RATIO | ASP_F_DETERMINISTIC))
        return fail(ASP_ERR_UNSUPPORTED, "more than two properties: no ASP_F_RATIO / "
                                         "ASP_F_DETERMINISTIC (fp64 sums; ratios with asp_ratio)");
    return ASP_OK;
}

// SPH weights (asp_project2d_sph, north_star's "mass/rho-weighted scatter"): the fp32
// working copy of a property A is fl32(A * (m / rho)) -- evaluated in fp64 from the
// caller's values, rounded once (rho NULL: fl32(A * m)).  The SPH estimate of a field is
// sum_j (m_j / rho_j) A_j W(r_ij, h_j) (get_densities: _SnapshotBase.py:833); the scatter
// then bins and deposits these coefficients as any property's.
template <class T>
__global__ __launch_bounds__(kBlock) void k_weigh(const T* __restrict__ a, const T* __restrict__ m,
                                                  const T* __restrict__ rho,
                                                  float* __restrict__ out, long long n) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n;
         i += (long long)gridDim.x * kBlock) {
        const double w = rho ? (double)m[i] / (double)rho[i] : (double)m[i];
        out[i] = (float)((double)a[i] * w);
    }
}

// The weighted fp32 copies of a0 (, a1) and properties 2.. into ws.wts (slot k = property
// k), on st; the pointers are redirected to them.  dev: m and rho are device arrays (else
// they are staged into ws.inw first).
template <class T>
static int weigh_props(Workspace& ws, const Props<T>& p, const T* a0, const T* a1, long long n,
                       bool dev, hipStream_t st, const float** da0, const float** da1,
                       const float** xw) {
    const T *dm = p.wm, *dr = p.wr;
    if (!dev) {
        ASP_TRY(to_device(ws, ws.inw[0], dm, (size_t)n * sizeof(T), st, Copy::kPinned));
        if (dr) ASP_TRY(to_device(ws, ws.inw[1], dr, (size_t)n * sizeof(T), st, Copy::kPinned));
    }
    const T* src[6] = {a0, a1, nullptr, nullptr, nullptr, nullptr};
    for (int j = 0; j < p.nxp; ++j) src[2 + j] = p.xprops[j];
    for (int k = 0; k < 6; ++k) {
        if (!src[k]) continue;
        ASP_TRY(ensure(ws.wts[k], (size_t)std::max(n, 1LL) * sizeof(float)));
        if (n > 0) {
            hipLaunchKernelGGL(k_weigh<T>, dim3(stream_blocks(n)), dim3(kBlock), 0, st, src[k], dm,
                               dr, (float*)ws.wts[k].p, n);
            ASP_LAUNCHED();
        }
    }
    *da0 = (const float*)ws.wts[0].p;
    if (a1) *da1 = (const float*)ws.wts[1].p;
    for (int j = 0; j < p.nxp; ++j) xw[j] = (const float*)ws.wts[2 + j].p;
    return ASP_OK;
}

// What every map entry point checks first (arrays: the particle arrays are all given).
template <class T>
static int check_map(const MapArgs& m, const Props<T>& p, long long n, bool arrays) {
    ASP_TRY(check_args(p.a1, m.out0, m.out1, n, m.kid, m.flags));
    ASP_TRY(check_props(p.nxp, (const void* const*)p.xprops, m.xouts, m.flags));
    if (p.nxp > 0 && !p.a1) return fail(ASP_ERR_INVALID, "properties 2.. need a1 / out1");
    if (n > 0 && !arrays) return fail(ASP_ERR_INVALID, "NULL particle array");
    return ASP_OK;
}

// xw: the fp32 arrays of properties 2.. (unused entries repeat the first)
static XArgs extra_args(const float* const* xw, int nxp) {
    XArgs xa{};
    for (int j = 0; j < 4; ++j) xa.a[j] = nxp ? xw[j < nxp ? j : 0] : nullptr;
    return xa;
}

static int project2d(const float* u, const float* v, const float* h, long long n,
                     const Props<float>& p, const MapArgs& m) {
    ASP_TRY(check_map(m, p, n, u && v && h && p.a0));
    Grid g;
    ASP_TRY(setup_grid(m, g));
    const int row_lo = m.row_lo, row_hi = m.row_hi < 0 ? m.nx : m.row_hi;
    if (row_lo < 0 || row_lo >= row_hi || row_hi > m.nx)
        return fail(ASP_ERR_INVALID, "rows: need 0 <= row_lo < row_hi <= nx");
    return with_workspace(m.device, (hipStream_t)m.stream, true, [&](Workspace& ws, hipStream_t st) -> int {
        const int nout = m.out1 ? 2 : 1;
        const bool dev = m.flags & ASP_F_DEVICE_PTRS;
        // the rows this call writes (the grid keeps the whole image's)
        const long long npix = (long long)(row_hi - row_lo) * m.ny;
        const float *du = u, *dv = v, *dh = h, *da0 = p.a0, *da1 = p.a1;
        float *d0 = m.out0, *d1 = m.out1;
        if (!dev) {
            const float** src[5] = {&du, &dv, &dh, &da0, &da1};
            for (int k = 0; k < 4 + (nout == 2); ++k)
                ASP_TRY(to_device(ws, ws.in[k], *src[k], (size_t)n * sizeof(float), st,
                                  Copy::kPinned));
            ASP_TRY(host_outputs(ws, m.out0, m.out1, npix, m.flags, st, d0, d1));
        }
        const float* xw[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int j = 0; j < p.nxp; ++j) xw[j] = p.xprops[j];
        if (p.wm)  // asp_project2d_sph: the properties times m / rho
            ASP_TRY(weigh_props<float>(ws, p, da0, da1, n, dev, st, &da0, &da1, xw));
        const Src64 s{nullptr, nullptr, nullptr, nullptr, nullptr, 0, du, dv, dh};
        const XArgs xa = extra_args(xw, p.nxp);
        ASP_TRY(project2d_full(ws, g, s, du, dv, dh, da0, da1, n, m.kid, m.flags, d0, d1, st,
                               m.device, dev, row_lo, row_hi, p.nxp ? &xa : nullptr, p.nxp, m.xouts));
        if (!dev) ASP_TRY(host_results(m.out0, m.out1, d0, d1, npix, st));
        return ASP_OK;
    });
}

// create_image on the reader's fp64 arrays: stage (axis selection, fp32 working copies in
// HBM) and project with the fp64 values kept for the exact re-decisions.
__global__ __launch_bounds__(kBlock) void k_to_f32(const double* __restrict__ a,
                                                   float* __restrict__ b, long long n) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n;
         i += (long long)gridDim.x * kBlock)
        b[i] = (float)a[i];  // round to nearest, as NumPy's astype(float32)
}

// axis: the pixel test's axis, | ASP_AXIS_CULL(c) to cull on axis c's columns
int decode_axis(int& axis, int& cull_axis) {
    cull_axis = (axis >> 4) ? (axis >> 4) - 1 : (axis & 15);
    axis &= 15;
    if (axis < 0 || axis > 2 || cull_axis < 0 || cull_axis > 2)
        return fail(ASP_ERR_INVALID, "projection axis must be 0 (X), 1 (Y) or 2 (Z)");
    return ASP_OK;
}

// The resident fp64 (n, 3) positions and h as the exact source of the image-plane
// coordinates, beside their fp32 working copies f = {u, v, h}.
Src64 src64_from_positions(const double* dpos, const double* dh, int axis, int cull_axis,
                                  float* const* f) {
    static const int cols[3][2] = {{1, 2}, {0, 2}, {0, 1}};  // _projector.py:38-46
    return Src64{dpos + cols[axis][0], dpos + cols[axis][1], dpos + cols[cull_axis][0],
                 dpos + cols[cull_axis][1], dh, 3, f[0], f[1], f[2]};
}

static int project2d_f64(const double* pos, const double* h, long long n, int axis,
                         const Props<double>& p, const MapArgs& m) {
    ASP_TRY(check_map(m, p, n, pos && h && p.a0));
    int cull_axis = 0;
    ASP_TRY(decode_axis(axis, cull_axis));
    Grid g;
    ASP_TRY(setup_grid(m, g));
    g.mixed = cull_axis != axis;
    return with_workspace(m.device, (hipStream_t)m.stream, true, [&](Workspace& ws, hipStream_t st) -> int {
        const int nout = m.out1 ? 2 : 1;
        const bool dev = m.flags & ASP_F_DEVICE_PTRS;
        const bool dev_out = dev || (m.flags & ASP_F_DEVICE_OUTPUTS);  // maps stay on the device
        const long long npix = (long long)m.nx * m.ny;
        const double *dpos = pos, *dh64 = h, *da0 = p.a0, *da1 = p.a1;
        float *d0 = m.out0, *d1 = m.out1;
        if (!dev) {
            // the fp64 arrays stay resident: the exact re-decisions read positions and h
            const double** src[4] = {&dpos, &dh64, &da0, &da1};
            for (int k = 0; k < 3 + (nout == 2); ++k)
                ASP_TRY(to_device(ws, ws.in64[k], *src[k], (size_t)n * (k ? 1 : 3) * sizeof(double),
                                  st, Copy::kPinned));
            if (!dev_out) ASP_TRY(host_outputs(ws, m.out0, m.out1, npix, m.flags, st, d0, d1));
        }
        for (int k = 0; k < 4 + (nout == 2); ++k)
            ASP_TRY(ensure(ws.in[k], (size_t)n * sizeof(float)));
        float* f[5] = {(float*)ws.in[0].p, (float*)ws.in[1].p, (float*)ws.in[2].p,
                       (float*)ws.in[3].p, nout == 2 ? (float*)ws.in[4].p : nullptr};
        // asp_project2d_sph_f64: the properties' fp32 copies are m / rho * A (weigh_props), so
        // the staging converts positions and h only
        const bool sph = p.wm != nullptr;
        ASP_TRY(stage_device(dpos, dh64, sph ? nullptr : da0, sph ? nullptr : da1, n, axis, f[0],
                             f[1], f[2], sph ? nullptr : f[3], sph ? nullptr : f[4], st));
        const float* fa0 = f[3];
        const float* fa1 = f[4];
        const float* xw[4] = {nullptr, nullptr, nullptr, nullptr};
        if (sph) ASP_TRY(weigh_props<double>(ws, p, da0, da1, n, dev, st, &fa0, &fa1, xw));
        const Src64 s = src64_from_positions(dpos, dh64, axis, cull_axis, f);
        for (int j = 0; j < p.nxp && !sph; ++j) {  // fp32 working copies of properties 2..
            ASP_TRY(ensure(ws.inx[j], (size_t)std::max(n, 1LL) * sizeof(float)));
            if (n > 0) {
                hipLaunchKernelGGL(k_to_f32, dim3(stream_blocks(n)), dim3(kBlock), 0, st,
                                   p.xprops[j], (float*)ws.inx[j].p, n);
                ASP_LAUNCHED();
            }
            xw[j] = (const float*)ws.inx[j].p;
        }
        const XArgs xa = extra_args(xw, p.nxp);
        ASP_TRY(project2d_full(ws, g, s, f[0], f[1], f[2], fa0, fa1, n, m.kid,
                               (m.flags & ~ASP_F_DEVICE_OUTPUTS) | ASP_F_DEVICE_PTRS, d0, d1, st,
                               m.device, dev, 0, -1, p.nxp ? &xa : nullptr, p.nxp, m.xouts));
        if (!dev_out) ASP_TRY(host_results(m.out0, m.out1, d0, d1, npix, st));
        return ASP_OK;
    });
}

// The first two of the props / outs lists are a0 / a1 and out0 / out1, the rest properties
// 2..5 (asp_project2d_props, asp_project2d_sph and their fp64 forms).
template <class T>
static int slice_props(const T* const* props, float* const* outs, int nprops, Props<T>& p,
                       MapArgs& m) {
    if (nprops < 1 || nprops > 6 || !props || !outs)
        return fail(ASP_ERR_INVALID, "nprops must be 1 .. 6 with props / outs given");
    p.a0 = props[0];
    p.a1 = nprops > 1 ? props[1] : nullptr;
    p.xprops = nprops > 2 ? props + 2 : nullptr;
    p.nxp = std::max(0, nprops - 2);
    m.out0 = outs[0];
    m.out1 = nprops > 1 ? outs[1] : nullptr;
    m.xouts = nprops > 2 ? outs + 2 : nullptr;
    return ASP_OK;
}

}  // namespace asp

// ==================================================================================
// C-ABI
// ==================================================================================
using namespace asp;

extern "C" {

int asp_version(void) { return ASP_API_VERSION * 10000 + 2; }

const char* asp_last_error(void) { return t_err.c_str(); }

int asp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int asp_project2d(const float* u, const float* v, const float* h, const float* a0,
                  const float* a1, int64_t n, double u_min, double u_max, double v_min,
                  double v_max, int32_t nx, int32_t ny, int32_t chunk_size, int32_t kernel_id,
                  int32_t flags, float* out0, float* out1, int32_t device, void* stream) {
    t_err.clear();
    return project2d(u, v, h, n, Props<float>{a0, a1},
                     MapArgs{u_min, u_max, v_min, v_max, nx, ny, chunk_size, kernel_id, flags, out0,
                             out1, device, stream});
}

int asp_project2d_rows(const float* u, const float* v, const float* h, const float* a0,
                       const float* a1, int64_t n, double u_min, double u_max, double v_min,
                       double v_max, int32_t nx, int32_t ny, int32_t chunk_size, int32_t row_lo,
                       int32_t row_hi, int32_t kernel_id, int32_t flags, float* out0,
                       float* out1, int32_t device, void* stream) {
    t_err.clear();
    return project2d(u, v, h, n, Props<float>{a0, a1},
                     MapArgs{u_min, u_max, v_min, v_max, nx, ny, chunk_size, kernel_id, flags, out0,
                             out1, device, stream, row_lo, row_hi});
}

int asp_project2d_props(const float* u, const float* v, const float* h, const float* const* props,
                        int32_t nprops, int64_t n, double u_min, double u_max, double v_min,
                        double v_max, int32_t nx, int32_t ny, int32_t chunk_size,
                        int32_t kernel_id, int32_t flags, float* const* outs, int32_t device,
                        void* stream) {
    t_err.clear();
    Props<float> p;
    MapArgs m{u_min, u_max, v_min, v_max, nx, ny, chunk_size, kernel_id, flags, nullptr,
              nullptr, device, stream};
    ASP_TRY(slice_props(props, outs, nprops, p, m));
    return project2d(u, v, h, n, p, m);
}

int asp_project2d_props_f64(const double* positions, const double* h,
                            const double* const* props, int32_t nprops, int64_t n, int32_t axis,
                            double u_min, double u_max, double v_min, double v_max, int32_t nx,
                            int32_t ny, int32_t chunk_size, int32_t kernel_id, int32_t flags,
                            float* const* outs, int32_t device, void* stream) {
    t_err.clear();
    Props<double> p;
    MapArgs m{u_min, u_max, v_min, v_max, nx, ny, chunk_size, kernel_id, flags, nullptr,
              nullptr, device, stream};
    ASP_TRY(slice_props(props, outs, nprops, p, m));
    return project2d_f64(positions, h, n, axis, p, m);
}

int asp_project2d_sph(const float* u, const float* v, const float* h, const float* mass,
                      const float* rho, const float* const* props, int32_t nprops, int64_t n,
                      double u_min, double u_max, double v_min, double v_max, int32_t nx,
                      int32_t ny, int32_t chunk_size, int32_t kernel_id, int32_t flags,
                      float* const* outs, int32_t device, void* stream) {
    t_err.clear();
    Props<float> p;
    MapArgs m{u_min, u_max, v_min, v_max, nx, ny, chunk_size, kernel_id, flags, nullptr,
              nullptr, device, stream};
    ASP_TRY(slice_props(props, outs, nprops, p, m));
    if (n > 0 && !mass) return fail(ASP_ERR_INVALID, "NULL mass array");
    p.wm = mass;
    p.wr = rho;
    return project2d(u, v, h, n, p, m);
}

int asp_project2d_sph_f64(const double* positions, const double* h, const double* mass,
                          const double* rho, const double* const* props, int32_t nprops,
                          int64_t n, int32_t axis, double u_min, double u_max, double v_min,
                          double v_max, int32_t nx, int32_t ny, int32_t chunk_size,
                          int32_t kernel_id, int32_t flags, float* const* outs, int32_t device,
                          void* stream) {
    t_err.clear();
    Props<double> p;
    MapArgs m{u_min, u_max, v_min, v_max, nx, ny, chunk_size, kernel_id, flags, nullptr,
              nullptr, device, stream};
    ASP_TRY(slice_props(props, outs, nprops, p, m));
    if (n > 0 && !mass) return fail(ASP_ERR_INVALID, "NULL mass array");
    p.wm = mass;
    p.wr = rho;
    return project2d_f64(positions, h, n, axis, p, m);
}

int asp_project2d_f64(const double* positions, const double* h, const double* a0,
                      const double* a1, int64_t n, int32_t axis, double u_min, double u_max,
                      double v_min, double v_max, int32_t nx, int32_t ny, int32_t chunk_size,
                      int32_t kernel_id, int32_t flags, float* out0, float* out1, int32_t device,
                      void* stream) {
    t_err.clear();
    return project2d_f64(positions, h, n, axis, Props<double>{a0, a1},
                         MapArgs{u_min, u_max, v_min, v_max, nx, ny, chunk_size, kernel_id, flags,
                                 out0, out1, device, stream});
}

int asp_ratio(float* out0, const float* out1, int64_t n, int32_t device, void* stream) {
    t_err.clear();
    if (n < 0 || !out0 || !out1) return fail(ASP_ERR_INVALID, "bad argument");
    if (n == 0) return ASP_OK;
    ASP_TRY(set_device(device));
    return launch_ratio(out0, out1, (long long)n, (hipStream_t)stream);
}

int asp_profile_stages(int32_t device, uint32_t stage_mask) {
    t_err.clear();
    ASP_TRY(set_device(device));
    for (int sl = 0; sl < kMapSlots; ++sl) {  // every map slot's workspace
        Workspace& ws = slot_ws(device, sl);
        std::lock_guard<std::mutex> lock(ws.mu);
        if (stage_mask && !ws.ev[0][0][0][0])
            for (int q = 0; q < 2; ++q)
                for (int k = 0; k < kStages; ++k)
                    for (int j = 0; j < kMarks; ++j)
                        for (int e = 0; e < 2; ++e) ASP_HIP(hipEventCreate(&ws.ev[q][k][j][e]));
        for (int k = 0; k < kStages; ++k) {
            ws.stage_ms[k] = 0.0;
            ws.stage_n[k] = 0;
            ws.ev_live[0][k] = ws.ev_live[1][k] = 0;
        }
        ws.prof = stage_mask != 0u;
        ws.prof_mask = stage_mask;
    }
    return ASP_OK;
}

int asp_profile(int32_t device, int32_t enable) {
    return asp_profile_stages(device, enable ? 0xffffffffu : 0u);
}

int asp_profile_read(int32_t device, double* ms_sum, int64_t* launches, int32_t nstages) {
    t_err.clear();
    if (device < 0 || device >= kMaxDevices || !ms_sum || !launches)
        return fail(ASP_ERR_INVALID, "bad argument");
    for (int k = 0; k < nstages; ++k) {
        ms_sum[k] = 0.0;
        launches[k] = 0;
    }
    for (int sl = 0; sl < kMapSlots; ++sl) {  // summed over the map slots
        Workspace& ws = slot_ws(device, sl);
        std::lock_guard<std::mutex> lock(ws.mu);
        if (ws.prof) {
            ASP_HIP(hipSetDevice(device));
            ASP_TRY(prof_fold(ws));
        }
        for (int k = 0; k < nstages && k < kStages; ++k) {
            ms_sum[k] += ws.stage_ms[k];
            launches[k] += ws.stage_n[k];
        }
    }
    return ASP_OK;
}

int asp_last_stats(int32_t device, int64_t* stats, int32_t nstats) {
    if (device < 0 || device >= kMaxDevices || !stats) return fail(ASP_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(g_ws[device].mu);  // a call in flight writes them
    for (int k = 0; k < nstats && k < kNStats; ++k) stats[k] = g_ws[device].stats[k];
    return ASP_OK;
}

int asp_release(int32_t device) {
    int lo = device < 0 ? 0 : device, hi = device < 0 ? kMaxDevices - 1 : device;
    int ndev = std::min(asp_device_count(), kMaxDevices);
    for (int d = lo; d <= hi && d < ndev; ++d)
      for (int sl = 0; sl < kMapSlots; ++sl) {
        Workspace& ws = slot_ws(d, sl);
        std::lock_guard<std::mutex> lock(ws.mu);
        if (hipSetDevice(d) != hipSuccess) continue;
        if (ws.last_ev) (void)hipEventSynchronize(ws.last_ev);
        free_buffers(ws);
        ws.layout = Layout{};
        if (ws.h_counters) (void)hipHostFree(ws.h_counters);
        ws.h_counters = nullptr;
        release_pinned(ws);
        ws.morton_ntx = ws.morton_nty = -1;
        ws.morton3_key[0] = ws.morton3_key[1] = ws.morton3_key[2] = -1;
    }
    return ASP_OK;
}

}  // extern "C"
