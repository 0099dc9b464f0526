// asp_map.hpp -- what the translation units of the 2-D map share on the host: the binning
// constants, the pass plan, the stage launchers (each defined in the unit that owns the
// kernels it launches) and the driver's entry points.
//
//   asp_map_bin.hip      K1 count, K3 scatter, K3b tile scale
//   asp_map_deposit.hip  K4 deposit, K4g gather, K5 merge, K6 wide, K7 ratio, the evals
//                        diagnostic
//   asp_project2d.hip    grids and windows, the pass driver, the map entry points
//   asp_pairs.hip        K8 pairs and the kernel_func plug-in session
//   asp_probes.hip       kernel evaluation, chunk ranges, neighbour lists
#pragma once

#include <algorithm>

#include "asp_device.hpp"
#include "asp_host.hpp"

namespace asp {

constexpr int kCountBlock = 256;   // count workgroup
#ifndef ASP_COUNT_UNROLL
#define ASP_COUNT_UNROLL 4
#endif
constexpr int kCountUnroll = ASP_COUNT_UNROLL;  // particles per lane and batch in count
// Scatter workgroup and how many consecutive count workgroups' particles it takes over:
// fewer, wider scatter workgroups keep fewer partially written record lines open at a
// time (each workgroup appends to its own segment of every tile).
#ifndef ASP_SCATTER_BLOCK
#define ASP_SCATTER_BLOCK 512
#endif
#ifndef ASP_SCATTER_GROUP_DEF
#define ASP_SCATTER_GROUP_DEF 4
#endif
constexpr int kScatterBlock = ASP_SCATTER_BLOCK;
constexpr int kScatterGroup = ASP_SCATTER_GROUP_DEF;
constexpr int kUnroll = (int)(kCountBlock * kCountUnroll / kScatterBlock);  // particles per lane and batch in scatter
// Particles per loop iteration of a count / scatter workgroup (a "batch").  Batches are
// dealt to the count workgroups round-robin (batch j to workgroup j % nblk; the scatter
// workgroup of count workgroups sb*grp.. takes their batches in order), so at any moment
// the whole grid streams one window of the particle arrays.
constexpr long long kBatch = (long long)kCountBlock * kCountUnroll;
static_assert(kBatch == (long long)kScatterBlock * kUnroll, "count and scatter batches differ");

static_assert(kAccF64 == 0 && kAccFix == 1, "dispatch() passes ACC as Int<0> / Int<1>");

// Properties 2..5 of asp_project2d_props (NX = 1): their arrays (unused ones repeat
// a[0]) and the per-record coefficient array ext (float4 {c2, c3, c4, c5} at the record's
// slot), written beside the records so every further pair of maps deposits from the SAME
// binning.
struct XArgs {
    const float* a[4];
    float4* ext;
};

struct Plan {
    long long n, nblk;  // particles, count workgroups
    long long nblk_s;   // scatter workgroups (grp count workgroups each)
    int grp;
    int n_items, n_merges, n_slabs, n_wide;
    long long n_recs, n_large;  // records; of them in the large stream
};

// What a map entry point is asked for, apart from the particles: the image, the kernel,
// the outputs and where to run.
struct MapArgs {
    double x_min, x_max, y_min, y_max;
    int nx, ny, cs, kid, flags;
    float *out0, *out1;
    int device;
    void* stream;
    int row_lo = 0, row_hi = -1;     // asp_project2d_rows
    float* const* xouts = nullptr;  // the maps of properties 2..
};

inline unsigned stream_blocks(long long n) {  // grid of a grid-stride streaming kernel
    return (unsigned)std::max<long long>(1, std::min<long long>((n + kBlock - 1) / kBlock, 8192));
}

// ----------------------------------------------------------------------------------
// Stage launchers: the kernel for the run-time (kernel id, map count, deterministic) on
// stream st, timed under the stage's StageMark.  The arrays are device pointers; the
// buffers of ws are sized by the driver (project2d_device) before the call.
// ----------------------------------------------------------------------------------
// asp_map_bin.hip
int launch_count(const Grid& g, const Src64& s, Workspace& ws, const Plan& pl, const float* u,
                 const float* v, const float* h, hipStream_t st);
// rec_cap / wide_cap: the capacities the kernel checks against the device counters (a
// speculative launch; see project2d_device).  probe: a launch of the placement trials.
// xa (asp_project2d_props): also write every record's coefficients of properties 2..5
// (two-map fp64 calls only).  verify: the layout in ws is an earlier call's; the kernel
// proves it exact for this call's particles or sets the counter word cLayoutBad.
int launch_scatter(const Grid& g, const Src64& s, Workspace& ws, const Plan& pl, int kid, int nout,
                   bool det, const float* u, const float* v, const float* h, const float* a0,
                   const float* a1, long long rec_cap, int wide_cap, hipStream_t st,
                   bool probe = false, const XArgs* xa = nullptr, bool verify = false);
// guard (here and in the deposit's launchers): the counter words behind a verifying
// scatter -- every kernel returns at once when the layout was rejected (layout_rejected) --
// or null.
int launch_tilescale(const Grid& g, Workspace& ws, const Plan& pl, int nout, hipStream_t st,
                     const int* guard = nullptr);
// asp_map_deposit.hip
// K4 / K4g / K5 / K6: the records in ws deposited into o0 (, o1) with their own two
// coefficients (a0 / a1: the properties' fp32 arrays, which the wide particles read
// directly).
int launch_deposit(const Grid& g, const Src64& s, Workspace& ws, const Plan& pl, int kid, int nout,
                   bool det, const float* u, const float* v, const float* h, const float* a0,
                   const float* a1, float* o0, float* o1, int dflags, hipStream_t st,
                   const int* guard = nullptr);
// The same for properties (2 pass, 2 pass + 1) of asp_project2d_props (pass = 1, 2), from
// the coefficients the scatter wrote beside each record (ws.ext); fp64 sums only.
int launch_deposit_props(const Grid& g, const Src64& s, Workspace& ws, const Plan& pl, int kid,
                         int nout, const float* u, const float* v, const float* h,
                         const float* a0, const float* a1, float* o0, float* o1, int dflags,
                         hipStream_t st, int pass);
int launch_ratio(float* o0, const float* o1, long long npix, hipStream_t st,
                 const int* guard = nullptr);  // no StageMark
// ASP_COUNT_EVALS: evals[0..2] += the deposit kernels' lane-slots (k_evals).
int launch_evals(const Grid& g, const Src64& s, Workspace& ws, const Plan& pl, int kid,
                 const float* u, const float* v, const float* h, unsigned long long* evals,
                 hipStream_t st);

// ----------------------------------------------------------------------------------
// asp_project2d.hip
// ----------------------------------------------------------------------------------
bool make_grid(double x_min, double x_max, double y_min, double y_max, int nx, int ny, int cs,
               Grid& g);
int setup_grid(const MapArgs& m, Grid& g);
int window_rows(const Grid& full);
Grid window_grid_rows(const Grid& full, int r0, int r1);
Grid window_grid(const Grid& full, int tx0, int tx1);
int decode_axis(int& axis, int& cull_axis);
Src64 src64_from_positions(const double* dpos, const double* dh, int axis, int cull_axis,
                           float* const* f);
int project2d_device(Workspace& ws, const Grid& gin, const Src64& s, const float* du,
                     const float* dv, const float* dh, const float* da0, const float* da1,
                     long long n, int kid, int flags, float* d0, float* d1, hipStream_t st,
                     int* bin_only = nullptr, const XArgs* xa = nullptr, int nxp = 0,
                     float* const* xo = nullptr, bool caller_arrays = false);

}  // namespace asp
