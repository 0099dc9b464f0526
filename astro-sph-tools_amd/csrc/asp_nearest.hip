// asp_nearest.hip -- nearest halo centre of every particle in a periodic box.
//
// Replaces the scipy KDTree query of the reference's _scripts/find_nearest_haloes.py:196-221:
// per minimum-halo-mass cut, KDTree(halo_centres[mask], boxsize=L).query(positions).  The
// arithmetic is scipy's for a periodic box, fp64, no contraction (asp.h has the definition),
// so the distances are bit-identical; the index is the centre's position in the caller's
// array, exact ties in d2 going to the lowest position.
//
// MI355X layout.  The centres are small (10^5-10^6, they stay in L2 / Infinity Cache); the
// query stream (10^8 rows) is the cost.
//   prep (per call): one reduction validates the centres and counts each set's members; each
//     set gets a cubic grid of G cells per axis over [0, L) (about kPerCell members per
//     cell; G = 1 for a set of at most kSmallSet members); the members are counting-sorted
//     by cell into 32-byte entries (x, y, z, original index) with one cell-start table over
//     all sets (a lane gathers whole cells, so an entry is one 32-byte segment, not four
//     words of four arrays).
//   search (k_nearest): one lane per query.  The position is read and wrapped once; the
//     sets are the outer loop, so one running (best d2, best index) pair is live at a time.
//     Within a set the lane walks shells of cells of periodic Chebyshev index distance
//     r = 0, 1, 2, ... around its own cell, skipping cells that cannot hold the nearest
//     (nearest_walk has the pruning and termination arguments).  A set with G = 1 is
//     staged through LDS per workgroup, every lane testing every entry.  Outputs are
//     set-major: contiguous in the query index, coalesced stores.
//   query order: the query indices of a batch are sorted by the Morton key of their cell
//     (rocPRIM radix sort) so that the lanes of a wave walk the same cells; results are
//     scattered back to input order.  ASP_NEAREST_SORT=0 searches in the caller's order
//     (1.07-6.6 times slower on a random-order input, DESIGN.md §17 has the A/B).
#include <hip/hip_runtime.h>


#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/asp.h"
#include "asp_host.hpp"
#include "asp_periodic.hpp"
#include "asp_prims.hpp"

namespace asp {

constexpr int kNBlock = 256;
constexpr int kMaxSets = 8;
constexpr int kPerCell = 2;      // members per cell the grid aims at
constexpr int kSmallSet = 64;    // sets up to this size: G = 1, staged through LDS
constexpr int kMaxG = 256;       // cells per axis at most (8-bit cell coordinates)
constexpr long long kNBatch = 1LL << 26;  // queries per launch (and per staged host piece)
constexpr int kSortQueries = 1;  // the default query order (DESIGN.md has the A/B)

// One centre of one set, in cell order.
struct __attribute__((aligned(32))) NEnt {
    double x, y, z;
    int idx;  // position in the caller's centres array
    int pad;
};
static_assert(sizeof(NEnt) == 32, "one 32-byte segment per entry");

struct NSet {
    int G;       // cells per axis (0: the set is empty)
    int M;       // members
    int cell0;   // the set's first cell in the cell-start table
    int first;   // the set's first entry (= start[cell0])
    double h;    // cell edge L / G
};
struct NTab {
    NSet s[kMaxSets];
    double L, halfL;
};

// Lexicographic (d2, original index): ties in d2 go to the lowest index, whatever the order
// the entries are met in (the counting sort's order within a cell is not deterministic).
__device__ __forceinline__ void take(double d2, int idx, double& best, int& bi) {
    if (d2 < best || (d2 == best && idx < bi)) {
        best = d2;
        bi = idx;
    }
}

// cnt[0] |= the centre_bits() of every centre; cnt[1 + s] += the members of set s.
__global__ __launch_bounds__(kNBlock) void k_ncheck(const double* __restrict__ c, long long m,
                                                     const unsigned* __restrict__ member,
                                                     int nsets, double L, int* __restrict__ cnt) {
    const long long j = (long long)blockIdx.x * kNBlock + threadIdx.x;
    int bad = 0;
    unsigned bits = 0;
    if (j < m) {
        bad = centre_bits(c, j, L);
        bits = member ? member[j] : 1u;
    }
    if (bad) atomicOr(&cnt[0], bad);
    for (int s = 0; s < nsets; ++s) {
        const unsigned long long b = __builtin_amdgcn_ballot_w64((bits >> s) & 1u);
        if (b && (threadIdx.x & 63) == 0) atomicAdd(&cnt[1 + s], __popcll(b));
    }
}

// Counting sort of the members by cell, pass 1: cnt[cell0_s + cell] += 1.
__global__ __launch_bounds__(kNBlock) void k_ncount(const double* __restrict__ c, long long m,
                                                     const unsigned* __restrict__ member,
                                                     int nsets, NTab T, int* __restrict__ cnt) {
    const long long j = (long long)blockIdx.x * kNBlock + threadIdx.x;
    if (j >= m) return;
    const unsigned bits = member ? member[j] : 1u;
    const double x = c[3 * j], y = c[3 * j + 1], z = c[3 * j + 2];
    for (int s = 0; s < nsets; ++s) {
        if (!((bits >> s) & 1u)) continue;
        const int G = T.s[s].G;
        const int cell = (cell_of(x, G, T.L) * G + cell_of(y, G, T.L)) * G + cell_of(z, G, T.L);
        atomicAdd(&cnt[T.s[s].cell0 + cell], 1);
    }
}

// Pass 2: each member takes the next slot of its cell (cur zeroed; start = the exclusive
// scan of the counts).
__global__ __launch_bounds__(kNBlock) void k_nfill(const double* __restrict__ c, long long m,
                                                    const unsigned* __restrict__ member,
                                                    int nsets, NTab T, const int* __restrict__ start,
                                                    int* __restrict__ cur, NEnt* __restrict__ ent) {
    const long long j = (long long)blockIdx.x * kNBlock + threadIdx.x;
    if (j >= m) return;
    const unsigned bits = member ? member[j] : 1u;
    const double x = c[3 * j], y = c[3 * j + 1], z = c[3 * j + 2];
    for (int s = 0; s < nsets; ++s) {
        if (!((bits >> s) & 1u)) continue;
        const int G = T.s[s].G;
        const int cell = T.s[s].cell0 +
                         (cell_of(x, G, T.L) * G + cell_of(y, G, T.L)) * G + cell_of(z, G, T.L);
        const int p = start[cell] + atomicAdd(&cur[cell], 1);
        ent[p] = NEnt{x, y, z, (int)j, 0};
    }
}

__device__ __forceinline__ unsigned spread8(unsigned v) {  // 8 bits -> every third bit
    v &= 0xffu;
    v = (v | v << 8) & 0x00f00fu;
    v = (v | v << 4) & 0x0c30c3u;
    v = (v | v << 2) & 0x249249u;
    return v;
}

// Sort key of a query: the Morton code of its cell on a G^3 grid (G <= 256); rows with a
// non-finite coordinate get key 0 (they walk nothing).
__global__ __launch_bounds__(kNBlock) void k_nkeys(const double* __restrict__ pos, long long n, int G,
                                                    double L, unsigned* __restrict__ keys,
                                                    int* __restrict__ idx) {
    const long long i = (long long)blockIdx.x * kNBlock + threadIdx.x;
    if (i >= n) return;
    const double x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
    unsigned k = 0;
    if (__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z))
        k = spread8(cell_of(wrap_box(x, L), G, L)) << 2 | spread8(cell_of(wrap_box(y, L), G, L)) << 1 |
            spread8(cell_of(wrap_box(z, L), G, L));
    keys[i] = k;
    idx[i] = (int)i;
}

// One lane's search of one gridded set (G >= 2).
//
// Shell r is the set of cells whose periodic Chebyshev index distance from the query's cell
// is r.  Per axis the offsets of shells 0..r are [-r, hi], hi = min(r, G - 1 - r): while
// 2r + 1 <= G that is [-r, r]; in the last shell of an even G (2r + 1 = G + 1) the offsets
// -r and +r name the same cell, so +r is left out and no cell is visited twice.  Shell r is
// then (offsets of 0..r)^3 minus (offsets of 0..r-1)^3: a triple has a NEW offset (-r, or +r
// when hi = r) on at least one axis.
//
// Geometry.  Cells come from cell_of(), the same monotone expression for queries and
// centres, so cell k of an axis is an interval [b_k, b_k+1) with b_k = k h, h = L / G, up to
// a few ulp of L (~2^-50 L).  fl and fu are the query's distances to the lower and upper
// face of its own cell.  A centre in the cell at offset o != 0 of an axis has at least
// |o| - 1 whole cells and fl (o < 0) or fu (o > 0) between itself and the query, so its
// periodic separation on that axis is at least  g(o) = (fl or fu) + (|o| - 1) h  less those
// few ulp -- the other way round the box is no shorter while 2r + 1 <= G (it crosses at
// least G - |o| - 1 >= |o| cells, and g(o) <= |o| h) -- and the folded difference the
// distance is built from equals that separation up to one more rounding.  Every bound below
// is reduced by eps = face_margin(h), far more than the rounding (asp_periodic.hpp), so
// "bound^2 > best" proves that the COMPUTED d2 of every centre concerned exceeds best.
//
// Pruning (prune != 0, shells with 2r + 1 <= G only): a cell is skipped when the sum over the
// axes of max(0, g(o) - eps)^2 is STRICTLY above best -- none of its centres can beat best or
// tie it.  Whole rows and planes of a shell go the same way.
//
// Termination.  After shells 0..r are complete, an unvisited cell has |o| >= r + 1 on some
// axis, so its centres are farther than  r h + min(fl, fu over the axes)  on that axis.  The
// walk stops only when best is STRICTLY below the square of that bound, reduced by eps and by
// 2^-20 relative (the rounding of r h): an unvisited centre can then neither beat the best
// nor tie it (a tie with a lower index would change the answer).  It also stops when
// 2r + 1 >= G: every cell is in.
template <bool COUNT>
__device__ __forceinline__ void nearest_walk(const NSet S, double L, double halfL, double wx,
                                             double wy, double wz, const NEnt* __restrict__ ent,
                                             const int* __restrict__ start, int prune, double& best,
                                             int& bi, unsigned& evals) {
    const int G = S.G;
    const double h = S.h, eps = face_margin(h);
    const int qx = cell_of(wx, G, L), qy = cell_of(wy, G, L), qz = cell_of(wz, G, L);
    const double flx = wx - (double)qx * h, fux = (double)(qx + 1) * h - wx;
    const double fly = wy - (double)qy * h, fuy = (double)(qy + 1) * h - wy;
    const double flz = wz - (double)qz * h, fuz = (double)(qz + 1) * h - wz;
    const double face = fmin(fmin(fmin(flx, fux), fmin(fly, fuy)), fmin(flz, fuz));
    const int* __restrict__ st = start + S.cell0;
    auto wrapc = [G](int c) { return c < 0 ? c + G : (c >= G ? c - G : c); };  // |offset| < G
    // max(0, g(o) - eps)^2
    auto lb2 = [h, eps](double fl, double fu, int o) {
        if (o == 0) return 0.0;
        const double g = (o < 0 ? fl + (double)(-o - 1) * h : fu + (double)(o - 1) * h) - eps;
        return g > 0.0 ? g * g : 0.0;
    };
    auto scan = [&](int cell) {
        const int a = st[cell], b = st[cell + 1];
        for (int j = a; j < b; ++j) {
            const NEnt e = ent[j];
            take(pdist2(wx, wy, wz, e.x, e.y, e.z, L, halfL), e.idx, best, bi);
        }
        if (COUNT) evals += (unsigned)(b - a);
    };
    for (int r = 0;; ++r) {
        const int hi = min(r, G - 1 - r);
        const bool pr = prune && 2 * r + 1 <= G;
        for (int ox = -r; ox <= hi; ++ox) {
            const double px = pr ? lb2(flx, fux, ox) : 0.0;
            if (px > best) continue;
            const bool nx = ox == -r || ox == r;
            const int cx = wrapc(qx + ox) * G;
            for (int oy = -r; oy <= hi; ++oy) {
                const double pxy = px + (pr ? lb2(fly, fuy, oy) : 0.0);
                if (pxy > best) continue;
                const int cxy = (cx + wrapc(qy + oy)) * G;
                if (nx || oy == -r || oy == r) {
                    for (int oz = -r; oz <= hi; ++oz)
                        if (!(pxy + (pr ? lb2(flz, fuz, oz) : 0.0) > best)) scan(cxy + wrapc(qz + oz));
                } else {  // r >= 1 here: only the new offsets of the last axis
                    if (!(pxy + (pr ? lb2(flz, fuz, -r) : 0.0) > best)) scan(cxy + wrapc(qz - r));
                    if (hi == r && !(pxy + (pr ? lb2(flz, fuz, r) : 0.0) > best))
                        scan(cxy + wrapc(qz + r));
                }
            }
        }
        if (2 * r + 1 >= G) break;
        const double bound = ((double)r * h + face) * (1.0 - 0x1p-20) - eps;
        if (bound > 0.0 && best < bound * bound) break;
    }
}

// One lane per query.  q = order ? order[i] : i is the query's row in pos and its column in
// the (nsets, ostride) outputs.
template <bool COUNT>
__global__ __launch_bounds__(kNBlock) void k_nearest(const double* __restrict__ pos, long long n,
                                                      const int* __restrict__ order, const NTab T,
                                                      int nsets, const NEnt* __restrict__ ent,
                                                      const int* __restrict__ start,
                                                      int* __restrict__ index,
                                                      double* __restrict__ distance,
                                                      long long ostride, int prune,
                                                      unsigned long long* __restrict__ evc) {
    __shared__ NEnt lds[kNBlock];
    const long long i = (long long)blockIdx.x * kNBlock + threadIdx.x;
    const bool act = i < n;  // (no early return: the LDS path has workgroup barriers)
    const long long q = act ? (order ? (long long)order[i] : i) : 0;
    const double L = T.L, halfL = T.halfL;
    double wx = 0.0, wy = 0.0, wz = 0.0;
    bool fin = false;
    if (act) {
        const double x = pos[3 * q], y = pos[3 * q + 1], z = pos[3 * q + 2];
        fin = __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
        if (fin) {
            wx = wrap_box(x, L);
            wy = wrap_box(y, L);
            wz = wrap_box(z, L);
        }
    }
    unsigned evals = 0;
    for (int s = 0; s < nsets; ++s) {
        const NSet S = T.s[s];  // uniform over the grid
        double best = INFINITY;
        int bi = INT_MAX;
        if (S.G == 1) {
            // every lane needs every entry: chunks of kNBlock entries through LDS
            for (int c0 = 0; c0 < S.M; c0 += kNBlock) {
                const int cnt = min(kNBlock, S.M - c0);
                if ((int)threadIdx.x < cnt) lds[threadIdx.x] = ent[S.first + c0 + threadIdx.x];
                __syncthreads();
                if (fin) {
                    for (int j = 0; j < cnt; ++j)
                        take(pdist2(wx, wy, wz, lds[j].x, lds[j].y, lds[j].z, L, halfL), lds[j].idx,
                             best, bi);
                    if (COUNT) evals += (unsigned)cnt;
                }
                __syncthreads();  // the chunk is rewritten next
            }
        } else if (S.G > 1 && fin) {
            nearest_walk<COUNT>(S, L, halfL, wx, wy, wz, ent, start, prune, best, bi, evals);
        }
        if (act) {
            // an empty set: -1 / +inf; a non-finite query: -1 / NaN
            index[(long long)s * ostride + q] = bi == INT_MAX ? -1 : bi;
            distance[(long long)s * ostride + q] = fin ? sqrt(best) : __builtin_nan("");
        }
    }
    if (COUNT && evals) atomicAdd(evc, (unsigned long long)evals);
}

static int nearest(const double* pos, long long n, const double* centres, long long m,
                   const unsigned* member, int nsets, double L, int* index, double* distance,
                   int flags, int device, hipStream_t st) {
    if (!(L > 0.0) || !std::isfinite(L))
        return fail(ASP_ERR_INVALID, "box_width must be finite and > 0");
    if (nsets < 1 || nsets > kMaxSets) return fail(ASP_ERR_INVALID, "nsets must be in [1, 8]");
    if (!member && nsets > 1) return fail(ASP_ERR_INVALID, "member is NULL with nsets > 1");
    if (n < 0) return fail(ASP_ERR_INVALID, "n < 0");
    if (m < 0) return fail(ASP_ERR_INVALID, "m < 0");
    if (n > 0 && (!pos || !index || !distance)) return fail(ASP_ERR_INVALID, "NULL array");
    if (m > 0 && !centres) return fail(ASP_ERR_INVALID, "NULL centres");
    if (m > 0x7fffffffLL) return fail(ASP_ERR_UNSUPPORTED, "m >= 2^31 centres per call");
    if (n == 0) return ASP_OK;
    return with_workspace(device, st, false, [&](Workspace& ws, hipStream_t st) -> int {
        const bool dev = flags & ASP_F_DEVICE_PTRS;
        if (ws.prof) ASP_TRY(prof_next(ws));
        stats_clear(ws);

        // ---- prep: the centres on the device, validated, counted, sorted by cell per set ----
        StageMark mprep(ws, kSNearestPrep, st);
        const double* dc = centres;
        const unsigned* dm = member;
        if (!dev && m > 0) {
            ASP_TRY(to_device(ws, ws.nearest[kNearCentres], dc, (size_t)m * 3 * sizeof(double), st,
                              Copy::kPlain));
            if (member)
                ASP_TRY(to_device(ws, ws.nearest[kNearMembers], dm, (size_t)m * sizeof(unsigned), st,
                                  Copy::kPlain));
        }
        const unsigned cgrid = (unsigned)((m + kNBlock - 1) / kNBlock);
        int h[1 + kMaxSets] = {0};
        if (m > 0) {
            ASP_TRY(ensure(ws.nearest[kNearCheck], sizeof(h)));
            int* dcnt = (int*)ws.nearest[kNearCheck].p;
            ASP_HIP(hipMemsetAsync(dcnt, 0, sizeof(h), st));
            hipLaunchKernelGGL(k_ncheck, dim3(cgrid), dim3(kNBlock), 0, st, dc, (long long)m, dm, nsets,
                               L, dcnt);
            ASP_LAUNCHED();
            ASP_HIP(hipMemcpyAsync(h, dcnt, sizeof(h), hipMemcpyDeviceToHost, st));
            ASP_HIP(hipStreamSynchronize(st));
        }
        ASP_TRY(centre_error(h[0]));
        const int small = (int)env_int("ASP_NEAREST_SMALL", kSmallSet, 0, 1 << 20);  // (tests raise it)
        NTab T;
        T.L = L;
        T.halfL = 0.5 * L;
        long long ncell = 0, nent = 0;
        int gmax = 1;
        for (int s = 0; s < kMaxSets; ++s) {
            NSet& S = T.s[s];
            S.M = s < nsets ? h[1 + s] : 0;
            S.G = 0;
            S.cell0 = (int)ncell;
            S.first = (int)nent;
            S.h = 0.0;
            if (S.M == 0) continue;
            S.G = S.M <= small ? 1
                               : std::max(2, std::min(kMaxG, (int)std::floor(std::cbrt((double)S.M / kPerCell))));
            S.h = L / (double)S.G;
            ncell += (long long)S.G * S.G * S.G;
            nent += S.M;
            gmax = std::max(gmax, S.G);
            if (nent > 0x7fffffffLL)
                return fail(ASP_ERR_UNSUPPORTED, ">= 2^31 set members over all sets");
        }
        // (counts, then cursors)
        ASP_TRY(ensure(ws.nearest[kNearCellCount], (size_t)(ncell + 1) * sizeof(int)));
        ASP_TRY(ensure(ws.nearest[kNearCellStart], (size_t)(ncell + 1) * sizeof(int)));  // cell starts
        ASP_TRY(ensure(ws.nearest[kNearEntries], (size_t)nent * sizeof(NEnt)));
        int* cnt = (int*)ws.nearest[kNearCellCount].p;
        int* start = (int*)ws.nearest[kNearCellStart].p;
        NEnt* ent = (NEnt*)ws.nearest[kNearEntries].p;
        if (nent > 0) {
            ASP_HIP(hipMemsetAsync(cnt, 0, (size_t)(ncell + 1) * sizeof(int), st));
            hipLaunchKernelGGL(k_ncount, dim3(cgrid), dim3(kNBlock), 0, st, dc, (long long)m, dm, nsets, T,
                               cnt);
            ASP_LAUNCHED();
            ASP_TRY(exclusive_scan_int(ws.nearest[kNearScanTmp], cnt, start, (size_t)(ncell + 1), st));
            ASP_HIP(hipMemsetAsync(cnt, 0, (size_t)(ncell + 1) * sizeof(int), st));
            hipLaunchKernelGGL(k_nfill, dim3(cgrid), dim3(kNBlock), 0, st, dc, (long long)m, dm, nsets, T,
                               (const int*)start, cnt, ent);
            ASP_LAUNCHED();
        }
        mprep.done();

        // ---- search, in batches of queries ----
        // ASP_NEAREST_COUNT: count the distances evaluated (one atomic per lane, so off in timed
        // runs) -> asp_last_stats[9]
        DiagCounter evals;
        ASP_TRY(evals.begin("ASP_NEAREST_COUNT", ws.nearest[kNearCounter], st));
        unsigned long long* const evc = evals.p;
        // ASP_NEAREST_SORT (read per call, so one process can time both): 1 = the queries of a
        // batch are searched in the order of their cell key, 0 = in the caller's order
        const bool sorted = env_int("ASP_NEAREST_SORT", kSortQueries) != 0;
        // ASP_NEAREST_PRUNE=0: every cell of every shell is scanned (diagnostic; same results)
        const int prune = env_int("ASP_NEAREST_PRUNE", 1) != 0;
        const long long B = std::min(n, (long long)env_int("ASP_NEAREST_BATCH", kNBatch, 1, kNBatch));
        // a batch's outputs share a slot: B * nsets distances, then as many indices
        const size_t dist_bytes = (size_t)B * nsets * sizeof(double);
        if (!dev) {  // (both up front, in this order: where the slots land is part of the speed)
            ASP_TRY(ensure(ws.nearest[kNearQueries], (size_t)B * 3 * sizeof(double)));
            ASP_TRY(ensure(ws.nearest[kNearOutputs], dist_bytes + (size_t)B * nsets * sizeof(int)));
        }
        unsigned *kin = nullptr, *kout = nullptr;
        int *iin = nullptr, *iout = nullptr;
        int key_bits = 3;
        while ((1 << (key_bits / 3)) < gmax) key_bits += 3;
        if (sorted) {
            ASP_TRY(ensure(ws.nearest[kNearSortKeys], (size_t)B * 2 * sizeof(unsigned)));
            ASP_TRY(ensure(ws.nearest[kNearSortIndex], (size_t)B * 2 * sizeof(int)));
            kin = (unsigned*)ws.nearest[kNearSortKeys].p;
            kout = kin + B;
            iin = (int*)ws.nearest[kNearSortIndex].p;
            iout = iin + B;
        }
        for (long long a = 0; a < n; a += B) {
            const long long nb = std::min(B, n - a);
            const unsigned grid = (unsigned)((nb + kNBlock - 1) / kNBlock);
            const double* dpos = pos + 3 * a;
            int* dindex = index + a;
            double* ddist = distance + a;
            long long ostride = n;
            if (!dev) {
                ASP_TRY(to_device(ws, ws.nearest[kNearQueries], dpos, (size_t)nb * 3 * sizeof(double),
                                  st, Copy::kPlain));
                ASP_TRY(device_scratch(ws.nearest[kNearOutputs], ddist, dist_bytes));
                ASP_TRY(device_scratch(ws.nearest[kNearOutputs], dindex, (size_t)B * nsets * sizeof(int),
                                       dist_bytes));
                ostride = B;
            }
            StageMark msearch(ws, kSNearestSearch, st);  // (with the query sort, when it is on)
            if (sorted) {
                hipLaunchKernelGGL(k_nkeys, dim3(grid), dim3(kNBlock), 0, st, dpos, nb, gmax, L, kin, iin);
                ASP_LAUNCHED();
                ASP_TRY(sort_pairs(ws.nearest[kNearSortTmp], kin, kout, iin, iout, (size_t)nb, key_bits,
                                   st));
            }
            if (evc)
                hipLaunchKernelGGL(k_nearest<true>, dim3(grid), dim3(kNBlock), 0, st, dpos, nb,
                                   (const int*)iout, T, nsets, (const NEnt*)ent, (const int*)start, dindex,
                                   ddist, ostride, prune, evc);
            else
                hipLaunchKernelGGL(k_nearest<false>, dim3(grid), dim3(kNBlock), 0, st, dpos, nb,
                                   (const int*)iout, T, nsets, (const NEnt*)ent, (const int*)start, dindex,
                                   ddist, ostride, prune, evc);
            ASP_LAUNCHED();
            msearch.done();
            if (!dev)
                for (int s = 0; s < nsets; ++s) {
                    ASP_TRY(to_host(index + (size_t)s * n + a, dindex + (size_t)s * B,
                                    (size_t)nb * sizeof(int), st));
                    ASP_TRY(to_host(distance + (size_t)s * n + a, ddist + (size_t)s * B,
                                    (size_t)nb * sizeof(double), st));
                }
        }
        ASP_TRY(evals.end(ws, st));
        if (!dev) ASP_HIP(hipStreamSynchronize(st));
        stats_publish(ws, device);
        return ASP_OK;
    });
}

}  // namespace asp

using namespace asp;

extern "C" int asp_nearest(const double* positions, int64_t n, const double* centres, int64_t m,
                           const uint32_t* member, int32_t nsets, double box_width,
                           int32_t* index, double* distance, int32_t flags, int32_t device,
                           void* stream) {
    t_err.clear();
    return nearest(positions, n, centres, m, member, nsets, box_width, index, distance, flags,
                   device, (hipStream_t)stream);
}
