// asp_match.hip -- cross-snapshot ID matching on the device (asp_match_ids) and the row
// gather that applies its result (asp_take_rows): the numerical core of the reference's
// tools/_ArrayReorder.py (ArrayReorder :815-1038, ArrayMapping :1042-1171), which matches
// two int64 ID orderings with argsort / isin / searchsorted and copies every field with a
// fancy index.  DESIGN.md §18.
//
// asp_match_ids is a partitioned hash join of 64-bit keys:
//   count    every filtered ID's partition (the top bits of a 64-bit finaliser of the ID),
//            both sides; index[] is set to -1 in the same pass;
//   scan     the partition counts (rocprim), per side;
//   scatter  (key, original position) records into partition order, both sides;
//   join     one workgroup per partition: the partition's source keys are staged into LDS in
//            chunks of kMChunk keys, inserted into an LDS table of int32 slots that hold the
//            key's position in the chunk, and probed by all the partition's targets.
// Equal partitions inside a wave are aggregated before the counter atomic (ballots per bit),
// so many copies of one ID cost one atomic per wave, not one per copy.  A partition larger
// than a chunk (skewed or repeated IDs) runs in rounds of one chunk each, every round probed
// by all its targets: no input overflows the table or takes another path.
//
// The table never holds a key: IDs are arbitrary int64, so there is no sentinel value, and a
// key stored after the slot's compare-and-swap would be visible too late to a concurrent
// inserter of an equal key.  A slot holds a chunk position r, claimed with
// atomicCAS(slot, EMPTY, r); equality is decided on keys[r], staged before the barrier.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/asp.h"
#include "asp_host.hpp"
#include "asp_prims.hpp"

namespace asp {

constexpr int kMBlock = 256;
constexpr int kMChunk = 4096;     // source keys per LDS round (ASP_MATCH_CHUNK_KEYS)
constexpr int kMChunkMin = 8;
constexpr int kMMaxBits = 24;     // at most 2^24 partitions
constexpr int kMEmpty = -1;

// LDS of the join for a chunk of K keys: K keys (8 B), 2K slots (4 B; load factor <= 1/2 in a
// full round, 1/4 on average), K "duplicated" and K "hit" bytes.
__host__ __device__ inline size_t match_lds_bytes(int K) { return (size_t)K * (8 + 8 + 2); }

// splitmix64's finaliser: every input bit reaches every output bit.
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}
// The partition: the hash's top `bits` bits (bits == 0: one partition).
__device__ __forceinline__ int part_of(unsigned long long h, int bits) {
    return bits ? (int)(h >> (64 - bits)) : 0;
}

// Lanes of the wave holding the same partition agree on one leader (the lowest such lane),
// which adds their number to the partition's counter: ONE atomic per distinct partition in
// the wave, all of them in one wave-instruction.  The groups are found bit by bit -- a ballot
// per partition bit, each lane keeping the lanes that agree with it -- so the cost is `bits`
// ballots whatever the number of distinct partitions.  Returns this lane's position in the
// partition (base + rank) -- or, with COUNT_ONLY, nothing.  Inactive lanes pass valid = false.
// Every lane of the wave must call this (ballots, shuffles).
template <bool COUNT_ONLY>
__device__ __forceinline__ int wave_claim(bool valid, int p, int bits, int* __restrict__ counter) {
    const int lane = (int)__lane_id();
    unsigned long long same = __ballot(valid);
    for (int b = 0; b < bits; ++b) {
        const bool bit = (p >> b) & 1;
        const unsigned long long m = __ballot(valid && bit);
        same &= bit ? m : ~m;
    }
    // (valid lanes: same = the valid lanes with this lane's partition, this lane included)
    const int leader = valid ? __ffsll((long long)same) - 1 : lane;
    int base = 0;
    if (valid && lane == leader) base = atomicAdd(&counter[p], __popcll(same));
    if (COUNT_ONLY) return 0;
    base = __shfl(base, leader);
    return base + __popcll(same & ((1ULL << lane) - 1ULL));
}

// count: cnt[partition] += 1 for every ID passing its filter.  fill: index[j] = -1 (the
// target side: dropped and unmatched targets keep it).
__global__ __launch_bounds__(kMBlock) void k_mcount(const long long* __restrict__ ids,
                                                    const unsigned char* __restrict__ filt,
                                                    long long n, int bits, int* __restrict__ cnt,
                                                    int* __restrict__ fill) {
    const long long stride = (long long)gridDim.x * kMBlock;
    // every lane of a wave runs the same number of iterations (wave_claim's ballots)
    const long long n_up = (n + kMBlock - 1) / kMBlock * kMBlock;
    for (long long i = (long long)blockIdx.x * kMBlock + threadIdx.x; i < n_up; i += stride) {
        const bool in = i < n;
        const bool ok = in && (!filt || filt[i] != 0);
        int p = 0;
        if (ok) p = part_of(mix64((unsigned long long)ids[i]), bits);
        if (in && fill) fill[i] = -1;
        wave_claim<true>(ok, p, bits, cnt);
    }
}

// scatter: the (key, original position) record of every filtered ID, in partition order.
__global__ __launch_bounds__(kMBlock) void k_mscatter(const long long* __restrict__ ids,
                                                      const unsigned char* __restrict__ filt,
                                                      long long n, int bits,
                                                      const int* __restrict__ start,
                                                      int* __restrict__ cursor,
                                                      long long* __restrict__ rkey,
                                                      int* __restrict__ ridx, int n_recs) {
    const long long stride = (long long)gridDim.x * kMBlock;
    const long long n_up = (n + kMBlock - 1) / kMBlock * kMBlock;
    for (long long i = (long long)blockIdx.x * kMBlock + threadIdx.x; i < n_up; i += stride) {
        const bool ok = i < n && (!filt || filt[i] != 0);
        int p = 0;
        long long id = 0;
        if (ok) {
            id = ids[i];
            p = part_of(mix64((unsigned long long)id), bits);
        }
        const int off = wave_claim<false>(ok, p, bits, cursor);
        if (ok) {
            const int at = start[p] + off;
            if (at >= 0 && at < n_recs) {  // (holds by construction: the counts of k_mcount)
                rkey[at] = id;
                ridx[at] = (int)i;
            }
        }
    }
}

// join: one workgroup per partition.  K = keys per round, TS = 2K slots (a power of two).
// ctr[0] += targets matched, ctr[1] += sources matched, ctr[2] += duplicates seen.
__global__ __launch_bounds__(kMBlock) void k_mjoin(const long long* __restrict__ skey,
                                                   const int* __restrict__ sidx,
                                                   const int* __restrict__ sstart,
                                                   const long long* __restrict__ tkey,
                                                   const int* __restrict__ tidx,
                                                   const int* __restrict__ tstart, int K,
                                                   int* __restrict__ index,
                                                   unsigned char* __restrict__ source_matched,
                                                   unsigned long long* __restrict__ ctr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int TS = 2 * K;
    long long* keys = (long long*)lds_raw;               // K
    int* tab = (int*)(lds_raw + (size_t)K * 8);          // TS
    unsigned char* dupf = lds_raw + (size_t)K * 16;      // K
    unsigned char* hitf = dupf + K;                      // K
    __shared__ unsigned wg_ctr[3];
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const int s0 = sstart[p], ns = sstart[p + 1] - s0;
    const int t0 = tstart[p], nt = tstart[p + 1] - t0;
    if (ns <= 0 || nt <= 0) return;  // nothing to match: index stays -1, no source is asked for
    if (tid < 3) wg_ctr[tid] = 0u;
    unsigned n_hit = 0, n_src = 0, n_dup = 0;
    const unsigned mask = (unsigned)TS - 1u;
    for (int base = 0; base < ns; base += K) {
        const int cnt = min(K, ns - base);
        for (int s = tid; s < TS; s += kMBlock) tab[s] = kMEmpty;
        for (int r = tid; r < K; r += kMBlock) {
            dupf[r] = 0;
            hitf[r] = 0;
            if (r < cnt) keys[r] = skey[s0 + base + r];
        }
        __syncthreads();
        // build
        for (int r = tid; r < cnt; r += kMBlock) {
            const long long k = keys[r];
            unsigned slot = (unsigned)mix64((unsigned long long)k) & mask;
            for (;;) {
                const int old = atomicCAS(&tab[slot], kMEmpty, r);
                if (old == kMEmpty) break;  // inserted
                if (keys[old] == k) {       // this key is present: a duplicated source ID
                    dupf[old] = 1;
                    break;
                }
                slot = (slot + 1u) & mask;  // (cnt <= K < TS: an empty slot exists)
            }
        }
        __syncthreads();
        // probe: every target of the partition, each by the same thread in every round
        for (int t = tid; t < nt; t += kMBlock) {
            const long long k = tkey[t0 + t];
            unsigned slot = (unsigned)mix64((unsigned long long)k) & mask;
            for (;;) {
                const int e = tab[slot];
                if (e == kMEmpty) break;
                if (keys[e] == k) {
                    const int j = tidx[t0 + t];
                    if (base > 0 && index[j] >= 0)
                        ++n_dup;  // matched in an earlier round too: duplicated across rounds
                    else
                        ++n_hit;
                    index[j] = sidx[s0 + base + e];
                    hitf[e] = 1;
                    if (dupf[e]) ++n_dup;
                    break;
                }
                slot = (slot + 1u) & mask;
            }
        }
        __syncthreads();
        for (int r = tid; r < cnt; r += kMBlock)
            if (hitf[r]) {
                ++n_src;
                if (source_matched) source_matched[sidx[s0 + base + r]] = 1;
            }
        __syncthreads();  // the next round clears the table and the flags
    }
    if (n_hit) atomicAdd(&wg_ctr[0], n_hit);
    if (n_src) atomicAdd(&wg_ctr[1], n_src);
    if (n_dup) atomicAdd(&wg_ctr[2], n_dup);
    __syncthreads();
    if (tid < 3 && wg_ctr[tid]) atomicAdd(&ctr[tid], (unsigned long long)wg_ctr[tid]);
}

__global__ __launch_bounds__(kMBlock) void k_mfill(int* __restrict__ a, long long n, int v) {
    const long long i = (long long)blockIdx.x * kMBlock + threadIdx.x;
    if (i < n) a[i] = v;
}

static unsigned match_grid(long long n) {
    // grid-stride kernels: enough workgroups to fill the chip, not one per 256 elements
    return (unsigned)std::max<long long>(1, std::min<long long>((n + kMBlock - 1) / kMBlock, 256 * 16));
}

static int match_ids(const long long* S, const unsigned char* sf, long long ns, const long long* T,
                     const unsigned char* tf, long long nt, int mode, int* index,
                     unsigned char* source_matched, long long* counts, int flags, int device,
                     hipStream_t st) {
    if (ns < 0) return fail(ASP_ERR_INVALID, "n_source < 0");
    if (nt < 0) return fail(ASP_ERR_INVALID, "n_target < 0");
    if (ns > 0 && !S) return fail(ASP_ERR_INVALID, "source_ids is NULL with n_source > 0");
    if (nt > 0 && !T) return fail(ASP_ERR_INVALID, "target_ids is NULL with n_target > 0");
    if (nt > 0 && !index) return fail(ASP_ERR_INVALID, "index is NULL with n_target > 0");
    if (!counts) return fail(ASP_ERR_INVALID, "counts is NULL");
    if (mode != ASP_MATCH_MAPPING && mode != ASP_MATCH_REORDER)
        return fail(ASP_ERR_INVALID, "mode must be ASP_MATCH_MAPPING (0) or ASP_MATCH_REORDER (1)");
    if (ns > 0x7fffffffLL) return fail(ASP_ERR_UNSUPPORTED, "n_source >= 2^31 IDs per call");
    if (nt > 0x7fffffffLL) return fail(ASP_ERR_UNSUPPORTED, "n_target >= 2^31 IDs per call");
    counts[0] = counts[1] = counts[2] = 0;
    if (nt == 0) return ASP_OK;
    const bool dev = flags & ASP_F_DEVICE_PTRS;
    if (ns == 0 && !dev) {  // nothing to match and nothing on the device
        std::fill(index, index + nt, -1);
        return ASP_OK;
    }
    return with_workspace(device, st, false, [&](Workspace& ws, hipStream_t st) -> int {
        if (ns == 0) {
            hipLaunchKernelGGL(k_mfill, dim3((unsigned)((nt + kMBlock - 1) / kMBlock)), dim3(kMBlock), 0, st,
                               index, nt, -1);
            ASP_LAUNCHED();
            return ASP_OK;
        }

        // ---- tuning: keys per round, partitions ----
        int K = (int)env_int("ASP_MATCH_CHUNK_KEYS", kMChunk, kMChunkMin, kMChunk);
        while (K & (K - 1)) K &= K - 1;  // a power of two (rounded down), so 2K slots mask cleanly
        int bits = 0;
        while (bits < kMMaxBits && ((long long)(K / 2) << bits) < ns) ++bits;  // ~K/2 keys each
        const long long P = 1LL << bits;
        // ASP_MATCH_STOP (diagnostic, tools/match_bench.py): 1 = return after the count and the
        // scans, 2 = after the scatter; the outputs are then meaningless.  Timing the three gives
        // the phases' times without events inside the call.
        const int stop = (int)env_int("ASP_MATCH_STOP", 3, 1, 3);

        // ---- inputs on the device ----
        const long long *dS = S, *dT = T;
        const unsigned char *dsf = sf, *dtf = tf;
        int* dindex = index;
        unsigned char* dmatched = source_matched;
        if (!dev) {
            // one slot each for the IDs, the filters and the outputs, sized for both sides
            // first: the source's part, then the target's
            Buf &ids = ws.match[kMatchIds], &filters = ws.match[kMatchFilters];
            ASP_TRY(ensure(ids, (size_t)(ns + nt) * 8));
            ASP_TRY(to_device(ws, ids, dS, (size_t)ns * 8, st, Copy::kPlain));
            ASP_TRY(to_device(ws, ids, dT, (size_t)nt * 8, st, Copy::kPlain, (size_t)ns * 8));
            ASP_TRY(ensure(filters, (size_t)(ns + nt)));
            if (sf) ASP_TRY(to_device(ws, filters, dsf, (size_t)ns, st, Copy::kPlain));
            if (tf) ASP_TRY(to_device(ws, filters, dtf, (size_t)nt, st, Copy::kPlain, (size_t)ns));
            ASP_TRY(ensure(ws.match[kMatchOutputs], (size_t)nt * 4 + (size_t)ns));
            ASP_TRY(device_scratch(ws.match[kMatchOutputs], dindex, (size_t)nt * 4));
            if (source_matched)
                ASP_TRY(device_scratch(ws.match[kMatchOutputs], dmatched, (size_t)ns, (size_t)nt * 4));
        }

        // ---- workspace: 2 x (P + 1) counts, 2 x (P + 1) starts, records (12 B per ID) ----
        ASP_TRY(ensure(ws.match[kMatchPartCount], (size_t)(P + 1) * 2 * sizeof(int)));
        ASP_TRY(ensure(ws.match[kMatchPartStart], (size_t)(P + 1) * 2 * sizeof(int)));
        ASP_TRY(ensure(ws.match[kMatchKeys], (size_t)(ns + nt) * 8));
        ASP_TRY(ensure(ws.match[kMatchPositions], (size_t)(ns + nt) * 4));
        ASP_TRY(ensure(ws.match[kMatchCounters], 4 * sizeof(unsigned long long)));
        int* scnt = (int*)ws.match[kMatchPartCount].p;
        int* tcnt = scnt + (P + 1);
        int* sstart = (int*)ws.match[kMatchPartStart].p;
        int* tstart = sstart + (P + 1);
        long long* skey = (long long*)ws.match[kMatchKeys].p;
        long long* tkey = skey + ns;
        int* sidx = (int*)ws.match[kMatchPositions].p;
        int* tidx = sidx + ns;
        unsigned long long* ctr = (unsigned long long*)ws.match[kMatchCounters].p;
        // the counters after the join, plus [3]: records per side (filtered IDs) are the scans' ends
        ASP_HIP(hipMemsetAsync(scnt, 0, (size_t)(P + 1) * 2 * sizeof(int), st));
        ASP_HIP(hipMemsetAsync(ctr, 0, 4 * sizeof(unsigned long long), st));
        if (dmatched) ASP_HIP(hipMemsetAsync(dmatched, 0, (size_t)ns, st));

        hipLaunchKernelGGL(k_mcount, dim3(match_grid(ns)), dim3(kMBlock), 0, st, dS, dsf, ns, bits, scnt,
                           (int*)nullptr);
        ASP_LAUNCHED();
        hipLaunchKernelGGL(k_mcount, dim3(match_grid(nt)), dim3(kMBlock), 0, st, dT, dtf, nt, bits, tcnt,
                           dindex);
        ASP_LAUNCHED();
        ASP_TRY(exclusive_scan_int(ws.match[kMatchScanTmp], scnt, sstart, (size_t)(P + 1), st, tcnt,
                                   tstart));
        ASP_HIP(hipMemsetAsync(scnt, 0, (size_t)(P + 1) * 2 * sizeof(int), st));  // now the cursors
        if (stop >= 2) {
            hipLaunchKernelGGL(k_mscatter, dim3(match_grid(ns)), dim3(kMBlock), 0, st, dS, dsf, ns, bits,
                               (const int*)sstart, scnt, skey, sidx, (int)ns);
            ASP_LAUNCHED();
            hipLaunchKernelGGL(k_mscatter, dim3(match_grid(nt)), dim3(kMBlock), 0, st, dT, dtf, nt, bits,
                               (const int*)tstart, tcnt, tkey, tidx, (int)nt);
            ASP_LAUNCHED();
        }

        const size_t lds = match_lds_bytes(K);
        ASP_TRY(allow_dyn_lds((const void*)k_mjoin, lds));
        if (stop >= 3) {
            hipLaunchKernelGGL(k_mjoin, dim3((unsigned)P), dim3(kMBlock), lds, st, (const long long*)skey,
                               (const int*)sidx, (const int*)sstart, (const long long*)tkey,
                               (const int*)tidx, (const int*)tstart, K, dindex, dmatched, ctr);
            ASP_LAUNCHED();
        }

        unsigned long long h[3] = {0, 0, 0};
        ASP_HIP(hipMemcpyAsync(h, ctr, sizeof(h), hipMemcpyDeviceToHost, st));
        if (!dev) {
            ASP_TRY(to_host(index, dindex, (size_t)nt * 4, st));
            if (source_matched) ASP_TRY(to_host(source_matched, dmatched, (size_t)ns, st));
        }
        ASP_HIP(hipStreamSynchronize(st));  // the counts decide the caller's exceptions
        for (int k = 0; k < 3; ++k) counts[k] = (long long)h[k];
        return ASP_OK;
    });
}

// ----------------------------------------------------------------------------------
// asp_take_rows: out[j] = data[index[j]], rows of W units of type U.  Every thread moves
// kTakeInFlight units per iteration, all loads issued before the first store: random rows
// are HBM-latency-bound, so several rows stay in flight per lane.
// ----------------------------------------------------------------------------------
constexpr int kTakeInFlight = 4;
typedef unsigned take16 __attribute__((ext_vector_type(4)));  // one 16-byte unit

template <class U, bool ONE>
__global__ __launch_bounds__(kMBlock) void k_take(const U* __restrict__ data, long long n_rows,
                                                  long long W, const int* __restrict__ index,
                                                  long long n_index, const U* __restrict__ fill,
                                                  U* __restrict__ out, int* __restrict__ bad) {
    const long long total = ONE ? n_index : n_index * W;
    const long long stride = (long long)gridDim.x * kMBlock;
    bool any_bad = false;
    for (long long e0 = (long long)blockIdx.x * kMBlock + threadIdx.x; e0 < total;
         e0 += stride * kTakeInFlight) {
        U v[kTakeInFlight];
        bool w[kTakeInFlight];
#pragma unroll
        for (int q = 0; q < kTakeInFlight; ++q) {
            const long long e = e0 + q * stride;
            w[q] = false;
            if (e < total) {
                const long long j = ONE ? e : e / W;
                const long long c = ONE ? 0 : e - j * W;
                const long long r = index[j];
                if (r >= n_rows) {
                    any_bad = true;  // reported, never dereferenced
                } else if (r >= 0) {
                    v[q] = data[(ONE ? r : r * W) + c];
                    w[q] = true;
                } else if (fill) {
                    v[q] = fill[c];
                    w[q] = true;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kTakeInFlight; ++q)
            if (w[q]) out[e0 + q * stride] = v[q];
    }
    if (any_bad) atomicOr(bad, 1);
}

template <class U>
static void launch_take(const void* data, long long n_rows, long long row_bytes, const int* index,
                        long long n_index, const void* fill, void* out, int* bad, hipStream_t st) {
    const long long W = row_bytes / (long long)sizeof(U);
    const long long total = n_index * W;
    const unsigned grid = (unsigned)std::max<long long>(
        1, std::min<long long>((total + kMBlock * kTakeInFlight - 1) / (kMBlock * kTakeInFlight),
                               256 * 32));
    if (W == 1)
        hipLaunchKernelGGL((k_take<U, true>), dim3(grid), dim3(kMBlock), 0, st, (const U*)data, n_rows,
                           W, index, n_index, (const U*)fill, (U*)out, bad);
    else
        hipLaunchKernelGGL((k_take<U, false>), dim3(grid), dim3(kMBlock), 0, st, (const U*)data, n_rows,
                           W, index, n_index, (const U*)fill, (U*)out, bad);
}

static int take_rows(const void* data, long long n_rows, long long row_bytes, const int* index,
                     long long n_index, const void* fill, void* out, int flags, int device,
                     hipStream_t st) {
    if (n_rows < 0) return fail(ASP_ERR_INVALID, "n_rows < 0");
    if (n_index < 0) return fail(ASP_ERR_INVALID, "n_index < 0");
    if (row_bytes < 1) return fail(ASP_ERR_INVALID, "row_bytes < 1");
    if (n_index > 0 && !out) return fail(ASP_ERR_INVALID, "out is NULL with n_index > 0");
    if (n_index > 0 && !index) return fail(ASP_ERR_INVALID, "index is NULL with n_index > 0");
    if (n_rows > 0 && !data) return fail(ASP_ERR_INVALID, "data is NULL with n_rows > 0");
    if (n_rows > 0x80000000LL) return fail(ASP_ERR_UNSUPPORTED, "n_rows > 2^31: index is int32");
    if (n_index == 0) return ASP_OK;
    return with_workspace(device, st, false, [&](Workspace& ws, hipStream_t st) -> int {
        const bool dev = flags & ASP_F_DEVICE_PTRS;
        const void *ddata = data, *dfill = fill;
        const int* dindex = index;
        void* dout = out;
        const size_t out_bytes = (size_t)n_index * (size_t)row_bytes;
        if (!dev) {
            const size_t rb16 = ((size_t)row_bytes + 15) / 16 * 16;
            ASP_TRY(to_device(ws, ws.match[kMatchRows], ddata, (size_t)n_rows * (size_t)row_bytes, st,
                              Copy::kPlain));
            // one slot: the fill row first (16-byte slot), then the output
            Buf& rows_out = ws.match[kMatchRowsOut];
            ASP_TRY(device_scratch(rows_out, dout, out_bytes, rb16));
            ASP_TRY(to_device(ws, ws.match[kMatchRowIndex], dindex, (size_t)n_index * 4, st,
                              Copy::kPlain));
            if (fill) {
                ASP_TRY(to_device(ws, rows_out, dfill, (size_t)row_bytes, st, Copy::kPlain));
            } else {  // unmatched rows keep the caller's bytes
                ASP_HIP(hipMemcpyAsync(dout, out, out_bytes, hipMemcpyHostToDevice, st));
            }
        }
        ASP_TRY(ensure(ws.match[kMatchCounters], 4 * sizeof(unsigned long long)));
        int* bad = (int*)ws.match[kMatchCounters].p;
        ASP_HIP(hipMemsetAsync(bad, 0, sizeof(int), st));
        // the widest unit that divides the row and that every pointer is aligned to
        const uintptr_t al = (uintptr_t)ddata | (uintptr_t)dout | (uintptr_t)dfill | (uintptr_t)row_bytes;
        if (al % 16 == 0)
            launch_take<take16>(ddata, n_rows, row_bytes, dindex, n_index, dfill, dout, bad, st);
        else if (al % 8 == 0)
            launch_take<uint2>(ddata, n_rows, row_bytes, dindex, n_index, dfill, dout, bad, st);
        else if (al % 4 == 0)
            launch_take<unsigned>(ddata, n_rows, row_bytes, dindex, n_index, dfill, dout, bad, st);
        else
            launch_take<unsigned char>(ddata, n_rows, row_bytes, dindex, n_index, dfill, dout, bad, st);
        ASP_LAUNCHED();
        int h_bad = 0;
        ASP_HIP(hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
        ASP_HIP(hipStreamSynchronize(st));
        if (h_bad) return fail(ASP_ERR_INVALID, "an index is >= n_rows");
        if (!dev) {
            ASP_TRY(to_host(out, dout, out_bytes, st));
            ASP_HIP(hipStreamSynchronize(st));
        }
        return ASP_OK;
    });
}

}  // namespace asp

using namespace asp;

extern "C" int asp_match_ids(const int64_t* source_ids, const uint8_t* source_filter,
                             int64_t n_source, const int64_t* target_ids,
                             const uint8_t* target_filter, int64_t n_target, int32_t mode,
                             int32_t* index, uint8_t* source_matched, int64_t* counts,
                             int32_t flags, int32_t device, void* stream) {
    t_err.clear();
    static_assert(sizeof(long long) == sizeof(int64_t), "int64_t is long long wide");
    return match_ids((const long long*)source_ids, source_filter, n_source,
                     (const long long*)target_ids, target_filter, n_target, mode, index,
                     source_matched, (long long*)counts, flags, device, (hipStream_t)stream);
}

extern "C" int asp_take_rows(const void* data, int64_t n_rows, int64_t row_bytes,
                             const int32_t* index, int64_t n_index, const void* fill_row, void* out,
                             int32_t flags, int32_t device, void* stream) {
    t_err.clear();
    return take_rows(data, n_rows, row_bytes, index, n_index, fill_row, out, flags, device,
                     (hipStream_t)stream);
}
