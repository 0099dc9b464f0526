// asp_wave.hpp -- the wave-level device helpers every unit shares: the LDS hand-over between
// the lanes of one wave, and the inclusive scan over a wave's lanes.  Both are
// __forceinline__: a call compiles to what the hand-written lines did.
#pragma once

#include <hip/hip_runtime.h>

namespace asp {

// LDS written by lanes of the wave before the call is read by its other lanes after it
// (the workgroup's other waves are not ordered: that takes __syncthreads()).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Inclusive sum of v over lanes 0 .. lane of the wave (T = int or long long).  W < 64: over
// the first W lanes only, a power of two -- what the other lanes return is not a sum.
template <int W = 64, class T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < W; o <<= 1) {
        const T u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

}  // namespace asp
