// asp_prims.hpp -- the two rocprim device primitives the library uses, each behind one
// function that asks rocprim for its scratch size, grows the workspace slot given for it
// and runs.  Included only by the units that sort or scan (asp_knn.hip, asp_nearest.hip,
// asp_match.hip, asp_profiles.hip and, through asp_sample.hpp, the two samplers): rocprim's
// headers are slow to compile.  Both are templates, so a unit instantiates the kernels of
// the one it calls and no others.
#pragma once

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "asp_host.hpp"

namespace asp {

// out[i] = in[0] + .. + in[i - 1] over n ints, on st.  in2 / out2: a second scan of the
// same length behind the first, in the same scratch.
template <class In>
inline int exclusive_scan_int(Buf& tmp, In in, int* out, size_t n, hipStream_t st,
                              In in2 = nullptr, int* out2 = nullptr) {
    size_t bytes = 0;
    ASP_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, 0, n, rocprim::plus<int>(), st));
    ASP_TRY(ensure(tmp, bytes));
    ASP_HIP(rocprim::exclusive_scan(tmp.p, bytes, in, out, 0, n, rocprim::plus<int>(), st));
    if (in2)
        ASP_HIP(rocprim::exclusive_scan(tmp.p, bytes, in2, out2, 0, n, rocprim::plus<int>(), st));
    return ASP_OK;
}

// (keys_in, vals_in) sorted by bits [0, end_bit) of the key into (keys_out, vals_out), on st.
template <class Key>
inline int sort_pairs(Buf& tmp, Key* keys_in, Key* keys_out, int* vals_in, int* vals_out, size_t n,
                      int end_bit, hipStream_t st) {
    size_t bytes = 0;
    ASP_HIP(rocprim::radix_sort_pairs(nullptr, bytes, keys_in, keys_out, vals_in, vals_out, n, 0,
                                      end_bit, st));
    ASP_TRY(ensure(tmp, bytes));
    ASP_HIP(rocprim::radix_sort_pairs(tmp.p, bytes, keys_in, keys_out, vals_in, vals_out, n, 0,
                                      end_bit, st));
    return ASP_OK;
}

}  // namespace asp
