// kind_switch.h -- THE dispatch on a segment's kind: the only `switch` over CFMM_KIND_* of the query code, host and device.
// with_kind(kind, f, none) calls f(std::integral_constant<int, KIND>{}) for the kind it is given -- the callable is generic
// (`[&](auto K) { ... <decltype(K)::value> ... }`), so every case instantiates it with its own constant -- and none() for a
// number that names no kind (a segment without pools has kind -1).  A new pool kind is one line here.
// The function returns nothing and initialises nothing: a caller that wants a result declares it uninitialised in front of the
// call and assigns it in both callables, which is the statement shape of a hand-written switch and compiles to its code.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/cfmm_amd.h"

namespace cfmm {

template <class F, class None>
__host__ __device__ __forceinline__ void with_kind(int kind, F&& f, None&& none)
{
    switch (kind) {
    case CFMM_KIND_PRODUCT: f(std::integral_constant<int, CFMM_KIND_PRODUCT>{}); break;
    case CFMM_KIND_GEOMEAN: f(std::integral_constant<int, CFMM_KIND_GEOMEAN>{}); break;
    case CFMM_KIND_UNIV3: f(std::integral_constant<int, CFMM_KIND_UNIV3>{}); break;
    case CFMM_KIND_WEIGHTED: f(std::integral_constant<int, CFMM_KIND_WEIGHTED>{}); break;
    case CFMM_KIND_CURVE: f(std::integral_constant<int, CFMM_KIND_CURVE>{}); break;
    case CFMM_KIND_SOLIDLY: f(std::integral_constant<int, CFMM_KIND_SOLIDLY>{}); break;
    default: none(); break;
    }
}

} // namespace cfmm
