// abi_util.h -- what the two extern "C" files (abi.cpp: the stateless entries, profiler.cpp: the
// nvrx_profiler handle) share: HIP error -> status code + the thread-local message of
// nvrx_last_error (one object, in abi.cpp), and the argument checks both use.
#pragma once
#include <string>

#include "nvrx_internal.h"

namespace nvrx {

int fail(int code, const std::string& msg);  // sets the message, returns code
int hip_status(hipError_t e, const char* where);
// the quantile requests of nvrx_*_quantiles*: a host array of 1..NVRX_MAX_QUANTILES permilles
int check_permille(const char* fn, const int32_t* permille, int32_t nq);

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

}  // namespace nvrx

#define NVRX_CHECK_ARG(cond, msg) \
    do {                          \
        if (!(cond)) return nvrx::fail(NVRX_ERR_INVALID, msg); \
    } while (0)
