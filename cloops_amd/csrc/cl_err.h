// cl_err.h -- error plumbing of libcloops_hip.so (g_err lives in cloops_hip.hip): the last error's text per thread, and the return
// codes that go with it.  Needs only the HIP runtime API, so host code that includes it compiles without a device compiler.
#pragma once
#include <string>
#include <hip/hip_runtime_api.h>

#include "../../include/cloops_hip.h"

extern thread_local std::string g_err;

static inline int fail(int code, const char* what, const char* detail = nullptr)
{
    g_err = what;
    if (detail) { g_err += ": "; g_err += detail; }
    return code;
}

// "<who>: <what>[: detail]" -- for code that several entry points share: the text still names the one that was called
static inline int fail_at(int code, const char* who, const char* what, const char* detail = nullptr)
{
    g_err = who;
    g_err += ": "; g_err += what;
    if (detail) { g_err += ": "; g_err += detail; }
    return code;
}

#define HIP_TRY(expr)                                                             \
    do {                                                                           \
        hipError_t e_ = (expr);                                                    \
        if (e_ != hipSuccess) return fail(CL_ERR_HIP, #expr, hipGetErrorString(e_)); \
    } while (0)
