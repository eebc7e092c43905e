// cl_prim.h -- host side shared by the translation units: the device buffer every handle is made of, and the one way a rocPRIM
// primitive is called on temporary storage that such a buffer holds.
#pragma once
#include "cl_common.h"

struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    bool fresh = false;               // (re)allocated since the flag was last cleared
    bool owned = true;                // false: a slice of the handle's arena (never freed on its own)
    int ensure(size_t need)
    {
        if (need <= bytes) return CL_OK;
        fresh = true;
        if (p && owned) (void)hipFree(p);
        p = nullptr; bytes = 0; owned = true;
        size_t want = need + need / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) return fail(CL_ERR_HIP, "hipMalloc", hipGetErrorString(e));
        bytes = want;
        return CL_OK;
    }
    void adopt(void* slice, size_t n) { if (p && owned) (void)hipFree(p); p = slice; bytes = n; owned = false; fresh = true; }
    void release() { if (p && owned) (void)hipFree(p); p = nullptr; bytes = 0; owned = true; }
    template <typename T> T* as() { return (T*)p; }
};

// One rocPRIM primitive on `tmp`: `call(storage, bytes)` holds the rocPRIM call once and is run twice, with null storage for the
// size and with tmp for the work, so the two cannot disagree about the arguments.  Every buffer the call names is allocated before.
template <typename Call>
static inline int prim_run(DevBuf& tmp, const char* label, Call&& call)
{
    size_t bytes = 0;
    hipError_t e = call(nullptr, bytes);
    if (e != hipSuccess) return fail_at(CL_ERR_HIP, label, "size query", hipGetErrorString(e));
    const int rc = tmp.ensure(std::max<size_t>(bytes, 16));
    if (rc) return rc;
    bytes = tmp.bytes;
    e = call(tmp.p, bytes);
    if (e != hipSuccess) return fail(CL_ERR_HIP, label, hipGetErrorString(e));
    return CL_OK;
}
