// cl_devbuf.h -- the device buffer every handle is made of.  A DevBuf owns its allocation: it frees it when it is destroyed, it
// cannot be copied, and a move hands the memory over and leaves the source empty.  So a struct of buffers is released by destroying
// it or by assigning a fresh one (`c->mx = cl_chrom::Mat()`), and no function keeps a list of buffer names.  None may have static
// storage duration: its destructor would call hipFree after the runtime has gone.
#pragma once
#include <cstddef>
#include "cl_err.h"

struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    bool fresh = false;               // (re)allocated since the flag was last cleared
    bool owned = true;                // false: a slice of the handle's arena (never freed on its own)
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), fresh(o.fresh), owned(o.owned) { o.p = nullptr; o.bytes = 0; o.owned = true; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p; bytes = o.bytes; fresh = o.fresh; owned = o.owned;
            o.p = nullptr; o.bytes = 0; o.owned = true;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    int ensure(size_t need)
    {
        if (need <= bytes) return CL_OK;
        fresh = true;
        release();
        size_t want = need + need / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return fail(CL_ERR_HIP, "hipMalloc", hipGetErrorString(e)); }
        bytes = want;
        return CL_OK;
    }
    void adopt(void* slice, size_t n) { release(); p = slice; bytes = n; owned = false; fresh = true; }
    void release() { if (p && owned) (void)hipFree(p); p = nullptr; bytes = 0; owned = true; }
    template <typename T> T* as() { return (T*)p; }
};
