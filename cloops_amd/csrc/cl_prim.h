// cl_prim.h -- host side shared by the translation units: the one way a rocPRIM primitive is called on temporary storage that a
// device buffer (cl_devbuf.h) holds.
#pragma once
#include "cl_common.h"
#include "cl_devbuf.h"

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
