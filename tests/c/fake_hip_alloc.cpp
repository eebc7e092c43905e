/* Test double of the three HIP entry points cloops_amd/csrc/cl_devbuf.h uses, on host memory (tests/test_devbuf.py): it counts
 * the live allocations, can be told to fail the next ones, and ends the program when hipFree is handed anything but the start of a
 * live block -- a slice of another block, or a block a second time. */
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstdlib>
#include <set>

static std::set<void*> g_blocks;
int fake_fail_next = 0;                               // so many of the next hipMalloc calls fail
long fake_frees = 0;                                  // blocks freed so far
long fake_live() { return (long)g_blocks.size(); }

hipError_t hipMalloc(void** p, size_t n)
{
    if (fake_fail_next > 0) { --fake_fail_next; return hipErrorOutOfMemory; }
    *p = std::malloc(n ? n : 1);
    g_blocks.insert(*p);
    return hipSuccess;
}
hipError_t hipFree(void* p)
{
    if (!p) return hipSuccess;
    if (!g_blocks.erase(p)) { std::fprintf(stderr, "fake hipFree: %p is no live block of hipMalloc\n", p); std::abort(); }
    std::free(p);
    ++fake_frees;
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake: out of memory"; }
