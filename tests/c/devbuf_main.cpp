/* cloops_amd/csrc/cl_devbuf.h on the host (tests/test_devbuf.py): the header is compiled unchanged with g++ under ASan and UBSan and
 * linked against tests/c/fake_hip_alloc.cpp.  Every step checks the number of live blocks itself; the fake ends the program when a
 * slice or an already freed block reaches hipFree. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>
#include "cl_devbuf.h"

thread_local std::string g_err;
extern int fake_fail_next;
extern long fake_frees;
long fake_live();

#define CHECK(cond) \
    do { if (!(cond)) { std::fprintf(stderr, "devbuf_main.cpp:%d: failed: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "a copy would be a double free");
static_assert(std::is_nothrow_move_constructible<DevBuf>::value && std::is_nothrow_move_assignable<DevBuf>::value, "containers move it");

struct Unit {                                         // shaped like an analysis unit of cl_chrom
    DevBuf a, b, c;
    std::vector<long long> bounds;
    struct State { bool ready = false; long long n = 0; } st;
};
static_assert(!std::is_copy_assignable<Unit>::value && std::is_move_assignable<Unit>::value, "a unit is reset by assigning a fresh one");

static bool empty(const DevBuf& b) { return b.p == nullptr && b.bytes == 0 && b.owned; }
static void fill(DevBuf& b) { std::memset(b.p, 0x5a, b.bytes); }          // (ASan sees every byte the buffer claims)

static void ensure_and_grow()
{
    const long f0 = fake_frees;
    DevBuf b;
    CHECK(empty(b) && !b.fresh && b.ensure(0) == CL_OK && empty(b));
    CHECK(b.ensure(1000) == CL_OK && b.p && b.bytes == 1000 + 125 + 256 && b.fresh && b.owned && fake_live() == 1);
    fill(b);
    void* const p0 = b.p;
    b.fresh = false;
    CHECK(b.ensure(1000) == CL_OK && b.ensure(b.bytes) == CL_OK && b.ensure(1) == CL_OK);
    CHECK(b.p == p0 && !b.fresh && fake_frees == f0 && fake_live() == 1);  // at or below the size held: nothing happens
    const size_t more = b.bytes + 1;
    CHECK(b.ensure(more) == CL_OK && b.bytes >= more && b.fresh && fake_frees == f0 + 1 && fake_live() == 1);
    fill(b);
    CHECK(b.as<int>() == (int*)b.p);
    b.release();
    CHECK(empty(b) && fake_frees == f0 + 2 && fake_live() == 0);
    b.release();                                                            // (of nothing)
    CHECK(empty(b) && fake_frees == f0 + 2);
}

static void failing_allocation()
{
    const long f0 = fake_frees;
    DevBuf b;
    fake_fail_next = 1;
    CHECK(b.ensure(64) == CL_ERR_HIP && empty(b) && fake_live() == 0 && g_err.rfind("hipMalloc", 0) == 0);
    CHECK(b.ensure(64) == CL_OK && fake_live() == 1);
    fake_fail_next = 1;
    CHECK(b.ensure(100000) == CL_ERR_HIP && empty(b) && fake_live() == 0 && fake_frees == f0 + 1);   // the block held is gone, no other came
    CHECK(b.ensure(64) == CL_OK && b.p && fake_live() == 1);               // ... and the buffer serves again
}                                                                           // (freed at scope exit: checked by main)

static void scope_exit()
{
    const long f0 = fake_frees;
    {
        DevBuf a, b, never;
        CHECK(a.ensure(10) == CL_OK && b.ensure(20) == CL_OK && fake_live() == 2);
    }
    CHECK(fake_live() == 0 && fake_frees == f0 + 2);
}

static void moves()
{
    const long f0 = fake_frees;
    DevBuf a;
    CHECK(a.ensure(500) == CL_OK);
    void* const pa = a.p;
    const size_t na = a.bytes;
    DevBuf b(std::move(a));                                                 // construction
    CHECK(empty(a) && b.p == pa && b.bytes == na && b.fresh && b.owned && fake_live() == 1 && fake_frees == f0);
    DevBuf c;
    c = std::move(b);                                                       // onto an empty target
    CHECK(empty(b) && c.p == pa && c.bytes == na && fake_live() == 1 && fake_frees == f0);
    DevBuf d;
    CHECK(d.ensure(700) == CL_OK && fake_live() == 2);
    d.fresh = false;
    c.fresh = false;
    d = std::move(c);                                                       // onto a full one: its block is freed, once
    CHECK(empty(c) && d.p == pa && d.bytes == na && !d.fresh && fake_live() == 1 && fake_frees == f0 + 1);
    DevBuf& self = d;
    d = std::move(self);                                                    // self-move
    CHECK(d.p == pa && d.bytes == na && d.owned && fake_live() == 1 && fake_frees == f0 + 1);
    fill(d);
    d = DevBuf();                                                           // release by assignment
    CHECK(empty(d) && fake_live() == 0 && fake_frees == f0 + 2);
}

static void slices()
{
    DevBuf arena;
    CHECK(arena.ensure(4096) == CL_OK);
    char* const base = arena.as<char>();
    const long f0 = fake_frees;
    {
        DevBuf s;
        s.adopt(base + 256, 512);
        CHECK(s.p == base + 256 && s.bytes == 512 && !s.owned && s.fresh);
        CHECK(s.ensure(512) == CL_OK && s.p == base + 256 && !s.owned);
        CHECK(s.ensure(513) == CL_OK && s.p != base + 256 && s.owned && fake_live() == 2 && fake_frees == f0);   // outgrown: a block of its own
        fill(s);
        s.adopt(base + 1024, 128);                                          // over an owned block, which is freed
        CHECK(!s.owned && s.bytes == 128 && fake_live() == 1 && fake_frees == f0 + 1);
        DevBuf t(std::move(s));                                             // a slice moves as a slice
        CHECK(empty(s) && t.p == base + 1024 && !t.owned && fake_frees == f0 + 1);
        DevBuf u;
        CHECK(u.ensure(64) == CL_OK && fake_live() == 2);
        u = std::move(t);                                                   // ... also onto an owned block
        CHECK(empty(t) && u.p == base + 1024 && !u.owned && fake_live() == 1 && fake_frees == f0 + 2);
        u.release();
        CHECK(empty(u) && fake_frees == f0 + 2);
        u.adopt(base, 64);
    }                                                                       // a slice dies: nothing is freed
    CHECK(fake_live() == 1 && fake_frees == f0 + 2);
    std::memset(base, 0, arena.bytes);                                      // the arena is whole
}

static void units()
{
    const long f0 = fake_frees;
    Unit u;
    CHECK(u.a.ensure(100) == CL_OK && u.b.ensure(200) == CL_OK && fake_live() == 2);
    u.bounds.assign(5, 7);
    u.st.ready = true; u.st.n = 9;
    Unit::State st;
    st.n = 3;
    u.st = st;                                                              // the state alone: the buffers stay
    CHECK(u.a.p && u.b.p && u.st.n == 3 && fake_live() == 2);
    u = Unit();
    CHECK(empty(u.a) && empty(u.b) && empty(u.c) && u.bounds.empty() && !u.st.ready && u.st.n == 0 && fake_live() == 0 && fake_frees == f0 + 2);
    u = Unit();                                                             // (of nothing)
    CHECK(fake_live() == 0 && fake_frees == f0 + 2);

    std::vector<std::unique_ptr<Unit>> list, other;
    for (int k = 0; k < 3; ++k) {
        std::unique_ptr<Unit> p(new Unit());
        CHECK(p->a.ensure(64 + k) == CL_OK && p->c.ensure(8) == CL_OK);
        (k < 2 ? list : other).push_back(std::move(p));
    }
    { std::unique_ptr<Unit> dropped(new Unit()); CHECK(dropped->b.ensure(32) == CL_OK && fake_live() == 7); }    // an error path: never pushed
    CHECK(fake_live() == 6);
    list.insert(list.end(), std::make_move_iterator(other.begin()), std::make_move_iterator(other.end()));
    other.clear();
    CHECK(list.size() == 3 && fake_live() == 6);
    list.clear();
    CHECK(fake_live() == 0 && fake_frees == f0 + 2 + 7);
}

int main()
{
    void (*const cases[])() = {ensure_and_grow, failing_allocation, scope_exit, moves, slices, units};
    for (auto run : cases) {
        run();
        CHECK(fake_live() == 0 && fake_fail_next == 0);
    }
    std::puts("devbuf ok");
    return 0;
}
