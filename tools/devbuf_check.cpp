// devbuf_check.cpp -- DevBuf (odr-dabmod_amd/csrc/devbuf.h) on the host alone: hipMalloc / hipFree are counting fakes over
// malloc / free defined here, no HIP library is linked.  What it holds DevBuf to: reserve grows and never shrinks, a failed
// allocation leaves the buffer empty, moves empty their source, std::swap neither allocates nor frees, assigning onto a
// buffer frees what it held exactly once, and nothing is left allocated at the end.
//   c++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include -Iodr-dabmod_amd/csrc tools/devbuf_check.cpp  (tests/test_devbuf_host.py)
#include "devbuf.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

namespace {
int g_mallocs = 0, g_frees = 0, g_bad_frees = 0;
std::set<void *> g_live;
constexpr size_t kRefuseAbove = 1 << 20;       // the fake device is out of memory beyond this
int g_failed = 0;

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            ++g_failed;                                                            \
        }                                                                          \
    } while (0)
}  // namespace

extern "C" hipError_t hipMalloc(void **ptr, size_t size)
{
    if (size > kRefuseAbove) return hipErrorOutOfMemory;   // (*ptr is left as it was, like the runtime)
    *ptr = std::malloc(size ? size : 1);
    if (!*ptr) return hipErrorOutOfMemory;
    g_live.insert(*ptr);
    ++g_mallocs;
    return hipSuccess;
}

extern "C" hipError_t hipFree(void *ptr)
{
    if (!ptr) return hipSuccess;
    if (!g_live.erase(ptr)) {
        ++g_bad_frees;                                     // a double free, or a pointer that was never handed out
        return hipErrorInvalidValue;
    }
    std::free(ptr);
    ++g_frees;
    return hipSuccess;
}

using dabgpu_api::DevBuf;

int main()
{
    {
        // reserve: grows, does not shrink, does nothing when the capacity is there
        DevBuf b;
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(b.reserve(0) == hipSuccess && b.p == nullptr && g_mallocs == 0);
        CHECK(b.reserve(100) == hipSuccess && b.p && b.cap == 100 && g_mallocs == 1);
        void *first = b.p;
        CHECK(b.reserve(40) == hipSuccess && b.p == first && b.cap == 100 && g_mallocs == 1 && g_frees == 0);
        CHECK(b.reserve(100) == hipSuccess && b.p == first && g_mallocs == 1);
        CHECK(b.reserve(101) == hipSuccess && b.cap == 101 && g_mallocs == 2 && g_frees == 1);   // free, then allocate

        // a failed allocation: the error comes back, the buffer is empty, the old memory has been freed
        CHECK(b.reserve(kRefuseAbove + 1) == hipErrorOutOfMemory);
        CHECK(b.p == nullptr && b.cap == 0 && g_frees == 2 && g_live.empty());
        CHECK(b.reserve(8) == hipSuccess && b.cap == 8);   // and it serves again

        // moves empty their source
        void *held = b.p;
        DevBuf m(std::move(b));
        CHECK(b.p == nullptr && b.cap == 0 && m.p == held && m.cap == 8);
        DevBuf n;
        n = std::move(m);
        CHECK(m.p == nullptr && m.cap == 0 && n.p == held && n.cap == 8);
        DevBuf &same = n;
        n = std::move(same);                               // (self-assignment keeps the memory)
        CHECK(n.p == held && n.cap == 8);

        // std::swap (LaneScope::swap): three moves, no allocation, no free
        DevBuf o;
        CHECK(o.reserve(16) == hipSuccess);
        void *other = o.p;
        const int mallocs = g_mallocs, frees = g_frees;
        std::swap(n, o);
        CHECK(n.p == other && n.cap == 16 && o.p == held && o.cap == 8);
        CHECK(g_mallocs == mallocs && g_frees == frees);
        DevBuf empty;
        std::swap(n, empty);                               // (a lane that has no scratch yet)
        CHECK(n.p == nullptr && n.cap == 0 && empty.p == other && empty.cap == 16);
        CHECK(g_mallocs == mallocs && g_frees == frees);

        // assigning onto a buffer that holds memory frees it, once
        o = std::move(empty);
        CHECK(o.p == other && o.cap == 16 && empty.p == nullptr && g_frees == frees + 1 && !g_live.count(held));

        // release empties; the destructor of what is left frees the rest
        DevBuf r;
        CHECK(r.reserve(32) == hipSuccess);
        r.release();
        CHECK(r.p == nullptr && r.cap == 0);
        r.release();
    }
    CHECK(g_live.empty());
    CHECK(g_mallocs == g_frees);
    CHECK(g_bad_frees == 0);
    if (g_failed) return 1;
    std::printf("devbuf ok: %d allocations, %d frees, none live\n", g_mallocs, g_frees);
    return 0;
}
