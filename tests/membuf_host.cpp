// The owning buffer types of csrc/ffq_mem.h (Buf, MirrorOf), driven on the host with a counting allocator in place of
// the device and pinned ones: malloc / free that count the live blocks and can be told to fail the k-th request from now.
// What the library relies on, and what no GPU test can see (a leak, a second free):
//   * a grow within the capacity keeps the block;
//   * a regrow frees exactly one block, before it asks for the new one, and leaves one;
//   * a grow that fails leaves p == nullptr, cap == 0, no live block -- and the buffer can be grown again;
//   * a pair whose second half fails ends with both halves empty;
//   * a moved-from buffer is empty and its destructor frees nothing; move assignment frees what the target held;
//   * reset() twice is harmless;
//   * when everything has gone out of scope no block is live.
//
//   clang++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I <package>/csrc tests/membuf_host.cpp -o membuf_host
// Run it with leak detection ON under AddressSanitizer: leaks are what it is for.
// Exit status 0 and "ok" on the last line, or 1 and a line per failure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#define FFQ_MEM_NO_HIP
#include "ffq_mem.h"

using namespace ffq;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_fail++; std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

// `Tag` makes two allocators with counters of their own (the two halves of a pair)
template <int Tag>
struct CountAlloc {
    using error = int;
    static constexpr error ok = 0;
    static long live, allocs, frees, live_at_alloc;
    static int fail_in;              // > 0: the fail_in-th request from now fails
    static error alloc(void **p, size_t bytes)
    {
        live_at_alloc = live;
        if (fail_in > 0 && --fail_in == 0) return 2;       // (like hipMalloc: *p is left alone)
        *p = std::malloc(bytes ? bytes : 1);
        if (!*p) return 2;
        std::memset(*p, 0xA5, bytes);
        live++; allocs++;
        return ok;
    }
    static void release(void *p)
    {
        if (!p) { g_fail++; std::printf("FAIL: release(nullptr)\n"); return; }
        std::free(p);                 // (a second free of one block: AddressSanitizer reports it)
        live--; frees++;
    }
};
template <int Tag> long CountAlloc<Tag>::live = 0;
template <int Tag> long CountAlloc<Tag>::allocs = 0;
template <int Tag> long CountAlloc<Tag>::frees = 0;
template <int Tag> long CountAlloc<Tag>::live_at_alloc = 0;
template <int Tag> int CountAlloc<Tag>::fail_in = 0;

using A = CountAlloc<0>;
using B = CountAlloc<1>;
struct Row { int64_t v[6]; };

static void test_grow()
{
    Buf<int64_t, A> b;
    CHECK(b.p == nullptr && b.cap == 0 && A::live == 0);
    CHECK(b.grow(0) == A::ok && b.p == nullptr && A::allocs == 0);        // nothing asked for, nothing done
    CHECK(b.grow(100) == A::ok && b.p != nullptr && b.cap == 100 && A::live == 1);
    b.p[99] = 7;                                                           // (100 ELEMENTS: the last one is there)
    int64_t *const first = b.p;
    CHECK(static_cast<int64_t *>(b) == first);
    // within the capacity: the same block, no call of the allocator
    CHECK(b.grow(100) == A::ok && b.grow(1) == A::ok && b.grow(99) == A::ok);
    CHECK(b.p == first && b.cap == 100 && A::allocs == 1 && A::frees == 0);
    // regrow: the old block is freed first (nothing is live when the new one is asked for), one new block
    CHECK(b.grow(101) == A::ok && b.cap == 101 && A::allocs == 2 && A::frees == 1 && A::live == 1 && A::live_at_alloc == 0);
    b.p[100] = 9;
    // elements, not bytes
    Buf<Row, A> r;
    CHECK(r.grow(3) == A::ok && r.cap == 3);
    r.p[2].v[5] = 1;
    CHECK(r->v[0] == (int64_t)0xA5A5A5A5A5A5A5A5ull);                      // operator->: the first element
}

static void test_failed_grow()
{
    Buf<int64_t, A> b;
    CHECK(b.grow(10) == A::ok);
    const long frees = A::frees;
    A::fail_in = 1;
    CHECK(b.grow(20) != A::ok);
    CHECK(b.p == nullptr && b.cap == 0 && A::live == 0 && A::frees == frees + 1);
    // ... and it can be grown again, also to what it held before
    CHECK(b.grow(10) == A::ok && b.p != nullptr && b.cap == 10 && A::live == 1);
    // a failure on an empty buffer
    Buf<int64_t, A> e;
    A::fail_in = 1;
    CHECK(e.grow(5) != A::ok && e.p == nullptr && e.cap == 0);
    CHECK(A::live == 1);
}

static void test_mirror()
{
    MirrorOf<int64_t, A, B> m;
    CHECK(m.grow(50) == A::ok && m.d.cap == 50 && m.h.cap == 50 && A::live == 1 && B::live == 1);
    int64_t *const d = m.d.p, *const h = m.h.p;
    CHECK(m.grow(50) == A::ok && m.grow(7) == A::ok && m.d.p == d && m.h.p == h);     // within the capacity
    // the second half fails: both empty
    B::fail_in = 1;
    CHECK(m.grow(60) != A::ok);
    CHECK(m.d.p == nullptr && m.d.cap == 0 && m.h.p == nullptr && m.h.cap == 0 && A::live == 0 && B::live == 0);
    // the first half fails: the second is not asked
    const long b_allocs = B::allocs;
    CHECK(m.grow(60) == A::ok && B::allocs == b_allocs + 1);
    A::fail_in = 1;
    CHECK(m.grow(70) != A::ok && B::allocs == b_allocs + 1);
    CHECK(m.d.p == nullptr && m.h.p == nullptr && A::live == 0 && B::live == 0);
    CHECK(m.grow(70) == A::ok && m.d.cap == 70 && m.h.cap == 70);
    m.reset();
    CHECK(A::live == 0 && B::live == 0 && m.d.cap == 0 && m.h.cap == 0);
    m.reset();
    // moved as a whole (the stream's slots when the carry grows)
    MirrorOf<int64_t, A, B> old[2];
    CHECK(m.grow(8) == A::ok);
    int64_t *const h8 = m.h.p;
    old[1] = std::move(m);
    CHECK(m.d.p == nullptr && m.h.p == nullptr && m.h.cap == 0 && old[1].h.p == h8 && old[1].d.cap == 8);
    CHECK(m.grow(16) == A::ok && A::live == 2 && B::live == 2);
}

static void test_move_and_reset()
{
    const long frees = A::frees;
    {
        Buf<int64_t, A> a;
        CHECK(a.grow(4) == A::ok);
        int64_t *const p = a.p;
        Buf<int64_t, A> b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.p == p && b.cap == 4 && A::live == 1);
        CHECK(a.grow(2) == A::ok && A::live == 2);                       // the moved-from one is an ordinary empty buffer
        // move assignment: what the target held is freed, the source is empty
        Buf<int64_t, A> c;
        CHECK(c.grow(9) == A::ok && A::live == 3);
        c = std::move(b);
        CHECK(c.p == p && c.cap == 4 && b.p == nullptr && b.cap == 0 && A::live == 2);
        Buf<int64_t, A> &self = c;
        c = std::move(self);                                             // onto itself: nothing happens
        CHECK(c.p == p && c.cap == 4 && A::live == 2);
        c.reset();
        CHECK(c.p == nullptr && c.cap == 0 && A::live == 1);
        c.reset();                                                       // twice: harmless
        CHECK(A::live == 1);
    }
    // a, b, c have gone: b and c were empty, a held one block
    CHECK(A::live == 0 && A::frees == frees + 3);
}

int main()
{
    test_grow();
    CHECK(A::live == 0);
    test_failed_grow();
    CHECK(A::live == 0);
    test_mirror();
    CHECK(A::live == 0 && B::live == 0);
    test_move_and_reset();
    CHECK(A::live == 0 && B::live == 0 && A::allocs == A::frees && B::allocs == B::frees);
    std::printf("%d checks, %d failures, %ld + %ld blocks allocated, %ld + %ld live\n", g_checks, g_fail, A::allocs, B::allocs, A::live, B::live);
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}
