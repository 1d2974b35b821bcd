// devbuf_check.cpp -- csrc/sfm_devbuf.h against a HIP runtime made of malloc / free: what the wrappers allocate, keep, hand over and
// release, without a GPU and without libamdhip64.  Built and run by tests/test_devbuf_host.py; exits non-zero on the first
// failed check, or when an object is still alive at the end.
#include "sfm_devbuf.h"

#include <cstdio>
#include <cstdlib>

static int live_dev = 0, live_pinned = 0, live_events = 0, live_streams = 0;
static bool fail_next_alloc = false;      // the next hipMalloc / hipHostMalloc returns hipErrorOutOfMemory

static hipError_t stub_alloc(void** p, size_t bytes, int* live) {
    if (fail_next_alloc) { fail_next_alloc = false; *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(bytes ? bytes : 1);
    if (!*p) return hipErrorOutOfMemory;
    ++*live;
    return hipSuccess;
}

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(p, bytes, &live_dev); }
hipError_t hipFree(void* p) { if (p) { free(p); --live_dev; } return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return stub_alloc(p, bytes, &live_pinned); }
hipError_t hipHostFree(void* p) { if (p) { free(p); --live_pinned; } return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = (hipEvent_t)malloc(1); ++live_events; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); --live_events; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { *s = (hipStream_t)malloc(1); ++live_streams; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { free(s); --live_streams; return hipSuccess; }
}

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

using namespace sfm;

template <typename Buf>
static void check_buffer(int& live) {
    const int live0 = live;
    {
        Buf a;
        CHECK(a.get() == nullptr && a.cap() == 0 && !a);
        // alloc: exactly n, a second alloc replaces the block, alloc(0) leaves it empty
        CHECK(a.alloc(10) == hipSuccess && a.get() != nullptr && a.cap() == 10 && live == live0 + 1);
        a[9] = 7;
        CHECK(a.alloc(3) == hipSuccess && a.cap() == 3 && live == live0 + 1);
        CHECK(a.alloc(0) == hipSuccess && a.get() == nullptr && a.cap() == 0 && live == live0);
        // reserve: n + n / 2 + 16 when it grows, the same block while n fits
        CHECK(a.reserve(100) == hipSuccess && a.cap() == 100 + 50 + 16 && live == live0 + 1);
        int* const block = a;
        CHECK(a.reserve(100) == hipSuccess && a.reserve(1) == hipSuccess && a.reserve(166) == hipSuccess);
        CHECK(a.get() == block && a.cap() == 166 && live == live0 + 1);
        CHECK(a.reserve(167) == hipSuccess && a.cap() == 167 + 83 + 16 && live == live0 + 1);
        CHECK(a.reserve(7) == hipSuccess && a.cap() == 266);
        // an empty buffer allocates even for n == 0
        Buf z;
        CHECK(z.reserve(0) == hipSuccess && z.get() != nullptr && z.cap() == 16 && live == live0 + 2);
        CHECK(z.reset() == hipSuccess && z.get() == nullptr && z.cap() == 0 && live == live0 + 1);
        // move construction and move assignment hand the block over; the target's old block is freed
        int* const pa = a;
        Buf b(std::move(a));
        CHECK(b.get() == pa && b.cap() == 266 && a.get() == nullptr && a.cap() == 0 && live == live0 + 1);
        Buf c;
        CHECK(c.alloc(5) == hipSuccess && live == live0 + 2);
        c = std::move(b);
        CHECK(c.get() == pa && c.cap() == 266 && b.get() == nullptr && b.cap() == 0 && live == live0 + 1);
        Buf& self = c;
        c = std::move(self);                                       // (self-assignment keeps the block)
        CHECK(c.get() == pa && c.cap() == 266 && live == live0 + 1);
        // swap: pointer and capacity travel together (the ping-pong pairs)
        Buf d;
        CHECK(d.alloc(4) == hipSuccess);
        int* const pd = d;
        swap(c, d);
        CHECK(c.get() == pd && c.cap() == 4 && d.get() == pa && d.cap() == 266 && live == live0 + 2);
        // a group struct of buffers drops with `= {}`
        struct Group { bool on = false; Buf x, y; } g;
        g.on = true;
        CHECK(g.x.alloc(8) == hipSuccess && g.y.alloc(8) == hipSuccess && live == live0 + 4);
        g = {};
        CHECK(!g.on && !g.x && !g.y && live == live0 + 2);
        // a failing allocator: the old block is gone, the buffer is empty with capacity 0, and it works again afterwards
        fail_next_alloc = true;
        CHECK(d.alloc(1000) == hipErrorOutOfMemory && d.get() == nullptr && d.cap() == 0 && live == live0 + 1);
        fail_next_alloc = true;
        CHECK(c.reserve(1000) == hipErrorOutOfMemory && c.get() == nullptr && c.cap() == 0 && live == live0);
        CHECK(c.reserve(1000) == hipSuccess && c.cap() == 1516 && live == live0 + 1);
    }
    CHECK(live == live0);                                          // the destructors freed what was left
}

int main() {
    check_buffer<DevBuf<int>>(live_dev);
    check_buffer<PinnedBuf<int>>(live_pinned);
    CHECK(live_dev == 0 && live_pinned == 0);
    {
        Event e, f;
        CHECK(!e && e.create() == hipSuccess && e && live_events == 1);
        CHECK(e.create(hipEventDisableTiming) == hipSuccess && live_events == 1);      // (created again: the old one is destroyed)
        const hipEvent_t raw = e;
        f = std::move(e);
        CHECK(!e && (hipEvent_t)f == raw && live_events == 1);
        Event g(std::move(f));
        CHECK(!f && (hipEvent_t)g == raw && live_events == 1);
        Stream s;
        CHECK(!s && s.create(hipStreamNonBlocking) == hipSuccess && s && live_streams == 1);
        Stream t(std::move(s));
        CHECK(!s && t && live_streams == 1);
        t.reset();
        CHECK(!t && live_streams == 0);
    }
    if (live_dev || live_pinned || live_events || live_streams) {
        fprintf(stderr, "still alive: %d device, %d pinned, %d events, %d streams\n", live_dev, live_pinned, live_events, live_streams);
        return 1;
    }
    printf("devbuf_check ok\n");
    return 0;
}
