// Host-only check of csrc/pp_ring.h's bookkeeping: the slot cursor and the slots' parts of a bound array, and StageMem's
// register / release / rollback with the allocator stubbed.  Calls no HIP entry point, so it runs on a machine without a
// GPU, and is meant to be built with the host sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -I <package>/csrc \
//         tools/ring_host_check.hip -o ring_host_check && ./ring_host_check
#include <stdio.h>
#include <stdlib.h>
#include <set>

#include "pp_ring.h"

static std::set<void*> g_live;
static int g_allocs = 0, g_frees = 0, g_fail_at = -1;

static hipError_t stub_alloc(void** p, size_t bytes) {
    if (g_allocs == g_fail_at) { ++g_allocs; return hipErrorOutOfMemory; }
    ++g_allocs;
    *p = malloc(bytes);
    g_live.insert(*p);
    return hipSuccess;
}
static hipError_t stub_free(void* p) {
    if (!g_live.erase(p)) { fprintf(stderr, "free of a pointer that is not live\n"); abort(); }
    ++g_frees;
    free(p);
    return hipSuccess;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

struct Stage {              // as a stage struct on the handle: the owner beside the pointers it fills
    StageMem mem;
    float* a = nullptr;
    int* b = nullptr;
    double* c[2] = {nullptr, nullptr};
};

static void fill(Stage& s) {
    s.mem(&s.a, 100); s.mem(&s.b, 0); s.mem(&s.c[0], 7); s.mem(&s.c[1], 7);
}

int main() {
    // the cursor: 2 * OFF_RING + 1 takes walk the slots in order, twice round and one on
    int cursor = 0;
    for (int i = 0; i < 2 * OFF_RING + 1; ++i) {
        CHECK(cursor == i % OFF_RING);
        cursor = CallRing::next(cursor);
        CHECK(cursor >= 0 && cursor < OFF_RING);
    }
    CHECK(cursor == 1);
    // a bound array's parts tile it without overlap (the pinned allocation itself needs the runtime: a heap block stands in)
    {
        RingArray<double> arr;
        const size_t per_slot = 13 * 3;
        arr.base = (double*)malloc(OFF_RING * per_slot * sizeof(double));
        arr.per_slot = per_slot;
        for (int s = 0; s < OFF_RING; ++s) {
            CHECK(arr.at(s) == arr.base + (size_t)s * per_slot);
            for (size_t i = 0; i < per_slot; ++i) arr.at(s)[i] = s;          // (every element inside the block)
        }
        for (int s = 0; s < OFF_RING; ++s) CHECK(arr.at(s)[0] == s && arr.at(s)[per_slot - 1] == s);
        free(arr.base);
    }
    // StageMem: a complete run, released
    {
        Stage s;
        s.mem.alloc_fn = stub_alloc; s.mem.free_fn = stub_free;
        fill(s);
        CHECK(s.mem.failed() == hipSuccess);
        CHECK(s.a && s.b && s.c[0] && s.c[1] && g_live.size() == 4 && s.mem.owned.size() == 4);
        s.a[99] = 1.f; s.b[0] = 1; s.c[1][6] = 1.0;                            // (a count of 0 still leaves one element)
        s.mem.release();
        CHECK(!s.a && !s.b && !s.c[0] && !s.c[1] && g_live.empty() && s.mem.owned.empty());
        s.mem.release();                                                       // (again: nothing to do)
        CHECK(g_frees == 4);
        // ... and re-made after a release, as a configuration of another shape does
        fill(s);
        CHECK(s.mem.failed() == hipSuccess && g_live.size() == 4);
        s.mem.release();
        CHECK(g_live.empty());
    }
    // a run that fails at its third allocation rolls back by itself and can be tried again
    {
        Stage s;
        s.mem.alloc_fn = stub_alloc; s.mem.free_fn = stub_free;
        g_fail_at = g_allocs + 2;
        fill(s);
        CHECK(s.mem.st == hipErrorOutOfMemory && g_live.size() == 2 && !s.c[0] && !s.c[1]);   // (the fourth was not tried)
        CHECK(s.mem.failed() == hipErrorOutOfMemory);
        CHECK(!s.a && !s.b && g_live.empty() && s.mem.owned.empty() && s.mem.st == hipSuccess);
        g_fail_at = -1;
        fill(s);
        CHECK(s.mem.failed() == hipSuccess && g_live.size() == 4);
        s.mem.release();
        CHECK(g_live.empty());
    }
    printf("ring_host_check OK: %d allocations, %d frees\n", g_allocs, g_frees);
    return 0;
}
