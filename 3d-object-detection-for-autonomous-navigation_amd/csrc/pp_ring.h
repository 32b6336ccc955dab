// The pinned call ring and the owner of a stage's device memory: the host-side plumbing the stages on the resident frames
// share.  Nothing here names pp_engine, so tools/ring_host_check.hip exercises the bookkeeping without a GPU.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <vector>

// Small per-call host data (frame offsets, planes, poses and stamps, dt values, ingest records, feature tables, rig
// sources, OccCalls) reaches the device through page-locked memory: a pageable source would be staged synchronously, and a
// single pinned buffer could be rewritten while its copy is still queued.  So there are OFF_RING slots, and a slot is
// reused only after the event recorded behind its last copies has passed.  A call takes a slot after every check that can
// refuse it and before the first copy or launch it queues (a refused call leaves the cursor where it was), fills the
// slot's part of every array it sends, queues the copies and records the slot's event behind the last of them.  Several
// arrays share one ring and travel under one event: the handle's ring carries the offsets and, as riders, the ingest
// records and features, the rig sources, the crop planes and the sweep poses.  The tracker's dt and pose rings and the
// occupancy call ring are rings of their own because they are consumed on the main stream whatever the copy stream is
// doing: on the handle's ring a slot last used by a copy-stream upload would make a main-stream call wait for that upload.
constexpr int OFF_RING = 4;

struct CallRing {
    hipEvent_t ev[OFF_RING] = {};
    int cursor = 0;                    // the slot the next take() hands out
    std::vector<void**> arrays;        // the pinned arrays bound to this ring (RingArray::alloc): released with it

    static int next(int slot) { return (slot + 1) % OFF_RING; }
    hipError_t create() {              // (again after a failure: makes what is missing)
        for (hipEvent_t& x : ev)
            if (!x)
                if (hipError_t st = hipEventCreateWithFlags(&x, hipEventDisableTiming)) return st;
        return hipSuccess;
    }
    hipError_t take(int* slot) {       // the slot of this call, once the copies that last used it have been consumed
        if (hipError_t st = hipEventSynchronize(ev[cursor])) return st;
        *slot = cursor;
        cursor = next(cursor);
        return hipSuccess;
    }
    hipError_t sent(int slot, hipStream_t stream) { return hipEventRecord(ev[slot], stream); }
    void release() {
        for (void** p : arrays) { if (*p) (void)hipHostFree(*p); *p = nullptr; }
        arrays.clear();
        for (hipEvent_t& x : ev) { if (x) (void)hipEventDestroy(x); x = nullptr; }
        cursor = 0;
    }
};

// A pinned array of OFF_RING parts of `per_slot` elements, bound to a ring, which frees it.
template <typename Tp>
struct RingArray {
    Tp* base = nullptr;
    size_t per_slot = 0;

    hipError_t alloc(CallRing& ring, size_t n_per_slot) {      // (once: a second call finds it made; the ring's events too)
        if (base) return hipSuccess;
        if (hipError_t st = ring.create()) return st;
        if (hipError_t st = hipHostMalloc((void**)&base, (size_t)OFF_RING * n_per_slot * sizeof(Tp))) return st;
        per_slot = n_per_slot;
        ring.arrays.push_back((void**)&base);
        return hipSuccess;
    }
    Tp* at(int slot) const { return base + (size_t)slot * per_slot; }
    // queues the first `count` elements of the slot's part -> dst on `stream`
    hipError_t send(int slot, void* dst, size_t count, hipStream_t stream) const {
        return hipMemcpyAsync(dst, at(slot), count * sizeof(Tp), hipMemcpyHostToDevice, stream);
    }
};

// The device memory of a stage that re-makes its buffers when its configuration changes shape (what lives as long as the
// handle goes through DevAlloc into pp_engine::allocs instead).  A run of allocations stops at the first failure and
// `failed()` then gives everything back:  StageMem& M = g.mem;  M(&g.a, n);  M(&g.b, m);  if (hipError_t st = M.failed()) ...
// release() frees every pointer the owner filled and nulls it where it lives.
struct StageMem {
    std::vector<void**> owned;         // the addresses of the pointers filled
    hipError_t st = hipSuccess;
    hipError_t (*alloc_fn)(void**, size_t) = hipMalloc;
    hipError_t (*free_fn)(void*) = hipFree;

    template <typename Tp>
    void operator()(Tp** p, size_t count) {
        void* q = nullptr;
        if (st != hipSuccess || (st = alloc_fn(&q, (count ? count : 1) * sizeof(Tp))) != hipSuccess) return;
        *p = (Tp*)q;
        owned.push_back((void**)p);
    }
    hipError_t failed() {              // the first error of the run, rolled back; or hipSuccess
        const hipError_t r = st;
        if (r != hipSuccess) release();
        return r;
    }
    void release() {
        for (void** p : owned) { if (*p) (void)free_fn(*p); *p = nullptr; }
        owned.clear();
        st = hipSuccess;
    }
};
