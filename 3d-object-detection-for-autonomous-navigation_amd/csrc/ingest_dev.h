// What the two live-camera ingests share on the device (ingest.hip: PointCloud2 messages; depth_ingest.hip: raw depth
// images): the unaligned dword load, the scan of the chunk counts and the float64 camera -> lidar transform.  Both
// translation units wrap ingest_scan_frames in a kernel of their own, so each keeps its kernel name and its frame type.
#pragma once

#include "pp_common.h"

// four bytes at any address (nothing in a message is assumed to sit on a boundary): one unaligned dword load
__device__ __forceinline__ uint32_t ing_load32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// The body of a one-workgroup scan kernel of 16 waves (1024 threads): wave w scans the chunk counts of frames w, w + 16,
// ... into chunk bases and the frame's finite (valid) and kept counts; thread 0 then sums the kept counts into the
// offsets.  Frame: any per-frame record with an `nchunks` member.
template <typename Frame>
__device__ __forceinline__ void ingest_scan_frames(const Frame* __restrict__ frames, int batch, int stride, int first,
                                                   int decimate, const int* __restrict__ chunk_cnt,
                                                   int* __restrict__ chunk_base, int* __restrict__ finite,
                                                   int* __restrict__ kept, int* __restrict__ offsets) {
    const int lane = threadIdx.x & (PP_WAVE - 1), wave = threadIdx.x >> 6;
    for (int b = wave; b < batch; b += 16) {
        const int nchunks = frames[b].nchunks;
        int carry = 0;
        for (int c0 = 0; c0 < nchunks; c0 += PP_WAVE) {
            const int c = c0 + lane;
            const int v = c < nchunks ? chunk_cnt[(size_t)b * stride + c] : 0;
            const int incl = wave_inclusive_scan(v);
            if (c < nchunks) chunk_base[(size_t)b * stride + c] = carry + incl - v;
            carry += __builtin_amdgcn_readlane(incl, PP_WAVE - 1);
        }
        if (lane == 0) {
            finite[b] = carry;
            kept[b] = carry > first ? (carry - first + decimate - 1) / decimate : 0;
        }
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        int off = 0;
        offsets[0] = 0;
        for (int b = 0; b < batch; ++b) { off += kept[b]; offsets[b + 1] = off; }
    }
}

struct IngXform { double r[9], r2[9], lift[3]; };

// ((p . r) . r2) + lift, each sum left to right, products and sums rounded separately
__device__ __forceinline__ void ing_transform(const double p[3], const IngXform& x, float out[3]) {
#pragma clang fp contract(off)
    double q[3], s[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) q[j] = (p[0] * x.r[j] + p[1] * x.r[3 + j]) + p[2] * x.r[6 + j];
#pragma unroll
    for (int j = 0; j < 3; ++j) s[j] = (q[0] * x.r2[j] + q[1] * x.r2[3 + j]) + q[2] * x.r2[6 + j];
#pragma unroll
    for (int j = 0; j < 3; ++j) out[j] = (float)(s[j] + x.lift[j]);
}

template <typename Params>
inline IngXform ing_xform_of(const Params& p) {
    IngXform xf;
    for (int i = 0; i < 9; ++i) { xf.r[i] = p.r[i]; xf.r2[i] = p.r2[i]; }
    for (int i = 0; i < 3; ++i) xf.lift[i] = p.lift[i];
    return xf;
}
