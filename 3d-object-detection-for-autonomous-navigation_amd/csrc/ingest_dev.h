// What the two live-camera ingests share on the device (ingest.hip: PointCloud2 messages; depth_ingest.hip: raw depth
// images; rig_ingest.hip: several sources of either kind per frame): the chunking, the unaligned dword load, the per-record
// decode and validity of both feeds, the scan of the chunk counts and the float64 camera -> lidar transform.  ingest.hip
// and depth_ingest.hip wrap ingest_scan_frames in a kernel of their own, so each keeps its kernel name and its frame type.
#pragma once

#include "pp_common.h"

// four bytes at any address (nothing in a message is assumed to sit on a boundary): one unaligned dword load
__device__ __forceinline__ uint32_t ing_load32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

constexpr int ING_ITER = 8;                       // 64-record steps of a wave
constexpr int ING_CHUNK = PP_WAVE * ING_ITER;     // records per chunk (one wave)
constexpr int ING_WAVES = 4;                      // chunks per workgroup

// ---- PointCloud2 records (IngFrame): decode and validity, as k_ingest_count / k_ingest_scatter and the rig kernels use them
// one coordinate as float64 (a float32 field widens exactly)
__device__ __forceinline__ double ing_coord(const uint8_t* p, const IngFrame& f) {
    if (f.f64) {
        const uint32_t a = ing_load32(p), b = ing_load32(p + 4);
        unsigned long long v = ((unsigned long long)b << 32) | a;
        if (f.big_endian) v = __builtin_bswap64(v);
        return __longlong_as_double((long long)v);
    }
    uint32_t v = ing_load32(p);
    if (f.big_endian) v = __builtin_bswap32(v);
    return (double)__uint_as_float(v);
}

__device__ __forceinline__ bool ing_finite(double v) {
    return (((unsigned long long)__double_as_longlong(v) >> 52) & 0x7ffull) != 0x7ffull;
}

__device__ __forceinline__ const uint8_t* ing_record(const uint8_t* base, const IngFrame& f, int i) {
    // (the host hands a frame whose rows are tight over as ONE row: no division then)
    if (f.width >= f.n_rec) return base + (long long)i * f.point_step;
    const int row = i / f.width, col = i - row * f.width;
    return base + (long long)row * f.row_step + (long long)col * f.point_step;
}

__device__ __forceinline__ bool ing_read(const uint8_t* base, const IngFrame& f, int i, double p[3]) {
    const uint8_t* rec = ing_record(base, f, i);
    p[0] = ing_coord(rec + f.x_off, f);
    p[1] = ing_coord(rec + f.y_off, f);
    p[2] = ing_coord(rec + f.z_off, f);
    return ing_finite(p[0]) && ing_finite(p[1]) && ing_finite(p[2]);
}

// ---- feature columns (IngFeat): what the scatter kernels of pp_ingest_pointcloud2_fields* write behind x y z
// the raw element at any address, byte-swapped when the message is big-endian, widened exactly to float64
template <typename T>
__device__ __forceinline__ T ing_load(const uint8_t* p) {
    T v;
    __builtin_memcpy(&v, p, sizeof(T));
    return v;
}

__device__ __forceinline__ double ing_raw(const uint8_t* p, int type, bool big_endian) {
    switch (type) {                                // (the same for every lane of the wave: a scalar branch)
        case 1: return (double)ing_load<int8_t>(p);
        case 2: return (double)ing_load<uint8_t>(p);
        case 3: {
            uint16_t v = ing_load<uint16_t>(p);
            if (big_endian) v = __builtin_bswap16(v);
            return (double)(int16_t)v;
        }
        case 4: {
            uint16_t v = ing_load<uint16_t>(p);
            if (big_endian) v = __builtin_bswap16(v);
            return (double)v;
        }
        case 5: {
            uint32_t v = ing_load<uint32_t>(p);
            if (big_endian) v = __builtin_bswap32(v);
            return (double)(int32_t)v;
        }
        case 6: {
            uint32_t v = ing_load<uint32_t>(p);
            if (big_endian) v = __builtin_bswap32(v);
            return (double)v;
        }
        case 7: {
            uint32_t v = ing_load<uint32_t>(p);
            if (big_endian) v = __builtin_bswap32(v);
            return (double)__uint_as_float(v);
        }
        default: {                                 // 8 (the host refused every other code)
            unsigned long long v = ing_load<unsigned long long>(p);
            if (big_endian) v = __builtin_bswap64(v);
            return __longlong_as_double((long long)v);
        }
    }
}

// float32(float64(raw) * scale + bias), product and sum rounded separately; a constant column (type 0) reads nothing.
// A non-finite value is carried through as it is.
__device__ __forceinline__ float ing_feature(const uint8_t* rec, const IngFeat& t, bool big_endian) {
#pragma clang fp contract(off)
    if (t.type == 0) return (float)t.bias;
    const double prod = ing_raw(rec + t.off, t.type, big_endian) * t.scale;
    return (float)(prod + t.bias);
}

// one row of F floats, written once: a single 16-byte store for F = 4 (the rows of `out` are 16-byte aligned then)
template <int F>
__device__ __forceinline__ void ing_store_row(float* __restrict__ out, long long row, const float (&o)[F]) {
    if constexpr (F == 4) {
        *reinterpret_cast<float4*>(out + row * 4) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int j = 0; j < F; ++j) out[row * F + j] = o[j];
    }
}

// ---- depth pixels (DepthFrame): decode, validity and deprojection, as k_depth_count / k_depth_scatter and the rig kernels use them
// depth and validity of pixel i (i < n_pix) of a frame
__device__ __forceinline__ bool dep_read(const uint8_t* base, const DepthFrame& f, int i, float& z) {
    const int isz = f.f32 ? 4 : 2;
    const uint8_t* px;
    if (f.tight) {
        px = base + (long long)i * isz;
    } else {                                       // (only padded rows pay this division)
        const int v = i / f.width, u = i - v * f.width;
        px = base + (long long)v * f.row_step + (long long)u * isz;
    }
    bool ok;
    if (f.f32) {
        uint32_t w = ing_load32(px);
        if (f.big_endian) w = __builtin_bswap32(w);
        z = __uint_as_float(w);
        ok = ((w >> 23) & 0xffu) != 0xffu && z > 0.0f;
    } else {
        uint16_t d;
        __builtin_memcpy(&d, px, 2);
        if (f.big_endian) d = __builtin_bswap16(d);
        z = f.depth_scale * (float)d;
        ok = d != 0;
    }
    return ok && z > f.z_min && z <= f.z_max;
}

// the camera-frame point of pixel i with depth z, widened to float64
__device__ __forceinline__ void dep_deproject(const DepthFrame& f, int i, float z, double p[3]) {
#pragma clang fp contract(off)
    const int v = i / f.width, u = i - v * f.width;
    const float tx = ((float)u - f.ppx) / f.fx;
    const float ty = ((float)v - f.ppy) / f.fy;
    const float x = z * tx;
    const float y = z * ty;
    p[0] = (double)x;
    p[1] = (double)y;
    p[2] = (double)z;
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
