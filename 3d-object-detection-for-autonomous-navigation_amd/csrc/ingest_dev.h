// What the live-camera ingests share on the device (ingest.hip; PointCloud2 messages, raw depth images, and rigs of several
// sources of either kind per frame): the chunking, the unaligned dword load, the per-record decode and validity of both
// feeds, the float64 camera -> lidar transform, and ONE body per phase -- ing_count_chunk, ing_scan_chunks,
// ing_scatter_chunk -- written against three per-frame-type overloads (ing_records, ing_probe, ing_point).  The kernels of
// ingest.hip only say where a chunk's record, selection, matrices and first output row come from.
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

// ---- what the phase bodies need of either record type: records in all; validity of record i plus what its point is
// computed from (a PointCloud2 record: its three coordinates; a depth pixel: its float32 z, so that only kept pixels pay
// dep_deproject's divisions); the float64 camera-frame point of a kept record
template <typename Frame> struct IngProbe;
template <> struct IngProbe<IngFrame> { double p[3]; };
template <> struct IngProbe<DepthFrame> { float z = 0.0f; };
__device__ __forceinline__ int ing_records(const IngFrame& f) { return f.n_rec; }
__device__ __forceinline__ int ing_records(const DepthFrame& f) { return f.n_pix; }
__device__ __forceinline__ bool ing_probe(const uint8_t* base, const IngFrame& f, int i, IngProbe<IngFrame>& s) {
    return ing_read(base, f, i, s.p);
}
__device__ __forceinline__ bool ing_probe(const uint8_t* base, const DepthFrame& f, int i, IngProbe<DepthFrame>& s) {
    return dep_read(base, f, i, s.z);
}
__device__ __forceinline__ void ing_point(const IngFrame&, int, const IngProbe<IngFrame>& s, double p[3]) {
    p[0] = s.p[0]; p[1] = s.p[1]; p[2] = s.p[2];
}
__device__ __forceinline__ void ing_point(const DepthFrame& f, int i, const IngProbe<DepthFrame>& s, double p[3]) {
    dep_deproject(f, i, s.z, p);
}

// the chunk of this wave (grid.x * ING_WAVES chunks per record, grid.y records; the same for every lane of the wave)
__device__ __forceinline__ int ing_wave_chunk() { return blockIdx.x * ING_WAVES + (threadIdx.x >> 6); }

// The count body: one wave per chunk of ING_CHUNK records of record `y` (a frame, or a source of a rig): ballot + popcount
// of the valid flags -> chunk_cnt[y][chunk].
template <typename Frame>
__device__ __forceinline__ void ing_count_chunk(const uint8_t* __restrict__ raw, const Frame* __restrict__ frames, int stride,
                                                int* __restrict__ chunk_cnt) {
    const int y = blockIdx.y;
    const Frame f = frames[y];
    const int lane = threadIdx.x & (PP_WAVE - 1);
    const int c = ing_wave_chunk();
    if (c >= f.nchunks) return;
    const uint8_t* base = raw + f.byte_off;
    const int n = ing_records(f);
    int cnt = 0;
#pragma unroll 2
    for (int k = 0; k < ING_ITER; ++k) {
        const int i = c * ING_CHUNK + k * PP_WAVE + lane;
        IngProbe<Frame> s;
        const bool ok = i < n && ing_probe(base, f, i, s);
        cnt += __popcll(__ballot(ok));
    }
    if (lane == 0) chunk_cnt[(size_t)y * stride + c] = cnt;
}

// The scan body, for one wave: a record's chunk counts -> the valid records in front of each chunk; returns their sum
// (the same in every lane).
__device__ __forceinline__ int ing_scan_chunks(const int* __restrict__ cnt, int* __restrict__ base, size_t row, int nchunks) {
    const int lane = threadIdx.x & (PP_WAVE - 1);
    int carry = 0;
    for (int c0 = 0; c0 < nchunks; c0 += PP_WAVE) {
        const int c = c0 + lane;
        const int v = c < nchunks ? cnt[row + c] : 0;
        const int incl = wave_inclusive_scan(v);
        if (c < nchunks) base[row + c] = carry + incl - v;
        carry += __builtin_amdgcn_readlane(incl, PP_WAVE - 1);
    }
    return carry;
}

// points kept of `valid` under a selection
__device__ __forceinline__ int ing_kept(int valid, int first, int decimate) {
    return valid > first ? (valid - first + decimate - 1) / decimate : 0;
}

// The body of a one-workgroup scan kernel of 16 waves (1024 threads) of a plain call: wave w scans the chunk counts of
// frames w, w + 16, ... into chunk bases and the frame's finite (valid) and kept counts; thread 0 then sums the kept
// counts into the offsets.
template <typename Frame>
__device__ __forceinline__ void ingest_scan_frames(const Frame* __restrict__ frames, int batch, int stride, int first,
                                                   int decimate, const int* __restrict__ chunk_cnt,
                                                   int* __restrict__ chunk_base, int* __restrict__ finite,
                                                   int* __restrict__ kept, int* __restrict__ offsets) {
    const int lane = threadIdx.x & (PP_WAVE - 1), wave = threadIdx.x >> 6;
    for (int b = wave; b < batch; b += 16) {
        const int carry = ing_scan_chunks(chunk_cnt, chunk_base, (size_t)b * stride, frames[b].nchunks);
        if (lane == 0) {
            finite[b] = carry;
            kept[b] = ing_kept(carry, first, decimate);
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

inline IngXform ing_xform_of(const double* r, const double* r2, const double* lift) {
    IngXform xf;
    for (int i = 0; i < 9; ++i) { xf.r[i] = r[i]; xf.r2[i] = r2[i]; }
    for (int i = 0; i < 3; ++i) xf.lift[i] = lift[i];
    return xf;
}

// the F - 3 feature columns of one record of a _fields call (none for F = 3)
template <int N> struct IngCols { IngFeat c[N]; };
template <> struct IngCols<0> {};

// The scatter body: re-reads chunk c of record f; a valid record's rank is `run` (the valid records of f in front of the
// chunk) + the valid lanes below it + the steps before; it is kept when rank >= first and (rank - first) % decimate == 0,
// as row row0 + (rank - first) / decimate of `out`: its point, transformed, and for F > 3 (PointCloud2 only) its feature
// columns behind it -- three dword stores for F = 3, one 16-byte store for F = 4.
// row0 >= 0 (a rank never lowers a row: the callers' concern).
// Everything is taken by value: by reference costs the PointCloud2 instantiations one more computation of the record's
// address per step.
template <typename Frame, int F>
__device__ __forceinline__ void ing_scatter_chunk(const uint8_t* __restrict__ base, const Frame f, int c, int run, int first,
                                                  int decimate, const IngXform xf, const IngCols<F - 3> ft, long long row0,
                                                  float* __restrict__ out, long long out_rows) {
    const int lane = threadIdx.x & (PP_WAVE - 1);
    const int n = ing_records(f);
    const unsigned long long below = (1ull << lane) - 1ull;
    // a PointCloud2 chunk's eight steps are unrolled (eight records' loads in flight), a depth chunk's are not: said here,
    // so that a row width or a frame type more does not leave it to the unroller's size estimate
    constexpr int steps_unrolled = std::is_same<Frame, IngFrame>::value ? ING_ITER : 1;
#pragma unroll steps_unrolled
    for (int k = 0; k < ING_ITER; ++k) {
        const int i = c * ING_CHUNK + k * PP_WAVE + lane;
        IngProbe<Frame> s;
        const bool ok = i < n && ing_probe(base, f, i, s);
        const unsigned long long m = __ballot(ok);
        const int r = run + __popcll(m & below) - first;
        run += __popcll(m);
        if (ok && r >= 0 && r % decimate == 0) {
            const long long row = row0 + r / decimate;
            if (row < out_rows) {                  // (always: the host sized the call from the records' bounds)
                double p[3];
                float o[F];
                ing_point(f, i, s, p);
                ing_transform(p, xf, o);
                if constexpr (F > 3) {
                    const uint8_t* rec = ing_record(base, f, i);
#pragma unroll
                    for (int j = 0; j < F - 3; ++j) o[3 + j] = ing_feature(rec, ft.c[j], f.big_endian != 0);
                }
                ing_store_row<F>(out, row, o);
            }
        }
    }
}
