// Frustum crop (pp_frustum_crop*): the resident frames [n_b, F] -> the points inside the camera image's frustum, each
// frame compacted in its own order, frames back to back.  Restates box_np_ops.remove_outside_points' per-point half
// (second/core/geometry.py points_in_convex_polygon_3d_jit); the six planes per frame are the host's (frustum.py: a
// LAPACK inverse and a QR stand behind them):
//
//   s_k = ((x n0 + y n1) + z n2) + d of face k, in float64 on the widened float32 coordinates, summed left to right,
//   products and sums rounded separately;
//   a point is removed iff s_k >= 0 for some face -- kept iff !(s_k >= 0) for all six, so a NaN coordinate is kept;
//   `back`: column 0 is negated first (exact), tested negated and stored negated;
//   a kept row is copied whole, all F columns, bit for bit.
//
// Three launches, ordered by the stream alone (no workgroup waits for another, no slot is claimed with an atomic: the
// same input gives the same bytes):
//   k_crop_count    one wave per chunk of CROP_CHUNK points: ballot + popcount of the keep flags -> chunk counts
//   k_crop_scan     one workgroup: a wave per frame scans its chunk counts -> chunk bases and the frame's kept count;
//                   then the packed output offsets
//   k_crop_scatter  repeats the test; a kept point's row is offset[frame] + its chunk's base + the kept lanes below it
// Bandwidth-bound: 4 F bytes per point read twice, the kept part written once.  A frame's 24 plane values are read
// through a wave-uniform address (scalar loads: they sit in SGPRs).
#include "pp_common.h"

namespace {

constexpr int CROP_ITER = 4;                       // 64-point steps of a wave
constexpr int CROP_CHUNK = PP_WAVE * CROP_ITER;    // points per chunk (one wave)
constexpr int CROP_WAVES = 4;                      // chunks per workgroup

struct CropPlanes { double v[24]; };

__device__ __forceinline__ CropPlanes crop_planes(const double* __restrict__ planes, int b) {
    CropPlanes pl;
#pragma unroll
    for (int i = 0; i < 24; ++i) pl.v[i] = planes[(size_t)b * 24 + i];
    return pl;
}

__device__ __forceinline__ bool crop_keep(float xf, float yf, float zf, const CropPlanes& pl) {
#pragma clang fp contract(off)
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    bool keep = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double s = ((x * pl.v[4 * k] + y * pl.v[4 * k + 1]) + z * pl.v[4 * k + 2]) + pl.v[4 * k + 3];
        keep = keep && !(s >= 0.0);                // (not `s < 0`: a NaN survives every face)
    }
    return keep;
}

// A row of FT floats moved with the widest access its width allows: one 16-byte access for FT == 4 (VEC: both buffers
// sit on 16 bytes), one 12-byte access for FT == 3; FT == 0: any width F, a float at a time.
struct __attribute__((aligned(4))) CropRow3 { float v[3]; };
constexpr int CROP_MAX_F = 16;     // widest row the FT == 0 scatter holds in registers (the host refuses more)

template <int FT, bool VEC>
__device__ __forceinline__ void crop_load_xyz(const float* __restrict__ p, int F, float r[3]) {
    if (FT == 4 && VEC) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        r[0] = q.x; r[1] = q.y; r[2] = q.z;
    } else if (FT == 3) {
        const CropRow3 q = *reinterpret_cast<const CropRow3*>(p);
        r[0] = q.v[0]; r[1] = q.v[1]; r[2] = q.v[2];
    } else {
        r[0] = p[0]; r[1] = p[1]; r[2] = p[2];
    }
}

template <int FT, bool VEC>
__global__ __launch_bounds__(PP_WAVE * CROP_WAVES) void k_crop_count(const float* __restrict__ in,
                                                                    const int* __restrict__ offsets_in,
                                                                    const double* __restrict__ planes, int F, int stride,
                                                                    int back, int* __restrict__ chunk_cnt) {
    const int b = blockIdx.y;
    const int row0 = offsets_in[b], n = offsets_in[b + 1] - row0;
    const int lane = threadIdx.x & (PP_WAVE - 1);
    const int c = blockIdx.x * CROP_WAVES + (threadIdx.x >> 6);
    if (c * CROP_CHUNK >= n) return;               // (the same for every lane of the wave)
    const CropPlanes pl = crop_planes(planes, b);
    const int Fr = FT ? FT : F;
    const float* base = in + (size_t)row0 * Fr;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < CROP_ITER; ++k) {
        const int i = c * CROP_CHUNK + k * PP_WAVE + lane;
        bool keep = false;
        if (i < n) {
            float r[3];
            crop_load_xyz<FT, VEC>(base + (size_t)i * Fr, Fr, r);
            keep = crop_keep(back ? -r[0] : r[0], r[1], r[2], pl);
        }
        cnt += __popcll(__ballot(keep));
    }
    if (lane == 0) chunk_cnt[(size_t)b * stride + c] = cnt;
}

// One workgroup of 16 waves; wave w scans frames w, w + 16, ...; thread 0 then sums the kept counts into the offsets.
__global__ __launch_bounds__(1024) void k_crop_scan(const int* __restrict__ offsets_in, int batch, int stride,
                                                    const int* __restrict__ chunk_cnt, int* __restrict__ chunk_base,
                                                    int* __restrict__ kept, int* __restrict__ offsets_out) {
    const int lane = threadIdx.x & (PP_WAVE - 1), wave = threadIdx.x >> 6;
    for (int b = wave; b < batch; b += 16) {
        const int n = offsets_in[b + 1] - offsets_in[b];
        const int nchunks = (n + CROP_CHUNK - 1) / CROP_CHUNK;
        int carry = 0;
        for (int c0 = 0; c0 < nchunks; c0 += PP_WAVE) {
            const int c = c0 + lane;
            const int v = c < nchunks ? chunk_cnt[(size_t)b * stride + c] : 0;
            const int incl = wave_inclusive_scan(v);
            if (c < nchunks) chunk_base[(size_t)b * stride + c] = carry + incl - v;
            carry += __builtin_amdgcn_readlane(incl, PP_WAVE - 1);
        }
        if (lane == 0) kept[b] = carry;
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        int off = 0;
        offsets_out[0] = 0;
        for (int b = 0; b < batch; ++b) { off += kept[b]; offsets_out[b + 1] = off; }
    }
}

template <int FT, bool VEC>
__global__ __launch_bounds__(PP_WAVE * CROP_WAVES) void k_crop_scatter(const float* __restrict__ in,
                                                                      const int* __restrict__ offsets_in,
                                                                      const double* __restrict__ planes, int F, int stride,
                                                                      int back, const int* __restrict__ chunk_base,
                                                                      const int* __restrict__ offsets_out,
                                                                      float* __restrict__ out, long long out_rows) {
    const int b = blockIdx.y;
    const int row0 = offsets_in[b], n = offsets_in[b + 1] - row0;
    const int lane = threadIdx.x & (PP_WAVE - 1);
    const int c = blockIdx.x * CROP_WAVES + (threadIdx.x >> 6);
    if (c * CROP_CHUNK >= n) return;
    const CropPlanes pl = crop_planes(planes, b);
    const int Fr = FT ? FT : F;
    const float* base = in + (size_t)row0 * Fr;
    const long long orow0 = offsets_out[b];
    int run = chunk_base[(size_t)b * stride + c];
    const unsigned long long below = (1ull << lane) - 1ull;
    constexpr int NR = FT ? FT : CROP_MAX_F;
#pragma unroll
    for (int k = 0; k < CROP_ITER; ++k) {
        const int i = c * CROP_CHUNK + k * PP_WAVE + lane;
        float r[NR];
        bool keep = false;
        if (i < n) {
            const float* p = base + (size_t)i * Fr;
            if (FT == 4 && VEC) {
                const float4 q = *reinterpret_cast<const float4*>(p);
                r[0] = q.x; r[1] = q.y; r[2] = q.z; r[3] = q.w;
            } else if (FT == 3) {
                const CropRow3 q = *reinterpret_cast<const CropRow3*>(p);
                r[0] = q.v[0]; r[1] = q.v[1]; r[2] = q.v[2];
            } else {
#pragma unroll
                for (int j = 0; j < NR; ++j) if (j < Fr) r[j] = p[j];
            }
            if (back) r[0] = -r[0];
            keep = crop_keep(r[0], r[1], r[2], pl);
        }
        const unsigned long long m = __ballot(keep);
        const long long row = orow0 + run + __popcll(m & below);
        run += __popcll(m);
        if (keep && row < out_rows) {              // (always: a frame keeps no more than it holds)
            float* o = out + (size_t)row * Fr;
            if (FT == 4 && VEC) {
                *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
            } else if (FT == 3) {
                CropRow3 q;
                q.v[0] = r[0]; q.v[1] = r[1]; q.v[2] = r[2];
                *reinterpret_cast<CropRow3*>(o) = q;
            } else {
#pragma unroll
                for (int j = 0; j < NR; ++j) if (j < Fr) o[j] = r[j];
            }
        }
    }
}

template <int FT, bool VEC>
void crop_launch(const CropParams& p, hipStream_t s) {
    const dim3 grid((p.stride + CROP_WAVES - 1) / CROP_WAVES, p.batch), block(PP_WAVE * CROP_WAVES);
    if (p.stride > 0)
        PP_LAUNCH("k_crop_count", (k_crop_count<FT, VEC>), grid, block, 0, s, p.in, p.offsets_in, p.planes, p.F, p.stride,
                  p.back, p.chunk_cnt);
    PP_LAUNCH("k_crop_scan", k_crop_scan, dim3(1), dim3(1024), 0, s, p.offsets_in, p.batch, p.stride, p.chunk_cnt,
              p.chunk_base, p.kept, p.offsets_out);
    if (p.stride > 0)
        PP_LAUNCH("k_crop_scatter", (k_crop_scatter<FT, VEC>), grid, block, 0, s, p.in, p.offsets_in, p.planes, p.F,
                  p.stride, p.back, p.chunk_base, p.offsets_out, p.out, p.out_rows);
}

}  // namespace

int crop_chunks(int n) { return (n + CROP_CHUNK - 1) / CROP_CHUNK; }
int crop_max_features() { return CROP_MAX_F; }

void launch_frustum_crop(const CropParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    const bool vec = (((uintptr_t)p.in | (uintptr_t)p.out) & 15) == 0;
    if (p.F == 4 && vec) crop_launch<4, true>(p, s);
    else if (p.F == 3) crop_launch<3, false>(p, s);
    else crop_launch<0, false>(p, s);
}
