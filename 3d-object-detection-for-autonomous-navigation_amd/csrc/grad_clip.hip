// Gradient clipping and the non-finite step guard of the optimizer step (the lines the reference's trainStep carries
// commented out above optimizer.apply_gradients, train.py:293-294: tf.clip_by_value(grad, -0.1, +0.1) and
// tf.clip_by_norm(grad, 1) per tensor; tf.clip_by_global_norm is the third published rule).  TensorFlow 2.2 is not
// vendored; the rules are restated from its documentation, per element in float32, one rounding per written operation:
//   value        g' = min(max(g, -c), c); a NaN stays a NaN
//   norm         g' = (g * c) / max(norm_tensor, c)            (TensorFlow's order; a NaN norm stays a NaN)
//   global_norm  g' = g * scale, scale = c * min(1 / norm_global, 1 / c); NaN when the norm is not finite
// g' lives in registers of the update kernel only: the gradient buffer is neither rewritten nor read a second time.
//
// Norms: per group (the caller's int per segment) the sum of (double)g * (double)g -- every term exact -- in an order
// fixed by the segment table alone:
//   k_grad_sumsq        one workgroup per PP_GNORM_CHUNK consecutive floats of one segment; a thread adds every 256th
//                       of them in index order, the wave's 64 sums meet in a butterfly, the 4 waves' in wave order ->
//                       partial[chunk] and the chunk's group beside it.  No atomics.
//   k_grad_norm_finish  ONE workgroup: a wave per group adds that group's partials (lane l takes chunks l, l + 64, ...
//                       in order, then the butterfly), wave 0 adds the group sums in group order and writes the
//                       statistics block: norms, scales, the non-finite flag and the skip decision.
// A finite float32 buffer cannot overflow the float64 sum, so !isfinite(global sum) <=> some entry is NaN or Inf.
// The update kernel reads the finished scales (and the skip decision) from that block: the host is not asked.
#include <string.h>

#include "pp_common.h"

// floats per workgroup of the reduction = per partial sum (a build-time constant: A/B builds through PP_HIPCC_EXTRA)
#ifndef PP_GNORM_CHUNK
#define PP_GNORM_CHUNK 4096
#endif
#define PP_GNORM_SEGS 128       // segments per reduction launch (its table travels as a kernel argument, 3 KB)

GradClipLayout grad_clip_layout(int64_t n_floats, int n_segments, int n_groups) {
    GradClipLayout l;
    l.stats_words = (4 + 2 * (int64_t)n_groups + 1) / 2 * 2;             // (the doubles behind it stay 8-byte aligned)
    l.max_partials = n_floats / PP_GNORM_CHUNK + n_segments;             // disjoint segments cannot need more
    l.gsum_off = l.stats_words * 4;
    l.partial_off = l.gsum_off + 8 * (int64_t)n_groups;
    l.pgroup_off = l.partial_off + 8 * l.max_partials;
    l.bytes = (l.pgroup_off + 4 * l.max_partials + 15) / 16 * 16;
    return l;
}

int64_t grad_clip_partials(const int64_t* seg, int nseg) {
    int64_t p = 0;
    for (int i = 0; i < nseg; ++i) p += (seg[2 * i + 1] + PP_GNORM_CHUNK - 1) / PP_GNORM_CHUNK;
    return p;
}

struct GnormSegs {
    int64_t off[PP_GNORM_SEGS], size[PP_GNORM_SEGS];
    int pstart[PP_GNORM_SEGS + 1];      // first chunk of segment j within this launch
    int group[PP_GNORM_SEGS];
    int n;
};

__device__ __forceinline__ double wave_sum_fixed(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

__global__ __launch_bounds__(256) void k_grad_sumsq(const float* __restrict__ g, GnormSegs t,
                                                    double* __restrict__ partial, int* __restrict__ pgroup) {
    __shared__ double wsum[4];
    const int b = (int)blockIdx.x;
    int lo = 0, hi = t.n;                                  // uniform: pstart[lo] <= b < pstart[lo + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (b >= t.pstart[mid]) lo = mid; else hi = mid;
    }
    const int64_t base = (int64_t)(b - t.pstart[lo]) * PP_GNORM_CHUNK;
    const int64_t size = t.size[lo];
    const float* __restrict__ p = g + t.off[lo];
    // every load is issued before the first add: past the segment's end the index is clamped (the launch has no
    // empty segment) and the value replaced by 0, which leaves the sum as it is
    float x[PP_GNORM_CHUNK / 256];
#pragma unroll
    for (int k = 0; k < PP_GNORM_CHUNK / 256; ++k) {
        const int64_t e = base + k * 256 + threadIdx.x;
        const float y = p[e < size ? e : size - 1];
        x[k] = e < size ? y : 0.f;
    }
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < PP_GNORM_CHUNK / 256; ++k) acc += (double)x[k] * (double)x[k];
    acc = wave_sum_fixed(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[b] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        pgroup[b] = t.group[lo];
    }
}

__device__ __forceinline__ double lane_value(double x, int k) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), k),
                            __builtin_amdgcn_readlane(__double2loint(x), k));
}

__device__ __forceinline__ float clip_global_scale(float norm, float c) {
    if (!isfinite(norm)) return __builtin_nanf("");
    return __fmul_rn(c, fminf(__fdiv_rn(1.f, norm), __fdiv_rn(1.f, c)));
}

// max(norm, c) that keeps a NaN norm (fmaxf would drop it)
__device__ __forceinline__ float clip_norm_denominator(float norm, float c) { return !(norm <= c) ? norm : c; }

__global__ __launch_bounds__(1024) void k_grad_norm_finish(const double* __restrict__ partial,
                                                           const int* __restrict__ pgroup, int P, int G,
                                                           double* gsum, float* stats, int mode, float c, int skip) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int gi = wave; gi < G; gi += 16) {
        double acc = 0.0;
#pragma unroll 4
        for (int i = lane; i < P; i += 64) {
            const double x = partial[i];
            acc += (pgroup[i] == gi) ? x : 0.0;
        }
        acc = wave_sum_fixed(acc);
        if (lane == 0) gsum[gi] = acc;
    }
    __threadfence_block();
    __syncthreads();
    if (wave != 0) return;
    double total = 0.0;                        // the group sums in group order, the same in every lane
    for (int base = 0; base < G; base += 64) {
        const double x = (base + lane < G) ? gsum[base + lane] : 0.0;
#pragma unroll
        for (int k = 0; k < 64; ++k) total += lane_value(x, k);
    }
    const float gnorm = (float)sqrt(total);
    const float gscale = (mode == PP_CLIP_GLOBAL_NORM) ? clip_global_scale(gnorm, c) : 1.f;
    for (int gi = lane; gi < G; gi += 64) {
        const float norm = (float)sqrt(gsum[gi]);
        stats[4 + gi] = norm;
        stats[4 + G + gi] = (mode == PP_CLIP_NORM) ? __fdiv_rn(c, clip_norm_denominator(norm, c)) : gscale;
    }
    if (lane == 0) {
        // nonfinite is exact (some entry is NaN or Inf).  The guard also skips a step whose finite gradient has a norm
        // beyond float32 (the float64 sum is finite, the float32 norm is Inf): global_norm would scale by NaN
        const int nonfinite = isfinite(total) ? 0 : 1;
        stats[0] = gnorm;
        stats[1] = gscale;
        reinterpret_cast<int*>(stats)[2] = nonfinite;
        reinterpret_cast<int*>(stats)[3] = (skip && (nonfinite || !isfinite(gnorm))) ? 1 : 0;
    }
}

void launch_grad_norm(const float* g, const int64_t* seg, int nseg, const int32_t* groups, int ngroups, int mode,
                      float clip, int skip, void* ws, int64_t n_floats, hipStream_t s) {
    const GradClipLayout l = grad_clip_layout(n_floats, nseg, ngroups);
    char* base = static_cast<char*>(ws);
    double* gsum = reinterpret_cast<double*>(base + l.gsum_off);
    double* partial = reinterpret_cast<double*>(base + l.partial_off);
    int* pgroup = reinterpret_cast<int*>(base + l.pgroup_off);
    int64_t pbase = 0;
    for (int done = 0; done < nseg;) {
        GnormSegs t;
        memset(&t, 0, sizeof(t));
        int blocks = 0;
        while (done < nseg && t.n < PP_GNORM_SEGS) {
            const int64_t size = seg[2 * done + 1];
            if (size > 0) {
                t.off[t.n] = seg[2 * done];
                t.size[t.n] = size;
                t.pstart[t.n] = blocks;
                t.group[t.n] = groups ? groups[done] : 0;
                blocks += (int)((size + PP_GNORM_CHUNK - 1) / PP_GNORM_CHUNK);
                ++t.n;
            }
            ++done;
        }
        for (int k = t.n; k <= PP_GNORM_SEGS; ++k) t.pstart[k] = blocks;
        if (blocks > 0)
            PP_LAUNCH("k_grad_sumsq", k_grad_sumsq, dim3((unsigned)blocks), dim3(256), 0, s, g, t, partial + pbase,
                      pgroup + pbase);
        pbase += blocks;
    }
    PP_LAUNCH("k_grad_norm_finish", k_grad_norm_finish, dim3(1), dim3(1024), 0, s, (const double*)partial,
              (const int*)pgroup, (int)pbase, ngroups, gsum, reinterpret_cast<float*>(base), mode, clip, skip);
}

// k_adamw_seg (optim.hip) on the clipped gradient: the same table, the same thread-to-element map and, from g' on, the
// same operations in the same order, so an entry is bit-identical to what k_adamw_seg makes of a buffer holding g'.
struct AdamwClipSegs {
    AdamwSegs s;                        // optim.hip's table (adamw_fill_table)
    int group[PP_ADAMW_SEGS];
};

template <int MODE>
__global__ __launch_bounds__(256) void k_adamw_seg_clip(float* __restrict__ w, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, AdamwClipSegs t,
                                                        const float* __restrict__ stats, float c, int skip,
                                                        float lr_t, float beta1, float beta2, float eps, float wd) {
    if (skip && reinterpret_cast<const int*>(stats)[3]) return;       // the guard: decided on the device, uniform
    int j = 0;
    while (j + 1 < t.s.n && (int)blockIdx.x >= t.s.block_start[j + 1]) ++j;     // uniform
    float f = 1.f;
    if (MODE == PP_CLIP_GLOBAL_NORM) f = stats[1];
    if (MODE == PP_CLIP_NORM) f = clip_norm_denominator(stats[4 + t.group[j]], c);
    const int64_t base = ((int64_t)blockIdx.x - t.s.block_start[j]) * 1024;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t e = base + k * 256 + threadIdx.x;
        if (e >= t.s.size[j]) break;
        const int64_t i = t.s.off[j] + e;
        const float wv = w[i];
        float gv = g[i];
        if (MODE == PP_CLIP_VALUE) gv = (gv != gv) ? gv : fminf(fmaxf(gv, -c), c);
        if (MODE == PP_CLIP_NORM) gv = __fdiv_rn(__fmul_rn(gv, c), f);
        if (MODE == PP_CLIP_GLOBAL_NORM) gv = __fmul_rn(gv, f);
        float mv = m[i], vv = v[i];
        const float wd_w = __fsub_rn(wv, __fmul_rn(wd, wv));
        mv = __fadd_rn(__fmul_rn(beta1, mv), __fmul_rn(1.f - beta1, gv));
        vv = __fadd_rn(__fmul_rn(beta2, vv), __fmul_rn(1.f - beta2, __fmul_rn(gv, gv)));
        w[i] = __fsub_rn(wd_w, __fdiv_rn(__fmul_rn(lr_t, mv), __fadd_rn(__fsqrt_rn(vv), eps)));
        m[i] = mv;
        v[i] = vv;
    }
}

void launch_adamw_segments_clipped(float* w, const float* g, float* m, float* v, const int64_t* seg, int nseg,
                                   const int32_t* groups, int ngroups, int mode, float clip, int skip, const void* ws,
                                   float lr_t, float beta1, float beta2, float eps, float wd, hipStream_t s) {
    const float* stats = static_cast<const float*>(ws);
    for (int done = 0; done < nseg;) {
        AdamwClipSegs t;
        int src[PP_ADAMW_SEGS];
        const int blocks = adamw_fill_table(t.s, seg, nseg, &done, src);
        for (int j = 0; j < PP_ADAMW_SEGS; ++j) t.group[j] = (groups && j < t.s.n) ? groups[src[j]] : 0;
        if (blocks <= 0) continue;
        const dim3 grid((unsigned)blocks), block(256);
        switch (mode) {
        case PP_CLIP_VALUE:
            PP_LAUNCH("k_adamw_seg_clip", k_adamw_seg_clip<PP_CLIP_VALUE>, grid, block, 0, s, w, g, m, v, t, stats, clip,
                      skip, lr_t, beta1, beta2, eps, wd);
            break;
        case PP_CLIP_NORM:
            PP_LAUNCH("k_adamw_seg_clip", k_adamw_seg_clip<PP_CLIP_NORM>, grid, block, 0, s, w, g, m, v, t, stats, clip,
                      skip, lr_t, beta1, beta2, eps, wd);
            break;
        case PP_CLIP_GLOBAL_NORM:
            PP_LAUNCH("k_adamw_seg_clip", k_adamw_seg_clip<PP_CLIP_GLOBAL_NORM>, grid, block, 0, s, w, g, m, v, t, stats,
                      clip, skip, lr_t, beta1, beta2, eps, wd);
            break;
        default:
            PP_LAUNCH("k_adamw_seg_clip", k_adamw_seg_clip<PP_CLIP_NONE>, grid, block, 0, s, w, g, m, v, t, stats, clip,
                      skip, lr_t, beta1, beta2, eps, wd);
        }
    }
}
