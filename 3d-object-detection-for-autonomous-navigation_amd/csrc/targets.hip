// Training targets from ground-truth boxes (SURVEY section 8f, row f3 -- data half): the reference's
// create_target_np (load_data.py:331-532) through assign (:267-293), as the loader calls it (:3086-3101: anchors
// pruned by the frame's anchors_mask, no positive-fraction sampling, norm_by_num_examples=False, box code size 7),
// restated in target_assigner.py.  Bit-exact: every value is computed in the float32 operation order of the numpy
// code (the build has -ffp-contract=off; division and sqrt are IEEE), so the equality tests of the matching rule
// see the same numbers as on the host.
//
// Pass 1, a thread per (frame, anchor): the nearest-box IoU against every box of the frame, max-reduced per box over
// the kept anchors (the overlaps are >= 0, so their float bits order as unsigned integers).  Pass 2 recomputes the
// same overlaps and applies the rule:
//   forced  = some box g has iou[a, g] == top[g] > 0            (a box's best anchors, ties included)
//   label   = forced || best >= matched ? class[best_gt] : best < unmatched ? 0 : -1
//   targets = second_box_encode(gt[best_gt], anchor) for label > 0, else 0
// with best_gt the FIRST maximum of the anchor's row (numpy argmax) -- also for a forced anchor (the reference's
// labels[forced] = gt_classes[best_gt[forced]]).  Masked-out anchors: -1; a frame without boxes: 0.
#include <math.h>

#include "pp_common.h"

namespace {

// rbbox2d_to_near_bbox (load_data.py:535-551) of one (x, y, xdim, ydim, rad) box, float32: limit_period(r, 0.5, pi)
// (:805-806) and |.| > pi / 4 picks the standing or the lying box
__device__ __forceinline__ float4 near_box(float x, float y, float w, float l, float r) {
    const float pi = 3.14159265358979323846f;
    const float lp = r - floorf(r / pi + 0.5f) * pi;
    const bool swap = fabsf(lp) > 0.785398163397448309616f;
    const float dx = swap ? l : w, dy = swap ? w : l;
    return make_float4(x - dx / 2.0f, y - dy / 2.0f, x + dx / 2.0f, y + dy / 2.0f);
}

__device__ __forceinline__ float box_area(float4 b) { return (b.z - b.x) * (b.w - b.y); }

// iou_jit (load_data.py:206-235, eps 0): boxes = the anchor, query = the ground-truth box
__device__ __forceinline__ float near_iou(float4 a, float area_a, float4 g, float area_g) {
    const float iw = fminf(a.z, g.z) - fmaxf(a.x, g.x);
    const float ih = fminf(a.w, g.w) - fmaxf(a.y, g.y);
    if (!(iw > 0.f && ih > 0.f)) return 0.f;
    const float inter = iw * ih;
    const float ua = (area_a + area_g) - inter;
    return inter / ua;
}

// the frame's boxes as near boxes + areas (+ classes and per-box maxima for pass 2) in LDS; returns the box count
struct FrameBoxes {
    float4 nb[PP_MAX_GT_PER_FRAME];
    float area[PP_MAX_GT_PER_FRAME];
    float top[PP_MAX_GT_PER_FRAME];
    int cls[PP_MAX_GT_PER_FRAME];
};

__device__ __forceinline__ int stage_boxes(const TargetParams& p, int b, FrameBoxes& s, bool pass2, int* first) {
    int g0 = 0;
    for (int i = 0; i < b; ++i) g0 += p.gt_cnt[i];
    const int G = min(p.gt_cnt[b], PP_MAX_GT_PER_FRAME);
    for (int g = threadIdx.x; g < G; g += blockDim.x) {
        const float* q = p.gt + (size_t)(g0 + g) * 7;
        const float4 n = near_box(q[0], q[1], q[3], q[4], q[6]);
        s.nb[g] = n;
        s.area[g] = box_area(n);
        if (pass2) {
            s.top[g] = __uint_as_float(p.top[(size_t)b * PP_MAX_GT_PER_FRAME + g]);
            s.cls[g] = p.gt_cls ? p.gt_cls[g0 + g] : 1;
        }
    }
    *first = g0;
    __syncthreads();
    return G;
}

__global__ __launch_bounds__(256) void k_anchor_near(const float* __restrict__ anchors, int64_t A, float4* __restrict__ out) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    const float* q = anchors + a * 7;
    out[a] = near_box(q[0], q[1], q[3], q[4], q[6]);
}

// pass 1: per box, the largest overlap with a kept anchor of its frame
__global__ __launch_bounds__(256) void k_tgt_top(TargetParams p) {
    __shared__ FrameBoxes s;
    const int b = blockIdx.y;
    if (p.gt_cnt[b] <= 0) return;                                   // (uniform over the workgroup)
    int g0;
    const int G = stage_boxes(p, b, s, false, &g0);
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool kept = a < p.A && (p.mask == nullptr || p.mask[(size_t)b * p.A + a] != 0);
    if (!__syncthreads_or(kept)) return;
    const float4 an = kept ? p.anchor_near[a] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float aa = box_area(an);
    unsigned* top = p.top + (size_t)b * PP_MAX_GT_PER_FRAME;
    for (int g = 0; g < G; ++g) {
        const float v = kept ? near_iou(an, aa, s.nb[g], s.area[g]) : 0.f;
        const bool pos = v > 0.f;
        if (__ballot(pos) == 0) continue;                           // most boxes are far from most of a wave's anchors
        unsigned u = pos ? __float_as_uint(v) : 0u;
        for (int off = 32; off > 0; off >>= 1) u = max(u, (unsigned)__shfl_xor((int)u, off));
        if ((threadIdx.x & 63) == 0) atomicMax(top + g, u);
    }
}

// pass 2: labels and regression targets (second_box_encode, load_data.py:125-203, in target_assigner.second_box_encode's
// float32 order; log in double, rounded once)
__global__ __launch_bounds__(256) void k_tgt_assign(TargetParams p) {
    __shared__ FrameBoxes s;
    const int b = blockIdx.y;
    int g0;
    const int G = stage_boxes(p, b, s, true, &g0);
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= p.A) return;
    const size_t idx = (size_t)b * p.A + a;
    const bool kept = p.mask == nullptr || p.mask[idx] != 0;
    int label = -1, best_gt = -1;
    float best = kept ? 0.f : -1.f;
    float t[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (kept && G == 0) label = 0;
    if (kept && G > 0) {
        const float4 an = p.anchor_near[a];
        const float aa = box_area(an);
        bool forced = false;
        for (int g = 0; g < G; ++g) {
            const float v = near_iou(an, aa, s.nb[g], s.area[g]);
            if (g == 0 || v > best) { best = v; best_gt = g; }
            forced = forced || (v == s.top[g] && s.top[g] > 0.f);
        }
        label = (forced || best >= p.matched) ? s.cls[best_gt] : (best < p.unmatched ? 0 : -1);
        if (label > 0) {
            const float* q = p.anchors + a * 7;
            const float* r = p.gt + (size_t)(g0 + best_gt) * 7;
            const float za = q[2] + q[5] / 2.0f, zg = r[2] + r[5] / 2.0f;
            const float diag = sqrtf(q[4] * q[4] + q[3] * q[3]);
            t[0] = (r[0] - q[0]) / diag;
            t[1] = (r[1] - q[1]) / diag;
            t[2] = (zg - za) / q[5];
            t[3] = (float)log((double)(r[3] / q[3]));
            t[4] = (float)log((double)(r[4] / q[4]));
            t[5] = (float)log((double)(r[5] / q[5]));
            t[6] = r[6] - q[6];
        }
    }
    p.labels[idx] = label;
    float* out = p.reg_targets + idx * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) out[k] = t[k];
    if (p.gt_index) p.gt_index[idx] = best_gt;
    if (p.overlap) p.overlap[idx] = best;
}

}  // namespace

void launch_anchor_near(const float* anchors, int64_t A, float4* near, hipStream_t s) {
    if (A <= 0) return;
    hipLaunchKernelGGL(k_anchor_near, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, s, anchors, A, near);
}

void launch_targets(const TargetParams& p, hipStream_t s) {
    if (p.batch <= 0 || p.A <= 0) return;
    const dim3 grid((unsigned)((p.A + 255) / 256), (unsigned)p.batch);
    PP_LAUNCH("k_tgt_top", k_tgt_top, grid, dim3(256), 0, s, p);
    PP_LAUNCH("k_tgt_assign", k_tgt_assign, grid, dim3(256), 0, s, p);
}
