// Rotated-box overlaps of the KITTI-style AP evaluator.
//
// Replaces rotate_iou_gpu_eval / rotate_iou_kernel_eval and their device functions
// (reference second/core/non_max_suppression/nms_gpu.py:180-415, :564-653: numba-CUDA) and
// d3_box_overlap (second/utils/eval.py:132-163):
//   out[n][k] = inter(query[k], box[n]) / {a1 + a2 - inter | a1 | a2 | 1}     criterion -1 | 0 | 1 | 2
// where inter() clips two rotated rectangles: corners of each inside the other (>= tests), the 16
// edge/edge intersections, an angular insertion sort about the centroid, a triangle fan.  Every
// operation is float32 in the reference's order (no contraction: the library is built with
// -ffp-contract=off); cos / sin / sqrt are evaluated in double and rounded, like math.cos on a
// float32 scalar.  The 3D overlap multiplies the BEV intersection by the height overlap in float64.
//
// Mapping: k_riou_corners turns every box into 8 corner floats + area once (N + K threads, the
// double-precision sincos is the expensive part); k_riou_pairs runs one thread per (n, k) pair,
// 64 consecutive k per wavefront so the [N][K] output rows are written in full 256-byte segments.
// The rectangle clip itself (riou_dev.h) is shared with the rotated NMS: the per-thread polygon (<= 8 points) and its
// sort keys live in LDS in a [slot][thread] layout.
#include "riou_dev.h"

#define RIOU_TX 64
#define RIOU_TY 4

__global__ __launch_bounds__(256) void k_riou_corners(const float* __restrict__ boxes, int64_t n, float* __restrict__ corners) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* r = boxes + 5 * i;
    riou_box_corners(r[0], r[1], r[2], r[3], r[4], corners + 9 * i);
}

// criterion: -1 IoU, 0 / query area, 1 / box area, 2 raw intersection area
__global__ __launch_bounds__(RIOU_TX * RIOU_TY) void k_riou_pairs(const float* __restrict__ bc, int64_t N,
                                                                  const float* __restrict__ qc, int64_t K,
                                                                  int criterion, float* __restrict__ out) {
    __shared__ float s_px[RIOU_MAXP][RIOU_TX * RIOU_TY];
    __shared__ float s_py[RIOU_MAXP][RIOU_TX * RIOU_TY];
    __shared__ float s_vs[RIOU_MAXP][RIOU_TX * RIOU_TY];
    const int t = threadIdx.y * RIOU_TX + threadIdx.x;
    const int64_t k = (int64_t)blockIdx.x * RIOU_TX + threadIdx.x;
    const int64_t n = (int64_t)blockIdx.y * RIOU_TY + threadIdx.y;
    if (k >= K || n >= N) return;
    float c1[8], c2[8];   // c1: query (first argument of devRotateIoUEval), c2: box
#pragma unroll
    for (int j = 0; j < 8; ++j) { c1[j] = qc[9 * k + j]; c2[j] = bc[9 * n + j]; }
    const float area1 = qc[9 * k + 8], area2 = bc[9 * n + 8];

    const float area = riou_clip_area<RIOU_TX * RIOU_TY>(c1, c2, &s_px[0][0], &s_py[0][0], &s_vs[0][0], t);
    float v;
    if (criterion == -1) v = __fdiv_rn(area, __fsub_rn(__fadd_rn(area1, area2), area));
    else if (criterion == 0) v = __fdiv_rn(area, area1);
    else if (criterion == 1) v = __fdiv_rn(area, area2);
    else v = area;
    out[n * K + k] = v;
}

// d3_box_overlap_kernel (eval.py:132-156): camera boxes [x, y, z, l, h, w, ry] float64; rinc = BEV intersection
__global__ __launch_bounds__(256) void k_d3_finish(const double* __restrict__ boxes, int64_t N,
                                                   const double* __restrict__ qboxes, int64_t K, int criterion,
                                                   const float* __restrict__ rinc, double* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = blockIdx.y;
    if (k >= K) return;
    const double r = (double)rinc[n * K + k];
    double res = r;
    if (r > 0.0) {
        const double* b = boxes + 7 * n;
        const double* q = qboxes + 7 * k;
        const double iw = fmin(b[1], q[1]) - fmax(b[1] - b[4], q[1] - q[4]);
        if (iw > 0.0) {
            const double a1 = b[3] * b[4] * b[5], a2 = q[3] * q[4] * q[5];
            const double inc = iw * r;
            double ua;
            if (criterion == -1) ua = a1 + a2 - inc;
            else if (criterion == 0) ua = a1;
            else if (criterion == 1) ua = a2;
            else ua = 1.0;
            res = inc / ua;
        } else {
            res = 0.0;
        }
    }
    out[n * K + k] = res;
}

void launch_riou_corners(const float* boxes, int64_t n, float* corners, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_riou_corners, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, boxes, n, corners);
}

void launch_riou_pairs(const float* bc, int64_t N, const float* qc, int64_t K, int criterion, float* out, hipStream_t s) {
    if (N <= 0 || K <= 0) return;
    dim3 grid((unsigned)((K + RIOU_TX - 1) / RIOU_TX), (unsigned)((N + RIOU_TY - 1) / RIOU_TY));
    hipLaunchKernelGGL(k_riou_pairs, grid, dim3(RIOU_TX, RIOU_TY), 0, s, bc, N, qc, K, criterion, out);
}

void launch_d3_finish(const double* boxes, int64_t N, const double* qboxes, int64_t K, int criterion, const float* rinc,
                      double* out, hipStream_t s) {
    if (N <= 0 || K <= 0) return;
    dim3 grid((unsigned)((K + 255) / 256), (unsigned)N);
    hipLaunchKernelGGL(k_d3_finish, grid, dim3(256), 0, s, boxes, N, qboxes, K, criterion, rinc, out);
}
