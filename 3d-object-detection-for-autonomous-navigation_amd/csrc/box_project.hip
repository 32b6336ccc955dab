// Image boxes of any N camera-frame boxes over F frames, each frame with its own P2 (pp_box3d_to_bbox): labels and
// database boxes, without an engine pass.  One thread per box; the arithmetic is box_project_dev.h's, the same function
// the tail of k_postprocess calls.
#include "box_project_dev.h"
#include "pp_common.h"

// frame_start [frames + 1]: exclusive prefix of the frames' box counts (frame_start[frames] = n).  The frame of box i
// is the last f with frame_start[f] <= i -- frames without boxes are stepped over.
__global__ __launch_bounds__(256) void k_box3d_to_bbox(const double* __restrict__ boxes, long long n,
                                                       const long long* __restrict__ frame_start, int frames,
                                                       const double* __restrict__ p2, double* __restrict__ bbox) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = frames;          // invariant: frame_start[lo] <= i < frame_start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (frame_start[mid] <= i) lo = mid; else hi = mid;
    }
    double box[7], P[9], out[4];
#pragma unroll
    for (int q = 0; q < 7; ++q) box[q] = boxes[i * 7 + q];
    const double* M = p2 + (size_t)lo * 16;
#pragma unroll
    for (int r = 0; r < 3; ++r) { P[3 * r] = M[4 * r]; P[3 * r + 1] = M[4 * r + 1]; P[3 * r + 2] = M[4 * r + 2]; }
    box3d_to_bbox_dev(box, P, out);
#pragma unroll
    for (int q = 0; q < 4; ++q) bbox[i * 4 + q] = out[q];
}

void launch_box3d_to_bbox(const double* boxes, long long n, const long long* frame_start, int frames, const double* p2,
                          double* bbox, hipStream_t s) {
    if (n <= 0 || frames <= 0) return;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    PP_LAUNCH("k_box3d_to_bbox", k_box3d_to_bbox, dim3(blocks), dim3(256), 0, s, boxes, n, frame_start, frames, p2, bbox);
}
