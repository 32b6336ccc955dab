// Rotated-box NMS (what the rotated-IoU kernel "also unlocks").
//
// Replaces rotate_nms_gpu -> rotate_nms_kernel -> nms_postprocess (reference
// second/core/non_max_suppression/nms_gpu.py:419-490, :111-128: numba-CUDA + a host sweep) with the pre / post caps of
// nms() around it (libraries/eval_helper_functions.py:463-492):
//   order  = boxes by descending score (ties: lower index first -- the reference's argsort()[::-1] leaves them
//            implementation-defined), cut to the first m = min(n, pre_max)
//   mask   : bit j of mask[i][j / 64] = devRotateIoU(box_i, box_j) > thr for sorted positions j > i.  box_i, the
//            higher-scoring one, is the FIRST argument (the float32 clip is not symmetric bit for bit); strict >, so a
//            NaN IoU (two zero-area boxes) suppresses nothing
//   sweep  : boxes walked in order, a box not yet removed is kept and ORs its mask row into the removed set; at most
//            post_max kept; the kept positions are returned as order[position], indices into the caller's array.
//
// Mapping: k_rnms_rank ranks by counting (n^2 compares against n^2 / 2 polygon clips) and writes the sorted boxes;
// k_riou_corners (rotate_iou.hip) turns them into corners + area once; k_rnms_mask computes one 64 x 64 tile of the
// mask per workgroup, only tiles with col_block >= row_block (the sweep never reads the others): 256 threads = 64 rows
// x 4 quarters of the tile's columns, the column boxes staged in LDS, the clip of riou_dev.h; k_rnms_sweep is one
// wavefront with the removed-set words spread over its lanes (PP_RNMS_MAX_BOXES / 64 / 64 = 4 words per lane).
#include "riou_dev.h"

#define RNMS_TILE 64
#define RNMS_Q 4          // column quarters of a tile (threadIdx.y)
#define RNMS_WPL (PP_RNMS_MAX_BOXES / 64 / 64)   // removed-set words per lane of the sweep

static_assert(PP_RNMS_MAX_BOXES % (64 * 64) == 0, "the sweep spreads PP_RNMS_MAX_BOXES / 64 words over 64 lanes");

// rank of box i = boxes with a higher score, or the same score and a lower index; the first m ranks are written
__global__ __launch_bounds__(256) void k_rnms_rank(const float* __restrict__ dets, int n, int m, int* __restrict__ order,
                                                   float* __restrict__ sorted) {
    __shared__ float s_sc[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float me = (i < n) ? dets[6 * (size_t)i + 5] : 0.f;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + threadIdx.x;
        __syncthreads();
        s_sc[threadIdx.x] = (j < n) ? dets[6 * (size_t)j + 5] : 0.f;
        __syncthreads();
        const int cnt = min(256, n - j0);
        for (int k = 0; k < cnt; ++k) {
            const float o = s_sc[k];
            rank += (o > me || (o == me && j0 + k < i)) ? 1 : 0;
        }
    }
    if (i < n && rank < m) {
        order[rank] = i;
#pragma unroll
        for (int q = 0; q < 5; ++q) sorted[5 * (size_t)rank + q] = dets[6 * (size_t)i + q];
    }
}

// corners [m][9] of the sorted boxes; mask [m][cb] 64-bit words, cb = ceil(m / 64)
__global__ __launch_bounds__(RNMS_TILE * RNMS_Q) void k_rnms_mask(const float* __restrict__ corners, int m, int cb, float thr,
                                                                  unsigned long long* __restrict__ mask) {
    const int colb = blockIdx.x, rowb = blockIdx.y;
    if (colb < rowb) return;
    __shared__ float s_px[RIOU_MAXP][RNMS_TILE * RNMS_Q];
    __shared__ float s_py[RIOU_MAXP][RNMS_TILE * RNMS_Q];
    __shared__ float s_vs[RIOU_MAXP][RNMS_TILE * RNMS_Q];
    __shared__ float s_col[RNMS_TILE][9];
    __shared__ unsigned long long s_part[RNMS_Q][RNMS_TILE];
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * RNMS_TILE + tx;
    const int col_size = min(m - colb * RNMS_TILE, RNMS_TILE);
    for (int q = t; q < col_size * 9; q += RNMS_TILE * RNMS_Q) (&s_col[0][0])[q] = corners[(size_t)colb * RNMS_TILE * 9 + q];
    __syncthreads();
    const int i = rowb * RNMS_TILE + tx;
    unsigned long long bits = 0ull;
    if (i < m) {
        float c1[8], c2[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) c1[q] = corners[9 * (size_t)i + q];
        const float area1 = corners[9 * (size_t)i + 8];
        const int per = RNMS_TILE / RNMS_Q;
        int j = ty * per;
        const int jend = min(j + per, col_size);
        if (rowb == colb) j = max(j, tx + 1);      // the diagonal tile: only boxes behind box i
        for (; j < jend; ++j) {
#pragma unroll
            for (int q = 0; q < 8; ++q) c2[q] = s_col[j][q];
            const float iou = riou_iou<RNMS_TILE * RNMS_Q>(c1, area1, c2, s_col[j][8], &s_px[0][0], &s_py[0][0], &s_vs[0][0], t);
            if (iou > thr) bits |= 1ull << j;      // unsigned 64-bit shift: j reaches 63
        }
    }
    s_part[ty][tx] = bits;
    __syncthreads();
    if (ty == 0 && i < m) {
        unsigned long long v = 0ull;
#pragma unroll
        for (int q = 0; q < RNMS_Q; ++q) v |= s_part[q][tx];
        mask[(size_t)i * cb + colb] = v;
    }
}

// nms_postprocess on one wavefront: lane l holds the removed-set words l, l + 64, ...; the boxes of a 64-block are
// walked with find-first-set over "not yet visited and not removed"; a kept box's mask row is read by all lanes at once
__global__ __launch_bounds__(64) void k_rnms_sweep(const unsigned long long* __restrict__ mask, const int* __restrict__ order,
                                                   int m, int cb, int post_max, int* __restrict__ keep,
                                                   long long* __restrict__ n_keep) {
    const int lane = threadIdx.x;
    unsigned long long remv[RNMS_WPL];
#pragma unroll
    for (int k = 0; k < RNMS_WPL; ++k) remv[k] = 0ull;
    int nk = 0;
    for (int b = 0; b < cb && nk < post_max; ++b) {
        // the block's own word, from the lane that holds it
        unsigned long long mine = 0ull;
#pragma unroll
        for (int k = 0; k < RNMS_WPL; ++k) if ((b >> 6) == k) mine = remv[k];
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(mine & 0xffffffffull), b & 63);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(mine >> 32), b & 63);
        unsigned long long cur = ((unsigned long long)hi << 32) | lo;
        const int cnt = min(m - b * 64, 64);
        unsigned long long todo = (cnt >= 64) ? ~0ull : ((1ull << cnt) - 1ull);
        while (nk < post_max) {
            const unsigned long long c = todo & ~cur;
            if (c == 0ull) break;
            const int bit = __builtin_ctzll(c);
            const int i = b * 64 + bit;
            if (lane == 0) keep[nk] = order[i];
            ++nk;
            todo &= ~((2ull << bit) - 1ull);       // bit = 63: 2 << 63 wraps to 0, minus 1 = all ones
            const unsigned long long* row = mask + (size_t)i * cb;
            cur |= row[b];
#pragma unroll
            for (int k = 0; k < RNMS_WPL; ++k) {
                const int w = lane + 64 * k;
                if (w > b && w < cb) remv[k] |= row[w];
            }
        }
    }
    if (lane == 0) *n_keep = nk;
}

void launch_rnms(const float* dets, int n, int m, float thr, int post_max, int* order, float* sorted, float* corners,
                 unsigned long long* mask, int* keep, long long* n_keep, hipStream_t s) {
    const int cb = (m + 63) / 64;
    if (m > 0) {
        hipLaunchKernelGGL(k_rnms_rank, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dets, n, m, order, sorted);
        launch_riou_corners(sorted, m, corners, s);
        hipLaunchKernelGGL(k_rnms_mask, dim3((unsigned)cb, (unsigned)cb), dim3(RNMS_TILE, RNMS_Q), 0, s, corners, m, cb, thr, mask);
    }
    hipLaunchKernelGGL(k_rnms_sweep, dim3(1), dim3(64), 0, s, mask, order, m, cb, post_max, keep, n_keep);
}
