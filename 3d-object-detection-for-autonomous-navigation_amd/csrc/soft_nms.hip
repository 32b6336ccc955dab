// Standalone Soft-NMS: soft_nms_jit of second/core/non_max_suppression/nms_cpu.py:79-169
// with the pre / post caps of nms() around it (libraries/eval_helper_functions.py:463-492).  The rule and its arithmetic
// are in soft_nms_dev.h.
//
// Mapping: with a binding pre cap, k_snms_enter marks the m best boxes by score (rank by counting; equal scores: lower
// index first) and k_snms_compact lists them in input order, so that "lower index" in the rounds is the caller's index.
// k_soft_nms is one workgroup of 1024 threads: boxes and scores of the <= PP_SNMS_MAX_BOXES = 4096 entering rows in LDS
// (80 KB), four rows per thread in registers, per round a workgroup argmax and a parallel decay (snms_rounds).
#include "pp_common.h"
#include "soft_nms_dev.h"

#define SNMS_T 1024
#define SNMS_PER (PP_SNMS_MAX_BOXES / SNMS_T)
static_assert(PP_SNMS_MAX_BOXES % SNMS_T == 0, "every thread of k_soft_nms keeps PP_SNMS_MAX_BOXES / 1024 rows");

// enter[i] = 1 when fewer than m boxes have a higher score, or the same score and a lower index
__global__ __launch_bounds__(256) void k_snms_enter(const float* __restrict__ dets, int n, int m, int* __restrict__ enter) {
    __shared__ float s_sc[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float me = (i < n) ? dets[5 * (size_t)i + 4] : 0.f;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + threadIdx.x;
        __syncthreads();
        s_sc[threadIdx.x] = (j < n) ? dets[5 * (size_t)j + 4] : 0.f;
        __syncthreads();
        const int cnt = min(256, n - j0);
        for (int k = 0; k < cnt; ++k) {
            const float o = s_sc[k];
            rank += (o > me || (o == me && j0 + k < i)) ? 1 : 0;
        }
    }
    if (i < n) enter[i] = (rank < m) ? 1 : 0;
}

// order[position among the entering boxes, by index] = i
__global__ __launch_bounds__(256) void k_snms_compact(const int* __restrict__ enter, int n, int m, int* __restrict__ order) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || enter[i] == 0) return;
    int pos = 0;
    for (int j = 0; j < i; ++j) pos += enter[j];
    if (pos < m) order[pos] = i;
}

// dets [n][5] (x1, y1, x2, y2, score); order [m] the entering rows by index, or NULL: rows 0 .. m-1.  keep [post_max] and
// scores [post_max]: index into dets and final score of every selection, in selection order; *n_keep their number.
__global__ __launch_bounds__(SNMS_T) void k_soft_nms(const float* __restrict__ dets, const int* __restrict__ order, int m,
                                                     int method, float nt, float sigma, float score_floor, int post_max,
                                                     int* __restrict__ keep, float* __restrict__ scores,
                                                     long long* __restrict__ n_keep) {
    __shared__ float s_box[PP_SNMS_MAX_BOXES][4];
    __shared__ float s_sc[PP_SNMS_MAX_BOXES];
    __shared__ float s_red_v[2][SNMS_T / 64];
    __shared__ int s_red_i[2][SNMS_T / 64];
    const int tid = threadIdx.x;
    m = min(m, PP_SNMS_MAX_BOXES);
    for (int i = tid; i < m; i += SNMS_T) {
        const float* row = dets + 5 * (size_t)(order != nullptr ? order[i] : i);
        s_box[i][0] = row[0]; s_box[i][1] = row[1]; s_box[i][2] = row[2]; s_box[i][3] = row[3];
        s_sc[i] = row[4];
    }
    __syncthreads();
    const int nk = snms_rounds<SNMS_T, SNMS_PER>(s_box, s_sc, m, min(post_max, m), method, nt, sigma, score_floor, tid,
                                                 s_red_v, s_red_i, [&](int r, int idx, float sc) {
                                                     keep[r] = (order != nullptr) ? order[idx] : idx;
                                                     scores[r] = sc;
                                                 });
    if (tid == 0) *n_keep = nk;
}

void launch_soft_nms(const float* dets, int n, int m, int method, float nt, float sigma, float score_floor, int post_max,
                     int* enter, int* order, int* keep, float* scores, long long* n_keep, hipStream_t s) {
    const bool cut = m < n;
    if (cut) {
        const dim3 grid((unsigned)((n + 255) / 256));
        hipLaunchKernelGGL(k_snms_enter, grid, dim3(256), 0, s, dets, n, m, enter);
        hipLaunchKernelGGL(k_snms_compact, grid, dim3(256), 0, s, (const int*)enter, n, m, order);
    }
    hipLaunchKernelGGL(k_soft_nms, dim3(1), dim3(SNMS_T), 0, s, dets, cut ? (const int*)order : (const int*)nullptr, m, method,
                       nt, sigma, score_floor, post_max, keep, scores, n_keep);
}
