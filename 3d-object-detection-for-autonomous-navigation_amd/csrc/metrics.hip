// Training metrics at the head map: the per-step counts behind the reference's monitoring
// block, libraries/metrics.py -- Accuracy.call :60-83, PrecisionRecall.call with _calc_binary_metrics :103-161 -- for
// encode_background_as_zeros = true and use_sigmoid_score = true, the only combination the configuration accepts.
// One thread per head pixel, as k_loss_pixels: it reads the pixel's class logits (napl * ncls floats of the 128-byte head
// row, or of a plain [batch][A][ncls] array) and its napl labels, and decides 17 predicates per anchor; a wave counts each
// by ballot + popcount, the four waves' counts meet in LDS and leave one row of 32 integers per workgroup.  A second,
// one-workgroup launch adds the rows into counts[32] (int64).  Integers only: the same bytes on every run.
#include "pp_common.h"

#define MT 256
#define MROW PP_METRICS_COUNTS    // integers per partial row (17 in use, the rest 0)
#define MFIN 1024                 // threads of the finish launch

// score > t_i decides tp / fp: PrecisionRecall._thresholds, rounded to float32
__device__ __forceinline__ float metrics_threshold(int i) {
    constexpr float t[PP_METRICS_NTHRESH] = {0.1f, 0.3f, 0.5f, 0.7f, 0.8f, 0.9f, 0.95f};
    return t[i];
}

__device__ __forceinline__ int wave_count(bool pred) { return __popcll(__ballot(pred)); }

template <int NAPL, int NCLS>
__global__ __launch_bounds__(MT) void k_metrics_pixels(MetricsParams p) {
    constexpr int NC = NAPL * NCLS;      // class logits per pixel
    __shared__ int s_part[MT / 64][MROW];
    const int b = blockIdx.y;
    const int px = blockIdx.x * MT + threadIdx.x;
    const bool valid = px < p.npx;
    const int pxr = valid ? px : 0;      // (a tail thread reads pixel 0 and counts nothing: every lane reaches the ballots)
    // only the class columns of the row.  On the head map that is 64 different 128-byte lines per wave instruction;
    // reading the workgroup's rows as consecutive 16-byte pieces through LDS instead (what k_loss_pixels does for its
    // whole rows) measured no faster here: 10.4 against 9.5 us at B = 64
    const float* row = p.logits + ((size_t)b * p.npx + pxr) * p.row_stride + p.col_off;
    float x[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) x[j] = row[j];
    const int* lab = p.labels + (size_t)b * p.A + (size_t)pxr * NAPL;
    // wave-uniform counts: acc_hit, n_pos, n_neg, tp[7], fp[7]
    int hit = 0, npos = 0, nneg = 0, tp[PP_METRICS_NTHRESH], fp[PP_METRICS_NTHRESH];
#pragma unroll
    for (int i = 0; i < PP_METRICS_NTHRESH; ++i) tp[i] = fp[i] = 0;
#pragma unroll
    for (int r = 0; r < NAPL; ++r) {
        const int label = lab[r];
        // score = max_c sigmoid(x_c) (a NaN stays: it compares false below); predicted label = first maximum of the
        // logits + 1 where any score passes 0.5, else 0
        float best = x[r * NCLS];
        int arg = 0;
        float score = 1.f / (1.f + expf(-best));
        bool any = score > 0.5f;
#pragma unroll
        for (int c = 1; c < NCLS; ++c) {
            const float xc = x[r * NCLS + c];
            const float sc = 1.f / (1.f + expf(-xc));
            if (xc > best) { best = xc; arg = c; }
            if (sc > score || sc != sc) score = sc;
            any = any || sc > 0.5f;
        }
        const int pred = any ? arg + 1 : 0;
        const bool pos = valid && label > 0, neg = valid && label == 0;
        hit += wave_count(valid && pred == label);
        npos += wave_count(pos);
        nneg += wave_count(neg);
#pragma unroll
        for (int i = 0; i < PP_METRICS_NTHRESH; ++i) {
            const bool over = score > metrics_threshold(i);
            tp[i] += wave_count(pos && over);
            fp[i] += wave_count(neg && over);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        int* d = s_part[wave];
        d[0] = hit; d[1] = npos; d[2] = nneg;
#pragma unroll
        for (int i = 0; i < PP_METRICS_NTHRESH; ++i) { d[3 + i] = tp[i]; d[3 + PP_METRICS_NTHRESH + i] = fp[i]; }
    }
    __syncthreads();
    if (threadIdx.x < MROW) {
        int t = 0;
        if (threadIdx.x < 3 + 2 * PP_METRICS_NTHRESH)
            for (int w = 0; w < MT / 64; ++w) t += s_part[w][threadIdx.x];
        p.partials[((size_t)b * gridDim.x + blockIdx.x) * MROW + threadIdx.x] = t;
    }
}

// counts[k] = sum over the workgroup rows.  One workgroup, so what it costs is the depth of its chain of dependent
// loads: thread (slice, quad) adds four counters of rows slice, slice + 128, ... (16-byte loads, eight in flight), the
// 128 slices meet in LDS in two steps
__global__ __launch_bounds__(MFIN) void k_metrics_finish(MetricsParams p, int nrows) {
    constexpr int NQ = MROW / 4, NS = MFIN / NQ, NG = 8;      // quads per row, slices, groups of the first LDS step
    __shared__ long long s_sum[NS][MROW];
    __shared__ long long s_grp[NG][MROW];
    const int q = threadIdx.x % NQ, slice = threadIdx.x / NQ;
    const int4* rows = reinterpret_cast<const int4*>(p.partials);
    long long t0 = 0, t1 = 0, t2 = 0, t3 = 0;
#pragma unroll 8
    for (int i = slice; i < nrows; i += NS) {
        const int4 v = rows[(size_t)i * NQ + q];
        t0 += v.x; t1 += v.y; t2 += v.z; t3 += v.w;
    }
    long long* d = s_sum[slice] + 4 * q;
    d[0] = t0; d[1] = t1; d[2] = t2; d[3] = t3;
    __syncthreads();
    if (threadIdx.x < NG * MROW) {
        const int k = threadIdx.x % MROW, g = threadIdx.x / MROW;
        long long sum = 0;
#pragma unroll
        for (int s = 0; s < NS / NG; ++s) sum += s_sum[g * (NS / NG) + s][k];
        s_grp[g][k] = sum;
    }
    __syncthreads();
    if (threadIdx.x < MROW) {
        long long sum = 0;
#pragma unroll
        for (int g = 0; g < NG; ++g) sum += s_grp[g][threadIdx.x];
        p.counts[threadIdx.x] = sum;
    }
}

int metrics_blocks(int npx) { return (npx + MT - 1) / MT; }

template <int NAPL>
static int launch_pixels(const MetricsParams& p, dim3 grid, hipStream_t s) {
    switch (p.ncls) {
        case 1: PP_LAUNCH("k_metrics_pixels", (k_metrics_pixels<NAPL, 1>), grid, dim3(MT), 0, s, p); return 0;
        case 2: PP_LAUNCH("k_metrics_pixels", (k_metrics_pixels<NAPL, 2>), grid, dim3(MT), 0, s, p); return 0;
        case 3: PP_LAUNCH("k_metrics_pixels", (k_metrics_pixels<NAPL, 3>), grid, dim3(MT), 0, s, p); return 0;
        case 4: PP_LAUNCH("k_metrics_pixels", (k_metrics_pixels<NAPL, 4>), grid, dim3(MT), 0, s, p); return 0;
        default: return PP_ERR_UNSUPPORTED;
    }
}

int launch_head_metrics(const MetricsParams& p, hipStream_t s) {
    // the combinations launch_head_loss takes; a logits row holds at least the pixel's napl * ncls class columns
    if (p.napl < 1 || p.napl > 3 || p.ncls < 1 || p.ncls > 4 || p.npx < 1 || p.A != (int64_t)p.npx * p.napl ||
        p.col_off < 0 || p.col_off + p.napl * p.ncls > p.row_stride) return PP_ERR_UNSUPPORTED;
    const int nblocks = metrics_blocks(p.npx);
    if (p.batch > 0) {
        const dim3 grid(nblocks, p.batch);
        int st;
        if (p.napl == 1) st = launch_pixels<1>(p, grid, s);
        else if (p.napl == 2) st = launch_pixels<2>(p, grid, s);
        else st = launch_pixels<3>(p, grid, s);
        if (st) return st;
    }
    PP_LAUNCH("k_metrics_finish", k_metrics_finish, dim3(1), dim3(MFIN), 0, s, p, (p.batch > 0 ? p.batch : 0) * nblocks);
    return 0;
}
