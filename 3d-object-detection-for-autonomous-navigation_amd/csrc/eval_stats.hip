// KITTI AP evaluator: greedy ground-truth <-> detection matching and the tp / fp / fn / orientation-similarity
// statistics on the device (kitti_eval.compute_statistics, which restates compute_statistics_jit,
// second/utils/eval.py:166-287, and the accumulation of fused_compute_statistics, :298-345).
//
// One wavefront per independent item -- (frame, tier) for the matching pass, (frame, tier, threshold) for the
// counting pass -- one lane per detection, the ground-truth loop serial inside the wave.  Frames with more than
// 64 detections are walked in chunks of 64 (at most ES_MAX_CHUNKS); a lane keeps the state of its detection of
// every chunk as one bit per chunk.  A frame's overlaps are packed [G][D], so one ground truth's candidates are a
// contiguous read across the lanes.  Scores, overlaps, boxes and thresholds are float64 and every comparison is
// the host's comparison on the same bits; the only arithmetic whose rounding can differ from the host's is cos().
//
// The sums over frames are taken in a fixed order (k_es_reduce): no floating-point atomics, so two calls on the
// same input return the same bytes.
#include "pp_common.h"

namespace {

constexpr int ES_WAVES = 4;                 // wavefronts (items) per workgroup
constexpr int ES_NO_INDEX = 0x7fffffff;
constexpr double ES_NO_DETECTION = -10000000.0;

// the better of two (value, index) candidates on every lane: larger value, lower index on ties; an index of
// ES_NO_INDEX is "no candidate".  The order is total, so the xor butterfly leaves every lane with the same winner.
__device__ __forceinline__ void wave_best(double& v, int& idx) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(v, m, PP_WAVE);
        const int oi = __shfl_xor(idx, m, PP_WAVE);
        const bool take = oi != ES_NO_INDEX && (idx == ES_NO_INDEX || ov > v || (ov == v && oi < idx));
        if (take) { v = ov; idx = oi; }
    }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, PP_WAVE));
    return v;
}

// ---- pass 1 (compute_fp = False): which detection each ground truth takes as a true positive ----
__global__ __launch_bounds__(ES_WAVES * PP_WAVE) void k_es_match(EvalStatsParams p) {
    const int lane = threadIdx.x & (PP_WAVE - 1);
    const int k = blockIdx.y * ES_WAVES + (threadIdx.x >> 6);
    const int f = blockIdx.x;
    if (k >= p.K) return;                                   // whole waves leave together
    const int g0 = p.gt_off[f], G = p.gt_off[f + 1] - g0;
    const int d0 = p.dt_off[f], D = p.dt_off[f + 1] - d0;
    const double* ov = p.overlaps + p.ov_off[f];
    const double mo = p.min_overlaps[k];
    const int nch = (D + PP_WAVE - 1) / PP_WAVE;
    int* matched = p.matched + (long long)k * p.total_gt + g0;

    unsigned usable = 0, assigned = 0;                      // bit c: this lane's detection of chunk c
    for (int c = 0; c < nch; ++c) {
        const int j = c * PP_WAVE + lane;
        // a score at or below the sentinel can never replace it (`dt_score > valid_detection`)
        if (j < D && p.ign_dt[d0 + j] != -1 && p.scores[d0 + j] > ES_NO_DETECTION) usable |= 1u << c;
    }
    for (int i = 0; i < G; ++i) {
        const int ig = p.ign_gt[g0 + i];
        if (ig == -1) {
            if (lane == 0) matched[i] = -1;
            continue;
        }
        double best = 0.0;
        int bidx = ES_NO_INDEX;
        for (int c = 0; c < nch; ++c) {
            const int j = c * PP_WAVE + lane;
            if (!((usable & ~assigned) >> c & 1u)) continue;
            if (!(ov[(long long)i * D + j] > mo)) continue;
            const double s = p.scores[d0 + j];
            if (bidx == ES_NO_INDEX || s > best) { best = s; bidx = j; }     // strict: the first index keeps a tie
        }
        wave_best(best, bidx);
        int out = -1;
        if (bidx != ES_NO_INDEX) {
            if ((bidx & (PP_WAVE - 1)) == lane) assigned |= 1u << (bidx >> 6);
            if (ig == 0 && p.ign_dt[d0 + bidx] == 0) out = bidx;
        }
        if (lane == 0) matched[i] = out;
    }
}

// ---- pass 2 (compute_fp = True): tp, fp, fn and the similarity sum of one (frame, tier, threshold) ----
__global__ __launch_bounds__(ES_WAVES * PP_WAVE) void k_es_count(EvalStatsParams p) {
    const int lane = threadIdx.x & (PP_WAVE - 1);
    const int t = blockIdx.z * ES_WAVES + (threadIdx.x >> 6);
    const int k = blockIdx.y;
    const int f = blockIdx.x;
    if (t >= p.nthresh[k]) return;                          // whole waves leave together; nthresh <= PP_EVAL_NTHRESH
    const int g0 = p.gt_off[f], G = p.gt_off[f + 1] - g0;
    const int d0 = p.dt_off[f], D = p.dt_off[f + 1] - d0;
    const double* ov = p.overlaps + p.ov_off[f];
    const double mo = p.min_overlaps[k];
    const double thresh = p.thresholds[k * PP_EVAL_NTHRESH + t];
    const int nch = (D + PP_WAVE - 1) / PP_WAVE;

    unsigned usable = 0, real = 0, assigned = 0;
    for (int c = 0; c < nch; ++c) {
        const int j = c * PP_WAVE + lane;
        if (j >= D) continue;
        const int id = p.ign_dt[d0 + j];
        if (id != -1 && !(p.scores[d0 + j] < thresh)) usable |= 1u << c;     // a score equal to the threshold stays in
        if (id == 0) real |= 1u << c;
    }
    int tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    for (int i = 0; i < G; ++i) {
        const int ig = p.ign_gt[g0 + i];
        if (ig == -1) continue;
        double best = 0.0;
        int bidx = ES_NO_INDEX, neutral = ES_NO_INDEX;
        for (int c = 0; c < nch; ++c) {
            const int j = c * PP_WAVE + lane;
            if (!((usable & ~assigned) >> c & 1u)) continue;
            const double o = ov[(long long)i * D + j];
            if (!(o > mo)) continue;
            if (real >> c & 1u) {
                if (bidx == ES_NO_INDEX || o > best) { best = o; bidx = j; }
            } else {
                neutral = min(neutral, j);
            }
        }
        wave_best(best, bidx);
        int det = bidx;
        if (det == ES_NO_INDEX) det = wave_min(neutral);    // only neutral detections overlap: the first of them
        if (det == ES_NO_INDEX) {
            if (ig == 0) ++fn;
            continue;
        }
        if ((det & (PP_WAVE - 1)) == lane) assigned |= 1u << (det >> 6);
        if (ig == 1 || p.ign_dt[d0 + det] == 1) continue;   // marks the detection, counts nothing
        ++tp;
        if (p.compute_aos) sim += (1.0 + cos(p.gt_alpha[g0 + i] - p.dt_alpha[d0 + det])) / 2.0;
    }
    // false positives: countable detections at or above the threshold that nothing took, less (2D boxes only)
    // those lying in a DontCare region
    const int c0 = p.dc_off[f], C = p.metric == 0 ? p.dc_off[f + 1] - c0 : 0;
    for (int c = 0; c < nch; ++c) {
        const int j = c * PP_WAVE + lane;
        bool is_fp = (usable & real & ~assigned) >> c & 1u;
        if (is_fp && C > 0) {
            const double* b = p.dt_box + 4ll * (d0 + j);
            const double b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
            const double area = (b2 - b0) * (b3 - b1);
            for (int q = 0; q < C; ++q) {                   // image_box_overlap(dt, dc, criterion 0)
                const double* dc = p.dc_box + 4ll * (c0 + q);
                const double iw = fmin(b2, dc[2]) - fmax(b0, dc[0]);
                const double ih = fmin(b3, dc[3]) - fmax(b1, dc[1]);
                const double o = (iw > 0.0 && ih > 0.0) ? iw * ih / area : 0.0;
                if (o > mo) { is_fp = false; break; }
            }
        }
        fp += __popcll(__ballot(is_fp));
    }
    if (lane == 0) {
        double* out = p.partial + (((long long)f * p.K + k) * PP_EVAL_NTHRESH + t) * 4;
        out[0] = (double)tp;
        out[1] = (double)fp;
        out[2] = (double)fn;
        out[3] = sim;
    }
}

// ---- sum over frames, in a fixed order: thread i adds frames i, i + 256, ... ; then a fixed tree ----
__global__ __launch_bounds__(256) void k_es_reduce(EvalStatsParams p) {
    __shared__ double sh[256][4];
    const int t = blockIdx.x, k = blockIdx.y;
    const bool live = t < p.nthresh[k];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (live)
        for (int f = threadIdx.x; f < p.nframes; f += 256) {
            const double* in = p.partial + (((long long)f * p.K + k) * PP_EVAL_NTHRESH + t) * 4;
            for (int c = 0; c < 4; ++c) acc[c] += in[c];
        }
    for (int c = 0; c < 4; ++c) sh[threadIdx.x][c] = acc[c];
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int c = 0; c < 4; ++c) sh[threadIdx.x][c] += sh[threadIdx.x + s][c];
        __syncthreads();
    }
    if (threadIdx.x < 4) p.pr[((long long)k * PP_EVAL_NTHRESH + t) * 4 + threadIdx.x] = sh[0][threadIdx.x];
}

}  // namespace

void launch_eval_match(const EvalStatsParams& p, hipStream_t s) {
    if (p.nframes <= 0 || p.K <= 0) return;
    dim3 grid((unsigned)p.nframes, (unsigned)((p.K + ES_WAVES - 1) / ES_WAVES));
    hipLaunchKernelGGL(k_es_match, grid, dim3(ES_WAVES * PP_WAVE), 0, s, p);
}

void launch_eval_count(const EvalStatsParams& p, hipStream_t s) {
    if (p.nframes <= 0 || p.K <= 0) return;
    dim3 grid((unsigned)p.nframes, (unsigned)p.K, (unsigned)((PP_EVAL_NTHRESH + ES_WAVES - 1) / ES_WAVES));
    hipLaunchKernelGGL(k_es_count, grid, dim3(ES_WAVES * PP_WAVE), 0, s, p);
}

void launch_eval_reduce(const EvalStatsParams& p, hipStream_t s) {
    if (p.K <= 0) return;
    hipLaunchKernelGGL(k_es_reduce, dim3(PP_EVAL_NTHRESH, (unsigned)p.K), dim3(256), 0, s, p);
}
