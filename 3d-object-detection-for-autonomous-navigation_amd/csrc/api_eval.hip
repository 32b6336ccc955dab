// C-ABI, the AP evaluator (kitti_eval.py): rotated-box overlaps (kernels: rotate_iou.hip) and the matching / counting
// statistics (eval_stats.hip).  No handle: host buffers in, host buffers out, device memory for the call's duration.
#include "pp_engine.h"

namespace {
int riou_common(int device, const float* boxes, int64_t n, const float* qboxes, int64_t k, int32_t criterion,
                DevBuf& d_out, const char* who) {
    if (int st = check_device(who, device)) return st;
    if (n < 0 || k < 0 || (n > 0 && !boxes) || (k > 0 && !qboxes)) return fail(nullptr, PP_ERR_ARG, "%s: bad argument", who);
    if (criterion < -1 || criterion > 2) return fail(nullptr, PP_ERR_ARG, "%s: criterion %d not in {-1,0,1,2}", who, criterion);
    if (n > 200000) return fail(nullptr, PP_ERR_ARG, "%s: at most 200000 boxes per call (got %lld)", who, (long long)n);
    DEVCHK(hipSetDevice(device));
    DevBuf d_b, d_q, d_bc, d_qc;
    DEVCHK(d_b.alloc(sizeof(float) * 5 * n)); DEVCHK(d_q.alloc(sizeof(float) * 5 * k));
    DEVCHK(d_bc.alloc(sizeof(float) * 9 * n)); DEVCHK(d_qc.alloc(sizeof(float) * 9 * k));
    DEVCHK(d_out.alloc(sizeof(float) * n * k));
    if (n == 0 || k == 0) return PP_OK;
    DEVCHK(hipMemcpy(d_b.p, boxes, sizeof(float) * 5 * n, hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_q.p, qboxes, sizeof(float) * 5 * k, hipMemcpyHostToDevice));
    launch_riou_corners((const float*)d_b.p, n, (float*)d_bc.p, nullptr);
    launch_riou_corners((const float*)d_q.p, k, (float*)d_qc.p, nullptr);
    launch_riou_pairs((const float*)d_bc.p, n, (const float*)d_qc.p, k, criterion, (float*)d_out.p, nullptr);
    DEVCHK(hipGetLastError());
    return PP_OK;
}
}  // namespace

extern "C" {

int pp_rotate_iou_eval(int device, const float* boxes, int64_t n, const float* query_boxes, int64_t k,
                       int32_t criterion, float* out) {
    DevBuf d_out;
    int st = riou_common(device, boxes, n, query_boxes, k, criterion, d_out, "pp_rotate_iou_eval");
    if (st || n == 0 || k == 0) return st;
    if (!out) return fail(nullptr, PP_ERR_ARG, "pp_rotate_iou_eval: out is null");
    const char* who = "pp_rotate_iou_eval";
    DEVCHK(hipMemcpy(out, d_out.p, sizeof(float) * n * k, hipMemcpyDeviceToHost));
    return PP_OK;
}

int pp_d3_box_overlap(int device, const double* boxes, int64_t n, const double* query_boxes, int64_t k,
                      int32_t criterion, double* out) {
    const char* who = "pp_d3_box_overlap";
    if (n < 0 || k < 0 || (n > 0 && !boxes) || (k > 0 && !query_boxes)) return fail(nullptr, PP_ERR_ARG, "%s: bad argument", who);
    // BEV rectangles [x, z, l, w, ry] in float32, raw intersection area (criterion 2), like eval.py:160-161
    std::vector<float> b5((size_t)n * 5), q5((size_t)k * 5);
    const int sel[5] = {0, 2, 3, 5, 6};
    for (int64_t i = 0; i < n; ++i) for (int j = 0; j < 5; ++j) b5[i * 5 + j] = (float)boxes[i * 7 + sel[j]];
    for (int64_t i = 0; i < k; ++i) for (int j = 0; j < 5; ++j) q5[i * 5 + j] = (float)query_boxes[i * 7 + sel[j]];
    DevBuf d_rinc;
    int st = riou_common(device, b5.data(), n, q5.data(), k, 2, d_rinc, who);
    if (st || n == 0 || k == 0) return st;
    if (!out) return fail(nullptr, PP_ERR_ARG, "%s: out is null", who);
    if (criterion < -1 || criterion > 2) return fail(nullptr, PP_ERR_ARG, "%s: criterion %d not in {-1,0,1,2}", who, criterion);
    DevBuf d_b, d_q, d_o;
    DEVCHK(d_b.alloc(sizeof(double) * 7 * n)); DEVCHK(d_q.alloc(sizeof(double) * 7 * k)); DEVCHK(d_o.alloc(sizeof(double) * n * k));
    DEVCHK(hipMemcpy(d_b.p, boxes, sizeof(double) * 7 * n, hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_q.p, query_boxes, sizeof(double) * 7 * k, hipMemcpyHostToDevice));
    launch_d3_finish((const double*)d_b.p, n, (const double*)d_q.p, k, criterion, (const float*)d_rinc.p, (double*)d_o.p, nullptr);
    DEVCHK(hipGetLastError());
    DEVCHK(hipMemcpy(out, d_o.p, sizeof(double) * n * k, hipMemcpyDeviceToHost));
    return PP_OK;
}

namespace {
struct EvEvents {
    hipEvent_t a = nullptr, b = nullptr;
    ~EvEvents() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};
// the arguments both entry points share: checks them, uploads them and fills the shared part of `p`
struct EvalUpload {
    DevBuf gt_off, dt_off, ov_off, ov, scores, ign_gt, ign_dt, mo;
    int64_t total_gt = 0, total_dt = 0;
    int prepare(const char* who, int device, int32_t nframes, const int32_t* gt_off_h, const int32_t* dt_off_h,
                const int64_t* ov_off_h, const double* overlaps, const double* scores_h, const int32_t* ign_gt_h,
                const int32_t* ign_dt_h, const double* min_overlaps, int32_t K, EvalStatsParams& p) {
        if (int st = check_device(who, device)) return st;
        if (nframes < 0 || K < 0 || (K > 0 && !min_overlaps)) return fail(nullptr, PP_ERR_ARG, "%s: bad argument", who);
        if (K > 65535) return fail(nullptr, PP_ERR_ARG, "%s: at most 65535 overlap tiers (got %d)", who, K);
        if (nframes > 0 && (!gt_off_h || !dt_off_h || !ov_off_h)) return fail(nullptr, PP_ERR_ARG, "%s: frame offsets are NULL", who);
        if (nframes > 0 && (gt_off_h[0] != 0 || dt_off_h[0] != 0 || ov_off_h[0] != 0))
            return fail(nullptr, PP_ERR_ARG, "%s: frame offsets must start at 0", who);
        for (int32_t f = 0; f < nframes; ++f) {
            const int64_t G = (int64_t)gt_off_h[f + 1] - gt_off_h[f], D = (int64_t)dt_off_h[f + 1] - dt_off_h[f];
            if (G < 0 || D < 0) return fail(nullptr, PP_ERR_ARG, "%s: frame offsets not monotone at frame %d", who, f);
            if (G > PP_EVAL_MAX_BOXES || D > PP_EVAL_MAX_BOXES)
                return fail(nullptr, PP_ERR_ARG, "%s: frame %d has %lld ground truths and %lld detections; at most %d of each per frame",
                            who, f, (long long)G, (long long)D, PP_EVAL_MAX_BOXES);
            if (ov_off_h[f + 1] - ov_off_h[f] != G * D)
                return fail(nullptr, PP_ERR_ARG, "%s: frame %d: overlap offsets do not span %lld x %lld values", who, f,
                            (long long)G, (long long)D);
        }
        total_gt = nframes > 0 ? gt_off_h[nframes] : 0;
        total_dt = nframes > 0 ? dt_off_h[nframes] : 0;
        const int64_t total_ov = nframes > 0 ? ov_off_h[nframes] : 0;
        if ((total_gt > 0 && !ign_gt_h) || (total_dt > 0 && (!ign_dt_h || !scores_h)) || (total_ov > 0 && !overlaps))
            return fail(nullptr, PP_ERR_ARG, "%s: NULL box array", who);
        DEVCHK(hipSetDevice(device));
        if (nframes == 0 || K == 0) return PP_OK;
        const size_t nf1 = (size_t)nframes + 1;
#define EV_UP(buf, src, bytes) do { DEVCHK(buf.alloc(bytes)); if ((bytes) > 0) DEVCHK(hipMemcpy(buf.p, src, bytes, hipMemcpyHostToDevice)); } while (0)
        EV_UP(gt_off, gt_off_h, sizeof(int32_t) * nf1);
        EV_UP(dt_off, dt_off_h, sizeof(int32_t) * nf1);
        EV_UP(ov_off, ov_off_h, sizeof(int64_t) * nf1);
        EV_UP(ov, overlaps, sizeof(double) * (size_t)total_ov);
        EV_UP(scores, scores_h, sizeof(double) * (size_t)total_dt);
        EV_UP(ign_gt, ign_gt_h, sizeof(int32_t) * (size_t)total_gt);
        EV_UP(ign_dt, ign_dt_h, sizeof(int32_t) * (size_t)total_dt);
        EV_UP(mo, min_overlaps, sizeof(double) * (size_t)K);
        p.nframes = nframes; p.K = K; p.total_gt = (int)total_gt;
        p.gt_off = (const int*)gt_off.p; p.dt_off = (const int*)dt_off.p; p.ov_off = (const long long*)ov_off.p;
        p.overlaps = (const double*)ov.p; p.scores = (const double*)scores.p;
        p.ign_gt = (const int*)ign_gt.p; p.ign_dt = (const int*)ign_dt.p; p.min_overlaps = (const double*)mo.p;
        return PP_OK;
    }
};
}  // namespace

int pp_eval_match(int device, int32_t nframes, const int32_t* gt_off, const int32_t* dt_off, const int64_t* ov_off,
                  const double* overlaps, const double* scores, const int32_t* ignored_gt, const int32_t* ignored_det,
                  const double* min_overlaps, int32_t ntiers, int32_t* matched, float* kernel_ms) {
    const char* who = "pp_eval_match";
    EvalStatsParams p = {};
    EvalUpload up;
    int st = up.prepare(who, device, nframes, gt_off, dt_off, ov_off, overlaps, scores, ignored_gt, ignored_det,
                        min_overlaps, ntiers, p);
    if (st) return st;
    if (kernel_ms) *kernel_ms = 0.f;
    const size_t nout = (size_t)ntiers * (size_t)up.total_gt;
    if (nframes == 0 || nout == 0) return PP_OK;
    if (!matched) return fail(nullptr, PP_ERR_ARG, "%s: matched is null", who);
    DevBuf d_m;
    DEVCHK(d_m.alloc(sizeof(int32_t) * nout));
    p.matched = (int*)d_m.p;
    EvEvents ev;
    DEVCHK(hipEventCreate(&ev.a)); DEVCHK(hipEventCreate(&ev.b));
    DEVCHK(hipEventRecord(ev.a, nullptr));
    launch_eval_match(p, nullptr);
    DEVCHK(hipEventRecord(ev.b, nullptr));
    DEVCHK(hipGetLastError());
    DEVCHK(hipMemcpy(matched, d_m.p, sizeof(int32_t) * nout, hipMemcpyDeviceToHost));
    if (kernel_ms) DEVCHK(hipEventElapsedTime(kernel_ms, ev.a, ev.b));
    return PP_OK;
}

int pp_eval_pr(int device, int32_t nframes, const int32_t* gt_off, const int32_t* dt_off, const int64_t* ov_off,
               const double* overlaps, const double* scores, const int32_t* ignored_gt, const int32_t* ignored_det,
               const double* min_overlaps, int32_t ntiers, const double* gt_alphas, const double* dt_alphas,
               const double* dt_boxes, const int32_t* dc_off, const double* dc_boxes, int32_t metric,
               int32_t compute_aos, const double* thresholds, const int32_t* nthresh, double* pr, float* kernel_ms) {
    const char* who = "pp_eval_pr";
    EvalStatsParams p = {};
    EvalUpload up;
    int st = up.prepare(who, device, nframes, gt_off, dt_off, ov_off, overlaps, scores, ignored_gt, ignored_det,
                        min_overlaps, ntiers, p);
    if (st) return st;
    if (kernel_ms) *kernel_ms = 0.f;
    if (ntiers == 0) return PP_OK;
    if (!pr) return fail(nullptr, PP_ERR_ARG, "%s: pr is null", who);
    const size_t npr = (size_t)ntiers * PP_EVAL_NTHRESH * 4;
    memset(pr, 0, sizeof(double) * npr);
    if (nframes == 0) return PP_OK;
    if (metric < 0 || metric > 2) return fail(nullptr, PP_ERR_ARG, "%s: metric %d not in {0,1,2}", who, metric);
    if (!thresholds || !nthresh) return fail(nullptr, PP_ERR_ARG, "%s: thresholds / nthresh is null", who);
    for (int32_t k = 0; k < ntiers; ++k)
        if (nthresh[k] < 0 || nthresh[k] > PP_EVAL_NTHRESH)
            return fail(nullptr, PP_ERR_ARG, "%s: nthresh[%d] = %d not in [0,%d]", who, k, nthresh[k], PP_EVAL_NTHRESH);
    int64_t total_dc = 0;
    if (metric == 0) {
        if (!dc_off || dc_off[0] != 0) return fail(nullptr, PP_ERR_ARG, "%s: DontCare offsets are NULL or do not start at 0", who);
        for (int32_t f = 0; f < nframes; ++f)
            if (dc_off[f + 1] < dc_off[f]) return fail(nullptr, PP_ERR_ARG, "%s: DontCare offsets not monotone at frame %d", who, f);
        total_dc = dc_off[nframes];
        if ((total_dc > 0 && !dc_boxes) || (up.total_dt > 0 && !dt_boxes)) return fail(nullptr, PP_ERR_ARG, "%s: NULL 2D boxes", who);
    }
    if (compute_aos && ((up.total_gt > 0 && !gt_alphas) || (up.total_dt > 0 && !dt_alphas)))
        return fail(nullptr, PP_ERR_ARG, "%s: NULL alphas", who);
    DevBuf d_ga, d_da, d_db, d_dco, d_dcb, d_th, d_nt, d_part, d_pr;
    const size_t nf1 = (size_t)nframes + 1;
    if (compute_aos) {
        EV_UP(d_ga, gt_alphas, sizeof(double) * (size_t)up.total_gt);
        EV_UP(d_da, dt_alphas, sizeof(double) * (size_t)up.total_dt);
    }
    if (metric == 0) {
        EV_UP(d_db, dt_boxes, sizeof(double) * 4 * (size_t)up.total_dt);
        EV_UP(d_dco, dc_off, sizeof(int32_t) * nf1);
        EV_UP(d_dcb, dc_boxes, sizeof(double) * 4 * (size_t)total_dc);
    } else {                                            // the kernel reads dc_off only to find no boxes
        DEVCHK(d_dco.alloc(sizeof(int32_t) * nf1));
        DEVCHK(hipMemset(d_dco.p, 0, sizeof(int32_t) * nf1));
    }
    EV_UP(d_th, thresholds, sizeof(double) * (size_t)ntiers * PP_EVAL_NTHRESH);
    EV_UP(d_nt, nthresh, sizeof(int32_t) * (size_t)ntiers);
    DEVCHK(d_part.alloc(sizeof(double) * npr * (size_t)nframes));
    DEVCHK(d_pr.alloc(sizeof(double) * npr));
    p.gt_alpha = (const double*)d_ga.p; p.dt_alpha = (const double*)d_da.p; p.dt_box = (const double*)d_db.p;
    p.dc_off = (const int*)d_dco.p; p.dc_box = (const double*)d_dcb.p;
    p.thresholds = (const double*)d_th.p; p.nthresh = (const int*)d_nt.p;
    p.metric = metric; p.compute_aos = compute_aos ? 1 : 0;
    p.partial = (double*)d_part.p; p.pr = (double*)d_pr.p;
    EvEvents ev;
    DEVCHK(hipEventCreate(&ev.a)); DEVCHK(hipEventCreate(&ev.b));
    DEVCHK(hipEventRecord(ev.a, nullptr));
    launch_eval_count(p, nullptr);
    launch_eval_reduce(p, nullptr);
    DEVCHK(hipEventRecord(ev.b, nullptr));
    DEVCHK(hipGetLastError());
    DEVCHK(hipMemcpy(pr, d_pr.p, sizeof(double) * npr, hipMemcpyDeviceToHost));
    if (kernel_ms) DEVCHK(hipEventElapsedTime(kernel_ms, ev.a, ev.b));
#undef EV_UP
    return PP_OK;
}

}  // extern "C"
