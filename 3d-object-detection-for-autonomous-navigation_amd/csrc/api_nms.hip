// C-ABI, non-maximum suppression: the detector's rule (per handle; the kernel instantiations are in postprocess.hip), the
// standalone rotated NMS (kernels: rotate_nms.hip) and the standalone Soft-NMS (soft_nms.hip).  The latter two need no
// handle: host buffers in, host buffers out, device memory for the call's duration.
#include "pp_engine.h"

extern "C" {

int pp_set_nms_mode(pp_handle e, int32_t mode) {
    if (!e) return PP_ERR_ARG;
    if (mode != PP_NMS_STANDUP && mode != PP_NMS_ROTATED && mode != PP_NMS_SOFT)
        return fail(e, PP_ERR_ARG, "pp_set_nms_mode: unknown mode %d", mode);
    if (mode == e->rule.nms_mode) return PP_OK;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_nms_mode: a training step is in flight");
    if (mode + e->rule.nms_mode == PP_NMS_ROTATED + PP_NMS_SOFT)
        return fail(e, PP_ERR_UNSUPPORTED, "pp_set_nms_mode: soft re-scoring on the rotated overlap is not built; switch "
                                           "between PP_NMS_ROTATED and PP_NMS_SOFT through PP_NMS_STANDUP");
    e->rule.nms_mode = mode;
    return PP_OK;
}

int pp_get_nms_mode(pp_handle e, int32_t* mode) {
    if (!e || !mode) return PP_ERR_ARG;
    *mode = e->rule.nms_mode;
    return PP_OK;
}

static const char* soft_nms_args(int32_t method, float sigma, float score_floor) {
    if (method != PP_SOFT_NMS_HARD && method != PP_SOFT_NMS_LINEAR && method != PP_SOFT_NMS_GAUSSIAN) return "unknown method";
    if (!std::isfinite(sigma) || !(sigma > 0.f)) return "sigma must be finite and > 0";
    if (!std::isfinite(score_floor) || score_floor < 0.f) return "score_floor must be finite and >= 0";
    return nullptr;
}

int pp_set_soft_nms(pp_handle e, int32_t method, float sigma, float score_floor) {
    if (!e) return PP_ERR_ARG;
    if (const char* why = soft_nms_args(method, sigma, score_floor))
        return fail(e, PP_ERR_ARG, "pp_set_soft_nms: %s (method %d, sigma %g, score_floor %g)", why, method, sigma, score_floor);
    PostRule& r = e->rule;
    if (method == r.soft_method && sigma == r.soft_sigma && score_floor == r.soft_floor) return PP_OK;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_soft_nms: a training step is in flight");
    r.soft_method = method; r.soft_sigma = sigma; r.soft_floor = score_floor;
    return PP_OK;
}

int pp_get_soft_nms(pp_handle e, int32_t* method, float* sigma, float* score_floor) {
    if (!e || !method || !sigma || !score_floor) return PP_ERR_ARG;
    *method = e->rule.soft_method; *sigma = e->rule.soft_sigma; *score_floor = e->rule.soft_floor;
    return PP_OK;
}

int pp_soft_nms(int device, const float* dets, int64_t n, int32_t method, float sigma, float iou_threshold,
                float score_floor, int32_t pre_max_size, int32_t post_max_size, int32_t* keep, float* scores,
                int64_t* n_keep) {
    const char* who = "pp_soft_nms";
    if (n < 0 || (n > 0 && !dets) || !n_keep) return fail(nullptr, PP_ERR_ARG, "%s: bad argument", who);
    *n_keep = 0;
    if (const char* why = soft_nms_args(method, sigma, score_floor)) return fail(nullptr, PP_ERR_ARG, "%s: %s", who, why);
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(dets[5 * i + 4])) return fail(nullptr, PP_ERR_ARG, "%s: score of box %lld is not finite", who, (long long)i);
    const int64_t m = (pre_max_size > 0 && pre_max_size < n) ? (int64_t)pre_max_size : n;
    if (m > PP_SNMS_MAX_BOXES)
        return fail(nullptr, PP_ERR_ARG, "%s: %lld boxes enter the rounds; at most PP_SNMS_MAX_BOXES = %d (set pre_max_size)",
                    who, (long long)m, PP_SNMS_MAX_BOXES);
    if (n > (int64_t)1 << 24) return fail(nullptr, PP_ERR_ARG, "%s: at most %d boxes per call (got %lld)", who, 1 << 24, (long long)n);
    if (int st = check_device(who, device)) return st;
    if (m == 0) return PP_OK;
    if (!keep || !scores) return fail(nullptr, PP_ERR_ARG, "%s: keep or scores is null", who);
    DEVCHK(hipSetDevice(device));
    const int post = (post_max_size > 0 && post_max_size < m) ? post_max_size : (int)m;
    DevBuf d_dets, d_enter, d_order, d_keep, d_scores, d_nk;
    DEVCHK(d_dets.alloc(sizeof(float) * 5 * (size_t)n));
    DEVCHK(d_enter.alloc(sizeof(int) * (size_t)n));
    DEVCHK(d_order.alloc(sizeof(int) * (size_t)m));
    DEVCHK(d_keep.alloc(sizeof(int) * (size_t)post));
    DEVCHK(d_scores.alloc(sizeof(float) * (size_t)post));
    DEVCHK(d_nk.alloc(sizeof(long long)));
    DEVCHK(hipMemcpy(d_dets.p, dets, sizeof(float) * 5 * (size_t)n, hipMemcpyHostToDevice));
    launch_soft_nms((const float*)d_dets.p, (int)n, (int)m, method, iou_threshold, sigma, score_floor, post, (int*)d_enter.p,
                    (int*)d_order.p, (int*)d_keep.p, (float*)d_scores.p, (long long*)d_nk.p, nullptr);
    DEVCHK(hipGetLastError());
    long long nk = 0;
    DEVCHK(hipMemcpy(&nk, d_nk.p, sizeof(nk), hipMemcpyDeviceToHost));
    if (nk < 0 || nk > post) return fail(nullptr, PP_ERR_HIP, "%s: the rounds returned %lld of at most %d boxes", who, nk, post);
    if (nk > 0) {
        DEVCHK(hipMemcpy(keep, d_keep.p, sizeof(int) * (size_t)nk, hipMemcpyDeviceToHost));
        DEVCHK(hipMemcpy(scores, d_scores.p, sizeof(float) * (size_t)nk, hipMemcpyDeviceToHost));
    }
    *n_keep = nk;
    return PP_OK;
}

int pp_rotate_nms(int device, const float* dets, int64_t n, float iou_threshold, int32_t pre_max_size,
                  int32_t post_max_size, int32_t* keep, int64_t* n_keep) {
    const char* who = "pp_rotate_nms";
    if (n < 0 || (n > 0 && !dets) || !n_keep) return fail(nullptr, PP_ERR_ARG, "%s: bad argument", who);
    *n_keep = 0;
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(dets[6 * i + 5])) return fail(nullptr, PP_ERR_ARG, "%s: score of box %lld is not finite", who, (long long)i);
    const int64_t m = (pre_max_size > 0 && pre_max_size < n) ? (int64_t)pre_max_size : n;
    if (m > PP_RNMS_MAX_BOXES)
        return fail(nullptr, PP_ERR_ARG, "%s: %lld boxes enter the suppression; at most PP_RNMS_MAX_BOXES = %d (set pre_max_size)",
                    who, (long long)m, PP_RNMS_MAX_BOXES);
    if (n > (int64_t)1 << 24) return fail(nullptr, PP_ERR_ARG, "%s: at most %d boxes per call (got %lld)", who, 1 << 24, (long long)n);
    if (int st = check_device(who, device)) return st;
    if (m == 0) return PP_OK;
    if (!keep) return fail(nullptr, PP_ERR_ARG, "%s: keep is null", who);
    DEVCHK(hipSetDevice(device));
    const size_t cb = (size_t)((m + 63) / 64);
    DevBuf d_dets, d_order, d_sorted, d_corners, d_mask, d_keep, d_nk;
    DEVCHK(d_dets.alloc(sizeof(float) * 6 * (size_t)n));
    DEVCHK(d_order.alloc(sizeof(int) * (size_t)m));
    DEVCHK(d_sorted.alloc(sizeof(float) * 5 * (size_t)m));
    DEVCHK(d_corners.alloc(sizeof(float) * 9 * (size_t)m));
    DEVCHK(d_mask.alloc(sizeof(unsigned long long) * (size_t)m * cb));
    DEVCHK(d_keep.alloc(sizeof(int) * (size_t)m));
    DEVCHK(d_nk.alloc(sizeof(long long)));
    DEVCHK(hipMemcpy(d_dets.p, dets, sizeof(float) * 6 * (size_t)n, hipMemcpyHostToDevice));
    const int post = (post_max_size > 0 && post_max_size < m) ? post_max_size : (int)m;
    launch_rnms((const float*)d_dets.p, (int)n, (int)m, iou_threshold, post, (int*)d_order.p, (float*)d_sorted.p,
                (float*)d_corners.p, (unsigned long long*)d_mask.p, (int*)d_keep.p, (long long*)d_nk.p, nullptr);
    DEVCHK(hipGetLastError());
    long long nk = 0;
    DEVCHK(hipMemcpy(&nk, d_nk.p, sizeof(nk), hipMemcpyDeviceToHost));
    if (nk < 0 || nk > m) return fail(nullptr, PP_ERR_HIP, "%s: the sweep returned %lld of %lld boxes", who, nk, (long long)m);
    if (nk > 0) DEVCHK(hipMemcpy(keep, d_keep.p, sizeof(int) * (size_t)nk, hipMemcpyDeviceToHost));
    *n_keep = nk;
    return PP_OK;
}

}  // extern "C"
