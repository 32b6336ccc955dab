// C-ABI, image boxes: the detector's projection (per handle; the kernel instantiations are in postprocess.hip) and the
// standalone projection of any camera-frame boxes (kernel: box_project.hip).  The latter needs no handle: host buffers
// in, host buffers out, device memory for the call's duration.
#include <cstring>

#include "pp_engine.h"

extern "C" {

int pp_set_projection(pp_handle e, const double* p2, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    pp_engine::Projection& pj = e->proj;
    if (p2 == nullptr) {
        if (!e->rule.proj) return PP_OK;
        if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_projection: a training step is in flight");
        e->rule.proj = 0;
        return PP_OK;
    }
    if (batch < 1 || batch > e->B) return fail(e, PP_ERR_ARG, "pp_set_projection: batch=%d outside [1, max_batch=%d]", batch, e->B);
    const size_t n = (size_t)batch * 16;
    if (e->rule.proj && pj.batch == batch && memcmp(pj.h_p2.data(), p2, n * sizeof(double)) == 0) return PP_OK;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_projection: a training step is in flight");
    (void)hipSetDevice(e->device);
    if (pj.d_p2 == nullptr) {
        const size_t rows = (size_t)e->B * e->ncls * e->cfg.nms_post_max_size;   // the per-class mode's rows (pp_set_class_nms)
        DevAlloc A{e};
        A(&pj.d_p2, (size_t)e->B * 16);
        A(&pj.d_bbox, rows * 4);
        A(&pj.d_cls_bbox, rows * 4);
        if (A.st != PP_OK) { pj.d_p2 = nullptr; return A.st; }
        HIPCHK(e, hipHostMalloc((void**)&pj.h_bbox, rows * 4 * sizeof(double)));
    }
    // on the engine's stream, behind whatever pass is still reading the matrices; a replayed graph reads the new ones
    // (the source is pageable: the call returns once it has been staged)
    HIPCHK(e, hipMemcpyAsync(pj.d_p2, p2, n * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    pj.h_p2.assign(p2, p2 + n);
    pj.batch = batch;
    e->rule.proj = 1;
    return PP_OK;
}

int pp_get_projection(pp_handle e, int32_t* on) {
    if (!e || !on) return PP_ERR_ARG;
    *on = e->rule.proj;
    return PP_OK;
}

int pp_get_bboxes(pp_handle e, double* bbox) {
    if (!e) return PP_ERR_ARG;
    if (!bbox) return fail(e, PP_ERR_ARG, "pp_get_bboxes: NULL argument");
    const int B = e->proj.results;
    if (B < 1) return fail(e, PP_ERR_STATE, "pp_get_bboxes: the last pass ran without projection (pp_set_projection), or there are no results on this handle");
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (int st = check_numeric(e, e->h_ndets, B, "pp_get_bboxes")) return st;
    if (e->results_rows != det_rows(e))
        return fail(e, PP_ERR_STATE, "pp_get_bboxes: the last pass ran in the other class mode (pp_set_class_nms): run a new one");
    const size_t pm = (size_t)e->results_rows;
    for (int b = 0; b < B; ++b) {
        const size_t n = (size_t)std::max(0, std::min(e->h_ndets[b], (int)pm));
        memcpy(bbox + (size_t)b * pm * 4, e->proj.h_bbox + (size_t)b * pm * 4, n * 4 * sizeof(double));
    }
    return PP_OK;
}

int pp_box3d_to_bbox(int device, const double* boxes_camera, const int32_t* box_counts, int32_t frames, const double* p2,
                     double* bbox) {
    const char* who = "pp_box3d_to_bbox";
    if (frames < 0 || (frames > 0 && (!box_counts || !p2))) return fail(nullptr, PP_ERR_ARG, "%s: bad argument", who);
    std::vector<long long> start((size_t)frames + 1, 0);
    for (int f = 0; f < frames; ++f) {
        if (box_counts[f] < 0) return fail(nullptr, PP_ERR_ARG, "%s: box_counts[%d] = %d is negative", who, f, box_counts[f]);
        start[f + 1] = start[f] + box_counts[f];
    }
    const long long n = start[frames];
    if (n == 0) return PP_OK;
    if (!boxes_camera || !bbox) return fail(nullptr, PP_ERR_ARG, "%s: NULL boxes", who);
    if (n > (1ll << 31) * 256 - 256) return fail(nullptr, PP_ERR_ARG, "%s: too many boxes (%lld)", who, n);
    if (int st = check_device(who, device)) return st;
    DEVCHK(hipSetDevice(device));
    DevBuf d_boxes, d_start, d_p2, d_bbox;
    DEVCHK(d_boxes.alloc(sizeof(double) * 7 * (size_t)n));
    DEVCHK(d_start.alloc(sizeof(long long) * start.size()));
    DEVCHK(d_p2.alloc(sizeof(double) * 16 * (size_t)frames));
    DEVCHK(d_bbox.alloc(sizeof(double) * 4 * (size_t)n));
    DEVCHK(hipMemcpy(d_boxes.p, boxes_camera, sizeof(double) * 7 * (size_t)n, hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_start.p, start.data(), sizeof(long long) * start.size(), hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_p2.p, p2, sizeof(double) * 16 * (size_t)frames, hipMemcpyHostToDevice));
    launch_box3d_to_bbox((const double*)d_boxes.p, n, (const long long*)d_start.p, frames, (const double*)d_p2.p,
                         (double*)d_bbox.p, nullptr);
    DEVCHK(hipGetLastError());
    DEVCHK(hipMemcpy(bbox, d_bbox.p, sizeof(double) * 4 * (size_t)n, hipMemcpyDeviceToHost));
    return PP_OK;
}

}  // extern "C"
