// C-ABI, frustum crop (pp_frustum_crop*): the resident frames -> their points inside the camera image's frustum, compacted
// into the handle's other input buffer, which becomes the resident one (kernels: frustum_crop.hip)
#include "pp_engine.h"

namespace {

// Everything pp_frustum_crop* refuses, before anything is queued.
int check_crop(pp_engine* e, const char* who, const double* planes, int batch, int flags) {
    if (!planes) return fail(e, PP_ERR_ARG, "%s: planes is NULL", who);
    if (flags & ~PP_CROP_BACK) return fail(e, PP_ERR_ARG, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~PP_CROP_BACK));
    int st = check_resident_call(e, who, batch, "upload frames first"); if (st) return st;
    if ((st = require_host_exact(e, who))) return st;
    if (e->F > crop_max_features())
        return fail(e, PP_ERR_UNSUPPORTED, "%s: num_point_features is %d, rows of up to %d are moved", who, e->F, crop_max_features());
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < 24; ++i)
            if (!std::isfinite(planes[(size_t)b * 24 + i]))
                return fail(e, PP_ERR_ARG, "%s: frame %d: plane %d, value %d is not finite", who, b, i / 4, i % 4);
    return PP_OK;
}

int ensure_crop(pp_engine* e) {
    pp_engine::Crop& g = e->crop;
    if (g.planes) return PP_OK;
    HIPCHK(e, g.h_ring.alloc(e->ring, (size_t)e->B * 24));
    DevAlloc A{e};
    A(&g.kept, (size_t)e->B); A(&g.chunks, 2 * (size_t)e->B * crop_chunks(e->NMAX)); A(&g.planes, (size_t)e->B * 24);   // (planes last: the ready flag)
    return A.st;
}

// Queues planes -> device and the three kernels on `stream` along the rewrite path (pp_engine.h): the frames are written,
// compacted, into the other input buffer; the host then knows bounds only (the sizes before the crop).
int enqueue_crop(pp_engine* e, const double* planes, int batch, int flags, hipStream_t stream) {
    int st;
    if ((st = ensure_crop(e))) return st;
    pp_engine::Crop& g = e->crop;
    int slot;
    HIPCHK(e, e->ring.take(&slot));
    memcpy(g.h_ring.at(slot), planes, (size_t)batch * 24 * sizeof(double));
    Rewrite w;
    if ((st = rewrite_begin(e, batch, stream, &w))) return st;
    HIPCHK(e, g.h_ring.send(slot, g.planes, (size_t)batch * 24, stream));
    HIPCHK(e, e->ring.sent(slot, stream));
    CropParams p;
    memset(&p, 0, sizeof(p));
    p.in = w.src; p.offsets_in = w.offsets_in;
    p.planes = g.planes; p.batch = batch; p.F = e->F; p.stride = crop_chunks(w.max_n);
    p.back = (flags & PP_CROP_BACK) ? 1 : 0;
    p.chunk_cnt = g.chunks; p.chunk_base = g.chunks + (size_t)batch * p.stride;
    p.kept = g.kept; p.offsets_out = e->d_offsets; p.out = e->d_points;
    p.out_rows = (long long)e->B * e->NMAX;
    {
        ProfScope ps(e, nullptr);
        launch_frustum_crop(p, stream);
    }
    if ((st = rewrite_end(e, batch, w, stream))) return st;
    g.batch = batch;
    return PP_OK;
}

}  // namespace

extern "C" {

int pp_frustum_crop(pp_handle e, const double* planes, int32_t batch, int32_t flags, int32_t* kept_out, float* points_out,
                    int64_t points_capacity) {
    if (!e) return PP_ERR_ARG;
    if (!kept_out) return fail(e, PP_ERR_ARG, "pp_frustum_crop: kept_out is NULL");
    int st = check_crop(e, "pp_frustum_crop", planes, batch, flags);
    if (st) return st;
    if ((st = rewrite_run(e, batch, false, [&](hipStream_t s) { return enqueue_crop(e, planes, batch, flags, s); }))) return st;
    return rewrite_sync_tail(e, "pp_frustum_crop", "%s: frame %d: the device kept %d of %d points",
                             "%s: points_out holds %lld points, %d were kept", e->crop.kept, batch, kept_out, points_out, points_capacity);
}

int pp_frustum_crop_async(pp_handle e, const double* planes, int32_t batch, int32_t flags) {
    if (!e) return PP_ERR_ARG;
    if (int st = check_crop(e, "pp_frustum_crop_async", planes, batch, flags)) return st;
    return rewrite_run(e, batch, true, [&](hipStream_t s) { return enqueue_crop(e, planes, batch, flags, s); });
}

int pp_frustum_crop_info(pp_handle e, int32_t* kept_out, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    if (!kept_out) return fail(e, PP_ERR_ARG, "pp_frustum_crop_info: kept_out is NULL");
    if (int st = check_last_run(e, "pp_frustum_crop_info", e->crop.batch, batch, false, "no crop has run", "crop", "frames")) return st;
    (void)hipSetDevice(e->device);
    if (int st = quiesce(e)) return st;              // (an asynchronous crop runs on the copy stream)
    HIPCHK(e, hipMemcpy(kept_out, e->crop.kept, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PP_OK;
}

}  // extern "C"
