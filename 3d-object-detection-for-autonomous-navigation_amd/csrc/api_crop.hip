// C-ABI, frustum crop (pp_frustum_crop*): the resident frames -> their points inside the camera image's frustum, compacted
// into the handle's other input buffer, which becomes the resident one (kernels: frustum_crop.hip)
#include "pp_engine.h"

namespace {

// Everything pp_frustum_crop* refuses, before anything is queued.
int check_crop(pp_engine* e, const char* who, const double* planes, int batch, int flags) {
    if (e->train_pending) return fail(e, PP_ERR_STATE, "%s: a training step is in flight", who);
    if (!planes) return fail(e, PP_ERR_ARG, "%s: planes is NULL", who);
    if (flags & ~PP_CROP_BACK) return fail(e, PP_ERR_ARG, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~PP_CROP_BACK));
    if (e->cur_batch < 1) return fail(e, PP_ERR_STATE, "%s: no frames are resident (upload frames first)", who);
    int st = check_batch(e, batch); if (st) return st;
    if (batch != e->cur_batch) return fail(e, PP_ERR_ARG, "%s: %d frames are resident, batch is %d", who, e->cur_batch, batch);
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
    if (!g.ev_main) HIPCHK(e, hipEventCreateWithFlags(&g.ev_main, hipEventDisableTiming));
    if (!g.h_ring) HIPCHK(e, hipHostMalloc((void**)&g.h_ring, (size_t)pp_engine::OFF_RING * e->B * 24 * sizeof(double)));
    DevAlloc A{e};
    A(&g.kept, (size_t)e->B); A(&g.chunks, 2 * (size_t)e->B * crop_chunks(e->NMAX)); A(&g.planes, (size_t)e->B * 24);   // (planes last: the ready flag)
    return A.st;
}

// Queues planes -> device and the three kernels on `stream` (the main stream, or the copy stream): the resident frames are
// read where they lie (a zero-copy feed in the caller's page-locked memory) and written, compacted, into the other input
// buffer, to which the handle flips.  The host then knows bounds only (the sizes before the crop): set_resident, not exact.
int enqueue_crop(pp_engine* e, const double* planes, int batch, int flags, hipStream_t stream) {
    int st;
    if ((st = ensure_crop(e))) return st;
    pp_engine::Crop& g = e->crop;
    const int slot = e->off_slot;
    e->off_slot = (slot + 1) % pp_engine::OFF_RING;
    HIPCHK(e, hipEventSynchronize(e->off_ev[slot]));   // the copy that last used this slot has been consumed
    double* ring = g.h_ring + (size_t)slot * e->B * 24;
    memcpy(ring, planes, (size_t)batch * 24 * sizeof(double));
    CropParams p;
    memset(&p, 0, sizeof(p));
    if ((st = resident_points(e, batch, stream, true, &p.in))) return st;
    p.offsets_in = e->d_offsets;
    const std::vector<int> bound = e->h_cur_off;       // (set_resident assigns the vector it would otherwise read)
    const int max_n = e->cur_max_n;
    const int old = e->in_buf;
    const int nb = flip_input(e);
    HIPCHK(e, hipStreamWaitEvent(stream, e->ev_read[nb], 0));   // the pass that last read the buffer written here
    HIPCHK(e, hipMemcpyAsync(g.planes, ring, (size_t)batch * 24 * sizeof(double), hipMemcpyHostToDevice, stream));
    HIPCHK(e, hipEventRecord(e->off_ev[slot], stream));
    p.planes = g.planes; p.batch = batch; p.F = e->F; p.stride = crop_chunks(max_n);
    p.back = (flags & PP_CROP_BACK) ? 1 : 0;
    p.chunk_cnt = g.chunks; p.chunk_base = g.chunks + (size_t)batch * p.stride;
    p.kept = g.kept; p.offsets_out = e->d_offsets; p.out = e->d_points;
    p.out_rows = (long long)e->B * e->NMAX;
    {
        ProfScope ps(e, nullptr);
        launch_frustum_crop(p, stream);
    }
    HIPCHK(e, hipGetLastError());
    // the next upload flips back to the buffer read here: its writer waits for this event as for a pass
    if (stream != e->stream) HIPCHK(e, hipEventRecord(e->ev_read[old], stream));
    set_resident(e, batch, bound.data(), max_n, false);
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
    (void)hipSetDevice(e->device);
    // an asynchronous crop still running on the copy stream uses the same chunk tables
    HIPCHK(e, hipStreamWaitEvent(e->stream, e->ev_up, 0));
    prof_reset(e);
    if ((st = enqueue_crop(e, planes, batch, flags, e->stream))) return st;
    HIPCHK(e, hipMemcpyAsync(kept_out, e->crop.kept, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    // the counts read back become the host's copy of the offsets: everything downstream is sized from them
    std::vector<int> off((size_t)batch + 1, 0);
    int max_n = 0;
    for (int b = 0; b < batch; ++b) {
        const int bound = e->h_cur_off[(size_t)b + 1] - e->h_cur_off[(size_t)b];
        if (kept_out[b] < 0 || kept_out[b] > bound) return fail(e, PP_ERR_HIP, "pp_frustum_crop: frame %d: the device kept %d of %d points", b, kept_out[b], bound);
        off[(size_t)b + 1] = off[(size_t)b] + kept_out[b];
        max_n = std::max(max_n, kept_out[b]);
    }
    set_resident(e, batch, off.data(), max_n, true);
    if (points_out) {
        const int total = off[(size_t)batch];
        if (points_capacity < total)
            return fail(e, PP_ERR_ARG, "pp_frustum_crop: points_out holds %lld points, %d were kept", (long long)points_capacity, total);
        if (total) HIPCHK(e, hipMemcpy(points_out, e->d_points, (size_t)total * e->F * sizeof(float), hipMemcpyDeviceToHost));
    }
    return PP_OK;
}

int pp_frustum_crop_async(pp_handle e, const double* planes, int32_t batch, int32_t flags) {
    if (!e) return PP_ERR_ARG;
    int st = check_crop(e, "pp_frustum_crop_async", planes, batch, flags);
    if (st) return st;
    (void)hipSetDevice(e->device);
    if ((st = ensure_crop(e))) return st;
    // frames fed on the main stream (pp_upload_points_device) must have arrived, and the pass in flight reads the buffer
    // this crop writes: the copy stream waits for what the main stream holds now
    HIPCHK(e, hipEventRecord(e->crop.ev_main, e->stream));
    HIPCHK(e, hipStreamWaitEvent(e->copy_stream, e->crop.ev_main, 0));
    prof_reset(e);
    if ((st = enqueue_crop(e, planes, batch, flags, e->copy_stream))) return st;
    return finish_async_upload(e, batch);     // as pp_upload_points_async does
}

int pp_frustum_crop_info(pp_handle e, int32_t* kept_out, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    if (!kept_out) return fail(e, PP_ERR_ARG, "pp_frustum_crop_info: kept_out is NULL");
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_frustum_crop_info: a training step is in flight");
    if (e->crop.batch < 1) return fail(e, PP_ERR_STATE, "pp_frustum_crop_info: no crop has run");
    if (batch != e->crop.batch) return fail(e, PP_ERR_ARG, "pp_frustum_crop_info: the last crop had %d frames, batch is %d", e->crop.batch, batch);
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipEventSynchronize(e->ev_up));        // an asynchronous crop runs on the copy stream
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(kept_out, e->crop.kept, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PP_OK;
}

}  // extern "C"
