// C-ABI, live-camera ingest (pp_ingest_*): PointCloud2 messages (kernels: ingest.hip) or raw depth images (kernels:
// depth_ingest.hip) -> the resident points and offsets.  The two feeds differ in their checks, their frame records and
// their three launches; the staging, the input-buffer flip and the ordering are one path (enqueue_ingest).
#include "pp_engine.h"

namespace {

template <typename Frame>
struct IngestPlanT {
    std::vector<Frame> frames;
    std::vector<int> bound_off;    // [batch + 1] prefix sums of the frames' kept bounds
    int max_bound = 0, stride = 0;
    int64_t bytes = 0;             // byte_offsets[batch] - byte_offsets[0]
};
typedef IngestPlanT<IngFrame> IngestPlan;
typedef IngestPlanT<DepthFrame> DepthPlan;

// What both feeds refuse before they look at a frame.
int check_ingest_call(pp_engine* e, const char* who, const int64_t* bo, const void* L, int batch, const pp_ingest_config* c) {
    if (e->train_pending) return fail(e, PP_ERR_STATE, "%s: a training step is in flight", who);
    if (e->F != 3)
        return fail(e, PP_ERR_UNSUPPORTED, "%s: num_point_features is %d, the live path delivers x y z only (3)", who, e->F);
    if (!bo || !L || !c) return fail(e, PP_ERR_ARG, "%s: null argument", who);
    int st = check_batch(e, batch); if (st) return st;
    if (c->decimate < 1) return fail(e, PP_ERR_ARG, "%s: decimate %d < 1", who, c->decimate);
    if (c->first < 0) return fail(e, PP_ERR_ARG, "%s: first %d < 0", who, c->first);
    return PP_OK;
}

// Everything pp_ingest_pointcloud2* refuses, before anything is queued.
int check_ingest(pp_engine* e, const char* who, const uint8_t* data, const int64_t* bo, const pp_pc2_layout* L, int batch,
                 const pp_ingest_config* c, IngestPlan* plan) {
    int st = check_ingest_call(e, who, bo, L, batch, c); if (st) return st;
    plan->frames.assign((size_t)batch, IngFrame());
    plan->bound_off.assign((size_t)batch + 1, 0);
    for (int b = 0; b < batch; ++b) {
        const pp_pc2_layout& l = L[b];
        if (l.width < 0 || l.height < 0 || l.point_step < 1 || l.row_step < 0)
            return fail(e, PP_ERR_ARG, "%s: frame %d: width %d, height %d, point_step %d, row_step %d", who, b, l.width,
                        l.height, l.point_step, l.row_step);
        const int64_t n_rec = (int64_t)l.width * l.height;
        if (n_rec > (1ll << 30)) return fail(e, PP_ERR_ARG, "%s: frame %d: width %d x height %d records", who, b, l.width, l.height);
        if (l.datatype >> 8)
            return fail(e, PP_ERR_UNSUPPORTED, "%s: frame %d: datatype: x, y and z differ (%d, %d, %d)", who, b,
                        l.datatype & 255, (l.datatype >> 8) & 255, (l.datatype >> 16) & 255);
        if (l.datatype >= 1 && l.datatype <= 6)
            return fail(e, PP_ERR_UNSUPPORTED, "%s: frame %d: datatype %d is an integer type (7 FLOAT32 or 8 FLOAT64)", who, b, l.datatype);
        if (l.datatype != 7 && l.datatype != 8)
            return fail(e, PP_ERR_ARG, "%s: frame %d: unknown datatype %d", who, b, l.datatype);
        const int size = l.datatype == 8 ? 8 : 4;
        const int offs[3] = {l.x_offset, l.y_offset, l.z_offset};
        static const char* const names[3] = {"x_offset", "y_offset", "z_offset"};
        for (int k = 0; k < 3; ++k)
            if (offs[k] < 0 || (int64_t)offs[k] + size > l.point_step)
                return fail(e, PP_ERR_ARG, "%s: frame %d: %s %d (%d bytes) does not fit point_step %d", who, b, names[k], offs[k],
                            size, l.point_step);
        if ((int64_t)l.row_step < (int64_t)l.width * l.point_step)
            return fail(e, PP_ERR_ARG, "%s: frame %d: row_step %d < width %d x point_step %d", who, b, l.row_step, l.width, l.point_step);
        const int64_t need = (int64_t)l.height * l.row_step;
        if (bo[b] < 0 || bo[b + 1] < bo[b] || bo[b + 1] - bo[b] < need)
            return fail(e, PP_ERR_ARG, "%s: frame %d: byte_offsets give it %lld bytes, height %d x row_step %d = %lld needed", who, b,
                        (long long)(bo[b + 1] - bo[b]), l.height, l.row_step, (long long)need);
        const int64_t bound = n_rec > c->first ? (n_rec - c->first + c->decimate - 1) / c->decimate : 0;
        if (bound > e->NMAX)
            return fail(e, PP_ERR_ARG, "%s: frame %d: width %d x height %d keeps up to %lld points > max_points_per_frame=%d", who, b,
                        l.width, l.height, (long long)bound, e->NMAX);
        IngFrame& f = plan->frames[(size_t)b];
        f.byte_off = bo[b] - bo[0];
        f.n_rec = (int)n_rec;
        const bool tight = l.row_step == l.width * l.point_step || l.height <= 1;
        f.width = tight ? (int)n_rec : l.width;
        f.point_step = l.point_step; f.row_step = l.row_step;
        f.x_off = l.x_offset; f.y_off = l.y_offset; f.z_off = l.z_offset;
        f.f64 = l.datatype == 8; f.big_endian = l.is_bigendian != 0;
        f.nchunks = ingest_chunks(f.n_rec);
        plan->stride = std::max(plan->stride, f.nchunks);
        plan->max_bound = std::max(plan->max_bound, (int)bound);
        plan->bound_off[(size_t)b + 1] = plan->bound_off[(size_t)b] + (int)bound;
    }
    plan->bytes = bo[batch] - bo[0];
    if (plan->bytes > 0 && !data) return fail(e, PP_ERR_ARG, "%s: data is NULL", who);
    return PP_OK;
}

// Everything pp_ingest_depth* refuses, before anything is queued.
int check_depth(pp_engine* e, const char* who, const uint8_t* data, const int64_t* bo, const pp_depth_layout* L, int batch,
                const pp_ingest_config* c, DepthPlan* plan) {
    int st = check_ingest_call(e, who, bo, L, batch, c); if (st) return st;
    plan->frames.assign((size_t)batch, DepthFrame());
    plan->bound_off.assign((size_t)batch + 1, 0);
    for (int b = 0; b < batch; ++b) {
        const pp_depth_layout& l = L[b];
        if (l.width < 0 || l.height < 0 || l.row_step < 0)
            return fail(e, PP_ERR_ARG, "%s: frame %d: width %d, height %d, row_step %d", who, b, l.width, l.height, l.row_step);
        const int64_t n_pix = (int64_t)l.width * l.height;
        if (n_pix > (1ll << 30)) return fail(e, PP_ERR_ARG, "%s: frame %d: width %d x height %d pixels", who, b, l.width, l.height);
        if (l.encoding != PP_DEPTH_U16 && l.encoding != PP_DEPTH_F32)
            return fail(e, PP_ERR_ARG, "%s: frame %d: unknown encoding %d (PP_DEPTH_U16 %d or PP_DEPTH_F32 %d)", who, b, l.encoding,
                        (int)PP_DEPTH_U16, (int)PP_DEPTH_F32);
        const int size = l.encoding == PP_DEPTH_F32 ? 4 : 2;
        if ((int64_t)l.row_step < (int64_t)l.width * size)
            return fail(e, PP_ERR_ARG, "%s: frame %d: row_step %d < width %d x %d bytes", who, b, l.row_step, l.width, size);
        const int64_t need = (int64_t)l.height * l.row_step;
        if (bo[b] < 0 || bo[b + 1] < bo[b] || bo[b + 1] - bo[b] < need)
            return fail(e, PP_ERR_ARG, "%s: frame %d: byte_offsets give it %lld bytes, height %d x row_step %d = %lld needed", who, b,
                        (long long)(bo[b + 1] - bo[b]), l.height, l.row_step, (long long)need);
        const float focal[2] = {l.fx, l.fy}, centre[2] = {l.ppx, l.ppy};
        static const char* const fnames[2] = {"fx", "fy"};
        static const char* const cnames[2] = {"ppx", "ppy"};
        for (int k = 0; k < 2; ++k) {
            if (!std::isfinite(focal[k]) || focal[k] == 0.0f)
                return fail(e, PP_ERR_ARG, "%s: frame %d: %s %g is not a finite non-zero focal length", who, b, fnames[k], (double)focal[k]);
            if (!std::isfinite(centre[k]))
                return fail(e, PP_ERR_ARG, "%s: frame %d: %s %g is not finite", who, b, cnames[k], (double)centre[k]);
        }
        if (l.encoding == PP_DEPTH_U16 && !(std::isfinite(l.depth_scale) && l.depth_scale > 0.0f))
            return fail(e, PP_ERR_ARG, "%s: frame %d: depth_scale %g is not a finite positive number", who, b, (double)l.depth_scale);
        if (!(l.z_min <= l.z_max))
            return fail(e, PP_ERR_ARG, "%s: frame %d: z_min %g > z_max %g (or one is NaN)", who, b, (double)l.z_min, (double)l.z_max);
        const int64_t bound = n_pix > c->first ? (n_pix - c->first + c->decimate - 1) / c->decimate : 0;
        if (bound > e->NMAX)
            return fail(e, PP_ERR_ARG, "%s: frame %d: width %d x height %d keeps up to %lld points > max_points_per_frame=%d", who, b,
                        l.width, l.height, (long long)bound, e->NMAX);
        DepthFrame& f = plan->frames[(size_t)b];
        f.byte_off = bo[b] - bo[0];
        f.width = l.width; f.n_pix = (int)n_pix; f.row_step = l.row_step;
        f.tight = l.row_step == l.width * size || l.height <= 1;
        f.f32 = l.encoding == PP_DEPTH_F32; f.big_endian = l.is_bigendian != 0;
        f.nchunks = depth_chunks(f.n_pix);
        f.fx = l.fx; f.fy = l.fy; f.ppx = l.ppx; f.ppy = l.ppy;
        f.depth_scale = l.depth_scale; f.z_min = l.z_min; f.z_max = l.z_max;
        plan->stride = std::max(plan->stride, f.nchunks);
        plan->max_bound = std::max(plan->max_bound, (int)bound);
        plan->bound_off[(size_t)b + 1] = plan->bound_off[(size_t)b] + (int)bound;
    }
    plan->bytes = bo[batch] - bo[0];
    if (plan->bytes > 0 && !data) return fail(e, PP_ERR_ARG, "%s: data is NULL", who);
    return PP_OK;
}

int ensure_ing(pp_engine* e) {
    pp_engine::Ing& g = e->ing;
    if (g.frames) return PP_OK;
    HIPCHK(e, hipHostMalloc((void**)&g.h_ring, (size_t)pp_engine::OFF_RING * e->B * sizeof(pp_engine::Ing::Slot)));
    DevAlloc A{e};
    A(&g.finite, (size_t)e->B); A(&g.kept, (size_t)e->B); A(&g.frames, (size_t)e->B);     // (frames last: the ready flag)
    return A.st;
}

inline void launch_frames(const IngestParams& p, hipStream_t s) { launch_ingest(p, s); }
inline void launch_frames(const DepthIngestParams& p, hipStream_t s) { launch_depth_ingest(p, s); }

// Flips to the other input buffer (as set_offsets does) and queues bytes -> staging -> points + offsets on `stream`
// (the main stream, or the copy stream: it first waits for the pass that last read that buffer).
template <typename Frame>
int enqueue_ingest(pp_engine* e, const uint8_t* data, const int64_t* bo, int batch, const pp_ingest_config* c,
                   const IngestPlanT<Frame>& plan, hipStream_t stream) {
    int st;
    if ((st = ensure_ing(e))) return st;
    const size_t tables = 2 * (size_t)batch * plan.stride;
    if ((size_t)plan.bytes > e->ing.cap_raw || tables > e->ing.cap_chunks) {
        // an ingest queued earlier on the copy stream may still read what dgrow frees (it waits for the main stream only)
        HIPCHK(e, hipStreamSynchronize(e->copy_stream));
        if ((st = dgrow(e, &e->ing.raw, &e->ing.cap_raw, (size_t)plan.bytes))) return st;
        if ((st = dgrow(e, &e->ing.chunks, &e->ing.cap_chunks, tables))) return st;
    }
    e->zc = false;
    const int slot = e->off_slot;
    e->off_slot = (slot + 1) % pp_engine::OFF_RING;
    HIPCHK(e, hipEventSynchronize(e->off_ev[slot]));   // the copy that last used this slot has been consumed
    Frame* ring = (Frame*)(e->ing.h_ring + (size_t)slot * e->B);
    memcpy(ring, plan.frames.data(), (size_t)batch * sizeof(Frame));
    // the kept counts are device values: everything behind this call is sized from the frames' bounds
    set_resident(e, batch, plan.bound_off.data(), plan.max_bound, false);
    e->ing.batch = batch;
    const int nb = flip_input(e);
    HIPCHK(e, hipStreamWaitEvent(stream, e->ev_read[nb], 0));
    if (plan.bytes) HIPCHK(e, hipMemcpyAsync(e->ing.raw, data + bo[0], (size_t)plan.bytes, hipMemcpyHostToDevice, stream));
    HIPCHK(e, hipMemcpyAsync(e->ing.frames, ring, (size_t)batch * sizeof(Frame), hipMemcpyHostToDevice, stream));
    HIPCHK(e, hipEventRecord(e->off_ev[slot], stream));
    IngestParamsT<Frame> p;
    memset(&p, 0, sizeof(p));
    p.raw = e->ing.raw; p.frames = (const Frame*)e->ing.frames; p.batch = batch; p.stride = plan.stride;
    p.first = c->first; p.decimate = c->decimate;
    memcpy(p.r, c->r, sizeof(p.r)); memcpy(p.r2, c->r2, sizeof(p.r2)); memcpy(p.lift, c->lift, sizeof(p.lift));
    p.chunk_cnt = e->ing.chunks; p.chunk_base = e->ing.chunks + (size_t)batch * plan.stride;
    p.finite = e->ing.finite; p.kept = e->ing.kept; p.offsets = e->d_offsets; p.out = e->d_points;
    p.out_rows = (long long)e->B * e->NMAX;
    {
        ProfScope ps(e, nullptr);
        launch_frames(p, stream);
    }
    HIPCHK(e, hipGetLastError());
    return PP_OK;
}

// the synchronous call of either feed: queue on the main stream, wait, hand out the parity tap
template <typename Frame>
int ingest_sync(pp_engine* e, const char* who, const uint8_t* data, const int64_t* byte_offsets, int batch,
                const pp_ingest_config* cfg, const IngestPlanT<Frame>& plan, float* points_out, int64_t points_out_capacity) {
    int st;
    // an asynchronous ingest still running on the copy stream uses the same staging and chunk tables
    HIPCHK(e, hipStreamWaitEvent(e->stream, e->ev_up, 0));
    prof_reset(e);
    if ((st = enqueue_ingest(e, data, byte_offsets, batch, cfg, plan, e->stream))) return st;
    e->up_pending = false;
    HIPCHK(e, hipStreamSynchronize(e->stream));      // the host buffers may be pageable / reused by the caller
    if (points_out) {
        int total = 0;
        HIPCHK(e, hipMemcpy(&total, e->d_offsets + batch, sizeof(int), hipMemcpyDeviceToHost));
        if (points_out_capacity < total)
            return fail(e, PP_ERR_ARG, "%s: points_out holds %lld points, %d were kept", who, (long long)points_out_capacity, total);
        if (total) HIPCHK(e, hipMemcpy(points_out, e->d_points, (size_t)total * 3 * sizeof(float), hipMemcpyDeviceToHost));
    }
    return PP_OK;
}

}  // namespace

extern "C" {

int pp_ingest_pointcloud2(pp_handle e, const uint8_t* data, const int64_t* byte_offsets, const pp_pc2_layout* layouts,
                          int32_t batch, const pp_ingest_config* cfg, float* points_out, int64_t points_out_capacity) {
    if (!e) return PP_ERR_ARG;
    (void)hipSetDevice(e->device);
    IngestPlan plan;
    int st = check_ingest(e, "pp_ingest_pointcloud2", data, byte_offsets, layouts, batch, cfg, &plan);
    if (st) return st;
    return ingest_sync(e, "pp_ingest_pointcloud2", data, byte_offsets, batch, cfg, plan, points_out, points_out_capacity);
}

int pp_ingest_pointcloud2_async(pp_handle e, const uint8_t* data_pinned, const int64_t* byte_offsets,
                                const pp_pc2_layout* layouts, int32_t batch, const pp_ingest_config* cfg) {
    if (!e) return PP_ERR_ARG;
    (void)hipSetDevice(e->device);
    IngestPlan plan;
    int st = check_ingest(e, "pp_ingest_pointcloud2_async", data_pinned, byte_offsets, layouts, batch, cfg, &plan);
    if (st) return st;
    prof_reset(e);
    if ((st = enqueue_ingest(e, data_pinned, byte_offsets, batch, cfg, plan, e->copy_stream))) return st;
    return finish_async_upload(e, batch);     // as pp_upload_points_async does
}

int pp_ingest_depth(pp_handle e, const uint8_t* data, const int64_t* byte_offsets, const pp_depth_layout* layouts,
                    int32_t batch, const pp_ingest_config* cfg, float* points_out, int64_t points_out_capacity) {
    if (!e) return PP_ERR_ARG;
    (void)hipSetDevice(e->device);
    DepthPlan plan;
    int st = check_depth(e, "pp_ingest_depth", data, byte_offsets, layouts, batch, cfg, &plan);
    if (st) return st;
    return ingest_sync(e, "pp_ingest_depth", data, byte_offsets, batch, cfg, plan, points_out, points_out_capacity);
}

int pp_ingest_depth_async(pp_handle e, const uint8_t* data_pinned, const int64_t* byte_offsets,
                          const pp_depth_layout* layouts, int32_t batch, const pp_ingest_config* cfg) {
    if (!e) return PP_ERR_ARG;
    (void)hipSetDevice(e->device);
    DepthPlan plan;
    int st = check_depth(e, "pp_ingest_depth_async", data_pinned, byte_offsets, layouts, batch, cfg, &plan);
    if (st) return st;
    prof_reset(e);
    if ((st = enqueue_ingest(e, data_pinned, byte_offsets, batch, cfg, plan, e->copy_stream))) return st;
    return finish_async_upload(e, batch);     // as pp_upload_points_async does
}

int pp_ingest_info(pp_handle e, int32_t* finite_counts, int32_t* kept_counts, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_ingest_info: a training step is in flight");
    if (e->ing.batch < 1) return fail(e, PP_ERR_STATE, "pp_ingest_info: no ingest has run");
    if (batch != e->ing.batch) return fail(e, PP_ERR_ARG, "pp_ingest_info: the last ingest had %d frames, batch is %d", e->ing.batch, batch);
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipEventSynchronize(e->ev_up));        // an asynchronous ingest runs on the copy stream
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const size_t n = (size_t)batch * sizeof(int32_t);
    if (finite_counts) HIPCHK(e, hipMemcpy(finite_counts, e->ing.finite, n, hipMemcpyDeviceToHost));
    if (kept_counts) HIPCHK(e, hipMemcpy(kept_counts, e->ing.kept, n, hipMemcpyDeviceToHost));
    return PP_OK;
}

}  // extern "C"
