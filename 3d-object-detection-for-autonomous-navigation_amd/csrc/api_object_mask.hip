// C-ABI, the per-point object mask (pp_set_object_mask, pp_get_object_mask_config, pp_object_mask_async,
// pp_object_mask_shape, pp_get_object_mask, pp_object_mask_points): the resident rows and the last pass's detections or the
// streams' track slots -> one bit per row, on the device (kernels: object_mask.hip; the rule: object_mask.py).  A stage of
// its own, queued on the handle's stream as plain launches.  The occupancy update, the scan match and the costmap's point
// layer read the words through object_mask_for (pp_engine.h) and know nothing else of this stage.  The poses and dt values
// of a call travel from the host and are consumed on the main stream: a call ring of the stage's own (pp_ring.h).
// pp_object_mask_points needs no handle: host buffers in, host buffers out, device memory for the call's duration.
#include "pp_engine.h"

static_assert(sizeof(pp_object_mask_config) == 40, "pp_object_mask_config: 3 doubles, 4 int32 (the Python binding mirrors it)");
static_assert(PP_OBJMASK_MAX_FOOTPRINTS == 128 && PP_OBJMASK_INFO == 4, "a frame's table; its info words");

namespace {

constexpr int OM_ALL = PP_OBJMASK_OCCUPANCY | PP_OBJMASK_SCAN_MATCH | PP_OBJMASK_COSTMAP;

// Everything pp_set_object_mask refuses of a configuration, by field name.
int check_config(pp_engine* e, const pp_object_mask_config& c) {
    const char* who = "pp_set_object_mask";
    if (int st = check_cfg_doubles(e, who, {{"min_score", c.min_score, true}, {"min_speed", c.min_speed, true}, {"pad", c.pad, true}})) return st;
    if (!(c.min_speed >= 0.0)) return fail(e, PP_ERR_ARG, "%s: min_speed = %g must be >= 0", who, c.min_speed);
    if (!(c.pad >= 0.0)) return fail(e, PP_ERR_ARG, "%s: pad = %g must be >= 0", who, c.pad);
    if (c.objects != OM_DETECTIONS && c.objects != OM_TRACKS)
        return fail(e, PP_ERR_ARG, "%s: objects = %d (1 detections, 2 tracks)", who, c.objects);
    if (c.consumers < 0 || (c.consumers & ~OM_ALL))
        return fail(e, PP_ERR_ARG, "%s: consumers = %d holds bits outside PP_OBJMASK_OCCUPANCY | PP_OBJMASK_SCAN_MATCH | PP_OBJMASK_COSTMAP = %d",
                    who, c.consumers, OM_ALL);
    if (c.reserved != 0) return fail(e, PP_ERR_ARG, "%s: reserved = %d must be 0", who, c.reserved);
    return PP_OK;
}

int make_buffers(pp_engine* e) {
    pp_engine::ObjMask& g = e->omask;
    const size_t B = (size_t)e->B;
    HIPCHK(e, g.h_call.alloc(g.ring, B));
    if (g.d_call) return PP_OK;
    const int stride = 4 * ((e->NMAX + 255) / 256);
    DevAlloc A{e};
    A(&g.table, B * PP_OBJMASK_MAX_FOOTPRINTS); A(&g.info, B * PP_OBJMASK_INFO); A(&g.words, B * (size_t)std::max(stride, 1));
    A(&g.d_call, B);                                     // (d_call last: the ready flag)
    if (A.st) return A.st;
    g.stride = stride;
    return PP_OK;
}

}  // namespace

void object_mask_release(pp_engine* e) {
    e->omask.ring.release();
    e->omask = pp_engine::ObjMask();
}

extern "C" {

int pp_set_object_mask(pp_handle e, const pp_object_mask_config* cfg) {
    if (!e) return PP_ERR_ARG;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_object_mask: a training step is in flight");
    pp_engine::ObjMask& g = e->omask;
    if (!cfg) { g.on = false; return PP_OK; }
    pp_object_mask_config c = *cfg;
    if (int st = check_config(e, c)) return st;
    c.confirmed_only = c.confirmed_only ? 1 : 0;
    (void)hipSetDevice(e->device);
    if (int st = make_buffers(e)) return st;
    if (memcmp(&c, &g.cfg, sizeof(c)) != 0) g.batch = 0;   // the last mask is another rule's
    g.cfg = c;
    g.on = true;
    return PP_OK;
}

int pp_get_object_mask_config(pp_handle e, int32_t* on, pp_object_mask_config* cfg_out) {
    if (!e || !on) return PP_ERR_ARG;
    *on = e->omask.on ? 1 : 0;
    if (cfg_out) *cfg_out = e->omask.cfg;
    return PP_OK;
}

int pp_object_mask_async(pp_handle e, const double* poses, const double* dt, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_object_mask_async";
    pp_engine::ObjMask& g = e->omask;
    if (!g.on) return fail(e, PP_ERR_STATE, "%s: the object mask is not configured (pp_set_object_mask first)", who);
    if (int st = check_resident_call(e, who, batch, "upload or ingest frames first")) return st;
    const pp_object_mask_config& c = g.cfg;
    if (c.objects == OM_DETECTIONS) {
        if (poses || dt) return fail(e, PP_ERR_ARG, "%s: objects = detections takes neither poses nor dt (they bring tracks to now)", who);
        if (e->results_batch != batch || e->results_gen != e->resident_gen || e->results_rows < 1)
            return fail(e, PP_ERR_STATE, "%s: objects = detections and no pass has run on the resident frames (pp_detect_async first)", who);
        if (e->results_rows > PP_OBJMASK_MAX_FOOTPRINTS)
            return fail(e, PP_ERR_UNSUPPORTED, "%s: %d detection rows per frame; a frame's footprint table holds %d (lower nms_post_max_size, "
                        "or use the joint class mode)", who, e->results_rows, PP_OBJMASK_MAX_FOOTPRINTS);
    } else {
        if (!e->trk.configured) return fail(e, PP_ERR_STATE, "%s: objects = tracks and pp_set_tracking has given no configuration", who);
        if (dt)
            for (int b = 0; b < batch; ++b)
                if (!std::isfinite(dt[b]) || !(dt[b] >= 0.0))
                    return fail(e, PP_ERR_ARG, "%s: dt of stream %d is %g (must be finite and >= 0)", who, b, dt[b]);
        if (poses)
            if (int st = check_poses(e, who, poses, nullptr, batch, [](int, const double*) { return (int)PP_OK; })) return st;
    }
    (void)hipSetDevice(e->device);
    OmParams p;
    memset(&p, 0, sizeof(p));
    const bool rides = poses || dt;
    int slot = -1;
    if (rides) {
        HIPCHK(e, g.ring.take(&slot));                   // behind the last check that can refuse
        OmCall* call = g.h_call.at(slot);
        for (int b = 0; b < batch; ++b) {
            OmCall& k = call[b];
            memset(&k, 0, sizeof(k));
            if (poses) {
                const double* P = poses + (size_t)b * 12;
                memcpy(k.m, P, 12 * sizeof(double));
                k.psi = std::atan2(P[4], P[0]);          // as pp_set_track_pose computes it: atan2(R10, R00)
                k.has_pose = 1;
            }
            if (dt) { k.dt = dt[b]; k.has_dt = 1; }
        }
    }
    if (int st = resident_points(e, batch, e->stream, false, &p.points)) return st;
    p.cfg = c; p.objects = c.objects;
    p.batch = batch; p.F = e->F; p.max_n = std::min(e->cur_max_n, e->NMAX);
    p.offsets = e->d_offsets;
    p.dets = e->d_dets; p.n_dets = e->d_ndets; p.det_rows = c.objects == OM_DETECTIONS ? e->results_rows : 0;
    p.slots = e->trk.state; p.pose_prev = e->trk.d_pose_prev;
    p.call = rides ? g.d_call : nullptr;
    p.table = g.table; p.info = g.info; p.words = g.words; p.stride = g.stride;
    prof_reset(e);
    if (rides) {
        HIPCHK(e, g.h_call.send(slot, g.d_call, (size_t)batch, e->stream));
        HIPCHK(e, g.ring.sent(slot, e->stream));
    }
    {
        ProfScope ps(e, nullptr);
        launch_object_mask(p, e->stream);
    }
    HIPCHK(e, hipGetLastError());
    // the next upload but one writes the buffer read here: its writer waits for this event as for a pass
    HIPCHK(e, hipEventRecord(e->ev_read[e->in_buf], e->stream));
    g.batch = batch; g.run_words = (p.max_n + 63) / 64; g.gen = e->resident_gen;
    return PP_OK;
}

int pp_object_mask_shape(pp_handle e, int32_t* batch, int32_t* words_per_frame) {
    if (!e || !batch || !words_per_frame) return PP_ERR_ARG;
    *batch = e->omask.batch;
    *words_per_frame = e->omask.batch ? e->omask.run_words : 0;
    return PP_OK;
}

int pp_get_object_mask(pp_handle e, uint64_t* words, int32_t* info, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_get_object_mask";
    pp_engine::ObjMask& g = e->omask;
    if (int st = check_last_run(e, who, g.batch, batch, true, "no mask has been computed (pp_object_mask_async first)", "mask", "frames")) return st;
    if (g.gen != e->resident_gen)
        return fail(e, PP_ERR_STATE, "%s: the frames the last mask belongs to are gone (pp_object_mask_async again)", who);
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (words && g.run_words > 0)
        HIPCHK(e, hipMemcpy2D(words, (size_t)g.run_words * 8, g.words, (size_t)g.stride * 8, (size_t)g.run_words * 8, (size_t)batch,
                              hipMemcpyDeviceToHost));
    if (info) HIPCHK(e, hipMemcpy(info, g.info, (size_t)batch * PP_OBJMASK_INFO * sizeof(int), hipMemcpyDeviceToHost));
    return PP_OK;
}

int pp_object_mask_points(int device, const float* points, const int32_t* offsets, int32_t num_features, int32_t batch,
                          const double* footprints, const int32_t* counts, double pad, uint64_t* words, int32_t words_per_frame,
                          int32_t* info) {
    const char* who = "pp_object_mask_points";
    if (!offsets || !counts) return fail(nullptr, PP_ERR_ARG, "%s: offsets or counts is NULL", who);
    if (batch < 1 || batch > 65535) return fail(nullptr, PP_ERR_ARG, "%s: batch = %d outside [1, 65535]", who, batch);
    if (num_features < 3) return fail(nullptr, PP_ERR_ARG, "%s: num_features = %d must be >= 3", who, num_features);
    if (!std::isfinite(pad) || !(pad >= 0.0)) return fail(nullptr, PP_ERR_ARG, "%s: pad = %g must be finite and >= 0", who, pad);
    if (offsets[0] != 0) return fail(nullptr, PP_ERR_ARG, "%s: offsets[0] must be 0", who);
    int max_n = 0;
    std::vector<int> fp_off((size_t)batch + 1, 0);
    for (int b = 0; b < batch; ++b) {
        if (offsets[b + 1] < offsets[b]) return fail(nullptr, PP_ERR_ARG, "%s: offsets not monotone at frame %d", who, b);
        max_n = std::max(max_n, offsets[b + 1] - offsets[b]);
        if (counts[b] < 0 || counts[b] > PP_OBJMASK_MAX_FOOTPRINTS)
            return fail(nullptr, PP_ERR_ARG, "%s: counts[%d] = %d outside [0, PP_OBJMASK_MAX_FOOTPRINTS = %d]", who, b, counts[b],
                        PP_OBJMASK_MAX_FOOTPRINTS);
        fp_off[(size_t)b + 1] = fp_off[(size_t)b] + counts[b];
    }
    const size_t total = (size_t)offsets[batch], nfp = (size_t)fp_off[(size_t)batch];
    if (total && !points) return fail(nullptr, PP_ERR_ARG, "%s: points is NULL", who);
    if (nfp && !footprints) return fail(nullptr, PP_ERR_ARG, "%s: footprints is NULL", who);
    const int run_words = (max_n + 63) / 64;
    if (words && words_per_frame < run_words)
        return fail(nullptr, PP_ERR_ARG, "%s: words_per_frame = %d, the longest frame has %d rows: %d words", who, words_per_frame, max_n, run_words);
    if (int st = check_device(who, device)) return st;
    DEVCHK(hipSetDevice(device));
    OmParams p;
    memset(&p, 0, sizeof(p));
    p.cfg.pad = pad; p.objects = OM_GIVEN;
    p.batch = batch; p.F = num_features; p.max_n = max_n;
    p.stride = 4 * ((max_n + 255) / 256);
    DevBuf d_pts, d_off, d_fp, d_fpoff, d_table, d_info, d_words;
    DEVCHK(d_pts.alloc(total * num_features * sizeof(float)));
    DEVCHK(d_off.alloc((size_t)(batch + 1) * sizeof(int)));
    DEVCHK(d_fp.alloc(nfp * 5 * sizeof(double)));
    DEVCHK(d_fpoff.alloc((size_t)(batch + 1) * sizeof(int)));
    DEVCHK(d_table.alloc((size_t)batch * PP_OBJMASK_MAX_FOOTPRINTS * sizeof(OmFootprint)));
    DEVCHK(d_info.alloc((size_t)batch * PP_OBJMASK_INFO * sizeof(int)));
    DEVCHK(d_words.alloc((size_t)batch * p.stride * sizeof(unsigned long long)));
    if (total) DEVCHK(hipMemcpy(d_pts.p, points, total * num_features * sizeof(float), hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_off.p, offsets, (size_t)(batch + 1) * sizeof(int), hipMemcpyHostToDevice));
    if (nfp) DEVCHK(hipMemcpy(d_fp.p, footprints, nfp * 5 * sizeof(double), hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_fpoff.p, fp_off.data(), (size_t)(batch + 1) * sizeof(int), hipMemcpyHostToDevice));
    p.points = (const float*)d_pts.p; p.offsets = (const int*)d_off.p;
    p.given = (const double*)d_fp.p; p.given_off = (const int*)d_fpoff.p;
    p.table = (OmFootprint*)d_table.p; p.info = (int*)d_info.p; p.words = (unsigned long long*)d_words.p;
    launch_object_mask(p, nullptr);
    DEVCHK(hipGetLastError());
    DEVCHK(hipStreamSynchronize(nullptr));
    if (words) {
        memset(words, 0, (size_t)batch * words_per_frame * sizeof(uint64_t));
        if (run_words > 0)
            DEVCHK(hipMemcpy2D(words, (size_t)words_per_frame * 8, p.words, (size_t)p.stride * 8, (size_t)run_words * 8, (size_t)batch,
                               hipMemcpyDeviceToHost));
    }
    if (info) DEVCHK(hipMemcpy(info, p.info, (size_t)batch * PP_OBJMASK_INFO * sizeof(int), hipMemcpyDeviceToHost));
    return PP_OK;
}

}  // extern "C"
