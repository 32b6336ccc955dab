// C-ABI, tracking across frames: one track table per stream (frame b of a pass is stream b), advanced by k_track_step
// (track.hip) behind the detector's post-process -- on / off is PostRule::track -- or on host-given rows (pp_track_update).
#include "pp_engine.h"

static_assert(sizeof(pp_track_config) == 80, "pp_track_config: 8 doubles, 4 int32 (the Python binding mirrors it)");
static_assert(sizeof(pp_track) == 112, "pp_track: 10 doubles, a float, 7 int32 (the Python binding mirrors it)");
static_assert(PP_TRACK_MAX == PP_WAVE, "k_track_step: one lane per track slot");

namespace {

int ensure_track(pp_engine* e) {
    pp_engine::Track& t = e->trk;
    if (t.ready) return PP_OK;
    const size_t B = (size_t)e->B;
    DevAlloc A{e};
    A(&t.d_cfg, 1);
    A(&t.state, B * PP_TRACK_MAX);
    A(&t.next_id, B);
    A(&t.overflow, B);
    A(&t.d_dt, B);
    A(&t.in_dets, B * PP_TRACK_MASK_ROWS);
    A(&t.in_n, B);
    A(&t.d_pose_q, B);
    A(&t.d_pose_prev, B);
    if (A.st) return A.st;
    HIPCHK(e, t.h_dt.alloc(t.dt_ring, B));
    HIPCHK(e, t.h_pose.alloc(t.pose_ring, B));
    HIPCHK(e, hipHostMalloc((void**)&t.h_out, B * PP_TRACK_MAX * sizeof(pp_track)));
    HIPCHK(e, hipHostMalloc((void**)&t.h_nout, B * sizeof(int)));
    HIPCHK(e, hipHostMalloc((void**)&t.h_overflow, B * sizeof(int)));
    HIPCHK(e, hipHostMalloc((void**)&t.h_out_fixed, B * PP_TRACK_MAX * sizeof(pp_track)));
    HIPCHK(e, hipHostMalloc((void**)&t.h_nout_fixed, B * sizeof(int)));
    HIPCHK(e, hipMemset(t.d_pose_q, 0, B * sizeof(TrkPose)));
    HIPCHK(e, hipMemset(t.d_pose_prev, 0, B * sizeof(TrkPose)));
    HIPCHK(e, hipMemset(t.state, 0, B * PP_TRACK_MAX * sizeof(TrkSlot)));
    HIPCHK(e, hipMemset(t.overflow, 0, B * sizeof(int)));
    HIPCHK(e, hipMemset(t.d_dt, 0, B * sizeof(double)));
    HIPCHK(e, hipMemset(t.d_cfg, 0, sizeof(pp_track_config)));
    std::vector<int> ones(B, 1);
    HIPCHK(e, hipMemcpy(t.next_id, ones.data(), B * sizeof(int), hipMemcpyHostToDevice));
    memset(t.h_nout, 0, B * sizeof(int));
    memset(t.h_overflow, 0, B * sizeof(int));
    for (size_t b = 0; b < B; ++b) t.h_nout_fixed[b] = -1;
    t.ready = true;
    return PP_OK;
}

int check_rows(pp_engine* e, const char* who, int rows) {
    if (rows > PP_TRACK_MASK_ROWS)
        return fail(e, PP_ERR_UNSUPPORTED, "%s: %d detection rows per frame; the tracking step's row bitmask holds %d (lower "
                    "nms_post_max_size, or use the joint class mode)", who, rows, PP_TRACK_MASK_ROWS);
    return PP_OK;
}

void fill_params(pp_engine* e, TrackParams& p, int batch, int rows, const pp_detection* dets, const int* n_dets) {
    pp_engine::Track& t = e->trk;
    p.batch = batch; p.rows = rows; p.dets = dets; p.n_dets = n_dets; p.cfg = t.d_cfg; p.dt = t.d_dt;
    p.state = t.state; p.next_id = t.next_id; p.overflow = t.overflow;
    p.pose_q = t.d_pose_q; p.pose_prev = t.d_pose_prev;
    p.out = t.h_out; p.n_out = t.h_nout; p.overflow_out = t.h_overflow;
    p.out_fixed = t.h_out_fixed; p.n_out_fixed = t.h_nout_fixed;
}

// the seconds of the next step, through `slot` of their own ring (taken by the caller before it queued anything) into
// d_dt, on the handle's stream
int queue_dt(pp_engine* e, const double* dt, int batch, int slot) {
    pp_engine::Track& t = e->trk;
    double* ring = t.h_dt.at(slot);
    if (dt) memcpy(ring, dt, (size_t)batch * sizeof(double));
    else memset(ring, 0, (size_t)batch * sizeof(double));
    HIPCHK(e, t.h_dt.send(slot, t.d_dt, (size_t)batch, e->stream));
    HIPCHK(e, t.dt_ring.sent(slot, e->stream));
    return PP_OK;
}

// the poses of the next step, armed, through a ring slot of their own into d_pose_q, on the handle's stream
int queue_pose(pp_engine* e, const double* poses, int batch) {
    pp_engine::Track& t = e->trk;
    int slot;
    HIPCHK(e, t.pose_ring.take(&slot));
    TrkPose* ring = t.h_pose.at(slot);
    for (int b = 0; b < batch; ++b) {
        const double* P = poses + (size_t)b * 12;
        memcpy(ring[b].m, P, 12 * sizeof(double));
        ring[b].psi = std::atan2(P[4], P[0]);          // the yaw of the sensor's x axis in the fixed frame: atan2(R10, R00)
        ring[b].has = 1;
        ring[b].pad = 0;
    }
    HIPCHK(e, t.h_pose.send(slot, t.d_pose_q, (size_t)batch, e->stream));
    HIPCHK(e, t.pose_ring.sent(slot, e->stream));
    return PP_OK;
}

int check_dt(pp_engine* e, const char* who, const double* dt, int batch) {
    for (int b = 0; b < batch; ++b)
        if (!std::isfinite(dt[b]) || !(dt[b] > 0.0))
            return fail(e, PP_ERR_ARG, "%s: dt of stream %d is %g (must be finite and > 0)", who, b, dt[b]);
    return PP_OK;
}

}  // namespace

// rule.track is only ever set behind a successful ensure_track (pp_set_tracking), so a tracked pass has its tables
int track_check_pass(pp_engine* e) {
    return e->rule.track ? check_rows(e, "pp_detect_async (tracking on)", det_rows(e)) : PP_OK;
}

// (pp_detect_async has asked track_check_pass before it queued or captured anything)
int run_track(pp_engine* e, int batch) {
    TrackParams p;
    fill_params(e, p, batch, det_rows(e), e->d_dets, e->d_ndets);
    ProfScope ps(e, nullptr);
    launch_track_step(p, e->stream);
    HIPCHK(e, hipGetLastError());
    return PP_OK;
}

void track_release(pp_engine* e) {
    pp_engine::Track& t = e->trk;
    for (void* p : {(void*)t.h_out, (void*)t.h_nout, (void*)t.h_overflow, (void*)t.h_out_fixed, (void*)t.h_nout_fixed})
        if (p) (void)hipHostFree(p);
    t.dt_ring.release();
    t.pose_ring.release();
    t = pp_engine::Track();
}

extern "C" {

int pp_set_tracking(pp_handle e, const pp_track_config* cfg) {
    if (!e) return PP_ERR_ARG;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_tracking: a training step is in flight");
    if (!cfg) { e->rule.track = 0; return PP_OK; }
    const struct { const char* name; double v; bool positive; } dbl[] = {
        {"gate", cfg->gate, true}, {"q_acc", cfg->q_acc, true}, {"r_pos", cfg->r_pos, true}, {"p0_pos", cfg->p0_pos, true},
        {"p0_vel", cfg->p0_vel, true}, {"size_alpha", cfg->size_alpha, false}, {"birth_score", cfg->birth_score, false},
        {"period", cfg->period, true}};
    for (const auto& f : dbl) {
        if (!std::isfinite(f.v)) return fail(e, PP_ERR_ARG, "pp_set_tracking: %s is not finite", f.name);
        if (f.positive && !(f.v > 0.0)) return fail(e, PP_ERR_ARG, "pp_set_tracking: %s = %g must be > 0", f.name, f.v);
    }
    if (cfg->size_alpha < 0.0 || cfg->size_alpha > 1.0)
        return fail(e, PP_ERR_ARG, "pp_set_tracking: size_alpha = %g outside [0, 1]", cfg->size_alpha);
    if (cfg->max_misses < 0) return fail(e, PP_ERR_ARG, "pp_set_tracking: max_misses = %d must be >= 0", cfg->max_misses);
    if (cfg->min_hits < 1) return fail(e, PP_ERR_ARG, "pp_set_tracking: min_hits = %d must be >= 1", cfg->min_hits);
    if (int st = check_rows(e, "pp_set_tracking", det_rows(e))) return st;
    (void)hipSetDevice(e->device);
    if (int st = ensure_track(e)) return st;
    pp_track_config c = *cfg;
    c.class_aware = c.class_aware ? 1 : 0;
    c.reserved = 0;
    if (!e->trk.configured || memcmp(&c, &e->trk.cfg, sizeof(c)) != 0) {
        HIPCHK(e, hipStreamSynchronize(e->stream));    // a step in flight reads the old values to its end
        HIPCHK(e, hipMemcpy(e->trk.d_cfg, &c, sizeof(c), hipMemcpyHostToDevice));
        e->trk.cfg = c;
        e->trk.configured = true;
    }
    e->rule.track = 1;
    return PP_OK;
}

int pp_get_tracking(pp_handle e, int32_t* on, pp_track_config* cfg_out) {
    if (!e || !on) return PP_ERR_ARG;
    *on = e->rule.track;
    if (cfg_out) *cfg_out = e->trk.cfg;
    return PP_OK;
}

int pp_set_track_dt(pp_handle e, const double* dt, int32_t batch) {
    if (!e) return fail(nullptr, PP_ERR_ARG, "pp_set_track_dt: NULL handle");
    if (!dt) return fail(e, PP_ERR_ARG, "pp_set_track_dt: dt is NULL");
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_track_dt: a training step is in flight");
    if (int st = check_batch(e, batch)) return st;
    if (!e->trk.configured) return fail(e, PP_ERR_STATE, "pp_set_track_dt: pp_set_tracking has given no configuration");
    if (int st = check_dt(e, "pp_set_track_dt", dt, batch)) return st;
    (void)hipSetDevice(e->device);
    int slot;
    HIPCHK(e, e->trk.dt_ring.take(&slot));
    return queue_dt(e, dt, batch, slot);
}

int pp_set_track_pose(pp_handle e, const double* poses, int32_t batch) {
    if (!e) return fail(nullptr, PP_ERR_ARG, "pp_set_track_pose: NULL handle");
    if (!poses) return fail(e, PP_ERR_ARG, "pp_set_track_pose: poses is NULL");
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_track_pose: a training step is in flight");
    if (int st = check_batch(e, batch)) return st;
    if (!e->trk.configured) return fail(e, PP_ERR_STATE, "pp_set_track_pose: pp_set_tracking has given no configuration");
    if (int st = check_poses(e, "pp_set_track_pose", poses, nullptr, batch, [](int, const double*) { return (int)PP_OK; })) return st;
    (void)hipSetDevice(e->device);
    return queue_pose(e, poses, batch);
}

// the rows and counts the last step left in page-locked memory (`out`, `n_out`), frame by frame, zeros behind the live rows
static int copy_tracks(pp_engine* e, const char* who, const pp_track* out, const int* n_out, pp_track* tracks, int32_t* n_tracks) {
    if (!tracks || !n_tracks) return fail(e, PP_ERR_ARG, "%s: NULL argument", who);
    const int B = e->trk.results;
    if (B < 1) return fail(e, PP_ERR_STATE, "%s: the last pass ran untracked, or none has run (pp_set_tracking, then a pass)", who);
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (e->trk.from_pass)
        if (int st = check_numeric(e, e->h_ndets, B, who)) return st;
    for (int b = 0; b < B; ++b) {
        const size_t n = (size_t)std::max(0, std::min(n_out[b], PP_TRACK_MAX));
        memcpy(tracks + (size_t)b * PP_TRACK_MAX, out + (size_t)b * PP_TRACK_MAX, n * sizeof(pp_track));
        memset(tracks + (size_t)b * PP_TRACK_MAX + n, 0, (PP_TRACK_MAX - n) * sizeof(pp_track));
    }
    memcpy(n_tracks, n_out, (size_t)B * sizeof(int));
    return PP_OK;
}

int pp_get_tracks_fixed(pp_handle e, pp_track* tracks, int32_t* n_tracks) {
    if (!e) return PP_ERR_ARG;
    return copy_tracks(e, "pp_get_tracks_fixed", e->trk.h_out_fixed, e->trk.h_nout_fixed, tracks, n_tracks);
}

int pp_get_tracks(pp_handle e, pp_track* tracks, int32_t* n_tracks, int32_t* overflow) {
    if (!e) return PP_ERR_ARG;
    if (int st = copy_tracks(e, "pp_get_tracks", e->trk.h_out, e->trk.h_nout, tracks, n_tracks)) return st;
    if (overflow) memcpy(overflow, e->trk.h_overflow, (size_t)e->trk.results * sizeof(int));
    return PP_OK;
}

int pp_track_update(pp_handle e, const pp_detection* dets, const int32_t* n_dets, int32_t rows, int32_t batch,
                    const double* dt) {
    if (!e) return PP_ERR_ARG;
    if (!dets || !n_dets) return fail(e, PP_ERR_ARG, "pp_track_update: NULL argument");
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_track_update: a training step is in flight");
    if (int st = check_batch(e, batch)) return st;
    if (rows < 1) return fail(e, PP_ERR_ARG, "pp_track_update: rows = %d must be >= 1", rows);
    if (int st = check_rows(e, "pp_track_update", rows)) return st;
    if (!e->trk.configured) return fail(e, PP_ERR_STATE, "pp_track_update: pp_set_tracking has given no configuration");
    for (int b = 0; b < batch; ++b)     // (a count a pass flagged may come back as it is: its stream stays untouched)
        if (n_dets[b] < 0 || (!(n_dets[b] & PP_NDETS_NONFINITE) && n_dets[b] > rows))
            return fail(e, PP_ERR_ARG, "pp_track_update: n_dets[%d] = %d outside [0, rows = %d]", b, n_dets[b], rows);
    if (dt)
        if (int st = check_dt(e, "pp_track_update", dt, batch)) return st;
    (void)hipSetDevice(e->device);
    pp_engine::Track& t = e->trk;
    int slot;
    HIPCHK(e, t.dt_ring.take(&slot));
    HIPCHK(e, hipMemcpyAsync(t.in_dets, dets, (size_t)batch * rows * sizeof(pp_detection), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(t.in_n, n_dets, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, e->stream));
    if (int st = queue_dt(e, dt, batch, slot)) return st;
    TrackParams p;
    fill_params(e, p, batch, rows, t.in_dets, t.in_n);
    prof_reset(e);
    {
        ProfScope ps(e, nullptr);
        launch_track_step(p, e->stream);
    }
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->stream));
    t.results = batch;
    t.from_pass = false;
    return PP_OK;
}

int pp_track_reset(pp_handle e, int32_t stream) {
    if (!e) return PP_ERR_ARG;
    if (stream < -1 || stream >= e->B)
        return fail(e, PP_ERR_ARG, "pp_track_reset: stream %d outside [0, max_batch=%d) (-1: all)", stream, e->B);
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_track_reset: a training step is in flight");
    if (!e->trk.ready) return PP_OK;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    pp_engine::Track& t = e->trk;
    const size_t b0 = stream < 0 ? 0 : (size_t)stream, nb = stream < 0 ? (size_t)e->B : 1;
    HIPCHK(e, hipMemset(t.state + b0 * PP_TRACK_MAX, 0, nb * PP_TRACK_MAX * sizeof(TrkSlot)));
    HIPCHK(e, hipMemset(t.overflow + b0, 0, nb * sizeof(int)));
    HIPCHK(e, hipMemset(t.d_pose_prev + b0, 0, nb * sizeof(TrkPose)));      // the previous pose goes; an armed one stays
    std::vector<int> ones(nb, 1);
    HIPCHK(e, hipMemcpy(t.next_id + b0, ones.data(), nb * sizeof(int), hipMemcpyHostToDevice));
    return PP_OK;
}

int pp_track_info(pp_handle e, int32_t* live, int32_t* next_id, int32_t* overflow) {
    if (!e) return PP_ERR_ARG;
    const size_t B = (size_t)e->B;
    if (!e->trk.ready) {
        for (size_t b = 0; b < B; ++b) {
            if (live) live[b] = 0;
            if (next_id) next_id[b] = 1;
            if (overflow) overflow[b] = 0;
        }
        return PP_OK;
    }
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (live) {
        std::vector<TrkSlot> s(B * PP_TRACK_MAX);
        HIPCHK(e, hipMemcpy(s.data(), e->trk.state, s.size() * sizeof(TrkSlot), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; ++b) {
            int c = 0;
            for (int k = 0; k < PP_TRACK_MAX; ++k) c += s[b * PP_TRACK_MAX + k].live != 0;
            live[b] = c;
        }
    }
    if (next_id) HIPCHK(e, hipMemcpy(next_id, e->trk.next_id, B * sizeof(int), hipMemcpyDeviceToHost));
    if (overflow) HIPCHK(e, hipMemcpy(overflow, e->trk.overflow, B * sizeof(int), hipMemcpyDeviceToHost));
    return PP_OK;
}

}  // extern "C"
